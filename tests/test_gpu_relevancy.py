"""GPU parity for the relevancy half: every HIP kernel (through the C ABI) against a plain fp32 torch/numpy
reference of the same op, then the assembled path against the oracle and the golden vectors captured from the
reference.  Tolerances are stated where they are used: the ViT GEMM operands are fp16 (fp32 accumulate, fp32
residual stream / LayerNorm / softmax) against the reference's all-fp32 CPU path."""
import numpy as np
import pytest
import torch

import semabs_amd  # noqa: F401
from oracle import preprocess as op
from oracle import relevancy as orl
from semabs_amd.synth import synth_rgb
from semabs_amd.weights import DEFAULT_PROMPT, make_clip_state_dict

pytestmark = pytest.mark.gpu


def _rand16(rng, *shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float16))


# ---- GEMM ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(1, 128, 64), (3, 512, 768), (127, 128, 128), (129, 256, 192), (1000, 768, 3072),
                                   (591, 2304, 768), (4100, 384, 512)])
def test_gemm_epilogues(M, N, K):
    from semabs_amd.clip.vit import gemm
    rng = np.random.default_rng(M * 7 + N)
    A, B = _rand16(rng, M, K), _rand16(rng, N, K, scale=0.05)
    bias = torch.from_numpy(rng.standard_normal(N).astype(np.float32))
    ref = A.double() @ B.double().T + bias.double()                       # asymmetric operands: catches transposes
    Ad, Bd, bd = A.cuda(), B.cuda(), bias.cuda()
    tol = dict(rtol=2e-3, atol=2e-3 * float(ref.abs().max()))
    c = torch.empty(M, N, dtype=torch.float32, device="cuda")
    gemm(Ad, Bd, c, bd, M, N, K, K, K, N, 3)
    np.testing.assert_allclose(c.cpu().double().numpy(), ref.numpy(), rtol=1e-4, atol=1e-4 * float(ref.abs().max()))
    c16 = torch.empty(M, N, dtype=torch.float16, device="cuda")
    gemm(Ad, Bd, c16, bd, M, N, K, K, K, N, 0)
    np.testing.assert_allclose(c16.cpu().double().numpy(), ref.numpy(), **tol)
    gemm(Ad, Bd, c16, bd, M, N, K, K, K, N, 1)
    np.testing.assert_allclose(c16.cpu().double().numpy(), (ref * torch.sigmoid(1.702 * ref)).numpy(), **tol)
    res = torch.from_numpy(rng.standard_normal((M, N)).astype(np.float32))
    c = res.cuda()
    gemm(Ad, Bd, c, bd, M, N, K, K, K, N, 2)
    np.testing.assert_allclose(c.cpu().double().numpy(), (ref + res.double()).numpy(), rtol=1e-4,
                               atol=1e-4 * float(ref.abs().max()))
    c = torch.empty(M, N, dtype=torch.float32, device="cuda")
    gemm(Ad, Bd, c, None, M, N, K, K, K, N, 3)                             # no bias
    np.testing.assert_allclose(c.cpu().double().numpy(), (ref - bias.double()).numpy(), rtol=1e-4,
                               atol=1e-4 * float(ref.abs().max()))


def test_gemm_rowmap_and_strides():
    from semabs_amd.clip.vit import gemm
    rng = np.random.default_rng(5)
    n, G, T, N, K = 3, 49, 50, 768, 3072
    A, B = _rand16(rng, n * G, K), _rand16(rng, N, K, scale=0.02)
    pos = torch.from_numpy(rng.standard_normal((T, N)).astype(np.float32))
    out = torch.full((n * T, N), -7.0, dtype=torch.float32, device="cuda")
    gemm(A.cuda(), B.cuda(), out, None, n * G, N, K, K, K, N, 4, addend=pos.cuda(), rowmap=(G, T, 1))
    ref = (A.double() @ B.double().T).view(n, G, N) + pos[1:].double()
    got = out.cpu().view(n, T, N)
    np.testing.assert_allclose(got[:, 1:].double().numpy(), ref.numpy(), rtol=1e-4, atol=1e-4)
    assert (got[:, 0] == -7.0).all()                                       # CLS rows untouched
    # strided A rows (CLS rows of a [n, T, K] activation) and a row-sliced B
    n, T, K, N = 5, 7, 768, 768
    act = _rand16(rng, n * T, K)
    W = _rand16(rng, 3 * N, K, scale=0.03)
    c = torch.empty(n, N, dtype=torch.float32, device="cuda")
    gemm(act.cuda(), W.cuda()[N:2 * N], c, None, n, N, K, T * K, K, N, 3)
    ref = act.view(n, T, K)[:, 0].double() @ W[N:2 * N].double().T
    np.testing.assert_allclose(c.cpu().double().numpy(), ref.numpy(), rtol=1e-4, atol=1e-4)


def test_gemm_rejects_bad_shapes():
    from semabs_amd.clip.vit import gemm
    a = torch.zeros(4, 64, dtype=torch.float16, device="cuda")
    with pytest.raises(RuntimeError):
        gemm(a, a, torch.zeros(4, 100, device="cuda"), None, 4, 100, 64, 64, 64, 100, 3)      # N not multiple of 128


# ---- LayerNorm / attention -------------------------------------------------------------------------
@pytest.mark.parametrize("M,D", [(1, 768), (5, 512), (1000, 768), (7, 1024), (3, 256)])
def test_layernorm(M, D):
    from semabs_amd.clip.vit import layernorm
    rng = np.random.default_rng(D + M)
    x = torch.from_numpy((rng.standard_normal((M, D)) * 3 + 1).astype(np.float32))
    w = torch.from_numpy(rng.standard_normal(D).astype(np.float32))
    b = torch.from_numpy(rng.standard_normal(D).astype(np.float32))
    ref = torch.nn.functional.layer_norm(x, (D,), w, b, 1e-5)
    o32 = torch.empty(M, D, dtype=torch.float32, device="cuda")
    layernorm(x.cuda(), w.cuda(), b.cuda(), o32, M, D, out_f32=True)
    np.testing.assert_allclose(o32.cpu().numpy(), ref.numpy(), rtol=1e-5, atol=1e-5)
    o16 = torch.empty(M, D, dtype=torch.float16, device="cuda")
    layernorm(x.cuda(), w.cuda(), b.cuda(), o16, M, D)
    np.testing.assert_allclose(o16.cpu().float().numpy(), ref.numpy(), rtol=2e-3, atol=2e-3)


@pytest.mark.parametrize("T,H,causal", [(50, 12, 0), (197, 12, 0), (77, 8, 1), (33, 2, 0), (128, 3, 1), (20, 1, 0), (161, 2, 0)])
def test_attention(T, H, causal):
    from semabs_amd import _lib
    rng = np.random.default_rng(T)
    n, D = 3, H * 64
    qkv = _rand16(rng, n, T, 3 * D)
    qkv[..., :D] *= 0.4                                                    # moderately peaked softmax
    out = torch.zeros(n, T, D, dtype=torch.float16, device="cuda")
    qkv_d = qkv.cuda()
    _lib.call("semabs_attention", _lib.ptr(qkv_d), _lib.ptr(out), None, n, T, H, 64, 3 * D, causal, _lib.stream())
    q, k, v = (t.double().view(n, T, H, 64).transpose(1, 2) for t in qkv.chunk(3, dim=-1))
    s = q @ k.transpose(-1, -2)
    if causal:
        s = s + torch.full((T, T), float("-inf"), dtype=torch.float64).triu_(1)
    ref = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(n, T, D)
    np.testing.assert_allclose(out.cpu().double().numpy(), ref.numpy(), rtol=3e-3, atol=3e-3)
    # k_attention2 (row-major V read through ds_read_b64_tr_b16; bit 1 = register staging, bit 2 = LDS-DMA staging) stays selectable for A/B: same
    # scores, same P, the P.V products are summed in the same order -> identical outputs
    for bit in (2, 4):
        out2 = torch.zeros_like(out)
        _lib.call("semabs_attention", _lib.ptr(qkv_d), _lib.ptr(out2), None, n, T, H, 64, 3 * D, causal | bit, _lib.stream())
        assert torch.equal(out, out2), bit


# ---- tiling front / back -----------------------------------------------------------------------------
def _init_clip(arch, chunk=64):
    from semabs_amd.clip import ClipWrapper
    sd = make_clip_state_dict(arch, 0)
    ClipWrapper.engine = None
    ClipWrapper(arch, state_dict=sd, chunk_tiles=chunk, max_labels=4)
    return ClipWrapper, sd


@pytest.mark.parametrize("p,H,cfg", [
    (32, 240, [(240, 60), (224, 8), (160, 40), (60, 90), (17, 111)]),            # 7 / identity / 5 / 5 / 5 taps
    (16, 240, [(240, 60), (224, 8), (160, 40), (60, 90), (17, 111)]),
    (14, 240, [(240, 60), (224, 8), (97, 70)]),                                  # ViT-L/14's patch: pixel pairs never straddle a patch
    (16, 600, [(600, 1), (480, 60), (400, 100), (300, 150), (337, 131)]),        # 13 (generic tap loop) / 11 / 9 / 7 / 9 taps
])
def test_tile_patches_bit_exact(p, H, cfg):
    """crop -> Pillow-exact bicubic -> normalise -> im2col: equal to the oracle's fp32 tile rounded once to fp16; flip = 2 writes both passes."""
    from semabs_amd import _lib
    from semabs_amd.clip import ClipWrapper, plan_tiles
    CW, _ = _init_clip("ViT-B/32" if p == 32 else "ViT-B/16")
    W = H
    imgs = np.stack([synth_rgb(H, W, seed=3), synth_rgb(H, W, seed=4)])
    table, _ = plan_tiles(H, W, 2, [{"tile_size": a, "stride": b} for a, b in cfg])
    sel = np.unique(np.concatenate([np.arange(0, len(table), 5), np.arange(len(table) - 3, len(table))]))
    table = table[sel]
    co = CW._coeffs
    ids = np.asarray([co.id_of(int(t)) for t in table[:, 3]], np.int32)
    xmin_d, kk_d, ks_d = co.device()
    tiles_dev = torch.from_numpy(np.concatenate([table, ids[:, None]], 1).astype(np.int32)).cuda()
    g = 224 // p
    imgs_d = torch.from_numpy(imgs).cuda()
    n = len(table)
    ref = np.stack([op.preprocess_tile(imgs[im][x:x + ts, y:y + ts]) for im, x, y, ts in table]).astype(np.float16)
    outs = {}
    for flip in (0, 1, 2):
        patches = torch.zeros((2 if flip == 2 else 1) * n * g * g, 3 * p * p, dtype=torch.float16, device="cuda")
        _lib.call("semabs_tile_patches", _lib.ptr(imgs_d), 2, H, W, _lib.ptr(tiles_dev), n,
                  _lib.ptr(xmin_d), _lib.ptr(kk_d), _lib.ptr(ks_d), _lib.ptr(CW._lut), _lib.ptr(patches), p, flip,
                  max(co.ksize), _lib.stream())
        outs[flip] = patches.cpu().view(-1, g, g, 3, p, p).permute(0, 3, 1, 4, 2, 5).reshape(-1, 3, 224, 224).numpy()
    assert np.array_equal(outs[0], ref)
    assert np.array_equal(outs[1], ref[..., ::-1])
    assert np.array_equal(outs[2][:n], ref) and np.array_equal(outs[2][n:], ref[..., ::-1])


def _jitter_dev(img_u8, order, factors):
    from semabs_amd import _lib
    H, W = img_u8.shape[:2]
    d = torch.from_numpy(np.ascontiguousarray(img_u8)).cuda()
    scratch = torch.zeros(1, dtype=torch.int64, device="cuda")
    _lib.call("semabs_color_jitter", d.data_ptr(), H, W, _lib.iarr([int(o) for o in order]), _lib.farr([float(f) for f in factors]), _lib.ptr(scratch), _lib.stream())
    return d.cpu().numpy()


def test_color_jitter_all_orders_byte_exact(golden):
    """semabs_color_jitter against torchvision's PIL path executed with Pillow (g28): all 24 op orders at 480 x 480 with fixed factors (incl. the
    range ends and the identity) - byte equality - and against the oracle on a second image (CLIP/clip/__init__.py:55-57, 246-247)."""
    from conftest import sha
    g = golden("g28_color_jitter")
    img = synth_rgb(int(g["meta"][0]), int(g["meta"][1]), seed=int(g["meta"][2]))
    for o, f, want, sub in zip(g["orders"], g["factors"], g["sha"], g["sub"]):
        out = _jitter_dev(img, o, f)
        assert np.array_equal(out[::5, ::5], sub), (o, f, int((out[::5, ::5] != sub).sum()))
        assert np.array_equal(sha(out), want), (o, f)
    img2 = synth_rgb(200, 312, seed=9)
    rng = np.random.default_rng(5)
    for _ in range(6):
        o = rng.permutation(4)
        f = np.asarray([rng.uniform(0.4, 1.6), rng.uniform(0.4, 1.6), rng.uniform(0.4, 1.6), rng.uniform(-0.1, 0.1)], np.float32)
        assert np.array_equal(_jitter_dev(img2, o, f), op.color_jitter(img2, o, f.astype(np.float64))), (o, f)


def test_color_jitter_every_op_on_the_full_colour_cube(golden):
    """Each adjustment alone (semabs_color_jitter_op) on the 4096 x 4096 image of all 2^24 colours - both blend regimes (factor below / above 1),
    the hue rotation at 0 / + / - : sha256 of Pillow's bytes (g28)."""
    from conftest import sha
    from semabs_amd import _lib
    g = golden("g28_color_jitter")
    c = np.arange(1 << 24, dtype=np.uint32)
    allc = torch.from_numpy(np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)).cuda()
    scratch = torch.zeros(1, dtype=torch.int64, device="cuda")
    for (opid, f), want in zip(g["cube_ops"], g["cube_sha"]):
        d = allc.clone()
        _lib.call("semabs_color_jitter_op", d.data_ptr(), 4096, 4096, int(opid), float(np.float32(f)), _lib.ptr(scratch), _lib.stream())
        assert np.array_equal(sha(d.cpu().numpy()), want), (opid, f)


@pytest.mark.parametrize("tag,cfgname", [("ours120", "ours"), ("chefer96", "chefer_et_al"), ("ours56_g14", "ours"), ("ours64x48", "ours")])
def test_aggregate_vs_golden(golden, tag, cfgname):
    from semabs_amd.clip import ClipWrapper, plan_tiles, saliency_configs
    CW, _ = _init_clip("ViT-B/32")
    g = golden("g5_aggregate")
    H, gg, L, aug, flip, W = (int(v) for v in g[f"{tag}_meta"])
    cfg = saliency_configs[cfgname](H)
    table, scales = plan_tiles(H, W, aug + 1, cfg["cropping_augmentations"])
    assert np.array_equal(table, orl.tile_table(H, W, aug + 1, cfg["cropping_augmentations"]))
    rel = [torch.from_numpy(g[f"{tag}_rel"]).cuda()]
    if flip:
        rel.append(torch.from_numpy(g[f"{tag}_rel_flip"]).cuda())
    out_d = CW.aggregate_device(rel, scales, aug + 1, H, W)
    if flip:
        # aggregate_device averages the two passes once per map cell (semabs_unflip_average) and aggregates the result; the one-call form averages per
        # covered pixel: the same operation on the same operands - bit-identical
        from semabs_amd import _lib
        one = torch.empty_like(out_d)
        sc = torch.from_numpy(np.ascontiguousarray(scales, np.int32)).cuda()
        N = int(rel[0].shape[1])
        _lib.call("semabs_aggregate", _lib.ptr(rel[0]), _lib.ptr(rel[1]), L, N, gg, H, W, _lib.ptr(sc), len(scales), aug + 1, N // (aug + 1), _lib.ptr(one), _lib.stream())
        assert torch.equal(one, out_d)
    out = out_d.cpu().numpy()
    ref = g[f"{tag}_maps"]
    err = np.abs(out - ref)
    # same adds in the same order; an fp32 last-bit difference in the bilinear sample can flip one fp16 rounding of a
    # canvas (2^-11 of that element), nothing more
    # canvas (<= 2^-10 of that canvas value, which after cancellation between scales can exceed 2^-10 of the result)
    assert err.max() <= 2e-3 * np.abs(ref).max(), err.max()
    assert (err > 1e-6 * np.abs(ref).max()).mean() < 1e-2, (err > 1e-6 * np.abs(ref).max()).mean()


# ---- ViT + rollout ------------------------------------------------------------------------------------
def _tiles(n, seed):
    sizes = [120, 80, 60, 30, 97]
    return torch.from_numpy(np.stack([op.preprocess_tile(synth_rgb(sizes[i % 5], sizes[i % 5], seed=seed + i)) for i in range(n)]))


@pytest.mark.parametrize("arch,tag", [("ViT-B/32", "b32"), ("ViT-B/16", "b16")])
def test_vit_gradcam(golden, arch, tag):
    """HIP ViT + analytic rollout vs the reference's autograd result (golden) and vs the oracle.
    Tolerance: RELATIVE L-infinity (max|ours - ref| / max|ref|) <= conftest.tol(measured) = 1.3 x the value measured on MI355X for THAT case (fp16 GEMM
    operands over the 11 trunk blocks vs the fp32 CPU reference; round 6: the last block and the VJP chain run on [hi | lo] operand pairs): B/32 9.9e-4 /
    1.01e-3, B/16 7.55e-4 / 1.08e-3 for positive_attn_only True / False (round 5: 1.65e-3 / 1.68e-3, 7.5e-4 / 1.83e-3)."""
    from conftest import tol
    measured = {("b32", True): 9.90e-4, ("b32", False): 1.01e-3, ("b16", True): 7.55e-4, ("b16", False): 1.08e-3}
    CW, sd = _init_clip(arch)
    g = golden(f"g3g4_vit_{tag}")
    tiles = _tiles(3, 7)
    w_text = torch.from_numpy(g["w_text"]).T.contiguous().cuda()            # [L, E]
    for pos in (True, False):
        rel, logits, feat = CW.engine.gradcam_tiles(tiles.cuda(), w_text, pos)
        ref = g[f"rel_pos{int(pos)}"]
        err = np.abs(rel.cpu().numpy() - ref).max()
        print(f"{arch} pos={pos}: rel Linf {err:.3e} / max|ref| {np.abs(ref).max():.3e} = {err / np.abs(ref).max():.2e} relative")
        assert err <= tol(measured[(tag, pos)]) * np.abs(ref).max(), (err, np.abs(ref).max())
    np.testing.assert_allclose(feat.cpu().numpy(), g["feat"], rtol=0, atol=5e-3 * np.abs(g["feat"]).max())
    np.testing.assert_allclose(logits.cpu().numpy(), g["logits"], rtol=0, atol=5e-3 * np.abs(g["logits"]).max() + 0.05)
    probs = CW.engine._workspace()["probs"][:3].cpu().numpy()
    np.testing.assert_allclose(probs, g["probs_cls"], rtol=2e-2, atol=1e-5)
    # flipped input = flipped tiles
    rel_f, _, _ = CW.engine.gradcam_tiles(tiles.cuda(), w_text, True, flip=True)
    with torch.no_grad():
        ref_f, _ = orl.gradcam_tiles(make_clip_state_dict(arch, 0, text_tower=False), torch.flip(tiles, dims=[-1]),
                                     torch.from_numpy(g["w_text"]), True)
    e_f = np.abs(rel_f.cpu().numpy() - ref_f.numpy()).max() / ref_f.abs().max().item()
    print(f"{arch} flipped tiles vs the oracle: {e_f:.2e} relative")
    # measured, against the ORACLE's fp32 run of the flipped tiles.  (B/16 was 6.98e-4 in round 5 WITH the last block's and the VJP chain's fp16 roundings: on
    # these three tiles they happened to cancel part of the trunk's error - the CPU model reproduces it: trunk roundings alone 1.24e-3, all roundings 4.3e-4.)
    assert e_f <= tol({"b32": 4.85e-4, "b16": 1.13e-3}[tag])


def test_text_tower(golden):
    CW, sd = _init_clip("ViT-B/32")
    g = golden("g7_text")
    for tag, nt in (("t1", 1), ("t3", 3)):
        w = CW.text.zeroshot_weights(torch.from_numpy(g[f"{tag}_tokens"]), 4, nt).cpu().numpy()
        ref = g[f"{tag}_weights"].T
        assert np.abs(w - ref).max() <= 5e-3 * np.abs(ref).max(), np.abs(w - ref).max()


def test_tokenizer_matches_reference_ids(golden, bpe_vocab):
    from semabs_amd.clip.tokenizer import BPETokenizer
    g = golden("g7_text")
    tk = BPETokenizer(bpe_vocab)
    labels = ["chair", "table", "pink make up bag", "brown modern upholstered chair in faux leather with wooden legs"]
    assert np.array_equal(tk.tokenize([DEFAULT_PROMPT.format(c) for c in labels]).numpy(), g["t1_tokens"])
    assert np.array_equal(tk.tokenize(["Hello, World! it's 42 degrees", "a  b\tc", "don't you're we've"]).numpy(), g["misc_tokens"])


@pytest.mark.parametrize("arch,tag,name,H", [("ViT-B/32", "b32", "chefer96", 96), ("ViT-B/32", "b32", "ours96", 96),
                                             ("ViT-B/16", "b16", "two_scale64", 64)])
def test_end_to_end_maps(golden, arch, tag, name, H, bar):
    """uint8 image -> fp32 maps, whole HIP path, vs the reference's get_clip_saliency output (golden).
    Tolerance: RELATIVE L-infinity <= 3.5e-3 = 3 x the largest measured value (1.15e-3 / 9.3e-4 / 1.03e-3 on MI355X); the headline shape has its
    own test (test_gpu_headline.py)."""
    from semabs_amd.clip import saliency_configs
    CW, sd = _init_clip(arch)
    g = golden(f"g6_e2e_{tag}")
    if name == "ours96":
        cfg = dict(saliency_configs["ours"](96), augmentations=0)
    elif name == "chefer96":
        cfg = saliency_configs["chefer_et_al"](96)
    else:
        cfg = dict(saliency_configs["chefer_et_al"](64), horizontal_flipping=True,
                   cropping_augmentations=[{"tile_size": 64, "stride": 16}, {"tile_size": 32, "stride": 8}])
    w_text = torch.from_numpy(g[f"{name}_text"]).contiguous().cuda()          # [L, E]
    img = torch.from_numpy(synth_rgb(H, H, seed=42)).cuda()[None].contiguous()
    maps = CW.relevancy_device(img, w_text, cfg["cropping_augmentations"], cfg["horizontal_flipping"], cfg["positive_attn_only"])
    ref = g[f"{name}_maps"]
    err = np.abs(maps.cpu().numpy() - ref).max()
    print(f"{arch}/{name}: map Linf {err:.3e} / max|ref| {np.abs(ref).max():.3e} = {err / np.abs(ref).max():.2e}")
    assert bar("maps_abs", err, min(3.5e-3 * np.abs(ref).max(), 1e-4))          # per case: 1.3 x its measured error (tests/golden/measured_errors.json); BASELINE's bar is 1e-3 absolute


class _FixtureTokenizer:
    """String -> token ids from tests/golden/tokens_default.npz (the BPE merge table is not on the GPU box)."""

    def __init__(self, golden):
        g = golden("tokens_default")
        prompt = str(g["prompt"])
        self.map = {prompt.format(l): t for l, t in zip(g["labels"], g["tokens"])}

    def tokenize(self, texts, context_length=77, truncate=False):
        if isinstance(texts, str):
            texts = [texts]
        return torch.from_numpy(np.stack([self.map[t] for t in texts]))


def test_public_get_clip_saliency_with_text_tower(golden):
    """The reference's public call, strings in / CPU tensors out: tokenizer (fixture ids) -> HIP text tower -> HIP
    relevancy, against the reference's (maps, text features) for the same call."""
    from semabs_amd.clip import saliency_configs
    CW, sd = _init_clip("ViT-B/32")
    CW.tokenizer = _FixtureTokenizer(golden)
    g = golden("g6_e2e_b32")
    labels = ["chair", "table", "lamp"]
    img = synth_rgb(96, 96, seed=42)
    maps, feats = CW.get_clip_saliency(img=img, text_labels=np.array(labels), prompts=[DEFAULT_PROMPT], **saliency_configs["chefer_et_al"](96))
    assert maps.device.type == "cpu" and feats.device.type == "cpu" and maps.dtype == torch.float32
    assert tuple(maps.shape) == (3, 96, 96) and tuple(feats.shape) == (3, 512)
    ref_t = g["chefer96_text"]
    assert np.abs(feats.numpy() - ref_t).max() <= 5e-3 * np.abs(ref_t).max()
    ref = g["chefer96_maps"]
    err = np.abs(maps.numpy() - ref).max()
    print(f"public API chefer96: map Linf {err:.3e} / max|ref| {np.abs(ref).max():.3e}")
    from conftest import tol
    assert err <= tol(4.578e-5)                                         # measured 4.578e-5 absolute = 1.73e-3 of max|ref| (text tower included)
    # distractor labels subtract the mean distractor map (CLIP/clip/__init__.py:125-131)
    m2, _ = CW.get_clip_saliency(img=img, text_labels=labels[:2], prompts=[DEFAULT_PROMPT],
                                 **dict(saliency_configs["chefer_et_al"](96), distractor_labels={"lamp", "chair"}))
    np.testing.assert_allclose(m2.numpy(), (maps[:2] - maps[2:3]).numpy(), atol=2e-6)
    with pytest.raises(AssertionError):
        CW.get_clip_saliency(img=img.astype(np.float32), text_labels=labels, prompts=[DEFAULT_PROMPT], **saliency_configs["chefer_et_al"](96))
    CW.tokenizer = None


def test_add_layernorm():
    """x += delta (fp16) in place, then LayerNorm -> fp16; out = NULL adds only."""
    from semabs_amd.clip.vit import add_layernorm
    rng = np.random.default_rng(5)
    M, D = 333, 768
    x = torch.from_numpy(rng.standard_normal((M, D)).astype(np.float32) * 3 + 0.5)
    d = torch.from_numpy(rng.standard_normal((M, D)).astype(np.float32)).half()
    w = torch.from_numpy((1 + 0.1 * rng.standard_normal(D)).astype(np.float32))
    b = torch.from_numpy((0.1 * rng.standard_normal(D)).astype(np.float32))
    xs = x + d.float()
    ref = torch.nn.functional.layer_norm(xs, (D,), w, b, 1e-5)
    xd, out = x.cuda(), torch.empty(M, D, dtype=torch.float16, device="cuda")
    add_layernorm(xd, d.cuda(), w.cuda(), b.cuda(), out, M, D)
    assert torch.equal(xd.cpu(), xs)
    np.testing.assert_allclose(out.cpu().float().numpy(), ref.numpy(), rtol=2e-3, atol=2e-3)
    add_layernorm(xd, d.cuda(), None, None, None, M, D)
    assert torch.equal(xd.cpu(), xs + d.float())


@pytest.mark.parametrize("T,H,causal", [(197, 2, 0), (128, 2, 1), (77, 1, 1)])
def test_attention_rising_scores(T, H, causal):
    """The single-pass softmax keeps a lazy reference maximum and rescales only when a key block exceeds it by more than 8: here the scores
    grow steeply along the keys (and span > 60 per row), so every later block raises the reference and the rescaling path runs."""
    from semabs_amd import _lib
    rng = np.random.default_rng(T + 7)
    n, D = 2, H * 64
    qkv = _rand16(rng, n, T, 3 * D).float()
    ramp = torch.linspace(0.0, 1.0, T)[None, :, None]
    qkv[..., :D] = 0.25 * qkv[..., :D] + 1.0                               # queries: a common positive component ...
    qkv[..., D:2 * D] = 0.25 * qkv[..., D:2 * D] + ramp                    # ... that the keys pick up more and more strongly -> scores rise to ~64
    qkv = qkv.half()
    out = torch.zeros(n, T, D, dtype=torch.float16, device="cuda")
    qkv_d = qkv.cuda()
    _lib.call("semabs_attention", _lib.ptr(qkv_d), _lib.ptr(out), None, n, T, H, 64, 3 * D, causal, _lib.stream())
    q, k, v = (t.double().view(n, T, H, 64).transpose(1, 2) for t in qkv.chunk(3, dim=-1))
    s = q @ k.transpose(-1, -2)
    assert float(s.max() - s.min()) > 40.0
    if causal:
        s = s + torch.full((T, T), float("-inf"), dtype=torch.float64).triu_(1)
    ref = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(n, T, D)
    np.testing.assert_allclose(out.cpu().double().numpy(), ref.numpy(), rtol=3e-3, atol=3e-3)


def test_imagenet_prompt_ensemble_vs_reference(golden):
    """`imagenet_prompt_ensemble=True` the way generate_relevancy.py:70-80 runs it - `prompts=imagenet_templates`, 80 templates per label -
    through the public call: tokenizer (the reference's ids for the 160 strings, g24) -> HIP text tower -> per-template L2 normalise -> mean
    over templates (clip_gradcam.py:12-27) -> relevancy, against the unmodified reference's (maps, text features)."""
    from semabs_amd.clip import imagenet_templates, saliency_configs
    CW, sd = _init_clip("ViT-B/32")
    g = golden("g24_prompt_ensemble")
    labels = [str(l) for l in g["labels"]]
    texts = [t.format(c) for c in labels for t in imagenet_templates]

    class Tok:
        map = {t: ids for t, ids in zip(texts, g["tokens"].astype(np.int64))}

        def tokenize(self, tx, context_length=77, truncate=False):
            return torch.from_numpy(np.stack([self.map[t] for t in ([tx] if isinstance(tx, str) else tx)]))

    CW.tokenizer = Tok()
    try:
        cfg = dict(saliency_configs["chefer_et_al"](96), imagenet_prompt_ensemble=True)
        maps, feats = CW.get_clip_saliency(img=synth_rgb(96, 96, seed=42), text_labels=np.array(labels), prompts=imagenet_templates, **cfg)
    finally:
        CW.tokenizer = None
    assert tuple(maps.shape) == (2, 96, 96) and tuple(feats.shape) == (2, 512)
    e_t = float(np.abs(feats.numpy() - g["text"]).max() / np.abs(g["text"]).max())
    err = float(np.abs(maps.numpy() - g["maps"]).max())
    print(f"prompt ensemble (2 labels x 80 templates): text feature rel L-inf {e_t:.2e}, map L-inf {err:.3e} / max|ref| {np.abs(g['maps']).max():.3e}")
    from conftest import tol
    assert e_t <= tol(5.05e-4)                                          # measured 5.05e-4
    assert err <= tol(3.052e-5)                                         # measured 3.052e-5 absolute = 1.6e-3 of max|ref| - ONE tile: an L-infinity over 196 cells (round 5: 2.289e-5)
    # the mean over templates is NOT re-normalised (clip_gradcam.py:23-26): the ensemble weight is shorter than a unit vector
    assert float(np.linalg.norm(feats.numpy(), axis=1).max()) < 0.999


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("T", [50, 197])
def test_cls_scores_kernel_vs_fp64(T, split):
    """semabs_cls_scores: the CLS query's softmax row of the last block from (W_k^T q) . x instead of q . (W_k x): against the fp64 softmax of the direct form on the
    same operands (q fp32, W_k fp16-exact, x as fp16 rows or [hi | lo] pairs), peaked scores (sigma ~8), and semabs_attention_cls(k = NULL) against P . V."""
    from semabs_amd import _lib
    n, D, H = 7, 768, 12
    g = torch.Generator(device="cuda").manual_seed(T + split)
    x32 = torch.randn(n * T, D, device="cuda", generator=g) * 1.5 + 0.3
    wk = (torch.randn(D, D, device="cuda", generator=g) * 0.05).half()
    bk = torch.randn(D, device="cuda", generator=g) * 0.2
    q = torch.randn(n, D, device="cuda", generator=g) * 0.9
    hi = x32.half()
    if split:
        x = torch.cat([hi, (x32 - hi.float()).half()], dim=1).contiguous()
        xd = hi.double() + x[:, D:].double()
    else:
        x = hi.contiguous()
        xd = hi.double()
    probs = torch.full((n + 1, H, T), 7.0, dtype=torch.float32, device="cuda")
    _lib.call("semabs_cls_scores", _lib.ptr(q), _lib.ptr(wk), _lib.ptr(bk), _lib.ptr(x), x.shape[1], split, _lib.ptr(probs), n, T, D, _lib.stream())
    k = (xd @ wk.double().T + bk.double()).view(n, T, H, 64)
    s = torch.einsum("nhd,nthd->nht", q.double().view(n, H, 64), k)
    ref = torch.softmax(s, dim=-1)
    err = float((probs[:n].double() - ref).abs().max())
    print(f"semabs_cls_scores T={T} split={split}: probs L-inf {err:.2e} (score sigma {float(s.std(-1).mean()):.1f}, max prob {float(ref.max()):.3f})")
    assert err < 2e-5 and bool((probs[n] == 7.0).all())
    v = (torch.randn(n * T, D, device="cuda", generator=g)).half()
    o = torch.full((n + 1, 2 * D if split else D), 7.0, dtype=torch.float16, device="cuda")
    _lib.call("semabs_attention_cls", None, None, _lib.ptr(v), _lib.ptr(probs), _lib.ptr(o), n, T, H, 64, split, _lib.stream())
    want = torch.einsum("nht,nthd->nhd", probs[:n].double(), v.double().view(n, T, H, 64)).reshape(n, D)
    got = o[:n, :D].double() + (o[:n, D:].double() if split else 0.0)
    assert float((got - want).abs().max()) < (2e-6 if split else 2e-3) * float(want.abs().max()) and bool((o[n] == 7.0).all())
