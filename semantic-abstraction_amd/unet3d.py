"""Drop-in for the reference's `unet3d.ResidualUNet3D` (unet3d.py:658-689 -> Abstract3DUNet :481-621), inference only,
computed by the HIP implicit-GEMM kernels in csrc/unet.hip.

Same constructor arguments, same `state_dict` key names (`encoders.{i}.basic_module.conv{1,2,3}.{groupnorm,conv}.*`,
`decoders.{i}.upsampling.upsample.*`, `final_conv.*`), `forward(x[N, C, D, H, W]) -> [N, out, D, H, W]`.
Internally activations are channels-last [N, D, H, W, C]; `forward_cl` takes / returns that layout directly
(what `SemAbs3D` uses, so nothing is transposed on the hot path).

precision = "fp16": fp16 activations in HBM, one fp16 MFMA per k-step, fp32 accumulate, fp64 GroupNorm statistics.
precision = "exact": fp32 activations, operands split into fp16 hi + lo (3 MFMAs) - ~fp32 accuracy, used to show
that the residual L-inf of the fp16 mode is rounding, not a defect.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List

import numpy as np
import torch

from . import _lib


def number_of_features_per_level(init_channel_number, num_levels):
    return [init_channel_number * 2 ** k for k in range(num_levels)]


# ---- weight layouts ------------------------------------------------------------------------------------
# Pure data movement (permute / flip / reshape / cat / zero padding) of a weight-shaped tensor: `_Conv` / `_ConvT` apply them to the weights,
# train._WeightLayouts applies the SAME functions to an index tensor (1 .. numel, zeros = padding) to get its gather map.

def _pack_fragments(w: torch.Tensor) -> torch.Tensor:
    """[Cout, Kp] (Kp % 32 == 0, Cout % 16 == 0) -> [Kp / 32][Cout / 16][lane = kg * 16 + row][8] flattened, k = 32 * k-step + 8 * kg + e:
    the order in which a wave's 64 lanes hold the A operand of v_mfma_f32_16x16x32_f16 (csrc/unet.hip, SEMABS_CONV_PACKED)."""
    cout, kp = int(w.shape[0]), int(w.shape[1])
    assert cout % 16 == 0 and kp % 32 == 0
    # w[cb * 16 + vl, ks * 32 + kg * 8 + e] -> [ks, cb, kg, vl, e]
    return w.reshape(cout // 16, 16, kp // 32, 4, 8).permute(2, 0, 3, 1, 4).contiguous().reshape(-1)


def matrix_layout(m: torch.Tensor):
    """[rows, K] -> (flat, flag word): the matrix with K zero-padded to a multiple of 32, followed - when rows % 16 == 0 - by its fragment-packed copy
    (flag bit 9 of the convolution entry points' flag word, SEMABS_CONV_PACKED: one MFMA A operand = 1 KB of contiguous memory, see _pack_fragments)."""
    rows, k = int(m.shape[0]), int(m.shape[1])
    kp = (k + 31) // 32 * 32
    if kp != k:
        m = torch.cat([m, m.new_zeros(rows, kp - k)], dim=1)
    m = m.contiguous()
    if rows % 16 == 0:
        return torch.cat([m.reshape(-1), _pack_fragments(m)]), 512
    return m.reshape(-1), 0


def conv_fwd_layout(w: torch.Tensor):
    """Conv3d weight [Cout, Cin, k, k, k] -> [Cout, (kd, kh, kw, cin)].  Also the 1 x 1 x 1 `final_conv`, and the DATA-gradient matrix of a
    ConvTranspose3d weight [Cin, Cout, 3, 3, 3] -> [Cin, (k, cout)] (its gradient is a plain strided convolution with the same taps)."""
    return matrix_layout(w.permute(0, 2, 3, 4, 1).reshape(w.shape[0], -1))


def conv_bwd_layout(w: torch.Tensor):
    """Data-gradient matrix of a Conv3d weight [Cout, Cin, k, k, k]: taps flipped, channels swapped -> [Cin, (kd, kh, kw, cout)]."""
    return matrix_layout(w.flip(2, 3, 4).permute(1, 2, 3, 4, 0).reshape(w.shape[1], -1))


def linear_layout(w: torch.Tensor, transposed: bool = False):
    """Linear weight [Cout, Cin] as a 1 x 1 x 1 convolution matrix; transposed = the matrix of its data gradient."""
    return matrix_layout(w.t() if transposed else w)


def convT_class_layout(w: torch.Tensor):
    """ConvTranspose3d(k3, s2, p1) weight [Cin, Cout, 3, 3, 3] -> (flat, flag word, offsets): the eight output-parity-class matrices
    [Cout, ntaps * Cin] (offsets = where each starts), followed by their fragment-packed copies when EVERY class matrix can be packed."""
    cin, cout = int(w.shape[0]), int(w.shape[1])
    mats, offs, off = [], [], 0
    for cls in range(8):
        p = (cls >> 2, (cls >> 1) & 1, cls & 1)
        cols = []
        for t0 in range(p[0] + 1):
            for t1 in range(p[1] + 1):
                for t2 in range(p[2] + 1):
                    k = [1 if pp == 0 else (0 if t == 0 else 2) for pp, t in zip(p, (t0, t1, t2))]
                    cols.append(w[:, :, k[0], k[1], k[2]].t())          # [Cout, Cin]
        mats.append(torch.cat(cols, dim=1).contiguous())                   # [Cout, ntaps * Cin]
        offs.append(off)
        off += mats[-1].numel()
    packed = cout % 16 == 0 and cin % 32 == 0
    return torch.cat([m.reshape(-1) for m in mats] + ([_pack_fragments(m) for m in mats] if packed else [])), 512 if packed else 0, offs


def _split16(w: torch.Tensor, dev):
    hi = w.to(torch.float16)
    lo = (w - hi.float()).to(torch.float16)
    return hi.to(dev).contiguous(), lo.to(dev).contiguous()


# ---- operand records -----------------------------------------------------------------------------------
class _Conv:
    """Operands of GroupNorm (optional) + Conv3d k^3 pad k//2: split-fp16 weight matrix (conv_fwd_layout), GroupNorm affine, bias.
    Inference builds it from a weight (`_Conv(...)`); the trainer wraps its persistent hi / lo buffers and live parameters (`_Conv.of`)."""
    name = None          # training: the layer's key prefix in the state dict
    bwd = None           # training: (hi, lo, flag word) of the data-gradient matrix

    def __init__(self, weight: torch.Tensor, gn_w, gn_b, bias, groups: int, dev):
        flat, packed = conv_fwd_layout(weight.float())
        f = lambda t: None if t is None else t.float().to(dev).contiguous()
        self._set((*_split16(flat, dev), packed), weight.shape, f(gn_w), f(gn_b), f(bias), groups)

    def _set(self, fwd, wshape, gn_w, gn_b, bias, groups):
        self.w_hi, self.w_lo, self.packed = fwd
        self.cout, self.cin, self.k = int(wshape[0]), int(wshape[1]), int(wshape[2])
        self.gn_w, self.gn_b, self.bias = gn_w, gn_b, bias
        self.groups = groups if self.cin >= groups else 1

    @classmethod
    def of(cls, name, fwd, bwd, wshape, gn_w, gn_b, bias, groups):
        """Training: nothing is copied - fwd / bwd are _WeightLayouts' persistent gather targets, gn_w / gn_b / bias the live parameters.  UNetTrainer.refresh()
        rebuilds the record every step, so a replaced parameter tensor is picked up no later than the next step (when its layouts are re-gathered too)."""
        r = cls.__new__(cls)
        r.name, r.bwd = name, bwd
        r._set(fwd, wshape, gn_w, gn_b, bias, groups)
        return r


class _ConvT:
    """Operands of ConvTranspose3d k3 s2 p1 (+ output_padding 1 via output_size): 8 parity-class weight matrices (convT_class_layout)."""
    name = None
    bwd = None

    def __init__(self, weight: torch.Tensor, bias, dev):
        flat, packed, offs = convT_class_layout(weight.float())
        self._set((*_split16(flat, dev), packed, offs), weight.shape, bias.float().to(dev).contiguous())

    def _set(self, fwd, wshape, bias):
        self.w_hi, self.w_lo, self.packed, offs = fwd
        self.class_off = (C.c_long * 8)(*offs)
        self.cin, self.cout = int(wshape[0]), int(wshape[1])
        self.bias = bias

    @classmethod
    def of(cls, name, fwd, bwd, wshape, bias):
        """Training: like _Conv.of - persistent hi / lo buffers and the live bias parameter, rebuilt by every UNetTrainer.refresh()."""
        r = cls.__new__(cls)
        r.name, r.bwd = name, bwd
        r._set(fwd, wshape, bias)
        return r


class _Rec:
    """Tape entry of one GroupNorm + Conv3d: what the backward pass needs."""
    __slots__ = ("name", "x", "y", "mean", "rstd", "scale", "shift")


# ---- forward traversal -----------------------------------------------------------------------------------
# ONE launch sequence for inference (ResidualUNet3D.forward_cl) and training (train.UNetTrainer.forward).  `zeros(shape, dtype)` hands out zeroed
# statistics buffers; f32 = 1: fp32 activations ("exact"), 0: fp16; tape / rec: training only - what the backward pass needs is recorded.

def gn_conv(x, conv: _Conv, relu, zeros, f32, resid=None, gn=True, in_sums=None, out_groups=0, generic=False, occ=None, rec: _Rec | None = None):
    """GroupNorm (gn) + convolution (+ resid, ReLU) -> (y, GroupNorm statistics of y or None).
    in_sums: statistics of x (fp64 [B, groups, 2]) when its producer already has them (scatter / the previous convolution / the transposed
    convolution: fused into their epilogues, no pass over x); out_groups > 0: have this convolution produce the statistics of ITS output.
    generic: run the generic gather kernel even where an LDS-brick kernel exists (bit 8 of the flag word; per-call cross-check for tests).
    occ: x is SPARSE (semabs_scatter_mean_sparse): uint32 occupancy bitmap; voxels whose bit is clear are zero and are not read."""
    B, D0, D1, D2, Cc = x.shape
    nvox, dev, st = D0 * D1 * D2, x.device, _lib.stream()
    scale = shift = None
    if gn:
        G, sums = conv.groups, in_sums
        if sums is None:
            sums = zeros((B, G, 2), torch.float64)
            _lib.call("semabs_gn_stats", _lib.ptr(x), _lib.ptr(sums), B, nvox, Cc, G, f32, st)
        scale = torch.empty(B, Cc, dtype=torch.float32, device=dev)
        shift = torch.empty_like(scale)
        _lib.call("semabs_gn_finalize", _lib.ptr(sums), _lib.ptr(conv.gn_w), _lib.ptr(conv.gn_b), _lib.ptr(scale), _lib.ptr(shift),
                  B, Cc, G, nvox, 1e-5, st)
        if rec is not None:
            rec.mean = torch.empty(B, G, dtype=torch.float32, device=dev)
            rec.rstd = torch.empty_like(rec.mean)
            _lib.call("semabs_gn_meanrstd", _lib.ptr(sums), _lib.ptr(rec.mean), _lib.ptr(rec.rstd), B, G, nvox * (Cc // G), 1e-5, st)
    y = torch.empty(B, D0, D1, D2, conv.cout, dtype=torch.float32 if f32 else torch.float16, device=dev)
    if rec is not None:
        rec.name, rec.x, rec.y, rec.scale, rec.shift = conv.name, x, y, scale, shift
    args = (_lib.ptr(x), _lib.ptr(conv.w_hi), _lib.ptr(conv.w_lo), _lib.ptr(y), _lib.ptr(scale), _lib.ptr(shift),
            _lib.ptr(conv.bias), _lib.ptr(resid), B, D0, D1, D2, conv.cin, conv.cout, conv.k, int(relu), f32 | (256 if generic else 0) | conv.packed)
    if not out_groups:
        assert occ is None
        _lib.call("semabs_conv3d", *args, st)
        return y, None
    out_sums = zeros((B, out_groups, 2), torch.float64)
    if occ is not None:
        _lib.call("semabs_conv3d_sparse_stats", args[0], _lib.ptr(occ), *args[1:], _lib.ptr(out_sums), out_groups, st)
    else:
        _lib.call("semabs_conv3d_stats", *args, _lib.ptr(out_sums), out_groups, st)
    return y, out_sums


def res_block(x, convs, zeros, f32, in_sums=None, occ=None, tape=None):
    """relu(conv3(out2) + out1): conv1 / conv2 hand the statistics of their outputs to the GroupNorm of conv2 / conv3 (fused into the epilogue where
    supported); in_sums: the statistics of x when its producer already has them (the transposed convolution of a decoder level)."""
    r1, r2, r3 = (None,) * 3 if tape is None else (_Rec(), _Rec(), _Rec())
    out1, s1 = gn_conv(x, convs[0], True, zeros, f32, in_sums=in_sums, out_groups=convs[1].groups, occ=occ, rec=r1)
    out2, s2 = gn_conv(out1, convs[1], True, zeros, f32, in_sums=s1, out_groups=convs[2].groups, rec=r2)
    y, _ = gn_conv(out2, convs[2], True, zeros, f32, resid=out1, in_sums=s2, rec=r3)          # conv3 (no ReLU) + residual, then ReLU
    if tape is not None:
        tape.append(("block", r1, r2, r3))
    return y


def maxpool(x, f32):
    B, D0, D1, D2, Cc = x.shape
    y = torch.empty(B, D0 // 2, D1 // 2, D2 // 2, Cc, dtype=x.dtype, device=x.device)
    _lib.call("semabs_maxpool3d", _lib.ptr(x), _lib.ptr(y), B, D0, D1, D2, Cc, f32, _lib.stream())
    return y


def up_conv(x, skip, ct: _ConvT, zeros, f32, out_groups=0, generic=False):
    """ConvTranspose3d(k3, s2) + skip -> (y, GroupNorm statistics of y for the block that follows when out_groups > 0, else None)."""
    B, D0, D1, D2, _ = x.shape
    assert tuple(skip.shape) == (B, 2 * D0, 2 * D1, 2 * D2, ct.cout)
    y = torch.empty_like(skip)
    args = (_lib.ptr(x), _lib.ptr(ct.w_hi), _lib.ptr(ct.w_lo), ct.class_off, _lib.ptr(y),
            _lib.ptr(ct.bias), _lib.ptr(skip), B, D0, D1, D2, ct.cin, ct.cout, f32 | (256 if generic else 0) | ct.packed)
    if not out_groups:
        _lib.call("semabs_convtranspose3d", *args, _lib.stream())
        return y, None
    sums = zeros((B, out_groups, 2), torch.float64)
    _lib.call("semabs_convtranspose3d_stats", *args, _lib.ptr(sums), out_groups, _lib.stream())
    return y, sums


def unet_forward(x, enc, dec, final: _Conv, zeros, f32, in_sums=None, occ=None, taps=None, skip_final=False, tape=None, rows_w=None):
    """Encoder / decoder walk over the operand records enc = [[conv1, conv2, conv3]] per level, dec = [(_ConvT, [conv1, conv2, conv3])], final.
    in_sums / occ: see gn_conv (first layer only); taps: dict collecting the level outputs; skip_final: return the input of `final`.
    tape: list receiving ("pool", x, level) / ("up", name, x, level) / ("block", r1, r2, r3) / ("final", x) for the backward pass.
    rows_w: the fp32 [Cout, Cin] weight of `final` - the 1 x 1 x 1 convolution IS a row-linear layer over the voxels and semabs_linear_rows streams it
    at HBM speed (the gather kernel: 1.28 ms at 8 x 128^3); a different kernel with different rounding, so only the trainer passes it."""
    feats = []
    for i, convs in enumerate(enc):
        if i > 0:
            if tape is not None:
                tape.append(("pool", x, i - 1))
            x = maxpool(x, f32)
        x = res_block(x, convs, zeros, f32, in_sums=in_sums if i == 0 else None, occ=occ if i == 0 else None, tape=tape)
        if taps is not None:
            taps[f"enc{i}"] = x
        feats.insert(0, x)
    for i, (skip, (ct, convs)) in enumerate(zip(feats[1:], dec)):
        y, sums = up_conv(x, skip, ct, zeros, f32, out_groups=convs[0].groups)
        if tape is not None:
            tape.append(("up", ct.name, x, len(enc) - 2 - i))
        x = res_block(y, convs, zeros, f32, in_sums=sums, tape=tape)
        if taps is not None:
            taps[f"dec{i}"] = x
    if skip_final:
        return x
    if tape is not None:
        tape.append(("final", x))
    if rows_w is None:
        return gn_conv(x, final, False, zeros, f32, gn=False)[0]
    B, D0, D1, D2, _ = x.shape
    y = torch.empty(B, D0, D1, D2, final.cout, dtype=torch.float32, device=x.device)
    _lib.call("semabs_linear_rows", _lib.ptr(x), final.cin, _lib.ptr(rows_w), final.cin, 1, _lib.ptr(final.bias), _lib.ptr(y),
              B * D0 * D1 * D2, final.cin, final.cout, 0, 0.0, None, None, None, None, None, None, _lib.stream())
    return y


class ResidualUNet3D(torch.nn.Module):
    """nn.Module surface of the reference (`parameters()`, `state_dict()` / `load_state_dict()`, `.to()`, `train()` / `eval()`); the forward pass
    is inference-only (no autograd graph) and runs on the HIP kernels with operands derived from the parameters (see module.py)."""

    def __init__(self, in_channels, out_channels, f_maps=64, num_groups=8, num_levels=5, final_sigmoid=False,
                 layer_order="gcr", is_segmentation=False, precision: str = "exact", **kwargs):
        super().__init__()
        assert layer_order == "gcr" and not is_segmentation, "the path uses order 'gcr' without a final activation"
        assert precision in ("fp16", "exact")
        if isinstance(f_maps, int):
            f_maps = number_of_features_per_level(f_maps, num_levels=num_levels)
        self.f_maps = list(f_maps)
        self.in_channels, self.out_channels, self.num_groups = in_channels, out_channels, num_groups
        # "exact" (fp32 activations, split-fp16 MFMA operands: the reference's fp32 results to ~1e-5) is the default of the reference-surface
        # classes; "fp16" is the opt-in fast mode (activations rounded to fp16: 3.6e-3 on the voxel logits, measured)
        self.precision = precision
        self.f32 = int(precision == "exact")
        self.act_dtype = torch.float32 if self.f32 else torch.float16
        from .module import register_tree
        from .weights import make_unet_state_dict
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())            # follows torch's RNG like the reference's default init (seed_all)
        register_tree(self, make_unet_state_dict(seed, in_channels, out_channels, self.f_maps[0], len(self.f_maps)))
        self._sums_arena = None
        self.enc: List[List[_Conv]] = []
        self.dec: List = []
        self.final = None
        self._sig = None

    @property
    def dev(self):
        return _lib.require_gpu()

    # ---- weights -----------------------------------------------------------------------------------
    def expected_keys(self):
        from .weights import unet_layer_plan
        keys = []
        for pre, kind, cin, cout in unet_layer_plan(self.in_channels, self.out_channels, self.f_maps[0], len(self.f_maps)):
            if kind in ("gcr", "gc"):
                keys += [pre + "groupnorm.weight", pre + "groupnorm.bias", pre + "conv.weight"]
            else:
                keys += [pre + "weight", pre + "bias"]
        return keys

    def load_state_dict(self, state_dict, strict: bool = True, prefix: str = "", **kw):
        """nn.Module.load_state_dict (missing / unexpected keys raise under strict=True, are reported under strict=False) + an optional key
        `prefix` to pick this module's entries out of an enclosing state dict."""
        from .module import strip_module_prefix
        sd = strip_module_prefix(state_dict)
        if prefix:
            sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
        return super().load_state_dict(sd, strict=strict, **kw)

    def _sync(self):
        """(Re)build the kernel operands when a parameter changed (module.signature)."""
        from .module import signature
        dev = _lib.require_gpu()
        if any(p.device.type != "cuda" for p in self.parameters()):
            self.to(dev)                                # there is no CPU path: a module left on the host is moved to the HIP device on first use
        sig = signature(self)
        if sig == self._sig:
            return
        sd = {k: v.detach() for k, v in self.state_dict().items()}
        G = self.num_groups

        def block(pre):
            return [_Conv(sd[pre + f"conv{j}.conv.weight"], sd[pre + f"conv{j}.groupnorm.weight"],
                          sd[pre + f"conv{j}.groupnorm.bias"], None, G, dev) for j in (1, 2, 3)]

        L = len(self.f_maps)
        self.enc = [block(f"encoders.{i}.basic_module.") for i in range(L)]
        self.dec = [(_ConvT(sd[f"decoders.{i}.upsampling.upsample.weight"], sd[f"decoders.{i}.upsampling.upsample.bias"], dev),
                     block(f"decoders.{i}.basic_module.")) for i in range(L - 1)]
        self.final = _Conv(sd["final_conv.weight"], None, None, sd["final_conv.bias"], G, dev)
        self._sig = sig

    # ---- kernels (the launch sequences are the module-level functions above) ------------------------------
    def _zero_sums(self, shape, dtype=torch.float64) -> torch.Tensor:
        """fp64 [B, G, 2] of zeros for one layer's GroupNorm statistics, cut from an arena that ONE fill zeroes per forward pass (a forward needs ~30
        of them: one launch instead of thirty).  Outside a forward pass (no arena open) it is a plain zero-filled buffer."""
        assert dtype == torch.float64 and len(shape) == 3
        n = shape[0] * shape[1] * shape[2]
        a = self._sums_arena
        if a is None or a[1] + n > a[0].numel():
            return _lib.filled(tuple(shape), torch.float64, 0, self.dev)
        t = a[0][a[1]:a[1] + n].view(*shape)
        a[1] += n
        return t

    def _conv(self, x, conv: _Conv, relu, resid=None, gn=True, in_sums=None, out_groups=0, generic=False, occ=None):
        """gn_conv; out_groups > 0: -> (y, GroupNorm statistics of y, fp64 [B, out_groups, 2], for the next layer), else y."""
        y, sums = gn_conv(x, conv, relu, self._zero_sums, self.f32, resid, gn, in_sums, out_groups, generic, occ)
        return (y, sums) if out_groups else y

    @staticmethod
    def sparse_input_supported(shape, conv: "_Conv") -> bool:
        """The first convolution can read a sparse (bitmap-described) input: the 16 -> 16 level-0 kernel's shapes."""
        _, D0, D1, D2, Cc = shape
        return conv.k == 3 and conv.cin == 16 and conv.cout == 16 and Cc == 16 and D0 % 8 == 0 and D1 % 8 == 0 and D2 % 16 == 0 and D0 * D1 * D2 * 16 < 2 ** 31

    def _pool(self, x):
        return maxpool(x, self.f32)

    def _up(self, x, skip, ct: _ConvT, out_groups=0, generic=False):
        """up_conv; out_groups > 0: -> (y, GroupNorm statistics of y for the block that follows), else y."""
        y, sums = up_conv(x, skip, ct, self._zero_sums, self.f32, out_groups, generic)
        return (y, sums) if out_groups else y

    # ---- forward -----------------------------------------------------------------------------------
    @torch.no_grad()
    def forward_cl(self, x: torch.Tensor, taps: dict | None = None, skip_final: bool = False, in_sums=None, occ=None) -> torch.Tensor:
        """x [B, D0, D1, D2, Cin] channels-last (act dtype, GPU) -> [B, D0, D1, D2, Cout]  (skip_final: the input of `final_conv`;
        in_sums: GroupNorm statistics of x, fp64 [B, groups, 2], when its producer already has them; occ: x is sparse - occupancy bitmap, see gn_conv)."""
        self._sync()
        assert x.dtype == self.act_dtype and x.is_contiguous()
        # statistics arena of this pass: (3 per residual block + 1 per transposed convolution) x [B, <= num_groups, 2] doubles, zeroed by one launch;
        # a fresh allocation per pass (the caching allocator recycles it), so passes on different streams never share one
        n_layers = 3 * (len(self.enc) + len(self.dec)) + len(self.dec) + 2
        self._sums_arena = [_lib.filled((n_layers * int(x.shape[0]) * max(1, self.num_groups) * 2,), torch.float64, 0, self.dev), 0]
        try:
            return unet_forward(x, self.enc, self.dec, self.final, self._zero_sums, self.f32, in_sums, occ, taps, skip_final)
        finally:
            self._sums_arena = None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """NCDHW fp32 in / out like the reference (two layout copies around the channels-last core)."""
        dev = _lib.require_gpu()
        xc = x.to(dev).permute(0, 2, 3, 4, 1).contiguous().to(self.act_dtype)
        y = self.forward_cl(xc)
        return y.permute(0, 4, 1, 2, 3).contiguous().float()
