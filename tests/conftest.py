import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden():
    cache = {}

    def load(name):
        if name not in cache:
            cache[name] = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
        return cache[name]

    return load


@pytest.fixture(scope="session")
def bpe_vocab(tmp_path_factory):
    """Path of a CLIP BPE merge table rebuilt from tests/golden/bpe_merges_subset.npz (the published table is third-party data the repo does not
    carry): the tokenizer gives the published token ids for every string the tests encode (tests/_bpe_table.py)."""
    from _bpe_table import write_fixture_table
    return write_fixture_table(str(tmp_path_factory.mktemp("bpe") / "bpe_simple_vocab_16e6.txt.gz"))


def sha(a):
    import hashlib
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


# ---- tolerance bars of the hardware-dependent parity tests --------------------------------------------------------------------------------------
# The HIP results are bit-reproducible for a given build, so a bar can sit close to the measured value (1.3 x, so that a 2.5 x
# regression cannot pass) - but they depend on __expf / v_rcp approximations and on the compiler's instruction scheduling: a bar that
# tight is only meaningful for the toolchain it was measured with.  `tol(measured)` = 1.3 x measured on that toolchain, 2 x on any other.
MEASURED_WITH_HIP = "7.0.51831"          # torch.version.hip of the image the `measured` arguments were taken on (ROCm 7.2.0 image, PyTorch 2.10.0+rocm7.0)


def tol(measured: float, tight: float = 1.3, loose: float = 2.0) -> float:
    import torch
    return float(measured) * (tight if getattr(torch.version, "hip", None) == MEASURED_WITH_HIP else loose)


# Per-case measured errors (tests/golden/measured_errors.json: pytest node id + tag -> the error measured on MI355X with MEASURED_WITH_HIP), so that
# EVERY parametrised case of a kernel-level parity test has its own 1.3 x bar instead of one bar at several times the worst case.  Re-record with
#   SEMABS_RECORD_ERRORS=gpurun_out/measured_errors.json python -m pytest tests -m gpu -q     (then copy the file to tests/golden/)
_MEASURED_PATH = os.path.join(GOLDEN, "measured_errors.json")
try:
    import json as _json
    _MEASURED = _json.load(open(_MEASURED_PATH))
except Exception:
    _MEASURED = {}
_RECORDED = {}


@pytest.fixture
def bar(request):
    """bar(tag, err, ceiling) -> bool: err <= min(ceiling, max(tol(measured error of this case), floor)) - the ceiling (the old fixed bar) alone when
    the case has no recorded value.  floor (default 10 % of the ceiling): errors of a few fp32 ulps can double when one rounding flips (the fp64
    GroupNorm statistics are accumulated with atomics, i.e. in a run-dependent order: measured 3 ulps in one run, 4 in the next), so no bar is ever
    tighter than that.  A recorded 0.0 with
    floor = 0 demands 0.0 (bit-exact cases stay bit-exact)."""
    def check(tag: str, err: float, ceiling: float, floor: float | None = None) -> bool:
        key = request.node.nodeid.split("tests/")[-1] + ":" + tag
        err = float(err)
        if os.environ.get("SEMABS_RECORD_ERRORS"):
            _RECORDED[key] = max(err, _RECORDED.get(key, 0.0))
        m = _MEASURED.get(key)
        fl = 0.10 * float(ceiling) if floor is None else float(floor)
        limit = float(ceiling) if (m is None or os.environ.get("SEMABS_RECORD_ERRORS")) else min(float(ceiling), max(tol(m), fl))     # recording: the ceiling alone
        ok = err <= limit
        if not ok:
            print(f"[bar] {key}: error {err:.4e} > limit {limit:.4e} (measured {m}, ceiling {ceiling:.4e})")
        return ok
    return check


def pytest_sessionfinish(session, exitstatus):
    out = os.environ.get("SEMABS_RECORD_ERRORS")
    if out and _RECORDED:
        import json
        os.makedirs(os.path.dirname(os.path.abspath(out)) or ".", exist_ok=True)
        prev = {}
        if os.path.exists(out):
            try:
                prev = json.load(open(out))
            except Exception:
                prev = {}
        prev.update(_RECORDED)
        json.dump(dict(sorted(prev.items())), open(out, "w"), indent=0)
