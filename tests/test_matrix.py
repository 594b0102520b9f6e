"""Matrix engines (n inputs -> m outputs, one filter per pair) without a GPU: the C ABI as declared and exported, the
Python binding, the numpy reference the GPU tests use, and the register budget of k_mac_matrix."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bfir_hip.h")
MATRIX_FNS = ("bfir_engine_create_matrix", "bfir_engine_set_coeff_matrix", "bfir_engine_read_coeff_matrix")


def _decl(name):
    text = open(HEADER).read()
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text, re.S)
    assert m, name
    return m.group(1)


@pytest.mark.parametrize("name", MATRIX_FNS)
def test_header_declares_the_matrix_functions_without_long(name):
    args = _decl(name)
    assert not re.search(r"\blong\b", args), args
    for a in args.split(","):
        assert re.match(r"\s*(const\s+)?(int|int64_t|double|void|bfir_engine)\b", a), a


def test_library_exports_and_binding(bfir):
    from foo_dsp_bfir_amd import _lib
    lib = bfir.load()
    for name in MATRIX_FNS:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).restype == _lib.SIGNATURES[name][0]
    if shutil.which("nm"):
        syms = subprocess.run(["nm", "-D", "--defined-only", bfir.library_path()], capture_output=True, text=True).stdout
        for name in MATRIX_FNS:
            assert re.search(r"\bT %s$" % name, syms, re.M), name
    assert "BrutefirMatrix" in bfir.__all__ and bfir.BrutefirMatrix.__name__ == "BrutefirMatrix"


def test_shape_and_format_refusals_need_no_device(bfir):
    """Checked before any device is looked for: counts outside 1..8, integer frames."""
    import ctypes as C
    lib = bfir.load()
    for n_in, n_out, fi, fo, want in ((0, 2, 8, 8, bfir.ERR_ARG), (9, 2, 8, 8, bfir.ERR_ARG), (2, 0, 8, 8, bfir.ERR_ARG),
                                      (2, 9, 8, 8, bfir.ERR_ARG), (2, 2, 2, 8, bfir.ERR_UNSUPPORTED),
                                      (2, 2, 8, 6, bfir.ERR_UNSUPPORTED), (1, 1, 9, 8, bfir.ERR_UNSUPPORTED)):
        err = C.c_int(0)
        assert not lib.bfir_engine_create_matrix(256, 2, 4, n_in, n_out, fi, fo, 0, C.byref(err))
        assert err.value == want, (n_in, n_out, fi, fo, err.value)


def matrix_reference(orc, L, B, s, rows, x):
    """y[:, o] = sum_i (x_i convolved with h_{o,i}): one oracle engine per output, NULL filters as zeros, float64 sum."""
    fmt = 10 if s == 8 else 8
    dt = np.float64 if s == 8 else np.float32
    taps = max(h.size for r in rows for h in r if h is not None)
    out = []
    for row in rows:
        e = orc.Engine(L, B, s, x.shape[1], fmt, fmt)
        assert e.set_coeff([np.zeros(taps, dt) if h is None else h for h in row]) == 0
        rc, y = e.run(np.ascontiguousarray(x, dtype=dt))
        assert rc == 0
        out.append(y.astype(np.float64).sum(axis=1))
        e.close()
    return np.stack(out, axis=1)


def test_reference_is_the_sum_of_direct_convolutions(orc):
    """2 -> 3 with a ragged tail (taps not a multiple of L) and one NULL filter, against orc.direct_conv."""
    L, B, nb = 64, 3, 2 * 3 + 3
    rng = np.random.default_rng(5)
    taps = B * L - 13
    rows = [[orc.synth_ir(rng, 1, taps, np.float64)[0] for _ in range(2)] for _ in range(3)]
    rows[1][0] = None
    x = orc.synth_audio(rng, nb * L, 2, np.float64)
    y = matrix_reference(orc, L, B, 8, rows, x)
    want = np.zeros_like(y)
    for o, row in enumerate(rows):
        for i, h in enumerate(row):
            if h is not None:
                want[:, o] += orc.direct_conv(x[:, i], h)
    assert np.abs(y - want).max() <= 1e-12 * np.abs(want).max()


def test_mac_matrix_register_budget():
    """Every k_mac_matrix instance: no scratch, at least four waves per SIMD (k_mac_matrix)."""
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc on this machine")
    import importlib
    import sys
    sys.path.insert(0, ROOT)
    b = importlib.import_module("foo_dsp_bfir_amd._build")
    b.build()
    u = {k: v for k, v in b.resource_usage().items() if "k_mac_matrix" in k}
    # float: pairs / groups x 1, 2, 4 outputs x one-block / 8-block tiles; double: pairs / groups x 1, 2 outputs x two tiles
    assert len(u) == 20, sorted(u)
    for name, r in u.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["Dynamic Stack"] == "False", (name, r)
        assert r["Occupancy"] >= 4, (name, r)
