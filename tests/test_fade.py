"""Crossfaded coefficient changes (bfir_engine_set_coeff_fade) without a GPU: the C ABI as declared and exported, the
Python and C++ bindings, the register report of the fade kernels, and the expected-output helper the GPU tests use."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bfir_hip.h")
FADE_FNS = ("bfir_engine_set_coeff_fade", "bfir_engine_set_coeff_matrix_fade", "bfir_engine_fade_remaining")

# The compiler's occupancy (waves per SIMD by registers) per k_inv_fade instance, by log2 of its N = 2L points, as
# DESIGN.md "k_inv_fade" lists it beside the LDS footprint that bounds the workgroups per CU.
FADE_OCCUPANCY = {10: 5, 11: 5, 12: 4, 13: 4, 14: 4}
FADE_LDS_BYTES = {10: 8456, 11: 16912, 12: 33824, 13: 67648, 14: 135296}


def fade_weights(L, nb, t0, K):
    """w[n] of every sample of nb blocks: 0 before block t0, m / (K L - 1) for m = 0 .. K L - 1 from block t0, 1 after."""
    w = np.zeros(nb * L)
    w[t0 * L:] = 1.0
    n = min(K, nb - t0) * L
    w[t0 * L:t0 * L + n] = (np.arange(K * L) / (K * L - 1.0))[:n]
    return w


def fade_expected(orc, L, B, s, C, h_old, h_new, x, t0, K, in_fmt=None, out_fmt=None):
    """Two oracle engines with the old and the new filters, fed the same input from block 0, blended in float64:
    y_old (1 - w) + y_new w.  Returns (expected, y_old, y_new), float64 [frames, C]."""
    ys = []
    for h in (h_old, h_new):
        e = orc.Engine(L, B, s, C, in_fmt, out_fmt)
        assert e.set_coeff(h) == 0
        rc, y = e.run(x)
        assert rc == 0
        ys.append(np.asarray(y, dtype=np.float64))
        e.close()
    w = fade_weights(L, x.shape[0] // L, t0, K)[:, None]
    return ys[0] * (1.0 - w) + ys[1] * w, ys[0], ys[1]


def _decl(name):
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, open(HEADER).read(), re.S)
    assert m, name
    return m.group(1)


@pytest.mark.parametrize("name", FADE_FNS)
def test_header_declares_the_fade_functions(name):
    args = _decl(name)
    assert not re.search(r"\blong\b", args), args
    for a in args.split(","):
        assert re.match(r"\s*(const\s+)?(int|double|void|bfir_engine)\b", a), a


def test_library_exports_and_bindings(bfir):
    from foo_dsp_bfir_amd import _lib
    lib = bfir.load()
    for name in FADE_FNS:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).restype == _lib.SIGNATURES[name][0]
    if shutil.which("nm"):
        syms = subprocess.run(["nm", "-D", "--defined-only", bfir.library_path()], capture_output=True, text=True).stdout
        for name in FADE_FNS:
            assert re.search(r"\bT %s$" % name, syms, re.M), name
    for cls in (bfir.Brutefir, bfir.BrutefirMatrix):
        assert callable(cls.set_coeff_fade) and callable(cls.fade_remaining)
    assert bfir.BrutefirMatrix.set_coeff_fade is not bfir.Brutefir.set_coeff_fade


def test_null_engine_is_an_argument_error_without_a_device(bfir):
    lib = bfir.load()
    taps = np.zeros(4, np.float32)
    ptrs = (C.c_void_p * 1)(taps.ctypes.data)
    assert lib.bfir_engine_set_coeff_fade(None, ptrs, 1, 4, 1, 1.0, 1) == bfir.ERR_ARG
    assert lib.bfir_engine_set_coeff_matrix_fade(None, ptrs, 4, 1, 1.0, 1) == bfir.ERR_ARG
    assert lib.bfir_engine_fade_remaining(None) == bfir.ERR_ARG


def test_cpp_mirror_with_a_fade_caller_compiles(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++ on this machine")
    src = tmp_path / "caller.cpp"
    src.write_text('#include "%s"\n'
                   "int fade(brutefir &f, void **h) { int rc = f.set_coeff_fade(h, 2, 100, 4, 1.0, 7); return rc ? rc : f.fade_remaining(); }\n"
                   % os.path.join(ROOT, "foo-dsp-bfir_amd", "host", "brutefir_hip.hpp"))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", str(src)], check=True)


def test_fade_kernel_register_report():
    """Every k_inv_fade / k_fade_blend instance: no scratch, no spill, no dynamic stack; one k_inv_fade per pair plan size;
    occupancy and LDS as DESIGN.md records them, so a later regression shows."""
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc on this machine")
    import importlib
    import sys
    sys.path.insert(0, ROOT)
    b = importlib.import_module("foo_dsp_bfir_amd._build")
    b.build()
    u = b.resource_usage()
    inv = {k: v for k, v in u.items() if "k_inv_fade" in k}
    blend = {k: v for k, v in u.items() if "k_fade_blend" in k}
    assert len(inv) == 5, sorted(inv)
    assert len(blend) == 4, sorted(blend)                    # float / double x 16 bytes per lane / one sample per lane
    for name, r in list(inv.items()) + list(blend.items()):
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["Dynamic Stack"] == "False", (name, r)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name, r in inv.items():
        lg = int(re.search(r"k_inv_fadeILi(\d+)E", name).group(1))
        assert r["Occupancy"] == FADE_OCCUPANCY[lg] and r["LDS Size"] == FADE_LDS_BYTES[lg], (name, r)
        assert re.search(r"\|\s*%d\s*\|\s*%d\s*\|\s*%d\s*\|" % (1 << lg, FADE_LDS_BYTES[lg], FADE_OCCUPANCY[lg]), design), lg
    for r in blend.values():
        assert r["Occupancy"] == 8, r


@pytest.mark.parametrize("K", [1, 3])
def test_expected_output_helper_against_direct_convolution(orc, K):
    """2 channels, L = 64, B = 3, ragged taps: the helper equals (1 - w) direct(x, h_old) + w direct(x, h_new)."""
    L, B, Cn, t0 = 64, 3, 2, 4
    nb = 2 * B + K + 3
    rng = np.random.default_rng(40 + K)
    h_old = orc.synth_ir(rng, Cn, B * L - 13, np.float64)
    h_new = orc.synth_ir(rng, Cn, B * L - 29, np.float64)
    x = orc.synth_audio(rng, nb * L, Cn, np.float64)
    y, y_old, y_new = fade_expected(orc, L, B, 8, Cn, h_old, h_new, x, t0, K)
    w = fade_weights(L, nb, t0, K)
    assert w[t0 * L - 1] == 0.0 and w[t0 * L] == 0.0 and w[(t0 + K) * L - 1] == 1.0 and w[-1] == 1.0
    assert np.all(np.diff(w[t0 * L:(t0 + K) * L]) > 0)
    want = np.stack([(1 - w) * orc.direct_conv(x[:, c], h_old[c]) + w * orc.direct_conv(x[:, c], h_new[c])
                     for c in range(Cn)], axis=1)
    assert np.abs(y - want).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(y[:t0 * L], y_old[:t0 * L]) and np.array_equal(y[(t0 + K) * L:], y_new[(t0 + K) * L:])
