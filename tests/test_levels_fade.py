"""Crossfaded coefficient changes on two-level and multi-level engines (bfir_engine_set_coeff_nup_fade /
_set_coeff_levels_fade / _fade_remaining_levels) without a GPU: the C ABI as declared and exported, the Python and C++
bindings, the register report of the kernels of csrc/lfade.hip, and the definition the GPU tests hold the engine to: the
blend of two multi-level models (one uniform oracle engine per level, test_levels.levels_model) is the blend of two uniform
oracle engines (test_fade.fade_expected)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import TOL, rel_err
from test_fade import fade_expected, fade_weights
from test_levels import MODEL_SHAPES, level_geometry, levels_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bfir_hip.h")
LFADE_FNS = ("bfir_engine_set_coeff_nup_fade", "bfir_engine_set_coeff_levels_fade", "bfir_engine_fade_remaining_levels")

# Per k_inv_lfade instance, (log2 of its N = 2L points, rings per set): the compiler's occupancy (waves per SIMD by
# registers); the LDS footprint depends on the size alone.  As DESIGN.md "k_inv_lfade" lists them.
LFADE_OCCUPANCY = {(10, 1): 5, (10, 2): 5, (10, 3): 5, (11, 1): 5, (11, 2): 5, (11, 3): 5, (12, 1): 4, (12, 2): 4, (12, 3): 4,
                   (13, 1): 4, (13, 2): 4, (13, 3): 4, (14, 1): 4, (14, 2): 4, (14, 3): 4}
LFADE_LDS_BYTES = {10: 8456, 11: 16912, 12: 33824, 13: 67648, 14: 135296}


def _decl(name):
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, open(HEADER).read(), re.S)
    assert m, name
    return m.group(1)


@pytest.mark.parametrize("name", LFADE_FNS)
def test_header_declares_the_functions(name):
    args = _decl(name)
    assert not re.search(r"\blong\b", args), args
    for a in args.split(","):
        assert re.match(r"\s*(const\s+)?(int|double|void|bfir_engine)\b", a), a
    # each entry cites the reference's blend, as the uniform fade entry does
    before = open(HEADER).read().split(name + "(")[0]
    assert "fftw_convolver.cpp:275-321" in before[before.rindex("/*"):]


def test_library_exports_and_bindings(bfir):
    from foo_dsp_bfir_amd import _lib
    lib = bfir.load()
    for name in LFADE_FNS:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).restype == _lib.SIGNATURES[name][0]
    if shutil.which("nm"):
        syms = subprocess.run(["nm", "-D", "--defined-only", bfir.library_path()], capture_output=True, text=True).stdout
        for name in LFADE_FNS:
            assert re.search(r"\bT %s$" % name, syms, re.M), name
    for cls in (bfir.BrutefirNup, bfir.BrutefirLevels):
        assert callable(cls.fade_to) and cls.fade_remaining is not bfir.Brutefir.fade_remaining
        assert cls.set_coeff_fade is not bfir.Brutefir.set_coeff_fade    # ... which keeps raising
    assert bfir.BrutefirNup.fade_to is not bfir.BrutefirLevels.fade_to


def test_null_engine_is_an_argument_error_without_a_device(bfir):
    lib = bfir.load()
    taps = np.zeros(4, np.float32)
    ptrs = (C.c_void_p * 1)(taps.ctypes.data)
    assert lib.bfir_engine_set_coeff_nup_fade(None, ptrs, 1, 4, 1.0, 1) == bfir.ERR_ARG
    assert lib.bfir_engine_set_coeff_levels_fade(None, ptrs, 1, 4, 1.0, 1) == bfir.ERR_ARG
    assert lib.bfir_engine_fade_remaining_levels(None) == bfir.ERR_ARG


def test_cpp_mirror_with_a_fading_multi_level_caller_compiles(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++ on this machine")
    src = tmp_path / "caller.cpp"
    src.write_text('#include "%s"\n'
                   "int three(brutefir &f, void **h) { int rc = f.set_coeff_levels_fade(h, 8, 131072, 1.0, 7);\n"
                   "                                   return rc ? rc : f.fade_remaining_levels(); }\n"
                   "int two(brutefir &f, void **h) { int rc = f.set_coeff_nup_fade(h, 2, 65536, 0.5, 3);\n"
                   "                                 return rc ? rc : f.fade_remaining_levels(); }\n"
                   % os.path.join(ROOT, "foo-dsp-bfir_amd", "host", "brutefir_hip.hpp"))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", str(src)], check=True)


def test_lfade_kernel_register_report():
    """Every k_inv_lfade / k_lfade_sum instance: no scratch, no spill, no dynamic stack, LDS within 160 KB; three
    k_inv_lfade (one, two and three rings per set) per pair plan size; occupancy, registers and LDS as DESIGN.md records
    them, so a later regression shows.  The names stay clear of the kernels the other register tests count by substring."""
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc on this machine")
    import importlib
    import sys
    sys.path.insert(0, ROOT)
    b = importlib.import_module("foo_dsp_bfir_amd._build")
    assert "lfade.hip" in b.SOURCES
    b.build()
    u = b.resource_usage()
    inv = {k: v for k, v in u.items() if "k_inv_lfade" in k}
    summ = {k: v for k, v in u.items() if "k_lfade_sum" in k}
    assert len(inv) == 15, sorted(inv)
    assert len(summ) == 4, sorted(summ)                      # float / double x 16 bytes per lane / one sample per lane
    for name, r in list(inv.items()) + list(summ.items()):
        for other in ("k_inv_fade", "k_fade_blend", "k_inv_levels", "k_levels_combine", "k_inv_nup", "k_nup_combine"):
            assert other not in name, name
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["Dynamic Stack"] == "False", (name, r)
        assert r["LDS Size"] <= 160 * 1024, (name, r)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    seen = set()
    for name, r in inv.items():
        m = re.search(r"k_inv_lfadeILi(\d+)ELi(\d+)E", name)
        lg, nr = int(m.group(1)), int(m.group(2))
        seen.add((lg, nr))
        assert r["Occupancy"] == LFADE_OCCUPANCY[(lg, nr)] and r["LDS Size"] == LFADE_LDS_BYTES[lg], (name, r)
        assert re.search(r"\|\s*%d\s*\|\s*%d\s*\|\s*%d\s*\|\s*%d\s*\|\s*%d\s*\|"
                         % (1 << lg, nr, r["VGPRs"], LFADE_LDS_BYTES[lg], LFADE_OCCUPANCY[(lg, nr)]), design), (lg, nr)
    assert seen == set(LFADE_OCCUPANCY)
    for r in summ.values():
        assert r["Occupancy"] == 8 and r["LDS Size"] == 0, r


@pytest.mark.parametrize("shape", [MODEL_SHAPES[3], MODEL_SHAPES[4]], ids=lambda a: "-".join(map(str, a)))
@pytest.mark.parametrize("K", [1, 5])
def test_blend_of_two_level_models_is_the_blend_of_two_uniform_engines(orc, shape, K):
    """S_old and S_new, each ((y_head + z_1) + z_2) of one oracle engine per level on the whole signal history, blended with
    the ramp over K head blocks, against test_fade.fade_expected of the uniform oracle (L, ceil(taps / L)): the yardstick
    of the GPU tests.  One shape has D_1 = L_1, the other no D_k that is a multiple of L_k; the fade starts inside a block
    of every level."""
    s, L, blocks, ratios, Cn = shape
    dt = np.float64 if s == 8 else np.float32
    Ls, D = level_geometry(L, blocks, ratios)
    if shape == MODEL_SHAPES[3]:
        assert D[1] == Ls[1]
    else:
        assert all(D[k] % Ls[k] for k in range(1, len(Ls)))
    r_last = Ls[-1] // L
    taps = D[-2] + (blocks[-1] - 1) * Ls[-1] + Ls[-1] // 3 + 1          # ends inside the last partition of the last level
    t0 = (D[-2] // L + r_last) | 1                                       # odd: inside a block of every level
    assert all(t0 % (Lk // L) for Lk in Ls[1:])
    nb = t0 + K + r_last + 3
    rng = np.random.default_rng(sum(blocks) + L + Cn + K)
    h_old, h_new = orc.synth_ir(rng, Cn, taps, dt), orc.synth_ir(rng, Cn, taps, dt)
    x = orc.synth_audio(rng, nb * L, Cn, dt)
    want, y_old, y_new = fade_expected(orc, L, -(-taps // L), s, Cn, h_old, h_new, x, t0, K)
    w = fade_weights(L, nb, t0, K)[:, None]
    s_old = levels_model(orc, L, blocks, ratios, s, Cn, h_old, x)
    s_new = levels_model(orc, L, blocks, ratios, s, Cn, h_new, x)
    got = s_old * (1.0 - w) + s_new * w
    print("rel_err", shape, K, rel_err(got, want))
    assert rel_err(got, want) <= TOL[s]
    assert np.array_equal(got[:t0 * L], s_old[:t0 * L]) and np.array_equal(got[(t0 + K) * L:], s_new[(t0 + K) * L:])
    assert rel_err(got[t0 * L:(t0 + K) * L], y_old[t0 * L:(t0 + K) * L]) > TOL[s]     # the fade's blocks are neither set's
