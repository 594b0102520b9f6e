"""Crossfaded coefficient changes on multi-level matrix engines (bfir_engine_set_coeff_matrix_levels_fade) without a GPU:
the C ABI as declared and exported, the Python and C++ bindings, the register report of k_mac_duo (csrc/mfade.hip) and of the
kernels it must leave alone, and the definition the GPU tests hold the engine to: the blend of two per-pair level models
(test_mlevels.mlevels_model) is the blend of two uniform references (test_mlevels.uniform_reference) with
test_fade.fade_weights."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import TOL, rel_err
from test_fade import fade_weights
from test_levels import level_geometry
from test_mlevels import mlevels_model, uniform_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bfir_hip.h")
NAME = "bfir_engine_set_coeff_matrix_levels_fade"

# k_mac_duo<T, ILV, NO, TT> as launch_mac_duo picks them: fp32 one or two outputs per tile, fp64 one; the latency form
# (TT = 1) and the tiled one (fp32 8, fp64 4 blocks per lane); both spectrum layouts
DUO_INSTANCES = {(t, ilv, no, tt) for t, nos, tts in (("f", (1, 2), (1, 8)), ("d", (1,), (1, 4)))
                 for ilv in (0, 1) for no in nos for tt in tts}


def _decl(name):
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, open(HEADER).read(), re.S)
    assert m, name
    return m.group(1)


def test_header_declares_the_function():
    args = _decl(NAME)
    assert not re.search(r"\blong\b", args), args
    assert len(args.split(",")) == 5
    for a in args.split(","):
        assert re.match(r"\s*(const\s+)?(int|double|void|bfir_engine)\b", a), a
    # the entry cites the reference's blend, as the other fade entries do, and states its rules
    before = open(HEADER).read().split(NAME + "(")[0]
    comment = before[before.rindex("/*"):]
    assert "fftw_convolver.cpp:275-321" in comment
    for word in ("BFIR_ERR_ARG", "BFIR_ERR_STATE", "BFIR_ERR_COEFF", "BFIR_ERR_UNSUPPORTED", "per level", "BOTH sets"):
        assert word in comment, word
    assert "it has no crossfade" not in open(HEADER).read()


def test_library_exports_and_bindings(bfir):
    from foo_dsp_bfir_amd import _lib
    lib = bfir.load()
    assert NAME in _lib.SIGNATURES
    assert getattr(lib, NAME).restype == _lib.SIGNATURES[NAME][0] and len(_lib.SIGNATURES[NAME][1]) == 5
    if shutil.which("nm"):
        syms = subprocess.run(["nm", "-D", "--defined-only", bfir.library_path()], capture_output=True, text=True).stdout
        assert re.search(r"\bT %s$" % NAME, syms, re.M)
    cls = bfir.BrutefirMatrixLevels
    assert callable(cls.fade_to_rows) and not hasattr(bfir.BrutefirLevels, "fade_to_rows")
    assert cls.fade_to is not bfir.BrutefirLevels.fade_to                # ... which keeps raising on this kind, as does
    assert cls.set_coeff_fade is not bfir.BrutefirMatrix.set_coeff_fade   # the uniform matrix fade
    assert "ERR_UNSUPPORTED" in cls.fade_to_rows.__doc__ and "fade_to" in cls.fade_to_rows.__doc__


def test_null_engine_is_an_argument_error_without_a_device(bfir):
    lib = bfir.load()
    taps = np.zeros(4, np.float32)
    ptrs = (C.c_void_p * 1)(taps.ctypes.data)
    lens = (C.c_int * 1)(4)
    assert getattr(lib, NAME)(None, ptrs, lens, 1.0, 1) == bfir.ERR_ARG
    assert lib.bfir_engine_fade_remaining_levels(None) == bfir.ERR_ARG


def test_cpp_mirror_with_a_fading_matrix_caller_compiles(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++ on this machine")
    src = tmp_path / "caller.cpp"
    src.write_text('#include "%s"\n'
                   "int fade(brutefir &f, void **h, const int *lengths) {\n"
                   "    int rc = f.set_coeff_matrix_levels_fade(h, lengths, 1.0, 7);\n"
                   "    return rc ? rc : f.fade_remaining_levels(); }\n"
                   % os.path.join(ROOT, "foo-dsp-bfir_amd", "host", "brutefir_hip.hpp"))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", str(src)], check=True)
    mirror = os.path.join(ROOT, "tests", "cpp", "test_mlevels_fade_mirror.cpp")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", mirror], check=True)


def test_duo_kernel_register_report():
    """Every k_mac_duo instance: no scratch, no spill, no dynamic stack, no LDS, at least the four waves per SIMD of its
    launch bounds; the twelve instances launch_mac_duo can pick; registers and occupancy as DESIGN.md records them, so a
    later regression shows.  The kernels the other register tests count by substring keep their counts."""
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc on this machine")
    import importlib
    import sys
    sys.path.insert(0, ROOT)
    b = importlib.import_module("foo_dsp_bfir_amd._build")
    assert "mfade.hip" in b.SOURCES
    b.build()
    u = b.resource_usage()
    duo = {k: v for k, v in u.items() if "k_mac_duo" in k}
    assert len(duo) == 12, sorted(duo)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "twelve instances" in design
    seen = set()
    for name, r in duo.items():
        for other in ("k_mac_matrix", "k_inv_fade", "k_inv_lfade", "k_inv_lone", "k_inv_levels", "k_inv_nup"):
            assert other not in name, name
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["Dynamic Stack"] == "False", (name, r)
        assert r["LDS Size"] == 0 and r["Occupancy"] >= 4, (name, r)
        m = re.search(r"k_mac_duoI([fd])Lb([01])ELi(\d+)ELi(\d+)E", name)
        key = (m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)))
        seen.add(key)
        row = r"\|\s*%s\s*\|\s*%s\s*\|\s*%d\s*\|\s*%d\s*\|\s*%d\s*\|\s*%d\s*\|" % (
            "fp32" if key[0] == "f" else "fp64", "pairs" if key[1] else "groups", key[2], key[3], r["VGPRs"], r["Occupancy"])
        assert re.search(row, design), (key, r["VGPRs"], r["Occupancy"])
    assert seen == DUO_INSTANCES
    for sub, n in (("k_mac_matrix", 20), ("k_inv_lfade", 15), ("k_inv_lone", 20)):
        assert len([k for k in u if sub in k]) == n, sub


@pytest.mark.parametrize("s", [4, 8])
@pytest.mark.parametrize("K", [1, 5])
def test_blend_of_two_level_models_is_the_blend_of_two_uniform_references(orc, s, K):
    """S_old and S_new per output -- the sum over the inputs of ((y_head + z_1) + z_2) of every pair -- blended with the ramp
    over K head blocks, against the blend of two uniform references: the yardstick of tests/test_mlevels_fade_gpu.py.  2 -> 3
    on three levels (the model shape of test_mlevels); a NULL pair that moves, filters that change level between the sets,
    the fade starts inside a block of every level."""
    L, blocks, ratios = 16, (2, 2, 3), (1, 2, 2)
    Ls, D = level_geometry(L, blocks, ratios)
    dt = np.float64 if s == 8 else np.float32
    rng = np.random.default_rng(57 + s + K)
    lens = ([[D[1] - 5, D[3] - Ls[2] + Ls[2] // 3 + 1], [None, D[2] - 9], [D[1] + 3, None]],
            [[D[3] - 2 * Ls[2] + 7, D[1] - 3], [D[2] + 1, None], [None, D[1] + Ls[1] + 2]])
    sets = [[[None if n is None else orc.synth_ir(rng, 1, n, dt)[0] for n in r] for r in ln] for ln in lens]
    r_last = Ls[-1] // L
    t0 = (D[-2] // L + r_last) | 1                                       # odd: inside a block of every level
    assert all(t0 % (Lk // L) for Lk in Ls[1:])
    nb = t0 + K + r_last + 3
    x = orc.synth_audio(rng, nb * L, 2, dt)
    w = fade_weights(L, nb, t0, K)[:, None]
    u_old, u_new = (uniform_reference(orc, L, s, rows, x) for rows in sets)
    want = u_old * (1.0 - w) + u_new * w
    s_old, s_new = (mlevels_model(orc, L, blocks, ratios, s, rows, x) for rows in sets)
    got = s_old * (1.0 - w) + s_new * w
    print("rel_err", s, K, rel_err(got, want))
    assert rel_err(got, want) <= TOL[s]
    assert np.array_equal(got[:t0 * L], s_old[:t0 * L]) and np.array_equal(got[(t0 + K) * L:], s_new[(t0 + K) * L:])
    assert rel_err(got[t0 * L:(t0 + K) * L], u_old[t0 * L:(t0 + K) * L]) > TOL[s]     # the fade's blocks are neither set's
