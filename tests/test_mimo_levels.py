"""Multi-level mimo engines (bfir_engine_create_mimo_levels: up to 64 inputs -> 64 outputs, every filter on two to four
partition lengths) without a GPU: the C ABI as declared and exported, the refusals that need no device, the per-pair
levels model past 8 inputs against the uniform reference the GPU tests use, and the register budget of k_wduo
(csrc/wduo.hip) as DESIGN.md tabulates it."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import TOL, rel_err
from test_levels import level_geometry
from test_mlevels import mlevels_model, uniform_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bfir_hip.h")
NAME = "bfir_engine_create_mimo_levels"
F32, F64, S16, F32BE = 8, 10, 2, 9


def _create(lib, L, blocks, ratios, s, n_in, n_out, fi=F32, fo=F32):
    err = C.c_int(12345)
    n = len(blocks)
    h = getattr(lib, NAME)(L, n, (C.c_int * max(1, n))(*blocks), (C.c_int * max(1, n))(*ratios), s, n_in, n_out, fi, fo, 0,
                           C.byref(err))
    return h, err.value


def wide_reference(orc, L, s, rows, x):
    """test_mlevels.uniform_reference -- one uniform oracle engine per output, its channels summed in float64 -- for any number
    of inputs: the oracle stops at 8 channels, so the inputs go in groups of at most 8 and the groups' sums are added in
    float64.  A group no filter reads contributes nothing."""
    y = np.zeros((x.shape[0], len(rows)), np.float64)
    for g0 in range(0, x.shape[1], 8):
        sub = [r[g0:g0 + 8] for r in rows]
        if any(h is not None for r in sub for h in r):
            y += uniform_reference(orc, L, s, sub, np.ascontiguousarray(x[:, g0:g0 + 8]))
    return y


def test_refusals_need_no_device(bfir):
    """The symbol exists, is declared without `long` and bound; counts outside 1 .. 64, what check_levels_args refuses and
    integer or big-endian frames are refused before any device is looked for; valid arguments get as far as the device."""
    text = open(HEADER).read()
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % NAME, text, re.S)
    assert m, NAME
    for a in m.group(1).split(","):
        assert re.match(r"\s*(const\s+)?(int|double|void|bfir_engine)\b", a), a
    from foo_dsp_bfir_amd import _lib
    lib = bfir.load()
    assert _lib.SIGNATURES[NAME] == _lib.SIGNATURES["bfir_engine_create_matrix_levels"]
    assert getattr(lib, NAME).restype == _lib.SIGNATURES[NAME][0]
    if shutil.which("nm"):
        syms = subprocess.run(["nm", "-D", "--defined-only", bfir.library_path()], capture_output=True, text=True).stdout
        assert re.search(r"\bT %s$" % NAME, syms, re.M)
    assert "BrutefirMimoLevels" in bfir.__all__ and issubclass(bfir.BrutefirMimoLevels, bfir.BrutefirMatrixLevels)
    assert NAME in open(os.path.join(ROOT, "foo-dsp-bfir_amd", "host", "brutefir_hip.hpp")).read()
    lv = ((4, 2, 2), (1, 4, 2))
    cases = [((512,) + lv + (4, 0, 2), bfir.ERR_ARG), ((512,) + lv + (4, 65, 2), bfir.ERR_ARG),
             ((512,) + lv + (4, 2, 0), bfir.ERR_ARG), ((512,) + lv + (4, 2, 65), bfir.ERR_ARG),
             ((512, (8,), (1,), 4, 9, 9), bfir.ERR_ARG),                       # one level
             ((512, (3, 2, 2), (1, 4, 2), 4, 9, 9), bfir.ERR_ARG),             # D_1 < L_1
             ((512, (4, 2, 2), (1, 3, 2), 4, 9, 9), bfir.ERR_ARG),             # a ratio that is no power of two
             ((512, (4, 2, 2), (2, 4, 2), 4, 9, 9), bfir.ERR_ARG),             # ratios[0] != 1
             ((500,) + lv + (4, 9, 9), bfir.ERR_ARG), ((512,) + lv + (2, 9, 9), bfir.ERR_ARG),
             ((8,) + lv + (4, 9, 9), bfir.ERR_UNSUPPORTED),                    # L_0 below the uniform engine's range
             ((4096,) + lv + (4, 9, 9), bfir.ERR_UNSUPPORTED),                 # L_2 = 32768 above it
             ((512,) + lv + (4, 9, 9, S16, F32), bfir.ERR_UNSUPPORTED), ((512,) + lv + (4, 9, 9, F32, S16), bfir.ERR_UNSUPPORTED),
             ((512,) + lv + (4, 9, 9, F32BE, F32), bfir.ERR_UNSUPPORTED), ((512,) + lv + (4, 9, 9, F32, F32BE), bfir.ERR_UNSUPPORTED)]
    for args, want in cases:
        h, err = _create(lib, *args)
        assert not h and err == want, (args, err)
    err = C.c_int(0)
    assert not getattr(lib, NAME)(512, 3, None, None, 4, 9, 9, F32, F32, 0, C.byref(err)) and err.value == bfir.ERR_ARG
    if lib.bfir_device_count() == 0:
        for args in ((256, (4, 3, 15), (1, 4, 4), 4, 64, 64), (16, (2, 2, 3), (1, 2, 2), 4, 9, 3),
                     (64, (2, 2), (1, 2), 8, 9, 2, F32, F32), (64, (2, 2), (1, 2), 8, 9, 2, F64, F64)):
            h, err = _create(lib, *args)
            assert not h and err == bfir.ERR_NO_DEVICE, (args, err)
        with pytest.raises(bfir.BfirError) as ei:
            bfir.BrutefirMimoLevels(512, (4, 2, 2), (1, 4, 2), 4, 10, 12)
        assert ei.value.code == bfir.ERR_NO_DEVICE
    # the multi-level matrix engine keeps its own limit
    err = C.c_int(0)
    b, r = (C.c_int * 3)(4, 2, 2), (C.c_int * 3)(1, 4, 2)
    assert not lib.bfir_engine_create_matrix_levels(512, 3, b, r, 4, 9, 2, F32, F32, 0, C.byref(err)) and err.value == bfir.ERR_ARG
    assert lib.bfir_engine_set_coeff_matrix_levels(None, None, None, 1.0) == bfir.ERR_ARG


@pytest.mark.parametrize("s", [4, 8])
def test_cpu_model_past_eight_inputs_agrees_with_the_uniform_reference(orc, s):
    """10 -> 3 on three levels, ragged lengths that end on every level and one NULL pair: the sum over the inputs of the
    levels model of every pair against one uniform oracle engine per output and group of 8 inputs (wide_reference), the
    reference of test_mimo_levels_gpu.py."""
    L, blocks, ratios, n_in, n_out = 16, (2, 2, 3), (1, 2, 2), 10, 3
    Ls, D = level_geometry(L, blocks, ratios)
    dt = np.float64 if s == 8 else np.float32
    rng = np.random.default_rng(97 + s)
    ends = [D[1] - 5, D[2] - 9, D[3] - Ls[2] + Ls[2] // 3 + 1, D[1] + 3]
    lens = [[ends[(o + 2 * i) % 4] - (o + i) % 3 for i in range(n_in)] for o in range(n_out)]
    lens[1][8] = None
    flat = [n for r in lens for n in r if n is not None]
    assert all(any(D[k] < n <= D[k + 1] for n in flat) for k in range(3))
    rows = [[None if n is None else orc.synth_ir(rng, 1, n, dt)[0] for n in r] for r in lens]
    nb = D[2] // L + (Ls[2] // L) * (blocks[2] + 2) + 3
    x = orc.synth_audio(rng, nb * L, n_in, dt)
    y = mlevels_model(orc, L, blocks, ratios, s, rows, x)
    want = wide_reference(orc, L, s, rows, x)
    print("rel_err", s, rel_err(y, want))
    assert rel_err(y, want) <= TOL[s]


# k_wduo<T, ILV, NO, TT> as DESIGN.md ("k_wduo", the register table) lists them, with the waves per SIMD stated there:
# float: pairs / groups x 1, 2 outputs x the one-block form and 8-block tiles; double: one output x one block and 4-block tiles
WDUO_INSTANCES = {
    ("f", 0, 1, 1): 8, ("f", 0, 2, 1): 8, ("f", 1, 1, 1): 8, ("f", 1, 2, 1): 8,
    ("f", 0, 1, 8): 7, ("f", 0, 2, 8): 4, ("f", 1, 1, 8): 5, ("f", 1, 2, 8): 4,
    ("d", 0, 1, 1): 8, ("d", 1, 1, 1): 8, ("d", 0, 1, 4): 6, ("d", 1, 1, 4): 5,
}


def test_wduo_register_budget():
    """The k_wduo instances are exactly those of DESIGN.md's table, with its registers and waves per SIMD (at least 4);
    none has scratch, a spill, a dynamic stack or LDS.  The counted names of the other kernels stay what they were."""
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc on this machine")
    import importlib
    import sys
    sys.path.insert(0, ROOT)
    b = importlib.import_module("foo_dsp_bfir_amd._build")
    assert "wduo.hip" in b.SOURCES
    b.build()
    u = b.resource_usage()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    got = {}
    for name, r in u.items():
        if "k_wduo" not in name:
            continue
        m = re.search(r"k_wduoI([fd])Lb([01])ELi(\d+)ELi(\d+)E", name)
        assert m, name
        for other in ("k_mac_mimo", "k_mac_matrix", "k_mac_duo", "k_inv_", "k_delay_"):
            assert other not in name, name
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["Dynamic Stack"] == "False", (name, r)
        assert r["LDS Size"] == 0 and r["Occupancy"] >= 4, (name, r)
        key = (m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)))
        got[key] = r["Occupancy"]
        row = r"\|\s*%s\s*\|\s*%s\s*\|\s*%d\s*\|\s*%d\s*\|\s*%d\s*\|\s*%d\s*\|" % (
            "float" if key[0] == "f" else "double", "pairs" if key[1] else "groups", key[2], key[3], r["VGPRs"], r["Occupancy"])
        assert re.search(row, design), (key, r["VGPRs"], r["Occupancy"])
    assert got == WDUO_INSTANCES, sorted(set(got.items()) ^ set(WDUO_INSTANCES.items()))
    assert sum("k_mac_matrix" in k for k in u) == 20 and sum("k_mac_duo" in k for k in u) == 12
    assert sum("k_mac_mimo" in k for k in u) == 20
    assert sum("k_inv_lfade" in k for k in u) == 15 and sum("k_inv_lone" in k for k in u) == 20


def test_cpp_mirror_compiles_with_plain_gxx():
    if not shutil.which("g++"):
        pytest.skip("no g++ on this machine")
    src = os.path.join(ROOT, "tests", "cpp", "test_mimo_levels_mirror.cpp")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", src], check=True)
