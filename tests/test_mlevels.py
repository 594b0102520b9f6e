"""Multi-level matrix engines (bfir_engine_create_matrix_levels) without a GPU: the C ABI as declared and exported, its
argument checks, the definition the GPU tests rely on (one levels model per (output, input) pair, summed over the inputs,
against one uniform oracle engine per output) and the register report of csrc/mlevels.hip."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import TOL, rel_err
from test_levels import level_geometry, levels_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bfir_hip.h")
MLEVELS_FNS = ("bfir_engine_create_matrix_levels", "bfir_engine_set_coeff_matrix_levels",
               "bfir_engine_read_coeff_matrix_levels")
F32, F64, S16 = 8, 10, 2


def pad_rows(rows, dt):
    """rows with every filter zero-padded to the longest one (None stays None), and that length."""
    taps = max(h.size for r in rows for h in r if h is not None)
    out = []
    for r in rows:
        out.append([None if h is None else np.concatenate([np.asarray(h, dt), np.zeros(taps - h.size, dt)]) for h in r])
    return out, taps


def mlevels_model(orc, L, blocks, ratios, s, rows, x):
    """y[:, o] = sum over the inputs of test_levels.levels_model of the pair (o, i): float64 [frames, n_out]."""
    y = np.zeros((x.shape[0], len(rows)), np.float64)
    for o, row in enumerate(rows):
        for i, h in enumerate(row):
            if h is not None:
                y[:, o] += levels_model(orc, L, blocks, ratios, s, 1, [h], np.ascontiguousarray(x[:, i:i + 1]))[:, 0]
    return y


def uniform_reference(orc, L, s, rows, x):
    """The RefMatrix construction of test_matrix_gpu.py: one uniform orc.Engine(L, ceil(max taps / L), s, n_in) per output
    with that output's row of filters (zero-padded to the longest, NULL = zeros), summed over the inputs in float64."""
    from test_matrix_gpu import RefMatrix
    dt = np.float64 if s == 8 else np.float32
    padded, taps = pad_rows(rows, dt)
    ref = RefMatrix(orc, L, -(-taps // L), s, x.shape[1], len(rows))
    ref.set_coeff(padded)
    y = ref.run(x)
    for e in ref.engines:
        e.close()
    return y


def _decl(name):
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, open(HEADER).read(), re.S)
    assert m, name
    return m.group(1)


@pytest.mark.parametrize("name", MLEVELS_FNS)
def test_header_declares_the_functions(name):
    args = _decl(name)
    assert not re.search(r"\blong\b", args), args
    for a in args.split(","):
        assert re.match(r"\s*(const\s+)?(int|double|void|bfir_engine)\b", a), a


def test_library_exports_and_bindings(bfir):
    from foo_dsp_bfir_amd import _lib
    lib = bfir.load()
    for name in MLEVELS_FNS:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).restype == _lib.SIGNATURES[name][0]
    if shutil.which("nm"):
        syms = subprocess.run(["nm", "-D", "--defined-only", bfir.library_path()], capture_output=True, text=True).stdout
        for name in MLEVELS_FNS:
            assert re.search(r"\bT %s$" % name, syms, re.M), name
    assert "BrutefirMatrixLevels" in bfir.__all__
    assert issubclass(bfir.BrutefirMatrixLevels, bfir.BrutefirMatrix)
    assert bfir.BrutefirMatrixLevels.set_coeff is not bfir.BrutefirMatrix.set_coeff
    assert bfir.BrutefirMatrixLevels.coeff_block is not bfir.BrutefirMatrix.coeff_block


def _create(lib, L, blocks, ratios, s, n_in, n_out, fi=F32, fo=F32, n=None):
    err = C.c_int(12345)
    n = len(blocks) if n is None else n
    b = (C.c_int * max(1, len(blocks)))(*blocks) if blocks is not None else None
    r = (C.c_int * max(1, len(ratios)))(*ratios) if ratios is not None else None
    h = lib.bfir_engine_create_matrix_levels(L, n, b, r, s, n_in, n_out, fi, fo, 0, C.byref(err))
    return h, err.value


@pytest.mark.parametrize("args", [
    (1024, (8,), (1,), 4, 2, 2),                        # n_levels outside 2 .. 4
    (64, (2, 2, 2, 2, 2), (1, 2, 2, 2, 2), 4, 2, 2),
    (1024, (8, 2, 2), (2, 2, 2), 4, 2, 2),              # ratios[0] != 1
    (1024, (8, 2, 2), (1, 3, 2), 4, 2, 2),              # a ratio that is not a power of two
    (1024, (8, 2, 2), (1, 2, 1), 4, 2, 2),              # ... or below 2
    (1024, (8, 2, 2), (1, 2, 0), 4, 2, 2),
    (1024, (8, 2, 2), (1, -2, 2), 4, 2, 2),
    (1024, (8, 0, 2), (1, 2, 2), 4, 2, 2),              # a level without partitions
    (1024, (0, 2, 2), (1, 2, 2), 4, 2, 2),
    (1024, (3, 2, 2), (1, 4, 2), 4, 2, 2),              # D_1 = 3 L < L_1 = 4 L
    (1024, (4, 1, 2), (1, 4, 4), 4, 2, 2),              # D_2 = 8 L < L_2 = 16 L
    (64, (2, 1, 1, 1), (1, 2, 2, 4), 4, 2, 2),          # D_3 = 8 L < L_3 = 16 L
    (1024, (3, 2), (1, 4), 4, 2, 2),                    # two levels: head_blocks < tail_ratio
    (1024, (8, 2, 2), (1, 2, 2), 4, 0, 2),              # the matrix channel limits, either side
    (1024, (8, 2, 2), (1, 2, 2), 4, 9, 2),
    (1024, (8, 2, 2), (1, 2, 2), 4, 2, 0),
    (1024, (8, 2, 2), (1, 2, 2), 4, 2, 9),
    (1024, (8, 2, 2), (1, 2, 2), 2, 2, 2),              # realsize
    (1000, (8, 2, 2), (1, 2, 2), 4, 2, 2),              # not a power of two
    (1024, (1 << 20, 2, 2), (1, 1 << 30, 1 << 30), 4, 2, 2),   # D_2 < L_2, far outside every size
], ids=lambda a: "-".join(map(str, a)))
def test_argument_refusals(bfir, args):
    h, err = _create(bfir.load(), *args)
    assert not h and err == bfir.ERR_ARG


def test_null_arrays_are_argument_errors(bfir):
    lib = bfir.load()
    for blocks, ratios in [(None, (1, 2, 2)), ((8, 2, 2), None), (None, None)]:
        h, err = _create(lib, 1024, blocks, ratios, 4, 2, 3, n=3)
        assert not h and err == bfir.ERR_ARG


@pytest.mark.parametrize("args", [
    (8, (4, 2, 2), (1, 2, 2), 4, 2, 3, F32, F32),              # L_0 below what bfir_engine_create takes
    (32768, (4, 2, 2), (1, 2, 2), 4, 2, 3, F32, F32),          # L_0 above
    (4096, (4, 2, 2), (1, 4, 2), 4, 2, 3, F32, F32),           # L_2 = 32768 above
    (1024, (8, 4, 2), (1, 4, 4), 8, 2, 3, F64, F64),           # fp64: L_2 = 16384 above
    (512, (8, 4, 4, 2), (1, 4, 4, 4), 4, 2, 3, F32, F32),      # four levels: L_3 = 32768
    (1024, (8, 2, 2), (1, 2, 2), 4, 2, 3, S16, F32),           # frame formats
    (1024, (8, 2, 2), (1, 2, 2), 4, 2, 3, F32, S16),
    (1024, (8, 2, 2), (1, 2, 2), 4, 2, 3, 9, F32),             # FLOAT_BE
], ids=lambda a: "-".join(map(str, a)))
def test_unsupported_sizes_and_formats(bfir, args):
    h, err = _create(bfir.load(), *args)
    assert not h and err == bfir.ERR_UNSUPPORTED


def test_valid_arguments_reach_the_device_check(bfir):
    lib = bfir.load()
    for args in [(512, (4, 3, 15), (1, 4, 4), 4, 2, 3, F32, F32), (16, (2, 2, 3), (1, 2, 2), 4, 1, 8, F32, F32),
                 (64, (8, 8, 2, 15), (1, 8, 8, 2), 4, 8, 1, F32, F64), (1024, (8, 2, 2), (1, 4, 2), 8, 3, 3, F64, F64),
                 (1024, (8, 8), (1, 8), 8, 2, 2, F32, F32)]:
        h, err = _create(lib, *args)
        if lib.bfir_device_count() == 0:
            assert not h and err == bfir.ERR_NO_DEVICE, args
        else:
            assert h and err == 0, args
            lib.bfir_engine_destroy(h)


def test_null_engine_is_an_argument_error_without_a_device(bfir):
    lib = bfir.load()
    taps = np.zeros(4, np.float32)
    ptrs = (C.c_void_p * 1)(taps.ctypes.data)
    lens = (C.c_int * 1)(4)
    assert lib.bfir_engine_set_coeff_matrix_levels(None, ptrs, lens, 1.0) == bfir.ERR_ARG
    assert lib.bfir_engine_read_coeff_matrix_levels(None, 0, 0, 0, 0, taps.ctypes.data) == bfir.ERR_ARG


def test_python_mirror_geometry_and_refusal_without_a_device(bfir):
    try:
        eng = bfir.BrutefirMatrixLevels(512, (3, 2, 2), (1, 4, 2), 4, 2, 3)   # D_1 < L_1: refused before the device
    except bfir.BfirError as ex:
        assert ex.code == bfir.ERR_ARG
    else:
        eng.close()
        raise AssertionError("D_1 < L_1 was accepted")
    Ls, D = level_geometry(512, (5, 3, 2), (1, 4, 2))
    assert bfir.BrutefirMatrixLevels.geometry(512, (5, 3, 2), (1, 4, 2)) == (Ls, D[:-1], D[-1])
    assert D == [0, 2560, 8704, 16896]
    try:
        eng = bfir.BrutefirMatrixLevels(512, (5, 3, 2), (1, 4, 2), 4, 2, 3)
    except bfir.BfirError as ex:
        assert ex.code == bfir.ERR_NO_DEVICE                              # valid: only the device is missing
        return
    assert eng.lengths == Ls and eng.D == D[:-1] and eng.max_taps == D[-1]
    assert (eng.n_in, eng.n_out, eng.blocks, eng.ratios) == (2, 3, (5, 3, 2), (1, 4, 2))
    for call in (lambda: eng.set_coeff_fade([[None] * 2] * 3, 3), lambda: eng.fade_to([[None] * 2] * 3, 3)):
        with pytest.raises(bfir.BfirError) as ei:
            call()
        assert ei.value.code == bfir.ERR_UNSUPPORTED
    eng.close()


def test_cpp_mirror_compiles_with_plain_gxx():
    if not shutil.which("g++"):
        pytest.skip("no g++ on this machine")
    src = os.path.join(ROOT, "tests", "cpp", "test_mlevels_mirror.cpp")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", src], check=True)


@pytest.mark.parametrize("s", [4, 8])
def test_definition_levels_per_pair_equal_the_uniform_matrix_reference(orc, s):
    """2 -> 3 on three levels, two NULL pairs, filters that end in level 0, 1 and 2: the sum over the inputs of the levels
    model of every pair equals one uniform oracle engine per output -- the reference of tests/test_mlevels_gpu.py."""
    L, blocks, ratios = 16, (2, 2, 3), (1, 2, 2)
    Ls, D = level_geometry(L, blocks, ratios)
    dt = np.float64 if s == 8 else np.float32
    rng = np.random.default_rng(31 + s)
    lens = [[D[1] - 5, D[3] - Ls[2] + Ls[2] // 3 + 1],                     # level 0 | inside the last partition of level 2
            [None, D[2] - 9],                                              # NULL | level 1
            [D[1] + 3, None]]                                              # level 1, three taps past D_1 | NULL
    assert lens[0][0] <= D[1] < lens[2][0] <= D[2] and D[1] < lens[1][1] <= D[2] < lens[0][1] <= D[3]
    rows = [[None if n is None else orc.synth_ir(rng, 1, n, dt)[0] for n in r] for r in lens]
    nb = D[2] // L + (Ls[2] // L) * (blocks[2] + 2) + 3
    x = orc.synth_audio(rng, nb * L, 2, dt)
    y = mlevels_model(orc, L, blocks, ratios, s, rows, x)
    want = uniform_reference(orc, L, s, rows, x)
    print("rel_err", s, rel_err(y, want))
    assert rel_err(y, want) <= TOL[s]
    direct = np.zeros_like(want)
    for o, row in enumerate(rows):
        for i, h in enumerate(row):
            if h is not None:
                direct[:, o] += orc.direct_conv(x[:, i].astype(np.float64), np.asarray(h, np.float64))
    assert rel_err(want, direct) <= TOL[s]


def test_lone_kernel_register_report():
    """Every k_inv_lone instance (five plan sizes x no ring to three rings): no scratch, no spill, at least the 4 waves per
    SIMD that are k_inv_nup's lowest, LDS no larger than the k_inv_levels instance of the same N, and the numbers DESIGN.md
    records."""
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc on this machine")
    import importlib
    import sys
    sys.path.insert(0, ROOT)
    b = importlib.import_module("foo_dsp_bfir_amd._build")
    assert "mlevels.hip" in b.SOURCES
    b.build()
    u = b.resource_usage()
    lone = {k: v for k, v in u.items() if "k_inv_lone" in k}
    assert len(lone) == 20, sorted(lone)
    levels_lds = {}
    for name, r in u.items():
        m = re.search(r"k_inv_levelsILi(\d+)ELi(\d+)E", name)
        if m:
            levels_lds[int(m.group(1))] = r["LDS Size"]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    seen = set()
    for name, r in lone.items():
        m = re.search(r"k_inv_loneILi(\d+)ELi(\d+)E", name)
        lg, nr = int(m.group(1)), int(m.group(2))
        seen.add((lg, nr))
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["Dynamic Stack"] == "False", (name, r)
        assert r["Occupancy"] >= 4, (name, r)
        assert r["LDS Size"] <= levels_lds[lg], (name, r, levels_lds[lg])
        assert re.search(r"\|\s*%d\s*\|\s*%d\s*\|\s*%d\s*\|\s*%d\s*\|\s*%d\s*\|"
                         % (1 << lg, nr, r["VGPRs"], r["LDS Size"], r["Occupancy"]), design), (lg, nr, r)
    assert seen == {(lg, nr) for lg in (10, 11, 12, 13, 14) for nr in (0, 1, 2, 3)}
