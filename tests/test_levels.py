"""Multi-level partitioned engines (bfir_engine_create_levels) without a GPU: the C ABI as declared and exported, its
argument checks, the definition the GPU tests rely on (one uniform oracle engine per level composed against one), and the
register report of the back-end kernels of csrc/levels.hip."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import TOL, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bfir_hip.h")
LEVELS_FNS = ("bfir_engine_create_levels", "bfir_engine_set_coeff_levels", "bfir_engine_read_coeff_levels")
F32, F64, S16 = 8, 10, 2

# The compiler's occupancy (waves per SIMD by registers) per k_inv_levels instance, by log2 of its N = 2L points -- the same
# for two and three rings -- and the LDS footprint that bounds the workgroups per CU, as DESIGN.md "k_inv_levels" lists them.
LEVELS_OCCUPANCY = {10: 5, 11: 5, 12: 4, 13: 4, 14: 4}
LEVELS_LDS_BYTES = {10: 8464, 11: 16928, 12: 33856, 13: 67712, 14: 135424}


def level_geometry(L, blocks, ratios):
    """([L_k], [D_k] with D_n = capacity appended)."""
    Ls, D = [], [0]
    for b, r in zip(blocks, ratios):
        Ls.append(L if not Ls else Ls[-1] * r)
        D.append(D[-1] + b * Ls[-1])
    return Ls, D


def levels_model(orc, L, blocks, ratios, s, Cn, h, x, in_fmt=None, out_fmt=None):
    """((y_0 + z_1[n - D_1]) + z_2[n - D_2]) + z_3[n - D_3] from one uniform oracle engine per level: level k is
    Engine(L_k, blocks[k]) on h[D_k : D_k+1] run in blocks of L_k from sample 0 (the input zero-padded to whole blocks).
    float64 [frames, C]."""
    Ls, D = level_geometry(L, blocks, ratios)
    dt = np.float64 if s == 8 else np.float32
    n = x.shape[0]
    y = None
    for k, (Lk, Bk) in enumerate(zip(Ls, blocks)):
        if k > 0 and h[0].size <= D[k]:
            break
        eng = orc.Engine(Lk, Bk, s, Cn, in_fmt, out_fmt)
        assert eng.set_coeff([np.ascontiguousarray(c[D[k]:D[k + 1]], dtype=dt) for c in h]) == 0
        xp = np.zeros((-(-n // Lk) * Lk, Cn), x.dtype)
        xp[:n] = x
        rc, z = eng.run(xp)
        assert rc == 0
        eng.close()
        z = np.asarray(z, dtype=np.float64)
        if k == 0:
            y = z[:n].copy()
        elif n > D[k]:
            y[D[k]:] += z[:n - D[k]]
    return y


def _decl(name):
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, open(HEADER).read(), re.S)
    assert m, name
    return m.group(1)


@pytest.mark.parametrize("name", LEVELS_FNS)
def test_header_declares_the_levels_functions(name):
    args = _decl(name)
    assert not re.search(r"\blong\b", args), args
    for a in args.split(","):
        assert re.match(r"\s*(const\s+)?(int|double|void|bfir_engine)\b", a), a
    assert re.search(r"#define\s+BFIR_MAX_LEVELS\s+4\b", open(HEADER).read())


def test_library_exports_and_bindings(bfir):
    from foo_dsp_bfir_amd import _lib
    lib = bfir.load()
    for name in LEVELS_FNS:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).restype == _lib.SIGNATURES[name][0]
    if shutil.which("nm"):
        syms = subprocess.run(["nm", "-D", "--defined-only", bfir.library_path()], capture_output=True, text=True).stdout
        for name in LEVELS_FNS:
            assert re.search(r"\bT %s$" % name, syms, re.M), name
    assert issubclass(bfir.BrutefirLevels, bfir.Brutefir) and not issubclass(bfir.BrutefirLevels, bfir.BrutefirNup)
    assert bfir.BrutefirLevels.set_coeff is not bfir.Brutefir.set_coeff
    assert bfir.BrutefirLevels.coeff_block is not bfir.Brutefir.coeff_block


def _create(lib, L, blocks, ratios, s, Cn, fi=F32, fo=F32, n=None):
    err = C.c_int(12345)
    n = len(blocks) if n is None else n
    b = (C.c_int * max(1, len(blocks)))(*blocks) if blocks is not None else None
    r = (C.c_int * max(1, len(ratios)))(*ratios) if ratios is not None else None
    h = lib.bfir_engine_create_levels(L, n, b, r, s, Cn, fi, fo, 0, C.byref(err))
    return h, err.value


@pytest.mark.parametrize("args", [
    (1024, (8,), (1,), 4, 2),                        # n_levels outside 2 .. 4
    (64, (2, 2, 2, 2, 2), (1, 2, 2, 2, 2), 4, 2),
    (1024, (8, 2, 2), (2, 2, 2), 4, 2),              # ratios[0] != 1
    (1024, (8, 2, 2), (1, 3, 2), 4, 2),              # a ratio that is not a power of two
    (1024, (8, 2, 2), (1, 2, 1), 4, 2),              # ... or below 2
    (1024, (8, 2, 2), (1, 2, 0), 4, 2),
    (1024, (8, 2, 2), (1, -2, 2), 4, 2),
    (1024, (8, 0, 2), (1, 2, 2), 4, 2),              # a level without partitions
    (1024, (0, 2, 2), (1, 2, 2), 4, 2),
    (1024, (3, 2, 2), (1, 4, 2), 4, 2),              # D_1 = 3 L < L_1 = 4 L
    (1024, (4, 1, 2), (1, 4, 4), 4, 2),              # D_2 = 8 L < L_2 = 16 L
    (64, (2, 1, 1, 1), (1, 2, 2, 4), 4, 2),          # D_3 = 8 L < L_3 = 16 L
    (1024, (8, 2, 2), (1, 2, 2), 4, 0),              # channels
    (1024, (8, 2, 2), (1, 2, 2), 4, 9),
    (1024, (8, 2, 2), (1, 2, 2), 2, 2),              # realsize
    (1000, (8, 2, 2), (1, 2, 2), 4, 2),              # not a power of two
    (1024, (1 << 20, 2, 2), (1, 1 << 30, 1 << 30), 4, 2),   # D_2 < L_2, far outside every size
], ids=lambda a: "-".join(map(str, a)))
def test_argument_refusals(bfir, args):
    h, err = _create(bfir.load(), *args)
    assert not h and err == bfir.ERR_ARG


def test_null_arrays_are_argument_errors(bfir):
    lib = bfir.load()
    for blocks, ratios in [(None, (1, 2, 2)), ((8, 2, 2), None), (None, None)]:
        h, err = _create(lib, 1024, blocks, ratios, 4, 2, n=3)
        assert not h and err == bfir.ERR_ARG


@pytest.mark.parametrize("args", [
    (8, (4, 2, 2), (1, 2, 2), 4, 2, F32, F32),              # L_0 below what bfir_engine_create takes
    (32768, (4, 2, 2), (1, 2, 2), 4, 2, F32, F32),          # L_0 above
    (4096, (4, 2, 2), (1, 4, 2), 4, 2, F32, F32),           # L_2 = 32768 above
    (1024, (8, 4, 2), (1, 4, 4), 8, 2, F64, F64),           # fp64: L_2 = 16384 above
    (512, (8, 4, 4, 2), (1, 4, 4, 4), 4, 2, F32, F32),      # four levels: L_3 = 32768
    (1024, (8, 2, 2), (1, 2, 2), 4, 2, S16, F32),           # frame formats
    (1024, (8, 2, 2), (1, 2, 2), 4, 2, F32, S16),
    (1024, (8, 2, 2), (1, 2, 2), 4, 2, 9, F32),             # FLOAT_BE
], ids=lambda a: "-".join(map(str, a)))
def test_unsupported_sizes_and_formats(bfir, args):
    h, err = _create(bfir.load(), *args)
    assert not h and err == bfir.ERR_UNSUPPORTED


def test_valid_arguments_reach_the_device_check(bfir):
    lib = bfir.load()
    for args in [(512, (4, 3, 15), (1, 4, 4), 4, 8, F32, F32), (16, (2, 2, 3), (1, 2, 2), 4, 1, F32, F32),
                 (64, (8, 8, 2, 15), (1, 8, 8, 2), 4, 2, F32, F64), (1024, (8, 2, 2), (1, 4, 2), 8, 3, F64, F64),
                 (1024, (8, 8), (1, 8), 8, 2, F32, F32)]:
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
    assert lib.bfir_engine_set_coeff_levels(None, ptrs, 1, 4, 1.0) == bfir.ERR_ARG
    assert lib.bfir_engine_read_coeff_levels(None, 0, 0, 0, taps.ctypes.data) == bfir.ERR_ARG


def test_python_mirror_geometry_and_refusal_without_a_device(bfir):
    try:
        eng = bfir.BrutefirLevels(512, (3, 2, 2), (1, 4, 2), 4, 2)       # D_1 < L_1: refused before the device
    except bfir.BfirError as ex:
        assert ex.code == bfir.ERR_ARG
    else:
        eng.close()
        raise AssertionError("D_1 < L_1 was accepted")
    _, D = level_geometry(512, (5, 3, 2), (1, 4, 2))
    assert D == [0, 2560, 8704, 16896]


def test_cpp_mirror_with_a_multi_level_caller_compiles(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++ on this machine")
    src = tmp_path / "caller.cpp"
    src.write_text('#include "%s"\n'
                   "int three(void **h) { brutefir f(512, brutefir::multi_level{3, {4, 3, 15}, {1, 4, 4}}, 4, 8, 8, 8);\n"
                   "                      return f.set_coeff_levels(h, 8, 131072, 1.0); }\n"
                   % os.path.join(ROOT, "foo-dsp-bfir_amd", "host", "brutefir_hip.hpp"))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", str(src)], check=True)


# (s, L, blocks, ratios, C)
MODEL_SHAPES = [
    (4, 16, (2, 2, 3), (1, 2, 2), 1),                # three levels, fp32; D_1 = L_1
    (8, 64, (4, 3, 5), (1, 2, 2), 3),                # three levels, fp64
    (4, 16, (2, 2, 2, 2), (1, 2, 2, 2), 2),          # four levels
    (8, 32, (4, 2, 3), (1, 4, 2), 2),                # D_1 = L_1 = 4 L
    (4, 16, (3, 3, 2), (1, 2, 2), 2),                # D_1 = 3 L, D_2 = 9 L: no D_k is a multiple of L_k = 2 L, 4 L
]


@pytest.mark.parametrize("shape", MODEL_SHAPES, ids=lambda a: "-".join(map(str, a)))
def test_levels_compose_to_the_uniform_engine(orc, shape):
    """One oracle engine per level, delayed by D_k and added in level order, equals the uniform oracle
    (L, ceil(taps / L)) and the direct convolution: the definition the GPU tests hold the engine to."""
    s, L, blocks, ratios, Cn = shape
    dt = np.float64 if s == 8 else np.float32
    Ls, D = level_geometry(L, blocks, ratios)
    for k in range(1, len(Ls)):
        assert D[k] >= Ls[k]
    if shape == MODEL_SHAPES[3]:
        assert D[1] == Ls[1]
    if shape == MODEL_SHAPES[4]:
        assert all(D[k] % Ls[k] for k in range(1, len(Ls)))
    taps = D[-2] + (blocks[-1] - 1) * Ls[-1] + Ls[-1] // 3 + 1          # ends inside the last partition of the last level
    nb = D[-2] // L + (Ls[-1] // L) * (blocks[-1] + 2) + 3
    rng = np.random.default_rng(sum(blocks) + L + Cn)
    h = orc.synth_ir(rng, Cn, taps, dt)
    x = orc.synth_audio(rng, nb * L, Cn, dt)
    uni = orc.Engine(L, -(-taps // L), s, Cn)
    assert uni.set_coeff(h) == 0
    rc, want = uni.run(x)
    assert rc == 0
    uni.close()
    y = levels_model(orc, L, blocks, ratios, s, Cn, h, x)
    assert rel_err(y, want) <= TOL[s]
    direct = np.stack([orc.direct_conv(x[:, c].astype(np.float64), np.asarray(h[c], np.float64)) for c in range(Cn)], axis=1)
    assert rel_err(y, direct) <= TOL[s]
    # filters that end 3 taps short of D_2: the model is the first two levels alone
    y2 = levels_model(orc, L, blocks, ratios, s, Cn, [c[:D[2] - 3] for c in h], x)
    assert rel_err(y2, np.stack([orc.direct_conv(x[:, c].astype(np.float64), np.asarray(h[c][:D[2] - 3], np.float64))
                                 for c in range(Cn)], axis=1)) <= TOL[s]


def test_levels_kernel_register_report():
    """Every k_inv_levels / k_levels_combine instance: no scratch, no spill, no dynamic stack, LDS within 160 KB; two
    k_inv_levels (two and three rings) per pair plan size, each at 4 or more waves per SIMD; occupancy, registers and LDS
    as DESIGN.md records them, so a later regression shows.  The names stay clear of the two-level kernels' (test_nup.py
    counts those by substring)."""
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc on this machine")
    import importlib
    import sys
    sys.path.insert(0, ROOT)
    b = importlib.import_module("foo_dsp_bfir_amd._build")
    assert "levels.hip" in b.SOURCES
    b.build()
    u = b.resource_usage()
    inv = {k: v for k, v in u.items() if "k_inv_levels" in k}
    comb = {k: v for k, v in u.items() if "k_levels_combine" in k}
    assert len(inv) == 10, sorted(inv)
    assert len(comb) == 4, sorted(comb)                      # float / double x 16 bytes per lane / one sample per lane
    for name, r in list(inv.items()) + list(comb.items()):
        assert "k_inv_nup" not in name and "k_nup_combine" not in name
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["Dynamic Stack"] == "False", (name, r)
        assert r["LDS Size"] <= 160 * 1024, (name, r)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    seen = set()
    for name, r in inv.items():
        m = re.search(r"k_inv_levelsILi(\d+)ELi(\d+)E", name)
        lg, nr = int(m.group(1)), int(m.group(2))
        seen.add((lg, nr))
        assert r["Occupancy"] >= 4, (name, r)
        assert r["Occupancy"] == LEVELS_OCCUPANCY[lg] and r["LDS Size"] == LEVELS_LDS_BYTES[lg], (name, r)
        assert re.search(r"\|\s*%d\s*\|\s*%d\s*\|\s*%d\s*\|\s*%d\s*\|\s*%d\s*\|"
                         % (1 << lg, nr, r["VGPRs"], LEVELS_LDS_BYTES[lg], LEVELS_OCCUPANCY[lg]), design), (lg, nr)
    assert seen == {(lg, nr) for lg in LEVELS_OCCUPANCY for nr in (2, 3)}
    for r in comb.values():
        assert r["Occupancy"] == 8 and r["LDS Size"] == 0, r
