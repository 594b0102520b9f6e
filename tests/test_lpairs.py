"""Pair-list coefficient updates on multi-level matrix and mimo engines (bfir_engine_set_coeff_matrix_levels_pairs,
_pairs_fade) without a GPU: the two calls as declared, exported and bound, the refusal that needs no device, the C++ mirror's
two methods under -Wall -Werror, the register report of k_wpatch (csrc/wpatch.hip), and the shapes, lists and fade
geometry of tests/test_lpairs_gpu.py, held here to the conditions its cases must meet.

The lists.  Every list of every shape holds pair A = (0, 0), which has partitions on every level in both sets.  The list
`mixed` of every shape holds, beside A, one added path, one removed path, one filter that grows into a further level
(already active) and one that shrinks out of its last level; `column`, `single` and `row` cannot hold five pairs at every
shape (single holds one, a column of three outputs three), so the four kinds are asked of `mixed` alone."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_levels import level_geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bfir_hip.h")
NAMES = ("bfir_engine_set_coeff_matrix_levels_pairs", "bfir_engine_set_coeff_matrix_levels_pairs_fade")

LV3 = ((4, 2, 2), (1, 4, 2))                                             # at L = 512: 4 x 512, 2 x 2048, 2 x 4096
# id: (class, (realsize, L, blocks, ratios, n_in, n_out), K)
SHAPES = {
    "9x3": ("BrutefirMimoLevels", (4, 16, (2, 2, 3), (1, 2, 2), 9, 3), 5),        # grouped layout, general back end
    "9x10": ("BrutefirMimoLevels", (4, 512) + LV3 + (9, 10), 11),                 # (re, im) pairs, k_inv_lfade
    "9x2-f64": ("BrutefirMimoLevels", (8, 64, (2, 2), (1, 2), 9, 2), 5),          # fp64
    "m3x2": ("BrutefirMatrixLevels", (4, 16, (2, 2, 3), (1, 2, 2), 3, 2), 5),     # k_mac_matrix on every level
}
LISTS = ("column", "single", "row", "mixed")
A_F = 11                                                                 # the head block the change is made at


def geo(shape):
    """([L_k], [D_k] with the capacity appended, [r_k = L_k / L_0])."""
    Ls, D = level_geometry(shape[1], shape[2], shape[3])
    return Ls, D, [Lk // shape[1] for Lk in Ls]


def special(shape):
    """The pairs the lists are built around."""
    n_in, n_out = shape[4], shape[5]
    return dict(A=(0, 0), ADD=(0, n_in - 1), REM=(1, 1), GROW=(n_out - 1, 0), SHRINK=(0, 1))


def old_lengths(shape):
    """Tap counts of the first set, [o][i] (None: no path).  A, REM and SHRINK reach into the last partition of the last level,
    GROW ends in the head, ADD has no path; every other filter ends on level (o + i) mod n, in turn inside the last and the
    first partition of that level, a few taps apart."""
    s, L, blocks, ratios, n_in, n_out = shape
    Ls, D, _ = geo(shape)
    n = len(blocks)
    sp = special(shape)
    fixed = {sp["A"]: D[-1] - 1, sp["ADD"]: None, sp["REM"]: D[-1] - 9, sp["GROW"]: D[1] - 5, sp["SHRINK"]: D[-1] - 7}
    lens = []
    for o in range(n_out):
        row = []
        for i in range(n_in):
            if (o, i) in fixed:
                row.append(fixed[(o, i)])
                continue
            k = (o + i) % n
            last = blocks[k] - 1 if ((o + i) // n) % 2 == 0 else 0
            row.append(D[k] + last * Ls[k] + Ls[k] // 3 + 1 - (o * n_in + i) % 3)
        lens.append(row)
    return lens


def pair_list(shape, kind):
    """(pairs, new tap counts) of a list; None: the path is removed.  Pairs are listed out of input order where there is an
    order to break.  A pair that is none of the five special ones keeps its length and gets other taps."""
    s, L, blocks, ratios, n_in, n_out = shape
    Ls, D, _ = geo(shape)
    n = len(blocks)
    sp = special(shape)
    old = old_lengths(shape)
    new = {sp["A"]: D[-1] - 4, sp["ADD"]: D[1] + Ls[1] // 2, sp["REM"]: None, sp["GROW"]: D[1] + Ls[1] // 3,
           sp["SHRINK"]: D[n - 1] - 3}
    if kind == "column":
        pairs = [(o, 0) for o in range(n_out)]
    elif kind == "single":
        pairs = [sp["A"]]
    elif kind == "row":
        pairs = [(0, i) for i in range(min(3, n_in))][::-1]
    elif kind == "mixed":
        pairs = [sp["SHRINK"], sp["A"], sp["REM"], sp["GROW"], sp["ADD"]]
    else:
        raise KeyError(kind)
    return pairs, [new[p] if p in new else old[p[0]][p[1]] for p in pairs]


def merge(rows, pairs, filters):
    """test_pairs.merge: rows[o][i] with exactly the listed pairs replaced."""
    from test_pairs import merge as m
    return m(rows, pairs, filters)


def counts(shape, n_taps):
    """Partitions of a filter of n_taps taps (None: 0) on every level."""
    s, L, blocks, ratios, n_in, n_out = shape
    Ls, D, _ = geo(shape)
    n_taps = n_taps or 0
    return [-(-max(0, min(n_taps - D[k], blocks[k] * Ls[k])) // Ls[k]) for k in range(len(blocks))]


def fade_schedule(shape, a_f, K):
    """Per tail level of a fade of K head blocks made at head block a_f, every earlier block run: (blocks the catch-up covers,
    blocks run in lf_mode 1), as csrc/engine.hip schedules them (lfade_catch_up)."""
    _, D, r = geo(shape)
    L = shape[1]
    out = []
    for k in range(1, len(r)):
        Dk = D[k] // L
        z_next = a_f // r[k]                                             # the level's blocks complete before head block a_f
        j0 = max(0, (a_f - Dk) // r[k])                                  # the first one the fade reads under the new set
        j1 = (a_f + K - 1 - Dk) // r[k]                                  # the last one it reads under the old set
        out.append((z_next - j0, max(0, j1 - z_next + 1)))
    return out


# ---- declarations, exports, bindings ---------------------------------------------------------------------------------------------
def test_header_declares_both_calls():
    text = open(HEADER).read()
    for name, n_args in zip(NAMES, (7, 8)):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text, re.S)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == n_args, args
        assert args[:6] == ["bfir_engine *e", "int n_pairs", "const int *outputs", "const int *inputs", "const void *const *coeffs",
                            "const int *lengths"], args
        assert args[6] == "double scale" and (n_args == 7 or args[7] == "int fade_blocks"), args
        assert not re.search(r"\blong\b", m.group(1))
    assert "BFIR_PATCH_FUSED" in text and "a_f + K + r_max" in text


def test_library_exports_and_bindings(bfir):
    from foo_dsp_bfir_amd import _lib
    lib = bfir.load()
    for name in NAMES:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).restype == C.c_int
    assert len(_lib.SIGNATURES[NAMES[0]][1]) == 7 and len(_lib.SIGNATURES[NAMES[1]][1]) == 8
    if shutil.which("nm"):
        syms = subprocess.run(["nm", "-D", "--defined-only", bfir.library_path()], capture_output=True, text=True).stdout
        for name in NAMES:
            assert re.search(r"\bT %s$" % name, syms, re.M), name
    for meth in ("set_pairs", "fade_to_pairs"):
        assert callable(getattr(bfir.BrutefirMatrixLevels, meth))
        assert getattr(bfir.BrutefirMimoLevels, meth) is getattr(bfir.BrutefirMatrixLevels, meth)
        assert not hasattr(bfir.BrutefirMatrix, meth)
    for meth in ("set_coeff_pairs", "set_coeff_pairs_fade"):           # the uniform kinds' calls: inherited, untouched
        assert getattr(bfir.BrutefirMatrixLevels, meth) is getattr(bfir.BrutefirMatrix, meth)


def test_null_engine_is_refused_without_a_device(bfir):
    lib = bfir.load()
    one = (C.c_int * 1)(0)
    four = (C.c_int * 1)(4)
    h = np.zeros(4, np.float32)
    ptrs = (C.c_void_p * 1)(h.ctypes.data)
    assert lib.bfir_engine_set_coeff_matrix_levels_pairs(None, 1, one, one, ptrs, four, 1.0) == bfir.ERR_ARG
    assert lib.bfir_engine_set_coeff_matrix_levels_pairs_fade(None, 1, one, one, ptrs, four, 1.0, 2) == bfir.ERR_ARG


def test_cpp_mirror_methods_compile(tmp_path):
    """tests/cpp/test_lpairs_mirror.cpp calls both methods of brutefir_hip.hpp; compiled, not linked."""
    if not shutil.which("g++"):
        pytest.skip("no g++ on this machine")
    hpp = open(os.path.join(ROOT, "foo-dsp-bfir_amd", "host", "brutefir_hip.hpp")).read()
    assert "int set_coeff_matrix_levels_pairs(" in hpp and "int set_coeff_matrix_levels_pairs_fade(" in hpp
    src = os.path.join(ROOT, "tests", "cpp", "test_lpairs_mirror.cpp")
    text = open(src).read()
    assert ".set_coeff_matrix_levels_pairs(" in text and ".set_coeff_matrix_levels_pairs_fade(" in text
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-c", src, "-o", str(tmp_path / "mirror.o")], check=True)


def test_wpatch_kernel_register_report():
    """Every k_wpatch instance -- two precisions, two layouts, k_mac_mimo's output tiles, the one-block form and the tiled
    form -- has no scratch, no spill, no dynamic stack and no LDS, at the four waves per SIMD it is bounded for."""
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc on this machine")
    import importlib
    import sys
    sys.path.insert(0, ROOT)
    b = importlib.import_module("foo_dsp_bfir_amd._build")
    assert "wpatch.hip" in b.SOURCES
    b.build()
    u = b.resource_usage()
    got = set()
    for name, r in u.items():
        if "k_wpatch" not in name:
            continue
        m = re.search(r"k_wpatchI([fd])Lb([01])ELi(\d+)ELi(\d+)E", name)
        assert m, name
        for other in ("k_mac_matrix", "k_mac_duo", "k_mac_mimo", "k_wduo", "k_patch_pairs", "k_inv_", "k_delay_", "k_fade_blend"):
            assert other not in name, name
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["Dynamic Stack"] == "False", (name, r)
        assert r["LDS Size"] == 0 and r["Occupancy"] >= 4, (name, r)
        got.add((m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))))
    want = set()
    for ilv in (0, 1):
        for no in (1, 2, 4):                                             # fp32: TT = 8, but 4 in the grouped layout with four outputs
            want |= {("f", ilv, no, 1), ("f", ilv, no, 4 if (no == 4 and not ilv) else 8)}
        want |= {("d", ilv, 1, 1), ("d", ilv, 1, 8), ("d", ilv, 2, 1), ("d", ilv, 2, 4)}
    assert got == want, got ^ want
    # the kernels that were there before keep their instances
    assert sum("k_patch_pairs" in k for k in u) == 8 and sum("k_mac_mimo" in k for k in u) == 20 and sum("k_wduo" in k for k in u) == 12


# ---- the cases of tests/test_lpairs_gpu.py --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_geometry_of_the_gpu_cases(name):
    _, shape, K = SHAPES[name]
    s, L, blocks, ratios, n_in, n_out = shape
    Ls, D, r = geo(shape)
    n = len(blocks)
    old = old_lengths(shape)
    sp = special(shape)
    assert len(set(sp.values())) == 5
    # the old set reaches every level and reads every input; so the merged sets may be faded to
    assert all(any(counts(shape, v)[k] > 0 for row in old for v in row) for k in range(n))
    for kind in LISTS:
        pairs, new = pair_list(shape, kind)
        assert len(set(pairs)) == len(pairs)
        # a pair with partitions on every level in both sets
        assert any(min(counts(shape, old[o][i])) > 0 and min(counts(shape, v)) > 0 for (o, i), v in zip(pairs, new)), kind
        assert all(v is None or 0 < v <= D[-1] for v in new)
        merged = merge(old, pairs, new)
        assert all(any(counts(shape, v)[k] > 0 for row in merged for v in row) for k in range(n)), kind
        assert all(any(merged[o][i] for o in range(n_out)) for i in range(n_in)), kind       # every input is read
    pairs, new = pair_list(shape, "mixed")
    c_old = {p: counts(shape, old[p[0]][p[1]]) for p in pairs}
    c_new = {p: counts(shape, v) for p, v in zip(pairs, new)}
    assert sum(c_old[sp["ADD"]]) == 0 and sum(c_new[sp["ADD"]]) > 0                           # added
    assert sum(c_old[sp["REM"]]) > 0 and sum(c_new[sp["REM"]]) == 0                           # removed
    g_old, g_new = c_old[sp["GROW"]], c_new[sp["GROW"]]
    assert g_old[0] > 0 and g_old[1] == 0 and g_new[1] > 0                                    # grows into level 1, which is active
    s_old, s_new = c_old[sp["SHRINK"]], c_new[sp["SHRINK"]]
    assert s_old[n - 1] > 0 and s_new[n - 1] == 0 and s_new[n - 2] > 0                        # shrinks out of the last level
    assert pairs != sorted(pairs)                                                            # listed out of order
    # the fade
    r_max = r[-1]
    assert A_F % r_max != 0 and K > r_max
    for caught, both in fade_schedule(shape, A_F, K):
        assert caught >= 1 and both >= 1, (name, caught, both)
