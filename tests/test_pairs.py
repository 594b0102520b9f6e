"""Pair-list coefficient updates (bfir_engine_set_coeff_matrix_pairs, _pairs_fade) without a GPU: the two calls as declared,
exported and bound, the refusal that needs no device, the C++ mirror's two methods under -Wall -Werror, the register report
of k_patch_pairs (csrc/patch.hip), and merge(), the helper the GPU tests build their merged sets with."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bfir_hip.h")
NAMES = ("bfir_engine_set_coeff_matrix_pairs", "bfir_engine_set_coeff_matrix_pairs_fade")


def merge(rows, pairs, filters):
    """The merged set: rows[o][i] with exactly the listed pairs replaced, filters[k] (or None) at pairs[k] = (o, i).  The
    rows given are not written to."""
    assert len(pairs) == len(filters) and len(set(pairs)) == len(pairs)
    out = [list(r) for r in rows]
    for (o, i), h in zip(pairs, filters):
        out[o][i] = h
    return out


def test_merge_replaces_exactly_the_listed_pairs():
    a, b, c, d, e = (np.full(3, v) for v in (1.0, 2.0, 3.0, 4.0, 5.0))
    rows = [[a, None, b], [None, c, None]]
    got = merge(rows, [(0, 1), (1, 1), (0, 2), (1, 0)], [d, None, e, None])
    assert got[0][0] is a and got[0][1] is d and got[0][2] is e
    assert got[1] == [None, None, None]
    assert rows[0][1] is None and rows[0][2] is b and rows[1][1] is c          # the old set is untouched
    with pytest.raises(AssertionError):
        merge(rows, [(0, 0), (0, 0)], [a, b])


def test_header_declares_both_calls():
    text = open(HEADER).read()
    want = {NAMES[0]: 8, NAMES[1]: 9}
    for name, n_args in want.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text, re.S)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == n_args, args
        assert args[0] == "bfir_engine *e" and args[1] == "int n_pairs", args
        assert args[2] == "const int *outputs" and args[3] == "const int *inputs" and args[4] == "const void *const *coeffs", args
        assert not re.search(r"\blong\b", m.group(1))
    assert re.search(r"NOT bitwise", text) and re.search(r"blended with itself", text)


def test_library_exports_and_bindings(bfir):
    from foo_dsp_bfir_amd import _lib
    lib = bfir.load()
    for name in NAMES:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).restype == C.c_int
    assert len(_lib.SIGNATURES[NAMES[1]][1]) == len(_lib.SIGNATURES[NAMES[0]][1]) + 1 == 9
    if shutil.which("nm"):
        syms = subprocess.run(["nm", "-D", "--defined-only", bfir.library_path()], capture_output=True, text=True).stdout
        for name in NAMES:
            assert re.search(r"\bT %s$" % name, syms, re.M), name
    for meth in ("set_coeff_pairs", "set_coeff_pairs_fade"):
        assert callable(getattr(bfir.BrutefirMatrix, meth))
        assert getattr(bfir.BrutefirMimo, meth) is getattr(bfir.BrutefirMatrix, meth)


def test_null_engine_is_refused_without_a_device(bfir):
    lib = bfir.load()
    one = (C.c_int * 1)(0)
    h = np.zeros(4, np.float32)
    ptrs = (C.c_void_p * 1)(h.ctypes.data)
    assert lib.bfir_engine_set_coeff_matrix_pairs(None, 1, one, one, ptrs, 4, 1, 1.0) == bfir.ERR_ARG
    assert lib.bfir_engine_set_coeff_matrix_pairs_fade(None, 1, one, one, ptrs, 4, 1, 1.0, 2) == bfir.ERR_ARG


def test_cpp_mirror_methods_compile(tmp_path):
    """tests/cpp/test_pairs_mirror.cpp calls both methods of brutefir_hip.hpp; compiled, not linked."""
    if not shutil.which("g++"):
        pytest.skip("no g++ on this machine")
    hpp = open(os.path.join(ROOT, "foo-dsp-bfir_amd", "host", "brutefir_hip.hpp")).read()
    assert "int set_coeff_matrix_pairs(" in hpp and "int set_coeff_matrix_pairs_fade(" in hpp
    src = os.path.join(ROOT, "tests", "cpp", "test_pairs_mirror.cpp")
    text = open(src).read()
    assert ".set_coeff_matrix_pairs(" in text and ".set_coeff_matrix_pairs_fade(" in text
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-c", src, "-o", str(tmp_path / "mirror.o")], check=True)


def test_patch_kernel_register_report():
    """Every k_patch_pairs instance -- two precisions, two layouts, the one-block form and the tiled form -- has no scratch,
    no spill and no dynamic stack; its name carries none of the substrings other tests count kernels by."""
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc on this machine")
    import importlib
    import sys
    sys.path.insert(0, ROOT)
    b = importlib.import_module("foo_dsp_bfir_amd._build")
    assert "patch.hip" in b.SOURCES
    b.build()
    u = b.resource_usage()
    got = set()
    for name, r in u.items():
        if "k_patch_pairs" not in name:
            continue
        m = re.search(r"k_patch_pairsI([fd])Lb([01])ELi(\d+)E", name)
        assert m, name
        for other in ("k_mac_matrix", "k_mac_duo", "k_mac_mimo", "k_wduo", "k_inv_", "k_delay_", "k_fade_blend"):
            assert other not in name, name
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["Dynamic Stack"] == "False", (name, r)
        assert r["LDS Size"] == 0 and r["Occupancy"] >= 4, (name, r)
        got.add((m.group(1), int(m.group(2)), int(m.group(3))))
    assert got == {(t, ilv, tt) for t, tiled in (("f", 8), ("d", 4)) for ilv in (0, 1) for tt in (1, tiled)}, got
    # the instance counts of the kernels that were there before
    assert sum("k_mac_matrix" in k for k in u) == 20 and sum("k_mac_duo" in k for k in u) == 12
