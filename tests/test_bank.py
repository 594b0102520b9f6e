"""Coefficient banks (bfir_engine_bank_*, bfir_engine_set_coeff_matrix_bank, _bank_fade, _pairs_bank, _pairs_bank_fade)
without a GPU: the ten calls as declared, exported and bound, the refusal that needs no device, the C++ mirror's ten methods
under -Wall -Werror, and the register report of k_bank_gather (csrc/bank.hip)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bfir_hip.h")
# name -> the argument list the header declares
CALLS = {
    "bfir_engine_bank_create": ["bfir_engine *e", "int n_entries"],
    "bfir_engine_bank_destroy": ["bfir_engine *e"],
    "bfir_engine_bank_entries": ["const bfir_engine *e"],
    "bfir_engine_bank_blocks": ["const bfir_engine *e", "int entry"],
    "bfir_engine_bank_load": ["bfir_engine *e", "int first", "int n", "const void *const *coeffs", "int length",
                              "int coeff_blocks", "double scale"],
    "bfir_engine_bank_read": ["bfir_engine *e", "int entry", "int block", "void *dst"],
    "bfir_engine_set_coeff_matrix_bank": ["bfir_engine *e", "const int *entries"],
    "bfir_engine_set_coeff_matrix_bank_fade": ["bfir_engine *e", "const int *entries", "int fade_blocks"],
    "bfir_engine_set_coeff_matrix_pairs_bank": ["bfir_engine *e", "int n_pairs", "const int *outputs", "const int *inputs",
                                                "const int *entries"],
    "bfir_engine_set_coeff_matrix_pairs_bank_fade": ["bfir_engine *e", "int n_pairs", "const int *outputs", "const int *inputs",
                                                     "const int *entries", "int fade_blocks"],
}
METHODS = ("bank_create", "bank_destroy", "bank_entries", "bank_blocks", "bank_load", "bank_read", "set_coeff_bank",
           "set_coeff_bank_fade", "set_coeff_pairs_bank", "set_coeff_pairs_bank_fade")
MIRROR = ("bank_create", "bank_destroy", "bank_entries", "bank_blocks", "bank_load", "bank_read", "set_coeff_matrix_bank",
          "set_coeff_matrix_bank_fade", "set_coeff_matrix_pairs_bank", "set_coeff_matrix_pairs_bank_fade")


def test_header_declares_the_ten_calls():
    text = open(HEADER).read()
    for name, want in CALLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text, re.S)
        assert m, name
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert args == want, (name, args)
        assert not re.search(r"\blong\b", m.group(1))
    # the contract: what is out of scope, and the refusals, are written down
    flat = re.sub(r"\s*\n\s*\*\s*", " ", text)                                  # comment lines joined
    assert re.search(r"Multi-level kinds[^.]*have no banks", flat)
    for word in ("k_bank_gather", "a named entry is empty", "BFIR_ERR_STATE: no bank"):
        assert word in flat, word


def test_library_exports_and_bindings(bfir):
    from foo_dsp_bfir_amd import _lib
    lib = bfir.load()
    for name, want in CALLS.items():
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).restype == C.c_int
        assert len(_lib.SIGNATURES[name][1]) == len(want), name
    if shutil.which("nm"):
        syms = subprocess.run(["nm", "-D", "--defined-only", bfir.library_path()], capture_output=True, text=True).stdout
        for name in CALLS:
            assert re.search(r"\bT %s$" % name, syms, re.M), name
    for meth in METHODS:
        assert callable(getattr(bfir.BrutefirMatrix, meth))
        for cls in (bfir.BrutefirMimo, bfir.BrutefirMatrixLevels, bfir.BrutefirMimoLevels):   # inherited, not removed
            assert getattr(cls, meth) is getattr(bfir.BrutefirMatrix, meth), (cls.__name__, meth)


def test_null_engine_is_refused_without_a_device(bfir):
    lib = bfir.load()
    one = (C.c_int * 1)(0)
    h = np.zeros(4, np.float32)
    ptrs = (C.c_void_p * 1)(h.ctypes.data)
    dst = np.zeros(8, np.float32)
    assert lib.bfir_engine_bank_create(None, 4) == bfir.ERR_ARG
    assert lib.bfir_engine_bank_destroy(None) == bfir.ERR_ARG
    assert lib.bfir_engine_bank_entries(None) == bfir.ERR_ARG
    assert lib.bfir_engine_bank_blocks(None, 0) == bfir.ERR_ARG
    assert lib.bfir_engine_bank_load(None, 0, 1, ptrs, 4, 1, 1.0) == bfir.ERR_ARG
    assert lib.bfir_engine_bank_read(None, 0, 0, dst.ctypes.data) == bfir.ERR_ARG
    assert lib.bfir_engine_set_coeff_matrix_bank(None, one) == bfir.ERR_ARG
    assert lib.bfir_engine_set_coeff_matrix_bank_fade(None, one, 2) == bfir.ERR_ARG
    assert lib.bfir_engine_set_coeff_matrix_pairs_bank(None, 1, one, one, one) == bfir.ERR_ARG
    assert lib.bfir_engine_set_coeff_matrix_pairs_bank_fade(None, 1, one, one, one, 2) == bfir.ERR_ARG


def test_cpp_mirror_methods_compile(tmp_path):
    """tests/cpp/test_bank_mirror.cpp calls the ten methods of brutefir_hip.hpp; compiled, not linked."""
    if not shutil.which("g++"):
        pytest.skip("no g++ on this machine")
    hpp = open(os.path.join(ROOT, "foo-dsp-bfir_amd", "host", "brutefir_hip.hpp")).read()
    src = os.path.join(ROOT, "tests", "cpp", "test_bank_mirror.cpp")
    text = open(src).read()
    for meth in MIRROR:
        assert "int %s(" % meth in hpp, meth
        assert ".%s(" % meth in text, meth
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-c", src, "-o", str(tmp_path / "mirror.o")], check=True)


def test_gather_kernel_register_report():
    """Every k_bank_gather instance (there is one: a row is bytes) has no scratch, no spill, no dynamic stack and no LDS; its
    name carries none of the substrings other tests count kernels by, and those counts are what they were."""
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc on this machine")
    import importlib
    import sys
    sys.path.insert(0, ROOT)
    b = importlib.import_module("foo_dsp_bfir_amd._build")
    assert "bank.hip" in b.SOURCES
    b.build()
    u = b.resource_usage()
    got = [name for name in u if "k_bank_gather" in name]
    assert len(got) == 1, got
    for name in got:
        r = u[name]
        for other in ("k_mac_matrix", "k_mac_duo", "k_mac_mimo", "k_wduo", "k_wpatch", "k_patch_pairs", "k_inv_", "k_fwd",
                      "k_delay_", "k_fade_blend", "k_resample"):
            assert other not in name, name
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["Dynamic Stack"] == "False", (name, r)
        assert r["LDS Size"] == 0, (name, r)
    # the instance counts tests/test_pairs.py asserts for the kernels that were there before
    assert sum("k_mac_matrix" in k for k in u) == 20 and sum("k_mac_duo" in k for k in u) == 12
    assert sum("k_patch_pairs" in k for k in u) == 8
