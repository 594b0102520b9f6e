"""Bank mixes (bfir_engine_set_coeff_matrix_bank_mix, _bank_mix_fade, _pairs_bank_mix, _pairs_bank_mix_fade) without a GPU:
the four calls as declared, exported and bound, the refusal that needs no device, the C++ mirror's four methods under -Wall
-Werror, the register report of k_bank_mix (csrc/bankmix.hip), and the NumPy restatement (tests/bankmix_model.py) against
facts that need no device."""
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from bankmix_model import mix_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bfir_hip.h")
# name -> the argument list the header declares
CALLS = {
    "bfir_engine_set_coeff_matrix_bank_mix": ["bfir_engine *e", "int n_terms", "const int *entries", "const double *weights"],
    "bfir_engine_set_coeff_matrix_bank_mix_fade": ["bfir_engine *e", "int n_terms", "const int *entries",
                                                   "const double *weights", "int fade_blocks"],
    "bfir_engine_set_coeff_matrix_pairs_bank_mix": ["bfir_engine *e", "int n_pairs", "const int *outputs", "const int *inputs",
                                                    "int n_terms", "const int *entries", "const double *weights"],
    "bfir_engine_set_coeff_matrix_pairs_bank_mix_fade": ["bfir_engine *e", "int n_pairs", "const int *outputs",
                                                         "const int *inputs", "int n_terms", "const int *entries",
                                                         "const double *weights", "int fade_blocks"],
}
METHODS = ("set_coeff_bank_mix", "set_coeff_bank_mix_fade", "set_coeff_pairs_bank_mix", "set_coeff_pairs_bank_mix_fade")
MIRROR = ("set_coeff_matrix_bank_mix", "set_coeff_matrix_bank_mix_fade", "set_coeff_matrix_pairs_bank_mix",
          "set_coeff_matrix_pairs_bank_mix_fade")
# the substrings existing tests count kernels by
COUNTED = ("k_bank_gather", "k_mac_matrix", "k_mac_duo", "k_mac_mimo", "k_wduo", "k_wpatch", "k_patch_pairs", "k_inv_", "k_fwd",
           "k_delay_", "k_fade_blend", "k_resample", "k_lbank_gather")


def test_header_declares_the_four_calls():
    text = open(HEADER).read()
    for name, want in CALLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text, re.S)
        assert m, name
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert args == want, (name, args)
        assert not re.search(r"\blong\b", m.group(1))
    assert re.search(r"^#define\s+BFIR_BANK_MIX_TERMS\s+4\s*$", text, re.M)
    kernels_h = open(os.path.join(ROOT, "foo-dsp-bfir_amd", "csrc", "kernels.h")).read()
    assert re.search(r"BFIR_BANK_MIX_TERMS\s*(=|\s)\s*4\b", kernels_h)
    # the contract: the operation, the refusals and what is out of scope are written down
    flat = re.sub(r"\s*\n\s*\*\s*", " ", text)                                  # comment lines joined
    for word in ("k_bank_mix", "the first product starting the sum", "no fma", "a live term names an empty entry",
                 "n_terms outside 1 .. BFIR_BANK_MIX_TERMS", "becomes infinite in the working precision",
                 "Out of scope: mixes on the multi-level kinds", "complex weights"):
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


def test_terms_are_padded_to_the_longest_list(bfir):
    n, ents, wts = bfir.BrutefirMatrix._mix_args([[(3, 0.5)], None, [], [(1, 2.0), (None, 1.0), (7, -0.25)]])
    assert n == 3
    assert list(ents) == [3, -1, -1, -1, -1, -1, -1, -1, -1, 1, -1, 7]
    assert list(wts) == [0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 2.0, 1.0, -0.25]
    n, ents, wts = bfir.BrutefirMatrix._mix_args([None, []])                  # no path anywhere: one dead term per row
    assert n == 1 and list(ents) == [-1, -1] and list(wts) == [0.0, 0.0]


def test_null_engine_is_refused_without_a_device(bfir):
    lib = bfir.load()
    one = (C.c_int * 1)(0)
    w = (C.c_double * 1)(1.0)
    assert lib.bfir_engine_set_coeff_matrix_bank_mix(None, 1, one, w) == bfir.ERR_ARG
    assert lib.bfir_engine_set_coeff_matrix_bank_mix_fade(None, 1, one, w, 2) == bfir.ERR_ARG
    assert lib.bfir_engine_set_coeff_matrix_pairs_bank_mix(None, 1, one, one, 1, one, w) == bfir.ERR_ARG
    assert lib.bfir_engine_set_coeff_matrix_pairs_bank_mix_fade(None, 1, one, one, 1, one, w, 2) == bfir.ERR_ARG


def test_cpp_mirror_methods_compile(tmp_path):
    """tests/cpp/test_bankmix_mirror.cpp calls the four methods of brutefir_hip.hpp; compiled, not linked."""
    if not shutil.which("g++"):
        pytest.skip("no g++ on this machine")
    hpp = open(os.path.join(ROOT, "foo-dsp-bfir_amd", "host", "brutefir_hip.hpp")).read()
    src = os.path.join(ROOT, "tests", "cpp", "test_bankmix_mirror.cpp")
    text = open(src).read()
    for meth in MIRROR:
        assert "int %s(" % meth in hpp, meth
        assert ".%s(" % meth in text, meth
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-c", src, "-o", str(tmp_path / "mirror.o")], check=True)


def test_mix_kernel_register_report():
    """The two k_bank_mix instances (float, double) have no scratch, no spill, no dynamic stack and no LDS; their names carry
    none of the substrings other tests count kernels by, and those counts are what they were."""
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc on this machine")
    import importlib
    import sys
    sys.path.insert(0, ROOT)
    b = importlib.import_module("foo_dsp_bfir_amd._build")
    assert "bankmix.hip" in b.SOURCES
    b.build()
    u = b.resource_usage()
    got = [name for name in u if "k_bank_mix" in name]
    assert len(got) == 2, got
    for name in got:
        r = u[name]
        for other in COUNTED:
            assert other not in name, name
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["Dynamic Stack"] == "False", (name, r)
        assert r["LDS Size"] == 0, (name, r)
    assert sum("k_bank_gather" in k for k in u) == 1
    assert sum("k_mac_matrix" in k for k in u) == 20 and sum("k_mac_duo" in k for k in u) == 12
    assert sum("k_patch_pairs" in k for k in u) == 8


# ---- the model -----------------------------------------------------------------------------------------------------------------
B, N = 4, 32


def _entry(rng, dtype, count):
    """An entry as bank_read gives it: `count` partitions of spectra away from the subnormals, zeros behind them."""
    h = np.zeros((B, N), dtype)
    h[:count] = (rng.uniform(0.25, 1.0, (count, N)) * rng.choice([-1.0, 1.0], (count, N))).astype(dtype)
    return h


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_model_one_term_of_weight_one_is_the_entry(dtype):
    rng = np.random.default_rng(1)
    for c in (1, 3, B):
        e = _entry(rng, dtype, c)
        stale = e.copy(); stale[c:] = 7.0                    # what the store may hold past the count is not read
        row, cnt = mix_row([stale], [c], [1.0], dtype, B)
        assert cnt == c and row.tobytes() == e.tobytes()
        half, cnt2 = mix_row([stale, stale], [c, c], [0.5, 0.5], dtype, B)     # halving and adding the halves are exact
        assert cnt2 == c and half.tobytes() == e.tobytes()


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_model_dead_terms_take_no_part(dtype):
    rng = np.random.default_rng(2)
    a, b = _entry(rng, dtype, 2), _entry(rng, dtype, B)
    w = -0.7
    alone = mix_row([a], [2], [w], dtype, B)
    no_entry = mix_row([a, None], [2, 0], [w, 3.0], dtype, B)
    zero_weight = mix_row([a, b], [2, B], [w, 0.0], dtype, B)
    empty_named = mix_row([a, np.zeros((B, N), dtype)], [2, 0], [w, 0.0], dtype, B)   # weight 0 may name an empty entry
    for row, cnt in (no_entry, zero_weight, empty_named):
        assert cnt == alone[1] == 2 and row.tobytes() == alone[0].tobytes()
    if dtype == np.float32:                                  # 1e-60 converts to 0 in float and is handled like 0
        row, cnt = mix_row([a, b], [2, B], [w, 1e-60], dtype, B)
        assert cnt == 2 and row.tobytes() == alone[0].tobytes()
    else:
        row, cnt = mix_row([a, b], [2, B], [w, 1e-60], dtype, B)
        assert cnt == B
    for rows, counts, ws in (([None], [0], [1.0]), ([a, b], [2, B], [0.0, -0.0]), ([None, b], [0, B], [2.0, 0.0])):
        row, cnt = mix_row(rows, counts, ws, dtype, B)
        assert cnt == 0 and row.shape[0] == B and not row.any()


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_model_short_entries_leave_the_long_one_alone(dtype):
    rng = np.random.default_rng(3)
    short, long_ = _entry(rng, dtype, 1), _entry(rng, dtype, B)
    stale = short.copy(); stale[1:] = 5.0
    ws, wl = dtype(0.375), dtype(-1.5)
    for order in ((0, 1), (1, 0)):
        rows, counts, w = [[stale, long_][k] for k in order], [[1, B][k] for k in order], [[ws, wl][k] for k in order]
        row, cnt = mix_row(rows, counts, w, dtype, B)
        assert cnt == B
        assert row[1:].tobytes() == (wl * long_[1:]).tobytes()               # the long entry's product alone
        first = (ws * short[0], wl * long_[0])
        assert row[0].tobytes() == (first[order[0]] + first[order[1]]).tobytes()
    # -0 stays -0: the first product starts the sum, there is no 0 + ...
    z = np.zeros((B, N), dtype); z[0, 0] = 1.0; z[0, 1] = 0.0
    row, _ = mix_row([z], [1], [-2.0], dtype, B)
    assert row[0, 0] == -2.0 and np.signbit(row[0, 1])


def test_model_listed_order_is_part_of_the_definition():
    """In float32 there are values and weights for which another order of the same three terms rounds differently."""
    rng = np.random.default_rng(20240)
    found = None
    for _ in range(1000):
        h = rng.uniform(0.25, 1.0, (3, 1, 8)).astype(np.float32) * rng.choice([-1.0, 1.0], (3, 1, 1)).astype(np.float32)
        w = rng.uniform(2.0 ** -6, 4.0, 3)
        base, _ = mix_row(list(h), [1] * 3, list(w), np.float32, 1)
        for perm in itertools.permutations(range(3)):
            other, _ = mix_row([h[k] for k in perm], [1] * 3, [w[k] for k in perm], np.float32, 1)
            if other.tobytes() != base.tobytes():
                found = (perm, base, other)
                break
        if found:
            break
    assert found, "no triple in 1000 draws: float32 addition would have to be associative"
    perm, base, other = found
    # ... by roundings of sums of three products below 4 each, no more
    assert np.max(np.abs(base - other)) <= 4 * np.finfo(np.float32).eps * 12.0
