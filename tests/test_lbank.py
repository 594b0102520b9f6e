"""Coefficient banks on multi-level matrix and mimo engines (bfir_engine_levels_bank_*, bfir_engine_set_coeff_matrix_levels_bank,
_bank_fade, _pairs_bank, _pairs_bank_fade) without a GPU: the calls as declared, exported and bound, the refusal that needs
no device, the C++ mirror's methods under -Wall -Werror, the register report of k_lbank_gather (csrc/lbank.hip), and the
shapes of tests/test_lbank_gpu.py, held here to the conditions their descriptions state.

The shapes.  Beside the four of tests/test_lpairs.py (SHAPES, with its old_lengths, pair_list kinds and A_F):
  boundary   L = 16, blocks (40, 3), ratios (1, 2): head rows of 5120 / 10240 bytes (fp32 / fp64); entries whose head counts
             are 33 and 39, so the line between copied and zeroed bytes falls inside a span, while the tail's rows (768 / 1536
             bytes) lie below one span
  partial    L = 256, blocks (5, 2), ratios (1, 4): in fp32 a head row of 2.5 spans beside a tail row of exactly one workgroup
  big        L = 1024, blocks (4, 8), ratios (1, 4), fp32, 16385 entries: the tail level's store passes 4 GiB, its last entry
             starts at byte 2^32 (four head blocks, not one: a level must be complete when it is first read, D_1 >= L_1, so
             bfir_engine_create_matrix_levels refuses fewer at this ratio; the tail level, whose store it is, is unchanged)
In 9x10 the rows are 16, 32 and 64 KiB: the three levels take 1, 2 and 4 workgroups of a row."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_levels import level_geometry
from test_lpairs import SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bfir_hip.h")
SPAN, STEPS = 4096, 4                                                    # BFIR_BANK_SPAN, BFIR_BANK_STEPS (csrc/kernels.h)
PAIRS = ["bfir_engine *e", "int n_pairs", "const int *outputs", "const int *inputs", "const int *entries"]
# name -> the argument list the header declares
CALLS = {
    "bfir_engine_levels_bank_create": ["bfir_engine *e", "int n_entries"],
    "bfir_engine_levels_bank_destroy": ["bfir_engine *e"],
    "bfir_engine_levels_bank_entries": ["const bfir_engine *e"],
    "bfir_engine_levels_bank_length": ["const bfir_engine *e", "int entry"],
    "bfir_engine_levels_bank_blocks": ["const bfir_engine *e", "int entry", "int level"],
    "bfir_engine_levels_bank_load": ["bfir_engine *e", "int first", "int n", "const void *const *coeffs", "const int *lengths",
                                     "double scale"],
    "bfir_engine_levels_bank_read": ["bfir_engine *e", "int entry", "int level", "int block", "void *dst"],
    "bfir_engine_set_coeff_matrix_levels_bank": ["bfir_engine *e", "const int *entries"],
    "bfir_engine_set_coeff_matrix_levels_bank_fade": ["bfir_engine *e", "const int *entries", "int fade_blocks"],
    "bfir_engine_set_coeff_matrix_levels_pairs_bank": PAIRS,
    "bfir_engine_set_coeff_matrix_levels_pairs_bank_fade": PAIRS + ["int fade_blocks"],
}
METHODS = ("lbank_create", "lbank_destroy", "lbank_entries", "lbank_length", "lbank_blocks", "lbank_load", "lbank_read",
           "set_bank", "fade_to_rows_bank", "set_pairs_bank", "fade_to_pairs_bank")
MIRROR = tuple(name[len("bfir_engine_"):] for name in CALLS)

# id: (L, blocks, ratios); run in both precisions on the two kinds of KINDS
NEW_SHAPES = {"boundary": (16, (40, 3), (1, 2)), "partial": (256, (5, 2), (1, 4))}
KINDS = {"matrix": ("BrutefirMatrixLevels", 2, 3), "mimo": ("BrutefirMimoLevels", 9, 5)}
BOUNDARY_COUNTS = (33, 39)
BIG = (1024, (4, 8), (1, 4), 4, 16385)                                   # L, blocks, ratios, realsize, entries


def row_bytes(L, blocks, ratios, s):
    """Bytes of a row of every level's store: blocks[k] partitions of 2 L_k reals."""
    Ls, _ = level_geometry(L, blocks, ratios)
    return [b * 2 * Lk * s for b, Lk in zip(blocks, Ls)]


def workgroups(n_bytes):
    return -(-n_bytes // (STEPS * SPAN))


def test_header_declares_the_calls():
    text = open(HEADER).read()
    for name, want in CALLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text, re.S)
        assert m, name
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert args == want, (name, args)
        assert not re.search(r"\blong\b", m.group(1))
    flat = re.sub(r"\s*\n\s*\*\s*", " ", text)                                  # comment lines joined
    assert re.search(r"Multi-level kinds[^.]*have no banks", flat)             # of the uniform group, which points here
    assert re.search(r"have no banks of this group[^.]*bfir_engine_levels_bank_\*", flat)
    for word in ("k_lbank_gather", "a named entry is empty", "BFIR_ERR_STATE: no bank", "n_entries * 2 * realsize * D_(n_levels)",
                 "keep refusing these two", "never a skipped launch"):
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
        assert callable(getattr(bfir.BrutefirMatrixLevels, meth))
        assert getattr(bfir.BrutefirMimoLevels, meth) is getattr(bfir.BrutefirMatrixLevels, meth)
        assert not hasattr(bfir.BrutefirMatrix, meth)


def test_null_engine_is_refused_without_a_device(bfir):
    lib = bfir.load()
    one = (C.c_int * 1)(0)
    four = (C.c_int * 1)(4)
    h = np.zeros(4, np.float32)
    ptrs = (C.c_void_p * 1)(h.ctypes.data)
    dst = np.zeros(8, np.float32)
    assert lib.bfir_engine_levels_bank_create(None, 4) == bfir.ERR_ARG
    assert lib.bfir_engine_levels_bank_destroy(None) == bfir.ERR_ARG
    assert lib.bfir_engine_levels_bank_entries(None) == bfir.ERR_ARG
    assert lib.bfir_engine_levels_bank_length(None, 0) == bfir.ERR_ARG
    assert lib.bfir_engine_levels_bank_blocks(None, 0, 0) == bfir.ERR_ARG
    assert lib.bfir_engine_levels_bank_load(None, 0, 1, ptrs, four, 1.0) == bfir.ERR_ARG
    assert lib.bfir_engine_levels_bank_read(None, 0, 0, 0, dst.ctypes.data) == bfir.ERR_ARG
    assert lib.bfir_engine_set_coeff_matrix_levels_bank(None, one) == bfir.ERR_ARG
    assert lib.bfir_engine_set_coeff_matrix_levels_bank_fade(None, one, 2) == bfir.ERR_ARG
    assert lib.bfir_engine_set_coeff_matrix_levels_pairs_bank(None, 1, one, one, one) == bfir.ERR_ARG
    assert lib.bfir_engine_set_coeff_matrix_levels_pairs_bank_fade(None, 1, one, one, one, 2) == bfir.ERR_ARG


def test_cpp_mirror_methods_compile(tmp_path):
    """tests/cpp/test_lbank_mirror.cpp calls every method of the group in brutefir_hip.hpp; compiled, not linked."""
    if not shutil.which("g++"):
        pytest.skip("no g++ on this machine")
    hpp = open(os.path.join(ROOT, "foo-dsp-bfir_amd", "host", "brutefir_hip.hpp")).read()
    src = os.path.join(ROOT, "tests", "cpp", "test_lbank_mirror.cpp")
    text = open(src).read()
    for meth in MIRROR:
        assert "int %s(" % meth in hpp, meth
        assert ".%s(" % meth in text, meth
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-c", src, "-o", str(tmp_path / "mirror.o")], check=True)


def test_gather_kernel_register_report():
    """k_lbank_gather has one instance (a row is bytes, the levels are arguments) with no scratch, no spill, no dynamic stack
    and no LDS; its name carries none of the substrings other tests count kernels by, and those counts are what they were."""
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc on this machine")
    import importlib
    import sys
    sys.path.insert(0, ROOT)
    b = importlib.import_module("foo_dsp_bfir_amd._build")
    assert "lbank.hip" in b.SOURCES
    b.build()
    u = b.resource_usage()
    got = [name for name in u if "k_lbank_gather" in name]
    assert len(got) == 1, got
    for name in got:
        r = u[name]
        for other in ("k_bank_gather", "k_mac_matrix", "k_mac_duo", "k_mac_mimo", "k_wduo", "k_wpatch", "k_patch_pairs", "k_inv_",
                      "k_fwd", "k_delay_", "k_fade_blend", "k_resample"):
            assert other not in name, name
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["Dynamic Stack"] == "False", (name, r)
        assert r["LDS Size"] == 0, (name, r)
    assert sum("k_bank_gather" in k for k in u) == 1
    assert sum("k_mac_matrix" in k for k in u) == 20 and sum("k_mac_duo" in k for k in u) == 12
    assert sum("k_patch_pairs" in k for k in u) == 8


def test_the_shapes_lie_where_the_docstring_says():
    L, blocks, ratios = NEW_SHAPES["boundary"]
    for s, head, tail in ((4, 5120, 768), (8, 10240, 1536)):
        rows = row_bytes(L, blocks, ratios, s)
        assert rows == [head, tail]
        assert SPAN < head and tail < SPAN and SPAN % (2 * L * s) == 0            # a span holds whole partitions ...
        for c in BOUNDARY_COUNTS:
            assert c < blocks[0] and (c * 2 * L * s) % SPAN and c * 2 * L * s > SPAN   # ... and the line lies inside a later one
    L, blocks, ratios = NEW_SHAPES["partial"]
    rows = row_bytes(L, blocks, ratios, 4)
    assert rows[0] * 2 == 5 * SPAN and rows[1] == STEPS * SPAN                    # 2.5 spans beside exactly one workgroup
    assert workgroups(rows[0]) == 1 and workgroups(rows[1]) == 1
    assert [workgroups(r) for r in row_bytes(L, blocks, ratios, 8)] == [2, 2]     # fp64: the head's second workgroup is partial, the tail's full
    # 9x10: the piece-to-level mapping has 1, 2 and 4 workgroups to tell apart
    s, L, blocks, ratios = SHAPES["9x10"][1][:4]
    rows = row_bytes(L, blocks, ratios, s)
    assert rows == [16 << 10, 32 << 10, 64 << 10] and [workgroups(r) for r in rows] == [1, 2, 4]
    # big: the tail level's last entry starts at byte 2^32; the head level's store is small
    L, blocks, ratios, s, n = BIG
    rows = row_bytes(L, blocks, ratios, s)
    assert (n - 1) * rows[1] == 1 << 32 and n * rows[0] < 1 << 30 and blocks[0] * L == L * ratios[1]
    # every partition is whole 16 bytes at every shape of the file
    shapes = [v[1][:4] for v in SHAPES.values()] + [(s,) + v for v in NEW_SHAPES.values() for s in (4, 8)]
    for s, L, blocks, ratios in shapes:
        Ls, _ = level_geometry(L, blocks, ratios)
        assert all((2 * Lk * s) % 16 == 0 for Lk in Ls)
