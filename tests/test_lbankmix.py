"""Bank mixes on multi-level matrix and mimo engines (bfir_engine_set_coeff_matrix_levels_bank_mix, _bank_mix_fade,
_pairs_bank_mix, _pairs_bank_mix_fade) without a GPU: the four calls as declared, exported and bound, the refusal that needs no
device, the C++ mirror's four methods under -Wall -Werror, the register report of k_lbank_mix (csrc/lbankmix.hip), the host
arithmetic of its records under the host sanitizers (tests/cpp/test_level_mix_tables.cpp), and the shapes of
tests/test_lbankmix_gpu.py, held here to the conditions their descriptions state.

The shapes.  A workgroup of k_lbank_mix writes BFIR_BANK_MIX_STEPS = 2 spans of BFIR_BANK_SPAN = 4096 bytes of a row, 8192
bytes.  Beside the four of tests/test_lpairs.py (SHAPES):
  boundary   L = 16, blocks (40, 3), ratios (1, 2): head rows of 5120 / 10240 bytes (fp32 / fp64).  Terms with head counts 33,
             39 and 40 put both lines -- two terms | one term behind count 33, one term | zeros behind count 39 of a row of
             those two -- inside ONE span; the tail's rows (768 / 1536 bytes) lie below a span
  partial    L = 256, blocks (5, 2), ratios (1, 4): the head's last workgroup is partly filled (1.25 / 2.5 workgroups a row),
             the tail's are exactly filled (2 / 4)
In 9x10 the rows are 16, 32 and 64 KiB: the three levels take 2, 4 and 8 workgroups of a row."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from test_bankmix import COUNTED
from test_lbank import KINDS, NEW_SHAPES, row_bytes
from test_levels import level_geometry
from test_lpairs import SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bfir_hip.h")
SPAN, STEPS = 4096, 2                                                    # BFIR_BANK_SPAN, BFIR_BANK_MIX_STEPS (csrc/kernels.h)
PER = SPAN * STEPS
PAIRS = ["bfir_engine *e", "int n_pairs", "const int *outputs", "const int *inputs"]
TERMS = ["int n_terms", "const int *entries", "const double *weights"]
# name -> the argument list the header declares
CALLS = {
    "bfir_engine_set_coeff_matrix_levels_bank_mix": ["bfir_engine *e"] + TERMS,
    "bfir_engine_set_coeff_matrix_levels_bank_mix_fade": ["bfir_engine *e"] + TERMS + ["int fade_blocks"],
    "bfir_engine_set_coeff_matrix_levels_pairs_bank_mix": PAIRS + TERMS,
    "bfir_engine_set_coeff_matrix_levels_pairs_bank_mix_fade": PAIRS + TERMS + ["int fade_blocks"],
}
METHODS = ("set_bank_mix", "fade_to_rows_bank_mix", "set_pairs_bank_mix", "fade_to_pairs_bank_mix")
MIRROR = tuple(name[len("bfir_engine_"):] for name in CALLS)
# the head and tail counts of the four terms of the boundary row of tests/test_lbankmix_gpu.py
BOUNDARY_TERMS = ((33, 0), (39, 0), (40, 2), (40, 3))


def workgroups(n_bytes):
    return -(-n_bytes // PER)


def test_header_declares_the_four_calls():
    text = open(HEADER).read()
    for name, want in CALLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text, re.S)
        assert m, name
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert args == want, (name, args)
        assert not re.search(r"\blong\b", m.group(1))
    kernels_h = open(os.path.join(ROOT, "foo-dsp-bfir_amd", "csrc", "kernels.h")).read()
    assert re.search(r"BFIR_BANK_MIX_STEPS\s*=\s*%d\b" % STEPS, kernels_h) and re.search(r"BFIR_BANK_SPAN\s*=\s*%d\b" % SPAN, kernels_h)
    for word in ("struct LBankMixArgs", "bool lbank_mix_supported(", "int launch_lbank_mix("):
        assert word in kernels_h, word
    # the contract: the operation, the refusals, the cost, and the pointer from the uniform group
    flat = re.sub(r"\s*\n\s*\*\s*", " ", text)                                  # comment lines joined
    for word in ("k_lbank_mix", "The operation is k_bank_mix's, applied per level", "c_k = max c_j,k",
                 "the first product starting the sum", "no fma", "Nothing is multiplied by zero",
                 "a live term names an empty entry (length 0", "n_terms outside 1 .. BFIR_BANK_MIX_TERMS",
                 "becomes infinite in the working precision", "a launch is never skipped", "decided by the mixed rows' counts c_k",
                 "nb_new = c_k", "upload ONE table", "Out of scope: mixes on the multi-level kinds (BFIR_ERR_UNSUPPORTED there)"):
        assert word in flat, word
    assert re.search(r"Out of scope: mixes on the multi-level kinds[^;]*bfir_engine_set_coeff_matrix_levels_\*bank_mix\*", flat)


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
        assert not hasattr(bfir.BrutefirMatrix, meth) and not hasattr(bfir.BrutefirMimo, meth)
    for meth in ("set_coeff_bank_mix", "set_coeff_bank_mix_fade", "set_coeff_pairs_bank_mix", "set_coeff_pairs_bank_mix_fade", "_mix_args"):
        assert getattr(bfir.BrutefirMatrixLevels, meth) is getattr(bfir.BrutefirMatrix, meth)   # inherited, untouched


def test_null_engine_is_refused_without_a_device(bfir):
    lib = bfir.load()
    one = (C.c_int * 1)(0)
    w = (C.c_double * 1)(1.0)
    assert lib.bfir_engine_set_coeff_matrix_levels_bank_mix(None, 1, one, w) == bfir.ERR_ARG
    assert lib.bfir_engine_set_coeff_matrix_levels_bank_mix_fade(None, 1, one, w, 2) == bfir.ERR_ARG
    assert lib.bfir_engine_set_coeff_matrix_levels_pairs_bank_mix(None, 1, one, one, 1, one, w) == bfir.ERR_ARG
    assert lib.bfir_engine_set_coeff_matrix_levels_pairs_bank_mix_fade(None, 1, one, one, 1, one, w, 2) == bfir.ERR_ARG
    # a null engine comes before every other argument
    assert lib.bfir_engine_set_coeff_matrix_levels_bank_mix(None, 0, None, None) == bfir.ERR_ARG
    assert lib.bfir_engine_set_coeff_matrix_levels_pairs_bank_mix_fade(None, 0, None, None, 9, None, None, 0) == bfir.ERR_ARG


def test_cpp_mirror_methods_compile(tmp_path):
    """tests/cpp/test_lbankmix_mirror.cpp calls the four methods of brutefir_hip.hpp; compiled, not linked."""
    if not shutil.which("g++"):
        pytest.skip("no g++ on this machine")
    hpp = open(os.path.join(ROOT, "foo-dsp-bfir_amd", "host", "brutefir_hip.hpp")).read()
    src = os.path.join(ROOT, "tests", "cpp", "test_lbankmix_mirror.cpp")
    text = open(src).read()
    for meth in MIRROR:
        assert "int %s(" % meth in hpp, meth
        assert ".%s(" % meth in text, meth
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-c", src, "-o", str(tmp_path / "mirror.o")], check=True)


def test_mix_kernel_register_report():
    """The two k_lbank_mix instances (float, double) have no scratch, no spill, no dynamic stack and no LDS; their names carry
    none of the substrings other tests count kernels by, and those counts are what they were."""
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc on this machine")
    import importlib
    import sys
    sys.path.insert(0, ROOT)
    b = importlib.import_module("foo_dsp_bfir_amd._build")
    assert "lbankmix.hip" in b.SOURCES
    b.build()
    u = b.resource_usage()
    got = [name for name in u if "k_lbank_mix" in name]
    assert len(got) == 2, got
    for name in got:
        r = u[name]
        for other in COUNTED + ("k_bank_mix",):
            assert other not in name, name
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["Dynamic Stack"] == "False", (name, r)
        assert r["LDS Size"] == 0, (name, r)
    # the counts asserted in test_lbank.py and test_bankmix.py
    assert sum("k_lbank_gather" in k for k in u) == 1 and sum("k_bank_mix" in k for k in u) == 2
    assert sum("k_bank_gather" in k for k in u) == 1
    assert sum("k_mac_matrix" in k for k in u) == 20 and sum("k_mac_duo" in k for k in u) == 12
    assert sum("k_patch_pairs" in k for k in u) == 8


def test_level_mix_records_under_the_host_sanitizers(tmp_path):
    """tests/cpp/test_level_mix_tables.cpp includes coeff_tables.h alone; built with AddressSanitizer and
    UndefinedBehaviorSanitizer and run as a plain executable."""
    if not shutil.which("g++"):
        pytest.skip("no g++ on this machine")
    src = os.path.join(ROOT, "tests", "cpp", "test_level_mix_tables.cpp")
    includes = re.findall(r'^#\s*include\s+"([^"]+)"', open(src).read(), re.M)
    assert includes == ["../../foo-dsp-bfir_amd/csrc/coeff_tables.h"], includes
    exe = str(tmp_path / "test_level_mix_tables")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g",
                    src, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout[-4000:], p.stderr[-4000:])
    assert p.returncode == 0 and "ALL OK" in p.stdout and "FAIL" not in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


def test_the_host_has_one_copy_of_the_term_arithmetic():
    """level_mix_records reuses what mix_records does: the weight conversion and the liveness test stand once in the header,
    and engine.hip restates neither."""
    header = open(os.path.join(ROOT, "foo-dsp-bfir_amd", "csrc", "coeff_tables.h")).read()
    engine = open(os.path.join(ROOT, "foo-dsp-bfir_amd", "csrc", "engine.hip")).read()
    assert "inline int level_mix_records(" in header and "inline int mix_records(" in header
    assert (header + engine).count("const float wf = (float)w;") == 1
    assert (header + engine).count("// infinite in the working precision") == 1
    assert "level_mix_records(" in engine and "lbank_mix_gather(" in engine and "set_coeff_lbank_mix(" in engine


def test_the_shapes_lie_where_the_docstring_says():
    L, blocks, ratios = NEW_SHAPES["boundary"]
    assert blocks == (40, 3) and [t[0] for t in BOUNDARY_TERMS] == [33, 39, 40, 40] and [t[1] for t in BOUNDARY_TERMS] == [0, 0, 2, 3]
    for s, head, tail in ((4, 5120, 768), (8, 10240, 1536)):
        rows = row_bytes(L, blocks, ratios, s)
        part = 2 * L * s
        assert rows == [head, tail]
        assert tail < SPAN and SPAN % part == 0                                   # the tail row lies below a span
        lines = [c * part for c in (33, 39)]
        assert lines[0] // SPAN == lines[1] // SPAN and all(ln % SPAN for ln in lines)   # both lines inside ONE span
        assert (head - 1) // SPAN == lines[0] // SPAN                               # ... the row's last, which count 40 ends
        assert all(c <= blocks[0] and t <= blocks[1] for c, t in BOUNDARY_TERMS)
        assert max(t for _, t in BOUNDARY_TERMS) == blocks[1]                     # the last partition of the last level is reached
    L, blocks, ratios = NEW_SHAPES["partial"]
    for s, head_wg in ((4, 1.25), (8, 2.5)):
        rows = row_bytes(L, blocks, ratios, s)
        assert rows[0] == head_wg * PER and rows[0] % PER                         # the head's last workgroup is partly filled
        assert rows[1] % PER == 0 and workgroups(rows[1]) == 2 * s // 4           # the tail's are exactly filled
    # 9x10: the piece-to-level mapping has 2, 4 and 8 workgroups to tell apart
    s, L, blocks, ratios = SHAPES["9x10"][1][:4]
    rows = row_bytes(L, blocks, ratios, s)
    assert rows == [16 << 10, 32 << 10, 64 << 10] and [workgroups(r) for r in rows] == [2, 4, 8]
    # every partition is whole 16 bytes at every shape of the file
    shapes = [v[1][:4] for v in SHAPES.values()] + [(s,) + v for v in NEW_SHAPES.values() for s in (4, 8)]
    for s, L, blocks, ratios in shapes:
        Ls, _ = level_geometry(L, blocks, ratios)
        assert all((2 * Lk * s) % 16 == 0 for Lk in Ls)
    assert sorted(KINDS) == ["matrix", "mimo"]
