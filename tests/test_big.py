"""Long-partition engines (bfir_engine_create_big) without a GPU: the C ABI as declared and exported, the bindings, the
argument checks that need no device, the split every size gets (csrc/bigconv.hip against DESIGN.md) and the C++ mirror."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bfir_hip.h")
HOST = os.path.join(ROOT, "foo-dsp-bfir_amd", "host")
MIRROR = os.path.join(ROOT, "tests", "cpp", "test_big_mirror.cpp")


def test_header_declares_create_big():
    m = re.search(r"\bbfir_engine_create_big\s*\(([^;]*)\)\s*;", open(HEADER).read(), re.S)
    assert m
    args = m.group(1)
    assert not re.search(r"\blong\b", args), args
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == [
        "filter_length", "filter_blocks", "realsize", "channels", "in_format", "out_format", "sampling_rate", "apply_dither",
        "device", "err"]
    for a in args.split(","):
        assert re.match(r"\s*int\b", a), a


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler on this machine")
    src = tmp_path / "use.c"
    src.write_text('#include "bfir_hip.h"\n'
                   "bfir_engine *make(int *err) { return bfir_engine_create_big(65536, 16, 4, 8, 8, 8, 44100, 0, 0, err); }\n")
    subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)],
                   check=True)


def test_library_exports_and_bindings(bfir):
    from foo_dsp_bfir_amd import _lib
    lib = bfir.load()
    name = "bfir_engine_create_big"
    assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES[name] == _lib.SIGNATURES["bfir_engine_create"]            # the same arguments, another kind
    assert getattr(lib, name).restype == _lib.SIGNATURES[name][0]
    if shutil.which("nm"):
        syms = subprocess.run(["nm", "-D", "--defined-only", bfir.library_path()], capture_output=True, text=True).stdout
        assert re.search(r"\bT %s$" % name, syms, re.M)
    assert issubclass(bfir.BrutefirBig, bfir.Brutefir)
    assert "BrutefirBig" in bfir.__all__


@pytest.mark.parametrize("args,err", [
    ((40000, 2, 4, 2, 8, 8), "ERR_ARG"),            # not a power of two
    ((65536, 2, 2, 2, 8, 8), "ERR_ARG"),            # realsize
    ((65536, 0, 4, 2, 8, 8), "ERR_ARG"),            # no partitions
    ((65536, 2, 4, 9, 8, 8), "ERR_ARG"),            # channels
    ((16384, 2, 4, 2, 8, 8), "ERR_UNSUPPORTED"),    # bfir_engine_create's
    ((8192, 2, 8, 2, 10, 10), "ERR_UNSUPPORTED"),
    ((2097152, 2, 4, 2, 8, 8), "ERR_UNSUPPORTED"),  # past the range
    ((2097152, 2, 8, 2, 10, 10), "ERR_UNSUPPORTED"),
    ((1048576, 1024, 4, 1, 8, 8), "ERR_UNSUPPORTED"),   # one channel's delay line past 2^31 samples
])
def test_arguments_are_checked_before_the_device(bfir, args, err):
    lib = bfir.load()
    code = C.c_int(0)
    L, B, s, Cn, fin, fout = args
    assert not lib.bfir_engine_create_big(L, B, s, Cn, fin, fout, 44100, 0, 0, C.byref(code))
    assert code.value == getattr(bfir, err)


def test_split_per_size_matches_the_design():
    """M1 x M2 of every size: what big_split computes (restated from its three thresholds), the instances the two macros
    build, and the table in DESIGN.md."""
    src = open(os.path.join(ROOT, "foo-dsp-bfir_amd", "csrc", "bigconv.hip")).read()
    m1 = [int(v) for v in re.findall(r"F\((\d+)\)", re.search(r"#define BIG_FOR_LOG2M1\(F\)(.*)", src).group(1))]
    m2 = [int(v) for v in re.findall(r"F\((\d+)\)", re.search(r"#define BIG_FOR_LOG2M2\(F\)(.*)", src).group(1))]
    assert re.search(r"lg <= 16 \? 4 : lg <= 18 \? 6 : 8", src)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for lg in range(14, 21):
        l1 = 4 if lg <= 16 else 6 if lg <= 18 else 8
        assert l1 in m1 and lg - l1 in m2, lg
        assert (1 << l1) <= 256 and (1 << (lg - l1)) <= 4096
        assert re.search(r"\|\s*%d\s*\|\s*%d\s*[x×]\s*%d\s*\|" % (1 << lg, 1 << l1, 1 << (lg - l1)), design), lg


def test_cpp_mirror_with_a_big_caller_compiles():
    if not shutil.which("g++"):
        pytest.skip("no g++ on this machine")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", HOST, "-I", os.path.dirname(HEADER), MIRROR],
                   check=True)
