"""Two-level partitioned engines (bfir_engine_create_nup) without a GPU: the C ABI as declared and exported, its argument
checks, the definition the GPU tests rely on (two uniform oracle engines composed against one), and the register report
of the two back-end kernels."""
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
NUP_FNS = ("bfir_engine_create_nup", "bfir_engine_set_coeff_nup", "bfir_engine_read_coeff_nup")
F32, F64, S16 = 8, 10, 2

# The compiler's occupancy (waves per SIMD by registers) per k_inv_nup instance, by log2 of its N = 2L points, and the LDS
# footprint that bounds the workgroups per CU, as DESIGN.md "k_inv_nup" lists them.
NUP_OCCUPANCY = {10: 5, 11: 5, 12: 4, 13: 4, 14: 4}
NUP_LDS_BYTES = {10: 8464, 11: 16928, 12: 33856, 13: 67712, 14: 135424}


def nup_model(orc, L, Bh, r, Bt, s, Cn, h, x, in_fmt=None, out_fmt=None):
    """y_head + z[n - D] from two uniform oracle engines: head (L, Bh) on h[:D], tail (r L, Bt) on h[D:] run in blocks of
    r L from sample 0 (the input zero-padded to whole tail blocks).  float64 [frames, C]."""
    D, Lt = Bh * L, r * L
    dt = np.float64 if s == 8 else np.float32
    head = orc.Engine(L, Bh, s, Cn, in_fmt, out_fmt)
    assert head.set_coeff([np.ascontiguousarray(c[:D], dtype=dt) for c in h]) == 0
    rc, y = head.run(x)
    assert rc == 0
    y = np.asarray(y, dtype=np.float64).copy()
    head.close()
    if h[0].size > D:
        tail = orc.Engine(Lt, Bt, s, Cn, in_fmt, out_fmt)
        assert tail.set_coeff([np.ascontiguousarray(c[D:], dtype=dt) for c in h]) == 0
        n = x.shape[0]
        xp = np.zeros((-(-n // Lt) * Lt, Cn), x.dtype)
        xp[:n] = x
        rc, z = tail.run(xp)
        assert rc == 0
        tail.close()
        if n > D:
            y[D:] += np.asarray(z, dtype=np.float64)[:n - D]
    return y


def _decl(name):
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, open(HEADER).read(), re.S)
    assert m, name
    return m.group(1)


@pytest.mark.parametrize("name", NUP_FNS)
def test_header_declares_the_nup_functions(name):
    args = _decl(name)
    assert not re.search(r"\blong\b", args), args
    for a in args.split(","):
        assert re.match(r"\s*(const\s+)?(int|double|void|bfir_engine)\b", a), a


def test_library_exports_and_bindings(bfir):
    from foo_dsp_bfir_amd import _lib
    lib = bfir.load()
    for name in NUP_FNS:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).restype == _lib.SIGNATURES[name][0]
    if shutil.which("nm"):
        syms = subprocess.run(["nm", "-D", "--defined-only", bfir.library_path()], capture_output=True, text=True).stdout
        for name in NUP_FNS:
            assert re.search(r"\bT %s$" % name, syms, re.M), name
    assert issubclass(bfir.BrutefirNup, bfir.Brutefir)
    assert bfir.BrutefirNup.set_coeff is not bfir.Brutefir.set_coeff
    assert bfir.BrutefirNup.coeff_block is not bfir.Brutefir.coeff_block


def _create(lib, L, Bh, r, Bt, s, Cn, fi=F32, fo=F32):
    err = C.c_int(12345)
    h = lib.bfir_engine_create_nup(L, Bh, r, Bt, s, Cn, fi, fo, 0, C.byref(err))
    return h, err.value


@pytest.mark.parametrize("args", [
    (1024, 8, 3, 2, 4, 2),      # tail_ratio not a power of two
    (1024, 8, 1, 2, 4, 2),      # tail_ratio below 2
    (1024, 8, 0, 2, 4, 2),
    (1024, 3, 4, 2, 4, 2),      # head_blocks < tail_ratio
    (1024, 8, 8, 0, 4, 2),      # tail_blocks < 1
    (1024, 8, 8, 2, 4, 0),      # channels
    (1024, 8, 8, 2, 4, 9),
    (1024, 8, 8, 2, 2, 2),      # realsize
    (1000, 8, 8, 2, 4, 2),      # not a power of two
], ids=lambda a: "-".join(map(str, a)))
def test_argument_refusals(bfir, args):
    h, err = _create(bfir.load(), *args)
    assert not h and err == bfir.ERR_ARG


@pytest.mark.parametrize("args", [
    (8, 4, 2, 2, 4, 2, F32, F32),            # L below what bfir_engine_create takes
    (32768, 4, 2, 2, 4, 2, F32, F32),        # L above
    (8192, 4, 4, 2, 4, 2, F32, F32),         # the tail's 32768 above
    (8192, 2, 2, 2, 8, 2, F64, F64),         # fp64: the tail's 16384 above
    (16384, 2, 2, 2, 8, 2, F64, F64),
    (1024, 8, 8, 2, 4, 2, S16, F32),         # frame formats
    (1024, 8, 8, 2, 4, 2, F32, S16),
    (1024, 8, 8, 2, 4, 2, 9, F32),           # FLOAT_BE
], ids=lambda a: "-".join(map(str, a)))
def test_unsupported_sizes_and_formats(bfir, args):
    h, err = _create(bfir.load(), *args)
    assert not h and err == bfir.ERR_UNSUPPORTED


def test_valid_arguments_reach_the_device_check(bfir):
    lib = bfir.load()
    for args in [(1024, 8, 8, 2, 8, 2, F32, F32), (16, 2, 2, 1, 4, 1, F32, F32), (4096, 4, 4, 1, 4, 8, F32, F64),
                 (4096, 2, 2, 3, 8, 3, F64, F64)]:
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
    assert lib.bfir_engine_set_coeff_nup(None, ptrs, 1, 4, 1.0) == bfir.ERR_ARG
    assert lib.bfir_engine_read_coeff_nup(None, 0, 0, 0, taps.ctypes.data) == bfir.ERR_ARG


def test_cpp_mirror_with_a_two_level_caller_compiles(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++ on this machine")
    src = tmp_path / "caller.cpp"
    src.write_text('#include "%s"\n'
                   "int two(void **h) { brutefir f(1024, brutefir::two_level{8, 8, 31}, 8, 2, 8, 8); return f.set_coeff(h, 2, 262144, 1.0); }\n"
                   % os.path.join(ROOT, "foo-dsp-bfir_amd", "host", "brutefir_hip.hpp"))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", str(src)], check=True)


# (s, L, Bh, r, Bt, C): head blocks a multiple of r and not, one channel and an odd count, both precisions
MODEL_SHAPES = [(4, 64, 2, 2, 3, 1), (8, 64, 4, 2, 5, 3), (4, 16, 2, 2, 3, 1), (4, 64, 5, 4, 3, 2), (8, 32, 8, 8, 2, 2),
                (8, 64, 4, 4, 1, 2)]


@pytest.mark.parametrize("shape", MODEL_SHAPES, ids=lambda a: "-".join(map(str, a)))
def test_two_levels_compose_to_the_uniform_engine(orc, shape):
    """Head oracle (L, Bh) on h[:D] plus tail oracle (r L, Bt) on h[D:], delayed by D, equals the uniform oracle
    (L, ceil(taps / L)) and the direct convolution: the definition the GPU tests hold the engine to."""
    s, L, Bh, r, Bt, Cn = shape
    dt = np.float64 if s == 8 else np.float32
    D, Lt = Bh * L, r * L
    taps = D + (Bt - 1) * Lt + Lt // 3 + 1                              # ends inside the last tail partition
    nb = Bh + r * (Bt + 2) + 3
    rng = np.random.default_rng(sum(shape))
    h = orc.synth_ir(rng, Cn, taps, dt)
    x = orc.synth_audio(rng, nb * L, Cn, dt)
    uni = orc.Engine(L, -(-taps // L), s, Cn)
    assert uni.set_coeff(h) == 0
    rc, want = uni.run(x)
    assert rc == 0
    uni.close()
    y = nup_model(orc, L, Bh, r, Bt, s, Cn, h, x)
    assert rel_err(y, want) <= TOL[s]
    direct = np.stack([orc.direct_conv(x[:, c].astype(np.float64), np.asarray(h[c], np.float64)) for c in range(Cn)], axis=1)
    assert rel_err(y, direct) <= TOL[s]
    # head-only filters: the model is the head engine alone
    y0 = nup_model(orc, L, Bh, r, Bt, s, Cn, [c[:D - 3] for c in h], x)
    assert rel_err(y0, np.stack([orc.direct_conv(x[:, c].astype(np.float64), np.asarray(h[c][:D - 3], np.float64))
                                 for c in range(Cn)], axis=1)) <= TOL[s]


def test_nup_kernel_register_report():
    """Every k_inv_nup / k_nup_combine instance: no scratch, no spill, no dynamic stack, LDS within 160 KB; one k_inv_nup
    per pair plan size; occupancy and LDS as DESIGN.md records them, so a later regression shows."""
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc on this machine")
    import importlib
    import sys
    sys.path.insert(0, ROOT)
    b = importlib.import_module("foo_dsp_bfir_amd._build")
    b.build()
    u = b.resource_usage()
    inv = {k: v for k, v in u.items() if "k_inv_nup" in k}
    comb = {k: v for k, v in u.items() if "k_nup_combine" in k}
    assert len(inv) == 5, sorted(inv)
    assert len(comb) == 4, sorted(comb)                      # float / double x 16 bytes per lane / one sample per lane
    for name, r in list(inv.items()) + list(comb.items()):
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["Dynamic Stack"] == "False", (name, r)
        assert r["LDS Size"] <= 160 * 1024, (name, r)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name, r in inv.items():
        lg = int(re.search(r"k_inv_nupILi(\d+)E", name).group(1))
        assert r["Occupancy"] == NUP_OCCUPANCY[lg] and r["LDS Size"] == NUP_LDS_BYTES[lg], (name, r)
        assert re.search(r"\|\s*%d\s*\|\s*%d\s*\|\s*%d\s*\|\s*%d\s*\|" % (1 << lg, r["VGPRs"], NUP_LDS_BYTES[lg], NUP_OCCUPANCY[lg]),
                         design), lg
    for r in comb.values():
        assert r["Occupancy"] == 8 and r["LDS Size"] == 0, r
