"""Per-channel delays without a device: the sub-sample filters of bfir_subdelay_filter against the reference's own
firwindow_kaiser (tests/golden/kaiser_window_ref.json, recorded by make_kaiser_golden.py), its argument checks, and
that the header, the binding and the build know the five new entry points."""
import base64
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bfir_hip.h")
FIXTURE = os.path.join(ROOT, "tests", "golden", "kaiser_window_ref.json")
NEW = ("bfir_subdelay_filter", "bfir_engine_delay_init", "bfir_engine_set_delay", "bfir_engine_get_delay",
       "bfir_engine_delay_latency")


def _cases():
    return json.load(open(FIXTURE))["cases"]


def _arr(text, realsize):
    return np.frombuffer(base64.b64decode(text), dtype="<f4" if realsize == 4 else "<f8")


def _case_id(c):
    return "len%d_%+d_%d_b%g_r%d" % (c["len"], c["n"], c["steps"], c["beta"], c["realsize"])


def test_fixture_covers_the_cases_and_its_weights_explain_the_library_taps(bfir):
    cases = _cases()
    assert os.path.getsize(FIXTURE) < 100 * 1024
    seen = {(c["len"], c["n"], c["steps"], c["beta"], c["realsize"]) for c in cases}
    for length in (3, 9, 33, 63):
        for steps in (2, 10, 100):
            for n in (1, -1, steps - 1, -(steps - 1)):
                for beta in (9.0, 4.5):
                    for realsize in (4, 8):
                        assert (length, n, steps, beta, realsize) in seen
    for c in cases:   # the weights alone, recorded on an array of ones: the library's taps are sinc x weights, to a few roundings
        ones = _arr(c["ones"], c["realsize"])
        taps = bfir.subdelay_filter(c["len"] >> 1, c["n"], c["steps"], c["beta"], c["realsize"])
        assert ones.size == taps.size == c["len"] == _arr(c["sinc"], c["realsize"]).size
        h, off = c["len"] >> 1, c["n"] / c["steps"]
        x = math.pi * (np.arange(c["len"]) - h - off)
        eps = 2.0 ** -23 if c["realsize"] == 4 else 2.0 ** -52
        assert np.abs(taps - np.sin(x) / x * ones).max() <= 8 * eps


@pytest.mark.parametrize("case", _cases(), ids=_case_id)
def test_subdelay_filter_against_the_reference_window(bfir, case):
    """The mirror performs the reference's double operations in the reference's order, so only FMA contraction could
    differ (that would allow 4 * 2^-52 * max |taps| for realsize 8 and one float ulp per tap for realsize 4).  The
    library's host code is built without contraction across statements and for the baseline x86-64 instruction set:
    the taps are bit-equal to the reference's, for all 160 cases, and equality is what is asserted."""
    rs = case["realsize"]
    want = _arr(case["sinc"], rs)
    got = bfir.subdelay_filter(case["len"] >> 1, case["n"], case["steps"], case["beta"], rs)
    assert got.dtype == want.dtype and got.size == want.size
    assert np.array_equal(got, want), float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())


@pytest.mark.parametrize("realsize", [4, 8])
@pytest.mark.parametrize("h", [1, 4, 128])
def test_subdelay_zero_is_a_unit_tap(bfir, realsize, h):
    taps = bfir.subdelay_filter(h, 0, 10, 9.0, realsize)
    want = np.zeros(2 * h + 1)
    want[h] = 1.0
    assert taps.dtype == (np.float32 if realsize == 4 else np.float64)
    assert np.array_equal(taps, want) and not np.signbit(taps).any()


def test_kaiser_beta_is_honoured(bfir):
    """A deviation from the reference, which passes the literal 9 (delay.cpp:304)."""
    a, b = bfir.subdelay_filter(16, 3, 10, 9.0, 8), bfir.subdelay_filter(16, 3, 10, 4.5, 8)
    assert np.abs(a - b).max() > 1e-3
    assert abs(a.sum() - 1.0) < 1e-3   # a delay filter: unit gain at DC


def test_subdelay_filter_errors(bfir):
    lib = bfir.load()
    buf = (C.c_double * 300)()
    ok = dict(h=4, sub=3, steps=10, beta=9.0, rs=8)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.bfir_subdelay_filter(a["h"], a["sub"], a["steps"], a["beta"], a["rs"], a.get("taps", buf))

    assert call() == 0
    assert call(taps=None) == bfir.ERR_ARG
    for steps in (1, 0, -3):
        assert call(steps=steps, sub=0) == bfir.ERR_ARG
    for h in (0, -1, 129):
        assert call(h=h) == bfir.ERR_ARG
    assert call(h=128) == 0 and call(h=1) == 0
    for sub in (10, -10, 11, -400):
        assert call(sub=sub) == bfir.ERR_ARG
    assert call(sub=9) == 0 and call(sub=-9) == 0
    for rs in (0, 2, 16):
        assert call(rs=rs) == bfir.ERR_ARG
    assert call(rs=4) == 0
    with pytest.raises(bfir.BfirError) as ei:
        bfir.subdelay_filter(4, 10, 10)
    assert ei.value.code == bfir.ERR_ARG


def test_header_declares_and_documents_the_delay_calls(bfir):
    src = open(HEADER).read()
    bare = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, bare), name
    assert re.search(r"#define BFIR_DELAY_INPUT\s+0", src) and re.search(r"#define BFIR_DELAY_OUTPUT\s+1", src)
    # every entry cites the reference lines it replaces, and the deviations are stated
    for cite in ("delay.cpp:278-306", "firwindow.c:89-210", "delay.cpp:56-140", "delay.cpp:27-54", "delay.cpp:304",
                 "delay.cpp:158-161", "delay.cpp:585-596"):
        assert cite in src, cite
    assert "repeats samples" in src and "kaiser_beta is honoured" in src
    from importlib import import_module
    sigs = import_module("foo_dsp_bfir_amd._lib").SIGNATURES
    lib = bfir.load()
    for name in NEW:
        assert name in sigs and hasattr(lib, name)
    for m in ("delay_init", "set_delay", "get_delay", "delay_latency"):
        for cls in (bfir.Brutefir, bfir.BrutefirMatrix, bfir.BrutefirNup, bfir.BrutefirLevels, bfir.BrutefirMatrixLevels):
            assert callable(getattr(cls, m))
    assert (bfir.DELAY_INPUT, bfir.DELAY_OUTPUT) == (0, 1)


def test_delay_source_is_built_and_mirrored():
    from importlib import import_module
    build = import_module("foo_dsp_bfir_amd._build")
    assert "delay.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "delay.hip"))
    hpp = open(os.path.join(ROOT, "foo-dsp-bfir_amd", "host", "brutefir_hip.hpp")).read()
    for name in NEW:
        assert name in hpp, name


def test_delay_kernels_use_no_scratch():
    """The compiler's own per-kernel report, recorded at build time (_build.resource_usage): every instance of the two
    delay kernels runs out of registers alone."""
    import shutil
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc on this machine")
    from importlib import import_module
    build = import_module("foo_dsp_bfir_amd._build")
    build.build()
    u = {k: v for k, v in build.resource_usage().items() if "k_delay_" in k}
    assert any("k_delay_copy" in k for k in u) and any("k_delay_sub" in k for k in u), sorted(u)
    for name, r in u.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["Dynamic Stack"] == "False", (name, r)


def test_null_engine_is_an_argument_error(bfir):
    lib = bfir.load()
    d = (C.c_int * 8)()
    assert lib.bfir_engine_delay_init(None, 0, 16, 0, 0, 9.0) == bfir.ERR_ARG
    assert lib.bfir_engine_set_delay(None, 0, d, d, 2) == bfir.ERR_ARG
    assert lib.bfir_engine_get_delay(None, 0, d, d, 2) == bfir.ERR_ARG
    assert lib.bfir_engine_delay_latency(None, 0) == bfir.ERR_ARG
