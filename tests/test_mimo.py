"""Mimo engines (bfir_engine_create_mimo: up to 64 inputs -> 64 outputs in one matrix) without a GPU: the C ABI as declared
and exported, the bindings, the refusals that need no device, the grouped-oracle reference the GPU tests use, and the
register budget of k_mac_mimo (csrc/mimo.hip) as DESIGN.md tabulates it."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bfir_hip.h")
NAME = "bfir_engine_create_mimo"
ORC_MAXCH = 8   # channels of one oracle engine (oracle/bfir_oracle.h)


def test_header_declares_create_mimo_without_long():
    text = open(HEADER).read()
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % NAME, text, re.S)
    assert m, NAME
    assert not re.search(r"\blong\b", m.group(1)), m.group(1)
    for a in m.group(1).split(","):
        assert re.match(r"\s*(const\s+)?(int|int64_t|double|void|bfir_engine)\b", a), a
    assert re.search(r"#define\s+BFIR_MIMO_MAXCHANNELS\s+64\b", text)
    assert re.search(r"#define\s+BFIR_MAXCHANNELS\s+8\b", text)


def test_library_exports_and_bindings(bfir):
    from foo_dsp_bfir_amd import _lib
    lib = bfir.load()
    assert NAME in _lib.SIGNATURES
    assert _lib.SIGNATURES[NAME] == _lib.SIGNATURES["bfir_engine_create_matrix"]
    assert getattr(lib, NAME).restype == _lib.SIGNATURES[NAME][0]
    if shutil.which("nm"):
        syms = subprocess.run(["nm", "-D", "--defined-only", bfir.library_path()], capture_output=True, text=True).stdout
        assert re.search(r"\bT %s$" % NAME, syms, re.M)
    assert "BrutefirMimo" in bfir.__all__ and issubclass(bfir.BrutefirMimo, bfir.BrutefirMatrix)
    hpp = open(os.path.join(ROOT, "foo-dsp-bfir_amd", "host", "brutefir_hip.hpp")).read()
    assert NAME in hpp and "m_last[BFIR_MIMO_MAXCHANNELS]" in hpp


def test_refusals_need_no_device(bfir):
    """Checked before any device is looked for: counts outside 1 .. 64, integer and big-endian frames, a partition length
    outside the uniform engine's range.  Valid arguments get as far as the device."""
    lib = bfir.load()
    cases = [((256, 2, 4, 0, 2, 8, 8), bfir.ERR_ARG), ((256, 2, 4, 65, 2, 8, 8), bfir.ERR_ARG),
             ((256, 2, 4, 2, 0, 8, 8), bfir.ERR_ARG), ((256, 2, 4, 2, 65, 8, 8), bfir.ERR_ARG),
             ((256, 2, 4, 2, 2, 2, 8), bfir.ERR_UNSUPPORTED), ((256, 2, 4, 2, 2, 8, 2), bfir.ERR_UNSUPPORTED),
             ((256, 2, 4, 2, 2, 9, 8), bfir.ERR_UNSUPPORTED), ((256, 2, 4, 2, 2, 8, 9), bfir.ERR_UNSUPPORTED),
             ((32768, 2, 4, 2, 2, 8, 8), bfir.ERR_UNSUPPORTED), ((16384, 2, 8, 2, 2, 10, 10), bfir.ERR_UNSUPPORTED),
             ((8, 2, 4, 2, 2, 8, 8), bfir.ERR_UNSUPPORTED)]
    for args, want in cases:
        err = C.c_int(0)
        assert not lib.bfir_engine_create_mimo(*args, 0, C.byref(err))
        assert err.value == want, (args, err.value)
    if lib.bfir_device_count() == 0:
        for args in ((256, 2, 4, 64, 64, 8, 8), (1024, 3, 8, 9, 17, 10, 10)):
            err = C.c_int(0)
            assert not lib.bfir_engine_create_mimo(*args, 0, C.byref(err))
            assert err.value == bfir.ERR_NO_DEVICE, (args, err.value)
    # the matrix engine keeps its own limit
    err = C.c_int(0)
    assert not lib.bfir_engine_create_matrix(256, 2, 4, 9, 2, 8, 8, 0, C.byref(err)) and err.value == bfir.ERR_ARG


def mimo_reference(orc, L, B, s, rows, x):
    """y[:, o] = sum_i (x_i convolved with h_{o,i}) for any number of inputs: per output, oracle engines over groups of at
    most 8 inputs (the oracle's limit) with that output's filters, NULL filters and shorter ones padded with zeros, all
    their channels summed in float64.  A group without any filter contributes nothing."""
    fmt = 10 if s == 8 else 8
    dt = np.float64 if s == 8 else np.float32
    n_in = x.shape[1]
    given = [h.size for r in rows for h in r if h is not None]
    taps = max(given) if given else 1
    xs = np.ascontiguousarray(x, dtype=dt)
    out = np.zeros((x.shape[0], len(rows)))
    for o, row in enumerate(rows):
        for g0 in range(0, n_in, ORC_MAXCH):
            grp = row[g0:g0 + ORC_MAXCH]
            if all(h is None for h in grp):
                continue
            hs = []
            for h in grp:
                z = np.zeros(taps, dt)
                if h is not None:
                    z[:h.size] = h
                hs.append(z)
            e = orc.Engine(L, B, s, len(grp), fmt, fmt)
            assert e.set_coeff(hs) == 0
            rc, y = e.run(np.ascontiguousarray(xs[:, g0:g0 + len(grp)]))
            assert rc == 0
            out[:, o] += y.astype(np.float64).sum(axis=1)
            e.close()
    return out


def test_reference_is_the_sum_of_direct_convolutions(orc):
    """10 -> 3 (two oracle groups per output) with ragged taps and one NULL filter, against orc.direct_conv."""
    L, B, n_in, n_out = 64, 3, 10, 3
    nb = 2 * B + 3
    rng = np.random.default_rng(64)
    rows = [[orc.synth_ir(rng, 1, B * L - 13 - 5 * ((o + i) % 4), np.float64)[0] for i in range(n_in)] for o in range(n_out)]
    rows[1][8] = None
    x = orc.synth_audio(rng, nb * L, n_in, np.float64)
    y = mimo_reference(orc, L, B, 8, rows, x)
    want = np.zeros_like(y)
    for o, row in enumerate(rows):
        for i, h in enumerate(row):
            if h is not None:
                want[:, o] += orc.direct_conv(x[:, i], h)
    assert np.abs(y - want).max() <= 1e-12 * np.abs(want).max()


# k_mac_mimo<T, ILV, NO, TT> as DESIGN.md ("k_mac_mimo", the register table) lists them, with the waves per SIMD stated there:
# float: pairs / groups x 1, 2, 4 outputs x the one-block form and 8-block tiles; double: x 1, 2 outputs x one block and 8 / 4
MIMO_INSTANCES = {
    ("f", 0, 1, 1): 8, ("f", 0, 2, 1): 8, ("f", 0, 4, 1): 8, ("f", 1, 1, 1): 8, ("f", 1, 2, 1): 8, ("f", 1, 4, 1): 8,
    ("f", 0, 1, 8): 7, ("f", 0, 2, 8): 7, ("f", 0, 4, 8): 4, ("f", 1, 1, 8): 7, ("f", 1, 2, 8): 5, ("f", 1, 4, 8): 4,
    ("d", 0, 1, 1): 8, ("d", 0, 2, 1): 8, ("d", 1, 1, 1): 8, ("d", 1, 2, 1): 8,
    ("d", 0, 1, 8): 4, ("d", 0, 2, 4): 6, ("d", 1, 1, 8): 4, ("d", 1, 2, 4): 5,
}


def test_mac_mimo_register_budget():
    """The k_mac_mimo instances are exactly those of DESIGN.md's table; none has scratch, a spill, a dynamic stack or LDS,
    and each has the waves per SIMD the table states.  The counted names of the other kernels stay what they were."""
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc on this machine")
    import importlib
    import sys
    sys.path.insert(0, ROOT)
    b = importlib.import_module("foo_dsp_bfir_amd._build")
    b.build()
    u = b.resource_usage()
    got = {}
    for name, r in u.items():
        if "k_mac_mimo" not in name:
            continue
        m = re.search(r"k_mac_mimoI([fd])Lb([01])ELi(\d+)ELi(\d+)E", name)
        assert m, name
        for other in ("k_mac_matrix", "k_mac_duo", "k_inv_", "k_delay_"):
            assert other not in name, name
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["Dynamic Stack"] == "False", (name, r)
        assert r["LDS Size"] == 0, (name, r)
        got[(m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)))] = r["Occupancy"]
    assert got == MIMO_INSTANCES, sorted(set(got.items()) ^ set(MIMO_INSTANCES.items()))
    assert sum("k_mac_matrix" in k for k in u) == 20 and sum("k_mac_duo" in k for k in u) == 12
