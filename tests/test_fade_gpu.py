"""Crossfaded coefficient changes on the GPU (bfir_engine_set_coeff_fade / _matrix_fade / _fade_remaining).

The expected output is built from what oracle/ has: two oracle engines with the old and the new filters on the same input,
blended in float64 with the ramp of fftw_convolver::convolver_crossfade_inplace stretched over K blocks
(test_fade.fade_expected; matrix engines: test_matrix.matrix_reference twice).  Tolerances are the project's own: TOL and
rel_err of conftest, the LSB rule of test_formats_gpu for integer outputs, and 1e-6 where an fp64 engine writes float32
frames (test_matrix_gpu: the frame format's own rounding, 2^-24, bounds that case, not the arithmetic).  They apply unchanged
because the blend is a convex combination of two signals that each meet them, plus three roundings."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import TOL, rel_err
from test_fade import fade_expected, fade_weights
from test_matrix import matrix_reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64, S16, S24 = 8, 10, 2, 4
MODES = ("one", "small", "three", "chunk2", "device")


def _real(s):
    return np.float64 if s == 8 else np.float32


def _frames_dtype(fmt):
    return np.float64 if fmt == F64 else np.float32


def _tol(s, out_fmt):
    return 1e-6 if (s == 8 and out_fmt == F32) else TOL[s]


@pytest.fixture()
def log(bfir):
    from foo_dsp_bfir_amd import _lib
    lines = []
    cb = _lib.LOG_FN(lambda msg: lines.append(msg.decode(errors="replace")))
    lib = bfir.load()
    lib.bfir_set_log_callback(cb)
    yield lines
    lib.bfir_set_log_callback(_lib.LOG_FN())


def _path(lines):
    made = [ln for ln in lines if ln.startswith("bfir engine: ")]
    assert len(made) == 1, lines
    return dict(kv.split("=") for kv in made[0].split(". ")[-1].split())


def _filters(orc, rng, Cn, L, B, s, gain=1.0):
    dt = _real(s)
    taps = B * L - (L // 3 + 1)                                          # ragged tail
    return [[(h * gain).astype(dt) for h in orc.synth_ir(rng, Cn, taps, dt)] for _ in range(2)]


def feed(eng, x, L, t0, start_fade, mode="one"):
    """Blocks 0 .. t0-1 in one call, start_fade(), then the rest cut as `mode` says.  Returns (rcs, frames)."""
    nb = x.shape[0] // L
    rcs, outs = [], []
    if t0:
        rc, y = eng.run(x[:t0 * L]); rcs.append(rc); outs.append(y)
    start_fade()
    if mode == "device":
        import torch
        d_in = torch.from_numpy(np.ascontiguousarray(x[t0 * L:])).cuda()
        width = outs[0].shape[1] if outs else x.shape[1]
        d_out = torch.zeros((d_in.shape[0], width), dtype=torch.from_numpy(outs[0][:1]).dtype, device="cuda")
        torch.cuda.synchronize()
        eng.run_device(d_in.data_ptr(), d_out.data_ptr(), nb - t0)
        rcs.append(eng.sync()); outs.append(d_out.cpu().numpy())
    else:
        step = {"one": nb - t0, "chunk2": nb - t0, "small": 1, "three": 3}[mode]
        for b in range(t0, nb, step):
            rc, y = eng.run(x[b * L:min(nb, b + step) * L]); rcs.append(rc); outs.append(y)
    return rcs, np.concatenate(outs)


def _engine(bfir, L, B, s, Cn, in_fmt, out_fmt, h, mode="one"):
    eng = bfir.Brutefir(L, B, s, Cn, in_fmt, out_fmt)
    if mode == "chunk2":
        eng.set_chunk(2)
    assert eng.set_coeff(h) == 0
    return eng


# (id, realsize, C, L, B, in_fmt, out_fmt, path, layout)
PATHS = [
    ("pair-2ch", 4, 2, 1024, 3, F32, F32, "pair", "pairs"),
    ("pair-8ch", 4, 8, 1024, 3, F32, F32, "pair", "pairs"),
    ("pair-largest", 4, 2, 8192, 2, F32, F32, "pair", "pairs"),          # k_inv_fade<14>
    ("time-pair-3ch", 4, 3, 512, 3, F32, F32, "time-pair", "pairs"),
    ("time-pair-1ch", 4, 1, 512, 3, F32, F32, "time-pair", "pairs"),
    ("direct-grouped-f32", 4, 1, 128, 3, F32, F32, "direct", "grouped"),
    ("staging-pairs", 4, 3, 256, 3, F32, F32, "staging", "pairs"),
    ("general-16384", 4, 2, 16384, 2, F32, F32, "staging", "pairs"),     # past the pair plans: the general back end
    ("f64-run-kernels", 8, 2, 1024, 8, F32, F32, "direct", "pairs"),     # the plug-in's shape with a short impulse
    ("f64-grouped", 8, 3, 64, 3, F64, F64, "direct", "grouped"),
    ("f64-frames", 8, 2, 1024, 3, F64, F64, "direct", "pairs"),
    ("f32-f64-frames", 4, 2, 1024, 3, F64, F64, None, "pairs"),
    ("s16-out", 4, 2, 1024, 3, F32, S16, "staging", "pairs"),
    ("s24-out", 8, 2, 256, 3, F32, S24, "staging", "grouped"),
]


@pytest.mark.parametrize("K", [1, 3, 7])
@pytest.mark.parametrize("case", PATHS, ids=[p[0] for p in PATHS])
def test_fade_on_every_path(orc, bfir, log, case, K):
    _, s, Cn, L, B, in_fmt, out_fmt, path, layout = case
    rng = np.random.default_rng(L * 7 + Cn * 3 + s + K + out_fmt)
    nb, t0 = 2 * B + K + 3, B + 1
    h_old, h_new = _filters(orc, rng, Cn, L, B, s)
    x = orc.synth_audio(rng, nb * L, Cn, _frames_dtype(in_fmt))
    del log[:]
    eng = _engine(bfir, L, B, s, Cn, in_fmt, out_fmt, h_old)
    got = _path(log)
    assert (path is None or got["path"] == path) and got["layout"] == layout, got
    rcs, y = feed(eng, x, L, t0, lambda: _ok(eng.set_coeff_fade(h_new, K)))
    assert all(rc == 0 for rc in rcs) and eng.fade_remaining() == 0
    if out_fmt >= 8:
        want, _, _ = fade_expected(orc, L, B, s, Cn, h_old, h_new, x, t0, K, in_fmt, out_fmt)
        err = rel_err(y, want)
        print("%s K=%d rel err %.3g (tol %.3g)" % (case[0], K, err, _tol(s, out_fmt)))
        assert err <= _tol(s, out_fmt)
    else:
        # integer frames: the blend happens in working precision after the output scale (full scale) and before the
        # conversion, so the expectation is the float-frame expectation times full scale, rounded
        ffmt = F64 if s == 8 else F32
        want, _, _ = fade_expected(orc, L, B, s, Cn, h_old, h_new, x, t0, K, in_fmt, ffmt)
        full = float(1 << (8 * orc.FMT_BYTES[out_fmt] - 1))
        a, b = orc.decode_ints(y, out_fmt), np.floor(want * full + 0.5).astype(np.int64)
        lsb_tol = max(1, int(np.ceil(TOL[s] * full)))                    # test_formats_gpu.py:81-82
        print("%s K=%d max LSB diff %d (tol %d)" % (case[0], K, np.abs(a - b).max(), lsb_tol))
        assert np.abs(a - b).max() <= lsb_tol
        if lsb_tol == 1:
            assert (a != b).mean() < 0.01
    eng.close()


def _ok(rc):
    assert rc == 0, rc


# engines whose bytes do not depend on how a run is cut: (id, realsize, C, L, B, frames)
CUT_FREE = [("pair", 4, 2, 1024, 4, F32), ("f64", 8, 2, 1024, 4, F64)]
OTHER_CUT_FREE = [("direct-f32", 4, 1, 128, 3, F32)]


@pytest.mark.parametrize("case", CUT_FREE, ids=[c[0] for c in CUT_FREE])
def test_fade_does_not_depend_on_the_cut(orc, bfir, case):
    _, s, Cn, L, B, fmt = case
    K = 7
    rng = np.random.default_rng(L + s)
    nb, t0 = 2 * B + K + 3 + 3, B + 1
    h_old, h_new = _filters(orc, rng, Cn, L, B, s)
    x = orc.synth_audio(rng, nb * L, Cn, _frames_dtype(fmt))
    want, _, _ = fade_expected(orc, L, B, s, Cn, h_old, h_new, x, t0, K, fmt, fmt)
    outs = {}
    for mode in MODES:
        eng = _engine(bfir, L, B, s, Cn, fmt, fmt, h_old, mode)
        rcs, y = feed(eng, x, L, t0, lambda: _ok(eng.set_coeff_fade(h_new, K)), mode)
        assert all(rc == 0 for rc in rcs), (mode, rcs)
        assert rel_err(y, want) <= TOL[s], mode
        outs[mode] = y.tobytes()
        eng.close()
    assert all(outs[m] == outs["one"] for m in MODES), [m for m in MODES if outs[m] != outs["one"]]


@pytest.mark.parametrize("mode", ["small", "three", "chunk2"])
def test_time_pair_fade_survives_the_cut(orc, bfir, mode):
    s, Cn, L, B, K = 4, 3, 512, 3, 7
    rng = np.random.default_rng(99)
    nb, t0 = 2 * B + K + 4, B + 1
    h_old, h_new = _filters(orc, rng, Cn, L, B, s)
    x = orc.synth_audio(rng, nb * L, Cn, np.float32)
    want, _, _ = fade_expected(orc, L, B, s, Cn, h_old, h_new, x, t0, K)
    eng = _engine(bfir, L, B, s, Cn, F32, F32, h_old, mode)
    rcs, y = feed(eng, x, L, t0, lambda: _ok(eng.set_coeff_fade(h_new, K)), mode)
    assert all(rc == 0 for rc in rcs) and rel_err(y, want) <= TOL[s]
    eng.close()


@pytest.mark.parametrize("case", CUT_FREE + OTHER_CUT_FREE + [("time-pair", 4, 3, 512, 3, F32)],
                         ids=[c[0] for c in CUT_FREE + OTHER_CUT_FREE] + ["time-pair"])
def test_outside_the_fade_nothing_changes(orc, bfir, case):
    """Before t0: the bytes of an engine that never faded.  From t0 + K: the bytes of an engine that called plain set_coeff
    with the new filters right before block t0 + K.  Time-pair engines (their bytes depend on the cut): within TOL."""
    name, s, Cn, L, B, fmt = case
    K = 3
    rng = np.random.default_rng(L + s + Cn)
    nb, t0 = 2 * B + K + 3, B + 1
    h_old, h_new = _filters(orc, rng, Cn, L, B, s)
    x = orc.synth_audio(rng, nb * L, Cn, _frames_dtype(fmt))
    fading = _engine(bfir, L, B, s, Cn, fmt, fmt, h_old)
    _, y = feed(fading, x, L, t0, lambda: _ok(fading.set_coeff_fade(h_new, K)))
    plain = _engine(bfir, L, B, s, Cn, fmt, fmt, h_old)
    _, y_plain = plain.run(x)
    cut = _engine(bfir, L, B, s, Cn, fmt, fmt, h_old)
    _, y_cut = feed(cut, x, L, t0 + K, lambda: _ok(cut.set_coeff(h_new)))
    a, b = t0 * L, (t0 + K) * L
    if name == "time-pair":
        assert rel_err(y[:a], y_plain[:a]) <= TOL[s] and rel_err(y[b:], y_cut[b:]) <= TOL[s]
    else:
        assert y[:a].tobytes() == y_plain[:a].tobytes()
        assert y[b:].tobytes() == y_cut[b:].tobytes()
    assert not np.array_equal(y[a:b], y_plain[a:b]) and not np.array_equal(y[a:b], y_cut[a:b])
    for e in (fading, plain, cut):
        e.close()


@pytest.mark.parametrize("case", CUT_FREE + [("staging", 4, 3, 256, 3, F32)], ids=["pair", "f64", "staging"])
def test_identity_fade(orc, bfir, case):
    _, s, Cn, L, B, fmt = case
    K = 3
    rng = np.random.default_rng(7 + L)
    nb, t0 = 2 * B + K + 3, B + 1
    h, _ = _filters(orc, rng, Cn, L, B, s)
    x = orc.synth_audio(rng, nb * L, Cn, _frames_dtype(fmt))
    eng = _engine(bfir, L, B, s, Cn, fmt, fmt, h)
    _, y = feed(eng, x, L, t0, lambda: _ok(eng.set_coeff_fade(h, K)), "three")
    plain = _engine(bfir, L, B, s, Cn, fmt, fmt, h)
    _, y_plain = plain.run(x)
    for t in range(nb):
        assert rel_err(y[t * L:(t + 1) * L], y_plain[t * L:(t + 1) * L]) <= TOL[s], t
    eng.close(); plain.close()


# ---- matrix engines ------------------------------------------------------------------------------------------------
def _rows(orc, rng, n_in, n_out, taps, s, null=()):
    dt = _real(s)
    rows = [[orc.synth_ir(rng, 1, taps, dt)[0] for _ in range(n_in)] for _ in range(n_out)]
    for o, i in null:
        rows[o][i] = None
    return rows


def _matrix_expected(orc, L, B, s, rows_old, rows_new, x, t0, K):
    w = fade_weights(L, x.shape[0] // L, t0, K)[:, None]
    return matrix_reference(orc, L, B, s, rows_old, x) * (1.0 - w) + matrix_reference(orc, L, B, s, rows_new, x) * w


@pytest.mark.parametrize("L,B,s,n_in,n_out,path", [(1024, 3, 4, 2, 2, "pair"), (256, 3, 4, 3, 2, "direct"),
                                                   (1024, 3, 8, 2, 2, "direct")])
@pytest.mark.parametrize("mode", ["one", "small"])
def test_matrix_fade_with_filters_appearing_and_disappearing(orc, bfir, log, L, B, s, n_in, n_out, path, mode):
    K = 3
    rng = np.random.default_rng(L + n_in + s)
    nb, t0 = 2 * B + K + 3, B + 1
    taps = B * L - (L // 3 + 1)
    fmt = F64 if s == 8 else F32
    rows_old = _rows(orc, rng, n_in, n_out, taps, s, null=((1, 0),))     # NULL -> present
    rows_new = _rows(orc, rng, n_in, n_out, taps, s, null=((0, 1),))     # present -> NULL
    x = orc.synth_audio(rng, nb * L, n_in, _real(s))
    del log[:]
    m = bfir.BrutefirMatrix(L, B, s, n_in, n_out, fmt, fmt)
    assert _path(log)["path"] == path
    assert m.set_coeff(rows_old) == 0
    # wrong kind of call
    assert bfir.Brutefir.set_coeff_fade(m, [r for r in rows_new[0] if r is not None], K) == bfir.ERR_UNSUPPORTED
    rcs, y = feed(m, x, L, t0, lambda: _ok(m.set_coeff_fade(rows_new, K)), mode)
    assert all(rc == 0 for rc in rcs) and m.fade_remaining() == 0
    assert rel_err(y, _matrix_expected(orc, L, B, s, rows_old, rows_new, x, t0, K)) <= TOL[s]
    assert not [ln for ln in log if "from the next block on" in ln]      # every input is read under both sets
    got = m.coeff_block(1, 0, 0)
    ref = orc.Engine(L, B, s, 1); ref.set_coeff([rows_new[1][0]])
    assert rel_err(got, ref.coeff_block(0, 0)) <= TOL[s]                 # the new set is the active one
    m.close()


def test_matrix_fade_to_a_set_that_leaves_an_input_unread(orc, bfir, log):
    """2 -> 2, pair path.  The new set reads input 0 only and input 1 carries NaN from block t0 + K on: the fade's blocks
    leave the pair path (an unread input may not share a transform with a read one), outputs stay finite."""
    L, B, s, K = 1024, 3, 4, 3
    rng = np.random.default_rng(21)
    nb, t0 = 2 * B + K + 3, B + 1
    taps = B * L - 11
    rows_old = _rows(orc, rng, 2, 2, taps, s)
    rows_new = _rows(orc, rng, 2, 2, taps, s, null=((0, 1), (1, 1)))
    x = orc.synth_audio(rng, nb * L, 2, np.float32)
    clean = x.copy()
    clean[(t0 + K) * L:, 1] = 0.0
    x[(t0 + K) * L:, 1] = np.nan
    del log[:]
    m = bfir.BrutefirMatrix(L, B, s, 2, 2, F32, F32)
    assert _path(log)["path"] == "pair"
    assert m.set_coeff(rows_old) == 0
    rcs, y = feed(m, x, L, t0, lambda: _ok(m.set_coeff_fade(rows_new, K)))
    assert all(rc == 0 for rc in rcs) and m.sync() == 0 and np.isfinite(y).all()
    switches = [ln for ln in log if "from the next block on" in ln]
    assert switches == ["bfir matrix engine: an input feeds no output: path=direct from the next block on."], log
    assert rel_err(y, _matrix_expected(orc, L, B, s, rows_old, rows_new, clean, t0, K)) <= TOL[s]
    # ... and back: every input read again under the new set, but not under the old one: direct through the fade, pair after it
    del log[:]
    assert m.run(orc.synth_audio(rng, (B + 2) * L, 2, np.float32))[0] == 0   # input 1's NaN leaves the delay line
    x2 = orc.synth_audio(rng, (K + 2) * L, 2, np.float32)
    assert m.set_coeff_fade(rows_old, K) == 0 and not [ln for ln in log if "from the next block on" in ln]
    rc, _ = m.run(x2)
    assert rc == 0
    assert [ln for ln in log if "from the next block on" in ln] == [
        "bfir matrix engine: every input feeds an output: path=pair from the next block on."], log
    m.close()


# ---- bookkeeping ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CUT_FREE, ids=["pair", "f64"])
def test_overflow_statistics_count_the_blended_samples(orc, bfir, case):
    _, s, Cn, L, B, fmt = case
    K = 3
    rng = np.random.default_rng(5 + s)
    nb, t0 = 2 * B + K + 3, B + 1
    h_old, h_new = _filters(orc, rng, Cn, L, B, s, gain=40.0)            # loud enough to clip
    x = orc.synth_audio(rng, nb * L, Cn, _frames_dtype(fmt))
    eng = _engine(bfir, L, B, s, Cn, fmt, fmt, h_old)
    rcs, y = feed(eng, x, L, t0, lambda: _ok(eng.set_coeff_fade(h_new, K)))
    assert all(rc == 0 for rc in rcs)
    fade_part = np.abs(y[t0 * L:(t0 + K) * L])
    assert (fade_part > 1.0).any()
    for c in range(Cn):
        of = eng.overflow(c)
        assert of.n_overflows == int((np.abs(y[:, c]) > 1.0).sum())
        assert of.largest == float(np.abs(y[:, c]).max())
    eng.reset()
    assert all(eng.overflow(c).n_overflows == 0 and eng.overflow(c).largest == 0.0 for c in range(Cn))
    eng.close()


@pytest.mark.parametrize("case", CUT_FREE + [("staging", 4, 3, 256, 3, F32)], ids=["pair", "f64", "staging"])
@pytest.mark.parametrize("mode", ["one", "small"])
def test_nan_in_sample_0_of_a_fade_block(orc, bfir, case, mode):
    _, s, Cn, L, B, fmt = case
    K = 3
    rng = np.random.default_rng(3)
    nb, t0 = 2 * B + K + 3, B + 1
    h_old, h_new = _filters(orc, rng, Cn, L, B, s)
    x = orc.synth_audio(rng, nb * L, Cn, _frames_dtype(fmt))
    x[(t0 + 1) * L, 0] = np.nan                                          # data, not an address: sample 0 of fade block 1
    eng = _engine(bfir, L, B, s, Cn, fmt, fmt, h_old)
    rcs, _ = feed(eng, x, L, t0, lambda: _ok(eng.set_coeff_fade(h_new, K)), mode)
    if mode == "one":
        assert rcs == [0, bfir.ERR_NONFINITE]
    else:
        assert rcs[:3] == [0, 0, bfir.ERR_NONFINITE]                     # blocks < t0, block t0, block t0 + 1
    eng.close()


# ---- state and errors ----------------------------------------------------------------------------------------------
def test_error_codes(orc, bfir):
    L, B, s, Cn = 1024, 2, 4, 2
    rng = np.random.default_rng(1)
    h, h2 = _filters(orc, rng, Cn, L, B, s)
    eng = bfir.Brutefir(L, B, s, Cn)
    assert eng.set_coeff_fade(h2, 3) == bfir.ERR_STATE                   # no coefficients yet
    assert eng.set_coeff(h) == 0
    assert eng.set_coeff_fade(h2, 0) == bfir.ERR_ARG and eng.set_coeff_fade(h2, -1) == bfir.ERR_ARG
    assert eng.set_coeff_fade(h2, (1 << 24) // L + 1) == bfir.ERR_ARG    # K L > 2^24
    assert eng.set_coeff_fade(h2, (1 << 24) // L) == 0                   # K L = 2^24 is allowed
    assert eng.set_coeff_fade(h2, 3) == bfir.ERR_STATE                   # a fade is pending
    assert eng.fade_remaining() == (1 << 24) // L
    eng.close()
    batch = bfir.Brutefir(L, B, s, Cn, n_engines=2)
    for g in range(2):
        assert batch.set_coeff(h, engine_index=g) == 0
    assert batch.set_coeff_fade(h2, 3) == bfir.ERR_UNSUPPORTED
    batch.close()
    dith = bfir.Brutefir(256, B, s, Cn, F32, S16, apply_dither=True)
    hd, hd2 = _filters(orc, rng, Cn, 256, B, s)
    assert dith.set_coeff(hd) == 0 and dith.set_coeff_fade(hd2, 3) == bfir.ERR_UNSUPPORTED
    dith.close()
    m = bfir.BrutefirMatrix(L, B, s, 2, 2)
    rows = [[h[0], h[1]], [h2[0], h2[1]]]
    assert m.set_coeff_fade(rows, 3) == bfir.ERR_STATE
    assert m.set_coeff(rows) == 0
    ptrs = (C.c_void_p * 4)(*[a.ctypes.data for r in rows for a in r])
    lib = bfir.load()
    assert lib.bfir_engine_set_coeff_fade(m.handle, ptrs, 2, h[0].size, B, 1.0, 3) == bfir.ERR_UNSUPPORTED
    m.close()
    d = bfir.Brutefir(L, B, s, Cn); assert d.set_coeff(h) == 0
    assert lib.bfir_engine_set_coeff_matrix_fade(d.handle, ptrs, h[0].size, B, 1.0, 3) == bfir.ERR_UNSUPPORTED
    d.close()


@pytest.mark.parametrize("case", CUT_FREE, ids=["pair", "f64"])
def test_states_of_a_fade(orc, bfir, case):
    _, s, Cn, L, B, fmt = case
    K = 5
    rng = np.random.default_rng(2 + s)
    nb = 2 * B + K + 6
    t0 = B + 1
    h_old, h_new = _filters(orc, rng, Cn, L, B, s)
    x = orc.synth_audio(rng, nb * L, Cn, _frames_dtype(fmt))
    blk = lambda y, a, b=None: y[a * L:(nb if b is None else b) * L]
    refs = {}
    for name, h in (("old", h_old), ("new", h_new)):
        ref = orc.Engine(L, B, s, Cn, fmt, fmt); ref.set_coeff(h)
        refs[name] = ref.run(x)[1].astype(np.float64)
        refs[name + "_spec"] = ref.coeff_block(1, 0)
    want, _, _ = fade_expected(orc, L, B, s, Cn, h_old, h_new, x, t0, K, fmt, fmt)

    # fade_remaining counts down across calls; read_coeff reads the old set until the last fade block is queued
    eng = _engine(bfir, L, B, s, Cn, fmt, fmt, h_old)
    assert eng.fade_remaining() == 0
    assert eng.run(blk(x, 0, t0))[0] == 0
    assert eng.set_coeff_fade(h_new, K) == 0 and eng.fade_remaining() == K
    seen, parts = [], []
    for t in range(t0, t0 + K):
        assert rel_err(eng.coeff_block(1, 0), refs["old_spec"]) <= TOL[s]
        rc, y = eng.run(blk(x, t, t + 1)); assert rc == 0
        parts.append(y); seen.append(eng.fade_remaining())
    assert seen == list(range(K - 1, -1, -1))
    assert rel_err(eng.coeff_block(1, 0), refs["new_spec"]) <= TOL[s]
    assert rel_err(np.concatenate(parts), blk(want, t0, t0 + K)) <= TOL[s]
    assert eng.set_coeff_fade(h_old, 2) == 0                             # the next fade may start once this one is done
    eng.close()

    # a plain set_coeff mid-fade cuts hard
    eng = _engine(bfir, L, B, s, Cn, fmt, fmt, h_old)
    assert eng.run(blk(x, 0, t0))[0] == 0 and eng.set_coeff_fade(h_new, K) == 0
    rc, y = eng.run(blk(x, t0, t0 + 2)); assert rc == 0 and eng.fade_remaining() == K - 2
    assert rel_err(y, blk(want, t0, t0 + 2)) <= TOL[s]
    assert eng.set_coeff(h_new) == 0 and eng.fade_remaining() == 0
    rc, y = eng.run(blk(x, t0 + 2)); assert rc == 0
    assert rel_err(y, blk(refs["new"], t0 + 2)) <= TOL[s]
    eng.close()

    # a NaN tap: BFIR_ERR_COEFF, the engine stays initialised and keeps running the old filters
    eng = _engine(bfir, L, B, s, Cn, fmt, fmt, h_old)
    assert eng.run(blk(x, 0, t0))[0] == 0
    bad = [h.copy() for h in h_new]; bad[1][5] = np.inf
    assert eng.set_coeff_fade(bad, K) == bfir.ERR_COEFF
    assert eng.is_initialized() and eng.fade_remaining() == 0
    rc, y = eng.run(blk(x, t0)); assert rc == 0
    assert rel_err(y, blk(refs["old"], t0)) <= TOL[s]
    eng.close()

    # reset mid-fade leaves the new set active (and starts a new run, as reset does)
    eng = _engine(bfir, L, B, s, Cn, fmt, fmt, h_old)
    assert eng.run(blk(x, 0, t0))[0] == 0 and eng.set_coeff_fade(h_new, K) == 0
    assert eng.run(blk(x, t0, t0 + 2))[0] == 0
    eng.reset()
    assert eng.fade_remaining() == 0 and rel_err(eng.coeff_block(1, 0), refs["new_spec"]) <= TOL[s]
    ref = orc.Engine(L, B, s, Cn, fmt, fmt); ref.set_coeff(h_new)      # the time history does not depend on the filters
    ref.run(blk(x, 0, t0 + 2)); ref.reset()
    rc, y = eng.run(blk(x, t0 + 2)); assert rc == 0
    assert rel_err(y, ref.run(blk(x, t0 + 2))[1]) <= TOL[s]
    eng.close()


# ---- the C++ mirror -------------------------------------------------------------------------------------------------
def _fnv1a(data):
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return h


def test_cpp_mirror_fades_like_the_ctypes_engine(tmp_path, bfir):
    """tests/cpp/test_fade_mirror.cpp builds its input and filters from integer recurrences (restated here), fades once
    through brutefir::set_coeff_fade with one run() per block and prints the FNV-1a hash of its output bytes."""
    src = os.path.join(ROOT, "tests", "cpp", "test_fade_mirror.cpp")
    exe = str(tmp_path / "test_fade_mirror")
    libdir = os.path.dirname(bfir.library_path())
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", src, "-o", exe, "-L" + libdir, "-lbfir_hip",
                    "-Wl,-rpath," + libdir], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "ALL OK" in p.stdout
    L, B, Cn, taps, t0, K, nb = 1024, 2, 2, 1500, 2, 3, 8
    i = np.arange(nb * L * Cn, dtype=np.uint64)
    x = ((((i * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(8)).astype(np.float64) / 16777216.0 - 0.5)
    x = x.astype(np.float32).reshape(nb * L, Cn)

    def taps_of(c, salt):
        n = np.arange(taps, dtype=np.uint64)
        v = (((n + np.uint64(1)) * np.uint64(40503 * (c + 3) + salt)) & np.uint64(0xffff)).astype(np.float64) / 65536.0 - 0.5
        return (v / (8.0 * (1.0 + n.astype(np.float64)))).astype(np.float32)

    h_old = [taps_of(c, 0) for c in range(Cn)]
    h_new = [taps_of(c, 977) for c in range(Cn)]
    eng = bfir.Brutefir(L, B, 4, Cn)
    assert eng.set_coeff(h_old) == 0
    rcs, y = feed(eng, x, L, t0, lambda: _ok(eng.set_coeff_fade(h_new, K)), "small")
    # feed() runs blocks < t0 in one call; the mirror runs them one by one: the same bytes on the pair path
    assert all(rc == 0 for rc in rcs)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("checksum ")]
    assert line and int(line[0].split()[1], 16) == _fnv1a(y.tobytes())
    eng.close()
