"""Multi-level mimo engines on the GPU (bfir_engine_create_mimo_levels, BrutefirMimoLevels): up to 64 inputs -> 64 outputs,
every filter split between two or three levels; k_mac_mimo as the MAC of every level past 8 channels and k_wduo
(csrc/wduo.hip, BFIR_MFADE_DUO=1) for the launches of a crossfade that need both filter sets.

The reference is test_mlevels.uniform_reference -- one uniform oracle engine per output, summed over the inputs in float64 --
taken over groups of at most 8 inputs, the oracle's channel limit (test_mimo_levels.wide_reference), compared with rel_err <=
TOL of conftest and 1e-6 where fp64 arithmetic runs on FLOAT_LE frames, as in test_mlevels_gpu.py; a fade against the blend
of two such references with test_fade.fade_weights.  Runs are test_levels_gpu._nb blocks long, so every delay line and ring
wraps, with set_chunk(3) among them.  Run as a program (python tests/test_mimo_levels_gpu.py data.npz out.npz) this file
is the child process of the BFIR_MFADE_DUO comparison: the variable is read when an engine is created."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import TOL, rel_err
from test_fade import fade_weights
from test_levels import level_geometry
from test_levels_gpu import _nb, _taps
from test_mimo_levels import wide_reference
from test_mlevels import pad_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = 8, 10
LV3 = ((4, 2, 2), (1, 4, 2))                                             # at L = 512: 4 x 512, 2 x 2048, 2 x 4096

# (realsize, L, blocks, ratios, n_in, n_out), frame format (None = the working precision's), back end
CASES = {
    "9x3": ((4, 16, (2, 2, 3), (1, 2, 2), 9, 3), None, "general"),       # grouped layout, first input past 8, odd outputs
    "10x12": ((4, 512) + LV3 + (10, 12), None, "fused"),                 # pair front end, fused back end, two rings, outputs past 8
    "3x9": ((4, 512) + LV3 + (3, 9), None, "fused"),                     # the lone-output kernel on output 8
    "9x2-f64": ((8, 64, (2, 2), (1, 2), 9, 2), None, "general"),         # fp64
    "9x2-f64f": ((8, 64, (2, 2), (1, 2), 9, 2), F32, "general"),         # ... on FLOAT_LE frames
}
FADE = {                                                                 # the crossfade: 9 -> 10 on three levels, and the other layouts of k_wduo
    "9x10": ((4, 512) + LV3 + (9, 10), None),                            # (re, im) pairs, direct front end, k_inv_lfade
    "9x3": CASES["9x3"][:2],                                             # grouped layout, general back end
    "9x2-f64": CASES["9x2-f64"][:2],                                     # fp64
}


def _real(s):
    return np.float64 if s == 8 else np.float32


def _fmt(s, fmt):
    return (F64 if s == 8 else F32) if fmt is None else fmt


def _tol(s, fmt):
    return 1e-6 if (s == 8 and _fmt(s, fmt) == F32) else TOL[s]


def _lv(shape):
    return shape[:4] + (shape[4],)


def _geo(shape):
    Ls, D = level_geometry(shape[1], shape[2], shape[3])
    return Ls, D, [Lk // shape[1] for Lk in Ls]


def _lengths(shape, null=(), new=False):
    """Tap counts per filter, spread over the levels: filter j = o n_in + i ends on level (n - 1 - j) mod n -- the first one
    inside the last partition of the last level (test_levels_gpu._taps) -- in turn inside the last and the first partition of
    its level, a few taps apart.  new: the set a fade goes to, j shifted by one, so every filter changes its level."""
    s, L, blocks, ratios, n_in, n_out = shape
    Ls, D, _ = _geo(shape)
    n = len(blocks)
    lens = []
    for o in range(n_out):
        row = []
        for i in range(n_in):
            if (o, i) in null:
                row.append(None)
                continue
            j = o * n_in + i + (1 if new else 0)
            k = (n - 1 - j) % n
            last = blocks[k] - 1 if (j // n) % 2 == 0 else 0
            row.append(D[k] + last * Ls[k] + Ls[k] // 3 + 1 - j % 3 - (1 if new else 0))
        lens.append(row)
    return lens


def _rows(orc, shape, lens, seed=0, gain=1.0):
    s = shape[0]
    rng = np.random.default_rng(9000 + shape[1] + sum(shape[2]) + 10 * shape[4] + shape[5] + seed)
    return [[None if n is None else (orc.synth_ir(rng, 1, n, _real(s))[0] * gain).astype(_real(s)) for n in r] for r in lens]


def _audio(orc, shape, fmt=None, nb=None, seed=0):
    s, L = shape[0], shape[1]
    rng = np.random.default_rng(9500 + L + shape[4] + seed)
    dt = np.float64 if _fmt(s, fmt) == F64 else np.float32
    return orc.synth_audio(rng, (nb or _nb(_lv(shape))) * L, shape[4], dt)


_REF = {}


def _ref(orc, key, shape, rows, x):
    """The reference of (rows, x), computed once per key and shared read-only."""
    if key not in _REF:
        y = wide_reference(orc, shape[1], shape[0], rows, x)
        y.setflags(write=False)
        _REF[key] = y
    return _REF[key]


def _engine(bfir, shape, rows, fmt=None, chunk=3, cls=None):
    s, L, blocks, ratios, n_in, n_out = shape
    eng = (cls or bfir.BrutefirMimoLevels)(L, blocks, ratios, s, n_in, n_out, fmt, fmt)
    if chunk is not None:
        eng.set_chunk(chunk)
    assert not eng.is_initialized()
    if rows is not None:
        assert eng.set_coeff(rows) == 0 and eng.is_initialized()
    return eng


@pytest.fixture()
def log(bfir):
    from foo_dsp_bfir_amd import _lib
    lines = []
    cb = _lib.LOG_FN(lambda msg: lines.append(msg.decode(errors="replace")))
    lib = bfir.load()
    lib.bfir_set_log_callback(cb)
    yield lines
    lib.bfir_set_log_callback(_lib.LOG_FN())


def _case(orc, case):
    shape, fmt, _ = CASES[case]
    null = ((shape[5] - 1, 0),)
    lens = _lengths(shape, null)
    rows = _rows(orc, shape, lens)
    x = _audio(orc, shape, fmt)
    return shape, fmt, lens, rows, x


# ---- parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_parity_with_the_uniform_reference(orc, bfir, log, case):
    shape, fmt, lens, rows, x = _case(orc, case)
    s, L, blocks, ratios, n_in, n_out = shape
    Ls, D, _ = _geo(shape)
    flat = [n for r in lens for n in r if n is not None]
    for k in range(len(blocks)):                                         # at least one filter ends in every level
        assert any(D[k] < n <= D[k + 1] for n in flat), (k, flat)
    assert max(flat) == _taps(_lv(shape)) and min(flat) > 0
    want = _ref(orc, ("parity", case), shape, rows, x)
    eng = _engine(bfir, shape, rows, fmt, chunk=3)
    names = ", ".join("%d x %d" % (Lk, b) for Lk, b in zip(Ls, blocks))
    made = [ln for ln in log if ln.startswith("bfir engine: mimo %d -> %d, %d levels, %s;" % (n_in, n_out, len(blocks), names))]
    assert made and made[0].endswith("back end %s; MAC k_mac_mimo." % CASES[case][2]), log
    layouts = [ln.split("layout=")[1].split()[0] for ln in log if ln.startswith("bfir engine: mimo") and "layout=" in ln]
    assert layouts == ["pairs" if (s == 4 and Lk >= 256) else "grouped" for Lk in Ls], log
    rc, y = eng.run(x)
    assert rc == 0 and y.shape == (x.shape[0], n_out)
    err = rel_err(y, want)
    print("rel_err", case, err, "tol", _tol(s, fmt))
    assert err <= _tol(s, fmt)
    eng.close()


def _banded(o, i, n):
    """Three filters per output, wrapping round; output 5 has none."""
    return o != 5 and (i - o) % n < 3


def test_64_to_64_banded_with_overflow_records(orc, bfir):
    """64 -> 64 with a band of 3 filters per output that wraps round, lengths spread over both levels, loud enough to clip;
    one output without any filter comes out as zeros; the overflow records of every output against numpy counts."""
    shape = (4, 64, (2, 2), (1, 2), 64, 64)
    s, L, blocks, ratios, n, _ = shape
    Ls, D, _ = _geo(shape)
    null = {(o, i) for o in range(n) for i in range(n) if not _banded(o, i, n)}
    lens = _lengths(shape, null)
    flat = [v for r in lens for v in r if v is not None]
    assert all(sum(v is not None for v in r) == (0 if o == 5 else 3) for o, r in enumerate(lens))
    assert any(v <= D[1] for v in flat) and any(v > D[1] for v in flat)
    assert all(any(lens[o][i] is not None for o in range(n)) for i in range(n))     # every input is read
    rows = _rows(orc, shape, lens, gain=40.0)
    x = _audio(orc, shape)
    ref = _ref(orc, "64x64", shape, rows, x)
    eng = _engine(bfir, shape, rows, chunk=3)
    rc, y = eng.run(x)
    assert rc == 0
    err = rel_err(y, ref)
    print("rel_err 64x64", err)
    assert err <= TOL[s]
    assert not y[:, 5].any()                                             # the output without any filter: zeros
    counts = []
    for o in range(n):
        of = eng.overflow(o)
        peak = np.abs(ref[:, o]).max()
        assert of.max == 1.0 and of.n_overflows == int(np.count_nonzero(np.abs(y[:, o].astype(np.float64)) > 1.0)), o
        assert abs(of.largest - peak) <= TOL[s] * max(1.0, peak) * 10, o
        counts.append(of.n_overflows)
    print("overflows", counts)
    assert sum(counts[8:]) > 0 and counts[5] == 0
    for ch in (-1, n):
        with pytest.raises(bfir.BfirError) as ei:
            eng.overflow(ch)
        assert ei.value.code == bfir.ERR_ARG
    eng.close()


# ---- the byte identities of the header ---------------------------------------------------------------------------------
def test_identity_1_within_eight_channels_the_matrix_levels_engine(orc, bfir, monkeypatch):
    """2 -> 3: the bytes of BrutefirMatrixLevels, plain and through a fade, with the default MAC and with k_mac_mimo forced."""
    shape = (4, 512) + LV3 + (2, 3)
    L = shape[1]
    old, new = _rows(orc, shape, _lengths(shape, ((2, 0),))), _rows(orc, shape, _lengths(shape, ((1, 1),), new=True), seed=1)
    t0, K = 11, 5
    x = _audio(orc, shape, nb=t0 + K + 11)

    def run(cls):
        eng = _engine(bfir, shape, old, cls=cls)
        rc, a = eng.run(x[:t0 * L]); assert rc == 0
        assert eng.fade_to_rows(new, K) == 0
        rc, b = eng.run(x[t0 * L:]); assert rc == 0
        eng.close()
        return np.concatenate([a, b]).tobytes()
    want = run(bfir.BrutefirMatrixLevels)
    assert run(bfir.BrutefirMimoLevels) == want
    monkeypatch.setenv("BFIR_MIMO_MAC", "1")
    assert run(bfir.BrutefirMimoLevels) == want
    monkeypatch.setenv("BFIR_MFADE_DUO", "1")
    assert run(bfir.BrutefirMimoLevels) == want


def test_identity_2_filters_that_end_by_d1_the_mimo_engine(orc, bfir):
    shape = CASES["10x12"][0]
    s, L, blocks, ratios, n_in, n_out = shape
    _, D, _ = _geo(shape)
    rng = np.random.default_rng(23)
    x = _audio(orc, shape)
    rows = [[None if (o, i) == (11, 0) else orc.synth_ir(rng, 1, D[1] - (o + 3 * i) % 9, np.float32)[0] for i in range(n_in)]
            for o in range(n_out)]
    padded, taps = pad_rows(rows, np.float32)
    assert taps == D[1]
    small = bfir.BrutefirMimo(L, blocks[0], s, n_in, n_out)
    small.set_chunk(3)
    assert small.set_coeff(padded) == 0
    rc0, y0 = small.run(x)
    eng = _engine(bfir, shape, rows)
    rc, y = eng.run(x)
    assert rc == rc0 == 0 and y.tobytes() == y0.tobytes()
    for o in (0, 8, 11):
        assert eng.overflow(o).largest == small.overflow(o).largest
    eng.close(); small.close()


def _blocks16(orc):
    """16 -> 16 made of two 8 x 8 blocks on the diagonal, both with taps on every level."""
    shape = (4, 512) + LV3 + (16, 16)
    sub = (4, 512) + LV3 + (8, 8)
    parts = [_rows(orc, sub, _lengths(sub, ((7, 0),)), seed=g) for g in (0, 1)]
    rows = [[parts[o // 8][o % 8][i % 8] if o // 8 == i // 8 else None for i in range(16)] for o in range(16)]
    return shape, sub, parts, rows, _audio(orc, shape)


def test_identity_3_blocks_on_the_diagonal_the_matrix_levels_engines(orc, bfir):
    shape, sub, parts, rows, x = _blocks16(orc)
    eng = _engine(bfir, shape, rows)
    rc, y = eng.run(x)
    assert rc == 0
    eng.close()
    for g in (0, 1):
        m = _engine(bfir, sub, parts[g], cls=bfir.BrutefirMatrixLevels)
        rc, yg = m.run(np.ascontiguousarray(x[:, 8 * g:8 * g + 8]))
        assert rc == 0 and np.ascontiguousarray(y[:, 8 * g:8 * g + 8]).tobytes() == yg.tobytes(), g
        m.close()


@pytest.mark.parametrize("case", ["10x12", "9x3"])
def test_identity_4_how_the_blocks_arrive(orc, bfir, case):
    import torch
    shape, fmt, lens, rows, x = _case(orc, case)
    s, L, blocks, ratios, n_in, n_out = shape
    nb = x.shape[0] // L
    eng = _engine(bfir, shape, rows, chunk=None)                         # one call, the default chunk
    rc, one = eng.run(x)
    assert rc == 0
    eng.close()
    eng = _engine(bfir, shape, rows, chunk=3)
    rc, y = eng.run(x)
    assert rc == 0 and y.tobytes() == one.tobytes()
    eng.close()
    eng = _engine(bfir, shape, rows, chunk=None)                         # one block per call: the latency path
    parts = []
    for b in range(nb):
        rc, y = eng.run(x[b * L:(b + 1) * L]); assert rc == 0
        parts.append(y)
    assert np.concatenate(parts).tobytes() == one.tobytes()
    eng.close()
    eng = _engine(bfir, shape, rows, chunk=5)                            # device pointers, two calls that split a block of every level
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.zeros((nb * L, n_out), dtype=d_in.dtype, device="cuda")
    torch.cuda.synchronize()
    cut = _geo(shape)[2][-1] + 1
    isz = x.dtype.itemsize
    eng.run_device(d_in.data_ptr(), d_out.data_ptr(), cut)
    eng.run_device(d_in.data_ptr() + cut * L * n_in * isz, d_out.data_ptr() + cut * L * n_out * isz, nb - cut)
    assert eng.sync() == 0
    assert d_out.cpu().numpy().tobytes() == one.tobytes()
    eng.close()


# ---- the crossfade -----------------------------------------------------------------------------------------------------
T0 = 11                                                                  # an odd head block, inside a block of every level (1, 4 / 2, 8 / 4)
KS = (1, 5)
_FADE = {}


def _fade_data(orc, name):
    """rows_old, rows_new (the NULL pair moves, every filter changes its level, both sets read every input and reach every
    level), x of the longest run and the two references: computed once, read-only."""
    if name not in _FADE:
        shape, fmt = FADE[name]
        n_out = shape[5]
        old = _rows(orc, shape, _lengths(shape, ((n_out - 1, 0),)))
        new = _rows(orc, shape, _lengths(shape, ((0, 1),), new=True), seed=1)
        x = _audio(orc, shape, fmt, nb=T0 + max(KS) + _geo(shape)[2][-1] + 3)
        ys = tuple(wide_reference(orc, shape[1], shape[0], r, x) for r in (old, new))
        for a in (x,) + ys:
            a.setflags(write=False)
        _FADE[name] = (old, new, x, ys)
    return _FADE[name]


def _faded(eng, x, L, t0, rows_new, K):
    """Blocks [0, t0) in one call, fade_to_rows, the rest in one call."""
    rc, a = eng.run(x[:t0 * L]); assert rc == 0
    assert eng.fade_to_rows(rows_new, K) == 0 and eng.fade_remaining() == K
    rc, b = eng.run(x[t0 * L:]); assert rc == 0
    assert eng.fade_remaining() == 0
    return np.concatenate([a, b])


def _child_main(data, out):
    """The fades of every FADE shape and K on engines created in THIS process (BFIR_MFADE_DUO as the parent set it): the
    output frames and what the library said about the MAC of the launches that need both sets."""
    import foo_dsp_bfir_amd as bfir
    from foo_dsp_bfir_amd import _lib
    said = []
    cb = _lib.LOG_FN(lambda msg: said.append(msg.decode(errors="replace")))
    bfir.load().bfir_set_log_callback(cb)
    z = np.load(data, allow_pickle=True)
    res = {}
    for name in FADE:
        shape, fmt = FADE[name]
        old, new, x = z[name + ":old"].tolist(), z[name + ":new"].tolist(), z[name + ":x"]
        for K in KS:
            for chunk in (None, 3):
                eng = _engine(bfir, shape, old, fmt, chunk=chunk)
                res["%s:%d:%s" % (name, K, chunk)] = _faded(eng, x, shape[1], T0, new, K)
                eng.close()
    res["said"] = np.array([ln for ln in said if ln.startswith("bfir matrix engine: crossfade over")])
    np.savez(out, **res)


def _obj(rows):
    """rows as an array np.savez takes: one list of filters per output."""
    a = np.empty(len(rows), dtype=object)
    for o, r in enumerate(rows):
        a[o] = list(r)
    return a


@pytest.fixture(scope="module")
def duo_children(orc, tmp_path_factory):
    """The child process with BFIR_MFADE_DUO=0 and the one with =1: {switch: its results}."""
    tmp = tmp_path_factory.mktemp("mfade_duo")
    data = {}
    for name in FADE:
        old, new, x, _ = _fade_data(orc, name)
        data[name + ":old"], data[name + ":new"], data[name + ":x"] = _obj(old), _obj(new), x
    np.savez(str(tmp / "data.npz"), **data)
    out = {}
    for duo in ("0", "1"):
        env = dict(os.environ, BFIR_MFADE_DUO=duo)
        dst = str(tmp / ("out%s.npz" % duo))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), str(tmp / "data.npz"), dst], env=env, cwd=ROOT,
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
        out[duo] = dict(np.load(dst, allow_pickle=True))
    return out


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", sorted(FADE))
def test_fade_parity_and_the_bytes_outside_it(orc, bfir, duo_children, name, K):
    shape, fmt = FADE[name]
    s, L = shape[0], shape[1]
    old, new, x, ys = _fade_data(orc, name)
    nb = x.shape[0] // L
    eng = _engine(bfir, shape, old, fmt)
    y = _faded(eng, x, L, T0, new, K)
    eng.close()
    w = fade_weights(L, nb, T0, K)[:, None]
    err = rel_err(y, ys[0] * (1.0 - w) + ys[1] * w)
    print("rel_err", name, "K", K, err, "tol", _tol(s, fmt))
    assert err <= _tol(s, fmt)
    plain = []
    for rows in (old, new):
        eng = _engine(bfir, shape, rows, fmt)
        rc, p = eng.run(x); assert rc == 0
        plain.append(p); eng.close()
    assert np.array_equal(y[:T0 * L], plain[0][:T0 * L])                 # before a_f: an engine that never faded
    assert np.array_equal(y[(T0 + K) * L:], plain[1][(T0 + K) * L:])     # from a_f + K on: the new set all along
    mid = slice(T0 * L + 1, (T0 + K) * L - 1)
    assert not np.array_equal(y[mid], plain[0][mid]) and not np.array_equal(y[mid], plain[1][mid])
    # BFIR_MFADE_DUO=0 and =1, each in a process of its own, one call and set_chunk(3): the bytes of this process's engine
    for chunk in (None, 3):
        key = "%s:%d:%s" % (name, K, chunk)
        assert duo_children["0"][key].tobytes() == duo_children["1"][key].tobytes() == y.tobytes(), key


def test_the_switch_chose_the_kernels_in_the_children(duo_children):
    n = len(FADE) * len(KS) * 2
    for duo, kernel in (("0", "k_mac_mimo twice"), ("1", "k_wduo")):
        said = list(duo_children[duo]["said"])
        assert len(said) == n and all(ln.endswith("runs %s." % kernel) for ln in said), said


def test_fade_refusals_and_the_count_down(orc, bfir):
    name = "9x3"
    shape, fmt = FADE[name]
    s, L, blocks, ratios, n_in, n_out = shape
    _, D, _ = _geo(shape)
    old, new, x, _ = _fade_data(orc, name)
    # a set with taps on a level the old set never reached: refused, nothing changes
    short = [[None if h is None else h[:min(h.size, D[2] - 3)] for h in r] for r in old]
    never = _engine(bfir, shape, short)
    rc, want = never.run(x); assert rc == 0
    never.close()
    eng = _engine(bfir, shape, short)
    rc, a = eng.run(x[:T0 * L]); assert rc == 0
    assert eng.fade_to_rows(new, 5) == bfir.ERR_UNSUPPORTED and eng.fade_remaining() == 0 and eng.is_initialized()
    # a NaN tap in the fade call: the engine keeps the old set
    bad = [[None if h is None else h.copy() for h in r] for r in short]
    bad[2][8][-1] = np.nan
    assert eng.fade_to_rows(bad, 5) == bfir.ERR_COEFF and eng.fade_remaining() == 0 and eng.is_initialized()
    rc, b = eng.run(x[T0 * L:]); assert rc == 0
    assert np.concatenate([a, b]).tobytes() == want.tobytes()
    eng.close()
    # the count-down, and a second fade while one runs
    eng = _engine(bfir, shape, old)
    assert eng.run(x[:T0 * L])[0] == 0
    assert eng.fade_to_rows(new, 5) == 0 and eng.fade_remaining() == 5
    assert eng.fade_to_rows(old, 2) == bfir.ERR_STATE
    assert eng.run(x[T0 * L:(T0 + 2) * L])[0] == 0 and eng.fade_remaining() == 3
    assert eng.fade_to_rows(old, 2) == bfir.ERR_STATE
    assert eng.run(x[(T0 + 2) * L:(T0 + 5) * L])[0] == 0 and eng.fade_remaining() == 0
    assert eng.fade_to_rows(old, 2) == 0 and eng.fade_remaining() == 2
    eng.close()
    # a NaN tap in the plain call: the engine is uninitialised
    eng = _engine(bfir, shape, old)
    nan = [[None if h is None else h.copy() for h in r] for r in old]
    nan[0][8][-2] = np.nan
    assert eng.set_coeff(nan) == bfir.ERR_COEFF and not eng.is_initialized()
    assert eng.run(x[:L])[0] == bfir.ERR_STATE
    eng.close()


# ---- unread input, refusals, read-back -----------------------------------------------------------------------------------
def test_a_nan_on_an_input_no_filter_reads_reaches_no_output(orc, bfir):
    shape, fmt, lens, rows, x = _case(orc, "10x12")
    s, L = shape[0], shape[1]
    _, D, _ = _geo(shape)
    sparse = [[None if i == 3 else h for i, h in enumerate(r)] for r in rows]
    clean = x.copy(); clean[:, 3] = 0
    bad = x.copy()
    bad[3 * L + 5, 3] = np.nan
    bad[(D[2] // L + 1) * L, 3] = np.nan                                 # sample 0 of a block, past D_2
    bad[-L + 7, 3] = np.inf
    eng = _engine(bfir, shape, sparse)
    rc, y = eng.run(bad)
    assert rc == 0 and np.all(np.isfinite(y))
    assert rel_err(y, _ref(orc, "sparse", shape, sparse, clean)) <= TOL[s]
    eng.close()


def test_refusals_change_nothing(orc, bfir):
    import torch
    shape, sub, parts, rows, x = _blocks16(orc)
    s, L, blocks, ratios, n_in, n_out = shape
    Ls, _, _ = _geo(shape)
    lib = bfir.load()
    U = bfir.ERR_UNSUPPORTED
    fresh = _engine(bfir, shape, rows, chunk=None)
    rc, want = fresh.run(x); assert rc == 0
    fresh.close()
    eng = _engine(bfir, shape, rows, chunk=None)
    for side in (0, 1):
        with pytest.raises(bfir.BfirError) as ei:
            eng.delay_init(side, 16)
        assert ei.value.code == U
        assert eng.set_delay(side, [0] * 16) == U and eng.delay_latency(side) == U
        d = (C.c_int * 16)()
        assert lib.bfir_engine_get_delay(eng.handle, side, d, d, 16) == U
    h = parts[0][0][0]
    ptrs = (C.c_void_p * 256)(*([h.ctypes.data] * 256))
    dst = np.zeros(2 * Ls[-1], np.float32)
    assert lib.bfir_engine_set_coeff(eng.handle, ptrs, n_in, 100, blocks[0], 1.0) == U
    assert lib.bfir_engine_set_coeff_at(eng.handle, 0, ptrs, n_in, 100, blocks[0], 1.0) == U
    assert lib.bfir_engine_read_coeff(eng.handle, 0, 0, dst.ctypes.data) == U
    assert lib.bfir_engine_set_coeff_matrix(eng.handle, ptrs, 100, blocks[0], 1.0) == U
    assert lib.bfir_engine_read_coeff_matrix(eng.handle, 0, 0, 0, dst.ctypes.data) == U
    assert lib.bfir_engine_set_coeff_fade(eng.handle, ptrs, n_in, 100, blocks[0], 1.0, 3) == U
    assert lib.bfir_engine_set_coeff_matrix_fade(eng.handle, ptrs, 100, blocks[0], 1.0, 3) == U
    assert lib.bfir_engine_fade_remaining(eng.handle) == U
    assert lib.bfir_engine_set_coeff_nup(eng.handle, ptrs, n_in, 100, 1.0) == U
    assert lib.bfir_engine_read_coeff_nup(eng.handle, 0, 0, 0, dst.ctypes.data) == U
    assert lib.bfir_engine_set_coeff_nup_fade(eng.handle, ptrs, n_in, 100, 1.0, 3) == U
    assert lib.bfir_engine_set_coeff_levels(eng.handle, ptrs, n_in, 100, 1.0) == U
    assert lib.bfir_engine_read_coeff_levels(eng.handle, 0, 0, 0, dst.ctypes.data) == U
    assert lib.bfir_engine_set_coeff_levels_fade(eng.handle, ptrs, n_in, 100, 1.0, 3) == U
    for call in (lambda: eng.set_coeff_fade(rows, 3), lambda: eng.fade_to(rows, 3)):
        with pytest.raises(bfir.BfirError) as ei:
            call()
        assert ei.value.code == U
    # a uniform mimo engine keeps refusing the matrix-levels calls, the matrix-levels kind its limit of 8
    other = bfir.BrutefirMimo(L, blocks[0], s, n_in, n_out)
    lens = (C.c_int * 256)(*([100] * 256))
    assert lib.bfir_engine_set_coeff_matrix_levels(other.handle, ptrs, lens, 1.0) == U
    assert lib.bfir_engine_set_coeff_matrix_levels_fade(other.handle, ptrs, lens, 1.0, 2) == U
    assert lib.bfir_engine_read_coeff_matrix_levels(other.handle, 0, 0, 0, 0, dst.ctypes.data) == U
    other.close()
    with pytest.raises(bfir.BfirError) as ei:
        bfir.BrutefirMatrixLevels(L, blocks, ratios, s, 9, 2)
    assert ei.value.code == bfir.ERR_ARG
    # a launch past k_mac_mimo's grid: refused before anything is allocated or queued (these buffers hold one block)
    d_in = torch.zeros((L, n_in), dtype=torch.float32, device="cuda")
    d_out = torch.zeros((L, n_out), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    huge = 1 << 23
    eng.set_chunk(huge)
    with pytest.raises(bfir.BfirError) as ei:
        eng.run_device(d_in.data_ptr(), d_out.data_ptr(), huge)
    assert ei.value.code == U
    assert eng.sync() == 0
    eng.set_chunk(0)
    assert eng.is_initialized() and eng.fade_remaining() == 0
    rc, y = eng.run(x)
    assert rc == 0 and y.tobytes() == want.tobytes()
    eng.close()


@pytest.mark.parametrize("case", ["9x3", "9x2-f64"])
def test_partition_spectra_past_eight_channels(orc, bfir, case):
    """read_coeff_matrix_levels of filters whose input is past 8 (and, 10 -> 12 below, whose output is) against the oracle's
    spectrum of that partition, grouped layout."""
    shape, fmt, lens, rows, x = _case(orc, case)
    _check_spectra(orc, bfir, shape, rows, [(o, 8) for o in range(shape[5]) if rows[o][8] is not None])


def test_partition_spectra_past_eight_outputs_in_the_pairs_layout(orc, bfir):
    shape, fmt, lens, rows, x = _case(orc, "10x12")
    _check_spectra(orc, bfir, shape, rows, [(8, 8), (11, 9), (9, 0)])


def _check_spectra(orc, bfir, shape, rows, pairs):
    s, L, blocks, ratios, n_in, n_out = shape
    Ls, D, _ = _geo(shape)
    eng = _engine(bfir, shape, rows, chunk=None)
    assert eng.D == D[:-1] and eng.max_taps == D[-1] and eng.lengths == Ls
    padded, _ = pad_rows(rows, _real(s))
    assert pairs
    for o, i in pairs:
        for level, (Lp, Bp) in enumerate(zip(Ls, blocks)):
            part = np.zeros(Bp * Lp, _real(s))
            seg = padded[o][i][D[level]:D[level + 1]]
            part[:seg.size] = seg
            ref = orc.Engine(Lp, Bp, s, 1)
            assert ref.set_coeff([part]) == 0
            for b in range(Bp):
                got = eng.coeff_block(level, o, i, b)
                assert got.size == 2 * Lp and rel_err(got, ref.coeff_block(0, b)) <= TOL[s], (level, o, i, b)
            ref.close()
    lib = bfir.load()
    dst = np.zeros(2 * Ls[-1], _real(s))
    for lv, o, i, b in [(len(blocks), 0, 0, 0), (0, n_out, 0, 0), (0, 0, n_in, 0), (0, 0, 0, blocks[0]), (1, -1, 0, 0)]:
        assert lib.bfir_engine_read_coeff_matrix_levels(eng.handle, lv, o, i, b, dst.ctypes.data) == bfir.ERR_ARG
    eng.close()


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    _child_main(sys.argv[1], sys.argv[2])
