"""Multi-level matrix engines on the GPU (bfir_engine_create_matrix_levels / _set_coeff_matrix_levels /
_read_coeff_matrix_levels): n inputs -> m outputs, one filter per pair, every filter split between two to four levels.

The reference is test_mlevels.uniform_reference: one uniform oracle engine (L, ceil(max taps / L)) per output, summed over
the inputs in float64, compared with rel_err <= TOL of conftest (1e-6 where fp64 arithmetic runs on FLOAT_LE frames, as in
test_matrix_gpu.py); test_mlevels pins the per-pair levels definition to it on the CPU.  Runs are test_levels_gpu._nb blocks
long, so every delay line and ring wraps, and set_chunk(3) makes chunks cross the block boundaries of the levels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import TOL, rel_err
from test_levels import level_geometry
from test_levels_gpu import _nb, _settle, _taps
from test_mlevels import pad_rows, uniform_reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = 8, 10

# (realsize, L, blocks, ratios, n_in, n_out), frame format (None = the working precision's), back end
CASES = {
    "1": ((4, 16, (2, 2, 3), (1, 2, 2), 2, 3), None, "general"),         # grouped layout, smallest sizes, D_1 = L_1
    "2": ((4, 512, (4, 2, 2), (1, 4, 2), 2, 2), None, "fused"),          # pair front end, the existing fused kernels, two rings
    "3": ((4, 512, (4, 2, 2), (1, 4, 2), 1, 2), None, "fused"),          # direct front end, fused back end: the new dispatch
    "4a": ((4, 512, (4, 2, 2), (1, 4, 2), 2, 3), None, "fused"),         # pair kernels plus the lone kernel
    "4b": ((4, 512, (4, 2, 2), (1, 4, 2), 2, 1), None, "fused"),         # the lone kernel alone
    "5": ((4, 512, (2, 2, 2, 2), (1, 2, 2, 2), 3, 3), None, "fused"),    # three rings in the lone kernel, every D_k = L_k
    "6": ((4, 512, (4, 2), (1, 4), 2, 3), None, "fused"),                # one ring: the two-level case
    "7": ((4, 1024, (4, 4, 1), (1, 4, 4), 2, 2), None, "fused"),         # L_2 = 16384, the tail in direct mode
    "8": ((8, 1024, (4, 2, 2), (1, 2, 2), 2, 2), None, "general"),       # fp64, reference precision
    "8f": ((8, 1024, (4, 2, 2), (1, 2, 2), 2, 2), F32, "general"),       # ... on FLOAT_LE frames
}


def _real(s):
    return np.float64 if s == 8 else np.float32


def _fmt(s, fmt):
    return (F64 if s == 8 else F32) if fmt is None else fmt


def _tol(s, fmt):
    return 1e-6 if (s == 8 and fmt == F32) else TOL[s]


def _lv(shape):
    """The shape as test_levels_gpu's helpers take it: (s, L, blocks, ratios, channels)."""
    return shape[:4] + (shape[4],)


def _geo(shape):
    s, L, blocks, ratios, n_in, n_out = shape
    Ls, D = level_geometry(L, blocks, ratios)
    return Ls, D, [Lk // L for Lk in Ls]


def _lengths(shape, null=()):
    """Per-filter tap counts spread over the levels: the first filter ends inside the last partition of the last level,
    the following ones in level 0, 1, ... in turn (each inside the last partition of its level, a tap shorter per round)."""
    s, L, blocks, ratios, n_in, n_out = shape
    Ls, D, _ = _geo(shape)
    n = len(blocks)
    order = [n - 1] + list(range(n - 1))
    lens, j = [], 0
    for o in range(n_out):
        row = []
        for i in range(n_in):
            if (o, i) in null:
                row.append(None)
                continue
            k = order[j % n]
            j += 1
            row.append(D[k] + (blocks[k] - 1) * Ls[k] + Ls[k] // 3 + 1 - (j // n))
        lens.append(row)
    assert lens[0][0] == _taps(_lv(shape)) or (0, 0) in null
    return lens


def _null(shape):
    """One NULL pair in every case with three or more filters."""
    n_in, n_out = shape[4], shape[5]
    return ((n_out - 1, 0),) if n_in * n_out >= 3 else ()


def _rows(orc, shape, seed=0, null=None, gain=1.0):
    s = shape[0]
    null = _null(shape) if null is None else null
    rng = np.random.default_rng(4000 + shape[1] + sum(shape[2]) + 10 * shape[4] + shape[5] + seed)
    return [[None if n is None else (orc.synth_ir(rng, 1, n, _real(s))[0] * gain).astype(_real(s)) for n in r]
            for r in _lengths(shape, null)]


def _audio(orc, shape, fmt=None, seed=0, nb=None):
    s, L = shape[0], shape[1]
    rng = np.random.default_rng(5000 + L + shape[4] + seed)
    dt = np.float64 if _fmt(s, fmt) == F64 else np.float32
    return orc.synth_audio(rng, (nb or _nb(_lv(shape))) * L, shape[4], dt)


_REF = {}


def _ref(orc, key, shape, rows, x):
    """The uniform reference of (rows, x), computed once per key and shared read-only."""
    if key not in _REF:
        y = uniform_reference(orc, shape[1], shape[0], rows, x)
        y.setflags(write=False)
        _REF[key] = y
    return _REF[key]


def _engine(bfir, shape, rows, fmt=None, chunk=3):
    s, L, blocks, ratios, n_in, n_out = shape
    eng = bfir.BrutefirMatrixLevels(L, blocks, ratios, s, n_in, n_out, fmt, fmt)
    if chunk is not None:
        eng.set_chunk(chunk)
    assert not eng.is_initialized()
    if rows is not None:
        assert eng.set_coeff(rows) == 0
        assert eng.is_initialized()
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


@pytest.mark.parametrize("case", sorted(CASES))
def test_parity_with_the_uniform_reference(orc, bfir, log, case):
    shape, fmt, back = CASES[case]
    s, L, blocks, ratios, n_in, n_out = shape
    Ls, D, _ = _geo(shape)
    lens = _lengths(shape, _null(shape))
    flat = [n for r in lens for n in r if n is not None]
    if len(flat) >= len(blocks):                                         # at least one filter ends in every level
        for k in range(len(blocks)):
            assert any(D[k] < n <= D[k + 1] for n in flat), (k, flat)
    assert max(flat) == _taps(_lv(shape)) and D[-1] - Ls[-1] < max(flat) < D[-1]
    rows = _rows(orc, shape)
    x = _audio(orc, shape, fmt)
    want = _ref(orc, ("parity", case), shape, rows, x)
    eng = _engine(bfir, shape, rows, fmt, chunk=3)
    names = ", ".join("%d x %d" % (Lk, b) for Lk, b in zip(Ls, blocks))
    made = [ln for ln in log if ln.startswith("bfir engine: matrix %d -> %d, %d levels, %s;" % (n_in, n_out, len(blocks), names))]
    assert made and made[0].endswith("back end %s." % back), log
    rc, y = eng.run(x)
    assert rc == 0 and y.shape == (x.shape[0], n_out)
    print("rel_err", case, rel_err(y, want))
    assert rel_err(y, want) <= _tol(s, fmt)
    eng.close()


# ---- bitwise ---------------------------------------------------------------------------------------------------------
# (realsize, L, blocks, ratios, C), the back end both engines log
DIAG = [((4, 512, (4, 2, 2), (1, 4, 2), 2), "fused"), ((4, 512, (4, 2, 2), (1, 4, 2), 4), "fused"),
        ((4, 16, (2, 2, 3), (1, 2, 2), 1), "general"), ((8, 1024, (4, 2, 2), (1, 2, 2), 2), "general")]


@pytest.mark.parametrize("shape,back", DIAG, ids=["f32-2", "f32-4", "f32-16-1", "f64-2"])
def test_diagonal_matrix_equals_the_levels_engine_bitwise(orc, bfir, log, shape, back):
    s, L, blocks, ratios, Cn = shape
    rng = np.random.default_rng(L + Cn + s)
    h = [(c * 40).astype(_real(s)) for c in orc.synth_ir(rng, Cn, _taps(shape), _real(s))]   # loud enough to clip
    x = orc.synth_audio(rng, _nb(shape) * L, Cn, _real(s))
    d = bfir.BrutefirLevels(L, blocks, ratios, s, Cn)
    m = bfir.BrutefirMatrixLevels(L, blocks, ratios, s, Cn, Cn)
    ends = [ln for ln in log if "levels, " in ln and "back end" in ln]
    assert len(ends) == 2 and all(ln.endswith("back end %s." % back) for ln in ends), log
    d.set_chunk(3); m.set_chunk(3)
    assert d.set_coeff(h) == 0
    assert m.set_coeff([[h[o] if i == o else None for i in range(Cn)] for o in range(Cn)]) == 0
    rd, yd = d.run(x)
    rm, ym = m.run(x)
    assert rd == rm == 0
    assert yd.tobytes() == ym.tobytes()
    for c in range(Cn):
        a, b = d.overflow(c), m.overflow(c)
        assert (a.n_overflows, a.largest, a.max) == (b.n_overflows, b.largest, b.max)
    assert sum(d.overflow(c).n_overflows for c in range(Cn)) > 0
    d.close(); m.close()


@pytest.mark.parametrize("case", ["1", "2", "4a"])
def test_filters_that_end_by_d1_equal_the_matrix_engine_bitwise(orc, bfir, case):
    shape, fmt, _ = CASES[case]
    s, L, blocks, ratios, n_in, n_out = shape
    _, D, _ = _geo(shape)
    rng = np.random.default_rng(17 + L)
    x = _audio(orc, shape)
    for taps in (D[1], D[1] - 7):
        rows = [[None if (o, i) in _null(shape) else orc.synth_ir(rng, 1, taps, _real(s))[0] for i in range(n_in)]
                for o in range(n_out)]
        small = bfir.BrutefirMatrix(L, blocks[0], s, n_in, n_out)
        small.set_chunk(3)
        assert small.set_coeff(rows) == 0
        rc0, y0 = small.run(x)
        eng = _engine(bfir, shape, rows, chunk=3)
        rc, y = eng.run(x)
        assert rc == rc0 == 0 and y.tobytes() == y0.tobytes(), taps
        for o in range(n_out):
            assert eng.overflow(o).largest == small.overflow(o).largest
        eng.close(); small.close()


def test_pair_outputs_do_not_depend_on_the_lone_output_beside_them(orc, bfir):
    """Outputs 0 and 1 of a 1 -> 3 engine equal, byte for byte, the 1 -> 2 engine built from the same first two rows: the
    pair kernels beside a lone channel (frame stride 3) compute what they compute without one.  Both engines transform
    their one input in direct mode and invert the first D_1 / L blocks with k_inv."""
    s, L, blocks, ratios, _, _ = CASES["4a"][0]
    rows = _rows(orc, (s, L, blocks, ratios, 1, 3), null=())
    x = _audio(orc, (s, L, blocks, ratios, 1, 3))
    f3 = _engine(bfir, (s, L, blocks, ratios, 1, 3), rows)
    f2 = _engine(bfir, (s, L, blocks, ratios, 1, 2), rows[:2])
    (q3, z3), (q2, z2) = f3.run(x), f2.run(x)
    assert q3 == q2 == 0
    f3.close(); f2.close()
    assert np.ascontiguousarray(z3[:, :2]).tobytes() == z2.tobytes()


def test_case_4_outputs_0_and_1_equal_the_2_to_2_engine(orc, bfir):
    """Case 4: outputs 0 and 1 of the 2 -> 3 engine against the 2 -> 2 engine built from the same first two rows, byte for
    byte.  Both engines transform their two inputs as one channel pair (a level pairs by its input side alone), the MAC
    chains of an output do not depend on its neighbours, and outputs 0 and 1 go through the same pair kernels in both --
    k_inv_pair_ps for the first D_1 / L blocks, k_inv_nup and k_inv_levels after -- at frame strides 3 and 2."""
    shape = CASES["4a"][0]
    s, L, blocks, ratios, n_in, n_out = shape
    rows = _rows(orc, shape, null=())
    x = _audio(orc, shape)
    e3 = _engine(bfir, shape, rows)
    e2 = _engine(bfir, (s, L, blocks, ratios, 2, 2), rows[:2])
    (r3, y3), (r2, y2) = e3.run(x), e2.run(x)
    assert r3 == r2 == 0
    e3.close(); e2.close()
    print("2->3 vs 2->2: max |diff|", float(np.abs(y3[:, :2].astype(np.float64) - y2).max()))
    assert np.ascontiguousarray(y3[:, :2]).tobytes() == y2.tobytes()


@pytest.mark.parametrize("case", ["1", "4a", "4b", "8"])
def test_output_does_not_depend_on_how_the_blocks_arrive(orc, bfir, case):
    import torch
    shape, fmt, _ = CASES[case]
    s, L, blocks, ratios, n_in, n_out = shape
    _, _, r = _geo(shape)
    nb = _nb(_lv(shape)) + 2
    rows = _rows(orc, shape)
    x = _audio(orc, shape, nb=nb)
    eng = _engine(bfir, shape, rows, chunk=None)                         # one long run, the default chunk
    rc, one = eng.run(x)
    assert rc == 0
    eng.close()
    assert rel_err(one, _ref(orc, ("arrive", case), shape, rows, x)) <= TOL[s]
    for chunk in (1, 3, 64):
        eng = _engine(bfir, shape, rows, chunk=chunk)
        rc, y = eng.run(x)
        assert rc == 0 and y.tobytes() == one.tobytes(), chunk
        eng.close()
    eng = _engine(bfir, shape, rows, chunk=None)                         # calls of 1, 2, 5, ... blocks
    parts, b = [], 0
    for n in [1, 2, 5, 3, 7, 1, 1, 4, 6, 2, 5, 3, 4, 1, 9] * 4:
        n = min(n, nb - b)
        if n <= 0:
            break
        rc, y = eng.run(x[b * L:(b + n) * L]); assert rc == 0
        parts.append(y); b += n
    assert b == nb and np.concatenate(parts).tobytes() == one.tobytes()
    eng.close()
    eng = _engine(bfir, shape, rows, chunk=5)                            # device pointers, two calls that split a block of every level
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.zeros((nb * L, n_out), dtype=d_in.dtype, device="cuda")
    torch.cuda.synchronize()
    cut = r[-1] + 1
    isz = x.dtype.itemsize
    eng.run_device(d_in.data_ptr(), d_out.data_ptr(), cut)
    eng.run_device(d_in.data_ptr() + cut * L * n_in * isz, d_out.data_ptr() + cut * L * n_out * isz, nb - cut)
    assert eng.sync() == 0
    assert d_out.cpu().numpy().tobytes() == one.tobytes()
    eng.close()


# ---- state -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["4a", "8"])
def test_new_filters_mid_stream_and_reset(orc, bfir, case):
    """After a second set_coeff and `settle` further blocks the output is the reference's with the new filters fed the
    whole stream -- also when the first set ends below D_2 (level 2 starts mid-stream) -- and reset() gives a new engine."""
    shape, fmt, _ = CASES[case]
    s, L, blocks, ratios, n_in, n_out = shape
    _, D, r = _geo(shape)
    settle = _settle(_lv(shape))
    n1 = r[-1] + 3                                                       # the change falls inside a block of every level
    nb = n1 + settle + 4
    rows2 = _rows(orc, shape)
    rows1 = _rows(orc, shape, seed=5, null=((0, 1),))
    x = _audio(orc, shape, nb=nb)
    want = _ref(orc, ("mid", case), shape, rows2, x)
    for first in (rows1, [[None if h is None else h[:D[2] - 5] for h in row] for row in rows1]):
        eng = _engine(bfir, shape, first)
        assert eng.run(x[:n1 * L])[0] == 0
        assert eng.set_coeff(rows2) == 0
        rc, y = eng.run(x[n1 * L:])
        assert rc == 0
        print("rel_err", case, rel_err(y[settle * L:], want[(n1 + settle) * L:]))
        assert rel_err(y[settle * L:], want[(n1 + settle) * L:]) <= TOL[s]
        eng.close()
    fresh = _engine(bfir, shape, rows2)
    rc, y0 = fresh.run(x)
    assert rc == 0
    fresh.close()
    eng = _engine(bfir, shape, rows2)
    assert eng.run(x[:(D[2] // L + r[-1] + 1) * L])[0] == 0             # stops inside a block of every level, with output queued
    eng.reset()
    assert eng.is_initialized() and all(eng.overflow(o).largest == 0.0 for o in range(n_out))
    rc, y = eng.run(x)
    assert rc == 0 and y.tobytes() == y0.tobytes()
    eng.close()


@pytest.mark.parametrize("case", ["4a", "1"])
def test_overflow_count_and_peak_per_output(orc, bfir, case):
    shape, fmt, _ = CASES[case]
    s, L, blocks, ratios, n_in, n_out = shape
    rows = _rows(orc, shape, gain=40.0)                                  # loud: the outputs clip
    x = _audio(orc, shape)
    ref = _ref(orc, ("loud", case), shape, rows, x)
    eng = _engine(bfir, shape, rows)
    rc, y = eng.run(x)
    assert rc == 0
    clipped = 0
    for o in range(n_out):
        of = eng.overflow(o)
        print("overflow", case, o, of.n_overflows, of.largest, np.abs(ref[:, o]).max())
        assert of.max == 1.0 and of.n_overflows == int(np.count_nonzero(np.abs(y[:, o].astype(np.float64)) > 1.0))
        assert abs(of.largest - np.abs(ref[:, o]).max()) <= TOL[s] * max(1.0, np.abs(ref[:, o]).max()) * 10
        clipped += of.n_overflows
    assert clipped > 0
    eng.close()


@pytest.mark.parametrize("case", ["4a", "8"])
def test_partition_spectra_of_every_level(orc, bfir, case):
    shape, fmt, _ = CASES[case]
    s, L, blocks, ratios, n_in, n_out = shape
    Ls, D, _ = _geo(shape)
    rows = _rows(orc, shape)
    eng = _engine(bfir, shape, rows, chunk=None)
    assert eng.D == D[:-1] and eng.max_taps == D[-1] and eng.lengths == Ls
    padded, _ = pad_rows(rows, _real(s))
    for level, (Lp, Bp) in enumerate(zip(Ls, blocks)):
        for o in range(n_out):
            for i in range(n_in):
                if rows[o][i] is None:
                    continue
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
    n = len(blocks)
    for lv, o, i, b in [(n, 0, 0, 0), (-1, 0, 0, 0), (0, n_out, 0, 0), (0, 0, n_in, 0), (0, 0, 0, blocks[0]), (1, 0, 0, blocks[1]),
                        (n - 1, 0, 0, blocks[-1]), (1, -1, 0, 0), (1, 0, -1, 0), (2, 0, 0, -1)]:
        assert lib.bfir_engine_read_coeff_matrix_levels(eng.handle, lv, o, i, b, dst.ctypes.data) == bfir.ERR_ARG
    assert lib.bfir_engine_read_coeff_matrix_levels(eng.handle, 0, 0, 0, 0, None) == bfir.ERR_ARG
    eng.close()


# ---- unread input ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["2", "4a", "4b"])
def test_unread_input_skips_a_nan_and_reading_it_again_settles(orc, bfir, log, case):
    """A column that is NULL on every level: a NaN on that input reaches no output and no verdict, the frames kept for the
    partial blocks of the levels included.  A set that reads the column again changes the path of the levels that can pair
    channels (the log shows it) and the output settles on the reference."""
    shape, fmt, _ = CASES[case]
    s, L, blocks, ratios, n_in, n_out = shape
    _, D, r = _geo(shape)
    settle = _settle(_lv(shape))
    nb1 = _nb(_lv(shape))
    nb = nb1 + settle + 4
    dense = _rows(orc, shape, null=())
    sparse = [[row[0], None] for row in dense]
    x = _audio(orc, shape, nb=nb)
    clean = x.copy(); clean[:, 1] = 0
    bad = x.copy()
    bad[3 * L + 5, 1] = np.nan
    bad[(D[2] // L + 1) * L, 1] = np.nan                                 # sample 0 of a block, past D_2
    bad[(nb1 - 1) * L + 7, 1] = np.inf                                   # in the frames kept across the call
    del log[:]
    eng = _engine(bfir, shape, sparse)
    paired = n_in % 2 == 0                                               # a level pairs by its input side
    went = [ln for ln in log if ln.startswith("bfir matrix engine: an input feeds no output: path=direct")]
    assert len(went) == ((1 + sum(1 for Lk in _geo(shape)[0][1:] if Lk <= 8192)) if paired else 0), log
    rc, y = eng.run(bad[:nb1 * L])
    assert rc == 0 and np.all(np.isfinite(y))
    assert rel_err(y, _ref(orc, ("sparse", case), shape, sparse, clean[:nb1 * L])) <= TOL[s]
    del log[:]
    assert eng.set_coeff(dense) == 0
    back = [ln for ln in log if ln.startswith("bfir matrix engine: every input feeds an output: path=pair")]
    assert len(back) == len(went), log
    # the NaNs are now in reach of the filters (delay lines, kept frames): a verdict is in order while they play out
    assert eng.run(x[nb1 * L:(nb1 + settle) * L])[0] in (0, bfir.ERR_NONFINITE)
    rc, y = eng.run(x[(nb1 + settle) * L:])
    assert rc == 0
    want = _ref(orc, ("dense", case), shape, dense, x)
    print("rel_err", case, rel_err(y, want[(nb1 + settle) * L:]))
    assert rel_err(y, want[(nb1 + settle) * L:]) <= TOL[s]
    eng.close()


def test_an_input_read_by_the_head_only_counts_as_read(orc, bfir, log):
    """Input 1 has one short filter (it ends in level 0) and NULL elsewhere: it is read, so the engine keeps its channel
    pairs on every level and a NaN on it is a verdict."""
    shape = CASES["2"][0]
    s, L, blocks, ratios, n_in, n_out = shape
    rows = _rows(orc, shape, null=())
    rows = [[rows[0][0], rows[0][1][:L + 3]], [rows[1][0], None]]
    x = _audio(orc, shape)
    del log[:]
    eng = _engine(bfir, shape, rows)
    assert not [ln for ln in log if ln.startswith("bfir matrix engine: ")], log
    rc, y = eng.run(x)
    assert rc == 0 and rel_err(y, uniform_reference(orc, L, s, rows, x)) <= TOL[s]
    bad = x.copy(); bad[5 * L, 1] = np.nan
    eng.reset()
    assert eng.run(bad)[0] == bfir.ERR_NONFINITE
    eng.close()


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_calls_of_the_other_kinds_are_refused(orc, bfir):
    lib = bfir.load()
    shape = CASES["4a"][0]
    s, L, blocks, ratios, n_in, n_out = shape
    Ls, _, _ = _geo(shape)
    rows = _rows(orc, shape)
    x = _audio(orc, shape)
    U = bfir.ERR_UNSUPPORTED
    eng = _engine(bfir, shape, rows)
    rc, before = eng.run(x[:4 * L])
    assert rc == 0
    eng.reset()
    h = rows[0][0]
    ptrs = (C.c_void_p * 8)(*([h.ctypes.data] * 8))
    lens = (C.c_int * 8)(*([100] * 8))
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
    assert lib.bfir_engine_fade_remaining_levels(eng.handle) == 0        # fades on this kind are out of scope
    for call in (lambda: eng.set_coeff_fade(rows, 3), lambda: eng.fade_to(rows, 3)):
        with pytest.raises(bfir.BfirError) as ex:
            call()
        assert ex.value.code == U
    assert eng.is_initialized()                                          # a refused call changes nothing
    rc, after = eng.run(x[:4 * L])
    assert rc == 0 and after.tobytes() == before.tobytes()
    # a NaN tap, in the last level's part of one filter: BFIR_ERR_COEFF and the engine is uninitialised
    bad = [[None if c is None else c.copy() for c in row] for row in rows]
    bad[0][0][-3] = np.nan
    assert eng.set_coeff(bad) == bfir.ERR_COEFF and not eng.is_initialized()
    assert eng.run(x[:L])[0] == bfir.ERR_STATE
    too_long = [[np.zeros(eng.max_taps + 1, np.float32)] * n_in] * n_out
    assert eng.set_coeff(too_long) == bfir.ERR_ARG
    assert eng.set_coeff([[np.zeros(eng.max_taps, np.float32)] * n_in] * n_out) == 0
    eng.close()
    others = (bfir.Brutefir(L, blocks[0], s, 2), bfir.BrutefirMatrix(L, blocks[0], s, 2, 2),
              bfir.BrutefirNup(L, blocks[0], ratios[1], blocks[1], s, 2), bfir.BrutefirLevels(L, blocks, ratios, s, 2))
    for other in others:
        assert lib.bfir_engine_set_coeff_matrix_levels(other.handle, ptrs, lens, 1.0) == U
        assert lib.bfir_engine_read_coeff_matrix_levels(other.handle, 0, 0, 0, 0, dst.ctypes.data) == U
        other.close()


def test_profile_counts_every_level_and_no_staging_kernel(orc, bfir):
    """Case 4 (2 -> 3, the pair kernels and the lone kernel in one k_inv span): 32 blocks in launches of 4, levels of 1,
    4 and 8 blocks, as test_levels_gpu.test_profile_counts_every_level."""
    shape = CASES["4a"][0]
    s, L, blocks, ratios, n_in, n_out = shape
    _, D, r = _geo(shape)
    nb = 32
    rows = _rows(orc, shape)
    x = _audio(orc, shape, nb=nb)
    eng = _engine(bfir, shape, rows, chunk=4)
    assert eng.run(x)[0] == 0                                            # sizes the work buffers
    eng.reset()
    eng.set_profiling(True)
    assert eng.run(x)[0] == 0
    prof = eng.profile()
    want = nb // 4 + nb // r[1] + nb // r[2]
    print(prof)
    assert prof["k_fwd"][1] == want and prof["k_mac"][1] == want and prof["k_inv"][1] == want
    assert prof["k_stage_in"][1] == 0 and prof["k_stage_out"][1] == 0    # fused back end
    eng.close()


# ---- the C++ mirror --------------------------------------------------------------------------------------------------
def _fnv1a(data):
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return h


def test_cpp_mirror_runs_a_matrix_on_three_levels_like_the_ctypes_engine(tmp_path, bfir):
    """tests/cpp/test_mlevels_mirror.cpp builds its input and filters from integer recurrences (restated here), runs a
    2 -> 3 three-level brutefir one block per run() and prints the FNV-1a hash of its output bytes."""
    src = os.path.join(ROOT, "tests", "cpp", "test_mlevels_mirror.cpp")
    exe = str(tmp_path / "test_mlevels_mirror")
    libdir = os.path.dirname(bfir.library_path())
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", src, "-o", exe, "-L" + libdir, "-lbfir_hip",
                    "-Wl,-rpath," + libdir], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "ALL OK" in p.stdout
    L, blocks, ratios, NI, NO, nb = 512, (4, 2, 2), (1, 4, 2), 2, 3, 48
    lengths = [11000, 1500, 5000, 0, 2049, 14336]
    i = np.arange(nb * L * NI, dtype=np.uint64)
    x = ((((i * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(8)).astype(np.float64) / 16777216.0 - 0.5)
    x = x.astype(np.float32).reshape(nb * L, NI)
    flat = []
    for pidx, taps in enumerate(lengths):
        if taps == 0:
            flat.append(None)
            continue
        n = np.arange(taps, dtype=np.uint64)
        v = (((n + np.uint64(1)) * np.uint64(40503 * (pidx + 3))) & np.uint64(0xffff)).astype(np.float64) / 65536.0 - 0.5
        flat.append((v / (64.0 * (1.0 + n.astype(np.float64) / 64.0))).astype(np.float32))
    rows = [flat[o * NI:(o + 1) * NI] for o in range(NO)]
    eng = bfir.BrutefirMatrixLevels(L, blocks, ratios, 4, NI, NO)
    assert eng.set_coeff(rows) == 0
    rc, y = eng.run(x)
    assert rc == 0
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("checksum ")]
    assert line and int(line[0].split()[1], 16) == _fnv1a(y.tobytes())
    eng.close()
