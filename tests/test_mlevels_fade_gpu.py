"""Crossfaded coefficient changes on multi-level matrix engines on the GPU (bfir_engine_set_coeff_matrix_levels_fade,
BrutefirMatrixLevels.fade_to_rows) and k_mac_duo, the matrix MAC of a fading chunk (csrc/mfade.hip, BFIR_MFADE_DUO).

The reference is test_mlevels.uniform_reference, once per filter set on the longest input any case of a shape uses, blended
in float64 with test_fade.fade_weights: the ramp of fftw_convolver::convolver_crossfade_inplace stretched over K head
blocks.  A case of nb blocks blends the first nb blocks of the two signals (the oracle runs block after block).  Tolerances
are the project's own, unchanged: rel_err <= TOL[s] of conftest, and 1e-6 where fp64 arithmetic runs on FLOAT_LE frames
(test_mlevels_gpu._tol).  The argument is the one at the top of test_fade_gpu.py and test_levels_fade_gpu.py: a convex
combination of two signals that each meet the tolerance, plus the blend's roundings and at most three more additions per
set.  test_mlevels_fade pins the definition (the blend of two per-pair level models) to this reference on the CPU.

Filters have per-filter lengths that end inside different levels (_lens); the new set moves the level every filter ends on
and the NULL pair, so the two count tables differ and the longest filter of a MAC tile comes from the old set for some
inputs and from the new set for others (test_the_two_sets_differ_as_the_tests_need).  t0 and K are
test_levels_fade_gpu's; set_chunk(3)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import TOL, rel_err
from test_fade import fade_weights
from test_levels_fade_gpu import _Ks, _nb, _t0s
from test_levels_gpu import _make, _settle
from test_mlevels import uniform_reference
from test_mlevels_gpu import CASES, _audio, _fmt, _fnv1a, _geo, _lv, _real, _tol

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (s, L, blocks, ratios, n_in, n_out), frame format (None = the working precision's)
SHAPES = {
    "general": CASES["1"][:2],                                           # general back end, grouped layout
    "fused22": CASES["2"][:2],                                           # fused, pair front end, two rings
    "fused12": CASES["3"][:2],                                           # direct front end, fused back end
    "fused23": CASES["4a"][:2],                                          # odd n_out, frame pairs on odd floats
    "fused21": CASES["4b"][:2],                                          # odd n_out, single output
    "four33": CASES["5"][:2],                                            # three rings, every D_k = L_k
    "two23": CASES["6"][:2],                                             # two levels
    "deep22": ((4, 512, (8, 2, 2), (1, 2, 2), 2, 2), None),              # deep catch-up
    "f64": ((8, 64, (4, 3, 5), (1, 2, 2), 2, 2), None),                  # fp64, general
    "f64f": CASES["8f"][:2],                                             # fp64 on float32 frames
}
GRID = ("fused23", "general")                                            # the full t0 x K grid; the others two corners


def _lens(shape, new):
    """Tap counts per filter.  Old set: test_mlevels_gpu._lengths -- filter j ends in level order[j], the first one in the
    last level, inside the last partition of its level, one NULL pair in (n_out - 1, 0).  New set: the old one with the input
    columns mirrored (the outputs, with one input), so the NULL pair and the level of a filter move, and every other filter
    ends inside the FIRST partition of its level: partition counts differ between the sets at every level."""
    s, L, blocks, ratios, n_in, n_out = shape
    Ls, D, _ = _geo(shape)
    n = len(blocks)
    order = [n - 1] + list(range(n - 1))
    null = ((n_out - 1, 0),) if n_in * n_out >= 3 else ()
    levels, j = [], 0
    for o in range(n_out):
        row = []
        for i in range(n_in):
            if (o, i) in null:
                row.append(None)
                continue
            row.append((order[j % n], j // n))
            j += 1
        levels.append(row)
    if new:
        levels = [r[::-1] for r in levels] if n_in > 1 else levels[::-1]
    lens = []
    for o, r in enumerate(levels):
        row = []
        for i, e in enumerate(r):
            if e is None:
                row.append(None)
                continue
            k, short = e
            last = blocks[k] - 1 if not new or (o + i) % 2 == 0 else 0
            row.append(D[k] + last * Ls[k] + Ls[k] // 3 + 1 - short - (2 if new else 0))
        lens.append(row)
    return lens


def _counts(shape, lens):
    """[level][o][i]: partitions of h_{o,i} on the level, as bfir_engine_set_coeff_matrix_levels splits the filters."""
    s, L, blocks, ratios, n_in, n_out = shape
    Ls, D, _ = _geo(shape)
    return [[[0 if n is None else -(-max(0, min(n - D[k], blocks[k] * Ls[k])) // Ls[k]) for n in r] for r in lens]
            for k in range(len(blocks))]


def _mk_rows(orc, shape, lens, seed):
    s = shape[0]
    rng = np.random.default_rng(7000 + shape[1] + sum(shape[2]) + 10 * shape[4] + shape[5] + seed)
    return [[None if n is None else orc.synth_ir(rng, 1, n, _real(s))[0] for n in r] for r in lens]


def _nb_max(shape):
    lv = _lv(shape)
    return max(_nb(lv, max(_t0s(lv)), max(_Ks(lv))), _nb(lv, _t0s(lv)[1], 3) + _settle(lv) + 4)


_DATA = {}


def _refs(orc, shape, rows_old, rows_new, x):
    ys = tuple(uniform_reference(orc, shape[1], shape[0], rows, x) for rows in (rows_old, rows_new))
    for y in ys:
        y.setflags(write=False)
    return ys


def _data(orc, name):
    """rows_old, rows_new, x of the longest run and the uniform references (y_old, y_new): computed once, read-only."""
    if name not in _DATA:
        shape, fmt = SHAPES[name]
        rows_old, rows_new = _mk_rows(orc, shape, _lens(shape, False), 0), _mk_rows(orc, shape, _lens(shape, True), 1)
        x = _audio(orc, shape, fmt, nb=_nb_max(shape))
        x.setflags(write=False)
        _DATA[name] = (rows_old, rows_new, x, _refs(orc, shape, rows_old, rows_new, x))
    return _DATA[name]


def _blend(ys, L, nb, t0, K):
    w = fade_weights(L, nb, t0, K)[:, None]
    return ys[0][:nb * L] * (1.0 - w) + ys[1][:nb * L] * w


def _engine(bfir, shape, rows, fmt=None, chunk=3, scale=1.0):
    s, L, blocks, ratios, n_in, n_out = shape
    eng = bfir.BrutefirMatrixLevels(L, blocks, ratios, s, n_in, n_out, fmt, fmt)
    if chunk is not None:
        eng.set_chunk(chunk)
    if rows is not None:
        assert eng.set_coeff(rows, scale=scale) == 0
    return eng


def _faded(eng, x, L, t0, rows_new, K, scale=1.0, steps=None):
    """Blocks [0, t0) in one call, fade_to_rows, then the rest in one call or cut as `steps` says (cycled)."""
    nb = x.shape[0] // L
    outs = []
    if t0:
        rc, y = eng.run(x[:t0 * L]); assert rc == 0
        outs.append(y)
    assert eng.fade_to_rows(rows_new, K, scale=scale) == 0
    assert eng.fade_remaining() == K
    b, i = t0, 0
    while b < nb:
        n = nb - b if steps is None else min(steps[i % len(steps)], nb - b)
        rc, y = eng.run(x[b * L:(b + n) * L]); assert rc == 0
        outs.append(y); b += n; i += 1
    return np.concatenate(outs)


@pytest.fixture()
def log(bfir):
    from foo_dsp_bfir_amd import _lib
    lines = []
    cb = _lib.LOG_FN(lambda msg: lines.append(msg.decode(errors="replace")))
    lib = bfir.load()
    lib.bfir_set_log_callback(cb)
    yield lines
    lib.bfir_set_log_callback(_lib.LOG_FN())


def _mid(shape):
    """t0 inside a block of every level, and the longest K."""
    lv = _lv(shape)
    return _t0s(lv)[1], _Ks(lv)[2]


# ---- 1. parity ---------------------------------------------------------------------------------------------------------
PARITY = [(n, ti, ki) for n in GRID for ti in range(4) for ki in range(3)] + \
         [(n, ti, ki) for n in SHAPES if n not in GRID for ti, ki in ((1, 2), (3, 0))]


def test_the_two_sets_differ_as_the_tests_need():
    for name, (shape, _) in SHAPES.items():
        s, L, blocks, ratios, n_in, n_out = shape
        _, D, _ = _geo(shape)
        old, new = _lens(shape, False), _lens(shape, True)
        co, cn = _counts(shape, old), _counts(shape, new)
        assert co != cn, name
        for lens, cnt in ((old, co), (new, cn)):                         # every input is read, every level has taps
            assert all(any(r[i] is not None for r in lens) for i in range(n_in)), name
            assert all(any(c for r in lvl for c in r) for lvl in cnt), name
        if n_in * n_out >= 3:
            assert [[n is None for n in r] for r in old] != [[n is None for n in r] for r in new], name
        if n_in >= 2 and n_in * n_out >= 4:
            # a MAC tile (two outputs in fp32, one in fp64) and an input whose longest filter is the old set's, and one where
            # it is the new set's: the step loop of k_mac_duo runs to either set's maximum
            no = 2 if s == 4 else 1
            who = set()
            for k in range(len(blocks)):
                for o0 in range(0, n_out, no):
                    for i in range(n_in):
                        mo = max(co[k][o][i] for o in range(o0, min(o0 + no, n_out)))
                        mn = max(cn[k][o][i] for o in range(o0, min(o0 + no, n_out)))
                        who.add((mo > mn) - (mo < mn))
            assert {-1, 1} <= who, (name, who)


@pytest.mark.parametrize("name,ti,ki", PARITY, ids=["%s-t%d-K%d" % p for p in PARITY])
def test_parity_with_the_blend_of_two_uniform_references(orc, bfir, name, ti, ki):
    shape, fmt = SHAPES[name]
    s, L = shape[0], shape[1]
    lv = _lv(shape)
    t0, K = _t0s(lv)[ti], _Ks(lv)[ki]
    nb = _nb(lv, t0, K)
    rows_old, rows_new, x, ys = _data(orc, name)
    eng = _engine(bfir, shape, rows_old, fmt)
    y = _faded(eng, x[:nb * L], L, t0, rows_new, K)
    err, tol = rel_err(y, _blend(ys, L, nb, t0, K)), _tol(s, _fmt(s, fmt))
    print("rel_err", name, "t0", t0, "K", K, err, "tol", tol)
    assert err <= tol
    assert eng.fade_remaining() == 0
    eng.close()


# ---- 2. k_mac_duo against two launches of k_mac_matrix ---------------------------------------------------------------------
@pytest.mark.parametrize("steps", [None, [1]], ids=["one-call", "one-block-calls"])
@pytest.mark.parametrize("name", ["fused22", "fused23", "four33", "general", "f64"])
def test_one_duo_launch_gives_the_bytes_of_two_matrix_launches(orc, bfir, monkeypatch, log, name, steps):
    """BFIR_MFADE_DUO is read when an engine is created: the same fade on an engine of each kind.  One long call takes the
    tiled instances (set_chunk(8): eight blocks per launch where the fade and the levels allow it), one-block calls the
    TT = 1 instances."""
    shape, fmt = SHAPES[name]
    L = shape[1]
    t0, K = _mid(shape)
    nb = _nb(_lv(shape), t0, K)
    rows_old, rows_new, x, ys = _data(orc, name)
    out = {}
    for duo in ("1", "0"):
        monkeypatch.setenv("BFIR_MFADE_DUO", duo)
        eng = _engine(bfir, shape, rows_old, fmt, chunk=8)
        eng.set_profiling(True)
        out[duo] = _faded(eng, x[:nb * L], L, t0, rows_new, K, steps=steps)
        out[duo + "n"] = eng.profile()["k_mac"][1]
        eng.close()
        said = [ln for ln in log if ln.startswith("bfir matrix engine: crossfade over %d blocks" % K)]
        assert len(said) == 1 and said[0].endswith("runs %s." % ("k_mac_duo" if duo == "1" else "k_mac_matrix twice")), log
        del log[:]
    assert rel_err(out["1"], _blend(ys, L, nb, t0, K)) <= _tol(shape[0], _fmt(shape[0], fmt))
    assert out["1"].tobytes() == out["0"].tobytes()
    assert out["1n"] == out["0n"]                                        # a profile span is a MAC step, one launch or two


# ---- 3. diagonal rows: the diagonal engine's fade --------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", [2, 4])
def test_diagonal_rows_fade_as_the_levels_engine_bitwise(orc, bfir, Cn):
    shape = (4, 512, (4, 2, 2), (1, 4, 2), Cn)
    s, L, blocks, ratios, _ = shape
    t0, K = _t0s(shape)[1], _Ks(shape)[2]
    nb = _nb(shape, t0, K)
    h_old, x = _make(orc, shape, nb=nb)
    h_new, _ = _make(orc, shape, seed=5, nb=1)
    h_old, h_new = [(c * 30).astype(np.float32) for c in h_old], [(c * 30).astype(np.float32) for c in h_new]   # loud enough to clip
    diag = lambda h: [[h[o] if i == o else None for i in range(Cn)] for o in range(Cn)]
    d = bfir.BrutefirLevels(L, blocks, ratios, s, Cn)
    d.set_chunk(3)
    assert d.set_coeff(h_old) == 0
    rc, a = d.run(x[:t0 * L]); assert rc == 0
    assert d.fade_to(h_new, K) == 0
    rc, b = d.run(x[t0 * L:]); assert rc == 0
    m = _engine(bfir, shape + (Cn,), diag(h_old))
    y = _faded(m, x, L, t0, diag(h_new), K)
    assert y.tobytes() == np.concatenate([a, b]).tobytes()
    for c in range(Cn):
        p, q = d.overflow(c), m.overflow(c)
        assert (p.n_overflows, p.largest) == (q.n_overflows, q.largest)
    assert sum(d.overflow(c).n_overflows for c in range(Cn)) > 0
    d.close(); m.close()


# ---- 4. outside the fade nothing changes -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fused23", "general", "f64", "deep22"])
def test_outside_the_fade_nothing_changes(orc, bfir, name):
    """Both sets read every input, so no level changes its front end: before a_f the bytes of an engine that never faded,
    from a_f + K on those of an engine created with the new set and fed the same input from block 0."""
    shape, fmt = SHAPES[name]
    L = shape[1]
    t0, K = _t0s(_lv(shape))[1], 3
    nb = _nb(_lv(shape), t0, K)
    rows_old, rows_new, x, _ = _data(orc, name)
    x = x[:nb * L]
    plain = []
    for rows in (rows_old, rows_new):
        eng = _engine(bfir, shape, rows, fmt)
        rc, y = eng.run(x); assert rc == 0
        plain.append(y); eng.close()
    eng = _engine(bfir, shape, rows_old, fmt)
    y = _faded(eng, x, L, t0, rows_new, K)
    eng.close()
    assert np.array_equal(y[:t0 * L], plain[0][:t0 * L])
    assert np.array_equal(y[(t0 + K) * L:], plain[1][(t0 + K) * L:])
    for b in range(t0, t0 + K):
        blk = slice(b * L + (1 if b == t0 else 0), (b + 1) * L - (1 if b == t0 + K - 1 else 0))   # w = 0 and w = 1 at the two ends
        assert not np.array_equal(y[blk], plain[0][blk]) and not np.array_equal(y[blk], plain[1][blk]), b


# ---- 5. the cut does not matter ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fused23", "general"])
def test_fade_does_not_depend_on_how_the_blocks_arrive(orc, bfir, name):
    import torch
    shape, fmt = SHAPES[name]
    s, L, n_in, n_out = shape[0], shape[1], shape[4], shape[5]
    r = _geo(shape)[2]
    t0, K = r[-1] + 3, r[-1] + 2
    nb = _nb(_lv(shape), t0, K)
    rows_old, rows_new, x, ys = _data(orc, name)
    x = x[:nb * L]
    eng = _engine(bfir, shape, rows_old, chunk=None)                     # one call, the default chunk
    one = _faded(eng, x, L, t0, rows_new, K)
    eng.close()
    assert rel_err(one, _blend(ys, L, nb, t0, K)) <= TOL[s]
    for chunk, steps in ((1, None), (3, None), (None, [1]), (None, [1, 2, 5, 3, 7, 1, 1, 4, 6, 2, 5, 3, 4, 1, 9])):
        eng = _engine(bfir, shape, rows_old, chunk=chunk)
        y = _faded(eng, x, L, t0, rows_new, K, steps=steps)
        assert np.array_equal(y, one), (chunk, steps and steps[:3])
        eng.close()
    # device pointers: two calls after the fade request whose cut lies inside the fade and inside a block of every level
    eng = _engine(bfir, shape, rows_old, chunk=5)
    rc, head = eng.run(x[:t0 * L]); assert rc == 0
    assert eng.fade_to_rows(rows_new, K) == 0
    d_in = torch.from_numpy(np.array(x[t0 * L:])).cuda()
    d_out = torch.zeros((d_in.shape[0], n_out), dtype=d_in.dtype, device="cuda")
    torch.cuda.synchronize()
    cut = 2
    assert cut < K and all((t0 + cut) % rk for rk in r[1:])
    fi, fo = n_in * x.dtype.itemsize, n_out * x.dtype.itemsize
    eng.run_device(d_in.data_ptr(), d_out.data_ptr(), cut)
    eng.run_device(d_in.data_ptr() + cut * L * fi, d_out.data_ptr() + cut * L * fo, nb - t0 - cut)
    assert eng.sync() == 0
    assert np.array_equal(np.concatenate([head, d_out.cpu().numpy()]), one)
    eng.close()


# ---- 6. unread inputs --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fused22", "fused23"])
def test_new_set_drops_an_input_column(orc, bfir, name):
    """Input 1 is read by the old set and by no filter of the new one: the fade runs with every level in direct mode, and
    once it is over a NaN on that input reaches no output and no verdict."""
    shape, fmt = SHAPES[name]
    s, L = shape[0], shape[1]
    t0, K = _mid(shape)
    nb = _nb(_lv(shape), t0, K)
    rows_old, dense, x, ys = _data(orc, name)
    rows_new = [[row[0] if row[0] is not None else row[1][:row[1].size - 1], None] for row in dense]
    x = x[:nb * L]
    want = _blend((ys[0], uniform_reference(orc, L, s, rows_new, x)), L, nb, t0, K)
    bad = x.copy()
    bad[(t0 + K + 1) * L, 1] = np.nan                                    # sample 0 of a block after the fade
    bad[(t0 + K + 1) * L + 9:, 1] = np.inf
    eng = _engine(bfir, shape, rows_old)
    y = _faded(eng, bad, L, t0, rows_new, K)                             # asserts rc == 0: no verdict
    eng.close()
    assert np.all(np.isfinite(y))
    err = rel_err(y, want)
    print("rel_err", name, err)
    assert err <= TOL[s]


@pytest.mark.parametrize("name", ["fused22", "fused23"])
def test_new_set_reads_a_column_the_old_one_does_not(orc, bfir, name):
    shape, fmt = SHAPES[name]
    s, L = shape[0], shape[1]
    t0, K = _mid(shape)
    nb = _nb(_lv(shape), t0, K)
    dense, rows_new, x, ys = _data(orc, name)
    rows_old = [[row[0] if row[0] is not None else row[1][:row[1].size - 1], None] for row in dense]
    x = x[:nb * L]
    want = _blend((uniform_reference(orc, L, s, rows_old, x), ys[1]), L, nb, t0, K)
    eng = _engine(bfir, shape, rows_old)
    y = _faded(eng, x, L, t0, rows_new, K)
    eng.close()
    err = rel_err(y, want)
    print("rel_err", name, err)
    assert err <= TOL[s]


# ---- 7. level reach ----------------------------------------------------------------------------------------------------
def _cut(rows, taps):
    return [[None if h is None else h[:min(h.size, taps)] for h in r] for r in rows]


@pytest.mark.parametrize("name", ["fused23", "f64"])
def test_fade_to_a_set_that_ends_below_the_last_level(orc, bfir, name):
    """No filter of the new set reaches the last level: it runs through the fade with every count 0 for the new set and
    stops after it.  From a_f + K on the bytes are those of an engine that had the short set all along, and once every ring
    has played out those of an engine that took it with a plain set_coeff at a_f."""
    shape, fmt = SHAPES[name]
    s, L, blocks = shape[0], shape[1], shape[2]
    _, D, r = _geo(shape)
    settle = _settle(_lv(shape))
    t0, K = _t0s(_lv(shape))[1], 3
    nb = _nb(_lv(shape), t0, K) + settle + 4
    rows_old, rows_new, x, ys = _data(orc, name)
    short = _cut(rows_new, D[len(blocks) - 1] - 5)
    assert x.shape[0] >= nb * L
    x = x[:nb * L]
    want = _blend((ys[0], uniform_reference(orc, L, s, short, x)), L, nb, t0, K)
    eng = _engine(bfir, shape, rows_old)
    y = _faded(eng, x, L, t0, short, K)
    assert eng.fade_remaining() == 0
    eng.close()
    err = rel_err(y, want)
    print("rel_err", name, err)
    assert err <= TOL[s]
    eng = _engine(bfir, shape, short)
    rc, all_along = eng.run(x); assert rc == 0
    eng.close()
    assert np.array_equal(y[(t0 + K) * L:], all_along[(t0 + K) * L:])
    eng = _engine(bfir, shape, rows_old)
    rc, _ = eng.run(x[:t0 * L]); assert rc == 0
    assert eng.set_coeff(short) == 0
    rc, cut = eng.run(x[t0 * L:]); assert rc == 0
    eng.close()
    assert np.array_equal(y[(t0 + K + settle) * L:], cut[(K + settle) * L:])


@pytest.mark.parametrize("name", ["fused23", "f64"])
def test_fade_to_a_set_that_reaches_a_level_no_old_filter_reaches(orc, bfir, name):
    shape, fmt = SHAPES[name]
    s, L, blocks = shape[0], shape[1], shape[2]
    _, D, r = _geo(shape)
    t0, K = _t0s(_lv(shape))[1], 3
    nb = _nb(_lv(shape), t0, K)
    rows_old, rows_new, x, _ = _data(orc, name)
    x = x[:nb * L]
    short = _cut(rows_old, D[len(blocks) - 1] - 5)
    eng = _engine(bfir, shape, short)
    rc, _ = eng.run(x[:t0 * L]); assert rc == 0
    assert eng.fade_to_rows(rows_new, K) == bfir.ERR_UNSUPPORTED
    assert eng.fade_remaining() == 0 and eng.is_initialized()
    rc, after = eng.run(x[t0 * L:]); assert rc == 0
    eng.close()
    eng = _engine(bfir, shape, short)
    rc, plain = eng.run(x); assert rc == 0
    eng.close()
    assert np.array_equal(after, plain[t0 * L:])


def test_sets_that_end_by_d1_fade_as_the_matrix_engine_bitwise(orc, bfir):
    shape, fmt = SHAPES["fused22"]
    s, L, blocks, ratios, n_in, n_out = shape
    _, D, _ = _geo(shape)
    t0, K = 5, 3
    nb = t0 + K + 6
    rows_old, rows_new, x, _ = _data(orc, "fused22")
    x = x[:nb * L]
    taps = D[1] - 7
    pad = lambda rows: [[None if h is None else np.concatenate([h[:taps], np.zeros(max(0, taps - h.size), h.dtype)]) for h in r]
                        for r in rows]
    old, new = pad(rows_old), pad(rows_new)
    small = bfir.BrutefirMatrix(L, blocks[0], s, n_in, n_out)
    small.set_chunk(3)
    assert small.set_coeff(old) == 0
    rc, a = small.run(x[:t0 * L]); assert rc == 0
    assert small.set_coeff_fade(new, K) == 0
    rc, b = small.run(x[t0 * L:]); assert rc == 0
    small.close()
    eng = _engine(bfir, shape, old)
    y = _faded(eng, x, L, t0, new, K)
    eng.close()
    assert y.tobytes() == np.concatenate([a, b]).tobytes()


# ---- 8. states and arguments -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fused23", "general"])
def test_states_of_a_fade(orc, bfir, name):
    shape, fmt = SHAPES[name]
    s, L, blocks, ratios, n_in, n_out = shape
    _, D, r = _geo(shape)
    settle = _settle(_lv(shape))
    t0, K = r[-1] + 3, r[-1] + 2
    rows_old, rows_new, x, ys = _data(orc, name)
    assert x.shape[0] >= (t0 + K + settle + 4) * L
    # fade_remaining counts down; a second fade is refused while one is pending and accepted once it is done
    eng = _engine(bfir, shape, rows_old, chunk=None)
    assert eng.fade_remaining() == 0
    rc, _ = eng.run(x[:t0 * L]); assert rc == 0
    old_spec = eng.coeff_block(0, 0, 0, 0)
    assert eng.fade_to_rows(rows_new, K) == 0 and eng.fade_remaining() == K
    assert eng.fade_to_rows(rows_old, K) == bfir.ERR_STATE and eng.fade_remaining() == K
    for b in range(K):
        assert np.array_equal(eng.coeff_block(0, 0, 0, 0), old_spec)     # the head's old set while the fade remains
        rc, _ = eng.run(x[(t0 + b) * L:(t0 + b + 1) * L]); assert rc == 0
        assert eng.fade_remaining() == K - 1 - b
        if b < K - 1:
            assert eng.fade_to_rows(rows_old, K) == bfir.ERR_STATE
    fresh = _engine(bfir, shape, rows_new)
    assert not np.array_equal(fresh.coeff_block(0, 0, 0, 0), old_spec)
    for level in range(len(blocks)):                                     # ... and the new set at every level afterwards
        for o, i in ((0, 0), (n_out - 1, n_in - 1)):
            assert np.array_equal(eng.coeff_block(level, o, i, 0), fresh.coeff_block(level, o, i, 0)), (level, o, i)
    fresh.close()
    assert eng.fade_to_rows(rows_old, 2) == 0 and eng.fade_remaining() == 2
    rc, _ = eng.run(x[:2 * L]); assert rc == 0
    assert eng.fade_remaining() == 0
    eng.close()
    # a NaN tap in the last level's part of one filter: refused, the engine stays initialised on the old set, byte for byte
    plain = _engine(bfir, shape, rows_old)
    rc, want = plain.run(x[:(t0 + K + 3) * L]); assert rc == 0
    plain.close()
    eng = _engine(bfir, shape, rows_old)
    rc, a = eng.run(x[:t0 * L]); assert rc == 0
    bad = [[None if h is None else h.copy() for h in row] for row in rows_new]
    longest = max(((h.size, o, i) for o, row in enumerate(bad) for i, h in enumerate(row) if h is not None))
    assert longest[0] > D[len(blocks) - 1] + 3
    bad[longest[1]][longest[2]][D[len(blocks) - 1] + 3] = np.nan
    assert eng.fade_to_rows(bad, K) == bfir.ERR_COEFF
    assert eng.is_initialized() and eng.fade_remaining() == 0
    rc, b = eng.run(x[t0 * L:(t0 + K + 3) * L]); assert rc == 0
    assert np.concatenate([a, b]).tobytes() == want.tobytes()
    eng.close()
    # a plain set_coeff mid-fade ends it: a hard cut, the output stays finite and settles on the new filters
    eng = _engine(bfir, shape, rows_old)
    rc, _ = eng.run(x[:t0 * L]); assert rc == 0
    assert eng.fade_to_rows(rows_new, K) == 0
    rc, _ = eng.run(x[t0 * L:(t0 + 2) * L]); assert rc == 0
    assert eng.fade_remaining() == K - 2
    assert eng.set_coeff(rows_new) == 0 and eng.fade_remaining() == 0
    n1 = t0 + 2
    rc, y = eng.run(x[n1 * L:(n1 + settle + 4) * L]); assert rc == 0
    assert np.all(np.isfinite(y))
    err = rel_err(y[settle * L:], ys[1][(n1 + settle) * L:(n1 + settle + 4) * L])
    print("rel_err after set_coeff mid-fade", name, err)
    assert err <= TOL[s]
    eng.close()
    # reset() mid-fade: the new set is active at every level, all signal state is gone
    x2 = _audio(orc, shape, fmt, seed=1, nb=settle)
    fresh = _engine(bfir, shape, rows_new)
    rc, want = fresh.run(x2); assert rc == 0
    fresh.close()
    eng = _engine(bfir, shape, rows_old)
    rc, _ = eng.run(x[:t0 * L]); assert rc == 0
    assert eng.fade_to_rows(rows_new, K) == 0
    rc, _ = eng.run(x[t0 * L:(t0 + 2) * L]); assert rc == 0
    eng.reset()
    assert eng.fade_remaining() == 0 and eng.is_initialized()
    rc, y = eng.run(x2)
    assert rc == 0 and np.array_equal(y, want)
    eng.close()


def test_argument_checks_and_other_kinds_of_engine(orc, bfir):
    lib = bfir.load()
    shape, fmt = SHAPES["fused23"]
    s, L, blocks, ratios, n_in, n_out = shape
    rows_old, rows_new, x, _ = _data(orc, "fused23")
    A, U = bfir.ERR_ARG, bfir.ERR_UNSUPPORTED
    P = n_in * n_out
    flat = [h for r in rows_new for h in r]
    ptrs = (C.c_void_p * P)(*[None if h is None else h.ctypes.data for h in flat])
    lens = (C.c_int * P)(*[0 if h is None else h.size for h in flat])
    fade = lib.bfir_engine_set_coeff_matrix_levels_fade
    eng = _engine(bfir, shape, None)
    assert eng.fade_to_rows(rows_new, 3) == bfir.ERR_STATE               # not initialised
    assert eng.set_coeff(rows_old) == 0
    for K in (0, -1, (1 << 24) // L + 1):
        assert eng.fade_to_rows(rows_new, K) == A, K
    assert fade(eng.handle, None, lens, 1.0, 3) == A
    assert fade(eng.handle, ptrs, None, 1.0, 3) == A
    for n in (-1, eng.max_taps + 1):
        too = (C.c_int * P)(*lens); too[1] = n
        assert fade(eng.handle, ptrs, too, 1.0, 3) == A, n
    assert eng.fade_remaining() == 0
    with pytest.raises(bfir.BfirError):                                  # the calls of the other kinds stay refused
        eng.fade_to(rows_new, 3)
    with pytest.raises(bfir.BfirError):
        eng.set_coeff_fade(rows_new, 3)
    assert lib.bfir_engine_set_coeff_levels_fade(eng.handle, ptrs, n_in, 100, 1.0, 3) == U
    assert lib.bfir_engine_set_coeff_matrix_fade(eng.handle, ptrs, 100, 1, 1.0, 3) == U
    assert eng.fade_to_rows(rows_new, (1 << 24) // L) == 0 and eng.fade_remaining() == (1 << 24) // L
    plain = bfir.Brutefir(L, blocks[0], s, n_in)
    matrix = bfir.BrutefirMatrix(L, blocks[0], s, n_in, n_out)
    nup = bfir.BrutefirNup(L, blocks[0], ratios[1], blocks[1], s, n_in)
    lv = bfir.BrutefirLevels(L, blocks, ratios, s, n_in)
    for other in (plain, matrix, nup, lv):
        assert fade(other.handle, ptrs, lens, 1.0, 3) == U
        other.close()
    eng.close()


# ---- 9. overflow statistics and the NaN guard -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fused23", "f64"])
def test_overflow_counts_and_nan_guard_act_on_the_blend(orc, bfir, name):
    shape, fmt = SHAPES[name]
    s, L, n_out = shape[0], shape[1], shape[5]
    t0, K = _mid(shape)
    nb = _nb(_lv(shape), t0, K)
    rows_old, rows_new, x, ys = _data(orc, name)
    x = x[:nb * L]
    want = _blend(ys, L, nb, t0, K)
    # per output: only samples of the fade exceed full scale, in the float64 blend and so (away from 1.0) in the engine
    gain = 1.0 / np.abs(want[t0 * L:(t0 + K) * L]).max() / 0.7           # the fade's loudest sample lands near 1.43
    eng = _engine(bfir, shape, rows_old, scale=gain)
    y = _faded(eng, x, L, t0, rows_new, K, scale=gain)
    clipped = 0
    for o in range(n_out):
        of = eng.overflow(o)
        ref = np.abs(want[:, o] * gain)
        print("overflow", name, o, of.n_overflows, of.largest, int((ref > 1.0).sum()), ref.max())
        assert of.max == 1.0
        assert of.n_overflows == int((np.abs(y[:, o]) > 1.0).sum())
        assert of.largest == float(np.abs(y[:, o]).max())
        sure = np.abs(ref - 1.0) > 4 * TOL[s] * ref.max()                # samples whose side of 1.0 the tolerance cannot change
        assert np.array_equal((np.abs(y[:, o]) > 1.0)[sure], (ref > 1.0)[sure])
        assert abs(of.largest - ref.max()) <= 4 * TOL[s] * ref.max()
        clipped += int((np.abs(y[t0 * L:(t0 + K) * L, o]) > 1.0).sum())
    assert clipped > 0                                                   # ... and some of it during the fade
    eng.close()
    bad = x.copy()
    bad[(t0 + 1) * L, 0] = np.nan                                        # data, not an address: sample 0 of fade block 1
    eng = _engine(bfir, shape, rows_old)
    rc, _ = eng.run(bad[:t0 * L]); assert rc == 0
    assert eng.fade_to_rows(rows_new, K) == 0
    rc, _ = eng.run(bad[t0 * L:])
    assert rc == bfir.ERR_NONFINITE
    eng.close()


# ---- 10. the C++ mirror ------------------------------------------------------------------------------------------------
def test_cpp_mirror_fades_a_matrix_on_three_levels_like_the_ctypes_engine(tmp_path, bfir):
    """tests/cpp/test_mlevels_fade_mirror.cpp builds its input and both filter matrices from integer recurrences (restated
    here), runs a 2 -> 3 three-level brutefir one block per run() with a fade requested before block 11 and prints the
    FNV-1a hash of its output bytes."""
    src = os.path.join(ROOT, "tests", "cpp", "test_mlevels_fade_mirror.cpp")
    exe = str(tmp_path / "test_mlevels_fade_mirror")
    libdir = os.path.dirname(bfir.library_path())
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", src, "-o", exe, "-L" + libdir, "-lbfir_hip",
                    "-Wl,-rpath," + libdir], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "ALL OK" in p.stdout
    L, blocks, ratios, NI, NO, nb, t0, K = 512, (4, 2, 2), (1, 4, 2), 2, 3, 48, 11, 10
    lengths = [[11000, 1500, 5000, 0, 2049, 14336], [1500, 14336, 0, 5000, 11000, 2049]]
    i = np.arange(nb * L * NI, dtype=np.uint64)
    x = ((((i * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(8)).astype(np.float64) / 16777216.0 - 0.5)
    x = x.astype(np.float32).reshape(nb * L, NI)
    sets = []
    for st in range(2):
        flat = []
        for pi, taps in enumerate(lengths[st]):
            n = np.arange(taps, dtype=np.uint64)
            v = (((n + np.uint64(1)) * np.uint64(40503 * (pi + 3 + 8 * st))) & np.uint64(0xffff)).astype(np.float64) / 65536.0 - 0.5
            flat.append((v / (64.0 * (1.0 + n.astype(np.float64) / 64.0))).astype(np.float32) if taps else None)
        sets.append([flat[o * NI:(o + 1) * NI] for o in range(NO)])
    eng = bfir.BrutefirMatrixLevels(L, blocks, ratios, 4, NI, NO)
    assert eng.set_coeff(sets[0]) == 0
    y = _faded(eng, x, L, t0, sets[1], K, steps=[1])
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("checksum ")]
    assert line and int(line[0].split()[1], 16) == _fnv1a(y.tobytes())
    eng.close()
