"""Crossfaded coefficient changes on two-level and multi-level engines on the GPU (bfir_engine_set_coeff_nup_fade /
_set_coeff_levels_fade / _fade_remaining_levels).

The yardstick is the uniform oracle: test_fade.fade_expected(orc, L, ceil(taps / L), s, C, h_old, h_new, x, t0, K, fmt, fmt),
two oracle engines with the old and the new filters on the same input from block 0, blended in float64 with the ramp of
fftw_convolver::convolver_crossfade_inplace stretched over K head blocks; test_levels_fade pins the multi-level definition
to it on the CPU.  It is called once per (shape, filters) on the longest input any case uses; a case of nb blocks blends the
first nb blocks of the two signals it returns with test_fade.fade_weights, which is what the call on the shorter input gives
(the oracle runs block after block).  Tolerances are the project's own, unchanged: TOL and rel_err of conftest, and 1e-6
where an fp64 engine writes float32 frames (test_fade_gpu._tol).  The argument is the one at the top of test_fade_gpu.py: a
convex combination of two signals that each meet the tolerance, plus the blend's roundings and at most three more additions
per set.  Data as in test_levels_gpu._make: taps that end inside the last partition of the last level, synth_audio input."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import TOL, rel_err
from test_fade import fade_expected, fade_weights
from test_fade_gpu import _tol
from test_levels_gpu import F32, _fmt, _fnv1a, _geo, _id, _make, _settle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (s, L, blocks, ratios, C), frame format (None = the working precision's), back end
SHAPES = [
    ((4, 512, (4, 2, 2), (1, 4, 2), 2), None, "fused"),                  # two rings
    ((4, 512, (2, 2, 2, 2), (1, 2, 2, 2), 4), None, "fused"),            # three rings, every D_k = L_k or just above
    ((4, 512, (5, 3, 2), (1, 4, 2), 4), None, "fused"),                  # ring reads that start mid-block of a level
    ((4, 512, (8, 2, 2), (1, 2, 2), 2), None, "fused"),                  # deep catch-up: D_1 / L_1 = 4
    ((4, 512, (4, 2, 2), (1, 4, 2), 3), None, "fused"),                  # odd channel count
    ((4, 64, (3, 3, 2), (1, 2, 2), 3), None, "general"),                 # general, fp32
    ((8, 64, (4, 3, 5), (1, 2, 2), 3), None, "general"),                 # general, fp64
    ((8, 1024, (8, 2, 2), (1, 4, 2), 2), F32, "general"),                # fp64, float32 frames
    ((4, 512, (4, 2), (1, 4), 2), None, "fused"),                        # one ring: BrutefirNup(512, 4, 4, 2, 4, 2) ...
]
FUSED, FUSED_MID, DEEP, GENERAL, F64_SHAPE, TWO = (SHAPES[0][0], SHAPES[2][0], SHAPES[3][0], SHAPES[5][0], SHAPES[6][0],
                                                   SHAPES[8][0])
# ... and its create_levels twin
ENGINES = [(sh, fmt, "levels") for sh, fmt, _ in SHAPES] + [(TWO, None, "nup")]


def _r_last(shape):
    return _geo(shape)[2][-1]


def _t0s(shape):
    """No tail contributes yet; inside a block of every level; on a boundary of every level; every ring and delay line has
    wrapped."""
    s, L, blocks, ratios, Cn = shape
    _, D, r = _geo(shape)
    return [1, r[-1] + 3, 2 * r[-1], D[-2] // L + r[-1] * (blocks[-1] + 2) + 1]


def _Ks(shape):
    return [1, 3, 2 * _r_last(shape) + 3]


def _nb(shape, t0, K):
    return t0 + K + _r_last(shape) + 3


def _nb_max(shape):
    """The longest parity run, or the two runs of the shrinking-set case."""
    r = _r_last(shape)
    return max(_nb(shape, max(_t0s(shape)), max(_Ks(shape))), 2 * _nb(shape, r + 3, 2 * r + 3))


_DATA = {}


def _data(orc, shape, fmt=None):
    """h_old, h_new, x of the longest run and the uniform oracle's (y_old, y_new) for them, computed once and read-only."""
    key = (shape, fmt)
    if key not in _DATA:
        s, L, blocks, ratios, Cn = shape
        nb = _nb_max(shape)
        h_old, x = _make(orc, shape, fmt, nb=nb)
        h_new, _ = _make(orc, shape, fmt, seed=5, nb=1)
        x.setflags(write=False)
        _DATA[key] = (h_old, h_new, x, _oracle_pair(orc, shape, fmt, h_old, h_new, x))
    return _DATA[key]


def _oracle_pair(orc, shape, fmt, h_old, h_new, x):
    s, L, blocks, ratios, Cn = shape
    taps = max(h_old[0].size, h_new[0].size)
    _, y_old, y_new = fade_expected(orc, L, -(-taps // L), s, Cn, h_old, h_new, x, 0, 1, _fmt(s, fmt), _fmt(s, fmt))
    for y in (y_old, y_new):
        y.setflags(write=False)
    return y_old, y_new


def _blend(ys, L, nb, t0, K):
    """fade_expected's own blend on the first nb blocks."""
    w = fade_weights(L, nb, t0, K)[:, None]
    return ys[0][:nb * L] * (1.0 - w) + ys[1][:nb * L] * w


def _engine(bfir, shape, h, fmt=None, kind="levels", chunk=3, scale=1.0):
    s, L, blocks, ratios, Cn = shape
    if kind == "nup":
        eng = bfir.BrutefirNup(L, blocks[0], ratios[1], blocks[1], s, Cn, fmt, fmt)
    else:
        eng = bfir.BrutefirLevels(L, blocks, ratios, s, Cn, fmt, fmt)
    if chunk is not None:
        eng.set_chunk(chunk)
    assert eng.set_coeff(h, scale=scale) == 0
    return eng


def _faded(eng, x, L, t0, h_new, K, scale=1.0, steps=None):
    """Blocks [0, t0) in one call, fade_to, then the rest in one call or cut as `steps` says (cycled).  Returns the frames."""
    nb = x.shape[0] // L
    outs = []
    if t0:
        rc, y = eng.run(x[:t0 * L]); assert rc == 0
        outs.append(y)
    assert eng.fade_to(h_new, K, scale=scale) == 0
    assert eng.fade_remaining() == K
    b, i = t0, 0
    while b < nb:
        n = nb - b if steps is None else min(steps[i % len(steps)], nb - b)
        rc, y = eng.run(x[b * L:(b + n) * L]); assert rc == 0
        outs.append(y); b += n; i += 1
    return np.concatenate(outs)


# ---- 1. parity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ki", range(3), ids=["K1", "K3", "K2r+3"])
@pytest.mark.parametrize("ti", range(4), ids=["t0-before-tails", "t0-mid-block", "t0-boundary", "t0-wrapped"])
@pytest.mark.parametrize("shape,fmt,kind", ENGINES, ids=[_id(e[0]) + "-" + e[2] for e in ENGINES])
def test_parity_with_the_blend_of_two_uniform_oracles(orc, bfir, shape, fmt, kind, ti, ki):
    s, L, blocks, ratios, Cn = shape
    t0, K = _t0s(shape)[ti], _Ks(shape)[ki]
    nb = _nb(shape, t0, K)
    h_old, h_new, x, ys = _data(orc, shape, fmt)
    eng = _engine(bfir, shape, h_old, fmt, kind)
    y = _faded(eng, x[:nb * L], L, t0, h_new, K)
    err, tol = rel_err(y, _blend(ys, L, nb, t0, K)), _tol(s, _fmt(s, fmt))
    print("rel_err", shape, kind, "t0", t0, "K", K, err, "tol", tol)
    assert err <= tol
    assert eng.fade_remaining() == 0
    eng.close()


@pytest.mark.parametrize("shape,fmt,back", SHAPES, ids=[_id(e[0]) for e in SHAPES])
def test_the_shapes_take_the_back_ends_they_are_listed_for(orc, bfir, shape, fmt, back):
    """The fused back end stores the frames itself; the general one ends in the staging path's output kernel."""
    s, L, blocks, ratios, Cn = shape
    t0, K = _t0s(shape)[3], 3
    h_old, h_new, x, _ = _data(orc, shape, fmt)
    eng = _engine(bfir, shape, h_old, fmt)
    rc, _ = eng.run(x[:t0 * L]); assert rc == 0
    assert eng.fade_to(h_new, K) == 0
    eng.set_profiling(True)
    rc, _ = eng.run(x[t0 * L:(t0 + K) * L]); assert rc == 0
    prof = eng.profile()
    eng.close()
    print(shape, prof)
    # fused: the rule of k_inv_fade (fp32 on pairs, FLOAT_LE frames, 512 <= L <= 8192), any channel count
    assert (back == "fused") == (s == 4 and _fmt(s, fmt) == F32 and 512 <= L <= 8192)
    assert (prof["k_stage_out"][1] == 0) == (back == "fused")


# ---- 2. outside the fade nothing changes -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [FUSED, GENERAL, F64_SHAPE, DEEP], ids=["fused", "general", "f64", "deep"])
def test_outside_the_fade_nothing_changes(orc, bfir, shape):
    s, L, blocks, ratios, Cn = shape
    r = _r_last(shape)
    t0, K = r + 3, 3
    nb = _nb(shape, t0, K)
    h_old, h_new, x, _ = _data(orc, shape)
    x = x[:nb * L]
    plain = []
    for h in (h_old, h_new):
        eng = _engine(bfir, shape, h)
        rc, y = eng.run(x); assert rc == 0
        plain.append(y); eng.close()
    eng = _engine(bfir, shape, h_old)
    y = _faded(eng, x, L, t0, h_new, K)
    eng.close()
    assert np.array_equal(y[:t0 * L], plain[0][:t0 * L])                 # an engine that never faded
    assert np.array_equal(y[(t0 + K) * L:], plain[1][(t0 + K) * L:])     # an engine that had h_new from block 0
    for b in range(t0, t0 + K):
        blk = slice(b * L + (1 if b == t0 else 0), (b + 1) * L - (1 if b == t0 + K - 1 else 0))   # w = 0 and w = 1 at the two ends
        assert not np.array_equal(y[blk], plain[0][blk]) and not np.array_equal(y[blk], plain[1][blk]), b


# ---- 3. the cut does not matter ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [FUSED_MID, GENERAL], ids=["fused", "general"])
def test_fade_does_not_depend_on_how_the_blocks_arrive(orc, bfir, shape):
    import torch
    s, L, blocks, ratios, Cn = shape
    r = _r_last(shape)
    t0, K = r + 3, r + 2
    nb = _nb(shape, t0, K)
    h_old, h_new, x, ys = _data(orc, shape)
    x = x[:nb * L]
    eng = _engine(bfir, shape, h_old, chunk=None)                        # one call, the default chunk
    one = _faded(eng, x, L, t0, h_new, K)
    eng.close()
    assert rel_err(one, _blend(ys, L, nb, t0, K)) <= TOL[s]
    for chunk, steps in ((1, None), (3, None), (None, [1]), (None, [1, 2, 5, 3, 7, 1, 1, 4, 6, 2, 5, 3, 4, 1, 9])):
        eng = _engine(bfir, shape, h_old, chunk=chunk)
        y = _faded(eng, x, L, t0, h_new, K, steps=steps)
        assert np.array_equal(y, one), (chunk, steps and steps[:3])
        eng.close()
    # device pointers: two calls after the fade request whose cut lies inside the fade and inside a block of every level
    eng = _engine(bfir, shape, h_old, chunk=5)
    rc, head = eng.run(x[:t0 * L]); assert rc == 0
    assert eng.fade_to(h_new, K) == 0
    d_in = torch.from_numpy(np.array(x[t0 * L:])).cuda()                 # a writable copy of the read-only input
    d_out = torch.zeros_like(d_in)
    torch.cuda.synchronize()
    cut = 2
    assert cut < K and all((t0 + cut) % rk for rk in _geo(shape)[2][1:])
    fb = Cn * x.dtype.itemsize
    eng.run_device(d_in.data_ptr(), d_out.data_ptr(), cut)
    eng.run_device(d_in.data_ptr() + cut * L * fb, d_out.data_ptr() + cut * L * fb, nb - t0 - cut)
    assert eng.sync() == 0
    assert np.array_equal(np.concatenate([head, d_out.cpu().numpy()]), one)
    eng.close()


def test_deep_catch_up_on_the_latency_path(orc, bfir):
    shape = DEEP
    s, L, blocks, ratios, Cn = shape
    r = _r_last(shape)
    t0, K = r + 3, r + 2
    nb = _nb(shape, t0, K)
    h_old, h_new, x, ys = _data(orc, shape)
    eng = _engine(bfir, shape, h_old, chunk=None)
    y = _faded(eng, x[:nb * L], L, t0, h_new, K, steps=[1])
    eng.close()
    err = rel_err(y, _blend(ys, L, nb, t0, K))
    print("rel_err deep, one run() per block", err)
    assert err <= TOL[s]


# ---- 4. identity fade --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [FUSED, GENERAL, F64_SHAPE], ids=["fused", "general", "f64"])
def test_fading_to_the_same_filters_keeps_the_output(orc, bfir, shape):
    s, L, blocks, ratios, Cn = shape
    r = _r_last(shape)
    t0, K = r + 3, 2 * r + 3
    nb = _nb(shape, t0, K)
    h_old, _, x, _ = _data(orc, shape)
    x = x[:nb * L]
    eng = _engine(bfir, shape, h_old)
    rc, plain = eng.run(x); assert rc == 0
    eng.close()
    eng = _engine(bfir, shape, h_old)
    y = _faded(eng, x, L, t0, h_old, K)
    eng.close()
    for b in range(nb):
        blk = slice(b * L, (b + 1) * L)
        assert np.abs(y[blk].astype(np.float64) - plain[blk]).max() <= TOL[s] * np.abs(plain).max(), b


# ---- 5. / 6. sets of different lengths ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [FUSED, F64_SHAPE], ids=["fused", "f64"])
def test_fade_to_a_set_that_ends_below_the_last_level(orc, bfir, shape):
    """h_new ends 5 taps below D_2: level 2 runs through the fade with no partitions for the new set and stops after it."""
    s, L, blocks, ratios, Cn = shape
    _, D, r = _geo(shape)
    t0, K = r[-1] + 3, 2 * r[-1] + 3
    nb = _nb(shape, t0, K)
    h_old, h_new, x, _ = _data(orc, shape)
    short = [c[:D[2] - 5] for c in h_new]
    assert x.shape[0] >= 2 * nb * L
    x = x[:2 * nb * L]
    ys = _oracle_pair(orc, shape, None, h_old, short, x)
    eng = _engine(bfir, shape, h_old)
    y = _faded(eng, x[:nb * L], L, t0, short, K)
    err = rel_err(y, _blend(ys, L, nb, t0, K))
    print("rel_err through the fade", shape, err)
    assert err <= TOL[s] and eng.fade_remaining() == 0
    rc, y2 = eng.run(x[nb * L:]); assert rc == 0
    err = rel_err(y2, ys[1][nb * L:])
    print("rel_err after it", shape, err)
    assert err <= TOL[s]
    eng.close()


@pytest.mark.parametrize("shape", [FUSED, F64_SHAPE], ids=["fused", "f64"])
def test_fade_to_a_set_that_reaches_a_level_the_old_one_does_not(orc, bfir, shape):
    s, L, blocks, ratios, Cn = shape
    _, D, r = _geo(shape)
    t0, K = r[-1] + 3, 3
    nb = _nb(shape, t0, K)
    h_old, h_new, x, _ = _data(orc, shape)
    x = x[:nb * L]
    short = [c[:D[2] - 5] for c in h_old]
    eng = _engine(bfir, shape, short)
    rc, _ = eng.run(x[:t0 * L]); assert rc == 0
    assert eng.fade_to(h_new, K) == bfir.ERR_UNSUPPORTED
    assert eng.fade_remaining() == 0 and eng.is_initialized()
    rc, after = eng.run(x[t0 * L:]); assert rc == 0
    eng.close()
    eng = _engine(bfir, shape, short)                                    # ... an engine that never saw the call
    rc, plain = eng.run(x); assert rc == 0
    eng.close()
    assert np.array_equal(after, plain[t0 * L:])
    # the way round it: the first set zero-padded to the longest length that will be faded to
    padded = [np.concatenate([c, np.zeros(h_new[0].size - c.size, c.dtype)]) for c in short]
    ys = _oracle_pair(orc, shape, None, padded, h_new, x)
    eng = _engine(bfir, shape, padded)
    y = _faded(eng, x, L, t0, h_new, K)
    eng.close()
    err = rel_err(y, _blend(ys, L, nb, t0, K))
    print("rel_err padded", shape, err)
    assert err <= TOL[s]


# ---- 7. states ---------------------------------------------------------------------------------------------------------
def _uniform(orc, shape, h, x):
    s, L, blocks, ratios, Cn = shape
    ref = orc.Engine(L, -(-h[0].size // L), s, Cn)
    assert ref.set_coeff(h) == 0
    rc, y = ref.run(x); assert rc == 0
    ref.close()
    return np.asarray(y, dtype=np.float64)


@pytest.mark.parametrize("shape", [FUSED, GENERAL], ids=["fused", "general"])
def test_states_of_a_fade(orc, bfir, shape):
    s, L, blocks, ratios, Cn = shape
    _, D, r = _geo(shape)
    settle = _settle(shape)
    t0, K = r[-1] + 3, r[-1] + 2
    h_old, h_new, x, ys = _data(orc, shape)
    assert x.shape[0] >= (t0 + K + settle + 4) * L
    # fade_remaining counts down; a second fade is refused while one is pending and accepted once it is done
    eng = _engine(bfir, shape, h_old, chunk=None)
    assert eng.fade_remaining() == 0
    rc, _ = eng.run(x[:t0 * L]); assert rc == 0
    assert eng.fade_to(h_new, K) == 0 and eng.fade_remaining() == K
    assert eng.fade_to(h_old, K) == bfir.ERR_STATE and eng.fade_remaining() == K
    for b in range(K):
        rc, _ = eng.run(x[(t0 + b) * L:(t0 + b + 1) * L]); assert rc == 0
        assert eng.fade_remaining() == K - 1 - b
        if b < K - 1:
            assert eng.fade_to(h_old, K) == bfir.ERR_STATE
    assert eng.fade_to(h_old, 2) == 0 and eng.fade_remaining() == 2
    rc, _ = eng.run(x[:2 * L]); assert rc == 0
    assert eng.fade_remaining() == 0
    # every level reads the new set once fade_remaining is 0 (h_old again here)
    fresh = _engine(bfir, shape, h_old)
    for level in range(len(blocks)):
        assert np.array_equal(eng.coeff_block(level, Cn - 1, blocks[level] - 1), fresh.coeff_block(level, Cn - 1, blocks[level] - 1))
    fresh.close(); eng.close()
    # a NaN tap in the last level's part: refused, the engine is still initialised and keeps running the old filters
    eng = _engine(bfir, shape, h_old)
    rc, _ = eng.run(x[:t0 * L]); assert rc == 0
    bad = [c.copy() for c in h_new]; bad[Cn - 1][D[2] + 3] = np.nan
    assert eng.fade_to(bad, K) == bfir.ERR_COEFF
    assert eng.is_initialized() and eng.fade_remaining() == 0
    rc, y = eng.run(x[t0 * L:(t0 + K + 3) * L]); assert rc == 0
    assert rel_err(y, ys[0][t0 * L:(t0 + K + 3) * L]) <= TOL[s]
    eng.close()
    # a plain set_coeff mid-fade ends it; after `settle` blocks the output is the new filters'
    eng = _engine(bfir, shape, h_old)
    rc, _ = eng.run(x[:t0 * L]); assert rc == 0
    assert eng.fade_to(h_new, K) == 0
    rc, _ = eng.run(x[t0 * L:(t0 + 2) * L]); assert rc == 0
    assert eng.fade_remaining() == K - 2
    assert eng.set_coeff(h_new) == 0 and eng.fade_remaining() == 0
    n1 = t0 + 2
    rc, y = eng.run(x[n1 * L:(n1 + settle + 4) * L]); assert rc == 0
    err = rel_err(y[settle * L:], ys[1][(n1 + settle) * L:(n1 + settle + 4) * L])
    print("rel_err after set_coeff mid-fade", shape, err)
    assert err <= TOL[s]
    eng.close()
    # reset() mid-fade: the new set is active at every level, all signal state is gone
    _, x2 = _make(orc, shape, seed=1, nb=settle)
    fresh = _engine(bfir, shape, h_new)
    rc, want = fresh.run(x2); assert rc == 0
    fresh.close()
    eng = _engine(bfir, shape, h_old)
    rc, _ = eng.run(x[:t0 * L]); assert rc == 0
    assert eng.fade_to(h_new, K) == 0
    rc, _ = eng.run(x[t0 * L:(t0 + 2) * L]); assert rc == 0
    eng.reset()
    assert eng.fade_remaining() == 0 and eng.is_initialized()
    rc, y = eng.run(x2)
    assert rc == 0 and np.array_equal(y, want)
    eng.close()


def test_argument_checks_and_other_kinds_of_engine(orc, bfir):
    lib = bfir.load()
    shape = FUSED
    s, L, blocks, ratios, Cn = shape
    h_old, h_new, x, _ = _data(orc, shape)
    A, U = bfir.ERR_ARG, bfir.ERR_UNSUPPORTED
    ptrs = (C.c_void_p * 4)(*[h_new[c % Cn].ctypes.data for c in range(4)])
    n = h_new[0].size
    lv = bfir.BrutefirLevels(L, blocks, ratios, s, Cn)
    assert lv.fade_to(h_new, 3) == bfir.ERR_STATE                        # not initialised
    assert lv.set_coeff(h_old) == 0
    for K in (0, -1, (1 << 24) // L + 1):
        assert lv.fade_to(h_new, K) == A, K
    assert lib.bfir_engine_set_coeff_levels_fade(lv.handle, None, Cn, n, 1.0, 3) == A
    assert lib.bfir_engine_set_coeff_levels_fade(lv.handle, ptrs, -1, n, 1.0, 3) == A
    assert lib.bfir_engine_set_coeff_levels_fade(lv.handle, ptrs, Cn, -1, 1.0, 3) == A
    assert lib.bfir_engine_set_coeff_levels_fade(lv.handle, ptrs, Cn, lv.max_taps + 1, 1.0, 3) == A
    assert lv.fade_remaining() == 0
    assert lv.fade_to(h_new, (1 << 24) // L) == 0 and lv.fade_remaining() == (1 << 24) // L
    plain = bfir.Brutefir(L, blocks[0], s, Cn)
    matrix = bfir.BrutefirMatrix(L, blocks[0], s, 2, 2)
    nup = bfir.BrutefirNup(L, blocks[0], ratios[1], blocks[1], s, Cn)
    assert nup.set_coeff([c[:nup.max_taps] for c in h_old]) == 0        # two levels hold fewer taps than three
    for other in (plain, matrix, nup):
        assert lib.bfir_engine_set_coeff_levels_fade(other.handle, ptrs, Cn, 100, 1.0, 3) == U
    for other in (plain, matrix, lv):
        assert lib.bfir_engine_set_coeff_nup_fade(other.handle, ptrs, Cn, 100, 1.0, 3) == U
    for other in (plain, matrix):
        assert lib.bfir_engine_fade_remaining_levels(other.handle) == U
    assert lib.bfir_engine_fade_remaining_levels(nup.handle) == 0
    # the uniform entry points keep refusing split engines
    assert lib.bfir_engine_fade_remaining(nup.handle) == U and lib.bfir_engine_fade_remaining(lv.handle) == U
    with pytest.raises(bfir.BfirError):
        nup.set_coeff_fade(h_new, 3)
    for e in (plain, matrix, nup, lv):
        e.close()


# ---- 8. overflow statistics and the NaN guard -------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [FUSED, F64_SHAPE], ids=["fused", "f64"])
def test_overflow_counts_and_nan_guard_act_on_the_blend(orc, bfir, shape):
    s, L, blocks, ratios, Cn = shape
    r = _r_last(shape)
    t0, K = r + 3, 2 * r + 3
    nb = _nb(shape, t0, K)
    h_old, h_new, x, ys = _data(orc, shape)
    x = x[:nb * L]
    want = _blend(ys, L, nb, t0, K)
    gain = 1.0 / np.abs(want[t0 * L:(t0 + K) * L]).max() / 0.7           # the fade's loudest sample lands near 1.43
    eng = _engine(bfir, shape, h_old, scale=gain)
    y = _faded(eng, x, L, t0, h_new, K, scale=gain)
    clipped = 0
    for c in range(Cn):
        of = eng.overflow(c)
        print("overflow", shape, c, of.n_overflows, of.largest)
        assert of.max == 1.0
        assert of.n_overflows == int((np.abs(y[:, c]) > 1.0).sum())
        assert of.largest == float(np.abs(y[:, c]).max())
        clipped += int((np.abs(y[t0 * L:(t0 + K) * L, c]) > 1.0).sum())
    assert clipped > 0                                                   # ... and some of it during the fade
    eng.close()
    bad = x.copy()
    bad[(t0 + 1) * L, 0] = np.nan                                        # data, not an address: sample 0 of fade block 1
    eng = _engine(bfir, shape, h_old)
    rc, _ = eng.run(bad[:t0 * L]); assert rc == 0
    assert eng.fade_to(h_new, K) == 0
    rc, _ = eng.run(bad[t0 * L:])
    assert rc == bfir.ERR_NONFINITE
    eng.close()


# ---- 9. the C++ mirror -------------------------------------------------------------------------------------------------
def test_cpp_mirror_fades_three_levels_like_the_ctypes_engine(tmp_path, bfir):
    """tests/cpp/test_levels_fade_mirror.cpp builds its input and both filter sets from integer recurrences (restated
    here), runs a three-level brutefir one block per run() with a fade requested before block 11 and prints the FNV-1a hash
    of its output bytes."""
    src = os.path.join(ROOT, "tests", "cpp", "test_levels_fade_mirror.cpp")
    exe = str(tmp_path / "test_levels_fade_mirror")
    libdir = os.path.dirname(bfir.library_path())
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", src, "-o", exe, "-L" + libdir, "-lbfir_hip",
                    "-Wl,-rpath," + libdir], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "ALL OK" in p.stdout
    L, blocks, ratios, Cn, taps, nb, t0, K = 512, (4, 2, 2), (1, 4, 2), 2, 11000, 48, 11, 10
    i = np.arange(nb * L * Cn, dtype=np.uint64)
    x = ((((i * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(8)).astype(np.float64) / 16777216.0 - 0.5)
    x = x.astype(np.float32).reshape(nb * L, Cn)
    n = np.arange(taps, dtype=np.uint64)
    h = []
    for k in range(2 * Cn):
        v = (((n + np.uint64(1)) * np.uint64(40503 * (k % Cn + 3 + 4 * (k // Cn)))) & np.uint64(0xffff)).astype(np.float64) / 65536.0 - 0.5
        h.append((v / (64.0 * (1.0 + n.astype(np.float64) / 64.0))).astype(np.float32))
    eng = bfir.BrutefirLevels(L, blocks, ratios, 4, Cn)
    assert eng.set_coeff(h[:Cn]) == 0
    y = _faded(eng, x, L, t0, h[Cn:], K, steps=[1])
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("checksum ")]
    assert line and int(line[0].split()[1], 16) == _fnv1a(y.tobytes())
    eng.close()
