"""The inverse kernel with 16-byte frame stores (csrc/quad.hip, k_inv_quad_ps): two channel pairs in turn per workgroup.

It does per pair what k_inv_pair_ps does, so everything it produces -- output frames, overflow counts, peaks per channel,
the NaN verdict -- is compared BIT FOR BIT with the pair kernel in the same process: BFIR_INV_QUAD=1 at engine creation
takes the quad kernel wherever it applies (by default only launches that fill the GPU get it), BFIR_INV_QUAD=0 never.
Which kernel ran cannot be seen from the output, so the tests read the library's launch counter.  One run of each shape
also goes against the oracle at the tolerance of tests/test_pair_path_gpu.py.

Every case runs at L = 512 and at L = 4096.  N = 1024 has no quad instantiation (it would lower the occupancy of that size,
tests/test_quad_isa.py), so at L = 512 the forced switch must leave the launches to the pair kernel and change nothing;
L = 4096 (N = 8192, the headline's instantiation) is the smallest size at which the quad kernel itself runs."""
import ctypes

import numpy as np
import pytest

from conftest import TOL, env_override, rel_err

pytestmark = pytest.mark.gpu

SIZES = [(512, False), (4096, True)]    # L, whether N = 2L has a quad instantiation
CALLS = (1, 2, 3, 5, 9)        # blocks per call at set_chunk(4): several launches, runs ending on either pair, one-block chunks


def _quad_launches(bfir):
    fn = bfir.load().bfir_inv_quad_launches
    fn.restype = ctypes.c_int64
    return fn()


def _engine(bfir, quad, L, B, C, h, chunk, n_engines=1):
    with env_override(BFIR_INV_QUAD=quad):
        eng = bfir.Brutefir(L, B, 4, C, n_engines=n_engines)
    eng.set_chunk(chunk)
    for g in range(n_engines):
        assert eng.set_coeff(h[g], engine_index=g) == 0
    return eng


def _stats(eng, n):
    return [(o.n_overflows, o.largest) for o in (eng.overflow(c) for c in range(n))]


def _both_paths(bfir, L, B, C, h, segs, chunk, n_engines=1, expect_quad=True, run_len=None):
    """Feed the calls `segs` to a quad engine and to a pair engine; -> per path (rcs, outputs, statistics).
    run_len: blocks per workgroup of the quad kernel (BFIR_QUAD_RUN_INV, read per launch); None = the launcher's choice,
    which is ONE block for launches as small as these -- the loop over blocks only turns with it set."""
    res = {}
    for quad in ("1", "0"):
        eng = _engine(bfir, quad, L, B, C, h, chunk, n_engines)
        n0 = _quad_launches(bfir)
        rcs, ys = [], []
        with env_override(BFIR_QUAD_RUN_INV=run_len):
            for seg in segs:
                rc, y = eng.run(seg)
                rcs.append(rc); ys.append(y)
        took = _quad_launches(bfir) - n0
        assert (took > 0) == (quad == "1" and expect_quad), (quad, took)
        res[quad] = (rcs, ys, _stats(eng, C * n_engines))
        eng.close()
    return res


def _assert_same_bits(res):
    (rq, yq, sq), (rp, yp, sp) = res["1"], res["0"]
    assert rq == rp
    for a, b in zip(yq, yp):
        assert np.array_equal(a, b, equal_nan=True)
    assert sq == sp                                          # counts and peaks, every channel, exactly


def _stream(orc, C, taps, blocks, L, seed, n_engines=1):
    rng = np.random.default_rng(seed)
    h = [orc.synth_ir(rng, C, taps, np.float32) for _ in range(n_engines)]
    x = np.stack([orc.synth_audio(rng, blocks * L, C, np.float32) for _ in range(n_engines)])
    return h, x


def _cut(x, L, calls):
    """[n_engines, frames, C] -> one array per call (the engine dimension dropped for a single engine)"""
    out, pos = [], 0
    for nb in calls:
        seg = x[:, pos * L:(pos + nb) * L]
        out.append(np.ascontiguousarray(seg[0] if x.shape[0] == 1 else seg))
        pos += nb
    return out


def test_three_quads_need_three_engines(bfir):
    """Twelve channels (three quads in one engine) cannot be built: an engine takes at most BFIR_MAXCHANNELS = 8, the
    reference's limit (brutefir.cpp:652).  A work map of three units, and one with two quads in each of two engines,
    come from batches of engines below."""
    with pytest.raises(bfir.BfirError):
        bfir.Brutefir(512, 3, 4, 12)


@pytest.mark.parametrize("run_len", [None, 2, 3])
@pytest.mark.parametrize("C,n_engines", [(4, 1), (8, 1), (4, 2), (4, 3), (8, 2)])
@pytest.mark.parametrize("L,has_quad", SIZES)
def test_quad_equals_pair_bit_for_bit_over_calls_and_chunks(orc, bfir, L, has_quad, C, n_engines, run_len):
    B = 3 if L == 512 else 2
    h, x = _stream(orc, C, B * L - 11, sum(CALLS), L, seed=100 * n_engines + C, n_engines=n_engines)
    segs = _cut(x, L, CALLS)
    res = _both_paths(bfir, L, B, C, h, segs, 4, n_engines, expect_quad=has_quad, run_len=run_len)
    _assert_same_bits(res)
    assert all(rc == 0 for rc in res["1"][0])
    for g in range(n_engines):                               # the oracle: one engine at a time, the same calls
        ref = orc.Engine(L, B, 4, C); ref.set_coeff(h[g])
        for seg, y in zip(segs, res["1"][1]):
            _, y_ref = ref.run(seg if n_engines == 1 else seg[g])
            assert rel_err(y if n_engines == 1 else y[g], y_ref) <= TOL[4]


@pytest.mark.parametrize("L,has_quad", SIZES)
def test_one_call_equals_single_block_calls_on_the_quad_path(orc, bfir, L, has_quad):
    B, C, nb = 3 if L == 512 else 2, 8, 9
    h, x = _stream(orc, C, B * L - 11, nb, L, seed=31)
    whole = _both_paths(bfir, L, B, C, h, _cut(x, L, (nb,)), 4, expect_quad=has_quad)
    parts = _both_paths(bfir, L, B, C, h, _cut(x, L, (1,) * nb), 4, expect_quad=has_quad)
    _assert_same_bits(whole)
    _assert_same_bits(parts)
    assert np.array_equal(np.concatenate(parts["1"][1]), whole["1"][1][0])
    assert parts["1"][2] == whole["1"][2]


@pytest.mark.parametrize("run_len", [None, 2, 4])
def test_headline_instantiation(orc, bfir, run_len):
    L, B, C, nb = 4096, 2, 8, 9
    h, x = _stream(orc, C, B * L - 11, nb, L, seed=13)
    res = _both_paths(bfir, L, B, C, h, _cut(x, L, (nb,)), 4, run_len=run_len)
    _assert_same_bits(res)
    ref = orc.Engine(L, B, 4, C); ref.set_coeff(h[0])
    assert res["1"][0] == [0] and rel_err(res["1"][1][0], ref.run(x[0])[1]) <= TOL[4]


@pytest.mark.parametrize("C", [6, 2])
@pytest.mark.parametrize("L", [512, 4096])
def test_channel_counts_the_quad_kernel_does_not_take_stay_on_the_pair_kernel(orc, bfir, L, C):
    B, nb = 3 if L == 512 else 2, 9
    h, x = _stream(orc, C, B * L - 11, nb, L, seed=C)
    res = _both_paths(bfir, L, B, C, h, _cut(x, L, (nb,)), 4, expect_quad=False)
    _assert_same_bits(res)
    ref = orc.Engine(L, B, 4, C); ref.set_coeff(h[0])
    assert rel_err(res["1"][1][0], ref.run(x[0])[1]) <= TOL[4]


@pytest.mark.parametrize("L,has_quad", SIZES)
def test_overflow_statistics_of_both_pairs(orc, bfir, L, has_quad):
    """Channels 1 (pair A) and 2 (pair B) clip, 0 and 3 do not."""
    B, C, nb = 2, 4, 10 if L == 512 else 4
    rng = np.random.default_rng(10)   # no |sample| within 1e-5 of the clip threshold (tests/test_pair_path_gpu.py)
    h = [[np.r_[np.float32(g), np.zeros(700, np.float32)] for g in (0.5, 3.0, 3.0, 0.25)]]   # pure gains
    x = orc.synth_audio(rng, nb * L, C, np.float32)[None]
    res = _both_paths(bfir, L, B, C, h, _cut(x, L, (nb,)), 4, expect_quad=has_quad)
    _assert_same_bits(res)
    ref = orc.Engine(L, B, 4, C); ref.set_coeff(h[0]); _, y_ref = ref.run(x[0])
    assert np.abs(np.abs(y_ref.astype(np.float64)) - 1.0).min() > 1e-5   # nothing sits on the threshold
    stats = res["1"][2]
    for c in range(C):
        r = ref.overflow(c)
        assert stats[c][0] == r.n_overflows and abs(stats[c][1] - r.largest) <= 1e-5 * r.largest
    assert stats[0][0] == 0 and stats[3][0] == 0 and stats[1][0] > 0 and stats[2][0] > 0


@pytest.mark.parametrize("L,has_quad", SIZES)
def test_nan_verdict_names_the_same_block_for_either_pair(orc, bfir, L, has_quad):
    """A NaN at sample 0 of block 2, once in channel 0 (pair A), once in channel 3 (pair B).  The library reports a
    verdict per call, so the stream goes in as single-block calls and the first refused call is the reported block;
    the whole stream in one call gives the verdict too."""
    B, C, nb, blk = 2, 4, 6, 2
    h = [[np.r_[np.float32(1.0), np.zeros(700, np.float32)] for _ in range(C)]]
    rng = np.random.default_rng(17)
    x = orc.synth_audio(rng, nb * L, C, np.float32)[None]
    first = {}
    for ch in (0, 3):
        bad = x.copy(); bad[0, blk * L, ch] = np.nan
        parts = _both_paths(bfir, L, B, C, h, _cut(bad, L, (1,) * nb), 4, expect_quad=has_quad)
        _assert_same_bits(parts)
        rcs = parts["1"][0]
        assert rcs[:blk] == [0] * blk and rcs[blk] != 0
        first[ch] = next(t for t, rc in enumerate(rcs) if rc != 0)
        whole = _both_paths(bfir, L, B, C, h, _cut(bad, L, (nb,)), 4, expect_quad=has_quad)
        _assert_same_bits(whole)
        assert whole["1"][0] == [-1]
    assert first[0] == first[3] == blk
