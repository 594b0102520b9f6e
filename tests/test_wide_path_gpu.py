"""The forward kernel with 16-byte frame loads (csrc/wide.hip, k_fwd_wide_ps): two channel pairs in turn per workgroup.

It does per pair what k_fwd_pair_ps does, so everything the engine produces behind it -- output frames, return codes,
overflow counts, peaks per channel -- is compared BIT FOR BIT with the pair kernel in the same process: BFIR_FWD_WIDE=1 at
engine creation takes the wide kernel wherever it applies (by default only launches that fill the GPU get it),
BFIR_FWD_WIDE=0 never.  Which kernel ran cannot be seen from the output, so the tests read the library's launch counter.
One run of each shape also goes against the oracle at the tolerance of tests/test_pair_path_gpu.py.

L = 4096 (N = 8192, the headline's instantiation) is the smallest size at which the kernel itself runs.  N = 1024 has no
wide instantiation (it would lower the occupancy of that size) and N = 4096 has none either (it spills at four waves per
SIMD, tests/test_wide_isa.py), so at L = 512 and L = 2048 the forced switch must leave the launches to the pair kernel and
change nothing.

The history (the raw frames of a chunk's last two blocks) has one layout for both kernels, and a launch of one block
(`n_t == 1`) moves the older history block on itself: calls of (1, 2, 3, 5, 9) blocks at four blocks per launch hand the
history over between launches of every length."""
import ctypes

import numpy as np
import pytest

from conftest import TOL, env_override, rel_err

pytestmark = pytest.mark.gpu

SIZES = [(512, False), (2048, False), (4096, True)]    # L, whether N = 2L has a wide instantiation
CALLS = (1, 2, 3, 5, 9)        # blocks per call at set_chunk(4): several launches, runs ending on either side, one-block chunks
CHUNK = 4


def _blocks_per_filter(L):
    return 3 if L == 512 else 2


def _wide_launches(bfir):
    fn = bfir.load().bfir_fwd_wide_launches
    fn.restype = ctypes.c_int64
    return fn()


def _quad_launches(bfir):
    fn = bfir.load().bfir_inv_quad_launches
    fn.restype = ctypes.c_int64
    return fn()


def _engine(bfir, env, L, B, C, h, chunk, n_engines=1):
    with env_override(**env):
        eng = bfir.Brutefir(L, B, 4, C, n_engines=n_engines)
    eng.set_chunk(chunk)
    for g in range(n_engines):
        assert eng.set_coeff(h[g], engine_index=g) == 0
    return eng


def _stats(eng, n):
    return [(o.n_overflows, o.largest) for o in (eng.overflow(c) for c in range(n))]


def _both_paths(bfir, L, B, C, h, segs, chunk=CHUNK, n_engines=1, expect_wide=True, run_len=None, quad=None):
    """Feed the calls `segs` to a wide engine and to a pair engine; -> per path (rcs, outputs, statistics).
    run_len: blocks per workgroup of the wide kernel (BFIR_WIDE_RUN_FWD, read per launch); None = the launcher's choice,
    which is ONE block for launches as small as these -- the loop over blocks only turns with it set.
    quad: True sets BFIR_INV_QUAD to the same value as BFIR_FWD_WIDE (the headline's combination)."""
    res = {}
    for wide in ("1", "0"):
        env = {"BFIR_FWD_WIDE": wide}
        if quad:
            env["BFIR_INV_QUAD"] = wide
        eng = _engine(bfir, env, L, B, C, h, chunk, n_engines)
        n0, q0 = _wide_launches(bfir), _quad_launches(bfir)
        rcs, ys = [], []
        with env_override(BFIR_WIDE_RUN_FWD=run_len, BFIR_QUAD_RUN_INV=run_len if quad else None):
            for seg in segs:
                rc, y = eng.run(seg)
                rcs.append(rc); ys.append(y)
        took = _wide_launches(bfir) - n0
        assert (took > 0) == (wide == "1" and expect_wide), (wide, took)
        if wide == "1" and expect_wide:                      # every call, those of one block included
            assert took >= len(segs), took
        if quad:
            assert (_quad_launches(bfir) - q0 > 0) == (wide == "1")
        res[wide] = (rcs, ys, _stats(eng, C * n_engines))
        eng.close()
    return res


def _assert_same_bits(res):
    (rw, yw, sw), (rp, yp, sp) = res["1"], res["0"]
    assert rw == rp
    for a, b in zip(yw, yp):
        assert np.array_equal(a, b, equal_nan=True)
    assert sw == sp                                          # counts and peaks, every channel, exactly


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


def _wraps(calls, chunk, ring, run_len):
    """(ring wraps in the stream, those that fall between two blocks of one workgroup's run): absolute block j lives in
    slot j % ring, a call goes out in launches of at most `chunk` blocks, a launch in runs of `run_len`"""
    total, inside, pos = 0, 0, 0
    for nb in calls:
        for c0 in range(0, nb, chunk):
            for t in range(min(chunk, nb - c0)):
                j = pos + c0 + t                             # the delay line wraps between blocks j - 1 and j
                if j > 0 and j % ring == 0:
                    total += 1
                    inside += t % run_len != 0
        pos += nb
    return total, inside


def _check_against_oracle(orc, L, B, C, h, segs, ys, n_engines=1):
    for g in range(n_engines):                               # one engine at a time, the same calls
        ref = orc.Engine(L, B, 4, C); ref.set_coeff(h[g])
        for seg, y in zip(segs, ys):
            _, y_ref = ref.run(seg if n_engines == 1 else seg[g])
            assert rel_err(y if n_engines == 1 else y[g], y_ref) <= TOL[4]


@pytest.mark.parametrize("run_len", [None, 2, 3])
@pytest.mark.parametrize("C,n_engines", [(4, 1), (8, 1), (4, 2), (4, 3), (8, 2)])
@pytest.mark.parametrize("L,has_wide", SIZES)
def test_wide_equals_pair_bit_for_bit_over_calls_and_chunks(orc, bfir, L, has_wide, C, n_engines, run_len):
    B = _blocks_per_filter(L)
    assert _wraps(CALLS, CHUNK, 2 * CHUNK + B, run_len or 1)[0] >= 1     # the 20 blocks go round the delay line
    h, x = _stream(orc, C, B * L - 11, sum(CALLS), L, seed=100 * n_engines + C, n_engines=n_engines)
    segs = _cut(x, L, CALLS)
    res = _both_paths(bfir, L, B, C, h, segs, n_engines=n_engines, expect_wide=has_wide, run_len=run_len)
    _assert_same_bits(res)
    assert all(rc == 0 for rc in res["1"][0])
    _check_against_oracle(orc, L, B, C, h, segs, res["1"][1], n_engines)


@pytest.mark.parametrize("run_len", [2, 3])
def test_ring_wrap_inside_a_run(orc, bfir, run_len):
    """The calls above in the other order, (9, 5, 3, 2, 1): in the order above every wrap of the ring of 2 * 4 + B slots falls
    between two launches; in this one the delay line wraps between two blocks that ONE workgroup transforms."""
    L, C, calls = 4096, 8, CALLS[::-1]
    B = _blocks_per_filter(L)
    assert _wraps(calls, CHUNK, 2 * CHUNK + B, run_len)[1] >= 1
    h, x = _stream(orc, C, B * L - 11, sum(calls), L, seed=77)
    segs = _cut(x, L, calls)
    res = _both_paths(bfir, L, B, C, h, segs, run_len=run_len)
    _assert_same_bits(res)
    _check_against_oracle(orc, L, B, C, h, segs, res["1"][1])


@pytest.mark.parametrize("L,has_wide", SIZES)
def test_one_call_equals_single_block_calls_on_the_wide_path(orc, bfir, L, has_wide):
    B, C, nb = _blocks_per_filter(L), 8, 9
    h, x = _stream(orc, C, B * L - 11, nb, L, seed=31)
    whole = _both_paths(bfir, L, B, C, h, _cut(x, L, (nb,)), expect_wide=has_wide)
    parts = _both_paths(bfir, L, B, C, h, _cut(x, L, (1,) * nb), expect_wide=has_wide)
    _assert_same_bits(whole)
    _assert_same_bits(parts)
    for wide in ("1", "0"):                                  # for both switch values
        assert np.array_equal(np.concatenate(parts[wide][1]), whole[wide][1][0])
        assert parts[wide][2] == whole[wide][2]


@pytest.mark.parametrize("C", [6, 2, 5])
@pytest.mark.parametrize("L", [512, 4096])
def test_channel_counts_the_wide_kernel_does_not_take(orc, bfir, L, C):
    """C = 6 and C = 2 stay on the pair kernel, an odd C on the time-pair kernel"""
    B, nb = _blocks_per_filter(L), 9
    h, x = _stream(orc, C, B * L - 11, nb, L, seed=C)
    res = _both_paths(bfir, L, B, C, h, _cut(x, L, (nb,)), expect_wide=False)
    _assert_same_bits(res)
    ref = orc.Engine(L, B, 4, C); ref.set_coeff(h[0])
    assert rel_err(res["1"][1][0], ref.run(x[0])[1]) <= TOL[4]


@pytest.mark.parametrize("value", [np.nan, np.inf])
@pytest.mark.parametrize("L,has_wide", [(512, False), (4096, True)])
def test_non_finite_input_in_either_pair(orc, bfir, L, has_wide, value):
    """A NaN, and separately an Inf, at sample 0 of block 2, once in channel 0 (pair A), once in channel 3 (pair B), as
    single-block calls and as one call: the same bits (NaNs included) and the same return codes as the pair kernel."""
    B, C, nb, blk = 2, 4, 6, 2
    h = [[np.r_[np.float32(1.0), np.zeros(700, np.float32)] for _ in range(C)]]
    rng = np.random.default_rng(17)
    x = orc.synth_audio(rng, nb * L, C, np.float32)[None]
    for ch in (0, 3):
        bad = x.copy(); bad[0, blk * L, ch] = value
        parts = _both_paths(bfir, L, B, C, h, _cut(bad, L, (1,) * nb), expect_wide=has_wide)
        _assert_same_bits(parts)
        rcs = parts["1"][0]
        assert rcs[:blk] == [0] * blk and rcs[blk] != 0      # the engine refuses the block whose sample 0 is not finite
        whole = _both_paths(bfir, L, B, C, h, _cut(bad, L, (nb,)), expect_wide=has_wide)
        _assert_same_bits(whole)
        assert whole["1"][0] == [-1]


@pytest.mark.parametrize("L", [512, 4096])
def test_misaligned_frames_decline_the_wide_kernel(orc, bfir, L):
    """run_device on frames that start 8 bytes off a 16-byte boundary (a tensor view two floats in): 16-byte loads
    cannot take them, the pair kernel does, also when the wide kernel is forced.  The aligned view of the same data,
    through the same entry, is taken."""
    import torch
    B, C, nb = _blocks_per_filter(L), 8, 5
    h, x = _stream(orc, C, B * L - 11, nb, L, seed=9)
    flat = torch.from_numpy(x[0].reshape(-1))
    outs = {}
    for off in (2, 4):                                       # floats: 8 bytes (declined), 16 bytes (taken where N = 2L is instantiated)
        buf = torch.zeros(flat.numel() + 8, dtype=torch.float32, device="cuda")
        assert buf.data_ptr() % 16 == 0
        d_in = buf[off:off + flat.numel()]
        d_in.copy_(flat)
        assert d_in.data_ptr() % 16 == (8 if off == 2 else 0)
        for wide in ("1", "0"):
            eng = _engine(bfir, {"BFIR_FWD_WIDE": wide}, L, B, C, h, CHUNK)
            d_out = torch.empty(flat.numel(), dtype=torch.float32, device="cuda")
            n0 = _wide_launches(bfir)
            eng.run_device(d_in.data_ptr(), d_out.data_ptr(), nb)
            assert eng.sync() == 0
            took = _wide_launches(bfir) - n0
            assert (took > 0) == (wide == "1" and off == 4 and L == 4096), (off, wide, took)
            outs[off, wide] = (d_out.cpu().numpy().reshape(nb * L, C), _stats(eng, C))
            eng.close()
    first = outs[2, "0"]
    for got in outs.values():
        assert np.array_equal(got[0], first[0], equal_nan=True) and got[1] == first[1]
    ref = orc.Engine(L, B, 4, C); ref.set_coeff(h[0])
    assert rel_err(outs[2, "1"][0], ref.run(x[0])[1]) <= TOL[4]


@pytest.mark.parametrize("run_len", [None, 4])
def test_headline_combination_with_the_quad_inverse(orc, bfir, run_len):
    """BFIR_FWD_WIDE=1 with BFIR_INV_QUAD=1 against both set to 0"""
    L, B, C, nb = 4096, 2, 8, 9
    h, x = _stream(orc, C, B * L - 11, nb, L, seed=13)
    res = _both_paths(bfir, L, B, C, h, _cut(x, L, (nb,)), run_len=run_len, quad=True)
    _assert_same_bits(res)
    ref = orc.Engine(L, B, 4, C); ref.set_coeff(h[0])
    assert res["1"][0] == [0] and rel_err(res["1"][1][0], ref.run(x[0])[1]) <= TOL[4]


@pytest.mark.parametrize("C,run_len", [(4, None), (8, 2), (8, 3)])
def test_the_largest_instantiation(orc, bfir, C, run_len):
    """N = 16384 (L = 8192) is instantiated and the default leaves it to the pair kernel (it did not pay in the pipeline,
    profiles/wide_io.txt): the forced switch runs it, calls of (1, 3, 4) blocks at four blocks per launch."""
    L, B, calls = 8192, 2, (1, 3, 4)
    h, x = _stream(orc, C, B * L - 11, sum(calls), L, seed=14 + C)
    segs = _cut(x, L, calls)
    res = _both_paths(bfir, L, B, C, h, segs, run_len=run_len)
    _assert_same_bits(res)
    assert all(rc == 0 for rc in res["1"][0])
    _check_against_oracle(orc, L, B, C, h, segs, res["1"][1])


def test_default_takes_filling_launches_only_and_hands_the_history_over(orc, bfir):
    """With BFIR_FWD_WIDE unset a launch of at least 512 quad-blocks goes to the wide kernel and a smaller one to the pair
    kernel: calls of (256, 3, 256, 1, 2) blocks at 256 blocks per launch alternate between the two in ONE engine, each taking
    the other's history (the raw frames of the last two blocks).  Same bits as the pair kernel alone."""
    L, B, C, chunk, calls = 4096, 2, 8, 256, (256, 3, 256, 1, 2)
    h, x = _stream(orc, C, B * L - 11, sum(calls), L, seed=5)
    segs = _cut(x, L, calls)
    out = {}
    for wide in (None, "0"):
        eng = _engine(bfir, {"BFIR_FWD_WIDE": wide}, L, B, C, h, chunk)
        n0 = _wide_launches(bfir)
        with env_override(BFIR_WIDE_RUN_FWD=None):
            got = [eng.run(seg) for seg in segs]
        took = _wide_launches(bfir) - n0
        assert took == (2 if wide is None else 0), (wide, took)      # the two calls of 256 blocks x 2 quads
        out[wide] = ([rc for rc, _ in got], [y for _, y in got], _stats(eng, C))
        eng.close()
    assert out[None][0] == out["0"][0] == [0] * len(calls)
    for a, b in zip(out[None][1], out["0"][1]):
        assert np.array_equal(a, b, equal_nan=True)
    assert out[None][2] == out["0"][2]
    # the oracle on the stream's tail: the last three calls and the filter's memory before them are what the hand-overs touch
    ref = orc.Engine(L, B, 4, C); ref.set_coeff(h[0])
    y_ref = ref.run(x[0])[1]
    assert rel_err(np.concatenate(out[None][1]), y_ref) <= TOL[4]
