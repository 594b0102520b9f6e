"""k_mac_stream's addressing (csrc/kernels.hip, MacIo): buffer descriptors, a scalar byte offset per sequence, and the
buffer range check in place of the branches round stores and read-backs.

The shapes are the smallest at which that addressing can go wrong, not the workload's: fp32 FLOAT_LE engines at
L = 512 (N = 1024: two bin columns of 256 lanes).  Every case compares the engine with the streaming MAC
(BFIR_MAC_SYS=0) BIT FOR BIT with the same engine on the systolic MAC (BFIR_MAC_SYS=1, own addressing, one fma chain
per output in the same order: tests/test_mac_sys_gpu.py holds the two bit-identical), and sampled blocks with the
oracle at the suite's fp32 tolerance.  Covered: the ring wrap inside a range, every partition batch (PB = 4, 8, 16,
32) with partition counts below the batch, the batches that continue sums left in Y (ACC), a last range shorter than
a group and a launch that is no multiple of the batch (the outputs past the end that must not be stored), several
ranges per column, bin 0 (DC | Nyquist: not the streaming lanes' to write), the channel stride and several engines,
and call-to-call continuation."""
import numpy as np
import pytest

from conftest import TOL
from test_launch_geometry_gpu import _check, _run_calls, _synth

pytestmark = pytest.mark.gpu

L = 512

# name, B, C, n_eng, calls, chunk, env of the streaming engine
CASES = [
    # ring = 2 * 7 + 5 = 19 slots: every launch of 7 blocks walks across slot 0
    ("ring_wrap_21", 5, 2, 1, [21], 7, {}),
    ("ring_wrap_33", 5, 2, 1, [33], 7, {}),
    # every instantiation, full and with zero partitions; 40 blocks, then 9 (n_t below / no multiple of the batch)
    ("B3", 3, 2, 1, [40, 9], 40, {}),
    ("B4", 4, 2, 1, [40, 9], 40, {}),
    ("B7", 7, 2, 1, [40, 9], 40, {}),
    ("B8", 8, 2, 1, [40, 9], 40, {}),
    ("B13", 13, 2, 1, [40, 9], 40, {}),
    ("B16", 16, 2, 1, [40, 9], 40, {}),
    ("B24", 24, 2, 1, [40, 9], 40, {}),
    ("B32", 32, 2, 1, [40, 9], 40, {}),
    # ACC: the second batch of 32 continues the sums in Y; 40 blocks would go to k_mac_lds (BFIR_MAC_BATCHED keeps
    # them here), 20 blocks come here by themselves; with short ranges the read-back runs below block 0 of every range
    ("acc_B40", 40, 2, 1, [40, 20], 40, {"BFIR_MAC_BATCHED": "1"}),
    ("acc_B40_ranges", 40, 2, 1, [40, 20], 40, {"BFIR_MAC_BATCHED": "1", "BFIR_MAC_RANGE": "32"}),
    # last range shorter than a group, n_t no multiple of the batch: 50 = 3 * 16 + 2 and 50 = 32 + 18
    ("tail_PB16", 13, 2, 1, [50], 50, {"BFIR_MAC_RANGE": "16"}),
    ("tail_PB32", 32, 2, 1, [50], 50, {"BFIR_MAC_RANGE": "16"}),
    # several ranges per column: five of one group, and five of two groups
    ("ranges_PB8", 7, 2, 1, [40], 40, {"BFIR_MAC_RANGE": "8"}),
    ("ranges_PB4", 3, 2, 1, [40], 40, {"BFIR_MAC_RANGE": "8"}),
    # channel stride and engines
    ("C6", 8, 6, 1, [40, 9], 40, {}),
    ("three_engines", 8, 2, 3, [40, 9], 40, {}),
    ("C6_three_engines_wrap", 32, 6, 3, [33], 11, {}),
]


def _both(bfir, torch, B, C, hs, d_in, calls, chunk, env):
    sys_env = {k: v for k, v in env.items() if k == "BFIR_MAC_RANGE"}
    ref = _run_calls(bfir, torch, L, B, 4, C, hs, d_in, calls, chunk, dict(sys_env, BFIR_MAC_SYS="1"))
    got = _run_calls(bfir, torch, L, B, 4, C, hs, d_in, calls, chunk, dict(env, BFIR_MAC_SYS="0"))
    for ci, (a, b) in enumerate(zip(got, ref)):
        if not torch.equal(a, b):
            diff = (a != b).any(dim=2).view(a.shape[0], -1, L).any(dim=2)          # [engine, block]
            raise AssertionError("call %d: %d blocks differ from the systolic MAC, first (engine, block): %s"
                                 % (ci, int(diff.sum()), diff.nonzero()[:8].tolist()))
    return got


@pytest.mark.parametrize("name,B,C,n_eng,calls,chunk,env", CASES, ids=[c[0] for c in CASES])
def test_streaming_mac_addressing(orc, bfir, name, B, C, n_eng, calls, chunk, env):
    import torch
    hs = _synth(orc, 4, C, B * L - 37, n_eng, seed=len(name) + B)
    rng = np.random.default_rng(B + C)
    x_host = rng.random((n_eng, max(calls) * L, C), dtype=np.float32)
    x_host *= 2.0; x_host -= 1.0
    d_in = torch.from_numpy(x_host).cuda()
    got = _both(bfir, torch, B, C, hs, d_in, calls, chunk, env)
    worst, n_pts = _check(orc, torch, L, B, 4, C, hs, x_host, calls, got, chunk, lambda tc: 0, max_points=12)
    print("%s: bit-identical to the systolic MAC; oracle: %d sampled blocks, worst rel err %.3g" % (name, n_pts, worst))


def test_bin_zero_is_left_to_the_dc_nyquist_workgroups(orc, bfir):
    """An impulse response with large DC and Nyquist gains, input with a DC offset: bin 0 of every product spectrum is
    then far from what the complex product of the streaming lanes would put there, so a streaming lane that wrote it
    shows against the oracle (and against the systolic MAC)."""
    import torch
    B, C, calls = 8, 2, [40, 9]
    taps = B * L - 37
    sign = 1.0 - 2.0 * (np.arange(taps) % 2)
    hs = [[(0.5 * h + 0.24 / taps + (0.24 / taps) * sign).astype(np.float32) for h in _synth(orc, 4, C, taps, 1, seed=3)[0]]]
    for h in hs[0]:
        assert abs(h.sum()) > 0.2 and abs((h * sign).sum()) > 0.2 and np.abs(h).sum() <= 1.0
    rng = np.random.default_rng(11)
    x_host = (0.5 * rng.random((1, max(calls) * L, C), dtype=np.float32) + 0.45).astype(np.float32)
    d_in = torch.from_numpy(x_host).cuda()
    for env in ({}, {"BFIR_MAC_RANGE": "8"}):
        got = _both(bfir, torch, B, C, hs, d_in, calls, 40, env)
        worst, n_pts = _check(orc, torch, L, B, 4, C, hs, x_host, calls, got, 40, lambda tc: 0, max_points=12)
        print("bin 0 %s: oracle: %d sampled blocks, worst rel err %.3g" % (env, n_pts, worst))


def test_the_same_blocks_in_calls_of_1_2_5_and_32(orc, bfir):
    """Call-to-call continuation: the delay line's base slot and the ring position move on between calls (the calls of
    one and two blocks take the small-run path, the same for both engines)."""
    import torch
    B, C, cuts = 8, 2, [1, 2, 5, 32]
    hs = _synth(orc, 4, C, B * L - 37, 1, seed=5)
    rng = np.random.default_rng(7)
    x_host = rng.random((1, sum(cuts) * L, C), dtype=np.float32)
    x_host *= 2.0; x_host -= 1.0
    d_in = torch.from_numpy(x_host).cuda()
    from test_launch_geometry_gpu import _Env
    outs = {}
    for sys in ("1", "0"):
        with _Env(BFIR_MAC_SYS=sys):
            eng = bfir.Brutefir(L, B, 4, C, 8, 8)
            eng.set_chunk(12)                                  # ring 32: the call of 32 blocks is three launches and wraps
            assert eng.set_coeff(hs[0]) == 0
            d_out = torch.empty_like(d_in)
            t0 = 0
            for n in cuts:
                off = t0 * L * C * 4
                eng.run_device(d_in.data_ptr() + off, d_out.data_ptr() + off, n,
                               stream=torch.cuda.current_stream().cuda_stream)
                assert eng.sync() == 0
                t0 += n
            eng.close()
            outs[sys] = d_out
    assert torch.equal(outs["0"], outs["1"])
    blocks = [0, 1, 2, 3, 7, 8, 9, 23, 24, 39]
    ref = orc.sampled_reference(hs[0], lambda g: x_host[0, g * L:(g + 1) * L], blocks, L, B, 4, C)
    y = outs["0"][0].cpu().numpy().astype(np.float64)
    for g in blocks:
        r = ref[g].astype(np.float64)
        err = float(np.abs(y[g * L:(g + 1) * L] - r).max() / np.abs(r).max())
        assert err <= TOL[4], (g, err)
