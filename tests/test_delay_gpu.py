"""Per-channel input and output delays (bfir_engine_delay_init / _set_delay; csrc/delay.hip).

One rule serves nearly every case: the delayed engine's bytes equal the plain engine of the same shape and chunk, run
with the same calls, fed the host-modelled delayed stream (input side), or the host model applied to the plain engine's
output bytes (output side).  Whole-sample delays involve no arithmetic, so those checks are bitwise; the sub-sample
stage is compared within the project's TOL[s] against a float64 direct-form model of the same taps."""
import os
import subprocess

import numpy as np
import pytest

from conftest import TOL, rel_err
from size_matrix import delay_n_blocks, uneven_calls   # shared with the delay cells of the size matrix

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN, OUT = 0, 1
# (realsize, L, B, C, delays): delays below, at and past a block; a piece shorter than the history (L = 16, 37 frames)
SHAPES = [(4, 16, 3, 3, (0, 1, 37)), (4, 512, 2, 2, (511, 513)), (8, 1024, 2, 1, (2048,)),
          (4, 256, 2, 8, (0, 5, 255, 256, 257, 600, 1, 1024))]
PATTERNS = ("one", "blocks", "uneven")


_n_blocks = delay_n_blocks   # 2 ceil(max_delay / L) + 3


def _calls(pattern, nb):
    if pattern == "one":
        return [nb]
    if pattern == "blocks":
        return [1] * nb
    return uneven_calls(nb)   # 2, 1, 3, 2, 1, 3, ...


def shift_model(u, L, delays):
    """w_c[n] = u_c[n - d_c(block of n)], zero bytes before the stream: `delays` is one tuple, or one per block."""
    u = np.asarray(u)
    w = np.zeros_like(u)
    nb = u.shape[0] // L
    per_block = delays if isinstance(delays, list) else [delays] * nb
    for t in range(nb):
        for c, d in enumerate(per_block[t]):
            idx = np.arange(t * L, (t + 1) * L) - d
            ok = idx >= 0
            w[t * L:(t + 1) * L, c][ok] = u[idx[ok], c]
    return w


def _run(eng, x, calls, entry="run", n_out=None):
    """The engine over x in the given calls (blocks per call); host pointers or device pointers."""
    L = eng.L
    if entry == "run":
        outs, pos = [], 0
        for n in calls:
            rc, y = eng.run(x[pos * L:(pos + n) * L])
            assert rc == 0
            outs.append(y.copy())
            pos += n
        return np.concatenate(outs)
    import torch
    x = np.ascontiguousarray(x)
    d_in = torch.from_numpy(x).cuda()
    d_out = torch.zeros((x.shape[0], n_out or x.shape[1]), dtype=d_in.dtype, device="cuda")
    torch.cuda.synchronize()
    fin, fout, pos = x.shape[1] * x.itemsize, d_out.shape[1] * x.itemsize, 0
    for n in calls:
        eng.run_device(d_in.data_ptr() + pos * L * fin, d_out.data_ptr() + pos * L * fout, n)
        pos += n
    assert eng.sync() == 0
    return d_out.cpu().numpy()


def _pair(bfir, orc, s, L, B, C, seed=0, **kw):
    """Two engines of one shape with the same filters; dt of their frames."""
    dt = orc.real_dtype(s)
    h = orc.synth_ir(np.random.default_rng(seed), C, B * L - 3, dt)
    engs = []
    for _ in range(2):
        e = bfir.Brutefir(L, B, s, C, **kw)
        assert e.set_coeff(h) == 0
        engs.append(e)
    return engs[0], engs[1], dt


# ---- 1, 2: whole samples, either side ----------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["run", "run_device"])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "s%d_L%d_C%d" % (v[0], v[1], v[3]))
@pytest.mark.parametrize("side", [IN, OUT])
def test_whole_sample_delay_is_a_byte_shift(orc, bfir, side, shape, pattern, entry):
    s, L, B, C, delays = shape
    nb = _n_blocks(max(delays), L)
    eng, plain, dt = _pair(bfir, orc, s, L, B, C)
    assert eng.delay_init(side, max(delays)) == 0 and eng.set_delay(side, delays) == 0
    assert eng.get_delay(side) == (list(delays), [0] * C) and eng.delay_latency(side) == 0
    x = orc.synth_audio(np.random.default_rng(1), nb * L, C, dt)
    calls = _calls(pattern, nb)
    y = _run(eng, x, calls, entry)
    if side == IN:
        want = _run(plain, shift_model(x, L, delays), calls, entry)
    else:
        want = shift_model(_run(plain, x, calls, entry), L, delays)
    assert y.tobytes() == want.tobytes()
    eng.close(); plain.close()


@pytest.mark.parametrize("fmt", [2, 4], ids=["S16_LE", "S24_LE"])
@pytest.mark.parametrize("side", [IN, OUT])
def test_whole_sample_delay_on_integer_frames(orc, bfir, side, fmt):
    """The delay copies raw sample bytes: 2-byte and 3-byte samples in and out, dither off."""
    s, L, B, C, delays = 4, 64, 2, 3, (0, 7, 150)
    nb = _n_blocks(max(delays), L)
    eng, plain, _ = _pair(bfir, orc, s, L, B, C, in_format=fmt, out_format=fmt, apply_dither=False)
    assert eng.delay_init(side, max(delays)) == 0 and eng.set_delay(side, delays) == 0
    bits = 8 * orc.FMT_BYTES[fmt]
    v = np.random.default_rng(2).integers(-(1 << (bits - 1)), 1 << (bits - 1), (nb * L, C), dtype=np.int64)
    x = orc.encode_ints(v, fmt)
    calls = _calls("uneven", nb)
    y = _run(eng, x, calls)
    want = _run(plain, shift_model(x, L, delays), calls) if side == IN else shift_model(_run(plain, x, calls), L, delays)
    assert y.shape == want.shape and y.tobytes() == want.tobytes() and np.any(y)
    eng.close(); plain.close()


# ---- 3: a matrix engine, both sides -----------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [4, 8])
def test_matrix_engine_with_input_and_output_delays(orc, bfir, s):
    """Pair (o, i) is delayed by d_i + d_o: what zero taps in front of the filters can only set per pair."""
    L, B, n_in, n_out, d_in, d_out = 128, 2, 3, 2, (3, 130, 0), (260, 17)
    dt = orc.real_dtype(s)
    nb = _n_blocks(max(d_in) + max(d_out), L)
    rng = np.random.default_rng(3)
    rows = [[orc.synth_ir(rng, 1, B * L - 9, dt)[0] for _ in range(n_in)] for _ in range(n_out)]
    eng, plain = bfir.BrutefirMatrix(L, B, s, n_in, n_out), bfir.BrutefirMatrix(L, B, s, n_in, n_out)
    assert eng.set_coeff(rows) == 0 and plain.set_coeff(rows) == 0
    assert eng.delay_init(IN, max(d_in)) == 0 and eng.delay_init(OUT, max(d_out)) == 0
    assert eng.set_delay(IN, d_in) == 0 and eng.set_delay(OUT, d_out) == 0
    assert eng.get_delay(IN)[0] == list(d_in) and eng.get_delay(OUT)[0] == list(d_out)
    x = orc.synth_audio(rng, nb * L, n_in, dt)
    calls = _calls("uneven", nb)
    y = _run(eng, x, calls)
    want = shift_model(_run(plain, shift_model(x, L, d_in), calls), L, d_out)
    assert y.tobytes() == want.tobytes()
    ref = np.zeros((nb * L, n_out))
    for o in range(n_out):
        for i in range(n_in):
            hz = np.r_[np.zeros(d_in[i] + d_out[o]), rows[o][i].astype(np.float64)]
            ref[:, o] += np.convolve(x[:, i].astype(np.float64), hz)[:nb * L]
    err = rel_err(y, ref)
    print("matrix s=%d rel err %.3g" % (s, err))
    assert err <= TOL[s]
    eng.close(); plain.close()


# ---- 4: the other kinds -----------------------------------------------------------------------------------------------
def test_levels_engine_with_input_delays(orc, bfir):
    L, blocks, ratios, C, delays = 64, (4, 2, 2), (1, 2, 2), 3, (0, 100, 321)
    nb = _n_blocks(max(delays), L) + 8   # long enough for every level to sound
    h = orc.synth_ir(np.random.default_rng(4), C, 1000, np.float32)
    eng, plain = bfir.BrutefirLevels(L, blocks, ratios, 4, C), bfir.BrutefirLevels(L, blocks, ratios, 4, C)
    assert eng.set_coeff(h) == 0 and plain.set_coeff(h) == 0
    assert eng.delay_init(IN, max(delays)) == 0 and eng.set_delay(IN, delays) == 0
    x = orc.synth_audio(np.random.default_rng(5), nb * L, C, np.float32)
    calls = _calls("uneven", nb)
    assert _run(eng, x, calls).tobytes() == _run(plain, shift_model(x, L, delays), calls).tobytes()
    eng.close(); plain.close()


@pytest.mark.parametrize("kind", ["levels", "matrix_levels"])
def test_output_only_delays_on_a_split_engine_in_many_pieces(orc, bfir, kind):
    """Only the output side delayed, one block per launch and calls of many blocks on device pointers: every block is a
    piece of its own, and a tail level's front in a later piece reads the caller's input on that level's own stream --
    it must wait for the caller's event like the first piece does.  The input is produced on the caller's stream right
    before the call, so a front that did not wait would read it half written."""
    import torch
    L, delays = 64, (0, 100, 321)
    if kind == "levels":
        n_in = n_out = 3
        h = orc.synth_ir(np.random.default_rng(4), n_in, 1000, np.float32)
        mk = lambda: bfir.BrutefirLevels(L, (4, 2, 2), (1, 2, 2), 4, n_in)
    else:
        n_in, n_out = 2, 3
        rng = np.random.default_rng(6)
        h = [[orc.synth_ir(rng, 1, 300 + 100 * (o + i), np.float32)[0] for i in range(n_in)] for o in range(n_out)]
        mk = lambda: bfir.BrutefirMatrixLevels(L, (4, 2), (1, 4), 4, n_in, n_out)
    nb = _n_blocks(max(delays), L) + 8
    eng, plain = mk(), mk()
    for e in (eng, plain):
        assert e.set_coeff(h) == 0
        e.set_chunk(1)
    assert eng.delay_init(OUT, max(delays)) == 0 and eng.set_delay(OUT, delays) == 0
    x = orc.synth_audio(np.random.default_rng(5), nb * L, n_in, np.float32)
    outs = []
    for e in (eng, plain):
        d_src = torch.from_numpy(x).cuda()
        d_in = torch.zeros_like(d_src)
        d_out = torch.zeros((nb * L, n_out), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()   # a stream of the caller's own (a null handle would mean the engine's)
        with torch.cuda.stream(stream):
            for lo, n in ((0, 5), (5, nb - 5)):   # the producer of each call's input is queued on the caller's stream just ahead of it
                d_in[lo * L:(lo + n) * L].copy_(d_src[lo * L:(lo + n) * L])
                e.run_device(d_in.data_ptr() + lo * L * n_in * 4, d_out.data_ptr() + lo * L * n_out * 4, n, stream=stream.cuda_stream)
        assert e.sync() == 0
        outs.append(d_out.cpu().numpy())
    assert outs[0].tobytes() == shift_model(outs[1], L, delays).tobytes()
    eng.close(); plain.close()


def test_matrix_levels_engine_with_input_delays(orc, bfir):
    L, blocks, ratios, n_in, n_out, delays = 64, (4, 2), (1, 4), 2, 3, (45, 200)
    nb = _n_blocks(max(delays), L) + 8
    rng = np.random.default_rng(6)
    rows = [[orc.synth_ir(rng, 1, 300 + 100 * (o + i), np.float32)[0] for i in range(n_in)] for o in range(n_out)]
    mk = lambda: bfir.BrutefirMatrixLevels(L, blocks, ratios, 4, n_in, n_out)
    eng, plain = mk(), mk()
    assert eng.set_coeff(rows) == 0 and plain.set_coeff(rows) == 0
    assert eng.delay_init(IN, max(delays)) == 0 and eng.set_delay(IN, delays) == 0
    x = orc.synth_audio(rng, nb * L, n_in, np.float32)
    calls = _calls("uneven", nb)
    assert _run(eng, x, calls).tobytes() == _run(plain, shift_model(x, L, delays), calls).tobytes()
    eng.close(); plain.close()


def test_delay_set_while_a_fade_runs(orc, bfir):
    s, L, B, C, delays = 4, 128, 2, 2, (200, 31)
    eng, plain, dt = _pair(bfir, orc, s, L, B, C)
    h2 = orc.synth_ir(np.random.default_rng(7), C, B * L - 3, dt)
    nb = 9
    assert eng.delay_init(IN, max(delays)) == 0
    x = orc.synth_audio(np.random.default_rng(8), nb * L, C, dt)
    per_block = [(0, 0)] * 3 + [delays] * (nb - 3)
    xm = shift_model(x, L, per_block)
    ys, ws = [], []
    for e, src, out in ((eng, x, ys), (plain, xm, ws)):
        out.append(_run(e, src[:2 * L], [2]))
        assert e.set_coeff_fade(h2, 3) == 0
        out.append(_run(e, src[2 * L:3 * L], [1]))       # the first fade block
        if e is eng:
            assert e.fade_remaining() == 2 and e.set_delay(IN, delays) == 0
        out.append(_run(e, src[3 * L:], [2, 4]))         # the fade ends inside the first of these calls
        assert e.fade_remaining() == 0
    assert np.concatenate(ys).tobytes() == np.concatenate(ws).tobytes()
    eng.close(); plain.close()


# ---- 5, 6: changes mid-stream, reset ----------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [IN, OUT])
def test_delay_change_mid_stream_is_a_hard_cut(orc, bfir, side):
    s, L, B, C, max_delay = 4, 64, 2, 2, 150
    eng, plain, dt = _pair(bfir, orc, s, L, B, C)
    assert eng.delay_init(side, max_delay) == 0
    steps = [((10, 0), 3), ((150, 150), 3), ((20, 149), 2), ((0, 0), 3)]   # raise to max_delay, lower, off
    nb = sum(n for _, n in steps)
    x = orc.synth_audio(np.random.default_rng(9), nb * L, C, dt)
    per_block = [d for d, n in steps for _ in range(n)]
    ys, pos = [], 0
    for d, n in steps:
        assert eng.set_delay(side, d) == 0 and eng.get_delay(side) == (list(d), [0, 0])
        ys.append(_run(eng, x[pos * L:(pos + n) * L], [n]))
        pos += n
    calls = [n for _, n in steps]
    want = _run(plain, shift_model(x, L, per_block), calls) if side == IN else shift_model(_run(plain, x, calls), L, per_block)
    assert np.concatenate(ys).tobytes() == want.tobytes()
    eng.close(); plain.close()


def test_reset_zeroes_the_histories_and_keeps_the_settings(orc, bfir):
    s, L, B, C, d_in, d_out = 4, 64, 2, 2, (70, 3), (0, 129)
    eng, plain, dt = _pair(bfir, orc, s, L, B, C)
    assert eng.delay_init(IN, 70) == 0 and eng.delay_init(OUT, 129) == 0
    assert eng.set_delay(IN, d_in) == 0 and eng.set_delay(OUT, d_out) == 0
    rng = np.random.default_rng(10)
    for part in range(2):   # the second part: both streams restart from n = 0; the engines proper share the kept input block
        x = orc.synth_audio(rng, 6 * L, C, dt)
        y = _run(eng, x, [6])
        want = shift_model(_run(plain, shift_model(x, L, d_in), [6]), L, d_out)
        assert y.tobytes() == want.tobytes(), part
        eng.reset(); plain.reset()
        assert eng.get_delay(IN)[0] == list(d_in) and eng.get_delay(OUT)[0] == list(d_out)
    eng.close(); plain.close()


# ---- 7, 8, 9: the sub-sample stage ------------------------------------------------------------------------------------
SUB_H, SUB_STEPS, SUB_SUB, SUB_DELAYS = 4, 10, (0, 3, -7, 9), (5, 0, 70, 130)
SUB_CASES = [(4, 8), (8, 10), (8, 8)]   # (realsize, frame format): fp32, fp64, FLOAT_LE frames on the fp64 engine


def sub_model(bfir, u, s, frame_dt):
    """float64 direct form of the stage with the library's taps, rounded once to the frame type; the channel without a
    filter is the shift by d + h."""
    n = u.shape[0]
    w = np.zeros((n, u.shape[1]), frame_dt)
    for c, (d, sd) in enumerate(zip(SUB_DELAYS, SUB_SUB)):
        if sd == 0:
            w[d + SUB_H:, c] = u[:n - d - SUB_H, c]
            continue
        f = bfir.subdelay_filter(SUB_H, sd, SUB_STEPS, 9.0, s).astype(np.float64)
        full = np.convolve(u[:, c].astype(np.float64), f)[:n]
        w[d:, c] = full[:n - d].astype(frame_dt)
    return w


def _sub_engines(bfir, orc, s, fmt):
    eng, plain, _ = _pair(bfir, orc, s, 64, 2, 4, in_format=fmt, out_format=fmt)
    frame_dt = np.float32 if fmt == 8 else np.float64
    nb = _n_blocks(max(SUB_DELAYS) + 2 * SUB_H, 64)
    x = orc.synth_audio(np.random.default_rng(11), nb * 64, 4, frame_dt)
    return eng, plain, frame_dt, nb, x


@pytest.mark.parametrize("s,fmt", SUB_CASES)
def test_sub_sample_delay_on_the_input_side(orc, bfir, s, fmt):
    eng, plain, frame_dt, nb, x = _sub_engines(bfir, orc, s, fmt)
    assert eng.delay_init(IN, max(SUB_DELAYS), SUB_STEPS, SUB_H, 9.0) == 0
    assert eng.set_delay(IN, SUB_DELAYS, SUB_SUB) == 0
    assert eng.get_delay(IN) == (list(SUB_DELAYS), list(SUB_SUB))
    assert eng.delay_latency(IN) == SUB_H and eng.delay_latency(OUT) == 0
    calls = _calls("uneven", nb)
    y = _run(eng, x, calls)
    want = _run(plain, sub_model(bfir, x, s, frame_dt), calls)
    err = rel_err(y, want)
    print("sub-sample input s=%d fmt=%d rel err %.3g" % (s, fmt, err))
    assert err <= TOL[s]
    # L = 64 is below the range of the kernels that transform two channels at once, so in all three cases a channel's
    # output depends on that channel alone: the channel that is only shifted (by d + h) gives the plain engine's bytes
    assert y[:, 0].tobytes() == want[:, 0].tobytes()
    eng.close(); plain.close()


@pytest.mark.parametrize("s,fmt", SUB_CASES)
def test_sub_sample_delay_on_the_output_side(orc, bfir, s, fmt):
    eng, plain, frame_dt, nb, x = _sub_engines(bfir, orc, s, fmt)
    assert eng.delay_init(OUT, max(SUB_DELAYS), SUB_STEPS, SUB_H, 9.0) == 0
    assert eng.set_delay(OUT, SUB_DELAYS, SUB_SUB) == 0 and eng.delay_latency(OUT) == SUB_H
    calls = _calls("blocks", nb)
    y = _run(eng, x, calls)
    want = sub_model(bfir, _run(plain, x, calls), s, frame_dt)
    err = rel_err(y, want)
    print("sub-sample output s=%d fmt=%d rel err %.3g" % (s, fmt, err))
    assert err <= TOL[s]
    assert y[:, 0].tobytes() == want[:, 0].tobytes()   # no filter: a pure shift of the bytes by d + h
    eng.close(); plain.close()


def test_sub_sample_result_does_not_depend_on_how_blocks_arrive(orc, bfir):
    outs = []
    for mode in ("one", "blocks", "chunk1"):
        eng, plain, frame_dt, nb, x = _sub_engines(bfir, orc, 4, 8)
        plain.close()
        if mode == "chunk1":
            eng.set_chunk(1)
        assert eng.delay_init(IN, max(SUB_DELAYS), SUB_STEPS, SUB_H, 9.0) == 0
        assert eng.set_delay(IN, SUB_DELAYS, SUB_SUB) == 0
        outs.append(_run(eng, x, _calls("blocks" if mode == "blocks" else "one", nb)).tobytes())
        eng.close()
    assert outs[0] == outs[1] == outs[2]


# ---- 10: errors -------------------------------------------------------------------------------------------------------
def test_every_error_of_the_delay_calls_and_a_refused_call_changes_nothing(orc, bfir):
    import ctypes as C
    lib = bfir.load()
    A, U, S = bfir.ERR_ARG, bfir.ERR_UNSUPPORTED, bfir.ERR_STATE
    s, L, B, Cn = 4, 64, 2, 2
    eng, twin, dt = _pair(bfir, orc, s, L, B, Cn)
    ints = (C.c_int * 8)()
    # a side never initialised
    assert eng.set_delay(IN, (0, 0)) == S and lib.bfir_engine_get_delay(eng.handle, IN, ints, ints, Cn) == S
    assert eng.delay_latency(IN) == 0
    # delay_init
    for side in (-1, 2):
        assert eng.delay_init(side, 10) == A and eng.delay_latency(side) == A
    for md in (-1, (1 << 24) + 1):
        assert eng.delay_init(IN, md) == A
    for steps in (1, -2):
        assert eng.delay_init(IN, 10, steps, 4) == A
    for h in (0, 129, -1):
        assert eng.delay_init(IN, 10, 10, h) == A
    batch = bfir.Brutefir(L, B, s, Cn, n_engines=2)
    assert batch.delay_init(IN, 10) == U
    batch.close()
    i16 = bfir.Brutefir(L, B, s, Cn, in_format=2, out_format=8)
    assert i16.delay_init(IN, 10, 10, 4) == U and i16.delay_init(OUT, 10, 10, 4) == 0 and i16.delay_init(IN, 10) == 0
    i16.close()
    m = bfir.BrutefirMatrix(L, B, s, 3, 2)
    assert m.delay_init(IN, 5) == 0 and m.delay_init(OUT, 5) == 0
    assert m.set_delay(IN, (1, 2)) == A and m.set_delay(IN, (1, 2, 3)) == 0      # the side's channel count: inputs ...
    assert m.set_delay(OUT, (1, 2, 3)) == A and m.set_delay(OUT, (1, 2)) == 0    # ... and outputs
    assert lib.bfir_engine_get_delay(m.handle, OUT, ints, ints, 3) == A
    m.close()
    # the engines under test: whole samples on the input side, the stage on the output side
    for e in (eng, twin):
        assert e.delay_init(IN, 100) == 0 and e.delay_init(OUT, 50, 10, 4) == 0
        assert e.set_delay(IN, (100, 9)) == 0 and e.set_delay(OUT, (50, 0), (-9, 9)) == 0
    x = orc.synth_audio(np.random.default_rng(12), 6 * L, Cn, dt)
    assert _run(eng, x[:4 * L], [2, 2]).tobytes() == _run(twin, x[:4 * L], [2, 2]).tobytes()
    before = (eng.get_delay(IN), eng.get_delay(OUT))
    assert eng.set_delay(IN, (101, 0)) == A and eng.set_delay(IN, (0, -1)) == A            # outside 0 .. max_delay
    assert eng.set_delay(IN, (1,)) == A and eng.set_delay(IN, (1, 2, 3)) == A                # not the channel count
    assert eng.set_delay(IN, (1, 2), (0, 1)) == A                                              # no stage on this side
    assert eng.set_delay(OUT, (1, 2), (10, 0)) == A and eng.set_delay(OUT, (1, 2), (0, -10)) == A   # |subdelay| >= step_count
    assert eng.set_delay(2, (1, 2)) == A
    assert lib.bfir_engine_set_delay(eng.handle, IN, None, None, Cn) == A
    assert lib.bfir_engine_get_delay(eng.handle, IN, None, ints, Cn) == A and lib.bfir_engine_get_delay(eng.handle, IN, ints, None, Cn) == A
    assert (eng.get_delay(IN), eng.get_delay(OUT)) == before
    assert _run(eng, x[4 * L:], [1, 1]).tobytes() == _run(twin, x[4 * L:], [1, 1]).tobytes()
    # delay_init again: that side's history is discarded and its delays are 0
    assert eng.delay_init(IN, 100) == 0 and eng.get_delay(IN) == ([0, 0], [0, 0]) and eng.get_delay(OUT) == before[1]
    eng.close(); twin.close()


# ---- 11: the C++ mirror -----------------------------------------------------------------------------------------------
def _fnv1a(data):
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return h


def test_cpp_mirror_delays_like_the_ctypes_engine(tmp_path, bfir):
    """tests/cpp/test_delay_mirror.cpp builds its input and filters from integer recurrences (restated here), delays
    both sides of a brutefir one block per run() and prints the FNV-1a hash of its output bytes."""
    src = os.path.join(ROOT, "tests", "cpp", "test_delay_mirror.cpp")
    exe = str(tmp_path / "test_delay_mirror")
    libdir = os.path.dirname(bfir.library_path())
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", src, "-o", exe, "-L" + libdir, "-lbfir_hip",
                    "-Wl,-rpath," + libdir], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "ALL OK" in p.stdout
    L, B, Cn, taps, nb = 256, 2, 2, 500, 10
    i = np.arange(nb * L * Cn, dtype=np.uint64)
    x = ((((i * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(8)).astype(np.float64) / 16777216.0 - 0.5)
    x = x.astype(np.float32).reshape(nb * L, Cn)
    n = np.arange(taps, dtype=np.uint64)
    h = []
    for c in range(Cn):
        v = (((n + np.uint64(1)) * np.uint64(40503 * (c + 3))) & np.uint64(0xffff)).astype(np.float64) / 65536.0 - 0.5
        h.append((v / (64.0 * (1.0 + n.astype(np.float64) / 64.0))).astype(np.float32))
    eng = bfir.Brutefir(L, B, 4, Cn)
    assert eng.set_coeff(h) == 0
    assert eng.delay_init(IN, 300) == 0 and eng.delay_init(OUT, 40, 10, 8, 9.0) == 0
    assert eng.set_delay(IN, (300, 17)) == 0 and eng.set_delay(OUT, (0, 40), (3, -4)) == 0
    y = _run(eng, x, [1] * nb)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("checksum ")]
    assert line and int(line[0].split()[1], 16) == _fnv1a(y.tobytes())
    eng.close()
