"""The delay cells of tests/size_matrix.py on the device: every instance of k_delay_sub and k_delay_copy, every tile shape
and history edge, on every kind of engine (DELAY_SUB_CELLS, DELAY_MID_CELLS, DELAY_COPY_CELLS, DELAY_KIND_CELLS).

The rule is that of tests/test_delay_gpu.py: a twin plain engine of the same shape, filters, chunk and calls.  An
output-side stage is seen alone -- its input u is the twin's output bytes -- and every sample is held to the derived bound of
size_matrix.delay_sub_bound around the float64 direct form of the library's taps on u; an unfiltered channel is the shift
by d + h, bit for bit.  An input-side stage is held to the project's TOL[s] behind the engine.  Whole-sample delays involve
no arithmetic: bytes equal the twin's under shift_model."""
import numpy as np
import pytest

import size_matrix as SM
from conftest import TOL, rel_err
from test_delay_gpu import _run, shift_model

pytestmark = pytest.mark.gpu

IN, OUT = SM.DELAY_IN, SM.DELAY_OUT
WORST = {}          # (side, realsize, frame format) -> (worst figure, cell id): error / bound (output), rel_err (input)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (side, s, fmt), (v, cid) in sorted(WORST.items()):
        print("delay matrix: worst %s realsize %d %s: %.3g at %s" % ("error / bound, output side" if side == OUT else
                                                                     "rel_err, input side", s, SM.FMT_NAMES[fmt], v, cid))


def _note(cell, value):
    key = (cell["side"], cell["s"], cell["fmt"])
    if value >= WORST.get(key, (-1.0, ""))[0]:
        WORST[key] = (value, cell["id"])


# ---- engines ----------------------------------------------------------------------------------------------------------
def _engines(bfir, orc, kind, s, L, n_in, n_out, fmt, seed, n_sets=1, **kw):
    """Two engines of one kind and shape with the same filters (orc.synth_ir); (eng, twin, further filter sets, fade call)."""
    dt, rng = orc.real_dtype(s), np.random.default_rng(seed)
    rows = lambda n: [[orc.synth_ir(rng, 1, n(o, i), dt)[0] for i in range(n_in)] for o in range(n_out)]
    if kind == "plain":
        mk = lambda: bfir.Brutefir(L, 2, s, n_in, in_format=fmt, out_format=fmt, **kw)
        sets = [orc.synth_ir(rng, n_in, 2 * L - 3, dt) for _ in range(n_sets)]
        fade = lambda e, h, K: e.set_coeff_fade(h, K)
    elif kind == "matrix":
        mk = lambda: bfir.BrutefirMatrix(L, 2, s, n_in, n_out, fmt, fmt)
        sets = [rows(lambda o, i: 2 * L - 9) for _ in range(n_sets)]
        fade = lambda e, h, K: e.set_coeff_fade(h, K)
    elif kind == "nup":
        mk = lambda: bfir.BrutefirNup(L, 2, 2, 2, s, n_in, fmt, fmt)
        sets = [orc.synth_ir(rng, n_in, 6 * L - SM.RAGGED, dt) for _ in range(n_sets)]
        fade = lambda e, h, K: e.fade_to(h, K)
    elif kind == "levels":
        mk = lambda: bfir.BrutefirLevels(L, (4, 2, 2), (1, 2, 2), s, n_in, fmt, fmt)
        sets = [orc.synth_ir(rng, n_in, 16 * L - 24, dt) for _ in range(n_sets)]
        fade = lambda e, h, K: e.fade_to(h, K)
    else:
        mk = lambda: bfir.BrutefirMatrixLevels(L, (4, 2), (1, 4), s, n_in, n_out, fmt, fmt)
        sets = [rows(lambda o, i: 5 * L + 100 * (o + i)) for _ in range(n_sets)]
        fade = lambda e, h, K: e.fade_to_rows(h, K)
    eng, twin = mk(), mk()
    assert eng.set_coeff(sets[0]) == 0 and twin.set_coeff(sets[0]) == 0
    return eng, twin, sets[1:], fade


def _run_steps(eng, src, cell, side=None):
    """The cell's calls on src; side: set the step's delays on that side before its calls.  reset() where the step says so."""
    L, steps, outs, pos = cell["L"], SM.delay_sub_steps(cell), [], 0
    for delays, subs, nb, reset in steps:
        if reset:
            eng.reset()
        if side is not None:
            assert eng.set_delay(side, delays, subs) == 0 and eng.get_delay(side) == (list(delays), list(subs))
        outs.append(_run(eng, src[pos * L:(pos + nb) * L], cell["calls"] if len(steps) == 1 else [nb]))
        pos += nb
    return np.concatenate(outs)


def _stage_cell(bfir, orc, cell, kind, chunk):
    s, fmt, L, side, h = cell["s"], cell["fmt"], cell["L"], cell["side"], cell["h"]
    n_in, n_out = cell.get("n_in", cell["C"]), cell.get("n_out", cell["C"])
    eng, twin, _, _ = _engines(bfir, orc, kind, s, L, n_in, n_out, fmt, 11)
    chunk = SM.delay_sub_chunk(cell, chunk)      # set, not left to the automatic choice: the launches are those of
    eng.set_chunk(chunk); twin.set_chunk(chunk)  # size_matrix.delay_sub_launches, whose tile edges the CPU test computes
    assert eng.delay_init(side, cell["max_delay"], cell["steps"], h, cell["beta"]) == 0
    assert eng.delay_latency(side) == h and eng.delay_latency(1 - side) == 0
    F = SM.frame_dtype(fmt)
    x = orc.synth_audio(SM._rng(cell), sum(cell["calls"]) * L, n_in, F)
    y = _run_steps(eng, x, cell, side)
    tag = "%s-chunk%d" % (cell["id"], chunk)
    if side == OUT:
        u = _run_steps(twin, x, cell)
        ref, amp, filt = SM.delay_sub_model(bfir.subdelay_filter, cell, u)
        bound = SM.delay_sub_bound(s, fmt, h, ref, amp)
        err = np.abs(y.astype(np.float64) - ref)
        ratio = float((err[filt] / np.maximum(bound[filt], 1e-300)).max()) if filt.any() else 0.0
        print("%s: worst error / bound %.3g" % (tag, ratio))
        _note(cell, ratio)
        assert np.all(err[filt] <= bound[filt]), np.argwhere(filt & (err > bound))[:4]
        assert y[~filt].tobytes() == ref.astype(F)[~filt].tobytes()            # the shift by d + h, bit for bit
        assert np.any(y[filt]) and (filt.all() or np.any(y[~filt]))
    else:
        ref, _, filt = SM.delay_sub_model(bfir.subdelay_filter, cell, x)
        want = _run_steps(twin, ref.astype(F), cell)                              # rounded once to the frame type
        err = rel_err(y, want)
        print("%s: rel_err %.3g (tol %.3g)" % (tag, err, TOL[s]))
        _note(cell, err)
        assert err <= TOL[s] and np.any(y)
        alone = kind in ("plain", "nup", "levels") and (cell["C"] % 2 == 1 or
                                                        L < 1 << (min(SM.source_limits()["pair_log2n"]) - 1))
        for c in range(cell["C"]):
            if alone and not filt[:, c].any():     # this channel's output depends on this channel alone: the twin's bytes
                assert y[:, c].tobytes() == want[:, c].tobytes(), c
    eng.close(); twin.close()


# ---- the sub-sample stage ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", SM.DELAY_SUB_CELLS, ids=[c["id"] for c in SM.DELAY_SUB_CELLS])
def test_sub_sample_stage_size_matrix(orc, bfir, cell):
    """An fp32 input-side cell at beta 9 is not expected to see the edge taps: there they weigh about 1e-7 of the centre tap,
    below TOL[4].  The beta 0 cells (a, c), the beta 2.0 cells (d) and the fp64 cells hold them, on the output side by the
    per-sample bound -- with one exception, fp64 arithmetic on FLOAT_LE frames at geometry b, where tap 2 h is 1e-4 of the
    float32 frame's unit roundoff (size_matrix.delay_sub_sees_last_tap; tests/test_delay_matrix.py shows the margins on the
    CPU)."""
    for chunk in cell["chunks"]:
        _stage_cell(bfir, orc, cell, "plain", chunk)


@pytest.mark.parametrize("cell", SM.DELAY_MID_CELLS, ids=[c["id"] for c in SM.DELAY_MID_CELLS])
def test_sub_sample_stage_changed_mid_stream_and_reset(orc, bfir, cell):
    """The model applies the delay and subdelay in force per block to the undelayed history; after reset() both streams
    start from silence.  Same bounds."""
    _stage_cell(bfir, orc, cell, "plain", None)


KIND_SUB_CELLS = [c for c in SM.DELAY_KIND_CELLS if not c.get("fade")]
KIND_FADE_CELLS = [c for c in SM.DELAY_KIND_CELLS if c.get("fade")]


@pytest.mark.parametrize("cell", KIND_SUB_CELLS, ids=[c["id"] for c in KIND_SUB_CELLS])
def test_sub_sample_stage_on_every_kind(orc, bfir, cell):
    """On the matrix kinds the model delays input i by d_i (input side) and output o by d_o (output side): the side's own
    stream."""
    _stage_cell(bfir, orc, cell, cell["kind"], None)


# ---- whole samples ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", KIND_FADE_CELLS, ids=[c["id"] for c in KIND_FADE_CELLS])
def test_whole_sample_delay_through_a_fade_on_every_kind(orc, bfir, cell):
    L, t0, K, nb, n_in = cell["L"], cell["t0"], cell["K"], cell["nb"], cell["n_in"]
    d0, d1 = cell["delays"], cell["delays_after"]
    eng, twin, (h2,), fade = _engines(bfir, orc, cell["kind"], 4, L, n_in, cell["n_out"], cell["fmt"], 12, n_sets=2)
    assert eng.delay_init(IN, cell["max_delay"]) == 0 and eng.set_delay(IN, d0) == 0
    x = orc.synth_audio(SM._rng(cell), nb * L, n_in, np.float32)
    xm = shift_model(x, L, [d0] * (t0 + 1) + [d1] * (nb - t0 - 1))
    ys = []
    for e, src in ((eng, x), (twin, xm)):
        out = [_run(e, src[:t0 * L], SM.uneven_calls(t0))]
        assert fade(e, h2, K) == 0
        out.append(_run(e, src[t0 * L:(t0 + 1) * L], [1]))                         # the first fade block
        assert e.fade_remaining() > 0
        if e is eng:
            assert e.set_delay(IN, d1) == 0                                        # from the second fade block on
        out.append(_run(e, src[(t0 + 1) * L:], [2, 4, nb - t0 - 7]))               # the head's fade ends with the first of these calls, a tail level's later
        assert e.fade_remaining() == 0
        ys.append(np.concatenate(out))
    assert ys[0].tobytes() == ys[1].tobytes() and np.any(ys[0])
    eng.close(); twin.close()


def _copy_frames(orc, cell):
    """Raw frames in the cell's format: integers over the whole range, or synth_audio."""
    fmt, n = cell["fmt"], sum(cell["calls"]) * cell["L"]
    rng = SM._rng(cell)
    if fmt in SM.INT_FMTS:
        bits = 8 * SM.FMT_BYTES[fmt]
        return np.ascontiguousarray(orc.encode_ints(rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), (n, cell["C"]), dtype=np.int64), fmt))
    return orc.synth_audio(rng, n, cell["C"], orc.fmt_dtype(fmt))


def _copy_engines(bfir, orc, cell, **kw):
    h = orc.synth_ir(np.random.default_rng(13), cell["C"], cell["B"] * cell["L"] - 3, orc.real_dtype(cell["s"]))
    engs = []
    for _ in range(2):
        e = bfir.Brutefir(cell["L"], cell["B"], cell["s"], cell["C"], **kw)
        assert e.set_coeff(h) == 0
        engs.append(e)
    return engs


FORMAT_CELLS = [c for c in SM.DELAY_COPY_CELLS if c["kind"] == "format"]
DITHER_CELLS = [c for c in SM.DELAY_COPY_CELLS if c["kind"] == "dither"]
ALIGN_CELLS = [c for c in SM.DELAY_COPY_CELLS if c["kind"] == "align"]


@pytest.mark.parametrize("cell", FORMAT_CELLS, ids=[c["id"] for c in FORMAT_CELLS])
def test_whole_sample_delay_in_every_sample_format(orc, bfir, cell):
    side, L, delays, fmt = cell["side"], cell["L"], cell["delays"], cell["fmt"]
    eng, twin = _copy_engines(bfir, orc, cell, in_format=fmt, out_format=fmt, apply_dither=False)
    assert eng.delay_init(side, cell["max_delay"]) == 0 and eng.set_delay(side, delays) == 0
    x = _copy_frames(orc, cell)
    y = _run(eng, x, cell["calls"])
    want = _run(twin, shift_model(x, L, delays), cell["calls"]) if side == IN else shift_model(_run(twin, x, cell["calls"]), L, delays)
    assert y.shape == want.shape and y.tobytes() == want.tobytes() and np.any(y)
    eng.close(); twin.close()


@pytest.mark.parametrize("cell", DITHER_CELLS, ids=[c["id"] for c in DITHER_CELLS])
def test_whole_sample_delay_behind_the_dither(orc, bfir, cell):
    """The output-side delay acts on the dithered bytes: the twin dithers alike (same table, same error feedback), and its
    bytes shifted are the delayed engine's."""
    L, delays, fmt = cell["L"], cell["delays"], cell["fmt"]
    kw = dict(in_format=SM.FLOAT_LE, out_format=fmt, sampling_rate=150)
    eng, twin = _copy_engines(bfir, orc, cell, apply_dither=True, **kw)
    assert eng.delay_init(OUT, cell["max_delay"]) == 0 and eng.set_delay(OUT, delays) == 0
    x = orc.synth_audio(SM._rng(cell), sum(cell["calls"]) * L, cell["C"], np.float32)
    y, u = _run(eng, x, cell["calls"]), _run(twin, x, cell["calls"])
    assert y.tobytes() == shift_model(u, L, delays).tobytes() and np.any(y)
    plain = bfir.Brutefir(L, cell["B"], 4, cell["C"], apply_dither=False, **kw)    # ... and the dither was at work
    assert plain.set_coeff(orc.synth_ir(np.random.default_rng(13), cell["C"], cell["B"] * L - 3, np.float32)) == 0
    if SM.FMT_BYTES[fmt] < 4:                                                      # (a +-1 LSB dither vanishes in fp32 next to 2^30)
        assert _run(plain, x, cell["calls"]).tobytes() != u.tobytes()
    eng.close(); twin.close(); plain.close()


def _run_offset(eng, x, out_dtype, calls, off_in, off_out):
    """run_device with the caller's buffers off_in / off_out bytes past a 16-byte boundary; the output bytes, and the 32 bytes
    on either side of them, which nothing may write."""
    import torch
    L = eng.L
    xb = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
    n = x.shape[0]
    fin, fout = xb.size // n, eng.C * np.dtype(out_dtype).itemsize
    d_in = torch.zeros(xb.size + 64, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(n * fout + 64, dtype=torch.uint8, device="cuda")
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    d_in[32 + off_in:32 + off_in + xb.size] = torch.from_numpy(xb).cuda()
    torch.cuda.synchronize()
    pos = 0
    for k in calls:
        eng.run_device(d_in.data_ptr() + 32 + off_in + pos * L * fin, d_out.data_ptr() + 32 + off_out + pos * L * fout, k)
        pos += k
    assert eng.sync() == 0
    raw = d_out.cpu().numpy()
    return raw[32 + off_out:32 + off_out + n * fout].tobytes(), raw[:32 + off_out].tobytes() + raw[32 + off_out + n * fout:].tobytes()


@pytest.mark.parametrize("cell", ALIGN_CELLS, ids=[c["id"] for c in ALIGN_CELLS])
def test_whole_sample_delay_on_an_unaligned_pointer(orc, bfir, cell):
    """The caller's pointer on the delayed side one sample, or one byte, past a 16-byte boundary: only the delay kernel
    touches it (the VEC = false instances on the output side, byte units where the sample is not aligned), and the bytes are
    those of the same run on aligned pointers."""
    side, fmt, off = cell["side"], cell["fmt"], cell["offset"]
    engs = _copy_engines(bfir, orc, cell, in_format=fmt, out_format=fmt, apply_dither=False)
    x = _copy_frames(orc, cell)
    dt = np.dtype((np.uint8, 3)) if SM.FMT_BYTES[fmt] == 3 else orc.fmt_dtype(fmt)
    outs = []
    for e, o in zip(engs, (0, off)):
        assert e.delay_init(side, cell["max_delay"]) == 0 and e.set_delay(side, cell["delays"]) == 0
        y, guard = _run_offset(e, x, dt, cell["calls"], o if side == IN else 0, o if side == OUT else 0)
        assert not any(guard)
        outs.append(y)
        e.close()
    assert outs[0] == outs[1] and any(outs[0])
