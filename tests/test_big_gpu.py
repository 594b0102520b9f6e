"""Long-partition ("big") engines on the GPU: bfir_engine_create_big, partitions of 32768 ... 1048576 samples (fp64 from
16384) through the two-pass transforms of csrc/bigconv.hip.

Every run cell follows the size matrix's recipe (tests/size_matrix.py): flat impulse responses with a ragged last
partition, taps = (B - 1) L + L / 2 + 17, uniform noise with the odd channels at 1/8, nb = B + 3 blocks, the per-block
error of SM.block_errors against the float64 reference SM.reference at the project's tolerance (SM.tolerance: 1e-5 for
fp32 arithmetic or float32 frames, conftest.TOL[8] for fp64), and up to L = 65536 against the oracle engine of the same
shape as well.  The data and the reference of a cell are computed once and shared by the tests that use it."""
import ctypes as C

import numpy as np
import pytest

import size_matrix as SM
from conftest import TOL
from test_dither_gpu import _OracleDither
from test_fade import fade_expected

pytestmark = pytest.mark.gpu

F32, F64, S16, S24 = SM.FLOAT_LE, SM.FLOAT64_LE, 2, 4


def _cell(id_, s, L, B, Cn, fin, fout, nb=None, cuts=None, chunk=0, oracle=True):
    return {"id": id_, "s": s, "L": L, "B": B, "C": Cn, "in_fmt": fin, "out_fmt": fout, "nb": nb or B + 3,
            "taps": (B - 1) * L + L // 2 + 17, "cuts": cuts, "chunk": chunk, "oracle": oracle}


CELLS = [
    # unequal split, odd channel count; a one-block call, history across calls, launches of two blocks
    _cell("f32-32768-3ch", 4, 32768, 2, 3, F32, F32, cuts=(0, 1, 3, 5), chunk=2),
    _cell("f32-65536-2ch", 4, 65536, 2, 2, F32, F32),
    _cell("f32-1048576-1ch", 4, 1048576, 1, 1, F32, F32, nb=3, oracle=False),        # the largest plan
    _cell("f64-16384-2ch", 8, 16384, 2, 2, F64, F64),                                # the smallest fp64 size
    _cell("f64-32768-3ch-mixed", 8, 32768, 2, 3, F32, F64),                          # FLOAT_LE in, FLOAT64_LE out
    _cell("f64-1048576-1ch", 8, 1048576, 1, 1, F64, F64, nb=3, oracle=False),        # the largest fp64 plan
]
BY_ID = {c["id"]: c for c in CELLS}
_DATA = {}


def _data(orc, cell):
    """(h, x, ref) of a cell: taps in working precision, frames in the input format, the float64 reference; made once."""
    if cell["id"] not in _DATA:
        rng = SM._rng(cell)
        h = [v.astype(orc.real_dtype(cell["s"])) for v in SM.flat_ir(rng, cell["C"], cell["taps"])]
        x = SM._noise(orc, rng, cell)
        ref = SM.reference(orc, x, h)
        for a in (x, ref):
            a.setflags(write=False)
        _DATA[cell["id"]] = (h, x, ref)
    return _DATA[cell["id"]]


def _make(bfir, cell, h, chunk=None, **kw):
    eng = bfir.BrutefirBig(cell["L"], cell["B"], cell["s"], cell["C"], cell["in_fmt"], cell["out_fmt"], **kw)
    chunk = cell["chunk"] if chunk is None else chunk
    if chunk:
        eng.set_chunk(chunk)
    assert eng.set_coeff(h) == 0
    return eng


def _run(eng, x, L, cuts=None):
    nb = x.shape[0] // L
    cuts = cuts or (0, nb)
    ys = []
    for a, e in zip(cuts[:-1], cuts[1:]):
        rc, y = eng.run(x[a * L:e * L])
        assert rc == 0
        ys.append(y)
    return np.concatenate(ys)


@pytest.fixture()
def log(bfir):
    from foo_dsp_bfir_amd import _lib
    lines = []
    cb = _lib.LOG_FN(lambda msg: lines.append(msg.decode(errors="replace")))
    lib = bfir.load()
    lib.bfir_set_log_callback(cb)
    yield lines
    lib.bfir_set_log_callback(_lib.LOG_FN())


@pytest.mark.parametrize("cell", CELLS, ids=[c["id"] for c in CELLS])
def test_big_engine_against_the_float64_reference(orc, bfir, log, cell):
    s, L, B, Cn = cell["s"], cell["L"], cell["B"], cell["C"]
    h, x, ref = _data(orc, cell)
    tol = SM.tolerance(cell, TOL)
    del log[:]
    eng = _make(bfir, cell, h)
    made = [ln for ln in log if ln.startswith("bfir engine: ")]
    assert len(made) == 1 and made[0].startswith("bfir engine: big, 1 x %d channels, partition %d = " % (Cn, L)), log
    assert made[0].endswith("layout=%s" % ("pairs" if s == 4 else "grouped")), made[0]
    y = _run(eng, x, L, cell["cuts"])
    eng.close()
    err = SM.block_errors(y, ref, L)
    print("big %s: worst per-block error vs float64 %.3g (tol %.3g)" % (cell["id"], err.max(), tol))
    assert err.max() <= tol, np.unravel_index(np.argmax(err), err.shape)
    if cell["oracle"]:
        o = orc.Engine(L, B, s, Cn, cell["in_fmt"], cell["out_fmt"])
        assert o.set_coeff(h) == 0
        rc, y_orc = o.run(x)
        assert rc == 0
        err = SM.block_errors(y, y_orc, L)
        print("big %s: worst per-block error vs the oracle engine %.3g" % (cell["id"], err.max()))
        assert err.max() <= tol


@pytest.mark.parametrize("cid", ["f32-32768-3ch", "f64-16384-2ch"])
def test_partition_spectra_in_natural_grouped_order(orc, bfir, cid):
    """read_coeff undoes the transposed bin order: every partition of every channel, the ragged last one included."""
    cell = BY_ID[cid]
    s, L, B, Cn = cell["s"], cell["L"], cell["B"], cell["C"]
    h, _, _ = _data(orc, cell)
    eng = _make(bfir, cell, h)
    worst = 0.0
    for c in range(Cn):
        for b in range(B):
            want = SM.grouped_spectrum(h[c][b * L:(b + 1) * L], L, 1.0)
            got = eng.coeff_block(c, b).astype(np.float64)
            e = np.abs(got - want).max() / np.abs(want).max()
            worst = max(worst, e)
            assert e <= TOL[s], (c, b, e)
    print("big %s: worst spectrum error %.3g" % (cid, worst))
    eng.close()


def test_output_bytes_do_not_depend_on_the_chunking(orc, bfir):
    cell = BY_ID["f32-32768-3ch"]
    h, x, _ = _data(orc, cell)
    outs = []
    for chunk in (1, 3, 0):
        eng = _make(bfir, cell, h, chunk=chunk)
        outs.append(_run(eng, x, cell["L"]).tobytes())
        eng.close()
    assert outs[0] == outs[1] == outs[2]


def test_reset_gives_the_same_bytes_again(orc, bfir):
    """The same input after reset(): a whole number of block pairs, so the time history the reference keeps across a reset
    (input_timecbuf) is the zero block both times."""
    cell = BY_ID["f32-32768-3ch"]
    h, x, _ = _data(orc, cell)
    L = cell["L"]
    z = np.zeros((L, cell["C"]), x.dtype)
    xs = np.concatenate([x[:3 * L], z])
    eng = _make(bfir, cell, h)
    first = _run(eng, xs, L)
    eng.reset()
    again = _run(eng, xs, L)
    eng.close()
    assert first.tobytes() == again.tobytes()


def test_fade_through_the_general_back_end(orc, bfir):
    s, L, B, Cn, K = 4, 32768, 2, 2, 2
    cell = _cell("fade-32768", s, L, B, Cn, F32, F32, nb=B + K + 2)
    nb, t0 = cell["nb"], B
    rng = SM._rng(cell)
    h_old = [v.astype(np.float32) for v in SM.flat_ir(rng, Cn, cell["taps"])]
    h_new = [(0.125 * v).astype(np.float32) for v in h_old]          # gain 1 -> 0.125
    x = SM._noise(orc, rng, cell)
    eng = _make(bfir, cell, h_old)
    rc, y0 = eng.run(x[:t0 * L])
    assert rc == 0 and eng.fade_remaining() == 0
    assert eng.set_coeff_fade(h_new, K) == 0 and eng.fade_remaining() == K
    ys = [y0]
    for t in range(t0, nb):                                          # block by block: the count goes down to 0
        rc, y = eng.run(x[t * L:(t + 1) * L])
        assert rc == 0 and eng.fade_remaining() == max(0, K - (t - t0 + 1))
        ys.append(y)
    eng.close()
    y = np.concatenate(ys)
    want, _, _ = fade_expected(orc, L, B, s, Cn, h_old, h_new, x, t0, K, F32, F32)
    err = SM.block_errors(y, want, L)
    print("big fade: worst per-block error %.3g" % err.max())
    assert err.max() <= SM.tolerance(cell, TOL)


def test_delays_shift_the_frames(orc, bfir):
    """Whole-sample delays sit on the frame streams outside the transforms: with an input delay of (0, 5) frames and an
    output delay of (3, 0) the engine gives, byte for byte, the output of the undelayed engine on the input whose channel 1
    is shifted by 5 frames, with channel 0 of that output shifted by 3."""
    cell = _cell("delay-32768", 4, 32768, 2, 2, F32, F32)
    L, nb = cell["L"], cell["nb"]
    rng = SM._rng(cell)
    h = [v.astype(np.float32) for v in SM.flat_ir(rng, 2, cell["taps"])]
    x = SM._noise(orc, rng, cell)
    xd = x.copy()
    xd[5:, 1] = x[:-5, 1]
    xd[:5, 1] = 0
    plain = _make(bfir, cell, h)
    y0 = _run(plain, xd, L)
    plain.close()
    eng = _make(bfir, cell, h)
    assert eng.delay_init(bfir.DELAY_INPUT, 8) == 0 and eng.delay_init(bfir.DELAY_OUTPUT, 8) == 0
    assert eng.set_delay(bfir.DELAY_INPUT, [0, 5]) == 0 and eng.set_delay(bfir.DELAY_OUTPUT, [3, 0]) == 0
    assert eng.get_delay(bfir.DELAY_INPUT)[0] == [0, 5] and eng.delay_latency(bfir.DELAY_OUTPUT) == 0
    y = _run(eng, x, L, (0, 1, nb))
    eng.close()
    assert np.all(y[:3, 0] == 0)
    assert y[3:, 0].tobytes() == y0[:nb * L - 3, 0].tobytes()
    assert y[:, 1].tobytes() == y0[:, 1].tobytes()


REFUSED = [(4, 16384, "ERR_UNSUPPORTED"), (8, 8192, "ERR_UNSUPPORTED"), (4, 2097152, "ERR_UNSUPPORTED"),
           (8, 2097152, "ERR_UNSUPPORTED"), (4, 40000, "ERR_ARG")]


@pytest.mark.parametrize("s,L,err", REFUSED)
def test_big_engine_refuses_size(bfir, s, L, err):
    lib = bfir.load()
    code = C.c_int(0)
    fmt = F32 if s == 4 else F64
    assert not lib.bfir_engine_create_big(L, 2, s, 2, fmt, fmt, 44100, 0, 0, C.byref(code))
    assert code.value == getattr(bfir, err)
    # nothing left behind: the device still makes and runs a big engine
    dt = np.float32 if s == 4 else np.float64
    Lb = 32768 if s == 4 else 16384
    eng = bfir.BrutefirBig(Lb, 1, s, 2)
    assert eng.set_coeff([np.ones(10, dt) / 10] * 2) == 0
    rc, y = eng.run(np.ones((Lb, 2), dt))
    assert rc == 0 and np.all(np.isfinite(y)) and abs(float(y[-1, 0]) - 1.0) <= 1e-5
    eng.close()


def test_foreign_kinds_are_refused_on_a_big_engine(bfir):
    L = 32768
    eng = bfir.BrutefirBig(L, 2, 4, 2)
    lib = bfir.load()
    taps = np.ones(8, np.float32)
    ptrs = (C.c_void_p * 4)(*[taps.ctypes.data] * 4)
    lens = (C.c_int * 4)(8, 8, 8, 8)
    assert lib.bfir_engine_set_coeff_nup(eng.handle, ptrs, 2, 8, 1.0) == bfir.ERR_UNSUPPORTED
    assert lib.bfir_engine_set_coeff_levels(eng.handle, ptrs, 2, 8, 1.0) == bfir.ERR_UNSUPPORTED
    assert lib.bfir_engine_set_coeff_matrix(eng.handle, ptrs, 8, 1, 1.0) == bfir.ERR_UNSUPPORTED
    assert lib.bfir_engine_set_coeff_matrix_levels(eng.handle, ptrs, lens, 1.0) == bfir.ERR_UNSUPPORTED
    assert not eng.is_initialized()
    eng.close()


def test_overflow_counter_and_nan_guard(orc, bfir):
    L = 32768
    d = np.zeros(4, np.float32); d[0] = 1.0
    eng = bfir.BrutefirBig(L, 1, 4, 1)
    assert eng.set_coeff([d]) == 0
    x = np.zeros((2 * L, 1), np.float32)
    x[7, 0] = 2.0
    rc, y = eng.run(x[:L])
    assert rc == 0 and abs(float(y[7, 0]) - 2.0) <= 2e-5
    of = eng.overflow(0)
    assert of.n_overflows == 1 and abs(of.largest - 2.0) <= 2e-5
    eng.close()
    # a NaN in sample 0 of block 1: the reference's -1, as on a uniform engine (tests/test_engine_gpu.py)
    x = np.zeros((3 * L, 1), np.float32)
    x[L, 0] = np.nan
    ref = orc.Engine(L, 1, 4, 1); ref.set_coeff([d])
    eng = bfir.BrutefirBig(L, 1, 4, 1); eng.set_coeff([d])
    assert ref.run(x)[0] == -1
    assert eng.run(x)[0] == -1
    eng.close()


def test_s24_in_s16_out_with_dither_bit_exact(orc, bfir):
    """Integer frames and HP-TPDF dither come through the staging kernels unchanged.  Held to what tests/test_dither_gpu.py
    holds uniform engines to: byte for byte the oracle's dither applied to the float output of the SAME engine (the output
    scale is a power of two, so the samples entering the quantiser are identical), the overflow counters included."""
    s, L, B, Cn, srate = 4, 32768, 2, 2, 1000
    cell = _cell("dither-32768", s, L, B, Cn, S24, S16)
    nb = cell["nb"]
    rng = SM._rng(cell)
    h = [v.astype(np.float32) for v in SM.flat_ir(rng, Cn, cell["taps"])]
    ints = np.round(rng.uniform(-1.0, 1.0, (nb * L, Cn)) * SM.amplitudes(nb, L, Cn, False) * (2 ** 23 - 1)).astype(np.int64)
    x = np.ascontiguousarray(orc.encode_ints(ints, S24))
    ef = bfir.BrutefirBig(L, B, s, Cn, S24, F32, sampling_rate=srate)
    assert ef.set_coeff(h, scale=3.0) == 0                              # loud enough to clip now and then
    rc, yf = ef.run(x); assert rc == 0
    ef.close()
    ed = bfir.BrutefirBig(L, B, s, Cn, S24, S16, sampling_rate=srate, apply_dither=True)
    assert ed.set_coeff(h, scale=3.0) == 0
    yd = np.concatenate([ed.run(x[a * L:b * L])[1] for a, b in ((0, 1), (1, 3), (3, nb))])
    od = _OracleDither(orc, S16, s, L, Cn, srate)
    assert np.array_equal(yd, od.apply(yf))
    for c in range(Cn):
        o = ed.overflow(c)
        assert (o.n_overflows, o.intlargest, o.largest) == (od.of[c].n_overflows, od.of[c].intlargest, od.of[c].largest)
    ed.close()
    # ... and the float output itself against the oracle engine on the same integer frames
    o = orc.Engine(L, B, s, Cn, S24, F32)
    assert o.set_coeff(h, scale=3.0) == 0
    rc, y_orc = o.run(x)
    assert rc == 0
    err = SM.block_errors(yf, y_orc, L)
    print("big S24 -> float: worst per-block error vs the oracle engine %.3g" % err.max())
    assert err.max() <= 1e-5
