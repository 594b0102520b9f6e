"""Every transform size through every kernel family (tests/size_matrix.py), the stage transforms at every size, the
FFT plans at every order and the td convolver up to its largest block, each against a float64 / long-double reference
computed here from the same inputs -- not only against the oracle, which shares the reference's algorithm."""
import ctypes as C
import re

import numpy as np
import pytest
import scipy.fft

import size_matrix as SM
from conftest import TOL, env_override

pytestmark = pytest.mark.gpu

WORST = {}          # (family, realsize) -> worst per-block error seen against the float64 reference


@pytest.fixture(scope="module")
def creation_log(bfir):
    """Lines the library logs, captured through bfir_set_log_callback (the callback object is kept alive here)."""
    from foo_dsp_bfir_amd import _lib
    lines = []
    cb = _lib.LOG_FN(lambda msg: lines.append(msg.decode(errors="replace")))
    lib = bfir.load()
    lib.bfir_set_log_callback(cb)
    yield lines
    lib.bfir_set_log_callback(_lib.LOG_FN())
    for k in sorted(WORST):
        print("size matrix: worst per-block error %-16s realsize %d: %.3g" % (k[0], k[1], WORST[k]))


def _frames(orc, fmt, x):
    return x.astype(orc.fmt_dtype(fmt))


@pytest.mark.parametrize("cell", SM.CELLS, ids=[c["id"] for c in SM.CELLS])
def test_engine_size_matrix(orc, bfir, creation_log, cell):
    s, L, Cn, fin, fout = cell["s"], cell["L"], cell["C"], cell["in_fmt"], cell["out_fmt"]
    B, nb = SM.B, 2 * SM.B + 5
    taps = B * L - SM.RAGGED
    rng = np.random.default_rng(L * 16 + Cn + 3 * s + fin + fout)
    h64 = SM.flat_ir(rng, Cn, taps)
    h = [v.astype(orc.real_dtype(s)) for v in h64]
    g = SM.amplitudes(nb, L, Cn, cell["path"] == "time-pair")
    x = _frames(orc, fin, rng.uniform(-1.0, 1.0, (nb * L, Cn)) * g)
    tol = 1e-5 if (s == 4 or fout == SM.FLOAT_LE) else TOL[s]

    with env_override(**cell["env"]):
        del creation_log[:]
        eng = bfir.Brutefir(L, B, s, Cn, fin, fout)
        made = [ln for ln in creation_log if ln.startswith("bfir engine: ")]
        assert len(made) == 1, creation_log
        m = re.search(r"path=(\S+) layout=(\S+) run=(\S+)$", made[0])
        assert m and m.groups() == (cell["path"], cell["layout"], cell["run"]), made[0]
        eng.set_chunk(3)
        assert eng.set_coeff(h) == 0
        # partition spectra, every partition the ragged one included, in the grouped layout read_coeff hands out
        for c in range(Cn):
            for b in range(B):
                want = SM.grouped_spectrum(h[c][b * L:(b + 1) * L], L, 1.0)
                got = eng.coeff_block(c, b).astype(np.float64)
                assert np.abs(got - want).max() <= TOL[s] * np.abs(want).max(), (c, b)
        # an odd chunk split over a 5-block call, one block alone (the latency path), then the rest
        ys = []
        for a, e in ((0, 5), (5, 6), (6, nb)):
            rc, y = eng.run(x[a * L:e * L])
            assert rc == 0
            ys.append(y)
        eng.close()
    y = np.concatenate(ys)

    x64 = x.astype(np.float64)
    ref = np.stack([SM.reference_conv(orc, x64[:, c], h[c].astype(np.float64)) for c in range(Cn)], axis=1)
    err = SM.block_errors(y, ref, L)
    key = (cell["family"], s)
    WORST[key] = max(WORST.get(key, 0.0), float(err.max()))
    assert err.max() <= tol, np.unravel_index(np.argmax(err), err.shape)

    o = orc.Engine(L, B, s, Cn, fin, fout)
    assert o.set_coeff(h) == 0
    rc, y_orc = o.run(x)
    assert rc == 0
    assert SM.block_errors(y, y_orc, L).max() <= tol


@pytest.mark.parametrize("s,L,err", SM.REFUSALS)
def test_engine_refuses_size(bfir, s, L, err):
    lib = bfir.load()
    code = C.c_int(0)
    h = lib.bfir_engine_create(L, 2, s, 2, 8, 8, 44100, 0, 0, C.byref(code))
    assert not h and code.value == getattr(bfir, err)
    code = C.c_int(0)
    assert not lib.bfir_convolver_create(L, s, 0, C.byref(code)) and code.value == getattr(bfir, err)
    # nothing left behind: the device still makes and runs an engine of a supported size
    dt = np.float32 if s == 4 else np.float64
    eng = bfir.Brutefir(1024, 2, s, 2)
    assert eng.set_coeff([np.ones(10, dt)] * 2) == 0
    rc, y = eng.run(np.ones((2048, 2), dt))
    assert rc == 0 and np.all(np.isfinite(y))
    eng.close()


# ---- stage level ---------------------------------------------------------------------------------------------------
STAGE = [(4, 1 << lg) for lg in range(4, 15)] + [(8, 1 << lg) for lg in range(4, 14)]


@pytest.mark.parametrize("s,L", STAGE)
def test_stage_transforms_every_size(orc, bfir, s, L):
    dt = orc.real_dtype(s)
    rng = np.random.default_rng(L + s)
    cv = bfir.FftwConvolver(L, s)
    x = rng.standard_normal(2 * L).astype(dt)
    hc = cv.new_cbuf(); cv.convolver_time2freq(x, hc)
    want = SM.halfcomplex(np.fft.rfft(x.astype(np.float64)), 2 * L)
    assert np.abs(hc - want).max() <= TOL[s] * np.abs(want).max()
    # the inverse on its own input, not on the forward's output: an error shared by both directions shows
    spec = rng.standard_normal(2 * L).astype(dt)
    back = cv.new_cbuf(); cv.convolver_freq2time(spec, back)
    want = SM.hc2r(spec)
    assert np.abs(back - want).max() <= TOL[s] * np.abs(want).max()
    # mixnscale and the convolve family: bit-exact with the oracle's restatement of the reference
    g = cv.new_cbuf(); cv.convolver_mixnscale([spec], g, [0.37], 1, bfir.MIXMODE_INPUT)
    assert np.array_equal(g, orc.mixnscale(spec, 0.37, orc.MIXMODE_INPUT))
    o = cv.new_cbuf(); cv.convolver_mixnscale([g], o, [1.7], 1, bfir.MIXMODE_OUTPUT)
    assert np.array_equal(o, orc.mixnscale(g, 1.7, orc.MIXMODE_OUTPUT))
    b, c, d0 = (rng.standard_normal(2 * L).astype(dt) for _ in range(3))
    d = cv.new_cbuf(); cv.convolver_convolve(b, c, d)
    assert np.array_equal(d, orc.convolve(b, c))
    da = d0.copy(); cv.convolver_convolve_add(b, c, da)
    assert np.array_equal(da, orc.convolve_add(b, c, d0))
    bi = b.copy(); cv.convolver_convolve_inplace(bi, c)
    assert np.array_equal(bi, orc.convolve_inplace(b, c))
    cv.close()


# ---- FFT plans -------------------------------------------------------------------------------------------------------
def _execute_both_ways(plan, x):
    """Out of place, then in place (in == out) on a copy: the two results must be the same bits."""
    out = plan.execute(x)
    buf = np.ascontiguousarray(x, dtype=plan.dtype).copy()
    assert plan._lib.bfir_fft_plan_execute(plan._h, buf.ctypes.data, buf.ctypes.data) == 0
    assert np.array_equal(buf, out)
    return out


@pytest.mark.parametrize("s", [4, 8])
@pytest.mark.parametrize("order", range(1, 26))
def test_fft_plan_every_order(bfir, s, order):
    n = 1 << order
    dt = np.float32 if s == 4 else np.float64
    rng = np.random.default_rng(order * 2 + s)
    x = rng.standard_normal(n).astype(dt)
    fwd = bfir.FftPlan(order, False, s)
    hc = _execute_both_ways(fwd, x)
    want = SM.halfcomplex(scipy.fft.rfft(x.astype(np.float64)), n)
    assert np.abs(hc - want).max() <= TOL[s] * np.abs(want).max()
    fwd.close()
    del hc, want
    inv = bfir.FftPlan(order, True, s)
    spec = rng.standard_normal(n).astype(dt)
    y = _execute_both_ways(inv, spec)
    want = SM.hc2r(spec)
    assert np.abs(y - want).max() <= TOL[s] * np.abs(want).max()
    inv.close()


# ---- td convolver ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,lg", [(4, 18), (4, 21), (4, 24), (8, 18), (8, 21)])
def test_td_convolver_large_blocks(bfir, s, lg):
    """convolver_td_convolve of 2 * blocklen reals: the circular convolution with [0 .. 0 | taps | 0 ..]."""
    dt = np.float32 if s == 4 else np.float64
    bl = 1 << lg
    n_taps = bl - 3
    rng = np.random.default_rng(lg + s)
    h = rng.standard_normal(n_taps).astype(dt)
    cv = bfir.FftwConvolver(256, s)
    tdc = cv.convolver_td_new(h, n_taps)
    assert tdc.blocklen == bl
    x = rng.standard_normal(2 * bl).astype(dt)
    y = x.copy()
    cv.convolver_td_convolve(tdc, y)
    tdc.close()
    hp = np.zeros(2 * bl)
    hp[bl:bl + n_taps] = h
    want = np.fft.irfft(np.fft.rfft(x.astype(np.float64)) * np.fft.rfft(hp), 2 * bl)
    del hp
    assert np.abs(y - want).max() <= TOL[s] * np.abs(want).max()
