"""Matrix engines on the GPU: n inputs -> m outputs, one filter per (output, input) pair, y_o = sum_i h_{o,i} * x_i.

References: per output, one oracle engine over all inputs with that output's row of filters (NULL = zeros), its channels
summed in float64 (test_matrix.matrix_reference); orc.direct_conv where the sizes allow."""
import ctypes as C

import numpy as np
import pytest

from conftest import TOL, rel_err
from test_matrix import matrix_reference

pytestmark = pytest.mark.gpu

F32, F64 = 8, 10


@pytest.fixture(scope="module")
def creation_log(bfir):
    from foo_dsp_bfir_amd import _lib
    lines = []
    cb = _lib.LOG_FN(lambda msg: lines.append(msg.decode(errors="replace")))
    lib = bfir.load()
    lib.bfir_set_log_callback(cb)
    yield lines
    lib.bfir_set_log_callback(_lib.LOG_FN())


def _rows(orc, rng, n_in, n_out, taps, s, null=()):
    dt = np.float64 if s == 8 else np.float32
    rows = [[orc.synth_ir(rng, 1, taps, dt)[0] for _ in range(n_in)] for _ in range(n_out)]
    for o, i in null:
        rows[o][i] = None
    return rows


class RefMatrix:
    """The oracle side of a matrix engine across calls: one orc.Engine per output."""

    def __init__(self, orc, L, B, s, n_in, n_out):
        self.fmt = F64 if s == 8 else F32
        self.dt = np.float64 if s == 8 else np.float32
        self.engines = [orc.Engine(L, B, s, n_in, self.fmt, self.fmt) for _ in range(n_out)]

    def set_coeff(self, rows):
        taps = max(h.size for r in rows for h in r if h is not None)
        for e, row in zip(self.engines, rows):
            assert e.set_coeff([np.zeros(taps, self.dt) if h is None else h for h in row]) == 0

    def run(self, x):
        return np.stack([e.run(np.ascontiguousarray(x, dtype=self.dt))[1].astype(np.float64).sum(axis=1)
                         for e in self.engines], axis=1)

    def reset(self):
        for e in self.engines:
            e.reset()


def _path(log):
    made = [ln for ln in log if ln.startswith("bfir engine: ")]
    assert len(made) == 1, log
    return dict(kv.split("=") for kv in made[0].split(". ")[-1].split())


# (L, B, realsize, n_in, n_out, frames, path, layout, NULL pairs)
SHAPES = [
    (4096, 32, 4, 2, 2, F32, "pair", "pairs", ()),                       # crossfeed
    (512, 4, 4, 1, 8, F32, "direct", "pairs", ((3, 0),)),
    (512, 4, 4, 8, 1, F32, "direct", "pairs", ((0, 5),)),
    (256, 5, 4, 3, 5, F32, "direct", "pairs", ((1, 2), (4, 0))),         # odd both sides, ragged tail
    (1024, 16, 4, 8, 8, F32, "pair", "pairs", ()),                       # dense
    (1024, 64, 8, 2, 2, F64, "direct", "pairs", ()),                     # the plug-in's arithmetic
    (1024, 64, 8, 2, 2, F32, "direct", "pairs", ()),
    (16, 3, 4, 2, 3, F32, "direct", "grouped", ((2, 1),)),
    (16, 3, 8, 3, 2, F64, "direct", "grouped", ()),
    (16384, 2, 4, 2, 2, F32, "direct", "pairs", ()),
    (8192, 2, 8, 2, 3, F64, "direct", "grouped", ()),
    (1024, 4, 4, 3, 3, F32, "direct", "pairs", ()),   # odd counts: no time pairs
]


@pytest.mark.parametrize("L,B,s,n_in,n_out,fmt,path,layout,null", SHAPES)
def test_matrix_parity(orc, bfir, creation_log, L, B, s, n_in, n_out, fmt, path, layout, null):
    rng = np.random.default_rng(L * 131 + B * 7 + n_in * 3 + n_out + s + fmt)
    nb = 2 * B + 3
    taps = B * L - (L // 3 + 1)                                          # ragged tail
    rows = _rows(orc, rng, n_in, n_out, taps, s, null)
    x = orc.synth_audio(rng, nb * L, n_in, np.float32 if fmt == F32 else np.float64)
    del creation_log[:]
    eng = bfir.BrutefirMatrix(L, B, s, n_in, n_out, fmt, fmt)
    got = _path(creation_log)
    assert got["path"] == path and got["layout"] == layout, got
    assert eng.set_coeff(rows) == 0 and eng.is_initialized()
    rc, y = eng.run(x)
    assert rc == 0 and y.shape == (nb * L, n_out)
    ref = matrix_reference(orc, L, B, s, rows, x)
    tol = TOL[s] if not (s == 8 and fmt == F32) else 1e-6
    assert rel_err(y, ref) <= tol
    if L * B <= 4096:                                                    # the independent reference where it is cheap
        want = np.zeros_like(ref)
        for o, row in enumerate(rows):
            for i, h in enumerate(row):
                if h is not None:
                    want[:, o] += orc.direct_conv(x[:, i].astype(np.float64), h)
        assert rel_err(y, want) <= 10 * tol
    eng.close()


# diagonal shapes on which both engines log the same path: (L, B, realsize, C, frames, path)
DIAG = [(1024, 4, 4, 2, F32, "pair"), (1024, 4, 4, 4, F32, "pair"), (16, 3, 4, 1, F32, "direct"),
        (256, 3, 4, 1, F32, "direct"), (1024, 8, 8, 2, F64, "direct"), (1024, 8, 8, 2, F32, "direct")]


@pytest.mark.parametrize("L,B,s,Cn,fmt,path", DIAG)
def test_diagonal_matrix_equals_diagonal_engine_bitwise(orc, bfir, creation_log, L, B, s, Cn, fmt, path):
    rng = np.random.default_rng(L + Cn + s)
    nb = 2 * B + 3
    dt = np.float64 if s == 8 else np.float32
    h = [(orc.synth_ir(rng, 1, B * L - 5, dt)[0] * 40).astype(dt) for _ in range(Cn)]   # loud enough to clip
    x = orc.synth_audio(rng, nb * L, Cn, np.float32 if fmt == F32 else np.float64)
    del creation_log[:]
    d = bfir.Brutefir(L, B, s, Cn, fmt, fmt)
    pd = _path(creation_log)
    del creation_log[:]
    m = bfir.BrutefirMatrix(L, B, s, Cn, Cn, fmt, fmt)
    pm = _path(creation_log)
    assert pd["path"] == pm["path"] == path and pd["layout"] == pm["layout"], (pd, pm)
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


def test_two_by_two_equals_the_four_channel_workaround(orc, bfir):
    L, B, nb = 1024, 8, 19
    rng = np.random.default_rng(22)
    rows = _rows(orc, rng, 2, 2, B * L - 100, 4)
    x = orc.synth_audio(rng, nb * L, 2, np.float32)
    m = bfir.BrutefirMatrix(L, B, 4, 2, 2)
    assert m.set_coeff(rows) == 0
    rc, y = m.run(x)
    w = bfir.Brutefir(L, B, 4, 4)
    assert w.set_coeff([rows[0][0], rows[0][1], rows[1][0], rows[1][1]]) == 0
    rcw, yw = w.run(np.ascontiguousarray(np.concatenate([x, x], axis=1)))
    assert rc == rcw == 0
    want = np.stack([yw[:, 0].astype(np.float64) + yw[:, 1], yw[:, 2].astype(np.float64) + yw[:, 3]], axis=1)
    assert rel_err(y, want) <= TOL[4]
    m.close(); w.close()


@pytest.mark.parametrize("L,s", [(1024, 4), (256, 4), (1024, 8)])
def test_null_column_skips_a_nan_input(orc, bfir, L, s):
    """NULL filters are skipped, not multiplied by zero: a NaN in an input no filter reads reaches no output."""
    B, nb = 3, 9
    rng = np.random.default_rng(3 + L + s)
    fmt = F64 if s == 8 else F32
    rows = _rows(orc, rng, 2, 2, B * L - 7, s, null=((0, 1), (1, 1)))
    x = orc.synth_audio(rng, nb * L, 2, np.float32 if s == 4 else np.float64)
    clean = x.copy(); clean[:, 1] = 0
    x[3 * L + 5, 1] = np.nan
    m = bfir.BrutefirMatrix(L, B, s, 2, 2, fmt, fmt)
    assert m.set_coeff(rows) == 0
    rc, y = m.run(x)
    assert rc == 0 and np.all(np.isfinite(y))
    assert rel_err(y, matrix_reference(orc, L, B, s, rows, clean)) <= TOL[s]
    rows[0][1] = orc.synth_ir(rng, 1, B * L - 7, np.float64 if s == 8 else np.float32)[0]
    m2 = bfir.BrutefirMatrix(L, B, s, 2, 2, fmt, fmt)
    assert m2.set_coeff(rows) == 0
    assert m2.run(x)[0] == bfir.ERR_NONFINITE
    m.close(); m2.close()


@pytest.mark.parametrize("L,B,s,n_in,n_out", [(512, 6, 4, 2, 3), (512, 6, 4, 2, 2), (256, 5, 4, 3, 2), (1024, 6, 8, 2, 3)])
def test_chunks_calls_and_device_runs_are_bit_invariant(orc, bfir, L, B, s, n_in, n_out):
    import torch
    nb = 2 * B + 3 + 64
    rng = np.random.default_rng(L + n_out)
    fmt = F64 if s == 8 else F32
    rows = _rows(orc, rng, n_in, n_out, B * L - 3, s, null=((1, 0),))
    x = orc.synth_audio(rng, nb * L, n_in, np.float32 if s == 4 else np.float64)
    outs = []
    for chunk in (1, 2, 5, 64, 0):
        m = bfir.BrutefirMatrix(L, B, s, n_in, n_out, fmt, fmt)
        m.set_chunk(chunk); assert m.set_coeff(rows) == 0
        rc, y = m.run(x)
        assert rc == 0
        outs.append(y.tobytes()); m.close()
    assert all(o == outs[-1] for o in outs), [o == outs[-1] for o in outs]
    m = bfir.BrutefirMatrix(L, B, s, n_in, n_out, fmt, fmt); assert m.set_coeff(rows) == 0
    parts = [m.run(x[t * L:(t + 1) * L])[1] for t in range(nb)]
    assert all(p is not None for p in parts)
    assert np.concatenate(parts).tobytes() == outs[-1]
    m.close()
    m = bfir.BrutefirMatrix(L, B, s, n_in, n_out, fmt, fmt); assert m.set_coeff(rows) == 0
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.zeros((nb * L, n_out), dtype=d_in.dtype, device="cuda")
    torch.cuda.synchronize()
    m.run_device(d_in.data_ptr(), d_out.data_ptr(), nb)
    assert m.sync() == 0
    assert d_out.cpu().numpy().tobytes() == outs[-1]
    assert rel_err(np.frombuffer(outs[-1], x.dtype).reshape(nb * L, n_out),
                   matrix_reference(orc, L, B, s, rows, x)) <= TOL[s]
    m.close()


@pytest.mark.parametrize("L,B,s", [(512, 4, 4), (256, 3, 4), (1024, 4, 8)])
def test_state_new_filters_reset_overflow_and_spectra(orc, bfir, L, B, s):
    n_in, n_out = 2, 3
    rng = np.random.default_rng(77 + L + s)
    fmt = F64 if s == 8 else F32
    dt = np.float32 if s == 4 else np.float64
    rows = _rows(orc, rng, n_in, n_out, B * L - 9, s, null=((2, 1),))
    rows2 = _rows(orc, rng, n_in, n_out, B * L - 9, s, null=((0, 0),))
    rows2 = [[None if h is None else (h * 40).astype(dt) for h in r] for r in rows2]   # loud: some outputs clip
    x = orc.synth_audio(rng, (2 * B + 3) * L, n_in, dt)
    m = bfir.BrutefirMatrix(L, B, s, n_in, n_out, fmt, fmt)
    ref = RefMatrix(orc, L, B, s, n_in, n_out)
    assert m.set_coeff(rows) == 0; ref.set_coeff(rows)
    ys, rs = [], []
    rc, y = m.run(x[:5 * L]); assert rc == 0; ys.append(y); rs.append(ref.run(x[:5 * L]))
    assert m.set_coeff(rows2) == 0; ref.set_coeff(rows2)                  # mid-stream: the delay line stays
    rc, y = m.run(x[5 * L:]); assert rc == 0; ys.append(y); rs.append(ref.run(x[5 * L:]))
    m.reset(); ref.reset()                                               # counters only: the time history stays
    rc, y = m.run(x[:7 * L]); assert rc == 0; ys.append(y); rs.append(ref.run(x[:7 * L]))
    for y, r in zip(ys, rs):
        assert rel_err(y, r) <= TOL[s]
    last, last_ref = ys[-1].astype(np.float64), rs[-1]
    clipped = 0
    for o in range(n_out):
        of = m.overflow(o)
        assert of.n_overflows == int(np.count_nonzero(np.abs(last[:, o]) > 1.0))
        assert abs(of.largest - np.abs(last_ref[:, o]).max()) <= TOL[s] * max(1.0, np.abs(last_ref[:, o]).max()) * 10
        clipped += of.n_overflows
    assert clipped > 0
    for o, i, b in ((0, 1, 0), (1, 0, B - 1), (2, 0, 1)):
        e = orc.Engine(L, B, s, 1, fmt, fmt)
        assert e.set_coeff([rows2[o][i]]) == 0
        assert rel_err(m.coeff_block(o, i, b), e.coeff_block(0, b)) <= TOL[s]
        e.close()
    m.close()


def test_refusals(orc, bfir):
    lib = bfir.load()
    for n_in, n_out in ((0, 2), (9, 2), (2, 0), (2, 9)):
        with pytest.raises(bfir.BfirError) as ei:
            bfir.BrutefirMatrix(256, 2, 4, n_in, n_out)
        assert ei.value.code == bfir.ERR_ARG
    for fi, fo in ((2, 8), (8, 6), (4, 4)):
        with pytest.raises(bfir.BfirError) as ei:
            bfir.BrutefirMatrix(256, 2, 4, 2, 2, fi, fo)
        assert ei.value.code == bfir.ERR_UNSUPPORTED
    L, B = 256, 2
    rng = np.random.default_rng(9)
    m = bfir.BrutefirMatrix(L, B, 4, 2, 2)
    d = bfir.Brutefir(L, B, 4, 2)
    h = orc.synth_ir(rng, 2, L, np.float32)
    ptrs = (C.c_void_p * 2)(*[a.ctypes.data for a in h])
    assert lib.bfir_engine_set_coeff(m.handle, ptrs, 2, L, B, 1.0) == bfir.ERR_UNSUPPORTED
    assert lib.bfir_engine_set_coeff_at(m.handle, 0, ptrs, 2, L, B, 1.0) == bfir.ERR_UNSUPPORTED
    dst = np.zeros(2 * L, np.float32)
    assert lib.bfir_engine_read_coeff(m.handle, 0, 0, dst.ctypes.data) == bfir.ERR_UNSUPPORTED
    ptrs4 = (C.c_void_p * 4)(*([h[0].ctypes.data] * 4))
    assert lib.bfir_engine_set_coeff_matrix(d.handle, ptrs4, L, B, 1.0) == bfir.ERR_UNSUPPORTED
    assert lib.bfir_engine_read_coeff_matrix(d.handle, 0, 0, 0, dst.ctypes.data) == bfir.ERR_UNSUPPORTED
    bad = h[1].copy(); bad[7] = np.inf
    assert m.set_coeff([[h[0], None], [None, h[1]]]) == 0 and m.is_initialized()
    assert m.set_coeff([[h[0], None], [None, bad]]) == bfir.ERR_COEFF
    assert not m.is_initialized()
    x = np.zeros((L, 2), np.float32)
    assert m.run(x)[0] == bfir.ERR_STATE
    m.close(); d.close()


def test_unread_input_moves_a_paired_engine_to_direct_mode_and_back(orc, bfir, creation_log):
    """An even/even fp32 engine runs channel pairs while every input feeds an output and direct mode while one does not
    (a channel pair is one transform); the delay line and the time history carry over both switches mid-stream."""
    L, B, seg = 1024, 4, 5
    rng = np.random.default_rng(404)
    dense = _rows(orc, rng, 2, 2, B * L - 21, 4)
    sparse = _rows(orc, rng, 2, 2, B * L - 21, 4, null=((0, 1), (1, 1)))
    x = orc.synth_audio(rng, 3 * seg * L, 2, np.float32)
    del creation_log[:]
    m = bfir.BrutefirMatrix(L, B, 4, 2, 2)
    assert _path(creation_log)["path"] == "pair"
    ref = RefMatrix(orc, L, B, 4, 2, 2)
    for k, rows in enumerate((dense, sparse, dense)):
        del creation_log[:]
        assert m.set_coeff(rows) == 0; ref.set_coeff(rows)
        switched = [ln for ln in creation_log if ln.startswith("bfir matrix engine: ")]
        assert switched == ([] if k == 0 else ["bfir matrix engine: %s: path=%s from the next block on."
                                               % (("an input feeds no output", "direct") if k == 1 else
                                                  ("every input feeds an output", "pair"))]), creation_log
        xs = x[k * seg * L:(k + 1) * seg * L]
        rc, y = m.run(xs)
        assert rc == 0 and rel_err(y, ref.run(xs)) <= TOL[4], k
    m.close()
