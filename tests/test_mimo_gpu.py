"""Mimo engines on the GPU (bfir_engine_create_mimo, BrutefirMimo; k_mac_mimo in csrc/mimo.hip): the two byte identities of
the header -- the matrix engine's bytes at <= 8 channels with the wide kernel forced, and a matrix engine's (a diagonal
engine's) bytes per block of a block-diagonal (diagonal) matrix -- then parity past 8 channels against two references:
size_matrix.reference_conv summed in float64, and test_mimo.mimo_reference (oracle engines over groups of 8 inputs).

Filters are size_matrix.flat_ir, each with its own tap count (0 = no filter, up to B partitions) zero-padded to the one
length a uniform matrix engine's set call takes; the frames are uniform noise with the odd inputs at 1/8.  Errors are per
block and per output (size_matrix.block_errors) against conftest.TOL."""
import ctypes as C

import numpy as np
import pytest

from conftest import TOL
from size_matrix import amplitudes, block_errors, flat_ir, reference_conv
from test_fade import fade_weights
from test_mimo import mimo_reference

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


def _made(log, kind="mimo"):
    made = [ln for ln in log if ln.startswith("bfir engine: ")]
    assert len(made) == 1 and made[0].startswith("bfir engine: %s " % kind), log
    return dict(kv.split("=") for kv in made[0].split(". ")[-1].split())


def _dt(s):
    return np.float64 if s == 8 else np.float32


def _frames(rng, nb, L, n_in, fmt):
    return (rng.uniform(-1.0, 1.0, (nb * L, n_in)) * amplitudes(nb, L, n_in, False)).astype(np.float32 if fmt == F32 else np.float64)


def _rows(rng, L, n_in, n_out, s, parts, gain=1.0):
    """rows[o][i]: a flat_ir filter of parts(o, i) partitions with a ragged end (0 partitions: None), working precision."""
    rows = []
    for o in range(n_out):
        row = []
        for i in range(n_in):
            nb = parts(o, i)
            row.append(None if nb == 0 else (flat_ir(rng, 1, nb * L - (L // 3 + 1) - (o + 2 * i) % 7)[0] * gain).astype(_dt(s)))
        rows.append(row)
    return rows


def _padded(rows, length):
    """The rows as one set call takes them: every filter zero-padded to `length` taps."""
    out = []
    for r in rows:
        out.append([None if h is None else np.concatenate([h, np.zeros(length - h.size, h.dtype)]) for h in r])
    return out


def _ref64(orc, rows, x):
    """y[:, o] = sum_i reference_conv(x_i, h_{o,i}) in float64, from the values actually sent."""
    x64 = np.asarray(x, np.float64)
    y = np.zeros((x.shape[0], len(rows)))
    for o, row in enumerate(rows):
        for i, h in enumerate(row):
            if h is not None:
                y[:, o] += reference_conv(orc, x64[:, i], np.asarray(h, np.float64))
    return y


def _worst(y, ref, L):
    e = block_errors(y, ref, L)
    live = np.abs(ref).max(axis=0) > 0          # an output without any filter is compared exactly by its test
    return float(e[live].max()) if live.any() else 0.0


def _overflow(eng, o):
    of = eng.overflow(o)
    return (of.n_overflows, of.largest, of.max)


def _run_cut(eng, x, L, cuts):
    """One run() per piece of `cuts` blocks; (verdicts, frames)."""
    rcs, ys, t = [], [], 0
    for n in cuts:
        rc, y = eng.run(x[t * L:(t + n) * L])
        rcs.append(rc); ys.append(y); t += n
    assert t * L == x.shape[0]
    return rcs, np.concatenate(ys)


# ---- 1. the matrix engine's bytes at <= 8 channels, k_mac_mimo forced --------------------------------------------------------
CUTS = (1, 2, 9, 3)   # blocks per call: the one-block-per-lane form (<= BFIR_MAT_SMALL_MAX) and the tiled form
SMALL = [
    (1024, 4, 4, 8, 8, F32, "pair", "pairs", ()),
    (256, 5, 4, 3, 5, F32, "direct", "pairs", ((1, 2), (4, 0))),
    (16, 3, 8, 3, 2, F64, "direct", "grouped", ()),
    (1024, 8, 8, 2, 2, F32, "direct", "pairs", ()),
]


@pytest.mark.parametrize("L,B,s,n_in,n_out,fmt,path,layout,null", SMALL)
def test_forced_mimo_mac_gives_the_matrix_engines_bytes(bfir, creation_log, monkeypatch, L, B, s, n_in, n_out, fmt, path, layout, null):
    rng = np.random.default_rng(L + 7 * B + n_in + s)
    nb = sum(CUTS)

    def parts(o, i):   # every count 0 .. B occurs, every input keeps a filter (the paired shape stays paired)
        return 0 if (o, i) in null else (B if o == i % n_out else 1 + (o * n_in + i) % B)
    rows = _padded(_rows(rng, L, n_in, n_out, s, parts), B * L)
    x = _frames(rng, nb, L, n_in, fmt)
    m = bfir.BrutefirMatrix(L, B, s, n_in, n_out, fmt, fmt)
    assert m.set_coeff(rows) == 0
    rc, y = m.run(x)
    assert rc == 0
    scale = 2.0 / float(np.abs(y).max())        # the upper half of the output's range clips
    m.close()
    monkeypatch.setenv("BFIR_MIMO_MAC", "1")
    outs = []
    for cls, kind in ((bfir.BrutefirMatrix, "matrix"), (bfir.BrutefirMimo, "mimo")):
        del creation_log[:]
        e = cls(L, B, s, n_in, n_out, fmt, fmt)
        got = _made(creation_log, kind)
        assert got["path"] == path and got["layout"] == layout, got
        assert e.set_coeff(rows, scale=scale) == 0
        rcs, y = _run_cut(e, x, L, CUTS)
        outs.append((rcs, y.tobytes(), [_overflow(e, o) for o in range(n_out)]))
        for o, i, b in ((0, 0, 0), (n_out - 1, n_in - 1, B - 1)):
            if rows[o][i] is not None:
                outs[-1][2].append(e.coeff_block(o, i, b).tobytes())
        e.close()
    assert outs[0][0] == outs[1][0] == [0] * len(CUTS)
    assert outs[0][1] == outs[1][1]
    assert outs[0][2] == outs[1][2]
    assert sum(n for n, _, _ in outs[1][2][:n_out]) > 0


# ---- 2. block-diagonal identities past 8 channels --------------------------------------------------------------------------------
def test_two_dense_blocks_equal_two_matrix_engines(bfir, creation_log):
    L, B, nb = 1024, 3, 2 * 3 + 3
    rng = np.random.default_rng(1616)
    blocks = [_padded(_rows(rng, L, 8, 8, 4, lambda o, i: 1 + (o + i) % B), B * L) for _ in range(2)]
    rows = [[None] * 16 for _ in range(16)]
    for k, blk in enumerate(blocks):
        for o in range(8):
            for i in range(8):
                rows[8 * k + o][8 * k + i] = blk[o][i]
    x = _frames(rng, nb, L, 16, F32)
    del creation_log[:]
    m = bfir.BrutefirMimo(L, B, 4, 16, 16)
    assert _made(creation_log)["path"] == "pair"
    assert m.set_coeff(rows) == 0
    rc, y = m.run(x)
    assert rc == 0
    for k, blk in enumerate(blocks):
        e = bfir.BrutefirMatrix(L, B, 4, 8, 8)
        assert e.set_coeff(blk) == 0
        rck, yk = e.run(np.ascontiguousarray(x[:, 8 * k:8 * k + 8]))
        assert rck == 0
        assert np.ascontiguousarray(y[:, 8 * k:8 * k + 8]).tobytes() == yk.tobytes(), k
        e.close()
    m.close()


@pytest.mark.parametrize("s,fmt,path", [(4, F32, "pair"), (8, F64, "direct")])
def test_diagonal_matrix_equals_diagonal_engines_per_group(bfir, creation_log, s, fmt, path):
    L, B, nb, Cn = 1024, 3, 2 * 3 + 3, 16
    rng = np.random.default_rng(160 + s)
    h = [(v * 120).astype(_dt(s)) for v in flat_ir(rng, Cn, B * L - 5)]   # loud enough to clip
    x = _frames(rng, nb, L, Cn, fmt)
    del creation_log[:]
    m = bfir.BrutefirMimo(L, B, s, Cn, Cn, fmt, fmt)
    assert _made(creation_log)["path"] == path
    assert m.set_coeff([[h[o] if i == o else None for i in range(Cn)] for o in range(Cn)]) == 0
    rc, y = m.run(x)
    assert rc == 0
    clipped = 0
    for g in range(0, Cn, 8):
        d = bfir.Brutefir(L, B, s, 8, fmt, fmt)
        assert d.set_coeff(h[g:g + 8]) == 0
        rcd, yd = d.run(np.ascontiguousarray(x[:, g:g + 8]))
        assert rcd == 0
        assert np.ascontiguousarray(y[:, g:g + 8]).tobytes() == yd.tobytes(), g
        for c in range(8):
            a = d.overflow(c)
            assert (a.n_overflows, a.largest, a.max) == _overflow(m, g + c)
            clipped += a.n_overflows
        d.close()
    assert clipped > 0
    m.close()


# ---- 3. parity past 8 channels --------------------------------------------------------------------------------------------------
def _banded(o, i):   # three filters per output, of 2, 1 and 2 partitions
    d = (i - o) % 64
    return {0: 2, 1: 1, 5: 2}.get(d, 0)


def _odd_parts(o, i):   # 9 -> 17: input 4 feeds nothing, output 11 gets nothing
    return 0 if i == 4 or o == 11 else 1 + (o + 2 * i) % 4


# id: (L, B, realsize, n_in, n_out, frames, path, layout, parts(o, i))
WIDE = {
    "16x16-dense": (512, 3, 4, 16, 16, F32, "pair", "pairs", lambda o, i: 1 + (o + i) % 3),
    "9x17-odd": (512, 4, 4, 9, 17, F32, "direct", "pairs", _odd_parts),
    "12x10-fp64": (64, 3, 8, 12, 10, F64, "direct", "grouped", lambda o, i: 1 + (2 * o + i) % 3),
    "64x64-banded": (1024, 2, 4, 64, 64, F32, "pair", "pairs", _banded),
    "64x2-dense": (512, 2, 4, 64, 2, F32, "pair", "pairs", lambda o, i: 1 + (o + i) % 2),
    "2x64-dense": (512, 2, 4, 2, 64, F32, "pair", "pairs", lambda o, i: 1 + (o + i) % 2),
    "33x64-nine": (256, 9, 4, 33, 64, F32, "direct", "pairs", lambda o, i: (3 * o + 7 * i) % 10 if (o + i) % 5 == 0 else 0),
}
_cases = {}


def _case(orc, cid):
    """(rows, x, float64 reference, grouped-oracle reference) of a WIDE shape: computed once, shared, never written to."""
    if cid not in _cases:
        L, B, s, n_in, n_out, fmt = WIDE[cid][:6]
        rng = np.random.default_rng(sum(cid.encode()))
        nb = B + 3                              # past the latency form's four blocks, and one block past the filters' reach
        rows = _rows(rng, L, n_in, n_out, s, WIDE[cid][8])
        x = _frames(rng, nb, L, n_in, fmt)
        refs = (_ref64(orc, rows, x), mimo_reference(orc, L, B, s, rows, x))
        for a in (x,) + refs:
            a.setflags(write=False)
        _cases[cid] = (_padded(rows, B * L), x) + refs
    return _cases[cid]


@pytest.mark.parametrize("cid", sorted(WIDE))
def test_wide_parity(orc, bfir, creation_log, cid):
    L, B, s, n_in, n_out, fmt, path, layout = WIDE[cid][:8]
    rows, x, ref, ref_orc = _case(orc, cid)
    del creation_log[:]
    m = bfir.BrutefirMimo(L, B, s, n_in, n_out, fmt, fmt)
    got = _made(creation_log)
    assert (got["path"], got["layout"]) == ("pair" if path == "pair" else "direct", layout), got
    assert m.set_coeff(rows) == 0 and m.is_initialized()
    rc, y = m.run(x)
    assert rc == 0 and y.shape == (x.shape[0], n_out)
    tol = TOL[s]
    e64, eorc = _worst(y, ref, L), _worst(y, ref_orc, L)
    print("%s: worst block error %.3g against float64, %.3g against the grouped oracle" % (cid, e64, eorc))
    assert e64 <= tol and eorc <= tol
    for o in range(n_out):
        if all(h is None for h in rows[o]):
            assert not np.any(y[:, o]), o       # no filter at all: exact zeros
    for o, i, b in ((0, 0, 0), (n_out - 1, n_in - 1, 0)):
        if rows[o][i] is not None:
            e = orc.Engine(L, B, s, 1, F64 if s == 8 else F32, F64 if s == 8 else F32)
            assert e.set_coeff([rows[o][i]]) == 0
            d = np.abs(m.coeff_block(o, i, b).astype(np.float64) - e.coeff_block(0, b))
            assert d.max() <= tol * np.abs(e.coeff_block(0, b)).max()
            e.close()
    m.close()


# ---- 4. an input no filter reads ------------------------------------------------------------------------------------------------
def test_unread_input_keeps_its_nan_to_itself(orc, bfir, creation_log):
    """12 -> 12 on the pair-capable shape with column 5 empty: direct mode, a NaN on input 5 reaches no output and no verdict.
    Once the column gets a filter (and the NaN has left the delay line) the engine pairs again."""
    L, B, n, seg = 512, 2, 12, 5
    rng = np.random.default_rng(1212)
    sparse = _rows(rng, L, n, n, 4, lambda o, i: 0 if i == 5 else 1 + (o + i) % 2)
    dense = _rows(rng, L, n, n, 4, lambda o, i: 1 + (o + i) % 2)
    x = _frames(rng, 2 * seg, L, n, F32)
    clean = x.copy()
    x[1 * L + 9, 5] = np.nan
    clean[1 * L + 9, 5] = 0.0
    del creation_log[:]
    m = bfir.BrutefirMimo(L, B, 4, n, n)
    assert _made(creation_log)["path"] == "pair"
    want = ("bfir matrix engine: an input feeds no output: path=direct from the next block on.",
            "bfir matrix engine: every input feeds an output: path=pair from the next block on.")
    for k, rows in enumerate((sparse, dense)):
        del creation_log[:]
        assert m.set_coeff(_padded(rows, B * L)) == 0
        assert [ln for ln in creation_log if ln.startswith("bfir matrix engine: ")] == [want[k]], creation_log
        rc, y = m.run(x[k * seg * L:(k + 1) * seg * L])
        assert rc == 0 and np.all(np.isfinite(y)), k
        # the delay line holds only finite blocks of the inputs the set reads, so block t is the convolution of the whole
        # (clean) stream with the set in force
        for ref in (_ref64(orc, rows, clean), mimo_reference(orc, L, B, 4, rows, clean)):
            assert _worst(y, ref[k * seg * L:(k + 1) * seg * L], L) <= TOL[4], k
    m.close()


# ---- 5. how the blocks arrive ---------------------------------------------------------------------------------------------------
def test_chunks_calls_and_device_runs_are_bit_invariant(orc, bfir):
    import torch
    cid = "16x16-dense"
    L, B, s, n_in, n_out = WIDE[cid][:5]
    rows, x, ref, _ = _case(orc, cid)
    nb = x.shape[0] // L

    def engine(chunk=0):
        m = bfir.BrutefirMimo(L, B, s, n_in, n_out)
        m.set_chunk(chunk)
        assert m.set_coeff(rows) == 0
        return m
    m = engine()
    rc, y = m.run(x); m.close()
    assert rc == 0 and _worst(y, ref, L) <= TOL[s]
    one = y.tobytes()
    m = engine(3)
    rc, y = m.run(x); m.close()
    assert rc == 0 and y.tobytes() == one
    m = engine()
    rcs, y = _run_cut(m, x, L, (1,) * nb); m.close()
    assert rcs == [0] * nb and y.tobytes() == one
    m = engine()
    d_in = torch.from_numpy(x.copy()).cuda()
    d_out = torch.zeros((nb * L, n_out), dtype=d_in.dtype, device="cuda")
    torch.cuda.synchronize()
    m.run_device(d_in.data_ptr(), d_out.data_ptr(), nb)
    assert m.sync() == 0
    assert d_out.cpu().numpy().tobytes() == one
    m.close()


# ---- 6. crossfades ---------------------------------------------------------------------------------------------------------------
def test_fade_past_eight_channels(orc, bfir):
    """12 -> 12, three fading blocks from block 4 on, one filter absent from the old set only (it fades in)."""
    L, B, n, K, t0, nb = 512, 2, 12, 3, 4, 10
    rng = np.random.default_rng(66)
    new = _rows(rng, L, n, n, 4, lambda o, i: 1 + (o + i) % 2)
    old = _rows(rng, L, n, n, 4, lambda o, i: 0 if (o, i) == (3, 7) else 1 + (o + 2 * i) % 2)
    x = _frames(rng, nb, L, n, F32)
    m = bfir.BrutefirMimo(L, B, 4, n, n)
    assert m.set_coeff(_padded(old, B * L)) == 0
    rc0, y0 = m.run(x[:t0 * L])
    assert m.set_coeff_fade(_padded(new, B * L), K) == 0 and m.fade_remaining() == K
    rc1, y1 = m.run(x[t0 * L:])
    assert rc0 == rc1 == 0 and m.fade_remaining() == 0
    y = np.concatenate([y0, y1])
    w = fade_weights(L, nb, t0, K)[:, None]
    for name, f in (("float64", lambda r: _ref64(orc, r, x)), ("grouped oracle", lambda r: mimo_reference(orc, L, B, 4, r, x))):
        want = f(old) * (1.0 - w) + f(new) * w
        err = _worst(y, want, L)
        print("fade 12 -> 12: worst block error %.3g against the %s blend" % (err, name))
        assert err <= TOL[4]
    m.close()


def test_fade_with_forced_mimo_mac_gives_the_matrix_engines_bytes(bfir, monkeypatch):
    L, B, n, K, t0, nb = 1024, 3, 8, 3, 2, 9
    rng = np.random.default_rng(88)
    old = _padded(_rows(rng, L, n, n, 4, lambda o, i: 1 + (o + i) % B), B * L)
    new = _padded(_rows(rng, L, n, n, 4, lambda o, i: 0 if (o, i) == (2, 6) else 1 + (o + 2 * i) % B), B * L)
    x = _frames(rng, nb, L, n, F32)
    monkeypatch.setenv("BFIR_MIMO_MAC", "1")
    outs = []
    for cls in (bfir.BrutefirMatrix, bfir.BrutefirMimo):
        e = cls(L, B, 4, n, n)
        assert e.set_coeff(old) == 0
        rc0, y0 = e.run(x[:t0 * L])
        assert e.set_coeff_fade(new, K) == 0
        rc1, y1 = e.run(x[t0 * L:(t0 + 1) * L])           # one fading block on the latency path
        rc2, y2 = e.run(x[(t0 + 1) * L:])                  # the rest of the fade and the new set alone
        assert rc0 == rc1 == rc2 == 0 and e.fade_remaining() == 0
        outs.append(np.concatenate([y0, y1, y2]).tobytes())
        e.close()
    assert outs[0] == outs[1]


# ---- 7. overflow statistics and refusals ----------------------------------------------------------------------------------------
def test_overflow_counts_of_the_upper_outputs(orc, bfir):
    """16 -> 16 with a gain that clips.  Every output's counter, 8 .. 15 among them, is numpy's count of |y| > 1 on the frames
    the engine wrote, to the sample, and what the reference says: a sample within d = TOL max |ref| of full scale may fall on
    either side, so the counter lies between the reference's counts at 1 + d and at 1 - d."""
    L, B, n, nb = 512, 2, 16, 7
    rng = np.random.default_rng(1600)
    rows = _rows(rng, L, n, n, 4, lambda o, i: 1 + (o + i) % 2, gain=12.0)
    x = _frames(rng, nb, L, n, F32)
    ref = _ref64(orc, rows, x)
    m = bfir.BrutefirMimo(L, B, 4, n, n)
    assert m.set_coeff(_padded(rows, B * L)) == 0
    rc, y = m.run(x)
    assert rc == 0 and _worst(y, ref, L) <= TOL[4]
    counts = []
    for o in range(n):
        of = m.overflow(o)
        peak = np.abs(ref[:, o]).max()
        d = TOL[4] * peak
        lo, hi = (int(np.count_nonzero(np.abs(ref[:, o]) > 1.0 + s * d)) for s in (1, -1))
        assert of.n_overflows == int(np.count_nonzero(np.abs(y[:, o]) > 1.0)), o
        assert lo <= of.n_overflows <= hi, (o, lo, of.n_overflows, hi)
        assert abs(of.largest - peak) <= d and of.max == 1.0, o
        counts.append(of.n_overflows)
    assert min(counts[8:]) > 0 and max(counts) < nb * L
    for ch in (-1, n):
        with pytest.raises(bfir.BfirError) as ei:
            m.overflow(ch)
        assert ei.value.code == bfir.ERR_ARG
    m.close()


def test_refusals_change_nothing(orc, bfir):
    import torch
    cid = "16x16-dense"
    L, B, s, n_in, n_out = WIDE[cid][:5]
    rows, x, ref, _ = _case(orc, cid)
    nb = x.shape[0] // L
    lib = bfir.load()
    for a, b in ((65, 2), (2, 65), (0, 1)):
        with pytest.raises(bfir.BfirError) as ei:
            bfir.BrutefirMimo(L, B, s, a, b)
        assert ei.value.code == bfir.ERR_ARG
    m = bfir.BrutefirMimo(L, B, s, n_in, n_out)
    assert m.set_coeff(rows) == 0
    # the calls of the other kinds, and the delays
    for side in (0, 1):
        with pytest.raises(bfir.BfirError) as ei:
            m.delay_init(side, 16)
        assert ei.value.code == bfir.ERR_UNSUPPORTED
        assert m.set_delay(side, [0] * 16) == bfir.ERR_UNSUPPORTED and m.delay_latency(side) == bfir.ERR_UNSUPPORTED
    h = [r for r in rows[0]]
    ptrs = (C.c_void_p * n_in)(*[a.ctypes.data for a in h])
    assert lib.bfir_engine_set_coeff(m.handle, ptrs, n_in, B * L, B, 1.0) == bfir.ERR_UNSUPPORTED
    assert lib.bfir_engine_set_coeff_at(m.handle, 0, ptrs, n_in, B * L, B, 1.0) == bfir.ERR_UNSUPPORTED
    assert lib.bfir_engine_set_coeff_fade(m.handle, ptrs, n_in, B * L, B, 1.0, 2) == bfir.ERR_UNSUPPORTED
    assert lib.bfir_engine_set_coeff_nup(m.handle, ptrs, n_in, B * L, 1.0) == bfir.ERR_UNSUPPORTED
    assert lib.bfir_engine_set_coeff_levels(m.handle, ptrs, n_in, B * L, 1.0) == bfir.ERR_UNSUPPORTED
    flat = [a for r in rows for a in r]
    pm = (C.c_void_p * len(flat))(*[a.ctypes.data for a in flat])
    lens = (C.c_int * len(flat))(*[B * L] * len(flat))
    assert lib.bfir_engine_set_coeff_matrix_levels(m.handle, pm, lens, 1.0) == bfir.ERR_UNSUPPORTED
    assert lib.bfir_engine_set_coeff_matrix_levels_fade(m.handle, pm, lens, 1.0, 2) == bfir.ERR_UNSUPPORTED
    dst = np.zeros(2 * L, np.float32)
    assert lib.bfir_engine_read_coeff(m.handle, 0, 0, dst.ctypes.data) == bfir.ERR_UNSUPPORTED
    assert m.is_initialized() and m.fade_remaining() == 0
    # a launch past k_mac_mimo's grid: refused before anything is allocated or queued (these buffers hold one block)
    d_in = torch.zeros((L, n_in), dtype=torch.float32, device="cuda")
    d_out = torch.zeros((L, n_out), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    huge = 1 << 23
    m.set_chunk(huge)
    with pytest.raises(bfir.BfirError) as ei:
        m.run_device(d_in.data_ptr(), d_out.data_ptr(), huge)
    assert ei.value.code == bfir.ERR_UNSUPPORTED
    assert m.sync() == 0
    m.set_chunk(0)
    rc, y = m.run(x)
    assert rc == 0
    fresh = bfir.BrutefirMimo(L, B, s, n_in, n_out)
    assert fresh.set_coeff(rows) == 0
    rcf, yf = fresh.run(x)
    assert rcf == 0 and y.tobytes() == yf.tobytes()
    assert block_errors(y, ref, L).max() <= TOL[s]
    assert nb > 4
    m.close(); fresh.close()
