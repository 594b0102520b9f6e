"""Pair-list coefficient updates on the GPU (bfir_engine_set_coeff_matrix_pairs, _pairs_fade; k_patch_pairs in
csrc/patch.hip) on matrix and mimo engines, one shape per spectrum layout and precision.

The twins.  A whole-matrix set call gives every filter the one partition count of the call, a patch gives the listed pairs
theirs, so a twin cannot hold a patched engine's counts.  It holds the same spectra: a filter loaded with coeff_blocks = c is
the filter cut to c L taps (partition p is the transform of taps [p L, (p + 1) L) alone, the partitions past c read as zeros
either way), and a partition of zeros adds fma(x, 0, acc) = acc to a sum that is not -0.  So the twin takes every filter cut
to what its call loaded, at coeff_blocks = B, and the bytes -- outputs and bfir_engine_read_coeff_matrix -- are the same.

The references are those of test_mimo_gpu: size_matrix.reference_conv summed in float64 (_ref64) and the grouped oracle
(test_mimo.mimo_reference), blended with test_fade.fade_weights; errors per block and output against conftest.TOL."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import TOL
from size_matrix import flat_ir
from test_fade import fade_weights
from test_mimo import mimo_reference
from test_mimo_gpu import _frames, _padded, _ref64, _rows, _run_cut, _worst
from test_pairs import merge

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = 8, 10
CUTS = (1, 2, 9, 3)   # blocks per call behind the patch: the one-block-per-lane form and the tiled form

# id: (class, L, B, realsize, n_in, n_out, frames, layout)
CASES = {
    "matrix-f64-grouped": ("BrutefirMatrix", 16, 3, 8, 3, 2, F64, "grouped"),
    "matrix-f32-direct": ("BrutefirMatrix", 256, 4, 4, 3, 5, F32, "pairs"),
    "mimo-f32-pair": ("BrutefirMimo", 512, 2, 4, 12, 12, F32, "pairs"),
    "matrix-f64-pairs": ("BrutefirMatrix", 1024, 3, 8, 2, 2, F64, "pairs"),
}
LISTS = ("column", "single", "row3", "mixed")
SMALL = "matrix-f64-grouped"   # the 3 -> 2 shape of the state and error tests


@pytest.fixture(scope="module")
def log(bfir):
    from foo_dsp_bfir_amd import _lib
    lines = []
    cb = _lib.LOG_FN(lambda msg: lines.append(msg.decode(errors="replace")))
    lib = bfir.load()
    lib.bfir_set_log_callback(cb)
    yield lines
    lib.bfir_set_log_callback(_lib.LOG_FN())


def _dt(s):
    return np.float64 if s == 8 else np.float32


def _cut(h, taps):
    """What a call with coeff_blocks = taps / L loads of a filter."""
    return None if h is None else np.ascontiguousarray(h[:taps])


def _filt(rng, s, taps, length):
    """A flat_ir filter of `taps` taps, zero-padded to `length`: a pairs call takes ONE length for all its filters."""
    h = np.zeros(length, _dt(s))
    h[:taps] = flat_ir(rng, 1, taps)[0]
    return h


def _engine(bfir, cid, rows, chunk=None):
    cls, L, B, s, n_in, n_out, fmt, _ = CASES[cid]
    e = getattr(bfir, cls)(L, B, s, n_in, n_out, fmt, fmt)
    if chunk is not None:
        e.set_chunk(chunk)
    assert e.set_coeff(_padded(rows, B * L)) == 0
    return e


def _old_rows(cid):
    """The first set of a shape: ragged filters of 1 .. B partitions -- (0, 0) with taps in all B, so that a patch to fewer
    partitions has live old partitions past the new count to take away -- pair (0, n_in - 1) without a path; every input read."""
    _, L, B, s, n_in, n_out, _, _ = CASES[cid]
    rng = np.random.default_rng(sum(cid.encode()))
    return _rows(rng, L, n_in, n_out, s, lambda o, i: 0 if (o, i) == (0, n_in - 1) else B if (o, i) == (0, 0) else 1 + (o + i) % B)


def _pair_list(cid, kind):
    """(pre, pairs, filters, coeff_blocks): `pre` is a patch applied before the first block -- pair (n_out - 1, 0) at ONE
    partition, so that the set holds mixed counts -- or None; then the list under test.
    column   every output's filter from input 1
    single   one pair
    row3     three pairs of row 0 (all of it where the row is shorter), the other rows none
    mixed    at coeff_blocks = max(1, B - 1): (0, 0) had B partitions of taps (fewer now; B = 2: 1 of 2), (n_out - 1, 0) had one
             (more now where B >= 3), (0, n_in - 1) had no path (added), (1, 1) loses its path (removed)
    Every filter has a ragged end and is zero-padded to B L taps."""
    _, L, B, s, n_in, n_out, _, _ = CASES[cid]
    rng = np.random.default_rng(sum((cid + kind).encode()))
    pre, cb = None, B
    if kind == "column":
        pairs = [(o, 1) for o in range(n_out)]
    elif kind == "single":
        pairs = [(n_out - 1, 0)]
    elif kind == "row3":
        pairs = [(0, i) for i in range(min(3, n_in))][::-1]          # listed out of input order
    else:
        pre = ([(n_out - 1, 0)], [_filt(rng, s, B * L - 3, B * L)])
        pairs, cb = [(0, 0), (n_out - 1, 0), (0, n_in - 1), (1, 1)], max(1, B - 1)
    filters = [_filt(rng, s, B * L - 1 - 2 * k, B * L) for k in range(len(pairs))]
    if kind == "mixed":
        filters[3] = None
    return pre, pairs, filters, cb


_setups = {}


def _setup(orc, cid, kind):
    """Everything the tests of one (shape, list) share, computed once and never written to: the frames, the set before the
    patch and the merged set as the engine holds them (cut to what each call loads), and both references of both."""
    if (cid, kind) not in _setups:
        _, L, B, s, n_in, n_out, fmt, _ = CASES[cid]
        pre, pairs, filters, cb = _pair_list(cid, kind)
        old = _old_rows(cid)
        if pre:
            old = merge(old, pre[0], [_cut(h, L) for h in pre[1]])
        merged = merge(old, pairs, [_cut(h, cb * L) for h in filters])
        t0 = 2 * B + 3
        nb = t0 + sum(CUTS)
        x = _frames(np.random.default_rng(len(cid) + 31 * len(kind)), nb, L, n_in, fmt)
        x.setflags(write=False)
        refs = {}
        for name, rows in (("old", old), ("merged", merged)):
            refs[name] = (_ref64(orc, rows, x), mimo_reference(orc, L, B, s, rows, x))
        _setups[(cid, kind)] = dict(pre=pre, pairs=pairs, filters=filters, cb=cb, old=old, merged=merged, t0=t0, nb=nb, x=x, refs=refs)
    return _setups[(cid, kind)]


def _start(bfir, cid, S, chunk=None):
    """An engine on S's old set, reached the way the list asks: the first set, then `pre` as a one-partition patch."""
    e = _engine(bfir, cid, _old_rows(cid), chunk)
    if S["pre"]:
        assert e.set_coeff_pairs(S["pre"][0], S["pre"][1], coeff_blocks=1) == 0
    return e


def _all_blocks(e, cid):
    _, L, B, s, n_in, n_out, _, _ = CASES[cid]
    return np.concatenate([e.coeff_block(o, i, b) for o in range(n_out) for i in range(n_in) for b in range(B)])


def _same_store(a, b, cut=False):
    """Two filter stores: byte for byte -- except between an engine whose call loaded fewer partitions than a filter has and
    its twin (`cut`), where the partitions past the count are cleared memory on one side and the transform of zero taps on
    the other: zeros of either sign, equal as numbers."""
    return np.array_equal(a, b) if cut else a.tobytes() == b.tobytes()


# ---- 1. the plain call equals a whole reload -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", LISTS)
@pytest.mark.parametrize("cid", sorted(CASES))
def test_plain_patch_equals_whole_reload(orc, bfir, log, cid, kind):
    _, L, B, s, n_in, n_out, fmt, layout = CASES[cid]
    S = _setup(orc, cid, kind)
    x, t0 = S["x"], S["t0"]
    del log[:]
    e = _start(bfir, cid, S, chunk=2)
    made = [ln for ln in log if ln.startswith("bfir engine: ")]
    assert len(made) == 1 and "layout=%s" % layout in made[0], made
    twin = _engine(bfir, cid, S["old"], chunk=2)
    cut = kind == "mixed"
    assert _same_store(_all_blocks(e, cid), _all_blocks(twin, cid), cut)   # the one-partition patch before the first block
    rc0, y0 = e.run(x[:t0 * L])                                      # 2 B + 3 blocks in launches of two: the ring has wrapped
    rct, yt = twin.run(x[:t0 * L])
    assert rc0 == rct == 0 and y0.tobytes() == yt.tobytes()
    assert e.set_coeff_pairs(S["pairs"], S["filters"], coeff_blocks=S["cb"]) == 0
    assert twin.set_coeff(_padded(S["merged"], B * L)) == 0
    assert e.is_initialized() and e.fade_remaining() == 0
    assert _same_store(_all_blocks(e, cid), _all_blocks(twin, cid), cut)
    rcs, y1 = _run_cut(e, x[t0 * L:], L, CUTS)
    rct, yt = _run_cut(twin, x[t0 * L:], L, CUTS)
    assert rcs == rct == [0] * len(CUTS)
    assert y1.tobytes() == yt.tobytes()
    # ... and the stream as a whole is the old set's up to the patch and the merged set's behind it
    y = np.concatenate([y0, y1])
    for k in (0, 1):
        assert _worst(y[:t0 * L], S["refs"]["old"][k][:t0 * L], L) <= TOL[s]
        assert _worst(y[t0 * L:], S["refs"]["merged"][k][t0 * L:], L) <= TOL[s]
    e.close(); twin.close()


# ---- 2. the fade -----------------------------------------------------------------------------------------------------------------
def _check_fade(start, cid, S, K, y, label):
    """start() gives a fresh engine on S's old set.  The three ranges of a pairs fade of K blocks from block t0 on in the whole stream y: before it an unpatched twin's
    bytes, in it the float64 blend of both references, behind it the bytes of a twin that faded with the whole-matrix call."""
    _, L, B, s, n_in, n_out, _, _ = CASES[cid]
    x, t0, nb = S["x"], S["t0"], S["nb"]
    a = start()
    rca, ya = a.run(x[:t0 * L]); a.close()
    assert rca == 0 and y[:t0 * L].tobytes() == ya.tobytes()
    w = fade_weights(L, nb, t0, K)[:, None]
    for k, name in enumerate(("float64", "grouped oracle")):
        want = S["refs"]["old"][k] * (1.0 - w) + S["refs"]["merged"][k] * w
        err = _worst(y[t0 * L:(t0 + K) * L], want[t0 * L:(t0 + K) * L], L)
        print("%s %s: worst fading block %.3g against the %s blend" % (cid, label, err, name))
        assert err <= TOL[s]
        assert _worst(y, want, L) <= TOL[s]
    b = start()
    rc0, _y = b.run(x[:t0 * L])
    assert b.set_coeff_fade(_padded(S["merged"], B * L), K) == 0
    rc1, yb = b.run(x[t0 * L:])
    assert rc0 == rc1 == 0
    assert y[(t0 + K) * L:].tobytes() == yb[K * L:].tobytes()
    err = _worst(y[t0 * L:(t0 + K) * L], yb[:K * L].astype(np.float64), L)
    print("%s %s: worst fading block %.3g from the whole-matrix fade's" % (cid, label, err))
    return b


@pytest.mark.parametrize("K", (3, 11))
@pytest.mark.parametrize("kind", LISTS)
@pytest.mark.parametrize("cid", sorted(CASES))
def test_fade(orc, bfir, cid, kind, K):
    """The first fading block arrives alone, the rest of the stream in one call: K = 3 is launches of 1 + 2 blocks, both the
    one-block form; K = 11 is 1 + 10, the ten in the tiled form with a ragged last tile (8 + 2 in fp32, 4 + 4 + 2 in fp64).
    One launch of all 11 (8 + 3, 4 + 4 + 3) is test 3's.  t0 = 2 B + 3 is no multiple of 8."""
    _, L, B, s, n_in, n_out, _, _ = CASES[cid]
    S = _setup(orc, cid, kind)
    x, t0, nb = S["x"], S["t0"], S["nb"]
    assert t0 % 8 and t0 + K < nb
    e = _start(bfir, cid, S)
    rc0, y0 = e.run(x[:t0 * L])
    assert e.fade_remaining() == 0
    before = _all_blocks(e, cid)
    assert e.set_coeff_pairs_fade(S["pairs"], S["filters"], K, coeff_blocks=S["cb"]) == 0
    assert e.fade_remaining() == K
    assert _same_store(_all_blocks(e, cid), before)                  # the old set is read until the last fading block is queued
    rc1, y1 = e.run(x[t0 * L:(t0 + 1) * L])
    assert e.fade_remaining() == K - 1
    rc2, y2 = e.run(x[(t0 + 1) * L:])
    assert rc0 == rc1 == rc2 == 0 and e.fade_remaining() == 0
    twin = _check_fade(lambda: _start(bfir, cid, S), cid, S, K, np.concatenate([y0, y1, y2]), "%s K=%d" % (kind, K))
    assert _same_store(_all_blocks(e, cid), _all_blocks(twin, cid), kind == "mixed")   # the merged set is active
    e.close(); twin.close()


def test_fade_on_a_large_store_holds_the_listed_row(bfir):
    """64 -> 64 at L = 1024, B = 16: a filter store of 512 MiB, whose copy into the second set takes several times as long
    as loading one row.  The one listed pair lies in the last output row, at the end of the store: after the fade it holds
    the new filter's spectra, byte for byte those a small engine gives the same taps, and its neighbours are untouched."""
    L, B, n = 1024, 16, 64
    rng = np.random.default_rng(6464)
    base = [_filt(rng, 4, B * L - 7 - k, B * L) * np.float32(0.01) for k in range(n)]
    new = _filt(rng, 4, B * L - 3, B * L) * np.float32(0.01)
    e = bfir.BrutefirMimo(L, B, 4, n, n)
    assert e.set_coeff([[base[(o + i) % n] for i in range(n)] for o in range(n)]) == 0
    near = [(n - 1, 4), (n - 1, 6), (n - 1, n - 1), (n - 2, 5)]
    before = [e.coeff_block(o, i, b).tobytes() for o, i in near for b in (0, B - 1)]
    assert e.set_coeff_pairs_fade([(n - 1, 5)], [new], 1) == 0
    rc, _y = e.run(np.zeros((2 * L, n), np.float32))
    assert rc == 0 and e.fade_remaining() == 0
    small = bfir.BrutefirMatrix(L, B, 4, 2, 2)
    assert small.set_coeff([[new, None], [None, new]]) == 0
    for b in range(B):
        assert e.coeff_block(n - 1, 5, b).tobytes() == small.coeff_block(0, 0, b).tobytes(), b
    assert [e.coeff_block(o, i, b).tobytes() for o, i in near for b in (0, B - 1)] == before
    e.close(); small.close()


# ---- 3. how the blocks arrive ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ("mimo-f32-pair", "matrix-f64-pairs"))
def test_fade_does_not_depend_on_how_the_blocks_arrive(orc, bfir, cid):
    import torch
    _, L, B, s, n_in, n_out, fmt, _ = CASES[cid]
    S = _setup(orc, cid, "mixed")
    x, t0, nb, K = S["x"], S["t0"], S["nb"], 11

    def faded(chunk, cuts, device=False):
        e = _start(bfir, cid, S, chunk)
        rc0, y0 = e.run(x[:t0 * L])
        assert rc0 == 0 and e.set_coeff_pairs_fade(S["pairs"], S["filters"], K, coeff_blocks=S["cb"]) == 0
        if device:
            d_in = torch.from_numpy(x[t0 * L:].copy()).cuda()
            d_out = torch.zeros(((nb - t0) * L, n_out), dtype=d_in.dtype, device="cuda")
            torch.cuda.synchronize()
            e.run_device(d_in.data_ptr(), d_out.data_ptr(), nb - t0)
            assert e.sync() == 0
            y1 = d_out.cpu().numpy()
        else:
            rcs, y1 = _run_cut(e, x[t0 * L:], L, cuts)
            assert rcs == [0] * len(cuts)
        assert e.fade_remaining() == 0
        e.close()
        return y0.tobytes() + y1.tobytes()
    one = faded(None, (nb - t0,))                                   # the default chunk, one call
    assert faded(1, (nb - t0,)) == one                              # launches of one block
    assert faded(None, (1,) * (nb - t0)) == one                     # one call per block
    assert faded(None, None, device=True) == one                    # device pointers


# ---- 4. a patch that changes the path -------------------------------------------------------------------------------------------
def test_patch_that_empties_a_column_takes_the_direct_path(orc, bfir, log):
    cid = "mimo-f32-pair"
    _, L, B, s, n_in, n_out, fmt, _ = CASES[cid]
    rng = np.random.default_rng(4242)
    old = _rows(rng, L, n_in, n_out, s, lambda o, i: (2 if o == 3 else 0) if i == 5 else 1 + (o + i) % B)   # input 5 feeds output 3 alone
    pairs, filters, K = [(3, 5), (0, 0)], [None, _filt(rng, s, B * L - 9, B * L)], 11
    t0, nb = 2 * B + 3, 2 * B + 3 + sum(CUTS)
    x = _frames(rng, nb, L, n_in, fmt)
    merged = merge(old, pairs, filters)
    S = dict(pre=None, pairs=pairs, filters=filters, cb=B, old=old, merged=merged, t0=t0, nb=nb, x=x,
             refs={k: (_ref64(orc, r, x), mimo_reference(orc, L, B, s, r, x)) for k, r in (("old", old), ("merged", merged))})
    del log[:]
    e = bfir.BrutefirMimo(L, B, s, n_in, n_out)
    assert "path=pair" in [ln for ln in log if ln.startswith("bfir engine: ")][0]
    assert e.set_coeff(_padded(old, B * L)) == 0
    rc0, y0 = e.run(x[:t0 * L])
    del log[:]
    assert e.set_coeff_pairs_fade(pairs, filters, K) == 0
    assert [ln for ln in log if ln.startswith("bfir matrix engine: ")] == \
        ["bfir matrix engine: an input feeds no output: path=direct from the next block on."], log
    rc1, y1 = e.run(x[t0 * L:])
    assert rc0 == rc1 == 0 and e.fade_remaining() == 0
    assert not [ln for ln in log if "path=pair" in ln], log          # the merged set keeps the direct path
    y = np.concatenate([y0, y1])

    def start():
        t = bfir.BrutefirMimo(L, B, s, n_in, n_out)
        assert t.set_coeff(_padded(old, B * L)) == 0
        return t
    twin = _check_fade(start, cid, S, K, y, "column 5 emptied K=%d" % K)
    e.close(); twin.close()


# ---- 5. an input no filter reads ------------------------------------------------------------------------------------------------
def test_unread_input_keeps_its_nan_through_a_patch_fade(orc, bfir):
    cid = "mimo-f32-pair"
    _, L, B, s, n_in, n_out, fmt, _ = CASES[cid]
    rng = np.random.default_rng(555)
    old = _rows(rng, L, n_in, n_out, s, lambda o, i: 0 if i == 5 else 1 + (o + i) % B)
    x = _frames(rng, 12, L, n_in, fmt)
    x[:, 5] = np.nan                                                  # every block of the unread input
    e = bfir.BrutefirMimo(L, B, s, n_in, n_out)
    assert e.set_coeff(_padded(old, B * L)) == 0
    rc0, y0 = e.run(x[:5 * L])
    # a None -> None pair of the unread input between two real replacements of its row, and one alone in its row
    pairs, filters = [(2, 4), (2, 5), (2, 6), (7, 5)], [_filt(rng, s, B * L - 4, B * L), None, _filt(rng, s, L - 2, B * L), None]
    assert e.set_coeff_pairs_fade(pairs, filters, 3) == 0
    rc1, y1 = e.run(x[5 * L:])
    assert rc0 == rc1 == 0 and e.fade_remaining() == 0
    y = np.concatenate([y0, y1])
    assert np.all(np.isfinite(y))
    clean = x.copy(); clean[:, 5] = 0.0
    w = fade_weights(L, 12, 5, 3)[:, None]
    want = _ref64(orc, old, clean) * (1.0 - w) + _ref64(orc, merge(old, pairs, filters), clean) * w
    assert _worst(y, want, L) <= TOL[s]
    e.close()


# ---- 6. state --------------------------------------------------------------------------------------------------------------------
def _small(orc):
    S = _setup(orc, SMALL, "column")
    rng = np.random.default_rng(606)
    _, L, B, s, n_in, n_out, _, _ = CASES[SMALL]
    second = ([(1, 2), (0, 0)], [_filt(rng, s, B * L - 2, B * L), None])    # another list, for whatever follows the first fade
    return S, second


def test_plain_patch_during_a_pairs_fade_cancels_it(orc, bfir):
    _, L, B, s, n_in, n_out, _, _ = CASES[SMALL]
    S, (pairs2, filters2) = _small(orc)
    x, t0 = S["x"], S["t0"]
    e, twin = _start(bfir, SMALL, S), _start(bfir, SMALL, S)
    for g in (e, twin):
        assert g.run(x[:t0 * L])[0] == 0
    assert e.set_coeff_pairs_fade(S["pairs"], S["filters"], 5) == 0
    assert e.run(x[t0 * L:(t0 + 2) * L])[0] == 0 and e.fade_remaining() == 3
    assert twin.run(x[t0 * L:(t0 + 2) * L])[0] == 0                  # the old set: its delay line is the same
    assert e.set_coeff_pairs(pairs2, filters2) == 0 and e.fade_remaining() == 0
    assert twin.set_coeff(_padded(merge(S["old"], pairs2, filters2), B * L)) == 0   # the OLD set, patched hard
    assert _same_store(_all_blocks(e, SMALL), _all_blocks(twin, SMALL))
    (rc, y), (rct, yt) = e.run(x[(t0 + 2) * L:]), twin.run(x[(t0 + 2) * L:])
    assert rc == rct == 0 and y.tobytes() == yt.tobytes()
    e.close(); twin.close()


def test_reset_during_a_pairs_fade_leaves_the_merged_set(orc, bfir):
    _, L, B, s, n_in, n_out, _, _ = CASES[SMALL]
    S, _ = _small(orc)
    x, t0 = S["x"], S["t0"]
    e, twin = _start(bfir, SMALL, S), _start(bfir, SMALL, S)
    for g in (e, twin):
        assert g.run(x[:(t0 + 2) * L if g is twin else t0 * L])[0] == 0
    assert e.set_coeff_pairs_fade(S["pairs"], S["filters"], 5, coeff_blocks=S["cb"]) == 0
    assert e.run(x[t0 * L:(t0 + 2) * L])[0] == 0 and e.fade_remaining() == 3
    assert twin.set_coeff(_padded(S["merged"], B * L)) == 0
    e.reset(); twin.reset()
    assert e.fade_remaining() == 0 and _same_store(_all_blocks(e, SMALL), _all_blocks(twin, SMALL))
    (rc, y), (rct, yt) = e.run(x[(t0 + 2) * L:]), twin.run(x[(t0 + 2) * L:])
    assert rc == rct == 0 and y.tobytes() == yt.tobytes()
    # the patch flag went with the fade: a whole-matrix fade behind it is a whole-matrix fade
    for g in (e, twin):
        assert g.set_coeff_fade(_padded(S["old"], B * L), 2) == 0
    (rc, y), (rct, yt) = e.run(x[:4 * L]), twin.run(x[:4 * L])
    assert rc == rct == 0 and y.tobytes() == yt.tobytes()
    e.close(); twin.close()


def test_whole_matrix_set_during_a_pairs_fade_cuts_hard(orc, bfir):
    _, L, B, s, n_in, n_out, _, _ = CASES[SMALL]
    S, (pairs2, filters2) = _small(orc)
    x, t0 = S["x"], S["t0"]
    other = _padded(merge(S["old"], pairs2, filters2), B * L)
    e, twin = _start(bfir, SMALL, S), _start(bfir, SMALL, S)
    assert e.run(x[:t0 * L])[0] == 0 and twin.run(x[:(t0 + 2) * L])[0] == 0
    assert e.set_coeff_pairs_fade(S["pairs"], S["filters"], 5) == 0
    assert e.run(x[t0 * L:(t0 + 2) * L])[0] == 0
    for g in (e, twin):
        assert g.set_coeff(other) == 0 and g.fade_remaining() == 0
    (rc, y), (rct, yt) = e.run(x[(t0 + 2) * L:]), twin.run(x[(t0 + 2) * L:])
    assert rc == rct == 0 and y.tobytes() == yt.tobytes()
    e.close(); twin.close()


def test_second_pairs_fade_starts_cleanly(orc, bfir):
    _, L, B, s, n_in, n_out, _, _ = CASES[SMALL]
    S, (pairs2, filters2) = _small(orc)
    x, t0, nb = S["x"], S["t0"], S["nb"]
    K1, K2, t1 = 3, 5, t0 + 4
    final = merge(S["merged"], pairs2, filters2)
    e, twin = _start(bfir, SMALL, S), _start(bfir, SMALL, S)
    ys = []
    for g in (e, twin):
        assert g.run(x[:t0 * L])[0] == 0
    assert e.set_coeff_pairs_fade(S["pairs"], S["filters"], K1, coeff_blocks=S["cb"]) == 0
    assert twin.set_coeff_fade(_padded(S["merged"], B * L), K1) == 0
    for g in (e, twin):
        assert g.run(x[t0 * L:t1 * L])[0] == 0 and g.fade_remaining() == 0
    assert e.set_coeff_pairs_fade(pairs2, filters2, K2) == 0 and e.fade_remaining() == K2
    assert twin.set_coeff_fade(_padded(final, B * L), K2) == 0
    for g in (e, twin):
        rc, y = g.run(x[t1 * L:])
        assert rc == 0 and g.fade_remaining() == 0
        ys.append(y)
    assert ys[0][K2 * L:].tobytes() == ys[1][K2 * L:].tobytes()
    w = fade_weights(L, nb, t1, K2)[:, None]
    want = _ref64(orc, S["merged"], x) * (1.0 - w) + _ref64(orc, final, x) * w
    assert _worst(ys[0], want[t1 * L:], L) <= TOL[s]
    assert _same_store(_all_blocks(e, SMALL), _all_blocks(twin, SMALL))
    e.close(); twin.close()


# ---- 7. errors -------------------------------------------------------------------------------------------------------------------
def _raw(lib, e, fade, n, outs, ins, ptrs, length, cb, K=2):
    f = lib.bfir_engine_set_coeff_matrix_pairs_fade if fade else lib.bfir_engine_set_coeff_matrix_pairs
    return f(e.handle, n, outs, ins, ptrs, length, cb, 1.0, *((K,) if fade else ()))


def test_refusals_change_nothing(orc, bfir):
    _, L, B, s, n_in, n_out, _, _ = CASES[SMALL]
    S, (pairs2, filters2) = _small(orc)
    x, t0 = S["x"], S["t0"]
    lib = bfir.load()
    h = np.ascontiguousarray(S["filters"][0])
    bad = h.copy(); bad[L + 1] = np.nan
    inf = h.copy(); inf[0] = np.inf

    def ints(*v):
        return (C.c_int * len(v))(*v)

    def ptrs(*a):
        return (C.c_void_p * len(a))(*[None if v is None else v.ctypes.data for v in a])
    e, twin = _start(bfir, SMALL, S), _start(bfir, SMALL, S)
    fresh = getattr(bfir, CASES[SMALL][0])(L, B, s, n_in, n_out)
    for fade in (False, True):
        assert _raw(lib, fresh, fade, 1, ints(0), ints(0), ptrs(h), h.size, B) == bfir.ERR_STATE      # no coefficients yet
        assert not fresh.is_initialized()
    fresh.close()
    assert e.run(x[:t0 * L])[0] == 0 and twin.run(x[:t0 * L])[0] == 0
    state = _all_blocks(e, SMALL)
    for fade in (False, True):
        A = bfir.ERR_ARG
        assert _raw(lib, e, fade, 1, None, ints(0), ptrs(h), h.size, B) == A
        assert _raw(lib, e, fade, 1, ints(0), None, ptrs(h), h.size, B) == A
        assert _raw(lib, e, fade, 1, ints(0), ints(0), None, h.size, B) == A
        assert _raw(lib, e, fade, 0, ints(0), ints(0), ptrs(h), h.size, B) == A
        assert _raw(lib, e, fade, -1, ints(0), ints(0), ptrs(h), h.size, B) == A
        for o, i in ((n_out, 0), (-1, 0), (0, n_in), (0, -1)):
            assert _raw(lib, e, fade, 1, ints(o), ints(i), ptrs(h), h.size, B) == A, (o, i)
        assert _raw(lib, e, fade, 2, ints(1, 1), ints(2, 2), ptrs(h, None), h.size, B) == A            # the same pair twice
        assert _raw(lib, e, fade, 1, ints(0), ints(0), ptrs(h), -1, B) == A
        assert _raw(lib, e, fade, 1, ints(0), ints(0), ptrs(h), h.size, 0) == A
        for v in (bad, inf):
            assert _raw(lib, e, fade, 2, ints(1, 0), ints(0, 1), ptrs(h, v), h.size, B) == bfir.ERR_COEFF
        assert e.is_initialized() and e.fade_remaining() == 0 and _same_store(_all_blocks(e, SMALL), state)
    for K in (0, -3, (1 << 24) // L + 1):
        assert _raw(lib, e, True, 1, ints(0), ints(0), ptrs(h), h.size, B, K) == bfir.ERR_ARG
    assert e.fade_remaining() == 0 and _same_store(_all_blocks(e, SMALL), state)
    (rc, y), (rct, yt) = e.run(x[t0 * L:(t0 + 3) * L]), twin.run(x[t0 * L:(t0 + 3) * L])
    assert rc == rct == 0 and y.tobytes() == yt.tobytes()
    # a fade pending or running: the fade call is refused, the fade goes on; a NaN on the plain call leaves it running too
    for g in (e, twin):
        assert g.set_coeff_pairs_fade(S["pairs"], S["filters"], 4) == 0
    assert e.set_coeff_pairs_fade(pairs2, filters2, 2) == bfir.ERR_STATE and e.fade_remaining() == 4
    (rc, y), (rct, yt) = e.run(x[(t0 + 3) * L:(t0 + 4) * L]), twin.run(x[(t0 + 3) * L:(t0 + 4) * L])
    assert rc == rct == 0 and y.tobytes() == yt.tobytes()
    assert e.set_coeff_pairs_fade(pairs2, filters2, 2) == bfir.ERR_STATE and e.fade_remaining() == 3
    assert e.set_coeff_pairs([(0, 0)], [bad]) == bfir.ERR_COEFF and e.fade_remaining() == 3 and e.is_initialized()
    (rc, y), (rct, yt) = e.run(x[(t0 + 4) * L:]), twin.run(x[(t0 + 4) * L:])
    assert rc == rct == 0 and y.tobytes() == yt.tobytes() and e.fade_remaining() == 0
    e.close(); twin.close()


def test_other_kinds_are_unsupported(bfir):
    L, B, blocks, ratios = 512, 2, (5, 3, 2), (1, 4, 2)
    lib = bfir.load()
    h = np.zeros(L, np.float32); h[0] = 1.0
    one, p = (C.c_int * 1)(0), (C.c_void_p * 1)(h.ctypes.data)
    engines = [bfir.Brutefir(L, B, 4, 2), bfir.Brutefir(L, B, 4, 2, n_engines=2), bfir.BrutefirLevels(L, blocks, ratios, 4, 2),
               bfir.BrutefirMatrixLevels(L, blocks, ratios, 4, 2, 2), bfir.BrutefirMimoLevels(L, blocks, ratios, 4, 2, 2)]
    for e in engines:
        for fade in (False, True):
            assert _raw(lib, e, fade, 1, one, one, p, L, 1) == bfir.ERR_UNSUPPORTED, (type(e).__name__, fade)
        assert not e.is_initialized()
        e.close()


# ---- 8. the C++ mirror -----------------------------------------------------------------------------------------------------------
def test_cpp_mirror_patches_and_fades(tmp_path, bfir):
    """tests/cpp/test_pairs_mirror.cpp through the brutefir class, and its sequence again through ctypes: the same bytes."""
    src = os.path.join(ROOT, "tests", "cpp", "test_pairs_mirror.cpp")
    exe = str(tmp_path / "test_pairs_mirror")
    libdir = os.path.dirname(bfir.library_path())
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", src, "-o", exe, "-L" + libdir, "-lbfir_hip",
                    "-Wl,-rpath," + libdir], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "ALL OK" in p.stdout
    m = re.search(r"^checksum ([0-9a-f]{16})$", p.stdout, re.M)
    assert m, p.stdout
    L, B, NC, taps, nb = 256, 2, 10, 356, 11
    i = np.arange(nb * L * NC, dtype=np.uint64)
    x = ((((i * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(8)).astype(np.float64) / 16777216.0 - 0.5).astype(np.float32)
    x = x.reshape(nb * L, NC)

    def filt(f):
        k = (np.arange(1, taps + 1, dtype=np.uint64) * np.uint64(40503 * (f + 3))) & np.uint64(0xffff)
        return ((k.astype(np.float64) / 65536.0 - 0.5) / 64.0).astype(np.float32)
    e = bfir.BrutefirMimo(L, B, 4, NC, NC)
    assert e.set_coeff([[filt(o * NC + i_) for i_ in range(NC)] for o in range(NC)], coeff_blocks=B) == 0
    ys = [e.run(x[:3 * L])[1]]
    assert e.set_coeff_pairs([(o, 4) for o in range(NC)], [filt(200 + o) for o in range(NC)]) == 0
    ys.append(e.run(x[3 * L:5 * L])[1])
    assert e.set_coeff_pairs_fade([(0, 1), (7, 1), (3, 1)], [filt(300), filt(307), None], 3, length=taps) == 0
    ys.append(e.run(x[5 * L:6 * L])[1])
    ys.append(e.run(x[6 * L:])[1])
    e.close()
    fnv = 1469598103934665603
    for byte in np.concatenate(ys).tobytes():
        fnv = ((fnv ^ byte) * 1099511628211) & 0xffffffffffffffff
    assert "%016x" % fnv == m.group(1)
