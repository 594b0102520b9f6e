"""Coefficient banks on the GPU (bfir_engine_bank_*, bfir_engine_set_coeff_matrix_bank, _bank_fade, _pairs_bank,
_pairs_bank_fade; k_bank_gather in csrc/bank.hip) against twin engines that get the same filters as host taps through the
calls that were there before: set_coeff, set_coeff_fade, set_coeff_pairs, set_coeff_pairs_fade.

A bank entry loaded with coeff_blocks = c and scale g holds what those calls write for the same taps, c and g, and a gathered
row is the entry's first c partitions with zeros behind them -- the row load_filters writes.  So every comparison with a
twin is of BYTES: bank_read against coeff_block, the filter stores, and every output block.  Where one call names entries of
different counts no single call with taps does the same: the plain calls are compared with a twin patched once per distinct
count (bytes), the fades with the float64 blend of two float64 direct convolutions at conftest.TOL -- the only tolerance
in this file.

The shapes are chosen around SPAN, the bytes one workgroup of k_bank_gather moves per step (256 lanes x 16 bytes; a
workgroup makes STEPS = 4 such steps, a row of B partitions of 2 L reals is B * 2 L * realsize bytes):
  below     L = 16,   B = 1    a row of 128 / 256 bytes, far below one span
  boundary  L = 16,   B = 40   5120 / 10240 bytes: a span holds whole partitions (32 / 16 of them), and with counts 33 and 39
                               the boundary between the copied and the zeroed part falls inside a span
  partial   L = 256,  B = 5    10240 / 20480 bytes: whole spans and half a span (fp32), one workgroup and a quarter (fp64)
  multiple  L = 1024, B = 4    32768 / 65536 bytes: a whole number of spans and of workgroups, more than one workgroup per row
on a BrutefirMatrix 2 -> 3 and a BrutefirMimo 9 -> 5 (k_mac_mimo), fp32 and fp64; L = 16 is the grouped spectrum layout in
both precisions, L >= 256 the (re, im) layout in fp32.  The bank holds, per count in {1, B - 1, B} (B = 40: 33 and 39 too),
three filters loaded in one call of their own scale, then an entry loaded as None and one never loaded."""
import ctypes as C

import numpy as np
import pytest

from conftest import TOL
from size_matrix import flat_ir
from test_fade import fade_weights
from test_mimo_gpu import _frames, _padded, _ref64, _rows, _run_cut, _worst
from test_pairs import merge

pytestmark = pytest.mark.gpu

F32, F64 = 8, 10
SPAN, STEPS = 4096, 4            # BFIR_BANK_SPAN, BFIR_BANK_STEPS (csrc/kernels.h)
SIZES = {"below": (16, 1), "boundary": (16, 40), "partial": (256, 5), "multiple": (1024, 4)}
_SHAPES = dict(SIZES, refusals=(16, 3))      # ... and the small shape of the refusal test
KINDS = {"matrix": ("BrutefirMatrix", 2, 3), "mimo": ("BrutefirMimo", 9, 5)}
CASES = [(k, z, s) for k in sorted(KINDS) for z in sorted(SIZES) for s in (4, 8)]
IDS = ["%s-%s-f%d" % (k, z, 8 * s) for k, z, s in CASES]
CUTS = (1, 3, 2)                 # blocks per call behind a change
PRE = 3                          # blocks before the first change
PER = 3                          # entries per count


def test_the_shapes_lie_where_the_docstring_says():
    for s in (4, 8):
        row = {z: B * 2 * L * s for z, (L, B) in SIZES.items()}
        assert row["below"] < SPAN // 8
        assert SPAN < row["boundary"] and SPAN % (2 * 16 * s) == 0           # a span holds whole partitions ...
        for c in (33, 39):
            assert (c * 2 * 16 * s) % SPAN and c * 2 * 16 * s > SPAN          # ... and the boundary lies inside a later one
        assert row["partial"] > SPAN and row["partial"] % SPAN == (SPAN // 2 if s == 4 else 0) and row["partial"] % (STEPS * SPAN)
        assert row["multiple"] % (STEPS * SPAN) == 0 and row["multiple"] >= 2 * STEPS * SPAN


def _dt(s):
    return np.float64 if s == 8 else np.float32


def _fmt(s):
    return F32 if s == 4 else F64


def _counts(B):
    return sorted({1, max(1, B - 1), B} | ({33, 39} if B == 40 else set()))


class _Bank:
    """The filters of one (L, B, realsize): filters[c][j], j < PER, of B L taps with a ragged end, loaded with coeff_blocks = c
    and scale[c] into entry index[c][j]; `empty` is loaded as None, `never` is not loaded.  Nothing here is written to."""

    def __init__(self, L, B, s):
        rng = np.random.default_rng(1000 * L + 10 * B + s)
        self.L, self.B, self.s = L, B, s
        self.counts = _counts(B)
        self.filters, self.scale, self.index = {}, {}, {}
        for n, c in enumerate(self.counts):
            fs = []
            for j in range(PER):
                h = np.zeros(B * L, _dt(s))
                taps = B * L - 1 - 2 * j - n
                h[:taps] = flat_ir(rng, 1, taps)[0]
                h.setflags(write=False)
                fs.append(h)
            self.filters[c], self.scale[c], self.index[c] = fs, (1.0, 0.5, 2.0)[n % 3], [PER * n + j for j in range(PER)]
        self.empty, self.never = PER * len(self.counts), PER * len(self.counts) + 1
        self.n = self.never + 1
        self.count_of = {en: c for c in self.counts for en in self.index[c]}

    def taps(self, entry):
        """(the taps, coeff_blocks, scale) an entry was loaded with; (None, B, 1.0) for None = no path."""
        if entry is None:
            return None, self.B, 1.0
        c = self.count_of[entry]
        return self.filters[c][self.index[c].index(entry)], c, self.scale[c]

    def loaded(self, entry):
        """The filter an entry stands for, as the float64 reference takes it: cut to its partitions and scaled."""
        h, c, g = self.taps(entry)
        return None if h is None else (h[:c * self.L] * _dt(self.s)(g))

    def load(self, e):
        assert e.bank_create(self.n) == 0 and e.bank_entries() == self.n
        for c in self.counts:
            assert e.bank_load(self.index[c][0], self.filters[c], coeff_blocks=c, scale=self.scale[c]) == 0
        assert e.bank_load(self.empty, [None]) == 0
        for c in self.counts:
            assert [e.bank_blocks(en) for en in self.index[c]] == [c] * PER
        assert e.bank_blocks(self.empty) == 0 and e.bank_blocks(self.never) == 0


_banks, _olds, _xs = {}, {}, {}


def _bank(L, B, s):
    if (L, B, s) not in _banks:
        _banks[(L, B, s)] = _Bank(L, B, s)
    return _banks[(L, B, s)]


def _old_rows(kind, size, s):
    """The first set: ragged filters of 1 .. B partitions, pair (0, n_in - 1) without a path; every input read."""
    if (kind, size, s) not in _olds:
        (_, n_in, n_out), (L, B) = KINDS[kind], _SHAPES[size]
        rng = np.random.default_rng(7 * len(kind) + 13 * L + B + s)
        _olds[(kind, size, s)] = _rows(rng, L, n_in, n_out, s, lambda o, i: 0 if (o, i) == (0, n_in - 1) else 1 + (o + i) % B)
    return _olds[(kind, size, s)]


def _x(kind, size, s, nb):
    if (kind, size, s, nb) not in _xs:
        x = _frames(np.random.default_rng(nb + len(kind) + _SHAPES[size][0]), nb, _SHAPES[size][0], KINDS[kind][1], _fmt(s))
        x.setflags(write=False)
        _xs[(kind, size, s, nb)] = x
    return _xs[(kind, size, s, nb)]


def _new(bfir, kind, size, s, chunk=None):
    (cls, n_in, n_out), (L, B) = KINDS[kind], _SHAPES[size]
    e = getattr(bfir, cls)(L, B, s, n_in, n_out)
    if chunk is not None:
        e.set_chunk(chunk)
    return e


def _started(bfir, kind, size, s, chunk=None, bank=True):
    """An engine on the first set (loaded from taps); with the bank loaded, or a twin without one."""
    e = _new(bfir, kind, size, s, chunk)
    if bank:
        _bank(*_SHAPES[size], s).load(e)
    assert e.set_coeff(_padded(_old_rows(kind, size, s), _SHAPES[size][1] * _SHAPES[size][0])) == 0
    return e


def _store(e):
    return b"".join(e.coeff_block(o, i, b).tobytes() for o in range(e.n_out) for i in range(e.n_in) for b in range(e.B))


def _both(e, twin, x, L, cuts):
    (rcs, y), (rct, yt) = _run_cut(e, x, L, cuts), _run_cut(twin, x, L, cuts)
    assert rcs == rct == [0] * len(cuts)
    assert y.tobytes() == yt.tobytes()
    return y


def _pair_list(bk, n_in, n_out, entries):
    """The list of the pairs tests: column n_in - 1 (its pair (0, n_in - 1) had no path: added), then (n_out - 1, 0) removed.
    The column's entries cycle through `entries`, so one entry serves several pairs."""
    pairs = [(o, n_in - 1) for o in range(n_out)] + [(n_out - 1, 0)]
    ents = [entries[o % len(entries)] for o in range(n_out)] + [None]
    assert len(set(ents[:-1])) < n_out
    return pairs, ents


def _twin_pairs(twin, bk, pairs, ents, fade=None):
    """The same change on a twin, from taps: one call per distinct (coeff_blocks, scale) among the entries, the removed
    paths in a call of their own; with `fade` there must be one group."""
    groups = {}
    for p, en in zip(pairs, ents):
        h, c, g = bk.taps(en)
        groups.setdefault((c, g, h is None), []).append((p, h))
    assert fade is None or len({k[:2] for k in groups if not k[2]}) == 1
    if fade is not None:
        (c, g) = next(k[:2] for k in groups if not k[2])
        return twin.set_coeff_pairs_fade(pairs, [bk.taps(en)[0] for en in ents], fade, length=bk.B * bk.L, coeff_blocks=c, scale=g)
    for (c, g, _), lst in sorted(groups.items(), key=lambda kv: kv[0]):
        assert twin.set_coeff_pairs([p for p, _ in lst], [h for _, h in lst], length=bk.B * bk.L, coeff_blocks=c, scale=g) == 0
    return 0


# ---- 1. the entries ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,size,s", CASES, ids=IDS)
def test_bank_entries_are_the_twins_spectra(bfir, kind, size, s):
    (_, n_in, n_out), (L, B) = KINDS[kind], SIZES[size]
    bk = _bank(L, B, s)
    e, twin = _new(bfir, kind, size, s), _new(bfir, kind, size, s)
    bk.load(e)
    assert not e.is_initialized()
    zeros = np.zeros(2 * L, _dt(s)).tobytes()
    for c in bk.counts:
        for j0 in range(0, PER, n_out * n_in):
            ents = bk.index[c][j0:j0 + n_out * n_in]
            flat = [bk.filters[c][bk.index[c].index(en)] for en in ents] + [None] * (n_out * n_in - len(ents))
            rows = [flat[o * n_in:(o + 1) * n_in] for o in range(n_out)]
            assert twin.set_coeff(rows, coeff_blocks=c, scale=bk.scale[c]) == 0
            for n, en in enumerate(ents):
                for b in range(B):
                    got = e.bank_read(en, b).tobytes()
                    assert got == twin.coeff_block(n // n_in, n % n_in, b).tobytes(), (c, en, b)
                    assert (got == zeros) == (b >= c), (c, en, b)
    for en in (bk.empty, bk.never):
        assert all(e.bank_read(en, b).tobytes() == zeros for b in range(B))
    e.close(); twin.close()


# ---- 2. plain pairs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,size,s", CASES, ids=IDS)
def test_plain_pairs_from_the_bank(bfir, kind, size, s):
    (_, n_in, n_out), (L, B) = KINDS[kind], SIZES[size]
    bk = _bank(L, B, s)
    nb = PRE + len(bk.counts) * sum(CUTS) + sum(CUTS)
    x = _x(kind, size, s, nb)
    for chunk in (0, 2):
        e, twin = _started(bfir, kind, size, s, chunk), _started(bfir, kind, size, s, chunk, bank=False)
        assert _store(e) == _store(twin)
        _both(e, twin, x[:PRE * L], L, (PRE,))
        t = PRE
        for c in bk.counts:
            pairs, ents = _pair_list(bk, n_in, n_out, bk.index[c][:2])
            assert e.set_coeff_pairs_bank(pairs, ents) == 0
            assert _twin_pairs(twin, bk, pairs, ents) == 0
            assert e.is_initialized() and e.fade_remaining() == 0
            assert _store(e) == _store(twin), c
            _both(e, twin, x[t * L:(t + sum(CUTS)) * L], L, CUTS)
            t += sum(CUTS)
        # the engine's rows are copies: other filters over the entries it was given change nothing in it
        before = _store(e)
        c = bk.counts[-1]
        assert e.bank_load(bk.index[c][0], bk.filters[bk.counts[0]][::-1], coeff_blocks=1, scale=3.0) == 0
        assert e.bank_blocks(bk.index[c][0]) == 1
        assert _store(e) == before
        _both(e, twin, x[t * L:], L, CUTS)
        assert e.bank_destroy() == 0 and e.bank_entries() == 0 and _store(e) == before
        e.close(); twin.close()


# ---- 3. fading pairs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,size,s", CASES, ids=IDS)
def test_fading_pairs_from_the_bank(bfir, kind, size, s):
    (_, n_in, n_out), (L, B) = KINDS[kind], SIZES[size]
    bk = _bank(L, B, s)
    c, K = max(1, B - 1), 3
    nb = PRE + 1 + K + 2
    x = _x(kind, size, s, nb)
    pairs, ents = _pair_list(bk, n_in, n_out, bk.index[c][1:])
    for how in ("through", "cancelled", "reset"):
        e, twin = _started(bfir, kind, size, s), _started(bfir, kind, size, s, bank=False)
        _both(e, twin, x[:PRE * L], L, (PRE,))
        before = _store(e)
        assert e.set_coeff_pairs_bank_fade(pairs, ents, K) == 0
        assert _twin_pairs(twin, bk, pairs, ents, fade=K) == 0
        assert e.fade_remaining() == twin.fade_remaining() == K
        assert _store(e) == before                                   # the old set is read until the last fading block is queued
        _both(e, twin, x[PRE * L:(PRE + 1) * L], L, (1,))
        assert e.fade_remaining() == twin.fade_remaining() == K - 1
        if how == "cancelled":   # a plain call during the fade: a hard cut, the old set patched
            assert e.set_coeff_pairs_bank([(0, 0)], [bk.index[c][0]]) == 0
            assert _twin_pairs(twin, bk, [(0, 0)], [bk.index[c][0]]) == 0
            assert e.fade_remaining() == twin.fade_remaining() == 0
        elif how == "reset":
            e.reset(); twin.reset()
            assert e.fade_remaining() == twin.fade_remaining() == 0
        if how == "through":
            _both(e, twin, x[(PRE + 1) * L:(PRE + 2) * L], L, (1,))
            assert e.fade_remaining() == twin.fade_remaining() == K - 2
            _both(e, twin, x[(PRE + 2) * L:], L, (nb - PRE - 2,))
        else:
            _both(e, twin, x[(PRE + 1) * L:], L, (2, nb - PRE - 3))
        assert e.fade_remaining() == twin.fade_remaining() == 0
        assert _store(e) == _store(twin)
        e.close(); twin.close()


# ---- 4. the whole matrix -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,size,s", CASES, ids=IDS)
def test_whole_matrix_from_the_bank(bfir, kind, size, s):
    (_, n_in, n_out), (L, B) = KINDS[kind], SIZES[size]
    bk = _bank(L, B, s)
    K = 2
    nb = PRE + K + 3
    x = _x(kind, size, s, nb)
    for c in sorted({bk.counts[0], bk.counts[-1]}):
        idx = bk.index[c]
        first = [[None if (o, i) == (1, 0) else idx[(o + 2 * i) % PER] for i in range(n_in)] for o in range(n_out)]
        second = [[None if (o, i) == (0, 0) else idx[(2 * o + i + 1) % PER] for i in range(n_in)] for o in range(n_out)]
        e, twin = _new(bfir, kind, size, s), _new(bfir, kind, size, s)
        bk.load(e)
        assert e.set_coeff_bank_fade(first, K) == bfir.ERR_STATE     # nothing to fade from
        assert e.set_coeff_bank(first) == 0
        assert e.is_initialized()                                    # from the bank alone
        assert twin.set_coeff([[bk.taps(en)[0] for en in r] for r in first], coeff_blocks=c, scale=bk.scale[c]) == 0
        assert _store(e) == _store(twin)
        _both(e, twin, x[:PRE * L], L, (1, PRE - 1))
        assert e.set_coeff_bank_fade(second, K) == 0
        assert twin.set_coeff_fade([[bk.taps(en)[0] for en in r] for r in second], K, coeff_blocks=c, scale=bk.scale[c]) == 0
        assert e.fade_remaining() == twin.fade_remaining() == K
        _both(e, twin, x[PRE * L:(PRE + 1) * L], L, (1,))
        assert e.fade_remaining() == twin.fade_remaining() == K - 1
        _both(e, twin, x[(PRE + 1) * L:], L, (nb - PRE - 1,))
        assert e.fade_remaining() == twin.fade_remaining() == 0 and _store(e) == _store(twin)
        # during a fade the plain call cancels it
        assert e.set_coeff_bank_fade(first, K) == 0 and twin.set_coeff_fade([[bk.taps(en)[0] for en in r] for r in first], K, coeff_blocks=c, scale=bk.scale[c]) == 0
        assert e.set_coeff_bank(second) == 0
        assert twin.set_coeff([[bk.taps(en)[0] for en in r] for r in second], coeff_blocks=c, scale=bk.scale[c]) == 0
        assert e.fade_remaining() == twin.fade_remaining() == 0 and _store(e) == _store(twin)
        _both(e, twin, x[:2 * L], L, (2,))
        e.close(); twin.close()


# ---- 5. entries of different counts in one call --------------------------------------------------------------------------------
def _mixed_rows(bk, n_in, n_out):
    """rows[o][i]: an entry of every count in turn, (1, 0) without a path."""
    ents = [en for j in range(PER) for c in bk.counts for en in (bk.index[c][j],)]
    return [[None if (o, i) == (1, 0) else ents[(o * n_in + i) % len(ents)] for i in range(n_in)] for o in range(n_out)]


@pytest.mark.parametrize("kind,size,s", CASES, ids=IDS)
def test_mixed_counts_plain(bfir, kind, size, s):
    (_, n_in, n_out), (L, B) = KINDS[kind], SIZES[size]
    bk = _bank(L, B, s)
    nb = PRE + 2 * sum(CUTS)
    x = _x(kind, size, s, nb)
    every = [(o, i) for o in range(n_out) for i in range(n_in)]
    rows = _mixed_rows(bk, n_in, n_out)
    # a pair list of all counts on a running engine
    e, twin = _started(bfir, kind, size, s), _started(bfir, kind, size, s, bank=False)
    _both(e, twin, x[:PRE * L], L, (PRE,))
    pairs = every[1::2] if len(every) > 8 else every[1:]
    ents = [rows[o][i] for o, i in pairs]
    assert e.set_coeff_pairs_bank(pairs, ents) == 0 and _twin_pairs(twin, bk, pairs, ents) == 0
    assert _store(e) == _store(twin)
    _both(e, twin, x[PRE * L:(PRE + sum(CUTS)) * L], L, CUTS)
    e.close(); twin.close()
    # the whole matrix on an engine that has had no filters: the twin's pairs, all of them, patched over its first set
    e, twin = _new(bfir, kind, size, s), _started(bfir, kind, size, s, bank=False)
    bk.load(e)
    assert e.set_coeff_bank(rows) == 0 and e.is_initialized()
    assert _twin_pairs(twin, bk, every, [rows[o][i] for o, i in every]) == 0
    assert _store(e) == _store(twin)
    _both(e, twin, x[(PRE + sum(CUTS)) * L:], L, CUTS)
    e.close(); twin.close()


@pytest.mark.parametrize("whole", (False, True), ids=("pairs", "whole"))
@pytest.mark.parametrize("kind,size,s", CASES, ids=IDS)
def test_mixed_counts_fade(orc, bfir, kind, size, s, whole):
    """Against the float64 blend of the float64 direct convolutions with the old and with the new set (every filter cut to its
    entry's partitions and scaled as loaded), per block and output at conftest.TOL."""
    (_, n_in, n_out), (L, B) = KINDS[kind], SIZES[size]
    bk = _bank(L, B, s)
    K = 3
    nb = PRE + K + 2
    x = _x(kind, size, s, nb)
    old = _old_rows(kind, size, s)
    rows = _mixed_rows(bk, n_in, n_out)
    every = [(o, i) for o in range(n_out) for i in range(n_in)]
    pairs = every if whole else (every[1::2] if len(every) > 8 else every[1:])
    ents = [rows[o][i] for o, i in pairs]
    new = merge(old, pairs, [bk.loaded(en) for en in ents])
    e = _started(bfir, kind, size, s)
    rc0, y0 = e.run(x[:PRE * L])
    assert (e.set_coeff_bank_fade(rows, K) if whole else e.set_coeff_pairs_bank_fade(pairs, ents, K)) == 0
    assert e.fade_remaining() == K
    rcs, y1 = _run_cut(e, x[PRE * L:], L, (1, nb - PRE - 1))
    assert rc0 == 0 and rcs == [0, 0] and e.fade_remaining() == 0
    zeros = np.zeros(2 * L, _dt(s)).tobytes()
    for (o, i), en in zip(pairs, ents):   # the new set is active, every listed filter at its own count
        assert all(e.coeff_block(o, i, b).tobytes() == (zeros if en is None else e.bank_read(en, b).tobytes()) for b in range(B))
    y = np.concatenate([y0, y1])
    w = fade_weights(L, nb, PRE, K)[:, None]
    want = _ref64(orc, old, x) * (1.0 - w) + _ref64(orc, new, x) * w
    err = _worst(y, want, L)
    print("%s %s f%d %s: worst block %.3g against the float64 blend" % (kind, size, 8 * s, "whole" if whole else "pairs", err))
    assert err <= TOL[s]
    e.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(bfir):
    """Every ARG and STATE refusal on a matrix engine; after each the next block's bytes are the twin's."""
    kind, s = "matrix", 4
    L, B = _SHAPES["refusals"]
    (_, n_in, n_out) = KINDS[kind]
    bk = _bank(L, B, s)
    lib = bfir.load()
    x = _x(kind, "refusals", s, 80)
    e, twin = _new(bfir, kind, "refusals", s), _started(bfir, kind, "refusals", s, bank=False)
    state = {"t": 0}
    ARG, STATE = bfir.ERR_ARG, bfir.ERR_STATE
    full = [[0] * n_in for _ in range(n_out)]

    def ints(*v):
        return (C.c_int * len(v))(*v)

    def refused(rc, want):
        assert rc == want, (rc, want)
        if e.is_initialized():
            t = state["t"]
            _both(e, twin, x[t * L:(t + 1) * L], L, (1,))
            state["t"] = t + 1

    # no bank
    assert e.bank_entries() == 0 and e.bank_destroy() == 0 and e.bank_blocks(0) == ARG
    for rc in (e.set_coeff_bank(full), e.set_coeff_bank_fade(full, 2), e.set_coeff_pairs_bank([(0, 0)], [0]),
               e.set_coeff_pairs_bank_fade([(0, 0)], [0], 2), e.bank_load(0, [bk.filters[1][0]])):
        refused(rc, STATE)
    with pytest.raises(bfir.BfirError) as ei:
        e.bank_read(0, 0)
    assert ei.value.code == STATE
    refused(e.bank_create(0), ARG)
    refused(e.bank_create(-3), ARG)
    bk.load(e)
    refused(e.bank_create(4), STATE)
    assert e.bank_entries() == bk.n
    # an engine without coefficients
    good = [[bk.index[B][0]] * n_in for _ in range(n_out)]
    refused(e.set_coeff_pairs_bank([(0, 0)], [bk.index[1][0]]), STATE)
    refused(e.set_coeff_pairs_bank_fade([(0, 0)], [bk.index[1][0]], 2), STATE)
    refused(e.set_coeff_bank_fade(good, 2), STATE)
    assert not e.is_initialized()
    assert e.set_coeff(_padded(_old_rows(kind, "refusals", s), B * L)) == 0
    _both(e, twin, x[:L], L, (1,))
    state["t"] = 1
    h = e._h
    one, ok = ints(0), ints(bk.index[1][0])
    # null pointers and counts
    refused(lib.bfir_engine_set_coeff_matrix_bank(h, None), ARG)
    refused(lib.bfir_engine_set_coeff_matrix_bank_fade(h, None, 2), ARG)
    for f, tail in ((lib.bfir_engine_set_coeff_matrix_pairs_bank, ()), (lib.bfir_engine_set_coeff_matrix_pairs_bank_fade, (2,))):
        refused(f(h, 1, None, one, ok, *tail), ARG)
        refused(f(h, 1, one, None, ok, *tail), ARG)
        refused(f(h, 1, one, one, None, *tail), ARG)
        refused(f(h, 0, one, one, ok, *tail), ARG)
        refused(f(h, -1, one, one, ok, *tail), ARG)
        refused(f(h, 1, ints(n_out), one, ok, *tail), ARG)            # a pair outside the matrix
        refused(f(h, 1, one, ints(n_in), ok, *tail), ARG)
        refused(f(h, 1, ints(-1), one, ok, *tail), ARG)
        refused(f(h, 2, ints(1, 1), ints(0, 0), ints(ok[0], ok[0]), *tail), ARG)   # the same pair twice
        refused(f(h, 1, one, one, ints(bk.n), *tail), ARG)            # an index outside -1 .. n_entries - 1
        refused(f(h, 1, one, one, ints(-2), *tail), ARG)
        refused(f(h, 1, one, one, ints(bk.empty), *tail), STATE)      # an empty entry: loaded as None, and never loaded
        refused(f(h, 1, one, one, ints(bk.never), *tail), STATE)
    for bad, want in ((bk.n, ARG), (-2, ARG), (bk.empty, STATE), (bk.never, STATE)):
        rows = [list(r) for r in good]
        rows[n_out - 1][n_in - 1] = bad
        refused(e.set_coeff_bank(rows), want)
        refused(e.set_coeff_bank_fade(rows, 2), want)
    assert e.is_initialized()
    # fade arguments, and one fade at a time
    for K in (0, -1, (1 << 24) // L + 1):
        refused(e.set_coeff_bank_fade(good, K), ARG)
        refused(e.set_coeff_pairs_bank_fade([(0, 0)], [ok[0]], K), ARG)
    assert e.set_coeff_pairs_bank_fade([(0, 0)], [bk.index[B][1]], 40) == 0
    assert twin.set_coeff_pairs_fade([(0, 0)], [bk.taps(bk.index[B][1])[0]], 40, coeff_blocks=B, scale=bk.scale[B]) == 0
    refused(e.set_coeff_pairs_bank_fade([(1, 0)], [ok[0]], 2), STATE)
    refused(e.set_coeff_bank_fade(good, 2), STATE)
    assert e.fade_remaining() == twin.fade_remaining() > 0
    # bank_load and bank_read
    f0 = bk.filters[1][0]
    p1 = (C.c_void_p * 1)(f0.ctypes.data)
    refused(lib.bfir_engine_bank_load(h, 0, 1, None, L, 1, 1.0), ARG)
    refused(lib.bfir_engine_bank_load(h, 0, 0, p1, L, 1, 1.0), ARG)
    refused(lib.bfir_engine_bank_load(h, -1, 1, p1, L, 1, 1.0), ARG)
    refused(lib.bfir_engine_bank_load(h, bk.n, 1, p1, L, 1, 1.0), ARG)
    refused(e.bank_load(bk.n - 1, [f0, f0]), ARG)
    refused(lib.bfir_engine_bank_load(h, 0, 1, p1, -1, 1, 1.0), ARG)
    refused(lib.bfir_engine_bank_load(h, 0, 1, p1, L, 0, 1.0), ARG)
    nan = np.array(f0); nan[L + 1] = np.nan
    was = [e.bank_read(en, b).tobytes() for en in range(3) for b in range(B)]
    refused(e.bank_load(0, [f0, nan, f0], coeff_blocks=2), bfir.ERR_COEFF)   # the bank is unchanged, the first row included
    assert [e.bank_read(en, b).tobytes() for en in range(3) for b in range(B)] == was
    assert [e.bank_blocks(en) for en in range(3)] == [bk.count_of[en] for en in range(3)]
    assert e.bank_load(0, [f0, nan, f0], coeff_blocks=1) == 0         # the NaN lies behind what one partition loads
    dst = np.zeros(2 * L, np.float32)
    for en, b, d in ((bk.n, 0, dst.ctypes.data), (-1, 0, dst.ctypes.data), (0, B, dst.ctypes.data), (0, -1, dst.ctypes.data), (0, 0, None)):
        refused(lib.bfir_engine_bank_read(h, en, b, d), ARG)
    refused(e.bank_blocks(bk.n), ARG)
    refused(e.bank_blocks(-1), ARG)
    assert state["t"] >= 50                                           # the refusals above were each followed by a block
    e.close(); twin.close()


def test_other_kinds_are_unsupported(bfir):
    L, B, blocks, ratios = 512, 2, (5, 3, 2), (1, 4, 2)
    lib = bfir.load()
    hh = np.zeros(L, np.float32); hh[0] = 1.0
    one, p = (C.c_int * 1)(0), (C.c_void_p * 1)(hh.ctypes.data)
    dst = np.zeros(2 * L, np.float32)
    U = bfir.ERR_UNSUPPORTED
    engines = [bfir.Brutefir(L, B, 4, 2), bfir.Brutefir(L, B, 4, 2, n_engines=2), bfir.BrutefirNup(L, 4, 4, 2, 4, 2),
               bfir.BrutefirLevels(L, blocks, ratios, 4, 2), bfir.BrutefirMatrixLevels(L, blocks, ratios, 4, 2, 2),
               bfir.BrutefirMimoLevels(L, blocks, ratios, 4, 2, 2)]
    for e in engines:
        h = e._h
        got = [lib.bfir_engine_bank_create(h, 4), lib.bfir_engine_bank_destroy(h), lib.bfir_engine_bank_entries(h),
               lib.bfir_engine_bank_blocks(h, 0), lib.bfir_engine_bank_load(h, 0, 1, p, L, 1, 1.0),
               lib.bfir_engine_bank_read(h, 0, 0, dst.ctypes.data), lib.bfir_engine_set_coeff_matrix_bank(h, one),
               lib.bfir_engine_set_coeff_matrix_bank_fade(h, one, 2), lib.bfir_engine_set_coeff_matrix_pairs_bank(h, 1, one, one, one),
               lib.bfir_engine_set_coeff_matrix_pairs_bank_fade(h, 1, one, one, one, 2)]
        assert got == [U] * 10, (type(e).__name__, got)
        assert not e.is_initialized()
        if isinstance(e, bfir.BrutefirMatrix):   # the methods are there on the multi-level classes and pass the refusal on
            assert e.bank_create(4) == U and e.bank_entries() == U and e.set_coeff_pairs_bank([(0, 0)], [0]) == U
            assert e.set_coeff_bank([[0, 0], [0, 0]]) == U and e.bank_load(0, [hh]) == U
            with pytest.raises(bfir.BfirError) as ei:
                e.bank_read(0, 0)
            assert ei.value.code == U
        e.close()


# ---- 7. offsets past 2^32 ------------------------------------------------------------------------------------------------------
def test_an_entry_beyond_4_gib(bfir):
    """16385 entries of L = 4096, B = 8 in fp32 are 256 KiB each: the last one starts at byte 2^32.  Only the first and the
    last are loaded; the last is gathered into a 2 -> 2 engine.  The test's own work is a third of a second; where it is the
    first of a session to import torch (for mem_get_info) it is charged that import too."""
    import torch
    L, B, s, n = 4096, 8, 4, 16385
    assert (n - 1) * B * 2 * L * s == 1 << 32
    if torch.cuda.mem_get_info()[0] < 12 << 30:
        pytest.skip("less than 12 GiB of device memory free")
    rng = np.random.default_rng(4096)
    hs = []
    for j in range(2):
        h = np.zeros(B * L, np.float32)
        h[:B * L - 5 - j] = flat_ir(rng, 1, B * L - 5 - j)[0]
        hs.append(h)
    e, twin = bfir.BrutefirMatrix(L, B, s, 2, 2), bfir.BrutefirMatrix(L, B, s, 2, 2)
    assert e.bank_create(n) == 0
    assert e.bank_load(0, [hs[0]]) == 0 and e.bank_load(n - 1, [hs[1]], coeff_blocks=B - 1) == 0
    assert e.bank_blocks(0) == B and e.bank_blocks(n - 1) == B - 1 and e.bank_blocks(n - 2) == 0
    assert e.set_coeff_bank([[n - 1, None], [None, n - 1]]) == 0
    assert twin.set_coeff([[hs[1], None], [None, hs[1]]], coeff_blocks=B - 1) == 0
    assert _store(e) == _store(twin)
    assert all(e.bank_read(n - 1, b).tobytes() == twin.coeff_block(0, 0, b).tobytes() for b in range(B))
    x = _frames(np.random.default_rng(5), 3, L, 2, F32)
    _both(e, twin, x, L, (1, 2))
    assert e.set_coeff_pairs_bank([(0, 1), (1, 1)], [0, None]) == 0
    assert twin.set_coeff_pairs([(0, 1)], [hs[0]]) == 0 and twin.set_coeff_pairs([(1, 1)], [None]) == 0
    assert _store(e) == _store(twin)
    _both(e, twin, x, L, (3,))
    e.close(); twin.close()

