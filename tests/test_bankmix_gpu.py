"""Bank mixes on the GPU (bfir_engine_set_coeff_matrix_bank_mix, _bank_mix_fade, _pairs_bank_mix, _pairs_bank_mix_fade;
k_bank_mix in csrc/bankmix.hip): a row of the filter store as fl(w_1 h_1), then fl(. + fl(w_m h_m)) over up to four bank entries.

The definition is checked BIT FOR BIT: every partition of every row read back with coeff_block equals bankmix_model.mix_row
of the entries' spectra as bank_read gives them (item 1).  The identities with the calls that were there before (one term of
weight 1; two halves; a power of two against a bank loaded at that scale) compare bytes of stores and of every output block
(item 2).  Outputs are held against the float64 direct convolution with taps sum w~_j loaded_j at conftest.TOL (items 3 and
5; w~ the weight as converted to the working precision) -- the only tolerance in this file.

The shapes, kinds and banks are test_bank_gpu's, for the reasons written there: k_bank_mix has k_bank_gather's spans of 256
lanes x 16 bytes (two per workgroup where the gather makes four), so `below`, `boundary` (counts 33 and 39: the live / zero
edge, and the edge between two terms' counts, inside a span), `partial` and `multiple` (more than one workgroup per row) lie
where they lie there.  Weights come from fixed seeds with |w| in [2^-6, 4] and mixed signs, filters from flat_ir, and the
model asserts that no product or sum is subnormal, so single and double IEEE arithmetic in NumPy is the device's."""
import ctypes as C

import numpy as np
import pytest

from bankmix_model import converted, mix_row
from conftest import TOL
from size_matrix import flat_ir
from test_bank_gpu import (CASES, CUTS, IDS, KINDS, PER, PRE, SIZES, _SHAPES, _bank, _both, _dt, _mixed_rows, _new, _old_rows,
                           _pair_list, _started, _store, _x)
from test_fade import fade_weights
from test_mimo_gpu import _ref64, _run_cut, _worst
from test_pairs import merge

pytestmark = pytest.mark.gpu

T = 4                            # BFIR_BANK_MIX_TERMS
K = 3                            # fading blocks


def _weights(rng, n):
    return [float(w) for w in rng.choice([-1.0, 1.0], n) * 2.0 ** rng.uniform(-6.0, 2.0, n)]


def _cycle(bk):
    """The loaded entries with the counts taking turns."""
    return [bk.index[c][j] for j in range(PER) for c in bk.counts]


def _mix_terms(bk, n_rows, n_terms, seed):
    """n_terms (entry, weight) per listed row, the terms of a row naming entries of different counts.  Row 0 begins with two
    middle counts (33 and 39 on `boundary`); row 1 has no live term; the last term of row 2 has no entry; the FIRST term of row
    3 names the empty entry with weight 0, so the sum starts with a later term."""
    assert n_rows >= 4
    rng = np.random.default_rng(seed)
    ents = _cycle(bk)
    rows = []
    for k in range(n_rows):
        es = [ents[(5 * k + 7 * j + k // len(ents)) % len(ents)] for j in range(n_terms)]
        rows.append(list(zip(es, _weights(rng, n_terms))))
    mid = [bk.index[bk.counts[min(m, len(bk.counts) - 1)]][0] for m in (1, 2)]
    for j in range(min(2, n_terms)):
        rows[0][j] = (mid[j], rows[0][j][1])
    rows[1] = [((None, 1.5), (bk.empty, 0.0), (bk.never, -0.0), (None, 0.0))[j] for j in range(n_terms)]
    rows[2][-1] = (None, rows[2][-1][1])
    rows[3][0] = (bk.empty, 0.0)
    return rows


def _count(bk, en):
    return 0 if en is None else bk.count_of.get(en, 0)


_read_cache = {}


def _reads(e, bk, key):
    """Every entry's B partitions as bank_read gives them, read once per (kind, size, precision)."""
    if key not in _read_cache:
        r = {}
        for en in range(bk.n):
            a = np.stack([e.bank_read(en, b) for b in range(bk.B)])
            a.setflags(write=False)
            r[en] = a
        _read_cache[key] = r
    return _read_cache[key]


def _model(reads, bk, terms, s):
    terms = terms or []
    row, c = mix_row([None if en is None else reads[en] for en, _ in terms], [_count(bk, en) for en, _ in terms],
                     [w for _, w in terms], _dt(s), bk.B)
    if row.shape[1] == 0:                                    # no term names an entry: the model has no width to go by
        assert c == 0
        row = np.zeros((bk.B, 2 * bk.L), _dt(s))
    return row, c


def _row(e, o, i):
    return b"".join(e.coeff_block(o, i, b).tobytes() for b in range(e.B))


def _mixed_taps(bk, terms, s):
    """The taps a mix stands for, as the float64 reference takes them: sum of w~_j loaded_j (None: no live term)."""
    live = [(en, float(converted(w, _dt(s)))) for en, w in (terms or []) if en is not None and converted(w, _dt(s)) != 0]
    if not live:
        return None
    h = np.zeros(max(_count(bk, en) for en, _ in live) * bk.L)
    for en, w in live:
        t = np.asarray(bk.loaded(en), np.float64)
        h[:t.size] += w * t
    return h


def _grid(flat, n_in, n_out):
    return [flat[o * n_in:(o + 1) * n_in] for o in range(n_out)]


def _every(n_in, n_out):
    return [(o, i) for o in range(n_out) for i in range(n_in)]


def _listed(every):
    return every[1::2] if len(every) > 8 else every[1:]


# ---- 1. the stores, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,size,s", CASES, ids=IDS)
def test_stores_are_the_models(bfir, kind, size, s):
    (_, n_in, n_out), (L, B) = KINDS[kind], SIZES[size]
    bk = _bank(L, B, s)
    e = _started(bfir, kind, size, s)
    reads = _reads(e, bk, (kind, size, s))
    every = _every(n_in, n_out)
    pairs = _listed(every)
    seen = set()
    for nt in range(1, T + 1):
        terms = _mix_terms(bk, len(every), nt, 100 * nt + s)
        assert e.set_coeff_bank_mix(_grid(terms, n_in, n_out)) == 0
        assert e.is_initialized() and e.fade_remaining() == 0
        for (o, i), t in zip(every, terms):
            want, c = _model(reads, bk, t, s)
            assert not want[c:].any()
            assert _row(e, o, i) == want.tobytes(), (nt, o, i, t)            # zeros at and past the count included
            seen.add(frozenset(_count(bk, en) for en, w in t if en is not None and w != 0))
        before = {p: _row(e, *p) for p in every if p not in pairs}
        pterms = _mix_terms(bk, len(pairs), nt, 100 * nt + s + 50)
        pterms[-1] = None                                                     # a pair removed by None
        assert e.set_coeff_pairs_bank_mix(pairs, pterms) == 0
        for (o, i), t in zip(pairs, pterms):
            assert _row(e, o, i) == _model(reads, bk, t, s)[0].tobytes(), (nt, o, i, t)
        assert all(_row(e, *p) == was for p, was in before.items())         # unlisted rows keep their bytes
    assert frozenset() in seen                                               # a row without a live term
    assert any(len(c) >= 2 for c in seen) or B == 1                          # terms of different counts in one row
    if size == "boundary":
        assert frozenset((33, 39)) in seen
    e.close()


# ---- 2. identities with the calls that were there before (bytes) ---------------------------------------------------------------
def _as_terms(en, halves):
    if en is None:
        return None
    return [(en, 0.5), (en, 0.5)] if halves else [(en, 1.0)]


@pytest.mark.parametrize("halves", (False, True), ids=("one", "halves"))
@pytest.mark.parametrize("kind,size,s", CASES, ids=IDS)
def test_one_term_of_weight_one_is_the_bank_call(bfir, kind, size, s, halves):
    """2a, 2b: (e, 1.0), and (e, 0.5), (e, 0.5), against set_coeff_bank, set_coeff_pairs_bank and both fades on a twin."""
    (_, n_in, n_out), (L, B) = KINDS[kind], SIZES[size]
    bk = _bank(L, B, s)
    nb = PRE + 4 * sum(CUTS)
    x = _x(kind, size, s, nb)
    e, twin = _started(bfir, kind, size, s), _started(bfir, kind, size, s)
    _both(e, twin, x[:PRE * L], L, (PRE,))
    t = PRE

    def same():
        nonlocal t
        assert _store(e) == _store(twin)
        _both(e, twin, x[t * L:(t + sum(CUTS)) * L], L, CUTS)
        t += sum(CUTS)

    rows = _mixed_rows(bk, n_in, n_out)
    assert e.set_coeff_bank_mix([[_as_terms(en, halves) for en in r] for r in rows]) == 0 and twin.set_coeff_bank(rows) == 0
    same()
    c = max(1, B - 1)
    pairs, ents = _pair_list(bk, n_in, n_out, bk.index[c][:2])
    assert e.set_coeff_pairs_bank_mix(pairs, [_as_terms(en, halves) for en in ents]) == 0
    assert twin.set_coeff_pairs_bank(pairs, ents) == 0
    same()
    pairs, ents = _pair_list(bk, n_in, n_out, bk.index[bk.counts[0]][1:])
    assert e.set_coeff_pairs_bank_mix_fade(pairs, [_as_terms(en, halves) for en in ents], K) == 0
    assert twin.set_coeff_pairs_bank_fade(pairs, ents, K) == 0
    assert e.fade_remaining() == twin.fade_remaining() == K
    same()                                                                   # CUTS reaches past the fade: the stores are the new set
    assert e.fade_remaining() == twin.fade_remaining() == 0
    rows = [r[::-1] for r in rows[::-1]]
    assert e.set_coeff_bank_mix_fade([[_as_terms(en, halves) for en in r] for r in rows], K) == 0
    assert twin.set_coeff_bank_fade(rows, K) == 0
    same()
    assert e.fade_remaining() == twin.fade_remaining() == 0
    e.close(); twin.close()


@pytest.mark.parametrize("k", (-3, 2))
@pytest.mark.parametrize("kind,size,s", CASES, ids=IDS)
def test_a_power_of_two_is_the_scale_of_the_load(bfir, kind, size, s, k):
    """2c: an entry loaded with scale g and mixed with weight 2^k, against the same taps loaded with scale g 2^k and gathered."""
    (_, n_in, n_out), (L, B) = KINDS[kind], SIZES[size]
    bk = _bank(L, B, s)
    g = 0.75
    hs = [bk.filters[bk.counts[-1]][0], bk.filters[bk.counts[0]][1]]
    e, twin = _new(bfir, kind, size, s), _new(bfir, kind, size, s)
    assert e.bank_create(2) == 0 and twin.bank_create(2) == 0
    assert e.bank_load(0, hs, coeff_blocks=B, scale=g) == 0 and twin.bank_load(0, hs, coeff_blocks=B, scale=g * 2.0 ** k) == 0
    ents = [[(o + i) % 2 for i in range(n_in)] for o in range(n_out)]
    assert e.set_coeff_bank_mix([[[(en, 2.0 ** k)] for en in r] for r in ents]) == 0 and twin.set_coeff_bank(ents) == 0
    assert _store(e) == _store(twin)
    _both(e, twin, _x(kind, size, s, sum(CUTS)), L, CUTS)
    e.close(); twin.close()


# ---- 3. outputs against float64 ------------------------------------------------------------------------------------------------
def _unequal_terms(bk, n_rows, seed):
    """Rows of two, three and four terms in turn; one term of every row at 1/8 of the others' magnitude."""
    rng = np.random.default_rng(seed)
    ents = _cycle(bk)
    rows = []
    for k in range(n_rows):
        nt = 2 + k % 3
        m = 2.0 ** rng.uniform(-2.0, 1.0)
        sg = rng.choice([-1.0, 1.0], nt)
        rows.append([(ents[(3 * k + 5 * j) % len(ents)], float(sg[j] * (m / 8 if j == k % nt else m))) for j in range(nt)])
    return rows


@pytest.mark.parametrize("kind,size,s", CASES, ids=IDS)
def test_outputs_against_float64(orc, bfir, kind, size, s):
    (_, n_in, n_out), (L, B) = KINDS[kind], SIZES[size]
    bk = _bank(L, B, s)
    nb = B + 3
    x = _x(kind, size, s, nb)
    terms = _unequal_terms(bk, n_in * n_out, 31 + s)
    terms[n_in] = None                                                        # pair (1, 0) without a path
    e = _started(bfir, kind, size, s)
    assert e.set_coeff_bank_mix(_grid(terms, n_in, n_out)) == 0
    rcs, y = _run_cut(e, x, L, (1, nb - 1))
    assert rcs == [0, 0]
    want = _ref64(orc, _grid([_mixed_taps(bk, t, s) for t in terms], n_in, n_out), x)
    err = _worst(y, want, L)
    print("%s %s f%d: worst block %.3g against float64" % (kind, size, 8 * s, err))
    assert err <= TOL[s]
    e.close()


# ---- 4. stale bytes are never read ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,size,s", [c for c in CASES if SIZES[c[1]][1] > 1], ids=[i for c, i in zip(CASES, IDS) if SIZES[c[1]][1] > 1])
def test_what_lies_past_an_entrys_count_is_not_read(bfir, kind, size, s):
    (_, n_in, n_out), (L, B) = KINDS[kind], SIZES[size]
    bk = _bank(L, B, s)
    first, other, long_ = bk.filters[B][0], bk.filters[B][1], bk.filters[B][2]
    e = _new(bfir, kind, size, s)
    assert e.bank_create(2) == 0
    assert e.bank_load(0, [first, long_], coeff_blocks=B) == 0
    terms = [(0, -1.25), (1, 0.625)]
    rows = [[terms] * n_in] * n_out
    assert e.set_coeff_bank_mix(rows) == 0
    with_first = _store(e)
    assert e.bank_load(0, [other], coeff_blocks=1, scale=0.5) == 0          # partitions 1 .. B - 1 of the store keep `first`
    assert e.bank_blocks(0) == 1 and e.bank_blocks(1) == B
    reads = [np.stack([e.bank_read(en, b) for b in range(B)]) for en in (0, 1)]
    assert not reads[0][1:].any()
    want, c = mix_row(reads, [1, B], [w for _, w in terms], _dt(s), B)
    assert c == B and want[1:].tobytes() == (_dt(s)(0.625) * reads[1][1:]).tobytes()
    assert e.set_coeff_bank_mix(rows) == 0
    assert all(_row(e, o, i) == want.tobytes() for o in range(n_out) for i in range(n_in))
    assert _store(e) != with_first
    # the same with the short entry listed last, and through a pairs call
    assert e.set_coeff_pairs_bank_mix([(0, 0)], [terms[::-1]]) == 0
    want, c = mix_row(reads[::-1], [B, 1], [0.625, -1.25], _dt(s), B)
    assert c == B and _row(e, 0, 0) == want.tobytes()
    e.close()


# ---- 5. fades ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("whole", (False, True), ids=("pairs", "whole"))
@pytest.mark.parametrize("kind,size,s", CASES, ids=IDS)
def test_fades_to_a_mixed_set(orc, bfir, kind, size, s, whole):
    (_, n_in, n_out), (L, B) = KINDS[kind], SIZES[size]
    bk = _bank(L, B, s)
    nb = PRE + sum(CUTS)
    assert sum(CUTS) > K
    x = _x(kind, size, s, nb)
    old = _old_rows(kind, size, s)
    every = _every(n_in, n_out)
    pairs = every if whole else _listed(every)
    terms = _unequal_terms(bk, len(pairs), 77 + s)
    terms[1] = [(None, 1.0), (bk.empty, 0.0)]                                 # a path removed
    new = merge(old, pairs, [_mixed_taps(bk, t, s) for t in terms])

    def plain(eng):
        return eng.set_coeff_bank_mix(_grid(terms, n_in, n_out)) if whole else eng.set_coeff_pairs_bank_mix(pairs, terms)

    def fade(eng):
        return (eng.set_coeff_bank_mix_fade(_grid(terms, n_in, n_out), K) if whole
                else eng.set_coeff_pairs_bank_mix_fade(pairs, terms, K))

    # through the fade
    e, never, twin = _started(bfir, kind, size, s), _started(bfir, kind, size, s, bank=False), _started(bfir, kind, size, s)
    y0 = _both(e, never, x[:PRE * L], L, (PRE,))                              # before t0: an engine never changed
    rct, _ = _run_cut(twin, x[:PRE * L], L, (PRE,))
    before = _store(e)
    assert fade(e) == 0 and plain(twin) == 0 and rct == [0]
    assert e.fade_remaining() == K and _store(e) == before                    # the old set is read until the fade is over
    left, ys, t = [], [], PRE
    for n in CUTS:
        rc, y = e.run(x[t * L:(t + n) * L])
        assert rc == 0
        ys.append(y); left.append(e.fade_remaining()); t += n
    assert left == [max(0, K - sum(CUTS[:j + 1])) for j in range(len(CUTS))] and left[0] == K - 1 and left[-1] == 0
    rct, yt = _run_cut(twin, x[PRE * L:], L, CUTS)
    y1 = np.concatenate(ys)
    assert rct == [0] * len(CUTS) and y1[K * L:].tobytes() == yt[K * L:].tobytes()   # from t0 + K on: the plain call's bytes
    assert _store(e) == _store(twin)
    w = fade_weights(L, nb, PRE, K)[:, None]
    want = _ref64(orc, old, x) * (1.0 - w) + _ref64(orc, new, x) * w
    err = _worst(np.concatenate([y0, y1]), want, L)
    print("%s %s f%d %s: worst block %.3g against the float64 blend" % (kind, size, 8 * s, "whole" if whole else "pairs", err))
    assert err <= TOL[s]
    e.close(); never.close(); twin.close()

    # a plain mix call during the fade cancels it: the old set, patched, goes on
    e, twin = _started(bfir, kind, size, s), _started(bfir, kind, size, s)
    _both(e, twin, x[:PRE * L], L, (PRE,))
    assert fade(e) == 0
    rc, _ = e.run(x[PRE * L:(PRE + 1) * L])
    rct, _ = twin.run(x[PRE * L:(PRE + 1) * L])
    assert rc == 0 and rct == 0 and e.fade_remaining() == K - 1
    patch = [(bk.index[bk.counts[-1]][2], -0.375), (bk.index[bk.counts[0]][0], 1.75)]
    assert e.set_coeff_pairs_bank_mix([(0, 0)], [patch]) == 0 and twin.set_coeff_pairs_bank_mix([(0, 0)], [patch]) == 0
    assert e.fade_remaining() == 0 and _store(e) == _store(twin)
    _both(e, twin, x[(PRE + 1) * L:], L, (2, nb - PRE - 3))
    e.close(); twin.close()

    # reset() ends it with the mixed set active
    e, twin = _started(bfir, kind, size, s), _started(bfir, kind, size, s)
    assert fade(e) == 0 and plain(twin) == 0
    rc, _ = e.run(x[:L])
    assert rc == 0 and e.fade_remaining() == K - 1
    e.reset(); twin.reset()
    assert e.fade_remaining() == 0 and _store(e) == _store(twin)
    _both(e, twin, x[:3 * L], L, (1, 2))
    e.close(); twin.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def _ints(*v):
    return (C.c_int * len(v))(*v)


def _dbls(*v):
    return (C.c_double * len(v))(*v)


def test_other_kinds_are_unsupported(bfir):
    """The kind comes before the arguments: null pointers and n_terms = 0 still give ERR_UNSUPPORTED."""
    L, B, blocks, ratios = 512, 2, (5, 3, 2), (1, 4, 2)
    lib = bfir.load()
    U = bfir.ERR_UNSUPPORTED
    one, w = _ints(0), _dbls(1.0)
    engines = [bfir.Brutefir(L, B, 4, 2), bfir.BrutefirMatrixLevels(L, blocks, ratios, 4, 2, 2),
               bfir.BrutefirMimoLevels(L, blocks, ratios, 4, 2, 2)]
    for e in engines:
        h = e._h
        for ents, wts, nt in ((one, w, 1), (None, None, 0)):
            got = [lib.bfir_engine_set_coeff_matrix_bank_mix(h, nt, ents, wts),
                   lib.bfir_engine_set_coeff_matrix_bank_mix_fade(h, nt, ents, wts, 2),
                   lib.bfir_engine_set_coeff_matrix_pairs_bank_mix(h, 1, one, one, nt, ents, wts),
                   lib.bfir_engine_set_coeff_matrix_pairs_bank_mix_fade(h, 1, one, one, nt, ents, wts, 2)]
            assert got == [U] * 4, (type(e).__name__, got)
        assert not e.is_initialized()
        if isinstance(e, bfir.BrutefirMatrix):   # the methods are there on the multi-level classes and pass the refusal on
            assert e.set_coeff_bank_mix([[[(0, 1.0)]] * 2] * 2) == U and e.set_coeff_pairs_bank_mix([(0, 0)], [[(0, 1.0)]]) == U
            assert e.set_coeff_bank_mix_fade([[[(0, 1.0)]] * 2] * 2, 2) == U
            assert e.set_coeff_pairs_bank_mix_fade([(0, 0)], [[(0, 1.0)]], 2) == U
        e.close()
    # a batch refuses the fades (it is no matrix engine: every call, in fact)
    e = bfir.Brutefir(L, B, 4, 2, n_engines=2)
    assert lib.bfir_engine_set_coeff_matrix_bank_mix_fade(e._h, 1, one, w, 2) == U
    e.close()


def test_refusals_change_nothing(bfir):
    """Every ARG and STATE refusal on a matrix engine, in the order of the header; after each the next block's bytes are those
    of a twin that got the accepted calls alone, and at the end the stores and a running fade's count are the twin's too."""
    kind, s = "matrix", 4
    L, B = _SHAPES["refusals"]
    (_, n_in, n_out) = KINDS[kind]
    bk = _bank(L, B, s)
    lib = bfir.load()
    x = _x(kind, "refusals", s, 128)
    ARG, STATE = bfir.ERR_ARG, bfir.ERR_STATE
    P = n_in * n_out
    good = bk.index[B][0]
    e, twin = _new(bfir, kind, "refusals", s), _new(bfir, kind, "refusals", s)
    h = e._h
    state = {"t": 0}
    whole = (lib.bfir_engine_set_coeff_matrix_bank_mix, lib.bfir_engine_set_coeff_matrix_bank_mix_fade)
    listed = (lib.bfir_engine_set_coeff_matrix_pairs_bank_mix, lib.bfir_engine_set_coeff_matrix_pairs_bank_mix_fade)

    def refused(rc, want):
        assert rc == want, (rc, want)
        assert e.is_initialized() == twin.is_initialized() and e.fade_remaining() == twin.fade_remaining()
        if e.is_initialized():
            t = state["t"]
            _both(e, twin, x[t * L:(t + 1) * L], L, (1,))
            state["t"] = t + 1

    def all_four(ents, wts, want, nt=1, tail=(2,), n_pairs=1, outs=None, ins=None):
        """The four calls with one listed row (the whole-matrix calls: that row first, the rest `good` at weight 1)."""
        outs, ins = outs or _ints(*[0] * n_pairs), ins or _ints(*range(n_pairs))
        full_e = None if ents is None else _ints(*(list(ents) + [good] * nt * (P - 1)))
        full_w = None if wts is None else _dbls(*(list(wts) + [1.0] * nt * (P - 1)))
        if n_pairs == 1:
            for f, tl in zip(whole, ((), tail)):
                refused(f(h, nt, full_e, full_w, *tl), want)
        for f, tl in zip(listed, ((), tail)):
            refused(f(h, n_pairs, outs, ins, nt, ents, wts, *tl), want)

    one, w1 = _ints(good), _dbls(1.0)
    # 3 before 4: the arguments before the missing bank; 4: no bank
    all_four(one, w1, ARG, nt=0)
    all_four(one, w1, ARG, nt=T + 1)
    all_four(None, w1, ARG)
    all_four(one, w1, STATE)
    bk.load(e); bk.load(twin)
    # 9 / 8: an engine without coefficients (the whole-matrix plain call would initialise it: not called here)
    refused(lib.bfir_engine_set_coeff_matrix_pairs_bank_mix(h, 1, _ints(0), _ints(0), 1, one, w1), STATE)
    refused(lib.bfir_engine_set_coeff_matrix_pairs_bank_mix_fade(h, 1, _ints(0), _ints(0), 1, one, w1, 2), STATE)
    refused(e.set_coeff_bank_mix_fade([[[(good, 1.0)]] * n_in] * n_out, 2), STATE)
    refused(e.set_coeff_bank_mix_fade([[[(good, 1.0)]] * n_in] * n_out, 0), ARG)      # 7 before 8
    refused(e.set_coeff_pairs_bank_mix_fade([(0, 0)], [[(bk.empty, 1.0)]], 0), STATE)   # 6 before 7
    assert not e.is_initialized()
    first = [[[(bk.index[c][(o + i) % PER], 0.5 + 0.25 * i) for c in bk.counts[:2]] for i in range(n_in)] for o in range(n_out)]
    assert e.set_coeff_bank_mix(first) == 0 and twin.set_coeff_bank_mix(first) == 0   # initialised from the bank alone
    assert e.is_initialized()
    # 3: null pointers and counts
    all_four(None, w1, ARG)
    all_four(one, None, ARG)
    all_four(one, w1, ARG, nt=0)
    all_four(one, w1, ARG, nt=-1)
    all_four(one, w1, ARG, nt=T + 1)
    for f, tl in zip(listed, ((), (2,))):
        refused(f(h, 1, None, _ints(0), 1, one, w1, *tl), ARG)
        refused(f(h, 1, _ints(0), None, 1, one, w1, *tl), ARG)
        refused(f(h, 0, _ints(0), _ints(0), 1, one, w1, *tl), ARG)
        refused(f(h, -1, _ints(0), _ints(0), 1, one, w1, *tl), ARG)
        # 5: pairs
        refused(f(h, 1, _ints(n_out), _ints(0), 1, one, w1, *tl), ARG)
        refused(f(h, 1, _ints(0), _ints(n_in), 1, one, w1, *tl), ARG)
        refused(f(h, 1, _ints(-1), _ints(0), 1, one, w1, *tl), ARG)
        refused(f(h, 2, _ints(1, 1), _ints(0, 0), 1, _ints(good, good), _dbls(1.0, 1.0), *tl), ARG)   # the same pair twice
    # 5: indices, live or not, and weights
    all_four(_ints(good, bk.n), _dbls(1.0, 0.0), ARG, nt=2)                   # n_entries in a dead term
    all_four(_ints(bk.n), w1, ARG)
    all_four(_ints(-2), _dbls(0.0), ARG)
    all_four(_ints(good), _dbls(float("nan")), ARG)
    all_four(_ints(good), _dbls(float("inf")), ARG)
    all_four(_ints(-1), _dbls(float("-inf")), ARG)                            # in a term without an entry too
    all_four(_ints(good), _dbls(1e39), ARG)                                   # infinite as a float
    all_four(_ints(good), _dbls(-3.5e38), ARG)                                # rounds past the largest float
    # 6: a live term names an empty entry -- loaded as None, and never loaded; behind 5 wherever the ARG stands in the call
    all_four(_ints(good, bk.empty), _dbls(1.0, 0.5), STATE, nt=2)
    all_four(_ints(bk.never), w1, STATE)
    all_four(_ints(bk.empty, good, good, bk.n), _dbls(1.0, 1.0, 1.0, 1.0), ARG, nt=2, n_pairs=2)   # pair 0: 6, pair 1: 5
    all_four(_ints(bk.empty), w1, STATE, tail=(0,))                           # 6 before 7
    # ... and what is NOT refused: weight 0, or one that converts to 0, may name an empty entry; the path is removed
    for wz in (0.0, -0.0, 1e-60):
        for eng in (e, twin):
            assert eng.set_coeff_pairs_bank_mix([(0, 1)], [[(bk.empty, wz), (bk.never, wz)]]) == 0
        assert not any(e.coeff_block(0, 1, b).any() for b in range(B))
        refused(0, 0)
    # 7: fade arguments
    for Kbad in (0, -1, (1 << 24) // L + 1):
        refused(e.set_coeff_bank_mix_fade(first, Kbad), ARG)
        refused(e.set_coeff_pairs_bank_mix_fade([(0, 0)], [[(good, 1.0)]], Kbad), ARG)
    # 8: one fade at a time; and every refusal above once more during the fade
    mix = [(bk.index[B][1], 0.75), (bk.index[1][2], -2.0)]
    assert e.set_coeff_pairs_bank_mix_fade([(0, 0)], [mix], 60) == 0 and twin.set_coeff_pairs_bank_mix_fade([(0, 0)], [mix], 60) == 0
    refused(e.set_coeff_pairs_bank_mix_fade([(1, 0)], [[(good, 1.0)]], 2), STATE)
    refused(e.set_coeff_bank_mix_fade(first, 2), STATE)
    for f, tl in zip(listed, ((), (2,))):
        refused(f(h, 1, _ints(0), _ints(0), 0, one, w1, *tl), ARG)
        refused(f(h, 1, _ints(0), _ints(0), 1, _ints(bk.n), _dbls(0.0), *tl), ARG)
        refused(f(h, 1, _ints(0), _ints(0), 1, one, _dbls(float("nan")), *tl), ARG)
        refused(f(h, 1, _ints(0), _ints(0), 1, _ints(bk.empty), w1, *tl), STATE)
    assert e.fade_remaining() == twin.fade_remaining() > 0
    assert _store(e) == _store(twin)
    assert state["t"] >= 90                                                   # the refusals above were each followed by a block
    e.close(); twin.close()


def test_a_weight_past_float_is_fine_in_double(bfir):
    """1e39 is refused on an fp32 engine (above) and accepted on an fp64 one; 1e-60 is live there."""
    kind, s = "matrix", 8
    L, B = _SHAPES["refusals"]
    bk = _bank(L, B, s)
    e = _new(bfir, kind, "refusals", s)
    bk.load(e)
    en = bk.index[B][0]
    (_, n_in, n_out) = KINDS[kind]
    rows = [[[(en, 1e39), (bk.index[1][0], -1e39)]] * n_in] * n_out
    assert e.set_coeff_bank_mix(rows) == 0
    reads = [np.stack([e.bank_read(k, b) for b in range(B)]) for k in (en, bk.index[1][0])]
    want, c = mix_row(reads, [B, 1], [1e39, -1e39], np.float64, B)
    assert c == B and _row(e, 0, 0) == want.tobytes()
    assert e.set_coeff_pairs_bank_mix([(0, 0)], [[(en, 1e-60)]]) == 0
    assert _row(e, 0, 0) == mix_row(reads[:1], [B], [1e-60], np.float64, B)[0].tobytes() and e.coeff_block(0, 0, 0).any()
    assert e.set_coeff_pairs_bank_mix([(0, 0)], [[(bk.empty, 1e-60)]]) == bfir.ERR_STATE   # ... and so may not name an empty entry
    e.close()


# ---- 7. the grid's edge --------------------------------------------------------------------------------------------------------
def test_every_row_of_a_64_by_64_matrix_in_one_call(bfir):
    """A mimo 64 -> 64, L = 16, B = 1, whole-matrix call with four terms: 4096 listed rows, one workgroup each.  A sample of
    rows against the model, and an output block against a twin that got the same mixes through 64 column calls."""
    L, B, s, n, NE = 16, 1, 4, 64, 12
    rng = np.random.default_rng(64)
    hs = [np.asarray(h, np.float32) for h in flat_ir(rng, NE, L - 1)]
    hs = [np.concatenate([h, np.zeros(1, np.float32)]) for h in hs]
    ents = rng.integers(0, NE, (n * n, T))
    wts = rng.choice([-1.0, 1.0], (n * n, T)) * 2.0 ** rng.uniform(-6.0, 2.0, (n * n, T))
    terms = [[(int(ents[r, j]), float(wts[r, j])) for j in range(T)] for r in range(n * n)]
    terms[n * n - 1][0] = (None, 1.0)
    terms[n + 1] = None
    e, twin = bfir.BrutefirMimo(L, B, s, n, n), bfir.BrutefirMimo(L, B, s, n, n)
    for eng in (e, twin):
        assert eng.bank_create(NE) == 0 and eng.bank_load(0, hs) == 0
    assert e.set_coeff_bank_mix(_grid(terms, n, n)) == 0
    assert twin.set_coeff_bank([[0] * n] * n) == 0                            # something to patch
    for i in range(n):
        assert twin.set_coeff_pairs_bank_mix([(o, i) for o in range(n)], [terms[o * n + i] for o in range(n)]) == 0
    reads = {en: np.stack([e.bank_read(en, 0)]) for en in range(NE)}
    for r in [0, 1, n - 1, n, n + 1, n * n - 1] + [int(v) for v in rng.integers(0, n * n, 40)]:
        t = terms[r] or []
        want, _ = mix_row([None if en is None else reads[en] for en, _ in t], [1] * len(t), [w for _, w in t], np.float32, B)
        want = want if want.shape[1] else np.zeros((B, 2 * L), np.float32)   # a row without any entry
        assert _row(e, r // n, r % n) == want.tobytes(), r
        assert _row(twin, r // n, r % n) == want.tobytes(), r
    x = (np.random.default_rng(5).uniform(-1.0, 1.0, (2 * L, n)) / 64).astype(np.float32)
    _both(e, twin, x, L, (1, 1))
    e.close(); twin.close()
