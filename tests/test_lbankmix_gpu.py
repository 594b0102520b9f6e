"""Bank mixes on multi-level matrix and mimo engines on the GPU (bfir_engine_set_coeff_matrix_levels_bank_mix, _bank_mix_fade,
_pairs_bank_mix, _pairs_bank_mix_fade; set_bank_mix, fade_to_rows_bank_mix, set_pairs_bank_mix and fade_to_pairs_bank_mix of
BrutefirMatrixLevels) and k_lbank_mix (csrc/lbankmix.hip): on every level a row of the filter store as fl(w_1 h_1), then
fl(. + fl(w_m h_m)) over up to four entries of the levels bank.

The definition is checked BIT FOR BIT: every partition of every row of every level read back with coeff_block equals
bankmix_model.mix_row of the entries' spectra as lbank_read gives them, applied per level with that level's counts (item 1).
The identities with the calls that were there before (one term of weight 1; two halves; weight 0.5 against a bank loaded at
scale 0.5; a row of dead terms) compare bytes of stores and of every output block with a twin that gets the _levels_bank calls
(items 2, 4).  Outputs are held against test_mimo_levels.wide_reference of the taps sum w~_j h_j, formed in float64 (w~: the
weight as converted to the working precision), at conftest.TOL per block and output, through the fades blended with
test_fade.fade_weights (item 3) -- the only tolerance in this file.

The shapes are the four of tests/test_lpairs.py and `boundary` and `partial` of tests/test_lbank.py in both precisions on
both kinds; tests/test_lbankmix.py holds them to their conditions without a GPU.  Their banks are test_lbank_gpu's: Banked
(the old filters of the shape, the `mixed` list's new ones, one entry never loaded) and _new_setup.  Weights come from fixed
seeds with |w| in [2^-6, 4] and mixed signs, and the model asserts that no product or sum is subnormal, so single and double
IEEE arithmetic in NumPy is the device's."""
import ctypes as C

import numpy as np
import pytest

from bankmix_model import converted, mix_row
from conftest import TOL
from test_bankmix_gpu import _weights
from test_fade import fade_weights
from test_lbank import BIG, KINDS, NEW_SHAPES
from test_lbank_gpu import NEW_K, Banked, _both, _new_setup
from test_lbankmix import BOUNDARY_TERMS
from test_levels_gpu import _settle
from test_lpairs import A_F, SHAPES, counts, geo, merge
from test_lpairs_gpu import CUTS, WIDE, _dt, _engine, _lv, _same_store, _setup, _synth
from test_mimo_gpu import _run_cut, _worst
from test_mimo_levels import wide_reference

pytestmark = pytest.mark.gpu

T = 4                            # BFIR_BANK_MIX_TERMS
NEW_CASES = [(k, z, s) for k in sorted(KINDS) for z in sorted(NEW_SHAPES) for s in (4, 8)]
CASES = sorted(SHAPES) + NEW_CASES
IDS = [c if isinstance(c, str) else "%s-%s-f%d" % (c[0], c[1], 8 * c[2]) for c in CASES]


# ---- a case: its class, shape, bank and frames ----------------------------------------------------------------------------------
class Ctx:
    """fl: the filters of the bank, entry by entry (None: loaded as None); entry len(fl) is never loaded."""

    def __init__(self, orc, case):
        self.case = case
        if isinstance(case, str):
            S = _setup(orc, case, "mixed")
            self.cls, self.shape, self.fl, self.x, self.K = SHAPES[case][0], S["shape"], Banked(S).flat, S["x"], S["K"]
            self.S = S
        else:
            N = _new_setup(orc, *case)
            self.cls, self.shape, self.fl, self.x, self.K = N["cls"], N["shape"], list(N["filters"]), N["x"], NEW_K
        self.s, self.L, self.blocks, self.ratios, self.n_in, self.n_out = self.shape
        self.never = len(self.fl)
        self.n = len(self.fl) + 1
        self.empty = next((k for k, h in enumerate(self.fl) if h is None), self.never)
        self.loaded = [k for k, h in enumerate(self.fl) if h is not None]
        self.cnt = [counts(self.shape, None if h is None else h.size) for h in self.fl] + [[0] * len(self.blocks)]
        self.every = [(o, i) for o in range(self.n_out) for i in range(self.n_in)]
        self.listed = self.every[1::2] if len(self.every) > 8 else self.every[1:]
        head_only = next(en for en in self.loaded if self.cnt[en][0] > 0 and not any(self.cnt[en][1:]))
        longest = next(en for en in self.loaded if self.cnt[en][-1] == self.blocks[-1])
        rest = [en for en in self.loaded if en not in (head_only, longest)]
        self.first_row = [head_only, longest] + rest[:2]                 # one ends in the head, one reaches the last partition
        if not isinstance(case, str) and case[1] == "boundary":
            self.first_row = [1, 2, 3, 0]
            assert tuple(tuple(self.cnt[en]) for en in self.first_row) == BOUNDARY_TERMS
        self._reads = {}

    def engine(self, bfir, chunk=3, scale=1.0):
        e = _engine(bfir, None, None, chunk=chunk, cls=self.cls, shape=self.shape)
        assert e.lbank_create(self.n) == 0 and e.lbank_load(0, self.fl, scale=scale) == 0
        return e

    def reads(self, e, en):
        """Entry en on every level as lbank_read gives it, [blocks[k]][2 L_k]; read once."""
        if en not in self._reads:
            assert [e.lbank_blocks(en, k) for k in range(len(self.blocks))] == self.cnt[en]
            r = [np.stack([e.lbank_read(en, k, b) for b in range(self.blocks[k])]) for k in range(len(self.blocks))]
            for a in r:
                a.setflags(write=False)
            self._reads[en] = r
        return self._reads[en]

    def model(self, e, terms):
        """Per level (row [blocks[k]][2 L_k], count): mix_row with that level's counts; a term whose entry does not reach the
        level takes no part there."""
        terms = terms or []
        Ls = geo(self.shape)[0]
        out = []
        for k in range(len(self.blocks)):
            here = [(en, w) for en, w in terms if en is not None and converted(w, _dt(self.s)) != 0 and self.cnt[en][k] > 0]
            row, c = mix_row([self.reads(e, en)[k] for en, _ in here], [self.cnt[en][k] for en, _ in here], [w for _, w in here],
                             _dt(self.s), self.blocks[k])
            if row.shape[1] == 0:
                row = np.zeros((self.blocks[k], 2 * Ls[k]), _dt(self.s))
            assert c == max([self.cnt[en][k] for en, _ in here], default=0) and not row[c:].any()   # the count is the maximum
            out.append((row, c))
        return out

    def live(self, terms):
        return [(en, float(converted(w, _dt(self.s)))) for en, w in (terms or []) if en is not None and converted(w, _dt(self.s)) != 0]

    def taps(self, terms):
        """The taps a mix stands for, in float64: sum of w~_j h_j (None: no live term)."""
        lv = self.live(terms)
        if not lv:
            return None
        h = np.zeros(max(self.fl[en].size for en, _ in lv))
        for en, w in lv:
            h[:self.fl[en].size] += w * np.asarray(self.fl[en], np.float64)
        return h

    def entry_taps(self, ents):
        return [[None if en is None else self.fl[en] for en in r] for r in ents]

    def grid(self, flat):
        return [flat[o * self.n_in:(o + 1) * self.n_in] for o in range(self.n_out)]

    def old_entries(self):
        """A first set from the bank that reaches every level and reads every input: entry by entry in turn, (1, 0) without a
        path, (0, 0) the longest."""
        flat = [self.loaded[(o * self.n_in + i) % len(self.loaded)] for o, i in self.every]
        flat[0] = self.first_row[1]
        if len(flat) > self.n_in:
            flat[self.n_in] = None
        return self.grid(flat)


_CTX = {}


def _ctx(orc, case):
    if case not in _CTX:
        _CTX[case] = Ctx(orc, case)
    return _CTX[case]


def _row(e, ctx, k, o, i):
    return b"".join(e.coeff_block(k, o, i, b).tobytes() for b in range(ctx.blocks[k]))


def _check_rows(e, ctx, pairs, terms, tag):
    for (o, i), t in zip(pairs, terms):
        for k, (want, c) in enumerate(ctx.model(e, t)):
            assert _row(e, ctx, k, o, i) == want.tobytes(), (tag, o, i, k, t)     # zeros at and past the count included


def _mix_terms(ctx, n_rows, n_terms, seed):
    """n_terms (entry, weight) per listed row.  Row 0 names ctx.first_row, its first weight negative; row 1 has no live term;
    the last term of row 2 has no entry; row 3 has a dead term in the middle (the first where there are two)."""
    assert n_rows >= 4
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(n_rows):
        es = [ctx.loaded[(5 * k + 7 * j + k // len(ctx.loaded)) % len(ctx.loaded)] for j in range(n_terms)]
        rows.append(list(zip(es, _weights(rng, n_terms))))
    rows[0] = [(en, -abs(w) if j == 0 else w) for j, (en, (_, w)) in enumerate(zip(ctx.first_row, rows[0]))]
    rows[1] = [((None, 1.5), (ctx.empty, 0.0), (ctx.never, -0.0), (None, 0.0))[j] for j in range(n_terms)]
    rows[2][-1] = (None, rows[2][-1][1])
    rows[3][min(1, n_terms - 1) if n_terms > 2 else 0] = (ctx.empty, 0.0)
    return rows


# ---- 1. the stores, bit for bit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_stores_are_the_models(orc, bfir, case):
    ctx = _ctx(orc, case)
    e = ctx.engine(bfir)
    seen = set()
    for nt in range(1, T + 1):
        terms = _mix_terms(ctx, len(ctx.every), nt, 100 * nt + ctx.s)
        assert e.set_bank_mix(ctx.grid(terms)) == 0
        assert e.is_initialized() and e.fade_remaining() == 0
        _check_rows(e, ctx, ctx.every, terms, nt)
        seen |= {len(ctx.live(t)) for t in terms}
        before = {p: [_row(e, ctx, k, *p) for k in range(len(ctx.blocks))] for p in ctx.every if p not in ctx.listed}
        pterms = _mix_terms(ctx, max(4, len(ctx.listed)), nt, 100 * nt + ctx.s + 50)[:len(ctx.listed)]
        pterms[-1] = None                                                     # a pair removed by None
        assert e.set_pairs_bank_mix(ctx.listed, pterms) == 0
        _check_rows(e, ctx, ctx.listed, pterms, (nt, "pairs"))
        assert all([_row(e, ctx, k, *p) for k in range(len(ctx.blocks))] == was for p, was in before.items())   # unlisted rows keep their bytes
    assert seen >= {0, 1, 2, 3, 4}                                           # no live term, and 1, 2, 3 and 4 of them
    lens = [ctx.cnt[en] for en in ctx.first_row]                             # of row 0: one ends in the head, one fills the last level
    assert any(not any(c[1:]) for c in lens) and any(c[-1] == ctx.blocks[-1] for c in lens)
    e.close()


# ---- 2. identities with the calls that were there before (bytes) ---------------------------------------------------------------
FORMS = ("one", "halves", "scale")


def _as_terms(en, form, n):
    """The mix that stands for entry en of the twin's bank; n varies where the dead terms stand."""
    if en is None:
        return [None, [], [(None, 2.0)], [(0, 0.0), (None, -1.0)]][n % 4]     # a row whose terms are all dead is entry -1
    if form == "one":
        return [[(en, 1.0)], [(None, 3.0), (en, 1.0)], [(en, 1.0), (en, 0.0)]][n % 3]
    if form == "halves":
        return [(en, 0.5), (en, 0.5)]
    return [(en, 0.5)]                                                        # the twin's bank is loaded at scale 0.5


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_identities_with_the_bank_calls(orc, bfir, case, form):
    """2a one term of weight 1, 2b two halves, 2c weight 0.5 against a bank loaded at scale 0.5, 2d all-dead rows: set_bank_mix,
    set_pairs_bank_mix, fade_to_pairs_bank_mix and fade_to_rows_bank_mix against the four _levels_bank calls on a twin, the
    stores and every output block over CUTS byte for byte."""
    ctx = _ctx(orc, case)
    L, K = ctx.L, ctx.K
    nb = A_F + 3 * sum(CUTS)
    assert sum(CUTS) > K
    x = orc.synth_audio(np.random.default_rng(7 + ctx.s), nb * L, ctx.n_in, _dt(ctx.s))
    e, twin = ctx.engine(bfir), ctx.engine(bfir, scale=0.5 if form == "scale" else 1.0)
    mix = lambda ents: [_as_terms(en, form, n) for n, en in enumerate(ents)]
    old = ctx.old_entries()
    assert e.set_bank_mix(ctx.grid(mix([en for r in old for en in r]))) == 0 and twin.set_bank(old) == 0
    assert e.is_initialized()
    t = [0]

    def same(ents, pairs, cuts):
        assert e.fade_remaining() == twin.fade_remaining()
        _both(e, twin, x[t[0] * L:(t[0] + sum(cuts)) * L], L, cuts)
        t[0] += sum(cuts)
        assert e.fade_remaining() == twin.fade_remaining() == 0
        _same_store(e, twin, ctx.shape, ctx.entry_taps(ents), pairs)

    same(old, ctx.listed, (A_F,))
    new = [None if k == 2 else ctx.loaded[(3 * k + 1) % len(ctx.loaded)] for k in range(len(ctx.listed))]
    assert e.set_pairs_bank_mix(ctx.listed, mix(new)) == 0 and twin.set_pairs_bank(ctx.listed, new) == 0
    merged = merge(old, ctx.listed, new)
    same(merged, ctx.listed, CUTS)
    back = [old[o][i] for o, i in ctx.listed]
    assert e.fade_to_pairs_bank_mix(ctx.listed, mix(back), K) == 0 and twin.fade_to_pairs_bank(ctx.listed, back, K) == 0
    assert e.fade_remaining() == K
    same(old, ctx.listed, CUTS)
    rot = [[None if en is None else ctx.loaded[(ctx.loaded.index(en) + 1) % len(ctx.loaded)] for en in r] for r in old]
    rot[0][0] = old[0][0]                                                     # every level stays reached
    assert e.fade_to_rows_bank_mix(ctx.grid(mix([en for r in rot for en in r])), K) == 0 and twin.fade_to_rows_bank(rot, K) == 0
    same(rot, ctx.every[::3], CUTS)
    e.close(); twin.close()


# ---- 3. outputs against the float64 reference -----------------------------------------------------------------------------------
def _unequal_terms(ctx, n_rows, seed):
    """Rows of two, three and four terms in turn; one term of every row at 1/8 of the others' magnitude."""
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(n_rows):
        nt = 2 + k % 3
        m = 2.0 ** rng.uniform(-2.0, 1.0)
        sg = rng.choice([-1.0, 1.0], nt)
        rows.append([(ctx.loaded[(3 * k + 5 * j) % len(ctx.loaded)], float(sg[j] * (m / 8 if j == k % nt else m))) for j in range(nt)])
    return rows


_REF = {}


def _mixed_case(orc, ctx):
    """The old set, the listed pairs' mixes, the whole-matrix terms of the same merged set (an unlisted pair: its old entry at
    weight 1), the frames and both references; computed once."""
    if ctx.case not in _REF:
        old = ctx.old_entries()
        terms = _unequal_terms(ctx, len(ctx.listed), 77 + ctx.s)
        terms[0] = [(ctx.first_row[1], terms[0][0][1]), (ctx.first_row[0], terms[0][1][1])]   # a listed pair keeps the last level reached
        terms[1] = [(None, 1.0), (ctx.empty, 0.0)]                            # a path removed
        whole = merge([[None if en is None else [(en, 1.0)] for en in r] for r in old], ctx.listed, terms)
        new_taps = merge(ctx.entry_taps(old), ctx.listed, [ctx.taps(t) for t in terms])
        nb = ctx.x.shape[0] // ctx.L
        assert nb >= A_F + sum(CUTS) + 1
        refs = tuple(wide_reference(orc, ctx.L, ctx.s, rows, ctx.x) for rows in (ctx.entry_taps(old), new_taps))
        _REF[ctx.case] = dict(old=old, terms=terms, whole=whole, refs=refs, nb=nb)
    return _REF[ctx.case]


@pytest.mark.parametrize("how", ("plain", "pairs", "whole"))
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_outputs_against_float64(orc, bfir, case, how):
    """plain: the mixed set from the first block on.  pairs / whole: the old set, at block A_F fade_to_pairs_bank_mix /
    fade_to_rows_bank_mix to the same merged set, against the float64 blend of both references."""
    ctx = _ctx(orc, case)
    M = _mixed_case(orc, ctx)
    L, K, x, nb = ctx.L, ctx.K, ctx.x, M["nb"]
    e = ctx.engine(bfir)
    if how == "plain":
        assert e.set_bank_mix(M["whole"]) == 0
        rcs, y = _run_cut(e, x, L, (1, nb - 1))
        want = M["refs"][1]
    else:
        assert e.set_bank(M["old"]) == 0
        rc, a = e.run(x[:A_F * L]); assert rc == 0
        assert (e.fade_to_pairs_bank_mix(ctx.listed, M["terms"], K) if how == "pairs" else e.fade_to_rows_bank_mix(M["whole"], K)) == 0
        assert e.fade_remaining() == K
        rcs, b = _run_cut(e, x[A_F * L:], L, CUTS + (nb - A_F - sum(CUTS),))
        assert e.fade_remaining() == 0
        y = np.concatenate([a, b])
        w = fade_weights(L, nb, A_F, K)[:, None]
        want = M["refs"][0] * (1.0 - w) + M["refs"][1] * w
        _check_rows(e, ctx, ctx.listed, M["terms"], how)                      # the mixed set is active on every level
    assert not any(rcs)
    err = _worst(y, want, L)
    print("%s %s: worst block %.3g against float64 (tol %g)" % (IDS[CASES.index(case)], how, err, TOL[ctx.s]))
    assert err <= TOL[ctx.s]
    e.close()


def test_a_level_newly_reached_a_level_left_and_the_fade_refused_per_level(orc, bfir):
    """9x3 with a first set that ends before the last level.  Both fades to a mix that reaches it are refused and change
    nothing; the plain pairs mix starts the level and a whole-matrix mix of short entries leaves it again: once everything
    computed before a change has played out (test_levels_gpu._settle), the blocks are the reference's at TOL."""
    name = "9x3"
    S = _setup(orc, name, "mixed")
    shape = S["shape"]
    s, L, blocks, ratios, n_in, n_out = shape
    _, D, _ = geo(shape)
    short = [[None if h is None else h[:min(h.size, D[2] - 3)] for h in row] for row in S["old"]]
    long_one = np.ascontiguousarray(S["filters"][1])
    assert long_one.size > D[2]
    P = n_in * n_out
    settle = _settle(_lv(shape))
    n0, n1 = A_F + 3, A_F + 3 + settle + 4
    nb = n1 + settle + 4
    x = orc.synth_audio(np.random.default_rng(93), nb * L, n_in, _dt(s))
    e, twin = _engine(bfir, name, None), _engine(bfir, name, None)
    for eng in (e, twin):
        assert eng.lbank_create(P + 1) == 0 and eng.lbank_load(0, [h for r in short for h in r] + [long_one]) == 0
    assert e.lbank_blocks(0, 2) == 0 and e.lbank_blocks(P, 2) > 0
    ent = [[None if h is None else o * n_in + i for i, h in enumerate(r)] for o, r in enumerate(short)]
    one = [[None if en is None else [(en, 1.0)] for en in r] for r in ent]
    assert e.set_bank_mix(one) == 0 and twin.set_bank(ent) == 0
    _both(e, twin, x[:A_F * L], L, (A_F,))
    reach = [(P, 0.5), (0, -0.25)]                                       # its count on the last level is the long entry's
    assert e.fade_to_pairs_bank_mix([(0, 0)], [reach], 5) == bfir.ERR_UNSUPPORTED
    assert e.fade_to_rows_bank_mix(merge(one, [(0, 0)], [reach]), 5) == bfir.ERR_UNSUPPORTED
    assert e.fade_remaining() == 0 and e.is_initialized()
    _both(e, twin, x[A_F * L:n0 * L], L, (3,))
    # the plain list starts the level
    assert e.set_pairs_bank_mix([(0, 0)], [reach]) == 0
    h00 = 0.5 * np.asarray(long_one, np.float64)
    h00[:short[0][0].size] -= 0.25 * np.asarray(short[0][0], np.float64)
    rc, y1 = e.run(x[n0 * L:n1 * L]); assert rc == 0
    ref = wide_reference(orc, L, s, merge(short, [(0, 0)], [h00]), x[:n1 * L])
    err1 = _worst(y1[settle * L:], ref[(n0 + settle) * L:], L)
    # ... and the whole-matrix call leaves it again
    half = [[None if en is None else [(en, 0.5)] for en in r] for r in ent]
    assert e.set_bank_mix(half) == 0
    rc, y2 = e.run(x[n1 * L:]); assert rc == 0
    ref = wide_reference(orc, L, s, [[None if h is None else 0.5 * np.asarray(h, np.float64) for h in r] for r in short], x)
    err2 = _worst(y2[settle * L:], ref[(n1 + settle) * L:], L)
    print("9x3: a level newly reached %.3g, left %.3g (tol %g)" % (err1, err2, TOL[s]))
    assert err1 <= TOL[s] and err2 <= TOL[s]
    e.close(); twin.close()


# ---- 4. state ---------------------------------------------------------------------------------------------------------------------
def test_a_plain_mix_cuts_the_fade_and_the_plain_list_waits(orc, bfir):
    name = "9x3"
    S = _setup(orc, name, "mixed")
    shape, x, K = S["shape"], S["x"], S["K"]
    L = shape[1]
    bk = Banked(S)
    halves = lambda ents: [None if en is None else [(en, 0.5), (en, 0.5)] for en in ents]
    grid = lambda rows: [halves(r) for r in rows]
    e, twin = bk.engine(bfir, name), bk.engine(bfir, name)
    _both(e, twin, x[:A_F * L], L, (A_F,))
    assert e.fade_to_pairs_bank_mix(S["pairs"], halves(bk.new), K) == 0 and twin.fade_to_pairs_bank(S["pairs"], bk.new, K) == 0
    assert e.set_pairs_bank_mix(S["pairs"], halves(bk.new)) == bfir.ERR_STATE      # pending
    _both(e, twin, x[A_F * L:(A_F + 2) * L], L, (2,))
    assert e.set_pairs_bank_mix(S["pairs"], halves(bk.new)) == bfir.ERR_STATE and e.fade_remaining() == K - 2   # running
    assert e.fade_to_pairs_bank_mix(S["pairs"], halves(bk.new), K) == bfir.ERR_STATE
    assert e.fade_to_rows_bank_mix(grid(bk.merged), K) == bfir.ERR_STATE
    assert e.set_bank_mix(grid(bk.merged)) == 0 and e.fade_remaining() == 0     # a hard cut, the twin's
    assert twin.set_bank(bk.merged) == 0
    _same_store(e, twin, shape, S["merged"], S["pairs"])
    _both(e, twin, x[(A_F + 2) * L:], L, (x.shape[0] // L - A_F - 2,))
    assert e.set_pairs_bank_mix(S["pairs"][:1], halves(bk.new[:1])) == 0        # no fade is left: the plain list is taken
    e.close(); twin.close()


@pytest.mark.parametrize("whole", (False, True), ids=("pairs", "whole"))
def test_reset_during_the_fade_leaves_the_mixed_set_active(orc, bfir, whole):
    ctx = _ctx(orc, "9x3")
    M = _mixed_case(orc, ctx)
    L, K, x = ctx.L, ctx.K, ctx.x
    e = ctx.engine(bfir)
    assert e.set_bank(M["old"]) == 0 and e.run(x[:A_F * L])[0] == 0
    assert (e.fade_to_rows_bank_mix(M["whole"], K) if whole else e.fade_to_pairs_bank_mix(ctx.listed, M["terms"], K)) == 0
    assert e.run(x[A_F * L:(A_F + 2) * L])[0] == 0 and e.fade_remaining() == K - 2
    e.reset()
    assert e.fade_remaining() == 0 and e.is_initialized()
    fresh = ctx.engine(bfir)
    assert fresh.set_bank_mix(M["whole"]) == 0
    _check_rows(e, ctx, ctx.listed, M["terms"], "reset")
    for o, i in ctx.every:
        assert all(_row(e, ctx, k, o, i) == _row(fresh, ctx, k, o, i) for k in range(len(ctx.blocks))), (o, i)
    _both(e, fresh, x, L, (x.shape[0] // L,))
    e.close(); fresh.close()


# ---- 5. how the blocks arrive -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_the_bytes_do_not_depend_on_set_chunk_or_on_how_the_blocks_arrive(orc, bfir, name):
    ctx = _ctx(orc, name)
    M = _mixed_case(orc, ctx)
    L, K, x = ctx.L, ctx.K, ctx.x
    nb = x.shape[0] // L
    out = {}
    for how, chunk, cuts in (("cuts", None, CUTS + (nb - A_F - sum(CUTS),)), ("one", None, (nb - A_F,)), ("chunk3", 3, (nb - A_F,)),
                             ("blocks", None, (1,) * (nb - A_F))):
        e = ctx.engine(bfir, chunk=chunk)
        assert e.set_bank(M["old"]) == 0
        rc, a = e.run(x[:A_F * L]); assert rc == 0
        assert e.fade_to_pairs_bank_mix(ctx.listed, M["terms"], K) == 0
        rcs, b = _run_cut(e, x[A_F * L:], L, cuts)
        assert rcs == [0] * len(cuts) and e.fade_remaining() == 0
        out[how] = np.concatenate([a, b]).tobytes()
        e.close()
    assert out["cuts"] == out["one"] == out["chunk3"] == out["blocks"]


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def _ints(v):
    return None if v is None else (C.c_int * max(1, len(v)))(*v)


def _dbls(v):
    return None if v is None else (C.c_double * max(1, len(v)))(*v)


def test_refusals_come_in_the_documented_order_and_change_nothing(orc, bfir):
    """The order of the header.  On the running engine every refusal is followed by a block whose bytes are those of a twin
    that got the accepted calls alone; at the end the stores and a running fade's count are the twin's too.  (The launch's own
    refusal, 7, needs a store the allocator never hands out and is not provoked.)"""
    ctx = _ctx(orc, "9x3")
    M = _mixed_case(orc, ctx)
    s, L, blocks, ratios, n_in, n_out = ctx.shape
    lib = bfir.load()
    A, U, ST = bfir.ERR_ARG, bfir.ERR_UNSUPPORTED, bfir.ERR_STATE
    P = n_in * n_out
    good = ctx.first_row[1]
    x = orc.synth_audio(np.random.default_rng(6), 128 * L, n_in, _dt(s))
    names = ("bfir_engine_set_coeff_matrix_levels_bank_mix", "bfir_engine_set_coeff_matrix_levels_bank_mix_fade",
             "bfir_engine_set_coeff_matrix_levels_pairs_bank_mix", "bfir_engine_set_coeff_matrix_levels_pairs_bank_mix_fade")
    fns = [getattr(lib, n) for n in names]

    def four(eng, ents, wts, nt=1, K_=2, n=1, o=(0,), i=(0,), which="wfpq"):
        """The four calls with one listed row (the whole-matrix calls: that row first, the rest `good` at weight 1)."""
        h = eng.handle
        full_e = None if ents is None else list(ents)[:max(nt, 0)] + [good] * max(nt, 0) * (P - 1)
        full_w = None if wts is None else list(wts)[:max(nt, 0)] + [1.0] * max(nt, 0) * (P - 1)
        call = dict(w=lambda: fns[0](h, nt, _ints(full_e), _dbls(full_w)), f=lambda: fns[1](h, nt, _ints(full_e), _dbls(full_w), K_),
                    p=lambda: fns[2](h, n, _ints(o), _ints(i), nt, _ints(ents), _dbls(wts)),
                    q=lambda: fns[3](h, n, _ints(o), _ints(i), nt, _ints(ents), _dbls(wts), K_))
        return [call[c]() for c in which]

    # 2. the kind, before the arguments: the uniform kinds and a diagonal multi-level engine have none of the group
    for other in (bfir.BrutefirMimo(L, blocks[0], s, n_in, n_out), bfir.BrutefirLevels(L, blocks, ratios, s, 2), bfir.Brutefir(L, 2, s, 2)):
        assert four(other, [0], [1.0]) == [U] * 4 and four(other, None, None, nt=0, n=0, o=None, i=None) == [U] * 4
        other.close()
    # 3. null arguments, n_pairs and n_terms come before 4. the missing bank, which comes before 5. the list and the terms
    new = _engine(bfir, "9x3", None)
    assert four(new, None, [1.0]) == [A] * 4 and four(new, [0], None) == [A] * 4
    assert four(new, [0], [1.0], o=None, which="pq") == [A] * 2 and four(new, [0], [1.0], i=None, which="pq") == [A] * 2
    assert four(new, [0], [1.0], n=0, which="pq") == [A] * 2 and four(new, [0], [1.0], n=-1, which="pq") == [A] * 2
    assert four(new, [0], [1.0], nt=0) == [A] * 4 and four(new, [0] * 5, [1.0] * 5, nt=T + 1) == [A] * 4 and four(new, [0], [1.0], nt=-1) == [A] * 4
    assert four(new, [99], [float("nan")], o=(n_out,), K_=0) == [ST] * 4
    assert new.lbank_create(ctx.n) == 0 and new.lbank_load(0, ctx.fl) == 0
    # 5. before 6. before 8. (the fade's arguments, then the engine's state: no coefficients)
    assert four(new, [good], [1.0], o=(n_out,), which="pq") == [A] * 2 and four(new, [good], [1.0], i=(-1,), which="pq") == [A] * 2
    assert four(new, [good, good], [1.0, 1.0], n=2, o=(1, 1), i=(2, 2), which="pq") == [A] * 2   # the same pair twice
    assert four(new, [ctx.n], [0.0]) == [A] * 4 and four(new, [-2], [0.0]) == [A] * 4               # dead, and still refused
    assert four(new, [good, ctx.n], [1.0, 0.0], nt=2) == [A] * 4
    for bad in (float("nan"), float("inf"), float("-inf"), 1e39, -3.5e38):
        assert four(new, [good], [bad]) == [A] * 4, bad
    assert four(new, [-1], [float("inf")]) == [A] * 4                     # in a term without an entry too
    assert four(new, [ctx.never, ctx.n], [1.0, 0.0], nt=2, K_=0) == [A] * 4   # 5 behind 6 in the row: still 5
    assert four(new, [good, ctx.never], [1.0, 0.5], nt=2, K_=0) == [ST] * 4   # 6 before the fade's arguments
    assert four(new, [ctx.empty], [1.0], K_=0) == [ST] * 4
    assert four(new, [good], [1.0], K_=0, which="fq") == [A] * 2 and four(new, [good], [1.0], K_=(1 << 24) // L + 1, which="fq") == [A] * 2
    assert four(new, [good], [1.0], which="fpq") == [ST] * 3              # nothing to patch or to fade from
    assert not new.is_initialized()
    for wz in (0.0, -0.0, 1e-60):                                        # NOT refused: a dead term may name an empty entry
        assert four(new, [ctx.never], [wz], which="w") == [0]
    new.close()
    # on a running engine
    e, twin = ctx.engine(bfir), ctx.engine(bfir)
    assert e.set_bank_mix(M["whole"]) == 0 and twin.set_bank_mix(M["whole"]) == 0
    t = [0]

    def refused(got, want):
        assert got == want, (got, want)
        assert e.is_initialized() and e.fade_remaining() == twin.fade_remaining()
        _both(e, twin, x[t[0] * L:(t[0] + 1) * L], L, (1,))
        t[0] += 1

    def battery():
        refused(four(e, None, [1.0]), [A] * 4)
        refused(four(e, [good], [1.0], nt=T + 1), [A] * 4)
        refused(four(e, [good], [1.0], o=(n_out,), which="pq"), [A] * 2)
        refused(four(e, [good, good], [1.0, 1.0], n=2, o=(1, 1), i=(2, 2), which="pq"), [A] * 2)
        refused(four(e, [ctx.n], [0.0]), [A] * 4)
        refused(four(e, [good], [float("nan")]), [A] * 4)
        refused(four(e, [good], [1e39]), [A] * 4)
        refused(four(e, [ctx.never], [1.0]), [ST] * 4)
        refused(four(e, [good, ctx.empty], [1.0, 0.5], nt=2), [ST] * 4)
        refused(four(e, [good], [1.0], K_=0, which="fq"), [A] * 2)
        refused(e.set_coeff_bank_mix(M["whole"]), U)                      # the uniform group keeps refusing the kind
        refused(e.set_coeff_pairs_bank_mix([(0, 0)], [[(good, 1.0)]]), U)

    battery()
    assert e.fade_remaining() == 0
    mix = [(ctx.first_row[1], 0.75), (ctx.first_row[0], -2.0)]
    assert e.fade_to_pairs_bank_mix([(0, 0)], [mix], 60) == 0 and twin.fade_to_pairs_bank_mix([(0, 0)], [mix], 60) == 0
    refused(four(e, [good], [1.0], which="fpq"), [ST] * 3)               # one fade at a time, and the plain list waits
    battery()
    assert e.fade_remaining() == twin.fade_remaining() > 0
    for o, i in ctx.every:
        assert all(_row(e, ctx, k, o, i) == _row(twin, ctx, k, o, i) for k in range(len(blocks))), (o, i)
    e.close(); twin.close()


def test_a_weight_past_float_is_fine_in_double(orc, bfir):
    """1e39 is refused on an fp32 engine (above) and accepted on an fp64 one; 1e-60 is live there."""
    ctx = _ctx(orc, "9x2-f64")
    e = ctx.engine(bfir)
    a, b = ctx.first_row[1], ctx.first_row[0]
    rows = ctx.grid([[(a, 1e39), (b, -1e39)]] * len(ctx.every))
    assert e.set_bank_mix(rows) == 0
    _check_rows(e, ctx, ctx.every[:2], [[(a, 1e39), (b, -1e39)]] * 2, "1e39")
    assert e.set_pairs_bank_mix([(0, 0)], [[(a, 1e-60)]]) == 0
    _check_rows(e, ctx, [(0, 0)], [[(a, 1e-60)]], "1e-60")
    assert e.coeff_block(0, 0, 0, 0).any()
    assert e.set_pairs_bank_mix([(0, 0)], [[(ctx.never, 1e-60)]]) == bfir.ERR_STATE   # ... and so may not name an empty entry
    e.close()


# ---- 7. the grid's edge -----------------------------------------------------------------------------------------------------------
def test_every_row_of_a_64_by_64_matrix_in_one_call(orc, bfir):
    """WIDE of tests/test_lpairs_gpu.py, 64 -> 64 on two levels: a whole-matrix call with four terms, 4096 listed rows in one
    launch.  A sample of rows against the model on both levels, and output blocks against a twin that got the same mixes
    through 64 column calls."""
    s, L, blocks, ratios, n, _ = WIDE
    NE = 12
    Ls, D, _ = geo(WIDE)
    rng = np.random.default_rng(64)
    hs = _synth(orc, rng, [D[-1] - 1 - k if k % 3 else D[1] - 2 - k for k in range(NE)], s)
    cnt = [counts(WIDE, h.size) for h in hs]
    ents = rng.integers(0, NE, (n * n, T))
    wts = rng.choice([-1.0, 1.0], (n * n, T)) * 2.0 ** rng.uniform(-6.0, 2.0, (n * n, T))
    terms = [[(int(ents[r, j]), float(wts[r, j])) for j in range(T)] for r in range(n * n)]
    terms[n * n - 1][0] = (None, 1.0)
    terms[n + 1] = None
    grid = [terms[o * n:(o + 1) * n] for o in range(n)]
    e, twin = (_engine(bfir, None, None, cls="BrutefirMimoLevels", shape=WIDE) for _ in range(2))
    for eng in (e, twin):
        assert eng.lbank_create(NE) == 0 and eng.lbank_load(0, hs) == 0
    assert e.set_bank_mix(grid) == 0
    assert twin.set_bank([[0] * n] * n) == 0                                  # something to patch
    for i in range(n):
        assert twin.set_pairs_bank_mix([(o, i) for o in range(n)], [terms[o * n + i] for o in range(n)]) == 0
    reads = {en: [np.stack([e.lbank_read(en, k, b) for b in range(blocks[k])]) for k in range(2)] for en in range(NE)}
    for r in [0, 1, n - 1, n, n + 1, n * n - 1] + [int(v) for v in rng.integers(0, n * n, 30)]:
        for k in range(2):
            here = [(en, w) for en, w in (terms[r] or []) if en is not None and cnt[en][k] > 0]
            want, _ = mix_row([reads[en][k] for en, _ in here], [cnt[en][k] for en, _ in here], [w for _, w in here], _dt(s), blocks[k])
            want = want if want.shape[1] else np.zeros((blocks[k], 2 * Ls[k]), _dt(s))
            for eng in (e, twin):
                got = b"".join(eng.coeff_block(k, r // n, r % n, b).tobytes() for b in range(blocks[k]))
                assert got == want.tobytes(), (r, k)
    x = (np.random.default_rng(5).uniform(-1.0, 1.0, (8 * L, n)) / 64).astype(_dt(s))
    _both(e, twin, x, L, (1, 4, 3))
    e.close(); twin.close()


# ---- 8. offsets past 2^32 -----------------------------------------------------------------------------------------------------------
def test_a_level_store_beyond_4_gib(orc, bfir):
    """BIG of tests/test_lbank.py: 16385 entries, the tail level's last entry starts at byte 2^32.  One mix whose terms are
    entry 0 and entry 16384, exact against mix_row on both levels."""
    import torch
    L, blocks, ratios, s, n = BIG
    if torch.cuda.mem_get_info()[0] < 12 << 30:
        pytest.skip("less than 12 GiB of device memory free")
    shape = (s, L, blocks, ratios, 2, 2)
    Ls, D, _ = geo(shape)
    rng = np.random.default_rng(1024)
    hs = _synth(orc, rng, [D[-1] - 5, D[-1] - 4096 - 6], s)
    e = bfir.BrutefirMatrixLevels(L, blocks, ratios, s, 2, 2)
    assert e.lbank_create(n) == 0
    assert e.lbank_load(0, [hs[0]]) == 0 and e.lbank_load(n - 1, [hs[1]]) == 0
    cnt = {0: [4, 8], n - 1: [4, 7]}
    assert all(e.lbank_blocks(en, k) == c[k] for en, c in cnt.items() for k in range(2))
    terms = [(0, -0.375), (n - 1, 1.75)]
    assert e.set_bank_mix([[terms, None], [[(n - 1, 1.0)], terms[::-1]]]) == 0
    reads = {en: [np.stack([e.lbank_read(en, k, b) for b in range(blocks[k])]) for k in range(2)] for en in cnt}
    for (o, i), t in (((0, 0), terms), ((1, 0), [(n - 1, 1.0)]), ((1, 1), terms[::-1])):
        for k in range(2):
            want, c = mix_row([reads[en][k] for en, _ in t], [cnt[en][k] for en, _ in t], [w for _, w in t], _dt(s), blocks[k])
            assert c == max(cnt[en][k] for en, _ in t)
            got = b"".join(e.coeff_block(k, o, i, b).tobytes() for b in range(blocks[k]))
            assert got == want.tobytes(), (o, i, k)
    assert not any(e.coeff_block(k, 0, 1, b).any() for k in range(2) for b in range(blocks[k]))
    x = orc.synth_audio(rng, 3 * L, 2, np.float32)
    rc, y = e.run(x)
    assert rc == 0 and np.all(np.isfinite(y)) and np.abs(y).max() > 0
    e.close()
