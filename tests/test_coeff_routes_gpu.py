"""The coefficient sources of a uniform matrix or mimo engine lead to one set (csrc/engine.hip: set_coeff_uniform).  From the
same old set the same merged set is reached by five routes -- the whole matrix from taps, the listed pairs from taps, the
whole matrix from bank entries, the listed pairs from bank entries, the listed pairs as mixes of one term of weight 1 --
at once and as a fade over three blocks run to its end.  The routes differ in where their rows come from and in nothing else:
the filter stores and the outputs behind the change are the same bytes, during the fade the listed routes give one stream of
bytes and the whole-matrix routes another, and all of them lie within conftest.TOL of the float64 reference.

The shapes, the old set and the `mixed` list (coeff_blocks = max(1, B - 1): one path added, one removed, one shortened, one
lengthened) are test_pairs_gpu's.  The whole-matrix call from taps loads every filter with B partitions where the other routes
give the listed pairs coeff_blocks: there the partitions past the count are the transform of zero taps on one side and cleared
memory on the other, zeros of either sign and equal as numbers (test_pairs_gpu._same_store with cut).

scripts/coeff_routes_digest.py makes the same calls through plan() and route() and prints a digest of what they leave."""
import numpy as np
import pytest

from conftest import TOL
from test_fade import fade_weights
from test_mimo_gpu import _frames, _padded, _worst
from test_pairs import merge
from test_pairs_gpu import CASES, CUTS, _all_blocks, _cut, _old_rows, _pair_list, _same_store, _setup

pytestmark = pytest.mark.gpu

SHAPES = ("matrix-f64-grouped", "matrix-f32-direct", "mimo-f32-pair")
ROUTES = ("whole-taps", "pairs-taps", "whole-bank", "pairs-bank", "pairs-mix")
LISTED = ("pairs-taps", "pairs-bank", "pairs-mix")
WHOLE = ("whole-taps", "whole-bank")
FADE = 3


def plan(cid):
    """What every route of one shape shares, without a reference: test_pairs_gpu._setup(orc, cid, "mixed") gives the same
    sets and frames.  The bank: entry o n_in + i holds the old filter of (o, i) at B partitions, as the first set call loads
    it (no path: empty), entry n_out n_in + k the k-th listed filter at coeff_blocks (a removed path: empty)."""
    _, L, B, s, n_in, n_out, fmt, _ = CASES[cid]
    pre, pairs, filters, cb = _pair_list(cid, "mixed")
    first = _old_rows(cid)
    old = merge(first, pre[0], [_cut(h, L) for h in pre[1]])
    merged = merge(old, pairs, [_cut(h, cb * L) for h in filters])
    t0 = 2 * B + 3
    nb = t0 + sum(CUTS)
    assert 2 * t0 + FADE <= nb
    x = _frames(np.random.default_rng(len(cid) + 31 * len("mixed")), nb, L, n_in, fmt)
    x.setflags(write=False)
    n_old = n_out * n_in
    new_ent = [None if h is None else n_old + k for k, h in enumerate(filters)]
    ent = [[None if first[o][i] is None else o * n_in + i for i in range(n_in)] for o in range(n_out)]
    ent = merge(ent, pairs, new_ent)
    return dict(pre=pre, pairs=pairs, filters=filters, cb=cb, first=first, merged=merged, t0=t0, nb=nb, x=x, n_old=n_old,
                new_ent=new_ent, ent=ent)


def start(bfir, cid, P):
    """An engine on the old set, reached as test_pairs_gpu._start reaches it, with the bank loaded."""
    cls, L, B, s, n_in, n_out, fmt, _ = CASES[cid]
    e = getattr(bfir, cls)(L, B, s, n_in, n_out, fmt, fmt)
    assert e.set_coeff(_padded(P["first"], B * L)) == 0
    assert e.set_coeff_pairs(P["pre"][0], P["pre"][1], coeff_blocks=1) == 0
    assert e.bank_create(P["n_old"] + len(P["filters"])) == 0
    assert e.bank_load(0, [h for r in _padded(P["first"], B * L) for h in r], coeff_blocks=B) == 0
    assert e.bank_load(P["n_old"], P["filters"], coeff_blocks=P["cb"]) == 0
    return e


def change(e, cid, P, name, K):
    """The call of route `name` to the merged set: at once (K is None) or faded over K blocks."""
    _, L, B, s, n_in, n_out, fmt, _ = CASES[cid]
    fade = () if K is None else (K,)
    if name == "whole-taps":
        return (e.set_coeff if K is None else e.set_coeff_fade)(_padded(P["merged"], B * L), *fade)
    if name == "pairs-taps":
        return (e.set_coeff_pairs if K is None else e.set_coeff_pairs_fade)(P["pairs"], P["filters"], *fade, coeff_blocks=P["cb"])
    if name == "whole-bank":
        return (e.set_coeff_bank if K is None else e.set_coeff_bank_fade)(P["ent"], *fade)
    if name == "pairs-bank":
        return (e.set_coeff_pairs_bank if K is None else e.set_coeff_pairs_bank_fade)(P["pairs"], P["new_ent"], *fade)
    assert name == "pairs-mix"
    terms = [None if en is None else [(en, 1.0)] for en in P["new_ent"]]
    return (e.set_coeff_pairs_bank_mix if K is None else e.set_coeff_pairs_bank_mix_fade)(P["pairs"], terms, *fade)


def route(bfir, cid, P, name, K):
    """One engine through one route: t0 blocks on the old set, the change, (a fade: its K blocks,) the store, t0 more blocks.
    Returns the outputs before, during (a fade, else empty) and behind the change, and the store behind it."""
    _, L, B, s, n_in, n_out, fmt, _ = CASES[cid]
    x, t0 = P["x"], P["t0"]
    k = K or 0
    e = start(bfir, cid, P)
    rc0, before = e.run(x[:t0 * L])
    assert rc0 == 0 and change(e, cid, P, name, K) == 0
    assert e.is_initialized() and e.fade_remaining() == k
    during = before[:0]
    if K:
        rc1, during = e.run(x[t0 * L:(t0 + k) * L])
        assert rc1 == 0 and e.fade_remaining() == 0
    store = _all_blocks(e, cid)
    rc2, behind = e.run(x[(t0 + k) * L:(2 * t0 + k) * L])
    assert rc2 == 0
    e.close()
    return dict(before=before, during=during, behind=behind, store=store)


@pytest.mark.parametrize("K", (None, FADE), ids=("plain", "fade"))
@pytest.mark.parametrize("cid", SHAPES)
def test_five_routes_reach_one_set(orc, bfir, cid, K):
    _, L, B, s, n_in, n_out, fmt, _ = CASES[cid]
    S = _setup(orc, cid, "mixed")
    P = plan(cid)
    assert P["x"].tobytes() == S["x"].tobytes() and P["t0"] == S["t0"] and 2 * B + 3 == P["t0"]
    t0, k = P["t0"], K or 0
    got = {name: route(bfir, cid, P, name, K) for name in ROUTES}
    base = got["pairs-taps"]
    for name in ROUTES:
        r = got[name]
        assert r["before"].tobytes() == base["before"].tobytes(), name
        assert _same_store(r["store"], base["store"], cut=name == "whole-taps"), name     # every (o, i, block) of coeff_block
        assert r["behind"].tobytes() == base["behind"].tobytes(), name                    # the next 2 B + 3 blocks
    for group in (LISTED, WHOLE) if K else ():
        for name in group[1:]:
            assert got[name]["during"].tobytes() == got[group[0]]["during"].tobytes(), name
    # the float64 reference: the old set's up to the change, the blend in the fade, the merged set's behind it
    w = np.zeros(P["nb"] * L) if K is None else fade_weights(L, P["nb"], t0, K)
    if K is None:
        w[t0 * L:] = 1.0
    n = (2 * t0 + k) * L
    want = (S["refs"]["old"][0] * (1.0 - w[:, None]) + S["refs"]["merged"][0] * w[:, None])[:n]
    for name in ROUTES:
        y = np.concatenate([got[name][part] for part in ("before", "during", "behind")])
        err_fade = _worst(y[t0 * L:(t0 + k) * L], want[t0 * L:(t0 + k) * L], L) if K else 0.0
        err = _worst(y, want, L)
        print("%s %s %s: worst block %.3g (in the fade %.3g) against the float64 reference, TOL %.0e" %
              (cid, "plain" if K is None else "fade", name, err, err_fade, TOL[s]))
        assert err_fade <= TOL[s] and err <= TOL[s], name
