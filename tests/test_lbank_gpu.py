"""Coefficient banks on multi-level matrix and mimo engines on the GPU (bfir_engine_levels_bank_*,
bfir_engine_set_coeff_matrix_levels_bank, _bank_fade, _pairs_bank, _pairs_bank_fade; the lbank_* methods, set_bank,
fade_to_rows_bank, set_pairs_bank and fade_to_pairs_bank of BrutefirMatrixLevels) and k_lbank_gather (csrc/lbank.hip).

Every comparison with a twin engine is of BYTES: the twin gets the same filters as host taps through set_coeff, fade_to_rows,
set_pairs and fade_to_pairs.  Compared are lbank_read against coeff_block, the stores over the partitions below each pair's
count (and zeros past them), and every output block.  Runs are at least test_levels_gpu._nb blocks long, so every delay line
and ring wraps, with set_chunk(3) among them; the call cuts are test_lpairs_gpu.CUTS.  The shapes are those of
tests/test_lpairs.py and tests/test_lbank.py, which holds the new ones to their conditions without a GPU.

The one tolerance of the file is conftest.TOL, per block and output (size_matrix.block_errors), for the fades of entries
loaded with different scales: no single call with taps gives those, so they are held to the float64 blend of two
test_mimo_levels.wide_reference runs with test_fade.fade_weights."""
import ctypes as C

import numpy as np
import pytest

from conftest import TOL
from test_fade import fade_weights
from test_lbank import BIG, BOUNDARY_COUNTS, KINDS, NEW_SHAPES
from test_levels_gpu import _nb
from test_lpairs import A_F, LISTS, SHAPES, counts, geo, merge
from test_lpairs_gpu import CUTS, _dt, _engine, _lv, _same_store, _setup, _synth
from test_mimo_gpu import _run_cut, _worst
from test_mimo_levels import wide_reference

pytestmark = pytest.mark.gpu


# ---- the bank of a (shape, list) of tests/test_lpairs.py ------------------------------------------------------------------------
class Banked:
    """Entries 0 .. P - 1: the old filters, entry o n_in + i for h_{o,i} (a pair without a path: loaded as None); then the
    list's new filters (a removed path: loaded as None); then one entry that is never loaded."""

    def __init__(self, S):
        self.S = S
        n_in = S["shape"][4]
        self.flat = [h for r in S["old"] for h in r] + list(S["filters"])
        P = len(self.flat) - len(S["filters"])
        self.n = len(self.flat) + 1
        self.empty = next(k for k, h in enumerate(self.flat) if h is None)   # an entry loaded as None
        self.old = [[None if h is None else o * n_in + i for i, h in enumerate(r)] for o, r in enumerate(S["old"])]
        self.new = [None if h is None else P + k for k, h in enumerate(S["filters"])]
        self.merged = merge(self.old, S["pairs"], self.new)

    def load(self, e):
        assert e.lbank_create(self.n) == 0 and e.lbank_entries() == self.n
        assert e.lbank_load(0, self.flat) == 0

    def engine(self, bfir, name, chunk=3, set_old=True):
        """An engine of the shape with the bank loaded and, from the bank alone, the old set."""
        e = _engine(bfir, name, None, chunk=chunk)
        self.load(e)
        if set_old:
            assert not e.is_initialized()
            assert e.set_bank(self.old) == 0 and e.is_initialized()
        return e


def _both(e, twin, x, L, cuts):
    """The same blocks through both engines in the same cuts: the same bytes."""
    rcs, y = _run_cut(e, x, L, cuts)
    rct, yt = _run_cut(twin, x, L, cuts)
    assert rcs == rct == [0] * len(cuts)
    assert y.tobytes() == yt.tobytes()
    return y


def _cuts(x, L, start):
    """CUTS and the rest of the blocks of x behind block `start`."""
    rest = x.shape[0] // L - start - sum(CUTS)
    assert rest >= 1
    return CUTS + (rest,)


# ---- 1. the entries ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_entries_are_the_twins_spectra(orc, bfir, name):
    S = _setup(orc, name, "mixed")
    shape = S["shape"]
    s, L, blocks, ratios, n_in, n_out = shape
    Ls = geo(shape)[0]
    bk = Banked(S)
    e, twin = bk.engine(bfir, name, set_old=False), _engine(bfir, name, S["old"])
    sample = set(S["pairs"]) | {(o, i) for o in (0, n_out - 1) for i in (2 % n_in, n_in - 2, n_in - 1)}
    for o, i in sorted(sample):
        h, en = S["old"][o][i], o * n_in + i
        cnt = counts(shape, None if h is None else h.size)
        assert e.lbank_length(en) == (0 if h is None else h.size)
        for k in range(len(blocks)):
            assert e.lbank_blocks(en, k) == cnt[k]
            for b in range(blocks[k]):
                got = e.lbank_read(en, k, b)
                assert got.size == 2 * Ls[k]
                if b < cnt[k]:
                    assert got.tobytes() == twin.coeff_block(k, o, i, b).tobytes(), (o, i, k, b)
                else:
                    assert not got.any(), (o, i, k, b)
    assert any(h is None for h in bk.flat)                                # an entry loaded as None, and the one never loaded
    for en in (bk.empty, bk.n - 1):
        assert e.lbank_length(en) == 0 and all(e.lbank_blocks(en, k) == 0 for k in range(len(blocks)))
        assert not any(e.lbank_read(en, k, b).any() for k in range(len(blocks)) for b in range(blocks[k]))
    assert not e.is_initialized()                                        # a bank alone sets no filters
    e.close(); twin.close()


# ---- 2. the plain calls -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", LISTS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_plain_calls(orc, bfir, name, kind):
    """set_bank on an engine without filters, A_F blocks, set_pairs_bank, the rest in CUTS."""
    S = _setup(orc, name, kind)
    shape, x = S["shape"], S["x"]
    L = shape[1]
    bk = Banked(S)
    e, twin = bk.engine(bfir, name), _engine(bfir, name, S["old"])
    every = [(o, i) for o in range(shape[5]) for i in range(shape[4])]
    _same_store(e, twin, shape, S["old"], every[::7])
    _both(e, twin, x[:A_F * L], L, (A_F,))
    assert e.set_pairs_bank(S["pairs"], bk.new) == 0
    assert twin.set_pairs(S["pairs"], S["filters"]) == 0
    assert e.is_initialized() and e.fade_remaining() == 0
    _same_store(e, twin, shape, S["merged"], S["pairs"])
    _both(e, twin, x[A_F * L:], L, _cuts(x, L, A_F))
    e.close(); twin.close()


# ---- 3. the fades -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", LISTS + ("whole",))
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_fades(orc, bfir, name, kind):
    """fade_to_pairs_bank against fade_to_pairs for every list; `whole`: fade_to_rows_bank to the mixed list's merged set
    against fade_to_rows."""
    whole = kind == "whole"
    S = _setup(orc, name, "mixed" if whole else kind)
    shape, x, K = S["shape"], S["x"], S["K"]
    L = shape[1]
    bk = Banked(S)
    e, twin = bk.engine(bfir, name), _engine(bfir, name, S["old"])
    _both(e, twin, x[:A_F * L], L, (A_F,))
    if whole:
        assert e.fade_to_rows_bank(bk.merged, K) == 0 and twin.fade_to_rows(S["merged"], K) == 0
    else:
        assert e.fade_to_pairs_bank(S["pairs"], bk.new, K) == 0 and twin.fade_to_pairs(S["pairs"], S["filters"], K) == 0
    assert e.fade_remaining() == K
    _both(e, twin, x[A_F * L:], L, _cuts(x, L, A_F))
    assert e.fade_remaining() == 0
    _same_store(e, twin, shape, S["merged"], S["pairs"])                 # the merged set is active on every level
    e.close(); twin.close()


def test_one_entry_named_for_several_pairs(orc, bfir):
    name = "9x3"
    S = _setup(orc, name, "mixed")
    shape, x, K = S["shape"], S["x"], S["K"]
    L, n_in = shape[1], shape[4]
    bk = Banked(S)
    e, twin = bk.engine(bfir, name), _engine(bfir, name, S["old"])
    _both(e, twin, x[:A_F * L], L, (A_F,))
    pairs, en = [(0, 2), (2, 3), (1, 4), (2, 8)], bk.old[0][0]
    h = S["old"][0][0]
    assert e.set_pairs_bank(pairs, [en] * 4) == 0 and twin.set_pairs(pairs, [h] * 4) == 0
    _same_store(e, twin, shape, merge(S["old"], pairs, [h] * 4), pairs)
    _both(e, twin, x[A_F * L:(A_F + 4) * L], L, (1, 3))
    pairs2, en2 = [(1, 1), (0, 5), (2, 2)], bk.old[1][0]
    h2 = S["old"][1][0]
    assert e.fade_to_pairs_bank(pairs2, [en2] * 3, K) == 0 and twin.fade_to_pairs(pairs2, [h2] * 3, K) == 0
    _both(e, twin, x[(A_F + 4) * L:], L, (x.shape[0] // L - A_F - 4,))
    e.close(); twin.close()


# ---- 4. state ---------------------------------------------------------------------------------------------------------------------
def test_a_plain_bank_call_cuts_the_fade_and_the_plain_list_waits(orc, bfir):
    name = "9x3"
    S = _setup(orc, name, "mixed")
    shape, x, K = S["shape"], S["x"], S["K"]
    L = shape[1]
    bk = Banked(S)
    e, twin = bk.engine(bfir, name), _engine(bfir, name, S["old"])
    _both(e, twin, x[:A_F * L], L, (A_F,))
    assert e.fade_to_pairs_bank(S["pairs"], bk.new, K) == 0 and twin.fade_to_pairs(S["pairs"], S["filters"], K) == 0
    assert e.set_pairs_bank(S["pairs"], bk.new) == bfir.ERR_STATE        # pending
    _both(e, twin, x[A_F * L:(A_F + 2) * L], L, (2,))
    assert e.set_pairs_bank(S["pairs"], bk.new) == bfir.ERR_STATE and e.fade_remaining() == K - 2        # running
    assert e.fade_to_pairs_bank(S["pairs"], bk.new, K) == bfir.ERR_STATE and e.fade_to_rows_bank(bk.merged, K) == bfir.ERR_STATE
    assert e.set_bank(bk.merged) == 0 and e.fade_remaining() == 0        # a hard cut, the twin's
    assert twin.set_coeff(S["merged"]) == 0
    _same_store(e, twin, shape, S["merged"], S["pairs"])
    _both(e, twin, x[(A_F + 2) * L:], L, (x.shape[0] // L - A_F - 2,))
    assert e.set_pairs_bank(S["pairs"][:1], bk.new[:1]) == 0             # no fade is left: the plain list is taken
    e.close(); twin.close()


@pytest.mark.parametrize("whole", (False, True), ids=("pairs", "whole"))
def test_reset_during_the_fade_leaves_the_new_set_active(orc, bfir, whole):
    name = "9x3"
    S = _setup(orc, name, "mixed")
    shape, x, K = S["shape"], S["x"], S["K"]
    L = shape[1]
    bk = Banked(S)
    e = bk.engine(bfir, name)
    assert e.run(x[:A_F * L])[0] == 0
    assert (e.fade_to_rows_bank(bk.merged, K) if whole else e.fade_to_pairs_bank(S["pairs"], bk.new, K)) == 0
    assert e.run(x[A_F * L:(A_F + 2) * L])[0] == 0 and e.fade_remaining() == K - 2
    e.reset()
    assert e.fade_remaining() == 0 and e.is_initialized()
    fresh = _engine(bfir, name, S["merged"])
    _same_store(e, fresh, shape, S["merged"], S["pairs"])
    _both(e, fresh, x, L, (x.shape[0] // L,))
    e.close(); fresh.close()


def test_a_level_newly_reached_a_level_left_and_the_fade_refused_per_level(orc, bfir):
    name = "9x3"
    S = _setup(orc, name, "mixed")
    shape, x, K = S["shape"], S["x"], S["K"]
    s, L, blocks, ratios, n_in, n_out = shape
    _, D, _ = geo(shape)
    short = [[None if h is None else h[:min(h.size, D[2] - 3)] for h in row] for row in S["old"]]
    long_one = np.ascontiguousarray(S["filters"][1])
    assert long_one.size > D[2]
    e, twin = _engine(bfir, name, None), _engine(bfir, name, short)
    P = n_in * n_out
    assert e.lbank_create(P + 1) == 0 and e.lbank_load(0, [h for r in short for h in r] + [long_one]) == 0
    assert e.lbank_blocks(0, 2) == 0 and e.lbank_blocks(P, 2) > 0
    ent = [[None if h is None else o * n_in + i for i, h in enumerate(r)] for o, r in enumerate(short)]
    assert e.set_bank(ent) == 0
    _both(e, twin, x[:A_F * L], L, (A_F,))
    # the last level is not running: neither fade may reach it
    assert e.fade_to_pairs_bank([(0, 0)], [P], K) == bfir.ERR_UNSUPPORTED
    assert e.fade_to_rows_bank(merge(ent, [(0, 0)], [P]), K) == bfir.ERR_UNSUPPORTED
    assert e.fade_remaining() == 0 and e.is_initialized()
    _both(e, twin, x[A_F * L:(A_F + 3) * L], L, (3,))
    # the plain list starts the level ...
    assert e.set_pairs_bank([(0, 0)], [P]) == 0 and twin.set_pairs([(0, 0)], [long_one]) == 0
    _same_store(e, twin, shape, merge(short, [(0, 0)], [long_one]), [(0, 0)])
    n1 = A_F + 3 + 6
    assert n1 + 9 <= x.shape[0] // L
    _both(e, twin, x[(A_F + 3) * L:n1 * L], L, (1, 5))
    # ... and the whole-matrix call leaves it again
    assert e.set_bank(ent) == 0 and twin.set_coeff(short) == 0
    _both(e, twin, x[n1 * L:(n1 + 3) * L], L, (1, 2))
    # ... as does a list
    assert e.set_pairs_bank([(0, 0)], [P]) == 0 and twin.set_pairs([(0, 0)], [long_one]) == 0
    _both(e, twin, x[(n1 + 3) * L:(n1 + 5) * L], L, (2,))
    assert e.set_pairs_bank([(0, 0)], [0]) == 0 and twin.set_pairs([(0, 0)], [short[0][0]]) == 0
    _both(e, twin, x[(n1 + 5) * L:], L, (x.shape[0] // L - n1 - 5,))
    e.close(); twin.close()


def test_loading_over_an_entry_in_use_and_destroying_the_bank_change_nothing(orc, bfir):
    name = "9x3"
    S = _setup(orc, name, "mixed")
    shape, x, K = S["shape"], S["x"], S["K"]
    L = shape[1]
    bk = Banked(S)
    e, twin = bk.engine(bfir, name), _engine(bfir, name, S["old"])
    _both(e, twin, x[:3 * L], L, (3,))
    assert e.lbank_load(0, [S["old"][1][1], None]) == 0                   # entries 0 and 1 are h_{0,0} and h_{0,1} of the active set
    assert e.lbank_length(0) == S["old"][1][1].size and e.lbank_length(1) == 0
    _same_store(e, twin, shape, S["old"], [(0, 0), (0, 1)])
    _both(e, twin, x[3 * L:A_F * L], L, (A_F - 3,))
    assert e.fade_to_pairs_bank(S["pairs"], bk.new, K) == 0 and twin.fade_to_pairs(S["pairs"], S["filters"], K) == 0
    _both(e, twin, x[A_F * L:(A_F + 2) * L], L, (2,))
    assert e.lbank_destroy() == 0 and e.lbank_entries() == 0 and e.fade_remaining() == K - 2
    assert e.set_pairs_bank([(0, 0)], [0]) == bfir.ERR_STATE and e.lbank_destroy() == 0
    with pytest.raises(bfir.BfirError):
        e.lbank_read(0, 0, 0)
    _both(e, twin, x[(A_F + 2) * L:], L, (x.shape[0] // L - A_F - 2,))
    _same_store(e, twin, shape, S["merged"], S["pairs"])
    assert e.lbank_create(2) == 0 and e.lbank_length(1) == 0              # and a new one may be made
    e.close(); twin.close()


# ---- 5. how the blocks arrive -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_the_bytes_do_not_depend_on_set_chunk_or_on_how_the_blocks_arrive(orc, bfir, name):
    S = _setup(orc, name, "mixed")
    shape, x, K = S["shape"], S["x"], S["K"]
    L = shape[1]
    nb = x.shape[0] // L
    bk = Banked(S)
    out = {}
    for how, chunk, cuts in (("cuts", None, _cuts(x, L, A_F)), ("one", None, (nb - A_F,)), ("chunk3", 3, (nb - A_F,)),
                             ("blocks", None, (1,) * (nb - A_F))):
        e = bk.engine(bfir, name, chunk=chunk)
        rc, a = e.run(x[:A_F * L]); assert rc == 0
        assert e.fade_to_pairs_bank(S["pairs"], bk.new, K) == 0
        rcs, b = _run_cut(e, x[A_F * L:], L, cuts)
        assert rcs == [0] * len(cuts) and e.fade_remaining() == 0
        out[how] = np.concatenate([a, b]).tobytes()
        e.close()
    assert out["cuts"] == out["one"] == out["chunk3"] == out["blocks"]


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_come_in_the_documented_order_and_change_nothing(orc, bfir):
    name = "9x3"
    S = _setup(orc, name, "mixed")
    shape, x, K = S["shape"], S["x"], S["K"]
    s, L, blocks, ratios, n_in, n_out = shape
    _, D, _ = geo(shape)
    lib = bfir.load()
    A, U, ST, CO = bfir.ERR_ARG, bfir.ERR_UNSUPPORTED, bfir.ERR_STATE, bfir.ERR_COEFF
    P = n_in * n_out
    ia = lambda v: None if v is None else (C.c_int * max(1, len(v)))(*v)
    w_plain = lambda eng, ents: lib.bfir_engine_set_coeff_matrix_levels_bank(eng.handle, ia(ents))
    w_fade = lambda eng, ents, K_=2: lib.bfir_engine_set_coeff_matrix_levels_bank_fade(eng.handle, ia(ents), K_)
    p_plain = lambda eng, n, o, i, en: lib.bfir_engine_set_coeff_matrix_levels_pairs_bank(eng.handle, n, ia(o), ia(i), ia(en))
    p_fade = lambda eng, n, o, i, en, K_=2: lib.bfir_engine_set_coeff_matrix_levels_pairs_bank_fade(eng.handle, n, ia(o), ia(i), ia(en), K_)

    def four(eng, code, ents=None, n=1, o=(0,), i=(0,), en=(0,), K_=2, which="wfpq"):
        ents = [0] * P if ents is None else ents
        call = dict(w=lambda: w_plain(eng, ents), f=lambda: w_fade(eng, ents, K_), p=lambda: p_plain(eng, n, o, i, en),
                    q=lambda: p_fade(eng, n, o, i, en, K_))
        got = {c: call[c]() for c in which}                              # only the calls asked for are made
        assert all(v == code for v in got.values()), (got, code)

    twin = _engine(bfir, name, S["old"])
    rc, want = twin.run(x); assert rc == 0
    twin.close()
    h = np.ascontiguousarray(S["filters"][1])
    # 1. the kind, before everything: the uniform kinds and a diagonal multi-level engine have none of the group
    others = (bfir.BrutefirMimo(L, blocks[0], s, n_in, n_out), bfir.BrutefirLevels(L, blocks, ratios, s, 2))
    for other in others:
        assert p_fade(other, 0, None, None, None, 0) == U and w_fade(other, None, 0) == U
        assert p_plain(other, 0, None, None, None) == U and w_plain(other, None) == U
        assert other.handle and lib.bfir_engine_levels_bank_create(other.handle, 0) == U
        assert lib.bfir_engine_levels_bank_destroy(other.handle) == U and lib.bfir_engine_levels_bank_entries(other.handle) == U
        assert lib.bfir_engine_levels_bank_length(other.handle, 0) == U and lib.bfir_engine_levels_bank_blocks(other.handle, 0, 0) == U
        assert lib.bfir_engine_levels_bank_load(other.handle, 0, 0, None, None, 1.0) == U
        assert lib.bfir_engine_levels_bank_read(other.handle, 0, 0, 0, None) == U
        other.close()
    # the bank calls' own arguments
    new = _engine(bfir, name, None)
    ptr = (C.c_void_p * 1)(h.ctypes.data)
    load = lambda first, n, p, lens, sc=1.0: lib.bfir_engine_levels_bank_load(new.handle, first, n, p, ia(lens), sc)
    assert new.lbank_create(0) == A and new.lbank_entries() == 0 and new.lbank_length(0) == A
    assert load(0, 1, None, [4]) == A and load(0, 1, ptr, None) == A and load(0, 0, ptr, [4]) == A and load(-1, 1, ptr, [4]) == A
    assert load(0, 1, ptr, [-1]) == A and load(0, 1, ptr, [D[-1] + 1]) == A
    assert load(0, 1, ptr, [4]) == ST                                    # no bank: before the range
    # 2. null arguments and n_pairs < 1 come before the missing bank, 3. the missing bank before the list
    four(new, A, ents=None, o=None, which="pq"); four(new, A, i=None, which="pq"); four(new, A, en=None, which="pq")
    four(new, A, n=0, which="pq")
    assert w_plain(new, None) == A and w_fade(new, None) == A
    four(new, ST, o=(n_out,), en=(99,), K_=0)
    assert new.lbank_create(3) == 0 and new.lbank_create(3) == ST
    assert load(2, 2, (C.c_void_p * 2)(h.ctypes.data, h.ctypes.data), [4, 4]) == A   # past the bank
    nan = h.copy(); nan[-1] = np.nan
    assert new.lbank_load(0, [h, nan]) == CO and new.lbank_length(0) == 0  # nothing was uploaded
    assert new.lbank_load(0, [h]) == 0 and new.lbank_length(0) == h.size
    dst = np.zeros(2 * L * 4, _dt(s))
    rd = lambda en, k, b, p=dst.ctypes.data: lib.bfir_engine_levels_bank_read(new.handle, en, k, b, p)
    assert rd(0, 0, 0, None) == A and rd(0, len(blocks), 0) == A and rd(0, -1, 0) == A and rd(0, 0, blocks[0]) == A and rd(0, 1, -1) == A
    assert rd(3, 0, 0) == A and rd(-1, 0, 0) == A and rd(0, 0, 0) == 0
    assert new.lbank_blocks(0, len(blocks)) == A and new.lbank_blocks(3, 0) == A
    # 4. the list, before 5. an empty entry, before 6. the fade's arguments, before 7. the engine's state (no coefficients)
    four(new, A, ents=[0] * (P - 1) + [3], o=(n_out,), en=(1,), K_=0)
    four(new, A, ents=[0] * (P - 1) + [-2], n=2, o=(1, 1), i=(2, 2), en=(0, 1), K_=0)
    four(new, A, i=(n_in,), which="pq"); four(new, A, o=(-1,), which="pq"); four(new, A, en=(3,), which="pq")
    four(new, ST, ents=[0] * (P - 1) + [1], en=(1,), K_=0)               # entry 1 is empty
    four(new, A, K_=0, which="fq"); four(new, A, K_=(1 << 24) // L + 1, which="fq")
    four(new, ST, which="fpq")                                           # nothing to patch or to fade from
    assert not new.is_initialized()
    new.close()
    # on a running engine: nothing of the above, and neither the per-level refusal, changes a byte
    bk = Banked(S)
    e = bk.engine(bfir, name)
    rc, a = e.run(x[:A_F * L]); assert rc == 0
    keep = _engine(bfir, name, S["old"])
    four(e, A, ents=[0] * (P - 1) + [bk.n], o=(n_out,))
    four(e, A, n=2, o=(1, 1), i=(2, 2), en=(0, 0), which="pq")
    four(e, ST, ents=[0] * (P - 1) + [bk.n - 1], en=(bk.n - 1,))         # the entry never loaded
    four(e, ST, ents=[bk.empty] * P, en=(bk.empty,))   # the entry loaded as None
    four(e, A, K_=0, which="fq")
    assert e.set_coeff_bank(bk.old) == U and e.set_coeff_pairs_bank([(0, 0)], [0]) == U and e.bank_create(2) == U   # the uniform group
    assert e.is_initialized() and e.fade_remaining() == 0
    _same_store(e, keep, shape, S["old"], S["pairs"])
    rc, b = e.run(x[A_F * L:])
    assert rc == 0 and np.concatenate([a, b]).tobytes() == want.tobytes()
    e.close(); keep.close()


# ---- 7. entries loaded with different scales ----------------------------------------------------------------------------------------
SCALES = (1.0, -0.5)                                                     # powers of two: h * scale is exact in either precision


def _scaled_bank(e, S):
    """The old filters at SCALES[0] in entries 0 .. P - 1, then the list's new ones, every second at SCALES[1]."""
    flat = [h for r in S["old"] for h in r]
    assert e.lbank_create(len(flat) + len(S["filters"])) == 0 and e.lbank_load(0, flat, scale=SCALES[0]) == 0
    for k, h in enumerate(S["filters"]):
        assert e.lbank_load(len(flat) + k, [h], scale=SCALES[k % 2]) == 0
    return [None if h is None else len(flat) + k for k, h in enumerate(S["filters"])]


@pytest.mark.parametrize("name", ["9x3", "9x2-f64"])
def test_entries_of_different_scales_in_one_plain_call(orc, bfir, name):
    """The twin is changed once per distinct scale: set_coeff for the first group and set_pairs for the other (whole matrix),
    or set_pairs once per scale (the list)."""
    S = _setup(orc, name, "mixed")
    shape, x = S["shape"], S["x"]
    L, n_in = shape[1], shape[4]
    pairs, filters = S["pairs"], S["filters"]
    grp = [[k for k in range(len(pairs)) if k % 2 == g] for g in (0, 1)]
    e, twin = _engine(bfir, name, None), _engine(bfir, name, S["old"])
    new = _scaled_bank(e, S)
    old = [[None if h is None else o * n_in + i for i, h in enumerate(r)] for o, r in enumerate(S["old"])]
    assert e.set_bank(old) == 0
    _both(e, twin, x[:A_F * L], L, (A_F,))
    assert e.set_pairs_bank(pairs, new) == 0
    for g in (0, 1):
        assert twin.set_pairs([pairs[k] for k in grp[g]], [filters[k] for k in grp[g]], scale=SCALES[g]) == 0
    _same_store(e, twin, shape, S["merged"], pairs)
    n1 = A_F + 3
    _both(e, twin, x[A_F * L:n1 * L], L, (1, 2))
    # the whole matrix: the merged set again on engines that run something else
    assert e.set_bank(old) == 0 and twin.set_coeff(S["old"]) == 0
    _both(e, twin, x[n1 * L:(n1 + 1) * L], L, (1,))
    assert e.set_bank(merge(old, pairs, new)) == 0
    at1 = [pairs[k] for k in grp[1]]
    assert twin.set_coeff(merge(S["merged"], at1, [None] * len(at1)), scale=SCALES[0]) == 0
    assert twin.set_pairs(at1, [filters[k] for k in grp[1]], scale=SCALES[1]) == 0
    _same_store(e, twin, shape, S["merged"], pairs)
    _both(e, twin, x[(n1 + 1) * L:], L, (x.shape[0] // L - n1 - 1,))
    e.close(); twin.close()


@pytest.mark.parametrize("whole", (False, True), ids=("pairs", "whole"))
@pytest.mark.parametrize("name", ["9x3", "9x2-f64"])
def test_entries_of_different_scales_in_one_fade(orc, bfir, name, whole):
    """Against the float64 blend of the references of the old set and of the merged set with every filter scaled as loaded,
    per block and output at conftest.TOL."""
    S = _setup(orc, name, "mixed")
    shape, x, K = S["shape"], S["x"], S["K"]
    s, L, n_in = shape[0], shape[1], shape[4]
    pairs = S["pairs"]
    e = _engine(bfir, name, None)
    new = _scaled_bank(e, S)
    old = [[None if h is None else o * n_in + i for i, h in enumerate(r)] for o, r in enumerate(S["old"])]
    assert e.set_bank(old) == 0
    rc, a = e.run(x[:A_F * L]); assert rc == 0
    assert (e.fade_to_rows_bank(merge(old, pairs, new), K) if whole else e.fade_to_pairs_bank(pairs, new, K)) == 0
    rcs, b = _run_cut(e, x[A_F * L:], L, _cuts(x, L, A_F))
    assert not any(rcs) and e.fade_remaining() == 0
    e.close()
    scaled = [None if h is None else (h * _dt(s)(SCALES[k % 2])).astype(_dt(s)) for k, h in enumerate(S["filters"])]
    ref_new = wide_reference(orc, L, s, merge(S["old"], pairs, scaled), x)
    nb = x.shape[0] // L
    w = fade_weights(L, nb, A_F, K)[:, None]
    want = S["refs"][0] * (1.0 - w) + ref_new * w
    err = _worst(np.concatenate([a, b]), want, L)
    print("%s %s: worst block %.3g against the float64 blend (tol %g)" % (name, "whole" if whole else "pairs", err, TOL[s]))
    assert err <= TOL[s]


# ---- 8. the rows around the gather's span -------------------------------------------------------------------------------------------
NEW_CASES = [(k, z, s) for k in sorted(KINDS) for z in sorted(NEW_SHAPES) for s in (4, 8)]
NEW_K = 5


def _new_lengths(size):
    """Tap counts of the entries of a new shape; the first reaches the last partition of the last level."""
    L, blocks, ratios = NEW_SHAPES[size]
    shape = (4, L, blocks, ratios, 1, 1)
    Ls, D, _ = geo(shape)
    if size == "boundary":
        lens = [D[-1] - 1] + [c * L - 5 + j for j, c in enumerate(BOUNDARY_COUNTS)] + [D[1] + Ls[1] + 7, D[-1] - 9, 3, D[1]]
        assert [counts(shape, n)[0] for n in lens[1:3]] == list(BOUNDARY_COUNTS) and counts(shape, lens[1])[1] == 0
    else:
        lens = [D[-1] - 1, 2 * L - 7, D[1] + Ls[1] + 5, D[-1] - 3, 4 * L + 100, D[1] + 1]
    return lens


_NEW = {}


def _new_setup(orc, kind, size, s):
    if (kind, size, s) not in _NEW:
        (cls, n_in, n_out), (L, blocks, ratios) = KINDS[kind], NEW_SHAPES[size]
        shape = (s, L, blocks, ratios, n_in, n_out)
        rng = np.random.default_rng(sum((kind + size).encode()) + s)
        filters = _synth(orc, rng, _new_lengths(size), s)
        nb = max(_nb(_lv(shape)), A_F + sum(CUTS) + 1 + NEW_K + geo(shape)[2][-1] + 3)
        x = orc.synth_audio(rng, nb * L, n_in, _dt(s))
        x.setflags(write=False)
        n = len(filters)
        every = [(o, i) for o in range(n_out) for i in range(n_in)]
        old = [[None if (o, i) == (1, 0) else (o * n_in + i) % n for i in range(n_in)] for o in range(n_out)]
        pairs = every[1::2] if len(every) > 8 else every[1:]
        new = [None if k == 2 else (3 * k + 1) % n for k in range(len(pairs))]
        _NEW[(kind, size, s)] = dict(cls=cls, shape=shape, filters=filters, x=x, old=old, pairs=pairs, new=new)
    return _NEW[(kind, size, s)]


@pytest.mark.parametrize("kind,size,s", NEW_CASES, ids=["%s-%s-f%d" % (k, z, 8 * s) for k, z, s in NEW_CASES])
def test_rows_around_the_span(orc, bfir, kind, size, s):
    """Entries, set_bank, set_pairs_bank, fade_to_pairs_bank and fade_to_rows_bank at the shapes whose rows end inside a
    span, below one, or on a workgroup's end."""
    N = _new_setup(orc, kind, size, s)
    shape, x, fl = N["shape"], N["x"], N["filters"]
    L, blocks = shape[1], shape[2]
    taps = lambda ents: [[None if en is None else fl[en] for en in r] for r in ents]
    e, twin = (_engine(bfir, None, None, cls=N["cls"], shape=shape) for _ in range(2))
    assert e.lbank_create(len(fl) + 1) == 0 and e.lbank_load(0, fl) == 0
    assert twin.set_coeff(taps(N["old"])) == 0 and e.set_bank(N["old"]) == 0
    every = [(o, i) for o in range(shape[5]) for i in range(shape[4])]
    for o, i in every[:len(fl) + 1]:                                      # the entries of the first pairs, one without a path
        en = N["old"][o][i]
        cnt = counts(shape, None if en is None else fl[en].size)
        for k in range(len(blocks)):
            for b in range(blocks[k] if en is not None else 0):
                got = e.lbank_read(en, k, b)
                assert got.tobytes() == twin.coeff_block(k, o, i, b).tobytes() if b < cnt[k] else not got.any(), (en, k, b)
    _same_store(e, twin, shape, taps(N["old"]), every[:len(fl) + 1])
    _both(e, twin, x[:A_F * L], L, (A_F,))
    new_taps = [None if en is None else fl[en] for en in N["new"]]
    assert e.set_pairs_bank(N["pairs"], N["new"]) == 0 and twin.set_pairs(N["pairs"], new_taps) == 0
    merged = merge(taps(N["old"]), N["pairs"], new_taps)
    _same_store(e, twin, shape, merged, N["pairs"])
    n1 = A_F + sum(CUTS)
    _both(e, twin, x[A_F * L:n1 * L], L, CUTS)
    back = [N["old"][o][i] for o, i in N["pairs"]]
    back_taps = [None if en is None else fl[en] for en in back]
    assert e.fade_to_pairs_bank(N["pairs"], back, NEW_K) == 0 and twin.fade_to_pairs(N["pairs"], back_taps, NEW_K) == 0
    _both(e, twin, x[n1 * L:(n1 + 1) * L], L, (1,))
    n2 = x.shape[0] // L - 4
    _both(e, twin, x[(n1 + 1) * L:n2 * L], L, (n2 - n1 - 1,))
    assert e.fade_remaining() == 0
    _same_store(e, twin, shape, taps(N["old"]), N["pairs"])
    rot = [[None if en is None else (en + 1) % len(fl) for en in r] for r in N["old"]]
    rot[0][0] = 0                                                        # the tail level stays reached
    assert e.fade_to_rows_bank(rot, 2) == 0 and twin.fade_to_rows(taps(rot), 2) == 0
    _both(e, twin, x[n2 * L:], L, (1, 3))
    _same_store(e, twin, shape, taps(rot), every[:len(fl) + 1])
    e.close(); twin.close()


# ---- 9. offsets past 2^32 -----------------------------------------------------------------------------------------------------------
def test_a_level_store_beyond_4_gib(orc, bfir):
    """16385 entries at L = 1024, blocks (4, 8), ratios (1, 4) in fp32: the tail level's rows are 256 KiB, its last entry starts
    at byte 2^32.  Only entries 0 and 16384 are loaded; the last is gathered into a 2 -> 2 engine.  (Four head blocks are
    the fewest the engine admits at this ratio; see tests/test_lbank.py.)"""
    import torch
    L, blocks, ratios, s, n = BIG
    if torch.cuda.mem_get_info()[0] < 12 << 30:
        pytest.skip("less than 12 GiB of device memory free")
    shape = (s, L, blocks, ratios, 2, 2)
    _, D, _ = geo(shape)
    rng = np.random.default_rng(1024)
    hs = _synth(orc, rng, [D[-1] - 5, D[-1] - 4096 - 6], s)
    e, twin = (bfir.BrutefirMatrixLevels(L, blocks, ratios, s, 2, 2) for _ in range(2))
    assert e.lbank_create(n) == 0
    assert e.lbank_load(0, [hs[0]]) == 0 and e.lbank_load(n - 1, [hs[1]]) == 0
    assert e.lbank_blocks(0, 1) == 8 and e.lbank_blocks(n - 1, 1) == 7 and e.lbank_length(n - 2) == 0
    assert e.set_bank([[n - 1, None], [None, n - 1]]) == 0
    assert twin.set_coeff([[hs[1], None], [None, hs[1]]]) == 0
    merged = [[hs[1], None], [None, hs[1]]]
    _same_store(e, twin, shape, merged, [(0, 0), (1, 1)])
    assert all(e.lbank_read(n - 1, 1, b).tobytes() == twin.coeff_block(1, 0, 0, b).tobytes() for b in range(7))
    x = orc.synth_audio(rng, 7 * L, 2, np.float32)
    _both(e, twin, x[:3 * L], L, (1, 2))
    assert e.set_pairs_bank([(0, 1), (1, 1)], [0, None]) == 0
    assert twin.set_pairs([(0, 1), (1, 1)], [hs[0], None]) == 0
    _same_store(e, twin, shape, merge(merged, [(0, 1), (1, 1)], [hs[0], None]), [(0, 1), (1, 1)])
    _both(e, twin, x[3 * L:5 * L], L, (2,))
    assert e.fade_to_pairs_bank([(1, 0)], [n - 1], 2) == 0 and twin.fade_to_pairs([(1, 0)], [hs[1]], 2) == 0
    _both(e, twin, x[5 * L:], L, (2,))
    e.close(); twin.close()
