"""Pair-list coefficient updates on multi-level matrix and mimo engines on the GPU (bfir_engine_set_coeff_matrix_levels_pairs,
_pairs_fade; BrutefirMatrixLevels.set_pairs / fade_to_pairs) and k_wpatch (csrc/wpatch.hip, BFIR_PATCH_FUSED).

Shapes, lists and the fade's geometry are those of tests/test_lpairs.py, which holds them to their conditions without a GPU.
References are test_mimo_levels.wide_reference of the old and the merged rows, blended with test_fade.fade_weights; errors
are taken per block and output (size_matrix.block_errors) against conftest.TOL.  Runs are at least test_levels_gpu._nb blocks
long, so every delay line and ring wraps, with set_chunk(3) among them.  Run as a program (python tests/test_lpairs_gpu.py
data.npz out.npz) this file is the child process of the BFIR_PATCH_FUSED / BFIR_MIMO_MAC comparison: both are read when an
engine is created.

Largest distance of a pairs fade from the whole-matrix fade to the same merged set, per block and output, as printed by
test_fade (one MI355X): see DESIGN.md, "Pair lists on multi-level engines"."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import TOL
from test_fade import fade_weights
from test_levels_gpu import _nb, _settle
from test_lpairs import A_F, LISTS, SHAPES, counts, geo, merge, old_lengths, pair_list, special
from test_mimo_gpu import _run_cut, _worst
from test_mimo_levels import wide_reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUTS = (1, 2, 9, 3)                                                      # blocks per call behind the fade call
MIMO = ("9x3", "9x10", "9x2-f64")                                        # the shapes whose MAC is k_mac_mimo on every level
WIDE = (4, 16, (2, 2), (1, 2), 64, 64)                                   # 64 -> 64, the listed pair in the last row
WIDE_K = 5


def _dt(s):
    return np.float64 if s == 8 else np.float32


def _lv(shape):
    return shape[:4] + (shape[4],)


def _nblocks(shape, K):
    r_max = geo(shape)[2][-1]
    return max(_nb(_lv(shape)), A_F + max(K + r_max + 3, sum(CUTS) + 1))


def _synth(orc, rng, lens, s):
    """One filter per tap count (None stays None)."""
    return [None if n is None else orc.synth_ir(rng, 1, n, _dt(s))[0].astype(_dt(s)) for n in lens]


_OLD, _SETUP = {}, {}


def _old(orc, name):
    """The first set of a shape, its frames and its reference: computed once, read-only."""
    if name not in _OLD:
        _, shape, K = SHAPES[name]
        s, L, blocks, ratios, n_in, n_out = shape
        rng = np.random.default_rng(sum(name.encode()))
        rows = [_synth(orc, rng, r, s) for r in old_lengths(shape)]
        x = orc.synth_audio(rng, _nblocks(shape, K) * L, n_in, _dt(s))
        ref = wide_reference(orc, L, s, rows, x)
        for a in (x, ref):
            a.setflags(write=False)
        _OLD[name] = (rows, x, ref)
    return _OLD[name]


def _setup(orc, name, kind):
    """Everything the tests of one (shape, list) share: the old rows, the list, the merged rows, the frames, both references."""
    if (name, kind) not in _SETUP:
        _, shape, K = SHAPES[name]
        s, L = shape[0], shape[1]
        rows, x, ref_old = _old(orc, name)
        pairs, lens = pair_list(shape, kind)
        rng = np.random.default_rng(sum((name + kind).encode()))
        filters = _synth(orc, rng, lens, s)
        merged = merge(rows, pairs, filters)
        ref_new = wide_reference(orc, L, s, merged, x)
        ref_new.setflags(write=False)
        _SETUP[(name, kind)] = dict(shape=shape, K=K, old=rows, pairs=pairs, filters=filters, merged=merged, x=x,
                                    refs=(ref_old, ref_new))
    return _SETUP[(name, kind)]


def _engine(bfir, name, rows, chunk=3, cls=None, shape=None):
    cls = cls or SHAPES[name][0]
    s, L, blocks, ratios, n_in, n_out = shape or SHAPES[name][1]
    eng = getattr(bfir, cls)(L, blocks, ratios, s, n_in, n_out)
    if chunk is not None:
        eng.set_chunk(chunk)
    if rows is not None:
        assert eng.set_coeff(rows) == 0 and eng.is_initialized()
    return eng


@pytest.fixture()
def log(bfir):
    from foo_dsp_bfir_amd import _lib
    lines = []
    cb = _lib.LOG_FN(lambda msg: lines.append(msg.decode(errors="replace")))
    lib = bfir.load()
    lib.bfir_set_log_callback(cb)
    yield lines
    lib.bfir_set_log_callback(_lib.LOG_FN())


def _same_store(e, twin, shape, merged, pairs):
    """The filter stores of a patched engine and of its whole-matrix twin, over the listed pairs and a few others: byte for
    byte over the partitions below each pair's count, zeros past it on the patched engine."""
    s, L, blocks, ratios, n_in, n_out = shape
    others = [(o, i) for o in (0, n_out - 1) for i in (2 % n_in, n_in - 2)]
    for o, i in list(pairs) + [p for p in others if p not in pairs]:
        h = merged[o][i]
        cnt = counts(shape, None if h is None else h.size)
        for k in range(len(blocks)):
            for b in range(blocks[k]):
                got = e.coeff_block(k, o, i, b)
                if b < cnt[k]:
                    assert got.tobytes() == twin.coeff_block(k, o, i, b).tobytes(), (o, i, k, b)
                else:
                    assert not got.any(), (o, i, k, b)


# ---- 1. the plain call equals the whole call mid-stream --------------------------------------------------------------------------
@pytest.mark.parametrize("kind", LISTS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_plain_call_equals_the_whole_call_mid_stream(orc, bfir, name, kind):
    S = _setup(orc, name, kind)
    shape, x = S["shape"], S["x"]
    L = shape[1]
    e, twin = _engine(bfir, name, S["old"]), _engine(bfir, name, S["old"])
    rc0, y0 = e.run(x[:A_F * L])
    rct, yt = twin.run(x[:A_F * L])
    assert rc0 == rct == 0 and y0.tobytes() == yt.tobytes()
    assert e.set_pairs(S["pairs"], S["filters"]) == 0
    assert twin.set_coeff(S["merged"]) == 0
    assert e.is_initialized() and e.fade_remaining() == 0
    _same_store(e, twin, shape, S["merged"], S["pairs"])
    rc1, y1 = e.run(x[A_F * L:])
    rct, yt = twin.run(x[A_F * L:])
    assert rc1 == rct == 0 and y1.tobytes() == yt.tobytes()
    e.close(); twin.close()


def test_a_list_that_leaves_an_input_unread_goes_direct(orc, bfir, log):
    """4 -> 4 at L = 512: the engine pairs channels until the list removes every filter of input 2."""
    shape = (4, 512, (4, 2, 2), (1, 4, 2), 4, 4)
    s, L, blocks, ratios, n_in, n_out = shape
    _, D, _ = geo(shape)
    rng = np.random.default_rng(44)
    rows = [_synth(orc, rng, [D[-1] - 3 - (o + i) % 4 for i in range(n_in)], s) for o in range(n_out)]
    pairs = [(o, 2) for o in range(n_out)][::-1]
    merged = merge(rows, pairs, [None] * n_out)
    nb = _nb(_lv(shape))
    x = orc.synth_audio(rng, nb * L, n_in, np.float32)
    e, twin = (_engine(bfir, None, rows, cls="BrutefirMimoLevels", shape=shape) for _ in range(2))
    assert any("path=pair" in ln for ln in log), log
    rc0, y0 = e.run(x[:A_F * L])
    rct, yt = twin.run(x[:A_F * L])
    assert rc0 == rct == 0 and y0.tobytes() == yt.tobytes()
    del log[:]
    assert e.set_pairs(pairs, [None] * n_out) == 0
    assert any("an input feeds no output" in ln and "path=direct" in ln for ln in log), log
    assert twin.set_coeff(merged) == 0
    bad = x[A_F * L:].copy()
    bad[5, 2] = np.nan                                                   # the unread input keeps its NaN to itself
    rc1, y1 = e.run(bad)
    rct, yt = twin.run(bad)
    assert rc1 == rct == 0 and np.all(np.isfinite(y1)) and y1.tobytes() == yt.tobytes()
    e.close(); twin.close()


# ---- 2. the fade -----------------------------------------------------------------------------------------------------------------
def _pairs_fade(e, x, L, pairs, filters, K, a_f=A_F):
    """Blocks [0, a_f) in one call, fade_to_pairs, one block, the rest in one call."""
    rc, a = e.run(x[:a_f * L]); assert rc == 0
    assert e.fade_to_pairs(pairs, filters, K) == 0 and e.fade_remaining() == K
    rc, b = e.run(x[a_f * L:(a_f + 1) * L]); assert rc == 0
    assert e.fade_remaining() == K - 1
    rc, c = e.run(x[(a_f + 1) * L:]); assert rc == 0
    assert e.fade_remaining() == 0
    return np.concatenate([a, b, c])


def _check_fade(y, twin_old, twin_whole, x, shape, K, merged, refs, label, a_f=A_F):
    """The ranges of a pairs fade of K blocks made at block a_f in the whole stream y.  twin_old: an engine on the old set
    that is never patched.  twin_whole: one on the old set that fades to `merged` with the whole-matrix call at a_f."""
    s, L = shape[0], shape[1]
    r_max = geo(shape)[2][-1]
    nb = x.shape[0] // L
    rc, ya = twin_old.run(x[:a_f * L])
    assert rc == 0 and y[:a_f * L].tobytes() == ya.tobytes()             # before a_f: never patched
    rc, _ya = twin_whole.run(x[:a_f * L]); assert rc == 0
    assert twin_whole.fade_to_rows(merged, K) == 0
    rc, yb = twin_whole.run(x[a_f * L:]); assert rc == 0
    yb = np.concatenate([_ya, yb])
    tail = (a_f + K + r_max) * L
    assert tail < nb * L and y[tail:].tobytes() == yb[tail:].tobytes()   # from a_f + K + r_max on: the whole-matrix fade's bytes
    w = fade_weights(L, nb, a_f, K)[:, None]
    want = refs[0] * (1.0 - w) + refs[1] * w
    err = _worst(y, want, L)
    far = _worst(y[a_f * L:tail], yb[a_f * L:tail].astype(np.float64), L)
    print("%s: worst block %.3g against the float64 blend (tol %g); %.3g from the whole-matrix fade's" % (label, err, TOL[s], far))
    assert err <= TOL[s]


@pytest.mark.parametrize("kind", LISTS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_fade(orc, bfir, name, kind):
    S = _setup(orc, name, kind)
    shape, x, K = S["shape"], S["x"], S["K"]
    e = _engine(bfir, name, S["old"])
    y = _pairs_fade(e, x, shape[1], S["pairs"], S["filters"], K)
    twin_old, twin_whole = _engine(bfir, name, S["old"]), _engine(bfir, name, S["old"])
    _check_fade(y, twin_old, twin_whole, x, shape, K, S["merged"], S["refs"], "%s %s K=%d" % (name, kind, K))
    _same_store(e, twin_whole, shape, S["merged"], S["pairs"])           # the merged set is active on every level
    for eng in (e, twin_old, twin_whole):
        eng.close()


def _banded(o, i, n):
    return o != 5 and (i - o) % n < 3


def test_64_to_64_with_the_listed_pair_in_the_last_row(orc, bfir):
    """The last row of a 64 x 64 store: the offsets of the copy, the row load and the patch are 64-bit.  Plain and faded."""
    shape = WIDE
    s, L, blocks, ratios, n, _ = shape
    _, D, r = geo(shape)
    rng = np.random.default_rng(6464)
    lens = [[(D[1] - 3 if (o + i) % 4 == 0 else D[-1] - 1 - (o + i) % 5) if _banded(o, i, n) else None for i in range(n)]
            for o in range(n)]
    assert lens[n - 1][n - 1] > D[1]
    rows = [_synth(orc, rng, r_, s) for r_ in lens]
    pairs, filters = [(n - 1, n - 1)], _synth(orc, rng, [D[-1] - 2], s)
    merged = merge(rows, pairs, filters)
    nb = _nblocks(shape, WIDE_K)
    x = orc.synth_audio(rng, nb * L, n, np.float32)
    refs = tuple(wide_reference(orc, L, s, rr, x) for rr in (rows, merged))
    mk = lambda: _engine(bfir, None, rows, cls="BrutefirMimoLevels", shape=shape)
    e, twin = mk(), mk()
    assert e.run(x[:A_F * L])[0] == 0 and twin.run(x[:A_F * L])[0] == 0
    assert e.set_pairs(pairs, filters) == 0 and twin.set_coeff(merged) == 0
    _same_store(e, twin, shape, merged, pairs)
    rc, y1 = e.run(x[A_F * L:])
    rct, yt = twin.run(x[A_F * L:])
    assert rc == rct == 0 and y1.tobytes() == yt.tobytes()
    e.close(); twin.close()
    e, twin_old, twin_whole = mk(), mk(), mk()
    y = _pairs_fade(e, x, L, pairs, filters, WIDE_K)
    assert not y[:, 5].any()                                             # the output without any filter: zeros
    _check_fade(y, twin_old, twin_whole, x, shape, WIDE_K, merged, refs, "64x64 single K=%d" % WIDE_K)
    for eng in (e, twin_old, twin_whole):
        eng.close()


# ---- 3. how the blocks arrive ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_the_fade_does_not_depend_on_how_the_blocks_arrive(orc, bfir, name):
    """The mixed list's fade with the blocks behind the call in cuts of (1, 2, 9, 3) and the rest, in one call at the default
    chunk, in one call at set_chunk(3), and one block per call (the latency path): launches of one to four blocks take the
    one-block-per-lane form of every MAC and patch kernel, longer ones the tiled form."""
    S = _setup(orc, name, "mixed")
    shape, x, K = S["shape"], S["x"], S["K"]
    L = shape[1]
    nb = x.shape[0] // L
    rest = nb - A_F - sum(CUTS)
    assert rest >= 1 and K > 4
    out = {}
    for how, chunk, cuts in (("cuts", None, CUTS + (rest,)), ("one", None, (nb - A_F,)), ("chunk3", 3, (nb - A_F,)),
                             ("blocks", None, (1,) * (nb - A_F))):
        e = _engine(bfir, name, S["old"], chunk=chunk)
        rc, a = e.run(x[:A_F * L]); assert rc == 0
        assert e.fade_to_pairs(S["pairs"], S["filters"], K) == 0
        rcs, b = _run_cut(e, x[A_F * L:], L, cuts)
        assert rcs == [0] * len(cuts) and e.fade_remaining() == 0
        out[how] = np.concatenate([a, b]).tobytes()
        e.close()
    assert out["cuts"] == out["one"] == out["chunk3"] == out["blocks"]


# ---- 4. BFIR_PATCH_FUSED and BFIR_MIMO_MAC, each in a process of its own ---------------------------------------------------------
SMALL_MIMO = "m3x2"                                                      # 3 -> 2 as a mimo engine: k_mac_matrix, or k_mac_mimo on BFIR_MIMO_MAC=1


def _child_cases():
    return [(name, SHAPES[name][0]) for name in MIMO] + [(SMALL_MIMO, "BrutefirMimoLevels")]


def _child_main(data, out):
    """The mixed list's fade of every child case on engines created in THIS process (the switches as the parent set them):
    the output frames, the BFIR_K_MAC launch count of the blocks from the fade call on, and what the library said."""
    import foo_dsp_bfir_amd as bfir
    from foo_dsp_bfir_amd import _lib
    said = []
    cb = _lib.LOG_FN(lambda msg: said.append(msg.decode(errors="replace")))
    bfir.load().bfir_set_log_callback(cb)
    z = np.load(data, allow_pickle=True)
    res = {}
    for name, cls in _child_cases():
        shape, K = SHAPES[name][1], SHAPES[name][2]
        L = shape[1]
        old, pairs, filters, x = z[name + ":old"].tolist(), z[name + ":pairs"].tolist(), z[name + ":filters"].tolist(), z[name + ":x"]
        for chunk in (None, 3):
            e = _engine(bfir, name, old, chunk=chunk, cls=cls)
            rc, a = e.run(x[:A_F * L]); assert rc == 0
            e.set_profiling(True)
            assert e.fade_to_pairs([tuple(p) for p in pairs], filters, K) == 0
            rc, b = e.run(x[A_F * L:]); assert rc == 0
            res["%s:%s" % (name, chunk)] = np.concatenate([a, b])
            res["%s:%s:mac" % (name, chunk)] = np.array(e.profile()["k_mac"][1])
            e.close()
    res["said"] = np.array([ln for ln in said if ln.startswith("bfir matrix engine: crossfade of")])
    np.savez(out, **res)


def _obj(items):
    a = np.empty(len(items), dtype=object)
    for k, v in enumerate(items):
        a[k] = list(v) if isinstance(v, (list, tuple)) else v
    return a


@pytest.fixture(scope="module")
def children(orc, tmp_path_factory):
    """{label: results} of the child processes: BFIR_PATCH_FUSED=0, =1, and =1 with BFIR_MIMO_MAC=1."""
    tmp = tmp_path_factory.mktemp("lpairs")
    data = {}
    for name, _ in _child_cases():
        S = _setup(orc, name, "mixed")
        data[name + ":old"], data[name + ":pairs"] = _obj(S["old"]), np.array(S["pairs"])
        data[name + ":filters"], data[name + ":x"] = _obj(S["filters"]), S["x"]
    np.savez(str(tmp / "data.npz"), **data)
    out = {}
    for label, env in (("two", {"BFIR_PATCH_FUSED": "0"}), ("fused", {"BFIR_PATCH_FUSED": "1"}),
                       ("fused-mimo", {"BFIR_PATCH_FUSED": "1", "BFIR_MIMO_MAC": "1"})):
        dst = str(tmp / ("out-%s.npz" % label))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), str(tmp / "data.npz"), dst], env=dict(os.environ, **env),
                           cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
        out[label] = dict(np.load(dst, allow_pickle=True))
    return out


@pytest.mark.parametrize("name", MIMO + (SMALL_MIMO,))
def test_the_switches_change_no_byte(orc, bfir, children, name):
    S = _setup(orc, name, "mixed")
    shape, x, K = S["shape"], S["x"], S["K"]
    L = shape[1]
    e = _engine(bfir, name, S["old"], cls="BrutefirMimoLevels")          # this process: the defaults
    rc, a = e.run(x[:A_F * L]); assert rc == 0
    assert e.fade_to_pairs(S["pairs"], S["filters"], K) == 0
    rc, b = e.run(x[A_F * L:]); assert rc == 0
    e.close()
    want = np.concatenate([a, b]).tobytes()
    for label in ("two", "fused", "fused-mimo"):
        for chunk in (None, 3):
            assert children[label]["%s:%s" % (name, chunk)].tobytes() == want, (label, chunk)


def test_the_switches_chose_the_kernels_in_the_children(children):
    """What the library said at every fade call, and the BFIR_K_MAC launch counts: a launch that takes both sets is two spans
    with two launches and one with k_wpatch, every other launch is one either way."""
    cases = _child_cases()
    for label in ("two", "fused", "fused-mimo"):
        said = list(children[label]["said"])
        assert len(said) == 2 * len(cases), said
        for k, (name, _) in enumerate(cases):
            small = name == SMALL_MIMO
            if label == "two":
                kernel = "k_mac_matrix and k_patch_pairs" if small else "k_mac_mimo and k_patch_pairs"
            elif label == "fused":
                kernel = "k_mac_matrix and k_patch_pairs" if small else "k_wpatch"      # k_mac_matrix levels take two launches
            else:
                kernel = "k_wpatch"
            assert all(ln.endswith("runs %s." % kernel) for ln in said[2 * k:2 * k + 2]), (label, name, said)
    for name, _ in cases:
        for chunk in (None, 3):
            key = "%s:%s:mac" % (name, chunk)
            two, fused, fm = (int(children[label][key]) for label in ("two", "fused", "fused-mimo"))
            print(key, "launches: two", two, "fused", fused, "fused with k_mac_mimo", fm)
            assert fm < two and fm > 0
            assert fused == (two if name == SMALL_MIMO else fm)


# ---- 5. two pairs fades back to back ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["9x3", "9x2-f64"])
def test_two_pairs_fades_back_to_back(orc, bfir, name):
    """column, then mixed with the first merged set as the old one: the second fade's H2 is the buffer that held the set
    before the first fade, and must be copied afresh."""
    _, shape, K = SHAPES[name]
    s, L = shape[0], shape[1]
    r_max = geo(shape)[2][-1]
    S1, S2 = _setup(orc, name, "column"), _setup(orc, name, "mixed")
    a2 = A_F + K + r_max + 2
    a2 += 1 if a2 % r_max == 0 else 0
    nb = a2 + K + r_max + 3
    rng = np.random.default_rng(55)
    x = orc.synth_audio(rng, nb * L, shape[4], _dt(s))
    merged1 = S1["merged"]
    merged2 = merge(merged1, S2["pairs"], S2["filters"])
    refs = [wide_reference(orc, L, s, rows, x) for rows in (S1["old"], merged1, merged2)]

    def first(e):
        rc, a = e.run(x[:A_F * L]); assert rc == 0
        assert e.fade_to_pairs(S1["pairs"], S1["filters"], K) == 0
        rc, b = e.run(x[A_F * L:a2 * L]); assert rc == 0 and e.fade_remaining() == 0
        return np.concatenate([a, b])
    e = _engine(bfir, name, S1["old"])
    y1 = first(e)
    assert e.fade_to_pairs(S2["pairs"], S2["filters"], K) == 0 and e.fade_remaining() == K
    rc, y2 = e.run(x[a2 * L:]); assert rc == 0 and e.fade_remaining() == 0
    y = np.concatenate([y1, y2])
    once = _engine(bfir, name, S1["old"])                                # the first fade alone
    ya = first(once)
    assert y1.tobytes() == ya.tobytes()
    whole = _engine(bfir, name, S1["old"])                               # the second fade as a whole-matrix fade
    yw = first(whole)
    assert whole.fade_to_rows(merged2, K) == 0
    rc, yb = whole.run(x[a2 * L:]); assert rc == 0
    tail = (a2 + K + r_max) * L
    assert y[tail:].tobytes() == np.concatenate([yw, yb])[tail:].tobytes()
    w1, w2 = fade_weights(L, nb, A_F, K)[:, None], fade_weights(L, nb, a2, K)[:, None]
    want = refs[0] * (1.0 - w1) + refs[1] * (w1 - w2) + refs[2] * w2
    err = _worst(y, want, L)
    print("%s: two fades, worst block %.3g against the float64 blend" % (name, err))
    assert err <= TOL[s]
    _same_store(e, whole, shape, merged2, S1["pairs"] + S2["pairs"])
    for eng in (e, once, whole):
        eng.close()


# ---- 6. an input no filter reads ---------------------------------------------------------------------------------------------------
def test_nan_on_an_input_no_filter_reads_in_either_set(orc, bfir):
    name = "9x3"
    S = _setup(orc, name, "mixed")
    shape, K = S["shape"], S["K"]
    L = shape[1]
    dead = 3
    assert all(p[1] != dead for p in S["pairs"])
    sparse = [[None if i == dead else h for i, h in enumerate(r)] for r in S["old"]]
    pairs, filters = S["pairs"] + [(1, dead)], S["filters"] + [None]     # listed, without a filter in either set
    clean = S["x"].copy(); clean[:, dead] = 0
    bad = S["x"].copy()
    bad[:, dead] = 0
    for blk in (2, A_F - 1, A_F, A_F + 2, A_F + K + 1):
        bad[blk * L + 5, dead] = np.nan
    bad[(A_F + 1) * L, dead] = np.inf
    e = _engine(bfir, name, sparse)
    y = _pairs_fade(e, bad, L, pairs, filters, K)
    e.close()
    e = _engine(bfir, name, sparse)
    want = _pairs_fade(e, clean, L, pairs, filters, K)
    e.close()
    assert np.all(np.isfinite(y)) and y.tobytes() == want.tobytes()


# ---- 7. state ----------------------------------------------------------------------------------------------------------------------
def test_reset_during_the_fade_leaves_the_merged_set_active(orc, bfir):
    name = "9x3"
    S = _setup(orc, name, "mixed")
    shape, x, K = S["shape"], S["x"], S["K"]
    L = shape[1]
    e = _engine(bfir, name, S["old"])
    assert e.run(x[:A_F * L])[0] == 0
    assert e.fade_to_pairs(S["pairs"], S["filters"], K) == 0
    assert e.run(x[A_F * L:(A_F + 2) * L])[0] == 0 and e.fade_remaining() == K - 2
    e.reset()
    assert e.fade_remaining() == 0 and e.is_initialized()
    fresh = _engine(bfir, name, S["merged"])
    _same_store(e, fresh, shape, S["merged"], S["pairs"])
    rc, y = e.run(x)
    rcf, yf = fresh.run(x)
    assert rc == rcf == 0 and y.tobytes() == yf.tobytes()
    assert e.set_pairs(S["pairs"][:1], S["filters"][:1]) == 0            # and no fade is left on any level
    e.close(); fresh.close()


def test_a_whole_matrix_set_call_ends_the_fade_and_the_plain_list_waits(orc, bfir):
    name = "9x3"
    S = _setup(orc, name, "mixed")
    shape, K = S["shape"], S["K"]
    L = shape[1]
    settle = A_F + 2 + _settle(_lv(shape))
    nb = settle + 3
    x = orc.synth_audio(np.random.default_rng(77), nb * L, shape[4], _dt(shape[0]))
    e = _engine(bfir, name, S["old"])
    assert e.run(x[:A_F * L])[0] == 0
    assert e.fade_to_pairs(S["pairs"], S["filters"], K) == 0
    assert e.set_pairs(S["pairs"], S["filters"]) == bfir.ERR_STATE       # pending
    assert e.run(x[A_F * L:(A_F + 2) * L])[0] == 0
    assert e.set_pairs(S["pairs"], S["filters"]) == bfir.ERR_STATE and e.fade_remaining() == K - 2      # running
    assert e.fade_to_pairs(S["pairs"], S["filters"], K) == bfir.ERR_STATE
    assert e.set_coeff(S["merged"]) == 0 and e.fade_remaining() == 0     # a hard cut
    rc, y = e.run(x[(A_F + 2) * L:])
    assert rc == 0 and np.all(np.isfinite(y))
    # once everything computed before the cut has played out: the merged set's own bytes
    fresh = _engine(bfir, name, S["merged"])
    rcf, yf = fresh.run(x)
    assert rcf == 0 and settle < nb and y[(settle - A_F - 2) * L:].tobytes() == yf[settle * L:].tobytes()
    assert e.set_pairs(S["pairs"][:1], S["filters"][:1]) == 0            # no fade is left: the plain list is taken
    e.close(); fresh.close()


def test_refusals_change_nothing(orc, bfir):
    name = "9x3"
    S = _setup(orc, name, "mixed")
    shape, x, K = S["shape"], S["x"], S["K"]
    s, L, blocks, ratios, n_in, n_out = shape
    _, D, _ = geo(shape)
    lib = bfir.load()
    plain, fade = lib.bfir_engine_set_coeff_matrix_levels_pairs, lib.bfir_engine_set_coeff_matrix_levels_pairs_fade
    A, U, ST, CO = bfir.ERR_ARG, bfir.ERR_UNSUPPORTED, bfir.ERR_STATE, bfir.ERR_COEFF
    twin = _engine(bfir, name, S["old"])
    rc, want = twin.run(x); assert rc == 0
    twin.close()
    h = np.ascontiguousarray(S["filters"][1])

    def both(eng, n, outs, ins, ptrs, lens, code, K_=2):
        ia = lambda v: None if v is None else (C.c_int * len(v))(*v)
        pa = None if ptrs is None else (C.c_void_p * len(ptrs))(*ptrs)
        assert plain(eng.handle, n, ia(outs), ia(ins), pa, ia(lens), 1.0) == code
        assert fade(eng.handle, n, ia(outs), ia(ins), pa, ia(lens), 1.0, K_) == code

    new = _engine(bfir, name, None)                                      # no coefficients yet
    both(new, 1, [0], [0], [h.ctypes.data], [h.size], ST)
    new.close()
    e = _engine(bfir, name, S["old"])
    rc, a = e.run(x[:A_F * L]); assert rc == 0
    p = h.ctypes.data
    both(e, 1, None, [0], [p], [h.size], A)
    both(e, 1, [0], None, [p], [h.size], A)
    both(e, 1, [0], [0], None, [h.size], A)
    both(e, 1, [0], [0], [p], None, A)
    both(e, 0, [0], [0], [p], [h.size], A)
    both(e, 1, [n_out], [0], [p], [h.size], A)
    both(e, 1, [0], [n_in], [p], [h.size], A)
    both(e, 1, [-1], [0], [p], [h.size], A)
    both(e, 2, [1, 1], [2, 2], [p, p], [h.size, h.size], A)              # the same pair twice
    both(e, 1, [0], [0], [p], [-1], A)
    both(e, 1, [0], [0], [p], [D[-1] + 1], A)                            # past the taps the levels hold
    ia = lambda v: (C.c_int * len(v))(*v)
    one = (C.c_void_p * 1)(p)
    assert fade(e.handle, 1, ia([0]), ia([0]), one, ia([h.size]), 1.0, 0) == A
    assert fade(e.handle, 1, ia([0]), ia([0]), one, ia([h.size]), 1.0, (1 << 24) // L + 1) == A
    nan = h.copy(); nan[-1] = np.nan                                     # a NaN tap: the engine keeps its filters and stays initialised
    assert e.set_pairs([(0, 0)], [nan]) == CO and e.fade_to_pairs([(0, 0)], [nan], 2) == CO
    assert e.is_initialized() and e.fade_remaining() == 0
    # the uniform kinds' calls keep refusing this kind, and these calls every other kind
    assert e.set_coeff_pairs([(0, 0)], [h]) == U and e.set_coeff_pairs_fade([(0, 0)], [h], 2) == U
    other = bfir.BrutefirMimo(L, blocks[0], s, n_in, n_out)
    both(other, 1, [0], [0], [p], [4], U)
    other.close()
    lev = bfir.BrutefirLevels(L, blocks, ratios, s, 2)
    both(lev, 1, [0], [0], [p], [4], U)
    lev.close()
    rc, b = e.run(x[A_F * L:])
    assert rc == 0 and np.concatenate([a, b]).tobytes() == want.tobytes()
    e.close()
    # a merged set with taps on a level no filter of the old set reaches: the fade is refused, the plain call starts the level
    short = [[None if r is None else r[:min(r.size, D[2] - 3)] for r in row] for row in S["old"]]
    twin = _engine(bfir, name, short)
    rc, want = twin.run(x); assert rc == 0
    twin.close()
    e = _engine(bfir, name, short)
    rc, a = e.run(x[:A_F * L]); assert rc == 0
    long_one = np.ascontiguousarray(S["filters"][1])
    assert long_one.size > D[2]
    assert e.fade_to_pairs([(0, 0)], [long_one], K) == U and e.fade_remaining() == 0 and e.is_initialized()
    rc, b = e.run(x[A_F * L:])
    assert rc == 0 and np.concatenate([a, b]).tobytes() == want.tobytes()
    twin = _engine(bfir, name, short)
    assert twin.run(x)[0] == 0                                           # both at the same block
    assert e.set_pairs([(0, 0)], [long_one]) == 0 and twin.set_coeff(merge(short, [(0, 0)], [long_one])) == 0
    rc, y = e.run(x[:8 * L])
    rct, yt = twin.run(x[:8 * L])
    assert rc == rct == 0 and y.tobytes() == yt.tobytes()
    e.close(); twin.close()


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    _child_main(sys.argv[1], sys.argv[2])
