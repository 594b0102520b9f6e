"""The size matrix of tests/test_size_matrix_gpu.py against the sources, on the CPU: adding a transform size to the
kernels or moving a size limit fails here until the matrix follows."""
import collections

import numpy as np
import pytest

import size_matrix as SM
from conftest import TOL, rel_err
from test_fade import fade_expected, fade_weights
from test_matrix import matrix_reference
from test_mlevels import uniform_reference

ALL_CELLS = SM.CELLS + SM.KIND_CELLS


def test_matrix_covers_exactly_what_the_sources_support():
    lim = SM.source_limits()
    want = SM.supported_set(lim)
    have = {(c["family"], c["s"], c["L"]) for c in ALL_CELLS}
    assert sorted(want - have) == [], "sizes the build supports that no cell runs"
    assert sorted(have - want) == [], "cells at sizes the build does not support"
    # ... list by list: a family's cells are in the list of its kind and nowhere else
    for prefix, cells in (("nup_", SM.NUP_CELLS), ("fade_", SM.FADE_CELLS), ("matrix", SM.MATRIX_CELLS),
                          ("levels_", SM.LEVELS_CELLS), ("lfade_", SM.LFADE_CELLS), ("mlevels_", SM.MLEVELS_CELLS),
                          ("mfade_", SM.MFADE_CELLS)):
        assert {k for k in want if k[0].startswith(prefix)} == {(c["family"], c["s"], c["L"]) for c in cells}
    assert not [c["id"] for c in SM.CELLS if c["family"].startswith(("nup_", "fade_", "matrix", "levels_", "lfade_", "mlevels_",
                                                                     "mfade_"))]


def test_matrix_refusals_are_the_unsupported_neighbours():
    lim = SM.source_limits()
    want = {(s, L) for s in (4, 8) for L in SM.refused_lengths(lim, s)}
    assert {(s, L) for s, L, _ in SM.REFUSALS} == want


def test_source_limits_parse():
    """The parser reads the values the kernels are built with (a silent regex miss would empty the matrix)."""
    lim = SM.source_limits()
    assert lim["log2m"] == list(range(min(lim["log2m"]), max(lim["log2m"]) + 1)) and len(lim["log2m"]) >= 2
    assert lim["pair_log2n"] and set(lim["pair_log2n"]) <= {lg + 1 for lg in lim["log2m"]}
    assert lim["run64_min_log2m"] <= lim["pairs64_max_log2m"] and (1 << lim["pairs64_max_log2m"]) <= lim["run64_max_len"]
    assert lim["lds_bytes"] > 0
    # the fused back ends of the two-level engines and of the fade run where the pair plans do (engine.hip asks
    # pair_supported for both), one instance per plan
    assert lim["nup_log2n"] == lim["pair_log2n"] and lim["fade_log2n"] == lim["pair_log2n"]
    assert max(SM.MATRIX_CALLS[0], 1) <= lim["mat_small_max"] < SM.MATRIX_CALLS[1]
    # ... and so do the fused back ends of the multi-level engines and of the fades on split engines; one ring per tail
    assert lim["levels_log2n"] == lim["lfade_log2n"] == lim["pair_log2n"]
    assert lim["level_rings"] == lim["max_levels"] - 1 and max(SM.LEVEL_BLOCKS) == lim["max_levels"]
    # ... and the lone kernel of a matrix head with an odd output count; the wide fade is one time-tiled launch of either precision
    assert lim["lone_log2n"] == lim["pair_log2n"]
    assert SM.MFADE_WIDE_K == SM.MATRIX_CALLS[1] > 2 * 4 and SM.MFADE_WIDE_K > 8 > lim["mat_small_max"]


def test_cells_set_every_path_switch_and_are_unique():
    ids = [c["id"] for c in ALL_CELLS]
    assert len(ids) == len(set(ids))
    for c in SM.KIND_CELLS:
        assert set(c["env"]) == set(SM.PATH_SWITCHES), c["id"]
    for c in SM.CELLS:
        assert set(c["env"]) == set(SM.PATH_SWITCHES), c["id"]
        assert c["path"] in ("pair", "time-pair", "direct", "staging") and c["layout"] in ("pairs", "grouped")
        assert c["run"] in ("on", "off")


@pytest.mark.parametrize("nx,nh", [(1, 1), (17, 5), (1000, 999), (4096, 3065), (20000, 1500)])
def test_fft_reference_matches_direct_form(orc, nx, nh):
    rng = np.random.default_rng(nx + nh)
    x, h = rng.uniform(-1, 1, nx), rng.uniform(-1, 1, nh)
    want = orc.direct_conv(x, h)
    got = SM.fft_conv(x, h)
    assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max()


def test_reference_helpers_match_the_oracle(orc):
    """grouped_spectrum / halfcomplex / hc2r, the float64 forms the GPU tests compare with, against the oracle's own
    restatement of the reference (float64)."""
    rng = np.random.default_rng(7)
    L = 64
    taps = rng.standard_normal(L - 5)
    assert np.allclose(SM.grouped_spectrum(taps, L, 0.5), orc.coeffs2cbuf(taps, L, 0.5), rtol=0, atol=1e-15)
    x = rng.standard_normal(2 * L)
    hc = orc.r2hc(x)
    assert np.allclose(SM.halfcomplex(np.fft.rfft(x), 2 * L), hc, rtol=0, atol=1e-12)
    assert np.allclose(SM.hc2r(hc), orc.hc2r(hc), rtol=0, atol=1e-12)


def test_flat_ir_keeps_the_tail_loud():
    rng = np.random.default_rng(0)
    L, taps = 256, SM.B * 256 - SM.RAGGED
    for h in SM.flat_ir(rng, 3, taps):
        assert abs(np.abs(h).sum() - 1.0) < 1e-12
        first, tail = np.abs(h[:L]).mean(), np.abs(h[(SM.B - 1) * L:]).mean()
        assert 0.5 < tail / first < 2.0


# ---- the engine kinds: two-level engines, fades, matrix engines ------------------------------------------------------
def test_kind_cells_are_the_ones_the_sweep_is_made_of():
    """Per family, the number of cells the sizes in the sources ask for: taking an entry out of a list fails here (or in
    the coverage test above, where it was the only one of its size)."""
    lim = SM.source_limits()
    f32, f64 = SM.supported_lengths(lim, 4), SM.supported_lengths(lim, 8)
    fused = [1 << (n - 1) for n in lim["pair_log2n"]]
    t32, t64 = [L for L in f32 if 2 * L in f32], [L for L in f64 if 2 * L in f64]
    want = {
        "nup_fused": 2 * len(fused) + 1,                                    # C = 2, 8; the large ratio
        "nup_general32": len(t32) + len([L for L in t32 if L < min(fused)]),       # C = 3; C = 2 below the pair plans
        "nup_general64": 2 * len(t64) + 3,                                  # C = 2, 3; the plug-in's frames at three sizes
        "fade_fused": 2 * len(fused),                                       # channel pairs, pairs in time
        "fade_general32": 2 * (len(f32) - len(fused)) + len(fused),         # C = 2, 3 outside the plans; double frames inside
        "fade_general64": len(f64) + 3,
        "matrix32": len(f32) + 3,
        "matrix64": len(f64) + 1,
    }
    # multi-level engines and fades on split engines: heads that take n levels of ratio 2
    fit = lambda Ls, full, n: [L for L in Ls if (L << (n - 1)) in full]
    want.update({
        "levels_fused": len(fit(fused, f32, 3)) + len(fit(fused, f32, 4)) + 2,     # C = 2 per depth and size; C = 8 once per depth
        # C = 3; C = 2 below the pair plans; four levels at three sizes
        "levels_general32": len(fit(f32, f32, 3)) + len([L for L in fit(f32, f32, 3) if L < min(fused)]) + 3,
        "levels_general64": 2 * len(fit(f64, f64, 3)) + 2 + 2,             # C = 2, 3; four levels twice; the plug-in's frames twice
        "lfade_fused": sum(len(fit(fused, f32, n)) for n in (2, 3, 4)),    # one per reachable (LOG2N, NR)
        "lfade_general32": 2 * len([L for L in fit(f32, f32, 2) if L < min(fused)]) + len(fit(fused, f32, 2)),
        "lfade_general64": len(fit(f64, f64, 3)) + 2 + 1 + 1,               # the plug-in's frames twice; the 8192 tail; four levels
    })
    # multi-level matrix engines and their fades
    lo32 = [L for L in f32 if L < min(fused)]
    want.update({
        # 2 -> 3 per depth and size; 2 -> 2, 1 -> 2, 2 -> 1 once per depth; one 3 -> 5
        "mlevels_fused": sum(len(fit(fused, f32, n)) for n in (2, 3, 4)) + 3 * 3 + 1,
        # 2 -> 3 and 3 -> 2 below the pair plans, four levels twice; double output frames at every pair plan
        "mlevels_general32": 2 * len(lo32) + 2 + len(fit(fused, f32, 2)),
        "mlevels_general64": len(fit(f64, f64, 3)) + 1 + 2 + 2,            # the 8192 tail; four levels twice; the plug-in's frames twice
        "mfade_fused": sum(len(fit(fused, f32, n)) for n in (2, 3, 4)),    # one per reachable (LOG2N, NR)
        "mfade_general32": 2 * len(lo32) + len(fit(fused, f32, 2)) + 4,    # as lfade_general32; four wide cells
        "mfade_general64": len(fit(f64, f64, 3)) + 2 + 1 + 1 + 2,          # as lfade_general64; two wide cells
    })
    assert dict(collections.Counter(c["family"] for c in SM.KIND_CELLS)) == want


def test_two_level_cells_reach_every_tail_length():
    lim = SM.source_limits()
    for s in (4, 8):
        tails = {c["r"] * c["L"] for c in SM.NUP_CELLS if c["s"] == s}
        assert tails == {Lt for Lt in SM.supported_lengths(lim, s) if Lt >= 32}, s
    for c in SM.NUP_CELLS:
        assert c["Bh"] == c["r"] and c["back"] == ("fused" if c["family"] == "nup_fused" else "general"), c["id"]
        # ends inside the last tail partition; both the tail's delay line and its time ring wrap
        assert 0 < c["Bh"] * c["L"] + c["Bt"] * c["r"] * c["L"] - c["taps"] < c["r"] * c["L"]
        assert c["nb"] >= c["Bh"] + c["r"] * (c["Bt"] + 2) + 3
        # what engine.hip's choose_path gives the head: channel pairs (no pairs in time on a two-level engine)
        pair = c["s"] == 4 and c["in_fmt"] == c["out_fmt"] == SM.FLOAT_LE and c["C"] % 2 == 0 and \
            c["L"] in [1 << (n - 1) for n in lim["nup_log2n"]]
        assert pair == (c["back"] == "fused"), c["id"]
    # the refusals: one step past the largest tail of each precision
    assert {(s, L) for s, L, r, _ in SM.NUP_REFUSALS if r == 2} == {(s, max(SM.supported_lengths(lim, s))) for s in (4, 8)}


def test_fade_cells_follow_the_engines_rule():
    """engine.hip `e->fade_fused = ...`: the rule as SM.fade_is_fused restates it, and every cell on its side of it."""
    lim = SM.source_limits()
    rule = SM.fade_fused_rule()
    assert rule == "e->s == 4 && e->ilv && e->out_fmt == BFIR_SAMPLE_FORMAT_FLOAT_LE && pair_supported(e->L)", rule
    for c in SM.FADE_CELLS:
        assert SM.fade_is_fused(lim, c["s"], c["L"], c["out_fmt"]) == (c["family"] == "fade_fused"), c["id"]
    # both gain directions in every family, and on both fused paths (channel pairs: C = 2, pairs in time: C = 3)
    for fam in ("fade_fused", "fade_general32", "fade_general64"):
        assert {c["new_gain"] for c in SM.FADE_CELLS if c["family"] == fam} == {0.125, 8.0}
    for Cn in (2, 3):
        assert {c["new_gain"] for c in SM.FADE_CELLS if c["family"] == "fade_fused" and c["C"] == Cn} == {0.125, 8.0}


def _cell_instances(cell):
    """(LOG2N, NR) of the fused inverse kernels a cell runs: a non-fading run of n levels passes through 0 .. n - 1 contributing
    rings, of which k_inv_levels takes 2 and up; a fade cell starts its fade with all n - 1 contributing."""
    lg, tails = cell["L"].bit_length(), len(cell["blocks"]) - 1             # the transform has 2 L points
    if cell["family"] == "mlevels_fused":
        # k_inv_lone: the last output of an odd count.  Behind the pair front end (an even input count) from no ring on; a
        # direct front end inverts the chunks before any level contributes with k_inv (engine.hip, queue_inv)
        return {(lg, nr) for nr in range(cell["n_in"] % 2, tails + 1)} if cell["n_out"] % 2 else set()
    return {(lg, nr) for nr in range(2, tails + 1)} if cell["family"] == "levels_fused" else {(lg, tails)}


def test_fused_level_cells_run_exactly_the_reachable_instances():
    """k_inv_levels<LOG2N, NR>, k_inv_lfade<LOG2N, NR> and k_inv_lone<LOG2N, NR>: every instance an engine can launch is run
    by a cell, and the ones no engine can launch are the three largest of each kernel.  Relaxing bfir_engine_create_levels (or
    adding a size to one of the macros) fails here until cells follow.  The matrix fades run the k_inv_lfade set a second
    time, with odd and with even output counts in every row."""
    lim = SM.source_limits()
    for fam, cells, log2n, nr_min in (("levels_fused", SM.LEVELS_CELLS, lim["levels_log2n"], 2),
                                      ("lfade_fused", SM.LFADE_CELLS, lim["lfade_log2n"], 1),
                                      ("mlevels_fused", SM.MLEVELS_CELLS, lim["lone_log2n"], 0),
                                      ("mfade_fused", SM.MFADE_CELLS, lim["lfade_log2n"], 1)):
        reach, built = SM.reachable_instances(lim, log2n, nr_min)
        run = set().union(*[_cell_instances(c) for c in cells if c["family"] == fam])
        assert run == reach, (fam, sorted(reach - run), sorted(run - reach))
        assert built - reach == {(14, 2), (14, 3), (13, 3)}, fam
        assert len(built) == len(log2n) * (lim["level_rings"] + 1 - nr_min)
    # every reachable k_inv_lone instance by a 2 -> 3 cell of its own depth (the strided pair kernels beside it), and every
    # k_inv_lfade instance once by the matrix fades
    two_three = [c for c in SM.MLEVELS_CELLS if c["family"] == "mlevels_fused" and (c["n_in"], c["n_out"]) == (2, 3)]
    reach, _ = SM.reachable_instances(lim, lim["lone_log2n"], 0)
    assert collections.Counter((c["L"].bit_length(), len(c["blocks"]) - 1) for c in two_three) == \
        collections.Counter({k: 1 for k in reach if k[1] >= 1})
    mf = [c for c in SM.MFADE_CELLS if c["family"] == "mfade_fused"]
    reach, _ = SM.reachable_instances(lim, lim["lfade_log2n"], 1)
    assert collections.Counter((c["L"].bit_length(), len(c["blocks"]) - 1) for c in mf) == collections.Counter({k: 1 for k in reach})


def test_level_cells_follow_the_rules_of_create_levels():
    """bfir_engine_create_levels: ratios[0] = 1, the others powers of two >= 2, D_k >= L_k, every L_k supported and at most
    16384; the geometry and run lengths the cells are made with; the back end each family name stands for."""
    lim = SM.source_limits()
    pair_plans = [1 << (n - 1) for n in lim["pair_log2n"]]
    for c in SM.LEVELS_CELLS + SM.LFADE_CELLS:
        n, L, blocks, ratios = len(c["blocks"]), c["L"], c["blocks"], c["ratios"]
        assert 2 <= n <= lim["max_levels"] and (n >= 3 or c in SM.LFADE_CELLS), c["id"]
        assert blocks == SM.LEVEL_BLOCKS[n] and ratios == (1,) + (2,) * (n - 1), c["id"]
        Ls, D = SM.level_geometry(L, blocks, ratios)
        ok = SM.supported_lengths(lim, c["s"])
        assert all(Lk in ok and Lk <= 16384 for Lk in Ls), c["id"]
        assert all(D[k] >= Ls[k] for k in range(1, n)), c["id"]
        assert c["in_fmt"] in (SM.FLOAT_LE, SM.FLOAT64_LE) and c["out_fmt"] in (SM.FLOAT_LE, SM.FLOAT64_LE)
        assert 0 < D[-1] - c["taps"] < Ls[-1], c["id"]                   # ends inside the last partition of the last level
        r_last = Ls[-1] // L
        if c in SM.LEVELS_CELLS:
            assert c["nb"] == D[-2] // L + r_last * (blocks[-1] + 2) + 3
            # engine.hip, choose_path: e->pair of the head (channel pairs; a split engine has no pairs in time)
            pair = c["s"] == 4 and c["in_fmt"] == c["out_fmt"] == SM.FLOAT_LE and c["C"] % 2 == 0 and L in pair_plans
            assert pair == (c["back"] == "fused") == (c["family"] == "levels_fused"), c["id"]
        else:
            assert c["t0"] == D[-2] // L + r_last + 1 and all(c["t0"] % (Lk // L) for Lk in Ls[1:]), c["id"]
            assert c["nb"] == c["t0"] + SM.FADE_K + 2 * r_last + 1
            assert SM.fade_is_fused(lim, c["s"], L, c["out_fmt"]) == (c["family"] == "lfade_fused"), c["id"]
    # the coverage the families are there for
    def have(cells, fam, **kv):
        return {c["L"] for c in cells if c["family"] == fam and all(
            (len(c["blocks"]) if k == "n" else c[k]) == v for k, v in kv.items())}
    f32, f64 = SM.supported_lengths(lim, 4), SM.supported_lengths(lim, 8)
    fit = lambda Ls, full, n: {L for L in Ls if (L << (n - 1)) in full}
    lo32 = {L for L in f32 if L < min(pair_plans)}
    LV, LF = SM.LEVELS_CELLS, SM.LFADE_CELLS
    assert all(c["C"] % 2 == 0 for c in LV if c["family"] == "levels_fused")
    for n in (3, 4):
        assert have(LV, "levels_fused", n=n, C=2) == fit(pair_plans, f32, n)
        assert len(have(LV, "levels_fused", n=n, C=8)) == 1
    assert have(LV, "levels_general32", n=3, C=3) == fit(f32, f32, 3) and have(LV, "levels_general32", n=3, C=2) == lo32
    four = have(LV, "levels_general32", n=4)
    assert len(four) == 3 and {min(f32), max(fit(f32, f32, 4))} <= four
    for Cn in (2, 3):
        assert have(LV, "levels_general64", n=3, C=Cn, out_fmt=SM.FLOAT64_LE) == fit(f64, f64, 3)
    assert have(LV, "levels_general64", n=4) == {min(f64), max(fit(f64, f64, 4))}
    assert len(have(LV, "levels_general64", out_fmt=SM.FLOAT_LE, in_fmt=SM.FLOAT_LE)) == 2
    for n in (2, 3, 4):
        assert have(LF, "lfade_fused", n=n) == fit(pair_plans, f32, n)
        assert {c["new_gain"] for c in LF if c["family"] == "lfade_fused" and len(c["blocks"]) == n} == {0.125, 8.0}
        row = [c["C"] for c in LF if c["family"] == "lfade_fused" and len(c["blocks"]) == n]
        assert set(row) == {2, 3} and all(a != b for a, b in zip(row, row[1:]))
        both = {(c["C"], c["new_gain"]) for c in LF if c["family"] == "lfade_fused" and len(c["blocks"]) == n}
        assert len(both) == min(4, len(row)), (n, both)                  # each channel count fades both ways where the row has four sizes
        for fam in ("lfade_general32", "lfade_general64"):
            assert have(LF, fam, n=n), (fam, n)
    for fam in ("lfade_fused", "lfade_general32", "lfade_general64"):
        assert {c["new_gain"] for c in LF if c["family"] == fam} == {0.125, 8.0}
    for Cn in (2, 3):
        assert have(LF, "lfade_general32", C=Cn, out_fmt=SM.FLOAT_LE) == lo32
    assert have(LF, "lfade_general32", out_fmt=SM.FLOAT64_LE) == fit(pair_plans, f32, 2)
    assert have(LF, "lfade_general64", n=3, out_fmt=SM.FLOAT64_LE) == fit(f64, f64, 3)
    assert max(f64) // 2 in have(LF, "lfade_general64", n=2)
    assert len(have(LF, "lfade_general64", out_fmt=SM.FLOAT_LE, in_fmt=SM.FLOAT_LE)) == 2
    # the refusals: the first shape past each limit
    assert SM.LEVELS_REFUSALS == [(4, 2 * max(fit(f32, f32, 3)), 3, "ERR_UNSUPPORTED"),
                                  (4, 2 * max(fit(f32, f32, 4)), 4, "ERR_UNSUPPORTED"),
                                  (8, 2 * max(fit(f64, f64, 3)), 3, "ERR_UNSUPPORTED")]


def _duo_launches(lim, cell):
    """{(T, ILV, NO, TT)} of the k_mac_duo launches of a fade cell, restated from mfade.hip and engine.hip.  duo_no: two
    outputs per tile where fp32 has two; duo_tt: one block per lane up to BFIR_MAT_SMALL_MAX blocks in the launch, else tiles
    of 8 (fp32) or 4 (fp64).  The layout is each level's own (choose_path: fp32 pairs from 2 L_k = 512, fp64 pairs where the run
    kernels keep them).  Blocks per launch: the head's fade in launches of cell["chunk"]; level k up to its last old block
    lf_j1 = (t0 + K - 1 - D_k / L) // r_k from the t0 // r_k it has run -- that one, which began before the fading call (t0 is
    inside a block of every level), alone from the kept frames, the others in launches of ceil(chunk / r_k) (nup_tail_ahead,
    ensure_chunk)."""
    s, L, t0, K, chunk = cell["s"], cell["L"], cell["t0"], cell["K"], cell["chunk"]
    Ls, D = SM.level_geometry(L, cell["blocks"], cell["ratios"])
    pairs64 = [1 << lg for lg in range(lim["run64_min_log2m"], lim["pairs64_max_log2m"] + 1)]
    no = 2 if s == 4 and cell["n_out"] >= 2 else 1
    out = set()
    for k, Lk in enumerate(Ls):
        r = Lk // L
        both = K if k == 0 else (t0 + K - 1 - D[k] // L) // r - t0 // r + 1     # blocks that need both sets
        if both <= 0:                # every old block the fade reads has run: the level is on the new set from the start
            continue
        per = -(-chunk // r)
        sizes = {min(per, both)} | ({both % per} if both % per and both > per else set())
        if k > 0:
            assert t0 % r, cell["id"]
            rest = both - 1
            sizes = {1} | ({min(per, rest)} if rest else set()) | ({rest % per} if rest % per and rest > per else set())
        ilv = (2 * Lk >= 512) if s == 4 else (Lk in pairs64)
        for n_t in sizes:
            out.add(("f" if s == 4 else "d", int(ilv), no, 1 if n_t <= lim["mat_small_max"] else (8 if s == 4 else 4)))
    return out


def test_mfade_cells_run_every_duo_instance():
    """k_mac_duo<T, ILV, NO, TT>: the twelve instances launch_mac_duo can pick (tests/test_mlevels_fade.py holds the build to
    them) are all launched by the cells, the time-tiled ones by the wide cells alone, whose head fades in ONE launch of
    MFADE_WIDE_K blocks: time tiles 8 + 3 (fp32) or 4 + 4 + 3 (fp64), the last one ragged, as MATRIX_CALLS has them for
    k_mac_matrix."""
    from test_mlevels_fade import DUO_INSTANCES
    lim = SM.source_limits()
    run = collections.defaultdict(list)
    for c in SM.MFADE_CELLS:
        for inst in _duo_launches(lim, c):
            run[inst].append(c["id"])
            assert (inst[3] > 1) <= c["wide"], (c["id"], inst)
    assert set(run) == DUO_INSTANCES and len(DUO_INSTANCES) == 12, sorted(DUO_INSTANCES - set(run))
    wide = [c for c in SM.MFADE_CELLS if c["wide"]]
    assert len(wide) == 6 and len(SM.MFADE_CELLS) == len(SM.LFADE_CELLS) + 6     # the diagonal fades mirrored, and the wide cells
    # every cell launches the latency form on some level, with its own precision and outputs per tile
    for c in SM.MFADE_CELLS:
        assert {i[3] for i in _duo_launches(lim, c)} >= {1}, c["id"]
    # one wide cell per (T, ILV, NO), at the smallest head whose levels all have that layout
    f32, f64 = SM.supported_lengths(lim, 4), SM.supported_lengths(lim, 8)
    pairs64 = [1 << lg for lg in range(lim["run64_min_log2m"], lim["pairs64_max_log2m"] + 1)]
    smallest = {("f", 0): min(f32), ("f", 1): min(L for L in f32 if 2 * L >= 512), ("d", 0): min(f64), ("d", 1): min(pairs64)}
    seen = set()
    for c in wide:
        tiled = {i for i in _duo_launches(lim, c) if i[3] > 1}
        assert len(tiled) == 1 and len({i[:3] for i in _duo_launches(lim, c)}) == 1, c["id"]
        (t, ilv, no, tt), = tiled
        seen.add((t, ilv, no))
        assert c["L"] == smallest[(t, ilv)] and c["K"] == c["chunk"] == SM.MFADE_WIDE_K > tt and SM.MFADE_WIDE_K % tt, c["id"]
        # the fade's blocks all have every level's contribution (t0 past every D_k, as the rule test has it): one nup_mask, one chunk
        assert c["nb"] - c["t0"] >= c["K"]
    assert seen == {k[:3] for k in DUO_INSTANCES}


def test_mlevels_cells_follow_the_rules_of_create_matrix_levels():
    """bfir_engine_create_matrix_levels: check_levels_args as test_level_cells_follow_the_rules_of_create_levels states it,
    the geometry and run lengths of _levels_cell, the back end each family name stands for (engine.hip, `e->back_fused = ...`),
    the filter lengths of matrix_level_lengths and what the families are there for."""
    lim = SM.source_limits()
    rule = SM.back_fused_rule()
    assert rule == ("e->nup && (e->matrix ? e->s == 4 && e->ilv && e->out_fmt == BFIR_SAMPLE_FORMAT_FLOAT_LE && pair_supported(e->L) "
                    ": e->pair)"), rule
    assert rule.split("?")[1].split(":")[0].strip() == SM.fade_fused_rule()    # the conditions of the fused fade
    pair_plans = [1 << (n - 1) for n in lim["pair_log2n"]]
    assert list(SM.PAIR_PLANS) == pair_plans
    # pair_supported decides the fused back end, so the lone kernel has the pair plans' sizes: each one, and no other
    assert lim["lone_log2n"] == lim["pair_log2n"]
    assert len([c for c in SM.MFADE_CELLS if c["wide"]]) == 6 and len(SM.MFADE_CELLS) == len(SM.LFADE_CELLS) + 6
    for c in SM.MLEVELS_CELLS + SM.MFADE_CELLS:
        n, L, blocks, ratios, n_in, n_out = len(c["blocks"]), c["L"], c["blocks"], c["ratios"], c["n_in"], c["n_out"]
        fade = c in SM.MFADE_CELLS
        assert 2 <= n <= lim["max_levels"] and 1 <= n_in <= 8 and 1 <= n_out <= 8 and c["C"] == n_in, c["id"]
        assert blocks == SM.LEVEL_BLOCKS[n] and ratios == (1,) + (2,) * (n - 1), c["id"]
        Ls, D = SM.level_geometry(L, blocks, ratios)
        ok = SM.supported_lengths(lim, c["s"])
        assert all(Lk in ok and Lk <= 16384 for Lk in Ls), c["id"]
        assert all(D[k] >= Ls[k] for k in range(1, n)), c["id"]
        assert c["in_fmt"] in (SM.FLOAT_LE, SM.FLOAT64_LE) and c["out_fmt"] in (SM.FLOAT_LE, SM.FLOAT64_LE)
        r_last = Ls[-1] // L
        fused = SM.matrix_back_is_fused(lim, c["s"], L, c["out_fmt"])
        assert fused == c["family"].endswith("_fused"), c["id"]
        assert c["family"].endswith(("_fused", "_general32") if c["s"] == 4 else "_general64"), c["id"]
        if not fade:
            assert c["nb"] == D[-2] // L + r_last * (blocks[-1] + 2) + 3 and c["back"] == ("fused" if fused else "general")
        else:
            K = c["K"]
            assert K == (SM.MFADE_WIDE_K if c["wide"] else SM.FADE_K) and c["chunk"] == (K if c["wide"] else 2)
            assert c["t0"] == D[-2] // L + r_last + 1 and all(c["t0"] % (Lk // L) for Lk in Ls[1:]), c["id"]
            assert c["nb"] == c["t0"] + K + 2 * r_last + 1
            # the gain rule of the fade cells with both sides counted; along a row of mfade_fused half the index joins it
            step = pair_plans.index(L) // 2 if c["family"] == "mfade_fused" else 0
            assert c["new_gain"] == (0.125 if (L.bit_length() - 1 + n_in + n_out + step) % 2 == 0 else 8.0), c["id"]
        # the NULL pair: the rule of MATRIX_CELLS, one step on where that is filter 0
        lg = L.bit_length() - 1
        if n_in * n_out < 3:
            assert c["null"] is None
        else:
            at = (lg % n_out, lg % n_in)
            assert c["null"] == (at if at != (0, 0) else ((0, 1) if n_in > 1 else (1, 0))), c["id"]
        # the filters: filter j of the old set ends inside the last partition of level order[j % n], the first one in the last
        # level's with the taps of the diagonal cells; with n or more of them one ends in every level
        order = [n - 1] + list(range(n - 1))
        flat = [v for row in c["lens"] for v in row]
        assert [v is None for v in flat] == [(o, i) == c["null"] for o in range(n_out) for i in range(n_in)], c["id"]
        have = [v for v in flat if v is not None]
        assert have[0] == c["taps"] == D[-1] - SM.RAGGED == max(have), c["id"]
        for j, v in enumerate(have):
            k = order[j % n]
            assert v == D[k + 1] - SM.RAGGED - j // n and D[k + 1] - Ls[k] < v < D[k + 1], (c["id"], j)
        if len(have) >= n:
            assert all(any(D[k] < v <= D[k + 1] for v in have) for k in range(n)), c["id"]
        if fade:
            # the new set: the old table with its columns mirrored (its outputs too where the mirror changes too little), every
            # filter inside the FIRST partition of its level; the NULL pair moves and the counts differ at every level
            new = [v for row in c["lens_new"] for v in row if v is not None]
            assert len(new) == len(have) and len(c["lens_new"]) == n_out and all(len(r) == n_in for r in c["lens_new"])
            ends = lambda vs: sorted((k, D[k + 1] - v if last else D[k] + Ls[k] - v) for v, last in vs
                                     for k in range(n) if D[k] < v <= D[k + 1])
            assert ends((v, True) for v in have) == ends((v, False) for v in new), c["id"]
            assert all(D[k] < v < D[k] + Ls[k] for v in new for k in range(n) if D[k] < v <= D[k + 1]), c["id"]
            assert SM.sets_differ(L, blocks, ratios, c["lens"], c["lens_new"]), c["id"]
            co, cn = SM.partition_counts(c, c["lens"]), SM.partition_counts(c, c["lens_new"])
            assert all(co[k] != cn[k] for k in range(n)), c["id"]
            for lens, cnt in ((c["lens"], co), (c["lens_new"], cn)):     # both sets read every input and reach every level
                assert all(any(r[i] is not None for r in lens) for i in range(n_in)), c["id"]
                assert all(any(v for r in lvl for v in r) for lvl in cnt), c["id"]
            mirrored = [r[::-1] for r in c["lens"]] if n_in > 1 else c["lens"][::-1]
            shape = lambda lens: [[v is None for v in r] for r in lens]
            assert shape(c["lens_new"]) in (shape(mirrored), shape(mirrored[::-1])), c["id"]

    # the coverage the families are there for
    def have(cells, fam, **kv):
        return {c["L"] for c in cells if c["family"] == fam and all(
            (len(c["blocks"]) if k == "n" else (c["n_in"], c["n_out"]) if k == "io" else c.get(k)) == v for k, v in kv.items())}
    f32, f64 = SM.supported_lengths(lim, 4), SM.supported_lengths(lim, 8)
    fit = lambda Ls, full, n: {L for L in Ls if (L << (n - 1)) in full}
    lo32 = {L for L in f32 if L < min(pair_plans)}
    ML, MF = SM.MLEVELS_CELLS, SM.MFADE_CELLS
    for n in (2, 3, 4):
        row = sorted(fit(pair_plans, f32, n))
        assert have(ML, "mlevels_fused", n=n, io=(2, 3)) == set(row)
        for io in ((2, 2), (1, 2), (2, 1)):
            assert have(ML, "mlevels_fused", n=n, io=io) == {row[1]}, (n, io)
        assert have(MF, "mfade_fused", n=n) == set(row)
        cells = [c for c in MF if c["family"] == "mfade_fused" and len(c["blocks"]) == n]
        assert {c["new_gain"] for c in cells} == {0.125, 8.0}
        ios = [(c["n_in"], c["n_out"]) for c in cells]
        assert set(ios) == {(2, 3), (3, 2)} and all(a != b for a, b in zip(ios, ios[1:]))
        for fam in ("mfade_general32", "mfade_general64"):
            assert have(MF, fam, n=n), (fam, n)
    assert [(len(c["blocks"]), c["L"]) for c in ML if (c["n_in"], c["n_out"]) == (3, 5)] == [(3, min(pair_plans))]
    assert all(c["in_fmt"] == c["out_fmt"] == SM.FLOAT_LE for c in ML + MF if c["family"].endswith("_fused"))
    for io in ((2, 3), (3, 2)):
        assert have(ML, "mlevels_general32", n=3, io=io, out_fmt=SM.FLOAT_LE) == lo32
    assert have(ML, "mlevels_general32", n=4) == {min(lo32), max(lo32)}
    assert have(ML, "mlevels_general32", n=2, io=(2, 3), out_fmt=SM.FLOAT64_LE) == set(pair_plans)      # 8192 x 16384 among them
    assert have(ML, "mlevels_general64", n=3, io=(2, 3), out_fmt=SM.FLOAT64_LE) == fit(f64, f64, 3)
    assert have(ML, "mlevels_general64", n=2) == {max(fit(f64, f64, 2))} and 2 * max(fit(f64, f64, 2)) == max(f64)
    assert have(ML, "mlevels_general64", n=4) == {min(f64), max(fit(f64, f64, 4))}
    assert have(ML, "mlevels_general64", io=(2, 2), in_fmt=SM.FLOAT_LE, out_fmt=SM.FLOAT_LE) == {64, 1024}
    plain = [c for c in MF if not c["wide"]]
    for io in ((2, 3), (3, 2)):
        assert have(plain, "mfade_general32", io=io, out_fmt=SM.FLOAT_LE) == lo32
    assert have(plain, "mfade_general32", out_fmt=SM.FLOAT64_LE) == fit(pair_plans, f32, 2)
    assert have(plain, "mfade_general64", n=3, io=(2, 3), out_fmt=SM.FLOAT64_LE) == fit(f64, f64, 3)
    assert max(f64) // 2 in have(plain, "mfade_general64", n=2)
    assert len(have(plain, "mfade_general64", out_fmt=SM.FLOAT_LE, in_fmt=SM.FLOAT_LE)) == 2
    for fam in ("mfade_fused", "mfade_general32", "mfade_general64"):
        assert {c["new_gain"] for c in plain if c["family"] == fam} == {0.125, 8.0}
    # the cells mirror the diagonal ones: the same (realsize, L, depth, formats) in the same order, a channel count of 2 as
    # 2 -> 3 and of 3 as 3 -> 2
    key = lambda c: (c["s"], c["L"], len(c["blocks"]), c["in_fmt"], c["out_fmt"])
    assert [key(c) + ((2, 3) if c["C"] == 2 else (3, 2),) for c in SM.LFADE_CELLS] == [key(c) + ((c["n_in"], c["n_out"]),) for c in plain]
    # the refusals: the first shape past each limit, those of the diagonal kind
    assert SM.MLEVELS_REFUSALS == SM.LEVELS_REFUSALS == [(4, 2 * max(fit(f32, f32, 3)), 3, "ERR_UNSUPPORTED"),
                                                         (4, 2 * max(fit(f32, f32, 4)), 4, "ERR_UNSUPPORTED"),
                                                         (8, 2 * max(fit(f64, f64, 3)), 3, "ERR_UNSUPPORTED")]


def _oracle_uniform(orc, cell, h, x):
    L = cell["L"]
    o = orc.Engine(L, -(-cell["taps"] // L), cell["s"], cell["C"], cell["in_fmt"], cell["out_fmt"])
    assert o.set_coeff(h) == 0
    rc, y = o.run(x)
    assert rc == 0
    o.close()
    return y


@pytest.mark.parametrize("cell", SM.KIND_CELLS, ids=[c["id"] for c in SM.KIND_CELLS])
def test_kind_cell_leaves_a_margin(orc, cell):
    """No cell sits at the edge of its tolerance because of its own data: the oracle's uniform engine on the cell's data
    is within half the tolerance of the float64 reference, in the norm the GPU test uses."""
    L, s = cell["L"], cell["s"]
    if cell in SM.NUP_CELLS or cell in SM.LEVELS_CELLS:
        h, x = SM.nup_data(orc, cell)
        y, ref = _oracle_uniform(orc, cell, h, x), SM.reference(orc, x, h)
    elif cell in SM.FADE_CELLS or cell in SM.LFADE_CELLS:
        h_old, h_new, x = SM.fade_data(orc, cell)
        y, _, _ = fade_expected(orc, L, -(-cell["taps"] // L), s, cell["C"], h_old, h_new, x, cell["t0"], SM.FADE_K,
                                cell["in_fmt"], cell["out_fmt"])
        ref = SM.fade_reference(orc, cell, h_old, h_new, x)
    elif cell in SM.MLEVELS_CELLS:
        rows, x = SM.mlevels_data(orc, cell)
        y, ref = uniform_reference(orc, L, s, rows, x), SM.matrix_reference_conv(orc, rows, x)
    elif cell in SM.MFADE_CELLS:
        # the blend tests/test_mlevels_fade.py defines: two uniform references under test_fade.fade_weights
        rows_old, rows_new, x = SM.mfade_data(orc, cell)
        w = fade_weights(L, cell["nb"], cell["t0"], cell["K"])[:, None]
        y = uniform_reference(orc, L, s, rows_old, x) * (1.0 - w) + uniform_reference(orc, L, s, rows_new, x) * w
        ref = SM.fade_reference(orc, cell, rows_old, rows_new, x)
    else:
        rows, x = SM.matrix_data(orc, cell)
        y, ref = matrix_reference(orc, L, SM.B, s, rows, x), SM.matrix_reference_conv(orc, rows, x)
    err = SM.block_errors(y, ref, L)
    assert err.max() <= 0.5 * SM.tolerance(cell, TOL), (err.max(), np.unravel_index(np.argmax(err), err.shape))


def test_a_quiet_tail_hides_what_the_per_block_norm_shows(orc):
    """Why the cells use flat_ir and block_errors: a last tail partition that is 0.1 % too loud moves the per-block,
    per-channel norm with flat filters by far more than the fp32 tolerance, and conftest.rel_err with oracle.synth_ir
    (e^-6 over the taps) on the same shape by less than it."""
    s, L, Bh, r, Bt, Cn = 8, 64, 4, 2, 5, 3
    taps, nb = Bh * L + Bt * r * L - SM.RAGGED, Bh + r * (Bt + 2) + 3
    last = Bh * L + (Bt - 1) * r * L
    rng = np.random.default_rng(11)

    def moved(h, x, norm):
        y = np.stack([SM.fft_conv(x[:, c], h[c]) for c in range(Cn)], axis=1)
        h2 = [v.copy() for v in h]
        for v in h2:
            v[last:] *= 1.0 + 1e-3
        return norm(np.stack([SM.fft_conv(x[:, c], h2[c]) for c in range(Cn)], axis=1), y)

    x_flat = rng.uniform(-1.0, 1.0, (nb * L, Cn)) * SM.amplitudes(nb, L, Cn, False)
    flat = moved(SM.flat_ir(rng, Cn, taps), x_flat, lambda y, ref: SM.block_errors(y, ref, L).max())
    quiet = moved(orc.synth_ir(rng, Cn, taps, np.float64), orc.synth_audio(rng, nb * L, Cn, np.float64), rel_err)
    print("last tail partition x (1 + 1e-3): flat_ir / block_errors %.3g, synth_ir / rel_err %.3g" % (flat, quiet))
    assert flat > 1e-5 and quiet < 1e-5
