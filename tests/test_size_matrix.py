"""The size matrix of tests/test_size_matrix_gpu.py against the sources, on the CPU: adding a transform size to the
kernels or moving a size limit fails here until the matrix follows."""
import collections

import numpy as np
import pytest

import size_matrix as SM
from conftest import TOL, rel_err
from test_fade import fade_expected
from test_matrix import matrix_reference

ALL_CELLS = SM.CELLS + SM.KIND_CELLS


def test_matrix_covers_exactly_what_the_sources_support():
    lim = SM.source_limits()
    want = SM.supported_set(lim)
    have = {(c["family"], c["s"], c["L"]) for c in ALL_CELLS}
    assert sorted(want - have) == [], "sizes the build supports that no cell runs"
    assert sorted(have - want) == [], "cells at sizes the build does not support"
    # ... list by list: a family's cells are in the list of its kind and nowhere else
    for prefix, cells in (("nup_", SM.NUP_CELLS), ("fade_", SM.FADE_CELLS), ("matrix", SM.MATRIX_CELLS),
                          ("levels_", SM.LEVELS_CELLS), ("lfade_", SM.LFADE_CELLS)):
        assert {k for k in want if k[0].startswith(prefix)} == {(c["family"], c["s"], c["L"]) for c in cells}
    assert not [c["id"] for c in SM.CELLS if c["family"].startswith(("nup_", "fade_", "matrix", "levels_", "lfade_"))]


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
    return {(lg, nr) for nr in range(2, tails + 1)} if cell["family"] == "levels_fused" else {(lg, tails)}


def test_fused_level_cells_run_exactly_the_reachable_instances():
    """k_inv_levels<LOG2N, NR> and k_inv_lfade<LOG2N, NR>: every instance an engine can launch is run by a cell, and the ones
    no engine can launch are the three largest of each kernel.  Relaxing bfir_engine_create_levels (or adding a size to either
    macro) fails here until cells follow."""
    lim = SM.source_limits()
    for fam, cells, log2n, nr_min in (("levels_fused", SM.LEVELS_CELLS, lim["levels_log2n"], 2),
                                      ("lfade_fused", SM.LFADE_CELLS, lim["lfade_log2n"], 1)):
        reach, built = SM.reachable_instances(lim, log2n, nr_min)
        run = set().union(*[_cell_instances(c) for c in cells if c["family"] == fam])
        assert run == reach, (fam, sorted(reach - run), sorted(run - reach))
        assert built - reach == {(14, 2), (14, 3), (13, 3)}, fam
        assert len(built) == len(log2n) * (lim["level_rings"] + 1 - nr_min)


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
