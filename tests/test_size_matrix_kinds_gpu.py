"""The size matrix for the engine kinds on top of the plain diagonal engine (tests/size_matrix.py: NUP_CELLS, FADE_CELLS,
MATRIX_CELLS, LEVELS_CELLS, LFADE_CELLS, MLEVELS_CELLS, MFADE_CELLS): two-level engines, crossfaded coefficient changes,
matrix engines, multi-level engines, crossfaded coefficient changes on split engines, multi-level matrix engines and their
crossfades at every transform size their kernels have, with flat-envelope filters, odd channels at 1/8 and the per-block,
per-channel norm, each against a float64 / long-double reference computed here from the frames and taps actually sent --
and against the oracle, as the plain sweep does (tests/test_size_matrix_gpu.py).  The wide cells of MFADE_CELLS run their
whole fade in one time-tiled k_mac_duo launch and a second time with BFIR_MFADE_DUO=0, byte for byte."""
import numpy as np
import pytest

import size_matrix as SM
from conftest import TOL, env_override
from test_fade import fade_expected, fade_weights
from test_matrix import matrix_reference
from test_mlevels import uniform_reference

pytestmark = pytest.mark.gpu

WORST = {}          # (family, realsize) -> worst per-block error seen against the float64 reference


@pytest.fixture(scope="module")
def creation_log(bfir):
    """Lines the library logs, captured through bfir_set_log_callback (the callback object is kept alive here)."""
    from foo_dsp_bfir_amd import _lib
    lines = []
    cb = _lib.LOG_FN(lambda msg: lines.append(msg.decode(errors="replace")))
    lib = bfir.load()
    lib.bfir_set_log_callback(cb)
    yield lines
    lib.bfir_set_log_callback(_lib.LOG_FN())
    for k in sorted(WORST):
        print("size matrix: worst per-block error %-16s realsize %d: %.3g" % (k[0], k[1], WORST[k]))


def _check(cell, y, ref, y_orc):
    """The per-block norm against the float64 reference (recorded in WORST), then against the oracle."""
    L, tol = cell["L"], SM.tolerance(cell, TOL)
    err = SM.block_errors(y, ref, L)
    key = (cell["family"], cell["s"])
    WORST[key] = max(WORST.get(key, 0.0), float(err.max()))
    print("%s: worst per-block error %.3g (tol %.3g)" % (cell["id"], err.max(), tol))
    assert err.max() <= tol, np.unravel_index(np.argmax(err), err.shape)         # (channel, block)
    err = SM.block_errors(y, y_orc, L)
    assert err.max() <= tol, np.unravel_index(np.argmax(err), err.shape)


def _run_calls(eng, x, L, cuts):
    """One run() per stretch of blocks [cuts[k], cuts[k + 1])."""
    ys = []
    for a, e in zip(cuts[:-1], cuts[1:]):
        rc, y = eng.run(x[a * L:e * L])
        assert rc == 0
        ys.append(y)
    return np.concatenate(ys)


def _engine_lines(creation_log):
    made = [ln for ln in creation_log if ln.startswith("bfir engine: ") and "two levels" not in ln and " levels, " not in ln]
    return [dict(kv.split("=") for kv in ln.split(". ")[-1].split()) for ln in made]


# ---- two-level engines -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", SM.NUP_CELLS, ids=[c["id"] for c in SM.NUP_CELLS])
def test_nup_size_matrix(orc, bfir, creation_log, cell):
    s, L, Cn, Bh, r, Bt = cell["s"], cell["L"], cell["C"], cell["Bh"], cell["r"], cell["Bt"]
    D, Lt, nb = Bh * L, r * L, cell["nb"]
    h, x = SM.nup_data(orc, cell)

    with env_override(**cell["env"]):
        del creation_log[:]
        eng = bfir.BrutefirNup(L, Bh, r, Bt, s, Cn, cell["in_fmt"], cell["out_fmt"])
        made = [ln for ln in creation_log if "two levels" in ln]
        assert made == ["bfir engine: two levels, head %d x %d, tail %d x %d; back end %s." % (L, Bh, Lt, Bt, cell["back"])], \
            creation_log
        eng.set_chunk(3)
        assert eng.set_coeff(h) == 0
        # partition spectra of both levels, the ragged last tail partition included, in the grouped layout
        for level, (Lp, Bp, lo) in enumerate(((L, Bh, 0), (Lt, Bt, D))):
            for c in range(Cn):
                for b in range(Bp):
                    want = SM.grouped_spectrum(h[c][lo + b * Lp:lo + (b + 1) * Lp], Lp, 1.0)
                    got = eng.coeff_block(level, c, b).astype(np.float64)
                    assert np.abs(got - want).max() <= TOL[s] * np.abs(want).max(), (level, c, b)
        # r + 1 blocks (the call ends inside a tail block), one block alone (the latency path), then the rest
        y = _run_calls(eng, x, L, (0, r + 1, r + 2, nb))
        eng.close()

    o = orc.Engine(L, -(-cell["taps"] // L), s, Cn, cell["in_fmt"], cell["out_fmt"])
    assert o.set_coeff(h) == 0
    rc, y_orc = o.run(x)
    assert rc == 0
    o.close()
    _check(cell, y, SM.reference(orc, x, h), y_orc)


@pytest.mark.parametrize("s,L,r,err", SM.NUP_REFUSALS)
def test_nup_refuses_size(bfir, s, L, r, err):
    with pytest.raises(bfir.BfirError) as ei:
        bfir.BrutefirNup(L, r, r, 2, s, 2)
    assert ei.value.code == getattr(bfir, err)
    # nothing left behind: the device still makes and runs a two-level engine of a supported size
    dt = np.float32 if s == 4 else np.float64
    eng = bfir.BrutefirNup(1024, 2, 2, 2, s, 2)
    assert eng.set_coeff([np.ones(2 * 1024 + 10, dt) / 4096] * 2) == 0
    rc, y = eng.run(np.ones((8 * 1024, 2), dt))
    assert rc == 0 and np.all(np.isfinite(y))
    assert abs(float(y[-1, 0]) - (2 * 1024 + 10) / 4096) <= 1e-5          # all taps under a constant input: their sum
    eng.close()


# ---- crossfaded coefficient changes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", SM.FADE_CELLS, ids=[c["id"] for c in SM.FADE_CELLS])
def test_fade_size_matrix(orc, bfir, creation_log, cell):
    s, L, Cn, t0, nb, K = cell["s"], cell["L"], cell["C"], cell["t0"], cell["nb"], SM.FADE_K
    fused = cell["family"] == "fade_fused"
    h_old, h_new, x = SM.fade_data(orc, cell)

    with env_override(**cell["env"]):
        del creation_log[:]
        eng = bfir.Brutefir(L, SM.B, s, Cn, cell["in_fmt"], cell["out_fmt"])
        made = _engine_lines(creation_log)
        assert len(made) == 1, creation_log
        path = made[0]["path"]
        assert not fused or path == ("pair" if Cn % 2 == 0 else "time-pair"), made
        eng.set_chunk(2)                     # the fade's K = 3 blocks are cut into 2 + 1: the second part starts at m0 = 2 L
        eng.set_profiling(True)
        assert eng.set_coeff(h_old) == 0
        rc, y0 = eng.run(x[:t0 * L])
        assert rc == 0
        assert eng.set_coeff_fade(h_new, K) == 0
        rc, y1 = eng.run(x[t0 * L:])
        assert rc == 0 and eng.fade_remaining() == 0
        # which back end ran: the plain chunks of these paths stage no output, the general fade does (queue_stage_out)
        if path != "staging":
            staged = eng.profile()["k_stage_out"][1]
            assert (staged == 0) if fused else (staged > 0), (path, staged)
        eng.close()
    y = np.concatenate([y0, y1])

    want, _, _ = fade_expected(orc, L, SM.B, s, Cn, h_old, h_new, x, t0, K, cell["in_fmt"], cell["out_fmt"])
    _check(cell, y, SM.fade_reference(orc, cell, h_old, h_new, x), want)


# ---- matrix engines --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", SM.MATRIX_CELLS, ids=[c["id"] for c in SM.MATRIX_CELLS])
def test_matrix_size_matrix(orc, bfir, creation_log, cell):
    s, L, n_in, n_out = cell["s"], cell["L"], cell["n_in"], cell["n_out"]
    rows, x = SM.matrix_data(orc, cell)
    first, second = SM.MATRIX_CALLS

    with env_override(**cell["env"]):
        del creation_log[:]
        eng = bfir.BrutefirMatrix(L, SM.B, s, n_in, n_out, cell["in_fmt"], cell["out_fmt"])
        made = _engine_lines(creation_log)
        assert len(made) == 1 and (made[0]["path"], made[0]["layout"]) == (cell["path"], cell["layout"]), creation_log
        eng.set_chunk(second)
        assert eng.set_coeff(rows) == 0
        # every present filter's partition spectra, the ragged one included; the NULL filter's stay out of the sums
        for o, row in enumerate(rows):
            for i, h in enumerate(row):
                for b in range(SM.B if h is not None else 0):
                    want = SM.grouped_spectrum(h[b * L:(b + 1) * L], L, 1.0)
                    got = eng.coeff_block(o, i, b).astype(np.float64)
                    assert np.abs(got - want).max() <= TOL[s] * np.abs(want).max(), (o, i, b)
        y = _run_calls(eng, x, L, (0, first, first + second))
        eng.close()
    assert y.shape == (cell["nb"] * L, n_out)

    _check(cell, y, SM.matrix_reference_conv(orc, rows, x), matrix_reference(orc, L, SM.B, s, rows, x))


# ---- multi-level engines ---------------------------------------------------------------------------------------------
def _oracle_uniform(orc, cell, h, x):
    L = cell["L"]
    o = orc.Engine(L, -(-cell["taps"] // L), cell["s"], cell["C"], cell["in_fmt"], cell["out_fmt"])
    assert o.set_coeff(h) == 0
    rc, y = o.run(x)
    assert rc == 0
    o.close()
    return y


@pytest.mark.parametrize("cell", SM.LEVELS_CELLS, ids=[c["id"] for c in SM.LEVELS_CELLS])
def test_levels_size_matrix(orc, bfir, creation_log, cell):
    s, L, Cn, blocks, ratios, nb = cell["s"], cell["L"], cell["C"], cell["blocks"], cell["ratios"], cell["nb"]
    Ls, D = SM.level_geometry(L, blocks, ratios)
    h, x = SM.nup_data(orc, cell)

    with env_override(**cell["env"]):
        del creation_log[:]
        eng = bfir.BrutefirLevels(L, blocks, ratios, s, Cn, cell["in_fmt"], cell["out_fmt"])
        made = [ln for ln in creation_log if " levels, " in ln]
        names = ", ".join("%d x %d" % (Lk, b) for Lk, b in zip(Ls, blocks))
        assert made == ["bfir engine: %d levels, %s; back end %s." % (len(blocks), names, cell["back"])], creation_log
        assert len(_engine_lines(creation_log)) == len(blocks), creation_log     # one diagonal engine per level, no more
        eng.set_chunk(3)
        assert eng.set_coeff(h) == 0
        # partition spectra of every level, the ragged last partition of the last level included, in the grouped layout
        for level, (Lp, Bp) in enumerate(zip(Ls, blocks)):
            for c in range(Cn):
                for b in range(Bp):
                    want = SM.grouped_spectrum(h[c][D[level] + b * Lp:D[level] + (b + 1) * Lp], Lp, 1.0)
                    got = eng.coeff_block(level, c, b).astype(np.float64)
                    assert np.abs(got - want).max() <= TOL[s] * np.abs(want).max(), (level, c, b)
        # a call that ends inside a block of the last level, one block alone (the latency path), then the rest
        r_last = Ls[-1] // L
        y = _run_calls(eng, x, L, (0, r_last + 1, r_last + 2, nb))
        eng.close()

    _check(cell, y, SM.reference(orc, x, h), _oracle_uniform(orc, cell, h, x))


@pytest.mark.parametrize("s,L,n,err", SM.LEVELS_REFUSALS)
def test_levels_refuses_size(bfir, s, L, n, err):
    with pytest.raises(bfir.BfirError) as ei:
        bfir.BrutefirLevels(L, SM.LEVEL_BLOCKS[n], (1,) + (2,) * (n - 1), s, 2)
    assert ei.value.code == getattr(bfir, err)
    # nothing left behind: the device still makes and runs a three-level engine of a supported size
    dt = np.float32 if s == 4 else np.float64
    eng = bfir.BrutefirLevels(1024, SM.LEVEL_BLOCKS[3], (1, 2, 2), s, 2)
    taps = 4 * 1024 + 10                                                    # ten taps into the last level
    assert eng.set_coeff([np.ones(taps, dt) / 8192] * 2) == 0
    rc, y = eng.run(np.ones((16 * 1024, 2), dt))
    assert rc == 0 and np.all(np.isfinite(y))
    assert abs(float(y[-1, 0]) - taps / 8192) <= 1e-5                       # all taps under a constant input: their sum
    eng.close()


# ---- crossfaded coefficient changes on two-level and multi-level engines --------------------------------------------------
@pytest.mark.parametrize("cell", SM.LFADE_CELLS, ids=[c["id"] for c in SM.LFADE_CELLS])
def test_lfade_size_matrix(orc, bfir, creation_log, cell):
    s, L, Cn, blocks, ratios = cell["s"], cell["L"], cell["C"], cell["blocks"], cell["ratios"]
    t0, nb, K = cell["t0"], cell["nb"], SM.FADE_K
    fused = cell["family"] == "lfade_fused"
    h_old, h_new, x = SM.fade_data(orc, cell)

    with env_override(**cell["env"]):
        if len(blocks) == 2:
            eng = bfir.BrutefirNup(L, blocks[0], ratios[1], blocks[1], s, Cn, cell["in_fmt"], cell["out_fmt"])
        else:
            eng = bfir.BrutefirLevels(L, blocks, ratios, s, Cn, cell["in_fmt"], cell["out_fmt"])
        eng.set_chunk(2)                     # the fade's K = 3 blocks are cut into 2 + 1: the second part starts at m0 = 2 L
        assert eng.set_coeff(h_old) == 0
        rc, y0 = eng.run(x[:t0 * L])
        assert rc == 0
        assert eng.fade_to(h_new, K) == 0 and eng.fade_remaining() == K
        # the first chunk of the fade on its own, profiled: the fused fade stores the frames itself, the general one ends in
        # k_stage_out (outside a fade the general back end of a split engine stages its output as well, so only the fade counts)
        eng.set_profiling(True)
        rc, y1 = eng.run(x[t0 * L:(t0 + 2) * L])
        assert rc == 0 and eng.fade_remaining() == K - 2
        staged = eng.profile()["k_stage_out"][1]
        assert (staged == 0) if fused else (staged > 0), staged
        eng.set_profiling(False)
        # the fade's last block (m0 = 2 L), the swap of the sets and the blocks after it in one call
        rc, y2 = eng.run(x[(t0 + 2) * L:])
        assert rc == 0 and eng.fade_remaining() == 0
        eng.close()
    y = np.concatenate([y0, y1, y2])
    assert y.shape == (nb * L, Cn)

    want, _, _ = fade_expected(orc, L, -(-cell["taps"] // L), s, Cn, h_old, h_new, x, t0, K, cell["in_fmt"], cell["out_fmt"])
    _check(cell, y, SM.fade_reference(orc, cell, h_old, h_new, x), want)


# ---- multi-level matrix engines --------------------------------------------------------------------------------------
def _matrix_levels_engine(bfir, creation_log, cell):
    """The engine of a MLEVELS / MFADE cell, its creation log line checked: the back end, one plain engine per level."""
    L, blocks, ratios, n_in, n_out = cell["L"], cell["blocks"], cell["ratios"], cell["n_in"], cell["n_out"]
    Ls, _ = SM.level_geometry(L, blocks, ratios)
    del creation_log[:]
    eng = bfir.BrutefirMatrixLevels(L, blocks, ratios, cell["s"], n_in, n_out, cell["in_fmt"], cell["out_fmt"])
    names = ", ".join("%d x %d" % (Lk, b) for Lk, b in zip(Ls, blocks))
    back = "fused" if cell["family"].endswith("_fused") else "general"
    made = [ln for ln in creation_log if " levels, " in ln]
    assert made == ["bfir engine: matrix %d -> %d, %d levels, %s; back end %s." % (n_in, n_out, len(blocks), names, back)], creation_log
    assert len(_engine_lines(creation_log)) == len(blocks), creation_log         # one matrix engine per level, no more
    return eng


def _check_matrix_spectra(eng, cell, rows):
    """Every partition spectrum of every level and pair against grouped_spectrum, the ragged last one of a filter included; a
    partition a filter does not reach, and every one of the NULL pair, reads as zeros (absent: the MAC skips it by its count)."""
    s, L = cell["s"], cell["L"]
    Ls, D = SM.level_geometry(L, cell["blocks"], cell["ratios"])
    lens = [[None if h is None else h.size for h in row] for row in rows]
    counts = SM.partition_counts(cell, lens)
    for level, (Lp, Bp) in enumerate(zip(Ls, cell["blocks"])):
        for o, row in enumerate(rows):
            for i, h in enumerate(row):
                for b in range(Bp):
                    got = eng.coeff_block(level, o, i, b).astype(np.float64)
                    if b >= counts[level][o][i]:
                        assert not got.any(), (level, o, i, b)
                        continue
                    want = SM.grouped_spectrum(h[D[level] + b * Lp:D[level] + (b + 1) * Lp], Lp, 1.0)
                    assert np.abs(got - want).max() <= TOL[s] * np.abs(want).max(), (level, o, i, b)


@pytest.mark.parametrize("cell", SM.MLEVELS_CELLS, ids=[c["id"] for c in SM.MLEVELS_CELLS])
def test_mlevels_size_matrix(orc, bfir, creation_log, cell):
    s, L, nb = cell["s"], cell["L"], cell["nb"]
    Ls, _ = SM.level_geometry(L, cell["blocks"], cell["ratios"])
    rows, x = SM.mlevels_data(orc, cell)

    with env_override(**cell["env"]):
        eng = _matrix_levels_engine(bfir, creation_log, cell)
        eng.set_chunk(3)
        assert eng.set_coeff(rows) == 0
        _check_matrix_spectra(eng, cell, rows)
        # a call that ends inside a block of the last level, one block alone (the latency path), then the rest
        r_last = Ls[-1] // L
        y = _run_calls(eng, x, L, (0, r_last + 1, r_last + 2, nb))
        eng.close()
    assert y.shape == (nb * L, cell["n_out"])

    _check(cell, y, SM.matrix_reference_conv(orc, rows, x), uniform_reference(orc, L, s, rows, x))


@pytest.mark.parametrize("s,L,n,err", SM.MLEVELS_REFUSALS)
def test_mlevels_refuses_size(bfir, s, L, n, err):
    with pytest.raises(bfir.BfirError) as ei:
        bfir.BrutefirMatrixLevels(L, SM.LEVEL_BLOCKS[n], (1,) + (2,) * (n - 1), s, 2, 3)
    assert ei.value.code == getattr(bfir, err)
    # nothing left behind: the device still makes and runs a three-level 2 -> 3 engine of a supported size
    dt = np.float32 if s == 4 else np.float64
    eng = bfir.BrutefirMatrixLevels(1024, SM.LEVEL_BLOCKS[3], (1, 2, 2), s, 2, 3)
    taps = 4 * 1024 + 10                                                    # ten taps into the last level
    h = np.ones(taps, dt) / 16384
    assert eng.set_coeff([[h, h], [h, None], [None, h]]) == 0
    rc, y = eng.run(np.ones((16 * 1024, 2), dt))
    assert rc == 0 and y.shape == (16 * 1024, 3) and np.all(np.isfinite(y))
    for o, paths in enumerate((2, 1, 1)):                                   # all taps under a constant input: their sum, per path
        assert abs(float(y[-1, o]) - paths * taps / 16384) <= 1e-5, o
    eng.close()


# ---- crossfaded coefficient changes on multi-level matrix engines --------------------------------------------------------
def _wide_mac_spans(cell):
    """MAC launches of the ONE call that holds the whole fade of a wide cell (a profile span is a MAC step, k_mac_duo or
    k_mac_matrix twice): one for the head's K blocks -- every level contributes to all of them, so run_blocks cuts the chunk
    nowhere but at the fade's end -- and three per tail level: the block the call began inside, alone from the kept frames,
    the others up to the last old one (lf_j1: both sets) and the ones after (nup_tail_ahead)."""
    L, t0, K = cell["L"], cell["t0"], cell["K"]
    Ls, D = SM.level_geometry(L, cell["blocks"], cell["ratios"])
    spans = 1
    for Lk, Dk in zip(Ls[1:], D[1:]):
        r = Lk // L
        z_next, j_end, j1 = t0 // r, (t0 + K) // r, (t0 + K - 1 - Dk // L) // r
        assert t0 % r and z_next < j1 < j_end - 1 and max(j1 - z_next, j_end - 1 - j1) <= -(-cell["chunk"] // r)
        spans += 3
    return spans


def _mfade_run(bfir, creation_log, cell, rows_old, rows_new, x, duo):
    """The cell's run with BFIR_MFADE_DUO unset or 0: (output, MAC spans and k_stage_out spans of the first fading call)."""
    L, t0, K = cell["L"], cell["t0"], cell["K"]
    first = K if cell["wide"] else 2
    env = dict(cell["env"], BFIR_MFADE_DUO=duo)
    with env_override(**env):
        eng = _matrix_levels_engine(bfir, creation_log, cell)
        eng.set_chunk(cell["chunk"])         # 2: the fade's K = 3 blocks are cut into 2 + 1; a wide cell: all K in one launch
        assert eng.set_coeff(rows_old) == 0
        rc, y0 = eng.run(x[:t0 * L])
        assert rc == 0
        del creation_log[:]
        assert eng.fade_to_rows(rows_new, K) == 0 and eng.fade_remaining() == K
        said = [ln for ln in creation_log if ln.startswith("bfir matrix engine: crossfade over %d blocks" % K)]
        assert len(said) == 1 and said[0].endswith("runs %s." % ("k_mac_duo" if duo is None else "k_mac_matrix twice")), creation_log
        # the first fading call on its own, profiled
        eng.set_profiling(True)
        rc, y1 = eng.run(x[t0 * L:(t0 + first) * L])
        assert rc == 0 and eng.fade_remaining() == K - first
        prof = eng.profile()
        eng.set_profiling(False)
        # the rest of the fade (m0 = 2 L), the swap of the sets and the blocks after it in one call
        rc, y2 = eng.run(x[(t0 + first) * L:])
        assert rc == 0 and eng.fade_remaining() == 0
        eng.close()
    y = np.concatenate([y0, y1, y2])
    assert y.shape == (cell["nb"] * L, cell["n_out"])
    return y, prof["k_mac"][1], prof["k_stage_out"][1]


@pytest.mark.parametrize("cell", SM.MFADE_CELLS, ids=[c["id"] for c in SM.MFADE_CELLS])
def test_mfade_size_matrix(orc, bfir, creation_log, cell):
    s, L, t0, nb, K = cell["s"], cell["L"], cell["t0"], cell["nb"], cell["K"]
    fused = cell["family"] == "mfade_fused"
    rows_old, rows_new, x = SM.mfade_data(orc, cell)

    y, macs, staged = _mfade_run(bfir, creation_log, cell, rows_old, rows_new, x, None)
    # the fused fade stores the frames itself, the general one ends in k_stage_out
    assert (staged == 0) if fused else (staged > 0), staged
    if cell["wide"]:
        print("%s: MAC spans of the fading call %d" % (cell["id"], macs))
        assert macs == _wide_mac_spans(cell)
        # k_mac_duo's specification is the bytes of two k_mac_matrix launches, which MATRIX_CELLS check at these time tiles
        y2, macs2, _ = _mfade_run(bfir, creation_log, cell, rows_old, rows_new, x, 0)
        assert macs2 == macs
        assert y.tobytes() == y2.tobytes()

    w = fade_weights(L, nb, t0, K)[:, None]
    want = uniform_reference(orc, L, s, rows_old, x) * (1.0 - w) + uniform_reference(orc, L, s, rows_new, x) * w
    _check(cell, y, SM.fade_reference(orc, cell, rows_old, rows_new, x), want)
