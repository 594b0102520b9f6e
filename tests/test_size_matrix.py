"""The size matrix of tests/test_size_matrix_gpu.py against the sources, on the CPU: adding a transform size to the
kernels or moving a size limit fails here until the matrix follows."""
import numpy as np
import pytest

import size_matrix as SM


def test_matrix_covers_exactly_what_the_sources_support():
    lim = SM.source_limits()
    want = SM.supported_set(lim)
    have = {(c["family"], c["s"], c["L"]) for c in SM.CELLS}
    assert sorted(want - have) == [], "sizes the build supports that no cell runs"
    assert sorted(have - want) == [], "cells at sizes the build does not support"


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


def test_cells_set_every_path_switch_and_are_unique():
    ids = [c["id"] for c in SM.CELLS]
    assert len(ids) == len(set(ids))
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
