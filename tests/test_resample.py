"""The resampler without a device: bfir_resample_filter against the definition restated in tests/resample_cells.py, the index
arithmetic, the limits, that the taps resample a sine, the margins of the bound the GPU test applies, the file mirror
(foo_dsp_bfir_amd.buffer) and the GPU cell table against csrc/resample.hip."""
import ctypes as C
import json
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import resample_cells as RC


# ---- taps ---------------------------------------------------------------------------------------------------------------
def _library_taps(bfir, in_rate, out_rate, Z, beta, cutoff, gain, s, p, K):
    lib = bfir.load()
    out = np.zeros((p, K), RC.DTYPE[s])
    k = C.c_int(0)
    for ph in range(p):
        assert lib.bfir_resample_filter(in_rate, out_rate, Z, beta, cutoff, gain, s, ph, out[ph].ctypes.data, C.byref(k)) == 0
        assert k.value == K
    return out


@pytest.mark.parametrize("ratio", RC.RATIOS, ids=["%d-%d" % r for r in RC.RATIOS])
def test_taps_match_the_definition(bfir, ratio):
    """Every phase, Z 1 / 16 / 128, beta 0 / 9, both ends of the cutoff, both precisions:
    |tap - model| <= u_R |model| + 1e-14 rho |gain| (the second term: the model's own error where it runs in float64)."""
    out_rate, in_rate = ratio
    for Z in (1, 16, 128):
        for beta in (0.0, 9.0):
            for cutoff in (0.5, 1.0):
                gain = 1.0 if Z != 16 else -0.75
                p, q, rho, W, Wc, K = RC.geometry(in_rate, out_rate, Z, cutoff)
                model = RC.model_taps(in_rate, out_rate, Z, beta, cutoff, gain)
                assert model.shape == (p, K) and np.all(np.isfinite(model))
                assert bfir.resample_taps(in_rate, out_rate, Z, beta, cutoff, gain, 4) == K
                for s in (4, 8):
                    taps = _library_taps(bfir, in_rate, out_rate, Z, beta, cutoff, gain, s, p, K)
                    err = np.abs(taps.astype(RC.LD) - model)
                    tol = RC.U[s] * np.abs(model) + 1e-14 * float(rho) * abs(gain)
                    assert np.all(err <= tol), (Z, beta, cutoff, s, float((err / tol).max()))
                # the shape of the thing: unit gain at DC per phase (the window leaks a little), symmetric about phase 0's centre
                if beta == 9.0 and Z >= 16:
                    assert abs(float(model.sum(axis=1).max()) / gain - 1.0) < 1e-3
                assert np.array_equal(model[0, :K - 1], model[0, K - 2::-1])


def test_tap_positions():
    """Tap j of phase ph sits at u = ph / p + Wc - 1 - j: tap Wc - 1 of phase 0 is the centre, gain rho."""
    m = RC.model_taps(147, 160, 16, 9.0, 0.9, 2.0)
    p, q, rho, W, Wc, K = RC.geometry(147, 160, 16, 0.9)
    assert float(m[0, Wc - 1]) == 2.0 * 0.9 and np.argmax(m[0]) == Wc - 1
    assert m[0, K - 1] == 0 and m[0, 0] != 0            # u = -Wc is outside the window, u = Wc - 1 inside
    assert np.argmax(m[p - 1]) == Wc and m[p - 1, Wc - 1] > m[p - 1, Wc + 1] > 0     # a late phase sits just before the next input frame


# ---- index arithmetic -----------------------------------------------------------------------------------------------------
def test_geometry_is_exact(bfir):
    """K = 2 ceil(Z / rho) in exact rationals, also where W is whole (1 -> 3 at cutoff 1) or a hair off it."""
    just_below_1 = float(np.nextafter(1.0, 0.0))
    for in_rate, out_rate, Z, cutoff in [(3, 1, 5, 1.0), (3, 1, 128, 1.0), (7, 3, 3, 1.0), (7, 3, 3, just_below_1), (48000, 44100, 64, 0.95),
                                         (44100, 48000, 64, 0.95), (96000, 44100, 64, 0.95), (8, 1, 128, 0.5), (2048, 1, 1, 1.0),
                                         (3, 1, 5, just_below_1), (10, 1, 100, 0.625)]:
        p, q, rho, W, Wc, K = RC.geometry(in_rate, out_rate, Z, cutoff)
        assert Wc - 1 < W <= Wc and bfir.resample_taps(in_rate, out_rate, Z, 9.0, cutoff, 1.0, 8) == K, (in_rate, out_rate, Z, cutoff)
    assert RC.geometry(3, 1, 5, 1.0)[4] == 15 and RC.geometry(3, 1, 5, just_below_1)[4] == 16
    assert RC.geometry(44100, 96000, 64, 0.95)[0] == 320 and RC.geometry(44100, 48000, 64, 0.95)[:2] == (160, 147)


def test_positions_hold_to_2_to_the_33():
    """n0 / phase / n_out as the reference model computes them in int64 against exact integers, for m up to 2^33."""
    rng = np.random.default_rng(5)
    for p, q in [(160, 147), (147, 160), (320, 147), (147, 320), (7, 3), (1, 2048), (1 << 20, 1)]:
        ms = np.concatenate([rng.integers(0, 1 << 33, 200), [0, 1, (1 << 32) // q, (1 << 32) // q + 1, (1 << 33) - 1, 1 << 33]]).astype(np.int64)
        n0, ph = RC.position(ms, p, q)
        for m, a, b in zip(ms.tolist(), n0.tolist(), ph.tolist()):
            assert (a, b) == divmod(m * q, p) and Fraction(m * q, p) == a + Fraction(b, p)
        for n_in in (0, 1, 5, q, q + 1, (1 << 33) + 7):
            got = RC.n_out(n_in, p, q)
            assert got == math.ceil(Fraction(n_in * p, q)) and (got == 0 or RC.position(got - 1, p, q)[0] < n_in)
            assert RC.position(got, p, q)[0] >= n_in          # the next frame would sit at or past the input's end
    assert (RC.BIG_CELL["n_out"] - 1) * RC.BIG_CELL["q"] >= 1 << 32


# ---- limits ---------------------------------------------------------------------------------------------------------------
def _filter_rc(bfir, *args, phase=0):
    k = C.c_int(0)
    return bfir.load().bfir_resample_filter(*args, phase, None, C.byref(k))


def test_limits(bfir):
    lim = RC.limits()
    assert lim == {"tile": 256, "lds": 65536, "max_taps": 4096, "max_table": 1 << 22}
    ok, A, U = 0, bfir.ERR_ARG, bfir.ERR_UNSUPPORTED
    assert _filter_rc(bfir, 8, 1, 128, 9.0, 0.5, 1.0, 8) == ok and bfir.resample_taps(8, 1, 128, 9.0, 0.5, 1.0, 8) == 4096
    assert _filter_rc(bfir, 8, 1, 128, 9.0, float(np.nextafter(0.5, 1.0)), 1.0, 8) == ok            # K = 4096 still
    assert _filter_rc(bfir, 9, 1, 128, 9.0, 0.5, 1.0, 8) == U                                       # K = 4608
    assert _filter_rc(bfir, 2049, 1, 1, 9.0, 1.0, 1.0, 4) == U                                      # K = 4098
    assert _filter_rc(bfir, 1, 16384, 128, 9.0, 1.0, 1.0, 4) == ok                                  # p K = 2^22
    assert _filter_rc(bfir, 1, 16385, 128, 9.0, 1.0, 1.0, 4) == U                                   # p K > 2^22
    assert _filter_rc(bfir, 44100, 96000, 128, 9.0, 0.5, 1.0, 4) == ok
    for args in [(0, 1, 16, 9.0, 0.9, 1.0, 4), (1, 0, 16, 9.0, 0.9, 1.0, 4), (-1, 1, 16, 9.0, 0.9, 1.0, 4), (2, 3, 0, 9.0, 0.9, 1.0, 4),
                 (2, 3, 129, 9.0, 0.9, 1.0, 4), (2, 3, 16, -1.0, 0.9, 1.0, 4), (2, 3, 16, float("nan"), 0.9, 1.0, 4),
                 (2, 3, 16, float("inf"), 0.9, 1.0, 4), (2, 3, 16, 9.0, 0.4999, 1.0, 4), (2, 3, 16, 9.0, 1.0001, 1.0, 4),
                 (2, 3, 16, 9.0, float("nan"), 1.0, 4), (2, 3, 16, 9.0, 0.9, float("inf"), 4), (2, 3, 16, 9.0, 0.9, 1.0, 2),
                 (2, 3, 16, 9.0, 0.9, 1.0, 16)]:
        assert _filter_rc(bfir, *args) == A, args
    assert _filter_rc(bfir, 2, 3, 16, 9.0, 0.9, 1.0, 4, phase=3) == A and _filter_rc(bfir, 2, 3, 16, 9.0, 0.9, 1.0, 4, phase=-1) == A
    assert _filter_rc(bfir, 2, 3, 16, 9.0, 0.9, 1.0, 4, phase=2) == ok
    assert bfir.load().bfir_resample_filter(2, 3, 16, 9.0, 0.9, 1.0, 4, 0, None, None) == A          # nowhere to put anything
    assert _filter_rc(bfir, 6, 9, 16, 9.0, 0.9, 1.0, 4, phase=3) == A                               # 6 -> 9 is 2 -> 3: three phases


def test_create_checks_arguments_before_the_device(bfir):
    lib = bfir.load()
    err = C.c_int(0)
    mk = lambda *a: (lib.bfir_resampler_create(*a, C.byref(err)), err.value)
    assert mk(44100, 48000, 64, 9.0, 0.95, 1.0, 4, 0, 0) == (None, bfir.ERR_ARG)
    assert mk(44100, 48000, 64, 9.0, 0.95, 1.0, 4, 9, 0) == (None, bfir.ERR_ARG)
    assert mk(44100, 48000, 200, 9.0, 0.95, 1.0, 4, 2, 0) == (None, bfir.ERR_ARG)
    assert mk(9, 1, 128, 9.0, 0.5, 1.0, 8, 2, 0) == (None, bfir.ERR_UNSUPPORTED)
    assert lib.bfir_resampler_out_frames(None, 5) == bfir.ERR_ARG and lib.bfir_resampler_run(None, None, 0, None, 0) == bfir.ERR_ARG
    assert lib.bfir_resampler_run_device(None, None, 0, None, 0) == bfir.ERR_ARG
    lib.bfir_resampler_destroy(None)
    if lib.bfir_device_count() > 0:
        return
    assert mk(44100, 48000, 64, 9.0, 0.95, 1.0, 4, 2, 0) == (None, bfir.ERR_NO_DEVICE)          # never a CPU stand-in
    assert mk(48000, 48000, 64, 9.0, 0.95, 1.0, 8, 1, 0) == (None, bfir.ERR_NO_DEVICE)
    with pytest.raises(bfir.BfirError) as ei:
        bfir.Resampler(44100, 48000, channels=2)
    assert ei.value.code == bfir.ERR_NO_DEVICE


# ---- it is a resampler ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", RC.RATIOS + [(3, 7)], ids=["%d-%d" % r for r in RC.RATIOS + [(3, 7)]])
def test_a_sine_comes_out_as_the_same_sine_at_the_new_rate(bfir, ratio):
    """The library's own taps (fp64) and a float64 dot product: a sine at 0.2 of the lower Nyquist, 4000 frames, within 2e-5
    away from 2 K p / q frames at each end -- three times what the float64 model of the definition reached (6.8e-6 at Z = 16).
    The inverted ratio misses by orders of magnitude."""
    out_rate, in_rate = ratio
    n_in = 4000
    for Z, cutoff in ((16, 0.9), (32, 0.95), (64, 0.95)):
        cell = dict(in_rate=in_rate, out_rate=out_rate, Z=Z, beta=9.0, cutoff=cutoff, gain=1.0, s=8)
        p, q, rho, W, Wc, K = RC.geometry(in_rate, out_rate, Z, cutoff)
        w = 0.2 * math.pi * min(1.0, p / q)                     # radians per input frame: 0.2 of the lower Nyquist
        x = np.sin(w * np.arange(n_in, dtype=np.float64))[:, None]
        T = RC.table(bfir, cell)
        n = RC.n_out(n_in, p, q)
        edge = -(-2 * K * p // q)
        frames = np.arange(edge, n - edge, dtype=np.int64)
        assert frames.size > 500
        X, phase = RC.gather(x, frames, p, q, Wc)
        y = np.einsum("mk,mk->m", T[phase], X[:, :, 0])
        want = np.sin(w * frames.astype(np.float64) * q / p)
        err = float(np.abs(y - want).max())
        print("%d/%d Z %d cutoff %.2f: %.3g" % (out_rate, in_rate, Z, cutoff, err))
        assert err <= 2e-5, (Z, cutoff, err)
        wrong = np.sin(w * frames.astype(np.float64) * p / q)
        assert p == q or float(np.abs(y - wrong).max()) > 1e-2


# ---- the margin of the bound ------------------------------------------------------------------------------------------------
def _sample_frames(cell):
    """every frame of a small cell; of the large one the last two tiles and 2000 frames across the run"""
    if cell["n_out"] <= 4096:
        return np.arange(cell["n_out"], dtype=np.int64)
    rng = np.random.default_rng(7)
    return np.unique(np.concatenate([rng.integers(0, cell["n_out"], 2000), np.arange(cell["n_out"] - 2 * cell["tile"], cell["n_out"])]))


SMALL = RC.CELLS + RC.IMPULSE_CELLS


@pytest.mark.parametrize("cell", SMALL, ids=[c["id"] for c in SMALL])
def test_the_bound_holds_for_the_kernel_arithmetic_and_sees_the_mutations(bfir, cell):
    """An emulation of k_resample in working precision stays inside the bound the GPU test applies, on every sample; with beta
    0 or Z = 1 a kernel that drops tap K - 1, starts its window one frame off or steps by p instead of q leaves it."""
    T = RC.table(bfir, cell)
    x = RC.audio(cell)
    frames = _sample_frames(cell)
    p, q, Wc, K, s = cell["p"], cell["q"], cell["Wc"], cell["K"], cell["s"]
    ref, amp = RC.reference(T, x, frames, p, q, Wc)
    bound = RC.bound(s, K, ref, amp)
    err = np.abs(RC.emulate(T, x, frames, p, q, Wc, s).astype(RC.LD) - ref).astype(np.float64)
    assert np.all(err <= bound), float((err / np.maximum(bound, 1e-300)).max())
    assert np.abs(ref).max() > 0.01 and bound.max() <= 1e-2 * float(np.abs(ref).max())          # not vacuous
    if cell["beta"] == 0.0 or cell["Z"] == 1:
        for kw in (dict(drop_last=True), dict(shift=1), dict(shift=-1), dict(step=p)):
            cut = np.abs(RC.emulate(T, x, frames, p, q, Wc, s, **kw).astype(RC.LD) - ref).astype(np.float64)
            assert np.all(np.any(cut > bound, axis=0)), kw


def test_some_cells_see_the_mutations():
    seeing = [c["id"] for c in RC.FILTERED if c["beta"] == 0.0 or c["Z"] == 1]
    assert len(seeing) >= 8 and {c["s"] for c in RC.FILTERED if c["beta"] == 0.0} == {4, 8}


# ---- the cell table against the source ------------------------------------------------------------------------------------------
def test_cells_name_exactly_the_instances_the_source_launches():
    src = RC.source_instances()
    assert src == {("float", "float"), ("double", "double")}
    assert {c["instance"] for c in RC.CELLS} == src and {c["instance"] for c in RC.IMPULSE_CELLS} == src
    ids = [c["id"] for c in RC.FILTERED]
    assert len(ids) == len(set(ids))


def test_cells_reach_every_tile_edge():
    lim = RC.limits()
    TILE = lim["tile"]
    by = lambda key: [c for c in RC.CELLS if c["id"].startswith(key)]
    for s in (4, 8):
        for d in ("b-up-", "b-down-"):
            mine = [c for c in by(d) if c["s"] == s]
            assert all(c["tile"] == TILE and c["C"] == 2 for c in mine)
            assert sorted(c["n_out"] for c in mine) == [TILE, TILE + 1, 3 * TILE - 1]
        assert {(c["out_rate"], c["in_rate"]) for c in by("b-") if c["s"] == s} == {(160, 147), (147, 160)}
        (a,) = [c for c in by("a-") if c["s"] == s]
        assert a["n_in"] == 5 and a["C"] == 3 and a["Z"] == 16 and a["n_out"] == 6 and a["n_in"] < a["Wc"]      # every window hangs over both ends
        (d,) = [c for c in by("d-") if c["s"] == s]
        assert d["K"] == 2 and d["beta"] == 0.0 and d["cutoff"] == 1.0 and (d["p"], d["q"]) == (3, 2) and d["n_out"] > 4 * TILE
        h = [c for c in by("h-") if c["s"] == s]
        assert sorted(c["C"] for c in h) == [1, 3, 8] and all(c["n_out"] > TILE and c["offset"] % s == 0 and c["offset"] % 16 for c in h)
        assert all((c["n_out"] * c["C"] * s) % 16 for c in h if c["C"] != 8)
    # the largest window and the largest LDS request a launch can make: K at its limit, 8 channels of doubles, exactly the limit
    (c,) = by("c-largest")
    assert c["K"] == lim["max_taps"] and c["C"] == 8 and c["s"] == 8 and (c["p"], c["q"]) == (1, 8) and c["n_out"] == 2 * c["tile"]
    assert c["tile"] == TILE and RC.lds_of(c["p"], c["q"], c["K"], c["C"], c["s"], lim) == lim["lds"]
    assert max(RC.lds_of(x["p"], x["q"], x["K"], x["C"], x["s"], lim) for x in RC.FILTERED) == lim["lds"]
    # ... and where a whole tile's request does not fit, the tile shrinks: halved, and down to 8
    (c,) = by("c-halved")
    assert c["K"] == lim["max_taps"] and c["tile"] == TILE // 2 and c["n_out"] == 2 * c["tile"] + 1
    assert RC.out_bytes(TILE, 8, 8) + RC.width(TILE, c["p"], c["q"], c["K"]) * 8 > lim["lds"]
    (c,) = by("c-small")
    assert c["tile"] == 8 and c["n_out"] == 17 and c["s"] == 4
    # no shape the limits allow asks for more than a launch may: the extremes of K, q / p, channels and sample size
    for p, q, K in [(1, 8, 4096), (1, 2048, 4096), (1, 2047, 4094), (160, 147, 4096), (147, 160, 2), (1, 1024, 2048)]:
        for Cn in (1, 8):
            for s in (4, 8):
                t = RC.tile_of(p, q, K, Cn, s, lim)
                assert t >= 1 and RC.lds_of(p, q, K, Cn, s, lim) <= lim["lds"], (p, q, K, Cn, s)
    big = RC.BIG_CELL
    assert big["C"] == 1 and big["s"] == 4 and (big["n_out"] - 1) * big["q"] >= 1 << 32 and big["n_in"] * 4 < 120e6


# ---- the file mirror ----------------------------------------------------------------------------------------------------------
def _wav(bfir, path, n, ch, rate, dtype=np.float32, seed=3):
    from foo_dsp_bfir_amd import wavio
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, ch)) * np.exp(-np.arange(n) / (n / 6.0))[:, None]).astype(dtype)
    wavio.write_wav_float(str(path), x, rate)
    return x


def test_cache_name_carries_the_reference_hash(bfir):
    cases = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "djb_hash_ref.json")))["cases"]
    seen = 0
    for c in cases:
        raw = bytes.fromhex(c["hex"])
        assert bfir.buffer.cache_name(raw, 2, 48000) == "ir-%x-2-48000.wav" % c["djb"]
        if raw and all(32 <= b < 127 for b in raw):
            assert bfir.buffer.cache_name(raw.decode("ascii"), 2, 48000) == "ir-%x-2-48000.wav" % c["djb"]
            seen += 1
    assert len(cases) >= 15
    assert bfir.buffer.cache_name("a", 8, 44100) == "ir-%x-8-44100.wav" % 177670


def test_params_check_and_load(bfir, tmp_path):
    B = bfir.buffer
    x = _wav(bfir, tmp_path / "ir.wav", 100, 3, 44100)
    f = str(tmp_path / "ir.wav")
    assert B.get_snd_file_params(f) == (3, 100, 44100)
    assert B.check_snd_file(f, 3, 44100) and not B.check_snd_file(f, 2, 44100) and not B.check_snd_file(f, 3, 48000)
    (tmp_path / "not.flac").write_bytes(b"fLaC" + bytes(64))                       # another container: refused, not raised
    assert B.get_snd_file_params(str(tmp_path / "not.flac")) is None and not B.check_snd_file(str(tmp_path / "not.flac"), 3, 44100)
    assert B.get_snd_file_params(str(tmp_path / "absent.wav")) is None
    assert B.load_from_snd_file(str(tmp_path / "absent.wav"), 4) is None
    # buffer.cpp:60-71: n_frames = the file's, or max_frames where it has more; pad: a buffer of max_frames, the rest zero
    buf, n = B.load_from_snd_file(f, 4)
    assert n == 100 and buf.dtype == np.float32 and np.array_equal(buf, x)
    buf, n = B.load_from_snd_file(f, 8, 40, False)
    assert n == 40 and buf.dtype == np.float64 and np.array_equal(buf, x[:40].astype(np.float64))
    buf, n = B.load_from_snd_file(f, 4, 250, False)
    assert n == 100 and buf.shape == (100, 3)
    buf, n = B.load_from_snd_file(f, 4, 250, True)
    assert n == 100 and buf.shape == (250, 3) and np.array_equal(buf[:100], x) and not buf[100:].any()
    buf, n = B.load_from_snd_file(f, 4, 40, True)
    assert n == 40 and buf.shape == (40, 3)
    assert B.load_from_snd_file(f, 4, -1, True) is None
    # interlace / deinterlace
    parts = B.deinterlace(x)
    assert len(parts) == 3 and all(a.flags.c_contiguous and np.array_equal(a, x[:, c]) for c, a in enumerate(parts))
    assert B.interlace(parts).tobytes() == x.tobytes() and B.interlace(parts, 2).tobytes() == np.ascontiguousarray(x[:, :2]).tobytes()
    coeffs, length = B.load_snd_coeff(f, 8, 64)
    assert length == 64 and len(coeffs) == 3 and np.array_equal(coeffs[2], x[:64, 2].astype(np.float64))
    B.save_to_snd_file(str(tmp_path / "out.wav"), x.astype(np.float64), 8, 96000)
    assert B.get_snd_file_params(str(tmp_path / "out.wav")) == (3, 100, 96000)
    assert np.array_equal(B.load_from_snd_file(str(tmp_path / "out.wav"), 8)[0], x.astype(np.float64))


def test_resample_snd_file_cache_and_refusals(bfir, tmp_path):
    B = bfir.buffer
    _wav(bfir, tmp_path / "ir.wav", 100, 2, 44100)
    f, cache = str(tmp_path / "ir.wav"), tmp_path / "cache"
    cache.mkdir()
    assert B.resample_snd_file(f, 3, 48000, str(cache)) == ""                      # fewer channels than asked
    assert B.resample_snd_file(str(tmp_path / "absent.wav"), 2, 48000, str(cache)) == ""
    assert not list(cache.iterdir())
    # an existing cache file is reused untouched, whatever it holds
    hit = cache / B.cache_name(f, 2, 48000)
    hit.write_bytes(b"kept as it is")
    assert B.resample_snd_file(f, 2, 48000, str(cache)) == str(hit) and hit.read_bytes() == b"kept as it is"
    if bfir.load().bfir_device_count() == 0:                                       # no device: the empty string, no file, no CPU stand-in
        assert B.resample_snd_file(f, 1, 48000, str(cache)) == "" and sorted(p.name for p in cache.iterdir()) == [hit.name]


def test_set_coeff_from_a_file_without_a_device(bfir, tmp_path):
    """The checks in front of the device: an incompatible or unreadable file is -1.  Without a GPU no engine exists to go
    further (the constructor raises ERR_NO_DEVICE)."""
    _wav(bfir, tmp_path / "ir.wav", 100, 2, 44100)
    f = str(tmp_path / "ir.wav")
    eng = bfir.Brutefir.__new__(bfir.Brutefir)                                   # the checks need no device
    eng.L, eng.B, eng.s, eng.C, eng.sampling_rate, eng._h = 64, 2, 4, 2, 48000, None
    assert eng.set_coeff(f, 2, 1.0) == -1 and eng.set_coeff_file(f) == -1         # 44100 on a 48000 engine
    eng.sampling_rate, eng.C = 44100, 3
    assert eng.set_coeff(f, 2, 1.0) == -1                                          # 2 channels on a 3-channel engine
    eng.C = 2
    assert eng.set_coeff(str(tmp_path / "absent.wav"), 2, 1.0) == -1
    if bfir.load().bfir_device_count() == 0:
        with pytest.raises(bfir.BfirError) as ei:
            bfir.Brutefir(64, 2, 4, 2)
        assert ei.value.code == bfir.ERR_NO_DEVICE
