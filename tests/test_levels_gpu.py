"""Multi-level partitioned engines on the GPU (bfir_engine_create_levels / _set_coeff_levels / _read_coeff_levels).

The reference is the uniform oracle engine of the same partition length and taps, Engine(L, ceil(taps / L)), compared with
rel_err <= TOL of conftest; test_levels.test_levels_compose_to_the_uniform_engine pins the multi-level definition to it on
the CPU.  Runs are nb >= D_last / L + (L_last / L) (blocks_last + 2) + 3 blocks long, so the deepest delay line and its ring
both wrap; the taps end inside the last partition of the last level."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import TOL, rel_err
from test_levels import level_geometry

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = 8, 10


def _real(s):
    return np.float64 if s == 8 else np.float32


def _fdt(fmt):
    return np.float64 if fmt == F64 else np.float32


def _fmt(s, fmt):
    return (F64 if s == 8 else F32) if fmt is None else fmt


def _geo(shape):
    """L_k, D_k (capacity appended) and r_k = L_k / L of a shape."""
    s, L, blocks, ratios, Cn = shape
    Ls, D = level_geometry(L, blocks, ratios)
    return Ls, D, [Lk // L for Lk in Ls]


def _taps(shape):
    Ls, D, _ = _geo(shape)
    return D[-2] + (shape[2][-1] - 1) * Ls[-1] + Ls[-1] // 3 + 1        # ends inside the last partition of the last level


def _nb(shape):
    Ls, D, r = _geo(shape)
    return D[-2] // shape[1] + r[-1] * (shape[2][-1] + 2) + 3


def _settle(shape):
    """Blocks after which nothing computed before a coefficient change is left in any level: its ring has played out
    (D_k / L + r_k blocks) and a delay line that started empty is full (r_k blocks_k more)."""
    Ls, D, r = _geo(shape)
    return max(D[k] // shape[1] + r[k] * (shape[2][k] + 2) for k in range(len(Ls)))


def _make(orc, shape, fmt=None, seed=0, nb=None):
    s, L, blocks, ratios, Cn = shape
    rng = np.random.default_rng(2000 + L + sum(blocks) + Cn + seed)
    h = orc.synth_ir(rng, Cn, _taps(shape), _real(s))
    x = orc.synth_audio(rng, (nb or _nb(shape)) * L, Cn, _fdt(_fmt(s, fmt)))
    return h, x


def _uniform(orc, shape, h, x, fmt=None, scale=1.0):
    """The uniform oracle's output (read-only) and overflow records."""
    s, L, blocks, ratios, Cn = shape
    ref = orc.Engine(L, -(-h[0].size // L), s, Cn, fmt, fmt)
    assert ref.set_coeff(h, scale=scale) == 0
    rc, y = ref.run(x)
    assert rc == 0
    ofs = [ref.overflow(c) for c in range(Cn)]
    ref.close()
    y = np.asarray(y, dtype=np.float64)
    y.setflags(write=False)
    return y, ofs


def _engine(bfir, shape, h, fmt=None, chunk=3, scale=1.0):
    s, L, blocks, ratios, Cn = shape
    eng = bfir.BrutefirLevels(L, blocks, ratios, s, Cn, fmt, fmt)
    if chunk is not None:
        eng.set_chunk(chunk)
    assert not eng.is_initialized()
    assert eng.set_coeff(h, scale=scale) == 0
    assert eng.is_initialized()
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


# (s, L, blocks, ratios, C), frame format (None = the working precision's), back end
PARITY = [
    ((4, 16, (2, 2, 3), (1, 2, 2), 1), None, "general"),             # smallest; D_1 = L_1
    ((4, 512, (4, 2, 2), (1, 4, 2), 2), None, "fused"),              # fused, smallest L, two rings
    ((4, 512, (5, 3, 2), (1, 4, 2), 4), None, "fused"),              # D_1 = 2560, D_2 = 8704: ring reads that start mid-block of the level
    ((4, 512, (2, 2, 2, 2), (1, 2, 2, 2), 4), None, "fused"),        # four levels, three rings, every D_k = L_k or just above
    ((4, 1024, (4, 4, 1), (1, 4, 4), 2), None, "fused"),             # L_2 = 16384, the largest fp32 transform
    ((4, 512, (4, 2, 2), (1, 4, 2), 3), None, "general"),            # odd count
    ((8, 64, (4, 3, 5), (1, 2, 2), 3), None, "general"),             # fp64
    ((8, 1024, (8, 2, 2), (1, 4, 2), 2), F32, "general"),            # float32 frames: the plug-in shape, L_2 = 8192, the largest fp64 transform
]
FUSED, GENERAL, F64_SHAPE = PARITY[1][0], (4, 64, (3, 3, 2), (1, 2, 2), 3), PARITY[6][0]


def _id(shape):
    s, L, blocks, ratios, Cn = shape
    return "%d-%d-%s-%s-%d" % (s, L, "x".join(map(str, blocks)), "x".join(map(str, ratios)), Cn)


@pytest.mark.parametrize("shape,fmt,back", PARITY, ids=[_id(p[0]) for p in PARITY])
def test_parity_with_the_uniform_oracle(orc, bfir, log, shape, fmt, back):
    s, L, blocks, ratios, Cn = shape
    Ls, _, _ = _geo(shape)
    h, x = _make(orc, shape, fmt)
    want, ofs = _uniform(orc, shape, h, x, fmt)
    eng = _engine(bfir, shape, h, fmt, chunk=3)
    names = ", ".join("%d x %d" % (Lk, b) for Lk, b in zip(Ls, blocks))
    assert [ln for ln in log if "%d levels, %s;" % (len(blocks), names) in ln and ln.endswith("back end %s." % back)], log
    rc, y = eng.run(x)
    assert rc == 0
    print("rel_err", shape, rel_err(y, want))
    assert rel_err(y, want) <= TOL[s]
    for c in range(Cn):
        o, ref = eng.overflow(c), ofs[c]
        assert o.max == ref.max == 1.0
        print("peak", c, o.largest, ref.largest)
        assert abs(o.largest - ref.largest) <= TOL[s] * max(ref.largest, 1e-30)
        assert o.n_overflows == ref.n_overflows == 0
    eng.close()


@pytest.mark.parametrize("shape", [(4, 512, (4, 2), (1, 4), 2), (4, 256, (4, 2), (1, 4), 3)], ids=["fused", "general"])
def test_two_levels_are_the_two_level_engine_bit_for_bit(orc, bfir, shape):
    s, L, blocks, ratios, Cn = shape
    h, x = _make(orc, shape)
    nup = bfir.BrutefirNup(L, blocks[0], ratios[1], blocks[1], s, Cn)
    nup.set_chunk(3)
    assert nup.set_coeff(h) == 0
    rc0, y0 = nup.run(x)
    eng = _engine(bfir, shape, h, chunk=3)
    assert eng.D == [0, nup.D] and eng.max_taps == nup.max_taps
    rc, y = eng.run(x)
    assert rc == rc0 == 0 and np.array_equal(y, y0)
    for c in range(Cn):
        assert eng.overflow(c).largest == nup.overflow(c).largest
    eng.close(); nup.close()


@pytest.mark.parametrize("shape", [FUSED, F64_SHAPE], ids=["fused", "f64"])
def test_short_filters_are_the_smaller_engines_bit_for_bit(orc, bfir, shape):
    """Taps that end at or before D_2: the two-level engine's bytes; at or before D_1: the plain engine's."""
    s, L, blocks, ratios, Cn = shape
    _, D, _ = _geo(shape)
    _, x = _make(orc, shape)
    rng = np.random.default_rng(7)
    for taps in (D[2], D[2] - 7, D[1], D[1] - 7):
        h = orc.synth_ir(rng, Cn, taps, _real(s))
        if taps > D[1]:
            small = bfir.BrutefirNup(L, blocks[0], ratios[1], blocks[1], s, Cn)
        else:
            small = bfir.Brutefir(L, blocks[0], s, Cn)
        small.set_chunk(3)
        assert small.set_coeff(h) == 0
        rc0, y0 = small.run(x)
        eng = _engine(bfir, shape, h, chunk=3)
        rc, y = eng.run(x)
        assert rc == rc0 == 0 and np.array_equal(y, y0), taps
        for c in range(Cn):
            assert eng.overflow(c).largest == small.overflow(c).largest
        eng.close(); small.close()


@pytest.mark.parametrize("shape", [PARITY[2][0], GENERAL], ids=["fused", "general"])
def test_output_does_not_depend_on_how_the_blocks_arrive(orc, bfir, shape):
    import torch
    s, L, blocks, ratios, Cn = shape
    _, _, r = _geo(shape)
    nb = _nb(shape) + 2
    h, x = _make(orc, shape, nb=nb)
    want, _ = _uniform(orc, shape, h, x)
    eng = _engine(bfir, shape, h, chunk=None)                            # one call, the default chunk
    rc, one = eng.run(x)
    assert rc == 0
    eng.close()
    assert rel_err(one, want) <= TOL[s]
    for chunk in (1, 3):
        eng = _engine(bfir, shape, h, chunk=chunk)
        rc, y = eng.run(x)
        assert rc == 0 and np.array_equal(y, one), chunk
        eng.close()
    # the plug-in's pattern: one run() per block (the latency path), then uneven calls of a few blocks
    for steps in ([1] * nb, [1, 2, 5, 3, 7, 1, 1, 4, 6, 2, 5, 3, 4, 1, 9]):
        eng = _engine(bfir, shape, h, chunk=None)
        parts, b = [], 0
        for n in steps:
            n = min(n, nb - b)
            if n <= 0:
                break
            rc, y = eng.run(x[b * L:(b + n) * L]); assert rc == 0
            parts.append(y); b += n
        if b < nb:
            rc, y = eng.run(x[b * L:]); assert rc == 0
            parts.append(y)
        assert np.array_equal(np.concatenate(parts), one), steps[:3]
        eng.close()
    # device pointers, two calls that split a block of every level
    eng = _engine(bfir, shape, h, chunk=5)
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.zeros_like(d_in)
    torch.cuda.synchronize()
    cut = r[-1] + 1
    fb = Cn * x.dtype.itemsize
    eng.run_device(d_in.data_ptr(), d_out.data_ptr(), cut)
    eng.run_device(d_in.data_ptr() + cut * L * fb, d_out.data_ptr() + cut * L * fb, nb - cut)
    assert eng.sync() == 0
    assert np.array_equal(d_out.cpu().numpy(), one)
    eng.close()


@pytest.mark.parametrize("shape", [FUSED, F64_SHAPE], ids=["fused", "f64"])
def test_set_coeff_mid_stream(orc, bfir, shape):
    """After a second set_coeff_levels and `settle` further blocks the output is the uniform oracle's with the new filters
    fed the whole stream; also from a set that ends below D_2 (level 2 starts mid-stream), to one (it stops and its queued
    output plays out) and back."""
    s, L, blocks, ratios, Cn = shape
    _, D, r = _geo(shape)
    settle = _settle(shape)
    n1 = r[-1] + 3                                                       # the change falls inside a block of every level
    n2 = settle + 3
    nb = n1 + n2 + settle + 4
    h2, x = _make(orc, shape, nb=nb)
    h1, _ = _make(orc, shape, seed=5, nb=1)
    short = [c[:D[2] - 5] for c in h2]
    want, _ = _uniform(orc, shape, h2, x)
    want_s, _ = _uniform(orc, shape, short, x)
    for first in (h1, [c[:D[2] - 5] for c in h1]):
        eng = _engine(bfir, shape, first, chunk=3)
        assert eng.run(x[:n1 * L])[0] == 0
        assert eng.set_coeff(h2) == 0
        rc, y = eng.run(x[n1 * L:(n1 + settle + 4) * L])
        assert rc == 0
        print("rel_err", shape, rel_err(y[settle * L:], want[(n1 + settle) * L:(n1 + settle + 4) * L]))
        assert rel_err(y[settle * L:], want[(n1 + settle) * L:(n1 + settle + 4) * L]) <= TOL[s]
        eng.close()
    # level 2 loses its taps, then gets them back
    eng = _engine(bfir, shape, h1, chunk=3)
    assert eng.run(x[:n1 * L])[0] == 0
    assert eng.set_coeff(short) == 0
    rc, y = eng.run(x[n1 * L:(n1 + n2) * L])
    assert rc == 0
    print("rel_err short", rel_err(y[settle * L:], want_s[(n1 + settle) * L:(n1 + n2) * L]))
    assert rel_err(y[settle * L:], want_s[(n1 + settle) * L:(n1 + n2) * L]) <= TOL[s]
    assert eng.set_coeff(h2) == 0
    rc, y = eng.run(x[(n1 + n2) * L:])
    assert rc == 0
    print("rel_err restored", rel_err(y[settle * L:], want[(n1 + n2 + settle) * L:]))
    assert rel_err(y[settle * L:], want[(n1 + n2 + settle) * L:]) <= TOL[s]
    # a NaN tap in the last level's part: BFIR_ERR_COEFF and the engine is uninitialised
    bad = [c.copy() for c in h2]; bad[Cn - 1][D[2] + 3] = np.inf
    assert eng.set_coeff(bad) == bfir.ERR_COEFF and not eng.is_initialized()
    assert eng.run(x[:L])[0] == bfir.ERR_STATE
    too_long = [np.zeros(eng.max_taps + 1, _real(s)) for _ in range(Cn)]
    assert eng.max_taps == D[-1] and eng.set_coeff(too_long) == bfir.ERR_ARG
    assert eng.set_coeff([np.zeros(eng.max_taps, _real(s)) for _ in range(Cn)]) == 0
    eng.close()


@pytest.mark.parametrize("shape", [FUSED, GENERAL], ids=["fused", "general"])
def test_reset_forgets_all_signal_state(orc, bfir, shape):
    s, L, blocks, ratios, Cn = shape
    _, D, r = _geo(shape)
    h, x = _make(orc, shape)
    _, x2 = _make(orc, shape, seed=1)
    fresh = _engine(bfir, shape, h)
    rc, want = fresh.run(x2)
    assert rc == 0
    fresh.close()
    eng = _engine(bfir, shape, h)
    assert eng.run(x[:(D[2] // L + r[-1] + 1) * L])[0] == 0             # stops inside a block of every level, with output queued
    eng.reset()
    assert eng.is_initialized() and all(eng.overflow(c).largest == 0.0 for c in range(Cn))
    rc, y = eng.run(x2)
    assert rc == 0 and np.array_equal(y, want)
    eng.close()


@pytest.mark.parametrize("shape", [FUSED, GENERAL], ids=["fused", "general"])
def test_nan_guard_and_recovery(orc, bfir, shape):
    s, L, blocks, ratios, Cn = shape
    _, D, _ = _geo(shape)
    h, x = _make(orc, shape)
    want, _ = _uniform(orc, shape, h, x)
    bad = x.copy()
    bad[(D[2] // L + 1) * L, 0] = np.nan                                 # data, not an address: sample 0 of a block
    eng = _engine(bfir, shape, h)
    rc, _ = eng.run(bad)
    assert rc == bfir.ERR_NONFINITE
    eng.reset()                                                          # every level forgets the NaN
    rc, y = eng.run(x)
    assert rc == 0 and rel_err(y, want) <= TOL[s]
    eng.close()


@pytest.mark.parametrize("shape", [FUSED, PARITY[3][0], GENERAL, F64_SHAPE], ids=["fused", "fused4", "general", "f64"])
def test_overflow_counts_the_sum(orc, bfir, shape):
    """Taps 0.2 at 0 and at every D_k, scale 2, constant input 0.9: level k alone gives 0.36, the sum passes full scale from
    sample D_2 on (1.08; 1.44 with a fourth level).  Counted once per sample, on the sum, as the uniform oracle counts."""
    s, L, blocks, ratios, Cn = shape
    _, D, _ = _geo(shape)
    nb = _nb(shape)
    h = np.zeros((Cn, D[-2] + 1), _real(s))
    for d in D[:-1]:
        h[:, d] = 0.2
    x = np.full((nb * L, Cn), 0.9, _real(s))
    _, ofs = _uniform(orc, shape, list(h), x, scale=2.0)
    eng = _engine(bfir, shape, list(h), chunk=3, scale=2.0)
    rc, y = eng.run(x)
    assert rc == 0
    for c in range(Cn):
        of = eng.overflow(c)
        print("overflow", shape, c, of.n_overflows, of.largest, ofs[c].n_overflows, ofs[c].largest)
        assert of.n_overflows == ofs[c].n_overflows == nb * L - D[2]
        assert abs(of.largest - ofs[c].largest) <= TOL[s] * ofs[c].largest
    assert np.abs(y[:D[2]]).max() < 1.0 and np.abs(y[D[2]:]).min() > 1.0
    eng.close()


@pytest.mark.parametrize("shape", [PARITY[2][0], (4, 128, (2, 2, 2, 2), (1, 2, 2, 2), 1), F64_SHAPE], ids=_id)
def test_partition_spectra_of_every_level(orc, bfir, shape):
    s, L, blocks, ratios, Cn = shape
    Ls, D, _ = _geo(shape)
    h, _ = _make(orc, shape, nb=1)
    eng = bfir.BrutefirLevels(L, blocks, ratios, s, Cn)
    assert eng.D == D[:-1] and eng.max_taps == D[-1]
    assert eng.set_coeff(h, scale=0.5) == 0
    for level, (Lp, Bp) in enumerate(zip(Ls, blocks)):
        ref = orc.Engine(Lp, Bp, s, Cn)
        assert ref.set_coeff([np.ascontiguousarray(c[D[level]:D[level + 1]]) for c in h], scale=0.5) == 0
        for c in range(Cn):
            for b in range(Bp):
                got = eng.coeff_block(level, c, b)
                assert got.size == 2 * Lp and rel_err(got, ref.coeff_block(c, b)) <= TOL[s]
        ref.close()
    lib = bfir.load()
    dst = np.zeros(2 * Ls[-1], _real(s))
    n = len(blocks)
    for lv, c, b in [(n, 0, 0), (-1, 0, 0), (0, Cn, 0), (0, 0, blocks[0]), (1, 0, blocks[1]), (n - 1, 0, blocks[-1]), (1, -1, 0),
                     (2, 0, -1)]:
        assert lib.bfir_engine_read_coeff_levels(eng.handle, lv, c, b, dst.ctypes.data) == bfir.ERR_ARG
    assert lib.bfir_engine_read_coeff_levels(eng.handle, 0, 0, 0, None) == bfir.ERR_ARG
    eng.close()


def test_calls_of_the_other_kinds_are_refused(orc, bfir):
    lib = bfir.load()
    shape = FUSED
    s, L, blocks, ratios, Cn = shape
    Ls, _, _ = _geo(shape)
    h, x = _make(orc, shape)
    U = bfir.ERR_UNSUPPORTED
    eng = _engine(bfir, shape, h)
    rc, before = eng.run(x[:4 * L])
    assert rc == 0
    eng.reset()
    ptrs = (C.c_void_p * 4)(*[h[c % Cn].ctypes.data for c in range(4)])
    dst = np.zeros(2 * Ls[-1], np.float32)
    assert lib.bfir_engine_set_coeff(eng.handle, ptrs, Cn, h[0].size, blocks[0], 1.0) == U
    assert lib.bfir_engine_set_coeff_at(eng.handle, 0, ptrs, Cn, h[0].size, blocks[0], 1.0) == U
    assert lib.bfir_engine_read_coeff(eng.handle, 0, 0, dst.ctypes.data) == U
    assert lib.bfir_engine_set_coeff_matrix(eng.handle, ptrs, h[0].size, blocks[0], 1.0) == U
    assert lib.bfir_engine_read_coeff_matrix(eng.handle, 0, 0, 0, dst.ctypes.data) == U
    assert lib.bfir_engine_set_coeff_fade(eng.handle, ptrs, Cn, h[0].size, blocks[0], 1.0, 3) == U
    assert lib.bfir_engine_set_coeff_matrix_fade(eng.handle, ptrs, h[0].size, blocks[0], 1.0, 3) == U
    assert lib.bfir_engine_fade_remaining(eng.handle) == U
    assert lib.bfir_engine_set_coeff_nup(eng.handle, ptrs, Cn, 100, 1.0) == U
    assert lib.bfir_engine_read_coeff_nup(eng.handle, 0, 0, 0, dst.ctypes.data) == U
    with pytest.raises(bfir.BfirError) as ex:
        eng.set_coeff_fade(h, 3)
    assert ex.value.code == U
    assert eng.is_initialized()                                          # a refused call changes nothing
    rc, after = eng.run(x[:4 * L])
    assert rc == 0 and np.array_equal(after, before)
    eng.close()
    plain = bfir.Brutefir(L, blocks[0], s, Cn)
    matrix = bfir.BrutefirMatrix(L, blocks[0], s, 2, 2)
    nup = bfir.BrutefirNup(L, blocks[0], ratios[1], blocks[1], s, Cn)
    for other in (plain, matrix, nup):
        assert lib.bfir_engine_set_coeff_levels(other.handle, ptrs, Cn, 100, 1.0) == U
        assert lib.bfir_engine_read_coeff_levels(other.handle, 0, 0, 0, dst.ctypes.data) == U
        other.close()


def test_profile_counts_every_level(orc, bfir):
    """32 blocks in launches of 4, levels of 1, 4 and 8 blocks: 8 head launches, 8 blocks of level 1 and 4 of level 2, one
    launch each because a level's blocks complete one per head launch at most; every change of the contributing levels
    (blocks 4 and 12) falls between two launches."""
    shape = FUSED
    s, L, blocks, ratios, Cn = shape
    _, D, r = _geo(shape)
    assert r == [1, 4, 8] and D[1] // L == 4 and D[2] // L == 12
    nb = 32
    h, x = _make(orc, shape, nb=nb)
    eng = _engine(bfir, shape, h, chunk=4)
    assert eng.run(x)[0] == 0                                            # sizes the work buffers
    eng.reset()
    eng.set_profiling(True)
    assert eng.run(x)[0] == 0
    prof = eng.profile()
    want = nb // 4 + nb // r[1] + nb // r[2]
    print(prof)
    assert prof["k_fwd"][1] == want and prof["k_mac"][1] == want and prof["k_inv"][1] == want
    assert prof["k_stage_in"][1] == 0 and prof["k_stage_out"][1] == 0    # fused back end
    eng.close()


# ---- the C++ mirror -------------------------------------------------------------------------------------------------
def _fnv1a(data):
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return h


def test_cpp_mirror_runs_three_levels_like_the_ctypes_engine(tmp_path, bfir):
    """tests/cpp/test_levels_mirror.cpp builds its input and filters from integer recurrences (restated here), runs a
    three-level brutefir one block per run() and prints the FNV-1a hash of its output bytes."""
    src = os.path.join(ROOT, "tests", "cpp", "test_levels_mirror.cpp")
    exe = str(tmp_path / "test_levels_mirror")
    libdir = os.path.dirname(bfir.library_path())
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", src, "-o", exe, "-L" + libdir, "-lbfir_hip",
                    "-Wl,-rpath," + libdir], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "ALL OK" in p.stdout
    L, blocks, ratios, Cn, taps, nb = 512, (4, 2, 2), (1, 4, 2), 2, 11000, 48
    i = np.arange(nb * L * Cn, dtype=np.uint64)
    x = ((((i * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(8)).astype(np.float64) / 16777216.0 - 0.5)
    x = x.astype(np.float32).reshape(nb * L, Cn)
    n = np.arange(taps, dtype=np.uint64)
    h = []
    for c in range(Cn):
        v = (((n + np.uint64(1)) * np.uint64(40503 * (c + 3))) & np.uint64(0xffff)).astype(np.float64) / 65536.0 - 0.5
        h.append((v / (64.0 * (1.0 + n.astype(np.float64) / 64.0))).astype(np.float32))
    eng = bfir.BrutefirLevels(L, blocks, ratios, 4, Cn)
    assert eng.set_coeff(h) == 0
    rc, y = eng.run(x)
    assert rc == 0
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("checksum ")]
    assert line and int(line[0].split()[1], 16) == _fnv1a(y.tobytes())
    eng.close()
