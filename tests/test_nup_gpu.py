"""Two-level partitioned engines on the GPU (bfir_engine_create_nup / _set_coeff_nup / _read_coeff_nup).

The reference is the uniform oracle engine of the same partition length and taps, Engine(L, ceil(taps / L)), compared with
rel_err <= TOL of conftest; test_nup.test_two_levels_compose_to_the_uniform_engine pins the two-level definition to it on
the CPU.  Runs are nb >= Bh + r (Bt + 2) + 3 blocks long, so the tail's delay line and its time ring both wrap."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import TOL, rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = 8, 10


def _real(s):
    return np.float64 if s == 8 else np.float32


def _fdt(fmt):
    return np.float64 if fmt == F64 else np.float32


def _fmt(s, fmt):
    return (F64 if s == 8 else F32) if fmt is None else fmt


def _taps(L, Bh, r, Bt):
    Lt = r * L
    return Bh * L + (Bt - 1) * Lt + Lt // 3 + 1                          # ends inside the last tail partition


def _nb(Bh, r, Bt):
    return Bh + r * (Bt + 2) + 3


def _make(orc, shape, fmt=None, seed=0, nb=None):
    s, L, Bh, r, Bt, Cn = shape
    rng = np.random.default_rng(1000 + sum(shape) + seed)
    h = orc.synth_ir(rng, Cn, _taps(L, Bh, r, Bt), _real(s))
    x = orc.synth_audio(rng, (nb or _nb(Bh, r, Bt)) * L, Cn, _fdt(_fmt(s, fmt)))
    return h, x


def _uniform(orc, shape, h, x, fmt=None):
    s, L, Bh, r, Bt, Cn = shape
    ref = orc.Engine(L, -(-h[0].size // L), s, Cn, fmt, fmt)
    assert ref.set_coeff(h) == 0
    rc, y = ref.run(x)
    assert rc == 0
    ofs = [ref.overflow(c) for c in range(Cn)]
    ref.close()
    return np.asarray(y, dtype=np.float64), ofs


def _engine(bfir, shape, h, fmt=None, chunk=None):
    s, L, Bh, r, Bt, Cn = shape
    eng = bfir.BrutefirNup(L, Bh, r, Bt, s, Cn, fmt, fmt)
    if chunk is not None:
        eng.set_chunk(chunk)
    assert not eng.is_initialized()
    assert eng.set_coeff(h) == 0
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


# (s, L, Bh, r, Bt, C), frame format (None = the working precision's), back end
PARITY = [
    ((4, 16, 2, 2, 3, 1), None, "general"),          # smallest
    ((4, 256, 2, 2, 2, 8), None, "general"),         # below the fused range
    ((4, 512, 4, 4, 2, 2), None, "fused"),           # fused, smallest L
    ((4, 512, 5, 4, 3, 4), None, "fused"),           # Bh not a multiple of r
    ((4, 2048, 4, 4, 2, 2), None, "fused"),          # Lt = 8192
    ((4, 4096, 4, 4, 1, 2), None, "fused"),          # Lt = 16384, the largest fp32 tail
    ((4, 512, 4, 4, 2, 3), None, "general"),         # odd count
    ((8, 64, 4, 2, 5, 3), None, "general"),          # fp64
    ((8, 1024, 8, 8, 2, 2), F32, "general"),         # float32 frames in and out: the plug-in shape
]
FUSED, GENERAL = (4, 512, 4, 4, 2, 2), (4, 256, 4, 4, 2, 3)              # r = 4 both; the second: odd count below the fused range


@pytest.mark.parametrize("shape,fmt,back", PARITY, ids=["-".join(map(str, p[0])) for p in PARITY])
def test_parity_with_the_uniform_oracle(orc, bfir, log, shape, fmt, back):
    s, L, Bh, r, Bt, Cn = shape
    h, x = _make(orc, shape, fmt)
    want, ofs = _uniform(orc, shape, h, x, fmt)
    eng = _engine(bfir, shape, h, fmt, chunk=3)                          # 3 divides no r
    assert [ln for ln in log if "two levels" in ln and ln.endswith("back end %s." % back)], log
    rc, y = eng.run(x)
    assert rc == 0
    print("rel_err", shape, rel_err(y, want))
    assert rel_err(y, want) <= TOL[s]
    for c in range(Cn):
        o, ref = eng.overflow(c), ofs[c]
        assert o.max == ref.max == 1.0
        assert abs(o.largest - ref.largest) <= TOL[s] * max(ref.largest, 1e-30)
        assert o.n_overflows == ref.n_overflows == 0
    eng.close()


@pytest.mark.parametrize("shape", [FUSED, (8, 64, 4, 2, 5, 3)], ids=["fused", "general"])
def test_head_only_filter_is_the_plain_engine_bit_for_bit(orc, bfir, shape):
    s, L, Bh, r, Bt, Cn = shape
    _, x = _make(orc, shape)
    rng = np.random.default_rng(7)
    for taps in (Bh * L, Bh * L - 7):
        h = orc.synth_ir(rng, Cn, taps, _real(s))
        plain = bfir.Brutefir(L, Bh, s, Cn)
        assert plain.set_coeff(h) == 0
        rc0, y0 = plain.run(x)
        eng = _engine(bfir, shape, h)
        rc, y = eng.run(x)
        assert rc == rc0 == 0 and np.array_equal(y, y0)
        for c in range(Cn):
            assert eng.overflow(c).largest == plain.overflow(c).largest
        eng.close(); plain.close()


@pytest.mark.parametrize("shape", [FUSED, GENERAL], ids=["fused", "general"])
def test_output_does_not_depend_on_how_the_blocks_arrive(orc, bfir, shape):
    import torch
    s, L, Bh, r, Bt, Cn = shape
    nb = _nb(Bh, r, Bt) + 2
    h, x = _make(orc, shape, nb=nb)
    want, _ = _uniform(orc, shape, h, x)
    outs = {}
    for chunk in (1, 3, 4, 5, 64):
        eng = _engine(bfir, shape, h, chunk=chunk)
        rc, outs[chunk] = eng.run(x)
        assert rc == 0
        eng.close()
    assert rel_err(outs[64], want) <= TOL[s]
    for chunk in (1, 3, 4, 5):
        assert np.array_equal(outs[chunk], outs[64]), chunk
    # the plug-in's pattern: one run() per block (the latency path), then uneven calls of a few blocks
    for steps in ([1] * nb, [2, 1, 4, 3, 7, 1, 1, 4, 6, 2, 5, 3, 4, 1, 9]):
        eng = _engine(bfir, shape, h)
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
        assert np.array_equal(np.concatenate(parts), outs[64]), steps[:3]
        eng.close()
    # device pointers, two calls that split a tail block
    eng = _engine(bfir, shape, h, chunk=5)
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.zeros_like(d_in)
    torch.cuda.synchronize()
    cut = r + 1
    fb = Cn * x.dtype.itemsize
    eng.run_device(d_in.data_ptr(), d_out.data_ptr(), cut)
    eng.run_device(d_in.data_ptr() + cut * L * fb, d_out.data_ptr() + cut * L * fb, nb - cut)
    assert eng.sync() == 0
    assert np.array_equal(d_out.cpu().numpy(), outs[64])
    eng.close()


@pytest.mark.parametrize("shape", [FUSED, GENERAL, (8, 64, 4, 2, 5, 3)], ids=["fused", "general", "f64"])
def test_overflow_counts_the_sum(bfir, shape):
    """h = 0.75 d[0] + 0.75 d[D], constant input 0.7: each level alone stays at 0.525, the sum is 1.05 from sample D on."""
    s, L, Bh, r, Bt, Cn = shape
    D, nb = Bh * L, _nb(Bh, r, Bt)
    h = np.zeros((Cn, D + 1), _real(s))
    h[:, 0] = h[:, D] = 0.75
    x = np.full((nb * L, Cn), 0.7, _real(s))
    eng = _engine(bfir, shape, list(h), chunk=3)
    rc, y = eng.run(x)
    assert rc == 0
    for c in range(Cn):
        of = eng.overflow(c)
        print("overflow", shape, c, of.n_overflows, of.largest)
        assert of.n_overflows == nb * L - D
        assert abs(of.largest - 1.05) <= TOL[s] * 1.05
    assert np.abs(y[:D]).max() < 1.0 and np.abs(y[D:]).min() > 1.0
    eng.close()


@pytest.mark.parametrize("shape", [FUSED, GENERAL], ids=["fused", "general"])
def test_nan_guard(orc, bfir, shape):
    import torch
    s, L, Bh, r, Bt, Cn = shape
    h, x = _make(orc, shape)
    x[(Bh + 1) * L, 0] = np.nan                                          # data, not an address: sample 0 of a block
    eng = _engine(bfir, shape, h)
    rc, _ = eng.run(x)
    assert rc == bfir.ERR_NONFINITE
    eng.close()
    plain = bfir.Brutefir(L, Bh, s, Cn)                                  # as the uniform engine does
    assert plain.set_coeff([c[:Bh * L] for c in h]) == 0
    assert plain.run(x)[0] == bfir.ERR_NONFINITE
    plain.close()
    eng = _engine(bfir, shape, h)
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.zeros_like(d_in)
    torch.cuda.synchronize()
    eng.run_device(d_in.data_ptr(), d_out.data_ptr(), x.shape[0] // L)
    assert eng.sync() == bfir.ERR_NONFINITE
    assert eng.sync() == 0
    eng.close()


@pytest.mark.parametrize("shape", [FUSED, GENERAL], ids=["fused", "general"])
def test_reset_forgets_all_signal_state(orc, bfir, shape):
    s, L, Bh, r, Bt, Cn = shape
    h, x = _make(orc, shape)
    _, x2 = _make(orc, shape, seed=1)
    fresh = _engine(bfir, shape, h)
    rc, want = fresh.run(x2)
    assert rc == 0
    fresh.close()
    eng = _engine(bfir, shape, h)
    assert eng.run(x[:(Bh + r + 1) * L])[0] == 0                         # stops inside a tail block, with tail output queued
    eng.reset()
    assert eng.is_initialized() and all(eng.overflow(c).largest == 0.0 for c in range(Cn))
    rc, y = eng.run(x2)
    assert rc == 0 and np.array_equal(y, want)
    eng.close()


@pytest.mark.parametrize("shape", [FUSED, GENERAL, (8, 64, 4, 2, 5, 3)], ids=["fused", "general", "f64"])
def test_set_coeff_mid_stream(orc, bfir, shape):
    """After a second set_coeff_nup and Bh + r (Bt + 2) further blocks the output is the uniform oracle's with the new
    filters fed the whole stream; also from a head-only first set (the tail starts mid-stream) and to one (it stops)."""
    s, L, Bh, r, Bt, Cn = shape
    settle = Bh + r * (Bt + 2)
    n1 = r + 3                                                           # the change falls inside a tail block
    nb = n1 + settle + 4
    h2, x = _make(orc, shape, nb=nb)
    h1, _ = _make(orc, shape, seed=5, nb=1)
    want, _ = _uniform(orc, shape, h2, x)
    for first in (h1, [c[:Bh * L - 5] for c in h1]):
        eng = _engine(bfir, shape, first, chunk=3)
        assert eng.run(x[:n1 * L])[0] == 0
        assert eng.set_coeff(h2) == 0
        rc, y = eng.run(x[n1 * L:])
        assert rc == 0
        assert rel_err(y[settle * L:], want[(n1 + settle) * L:]) <= TOL[s]
        eng.close()
    # to a head-only set: the tail stops, and once its queued output has played the plain engine's bits come out
    short = [c[:Bh * L] for c in h2]
    eng = _engine(bfir, shape, h1, chunk=3)
    assert eng.run(x[:n1 * L])[0] == 0
    assert eng.set_coeff(short) == 0
    rc, y = eng.run(x[n1 * L:])
    assert rc == 0
    ref = orc.Engine(L, Bh, s, Cn)
    assert ref.set_coeff(short) == 0
    want_s = np.asarray(ref.run(x)[1], dtype=np.float64)
    ref.close()
    assert rel_err(y[settle * L:], want_s[(n1 + settle) * L:]) <= TOL[s]
    # a NaN tap in the tail's part: BFIR_ERR_COEFF and the engine is uninitialised
    bad = [c.copy() for c in h2]; bad[Cn - 1][Bh * L + 3] = np.inf
    assert eng.set_coeff(bad) == bfir.ERR_COEFF and not eng.is_initialized()
    assert eng.run(x[:L])[0] == bfir.ERR_STATE
    too_long = [np.zeros(Bh * L + Bt * r * L + 1, _real(s)) for _ in range(Cn)]
    assert eng.set_coeff(too_long) == bfir.ERR_ARG
    eng.close()


@pytest.mark.parametrize("shape", [(4, 512, 5, 4, 3, 2), (4, 128, 2, 2, 2, 1), (8, 1024, 4, 2, 2, 2), (8, 64, 4, 2, 5, 3)],
                         ids=lambda a: "-".join(map(str, a)))
def test_partition_spectra_of_both_levels(orc, bfir, shape):
    s, L, Bh, r, Bt, Cn = shape
    D, Lt = Bh * L, r * L
    h, _ = _make(orc, shape, nb=1)
    eng = bfir.BrutefirNup(L, Bh, r, Bt, s, Cn)
    assert eng.set_coeff(h, scale=0.5) == 0
    for level, (Lp, Bp, part) in enumerate([(L, Bh, [c[:D] for c in h]), (Lt, Bt, [c[D:] for c in h])]):
        ref = orc.Engine(Lp, Bp, s, Cn)
        assert ref.set_coeff([np.ascontiguousarray(c) for c in part], scale=0.5) == 0
        for c in range(Cn):
            for b in range(Bp):
                got = eng.coeff_block(level, c, b)
                assert got.size == 2 * Lp and rel_err(got, ref.coeff_block(c, b)) <= TOL[s]
        ref.close()
    lib = bfir.load()
    dst = np.zeros(2 * Lt, _real(s))
    for lv, c, b in [(2, 0, 0), (-1, 0, 0), (0, Cn, 0), (0, 0, Bh), (1, 0, Bt), (1, -1, 0)]:
        assert lib.bfir_engine_read_coeff_nup(eng.handle, lv, c, b, dst.ctypes.data) == bfir.ERR_ARG
    eng.close()


def test_calls_of_the_other_kinds_are_refused(orc, bfir):
    lib = bfir.load()
    shape = (4, 512, 4, 4, 2, 2)
    s, L, Bh, r, Bt, Cn = shape
    h, _ = _make(orc, shape, nb=1)
    U = bfir.ERR_UNSUPPORTED
    eng = _engine(bfir, shape, h)
    ptrs = (C.c_void_p * 4)(*[h[c % Cn].ctypes.data for c in range(4)])
    dst = np.zeros(2 * r * L, np.float32)
    assert lib.bfir_engine_set_coeff(eng.handle, ptrs, Cn, h[0].size, Bh, 1.0) == U
    assert lib.bfir_engine_set_coeff_at(eng.handle, 0, ptrs, Cn, h[0].size, Bh, 1.0) == U
    assert lib.bfir_engine_read_coeff(eng.handle, 0, 0, dst.ctypes.data) == U
    assert lib.bfir_engine_set_coeff_matrix(eng.handle, ptrs, h[0].size, Bh, 1.0) == U
    assert lib.bfir_engine_read_coeff_matrix(eng.handle, 0, 0, 0, dst.ctypes.data) == U
    assert lib.bfir_engine_set_coeff_fade(eng.handle, ptrs, Cn, h[0].size, Bh, 1.0, 3) == U
    assert lib.bfir_engine_set_coeff_matrix_fade(eng.handle, ptrs, h[0].size, Bh, 1.0, 3) == U
    assert lib.bfir_engine_fade_remaining(eng.handle) == U
    assert eng.is_initialized()                                          # a refused call changes nothing
    eng.close()
    plain = bfir.Brutefir(L, Bh, s, Cn)
    matrix = bfir.BrutefirMatrix(L, Bh, s, 2, 2)
    for other in (plain, matrix):
        assert lib.bfir_engine_set_coeff_nup(other.handle, ptrs, Cn, h[0].size, 1.0) == U
        assert lib.bfir_engine_read_coeff_nup(other.handle, 0, 0, 0, dst.ctypes.data) == U
        other.close()


def test_profile_counts_both_levels(orc, bfir):
    shape = FUSED
    s, L, Bh, r, Bt, Cn = shape
    h, x = _make(orc, shape)
    eng = _engine(bfir, shape, h, chunk=4)
    eng.set_profiling(True)
    assert eng.run(x)[0] == 0
    prof = eng.profile()
    nb = x.shape[0] // L
    head = -(-nb // 4)
    assert prof["k_fwd"][1] > head and prof["k_mac"][1] > head and prof["k_inv"][1] > head   # the tail's launches on top
    assert prof["k_stage_in"][1] == 0 and prof["k_stage_out"][1] == 0                        # fused back end
    eng.close()


# ---- the C++ mirror -------------------------------------------------------------------------------------------------
def _fnv1a(data):
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return h


def test_cpp_mirror_runs_two_levels_like_the_ctypes_engine(tmp_path, bfir):
    """tests/cpp/test_nup_mirror.cpp builds its input and filters from integer recurrences (restated here), runs a
    two-level brutefir one block per run() and prints the FNV-1a hash of its output bytes."""
    src = os.path.join(ROOT, "tests", "cpp", "test_nup_mirror.cpp")
    exe = str(tmp_path / "test_nup_mirror")
    libdir = os.path.dirname(bfir.library_path())
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", src, "-o", exe, "-L" + libdir, "-lbfir_hip",
                    "-Wl,-rpath," + libdir], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "ALL OK" in p.stdout
    L, Bh, r, Bt, Cn, taps, nb = 512, 4, 4, 2, 2, 5000, 20
    i = np.arange(nb * L * Cn, dtype=np.uint64)
    x = ((((i * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(8)).astype(np.float64) / 16777216.0 - 0.5)
    x = x.astype(np.float32).reshape(nb * L, Cn)
    n = np.arange(taps, dtype=np.uint64)
    h = []
    for c in range(Cn):
        v = (((n + np.uint64(1)) * np.uint64(40503 * (c + 3))) & np.uint64(0xffff)).astype(np.float64) / 65536.0 - 0.5
        h.append((v / (64.0 * (1.0 + n.astype(np.float64) / 64.0))).astype(np.float32))
    eng = bfir.BrutefirNup(L, Bh, r, Bt, 4, Cn)
    assert eng.set_coeff(h) == 0
    rc, y = eng.run(x)
    assert rc == 0
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("checksum ")]
    assert line and int(line[0].split()[1], 16) == _fnv1a(y.tobytes())
    eng.close()
