"""The resampler on the device: every cell of tests/resample_cells.py through k_resample, every sample held to
    (K + 2) u_R sum |T_j| |x_j| + u_F |ref|
around the long-double (where numpy has it, else float64) direct form of the library's own rounded taps; the impulse, 64-bit,
equal-rate, unaligned and max_out cells; the file mirror end to end in Python and in C++.  One process has the GPU open."""
import os
import subprocess

import numpy as np
import pytest

import resample_cells as RC
from conftest import TOL, rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}          # instance -> (worst error / bound, cell id)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for inst, (v, cid) in sorted(WORST.items()):
        print("resample: worst error / bound, k_resample<%s, %s>: %.3g at %s" % (inst[0], inst[1], v, cid))


def _resampler(bfir, cell):
    return bfir.Resampler(cell["in_rate"], cell["out_rate"], cell["Z"], cell["beta"], cell["cutoff"], cell["gain"], cell["s"], cell["C"])


def _hold(bfir, cell, x, y, frames, channels=None):
    """y[frames] against the bound; notes the worst error / bound of the cell's instance"""
    T = RC.table(bfir, cell)
    ref, amp = RC.reference(T, x, frames, cell["p"], cell["q"], cell["Wc"])
    bound = RC.bound(cell["s"], cell["K"], ref, amp)
    err = np.abs(y[frames].astype(RC.LD) - ref).astype(np.float64)
    if channels is not None:
        err, bound, ref = err[:, channels], bound[:, channels], ref[:, channels]
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print("%s: worst error / bound %.3g" % (cell["id"], ratio))
    if ratio >= WORST.get(cell["instance"], (-1.0, ""))[0]:
        WORST[cell["instance"]] = (ratio, cell["id"])
    assert np.all(err <= bound), np.argwhere(err > bound)[:4]
    assert np.abs(ref).max() > 0.01
    return T


def _run_device(r, x, n_frames, off_in=0, off_out=0, max_out=None):
    """run_device with the caller's buffers off_in / off_out bytes past a 16-byte boundary: (frames written, their bytes, the 64
    bytes and more on either side of them, which nothing may write: 0xA5 before the call)"""
    import torch
    xb = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
    frame = x.shape[1] * x.dtype.itemsize
    d_in = torch.zeros(xb.size + 64, dtype=torch.uint8, device="cuda")
    d_out = torch.full((n_frames * frame + 128,), 0xA5, dtype=torch.uint8, device="cuda")
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    d_in[32 + off_in:32 + off_in + xb.size] = torch.from_numpy(xb).cuda()
    torch.cuda.synchronize()
    got = r.run_device(d_in.data_ptr() + 32 + off_in, x.shape[0], d_out.data_ptr() + 64 + off_out, n_frames if max_out is None else max_out)
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    a, b = 64 + off_out, 64 + off_out + got * frame
    return got, raw[a:b].tobytes(), raw[:a].tobytes() + raw[b:].tobytes()


# ---- a, b, c, d, h: the filtered cells --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", RC.CELLS, ids=[c["id"] for c in RC.CELLS])
def test_every_sample_of_every_cell_is_within_the_bound(bfir, cell):
    r = _resampler(bfir, cell)
    assert r.out_frames(cell["n_in"]) == cell["n_out"]
    x = RC.audio(cell)
    y = r.run(x)
    assert y.shape == (cell["n_out"], cell["C"]) and y.dtype == x.dtype
    _hold(bfir, cell, x, y, np.arange(cell["n_out"], dtype=np.int64))
    if "offset" in cell:          # h: both of the caller's pointers off a 16-byte boundary -- the same bytes, nothing beside them
        got, data, guard = _run_device(r, x, cell["n_out"], cell["offset"], cell["offset"])
        assert got == cell["n_out"] and data == y.tobytes() and set(guard) == {0xA5}
    r.close()


# ---- e: an impulse reads the table out --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", RC.IMPULSE_CELLS, ids=[c["id"] for c in RC.IMPULSE_CELLS])
def test_an_impulse_gives_the_table_entries_bit_for_bit(bfir, cell):
    k, Wc, K, p, q = cell["k"], cell["Wc"], cell["K"], cell["p"], cell["q"]
    x = (RC.audio(cell) / 8).astype(RC.DTYPE[cell["s"]])          # noise at 1/8 amplitude beside the impulse channel
    x[:, 1] = 0
    x[k, 1] = 1
    r = _resampler(bfir, cell)
    y = r.run(x)
    frames = np.arange(cell["n_out"], dtype=np.int64)
    T = _hold(bfir, cell, x, y, frames, channels=[0, 2])
    n0, phase = RC.position(frames, p, q)
    j = k - n0 + Wc - 1
    want = np.where((j >= 0) & (j < K), T[phase, np.clip(j, 0, K - 1)], 0).astype(x.dtype)
    assert np.count_nonzero(want) > K // 2 * p // q
    assert y[:, 1].tobytes() == want.tobytes()
    x[:, 2] = 0                                                   # an all-zero channel: exactly zero, the others as before
    z = r.run(x)
    assert not z[:, 2].any() and z[:, :2].tobytes() == np.ascontiguousarray(y[:, :2]).tobytes() and y[:, 2].any()
    r.close()


# ---- f: positions past 2^32 -------------------------------------------------------------------------------------------------
def test_positions_past_2_to_the_32(bfir):
    cell = RC.BIG_CELL
    assert (cell["n_out"] - 1) * cell["q"] >= 1 << 32
    r = _resampler(bfir, cell)
    x = RC.audio(cell)
    y = r.run(x)
    assert y.shape == (cell["n_out"], 1)
    rng = np.random.default_rng(7)
    frames = np.unique(np.concatenate([rng.integers(0, cell["n_out"], 2000), np.arange(cell["n_out"] - 2 * cell["tile"], cell["n_out"])]))
    assert frames[-1] * cell["q"] >= 1 << 32
    _hold(bfir, cell, x, y, frames)
    # the arithmetic of the frame count, further out than any buffer here goes
    for n_in in (0, 1, 319, 320, 321, (1 << 33) + 7, (1 << 40) + 1):
        assert r.out_frames(n_in) == RC.n_out(n_in, cell["p"], cell["q"])
    r.close()


# ---- g: equal rates copy the bytes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", (4, 8))
def test_equal_rates_copy_the_bytes_nans_included(bfir, s):
    rng = np.random.default_rng(9)
    raw = rng.integers(0, 256, (1000, 3 * s), dtype=np.uint8)
    raw[5, :s] = np.frombuffer(np.array([np.nan], RC.DTYPE[s]).tobytes(), np.uint8)
    x = raw.view(RC.DTYPE[s])
    assert x.shape == (1000, 3) and np.isnan(x).any()
    r = bfir.Resampler(96000, 96000, 1, 0.0, 0.5, -3.0, s, 3)
    assert r.out_frames(1000) == 1000
    assert r.run(x).tobytes() == x.tobytes()
    got, data, guard = _run_device(r, x, 1000, s, s)
    assert got == 1000 and data == x.tobytes() and set(guard) == {0xA5}
    got, data, guard = _run_device(r, x, 1000, max_out=10)
    assert got == 10 and data == x[:10].tobytes() and set(guard) == {0xA5}
    r.close()


# ---- i: host buffers and device buffers; max_out ----------------------------------------------------------------------------
@pytest.mark.parametrize("s", (4, 8))
def test_run_equals_run_device_and_max_out_is_kept(bfir, s):
    cell = [c for c in RC.CELLS if c["id"] == "b-up-three-tiles-minus-1-s%d" % s][0]
    r = _resampler(bfir, cell)
    x = RC.audio(cell)
    n = cell["n_out"]
    y = r.run(x)
    got, data, guard = _run_device(r, x, n)
    assert got == n and data == y.tobytes() and set(guard) == {0xA5}
    for max_out in (n + 5, n - 1, cell["tile"] + 3, cell["tile"], 1, 0):
        want = min(n, max_out)
        got, data, guard = _run_device(r, x, n, max_out=max_out)
        assert got == want and data == y[:want].tobytes() and set(guard) == {0xA5}, max_out
        out = np.full((n + 4, cell["C"]), 7, x.dtype)
        assert r.run(x, max_out=max_out, out=out) is out
        assert out[:want].tobytes() == y[:want].tobytes() and np.all(out[want:] == 7)
    assert r.run(x[:0]).shape == (0, cell["C"])
    r.close()


# ---- end to end: file -> cache file -> engine -----------------------------------------------------------------------------------
def _fnv1a(data):
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return h


def test_file_to_engine_end_to_end(bfir, orc, tmp_path):
    """A 2-channel 44100 Hz float WAV, 3000 frames of decaying noise -> resample_snd_file to 48000 -> set_coeff(filename) on a
    2-channel L = 256 engine -> 8 blocks of noise, against the same engine given the float64 resampling of the file through
    the array set_coeff.  The cached WAV is the kernel's output bit for bit."""
    from foo_dsp_bfir_amd import wavio
    B = bfir.buffer
    rng = np.random.default_rng(21)
    n, L, s = 3000, 256, 4
    ir = (rng.standard_normal((n, 2)) * np.exp(-np.arange(n) / 500.0)[:, None] * 0.05).astype(np.float32)
    f = str(tmp_path / "room.wav")
    wavio.write_wav_float(f, ir, 44100)
    eng = bfir.Brutefir(L, 13, s, 2, sampling_rate=48000)
    assert eng.set_coeff(f, 13, 1.0) == -1 and not eng.is_initialized()                     # 44100 on a 48000 stream
    assert not B.check_snd_file(f, 2, 48000)
    cached = B.resample_snd_file(f, 2, 48000, str(tmp_path))
    assert cached == str(tmp_path / B.cache_name(f, 2, 48000)) and B.check_snd_file(cached, 2, 48000)
    cell = dict(in_rate=44100, out_rate=48000, Z=64, beta=9.0, cutoff=0.95, gain=1.0, s=4)
    p, q, _, _, Wc, K = RC.geometry(44100, 48000, 64, 0.95)
    n_out = RC.n_out(n, p, q)
    assert B.get_snd_file_params(cached) == (2, n_out, 48000) and n_out == 3266
    r = bfir.Resampler(44100, 48000, realsize=4, channels=2)
    assert wavio.read_wav(cached)[0].tobytes() == r.run(ir).tobytes()                         # the kernel's output, bit for bit
    r.close()
    stamp = os.stat(cached).st_mtime_ns
    assert B.resample_snd_file(f, 2, 48000, str(tmp_path)) == cached and os.stat(cached).st_mtime_ns == stamp
    assert eng.set_coeff(cached, 13, 1.0) == 2 and eng.is_initialized()
    # three channels in the file, two asked for: the third is dropped
    f3 = str(tmp_path / "room3.wav")
    wavio.write_wav_float(f3, np.concatenate([ir, ir[:, :1] * 0 + 1], axis=1), 44100)
    c3 = B.resample_snd_file(f3, 2, 48000, str(tmp_path))
    assert c3 and c3 != cached and wavio.read_wav(c3)[0].tobytes() == wavio.read_wav(cached)[0].tobytes()
    # the float64 resampling of the file: the direct form of the library's taps
    ref, amp = RC.reference(RC.table(bfir, cell), ir, np.arange(n_out, dtype=np.int64), p, q, Wc)
    got = wavio.read_wav(cached)[0]
    err = np.abs(got.astype(RC.LD) - ref).astype(np.float64)
    bound = RC.bound(4, K, ref, amp)
    print("end to end: cached taps, worst error / bound %.3g" % float((err / np.maximum(bound, 1e-300)).max()))
    assert np.all(err <= bound)
    twin = bfir.Brutefir(L, 13, s, 2, sampling_rate=48000)
    h64 = ref.astype(np.float64)
    assert twin.set_coeff([h64[:, 0], h64[:, 1]]) == 0
    x = orc.synth_audio(rng, 8 * L, 2, np.float32)
    (rc, y), (rc2, want) = eng.run(x), twin.run(x)
    e = rel_err(y, want)
    print("end to end: rel_err %.3g (tol %.3g)" % (e, TOL[s]))
    assert rc == rc2 == 0 and e <= TOL[s] and np.any(y)
    # at most coeff_blocks * L frames of the file are used
    assert eng.set_coeff(cached, 2, 1.0) == 2 and twin.set_coeff([h64[:2 * L, 0], h64[:2 * L, 1]], coeff_blocks=2) == 0
    assert rel_err(eng.run(x)[1], twin.run(x)[1]) <= TOL[s]
    eng.close(); twin.close()


def test_cpp_mirror_resamples_and_loads_like_the_python_mirror(bfir, tmp_path):
    """tests/cpp/test_buffer_mirror.cpp writes a 44100 Hz WAV from an integer recurrence, takes it through buffer::check_snd_file
    -> resample_snd_file -> brutefir::set_coeff(filename) as the plug-in does (foo_dsp_bfir.cpp:181-233), runs 8 blocks and
    prints the FNV-1a hash of its output bytes; the Python mirror does the same with the file it wrote."""
    src = os.path.join(ROOT, "tests", "cpp", "test_buffer_mirror.cpp")
    exe = str(tmp_path / "test_buffer_mirror")
    libdir = os.path.dirname(bfir.library_path())
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", src, "-o", exe, "-L" + libdir, "-lbfir_hip",
                    "-Wl,-rpath," + libdir], check=True)
    (tmp_path / "cpp").mkdir()
    (tmp_path / "py").mkdir()
    p = subprocess.run([exe, str(tmp_path / "cpp")], capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "ALL OK" in p.stdout
    L, B, Cn, nb = 256, 6, 2, 8
    f = str(tmp_path / "cpp" / "impulse.wav")
    cached = bfir.buffer.resample_snd_file(f, Cn, 48000, str(tmp_path / "py"))
    assert cached
    cpp_cached = [ln.split(None, 1)[1] for ln in p.stdout.splitlines() if ln.startswith("cached ")][0]
    assert os.path.basename(cpp_cached) == os.path.basename(cached)
    assert open(cpp_cached, "rb").read() == open(cached, "rb").read()
    eng = bfir.Brutefir(L, B, 4, Cn, sampling_rate=48000)
    assert eng.set_coeff(cached, B, 0.5) == Cn
    i = np.arange(nb * L * Cn, dtype=np.uint64)
    x = ((((i * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(8)).astype(np.float64) / 16777216.0 - 0.5)
    x = x.astype(np.float32).reshape(nb * L, Cn)
    ys = [eng.run(x[t * L:(t + 1) * L]) for t in range(nb)]
    assert all(rc == 0 for rc, _ in ys)
    y = np.concatenate([b for _, b in ys])
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("checksum ")]
    assert line and int(line[0].split()[1], 16) == _fnv1a(y.tobytes())
    eng.close()
