"""What the resampler (bfir_resampler, csrc/resample.hip) costs on one GPU: fp32, Z = 64, beta 9, cutoff 0.95, 8 channels x
131072 frames, 44100 -> 48000 and 96000 -> 44100.

For each conversion: the kernel's time (HIP events around run_device, buffers resident), the whole call from host buffers
(Resampler.run: two copies, the kernel, the wait), each as median and range over ten repetitions behind one warm-up; and a
numpy float64 evaluation of the same sums from the library's taps, timed on the same host (three repetitions).  The lines go
to profiles/resample_shape.txt (or the file given as argument) with the date and the hash of csrc/."""
import hashlib, os, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S, Z, BETA, CUTOFF, C, N_IN, REPS = 4, 64, 9.0, 0.95, 8, 131072, 10
CONVERSIONS = [(44100, 48000), (96000, 44100)]


def csrc_hash():
    d = os.path.join(ROOT, "foo-dsp-bfir_amd", "csrc")
    h = hashlib.sha256()
    for name in sorted(os.listdir(d)):
        h.update(name.encode()); h.update(open(os.path.join(d, name), "rb").read())
    return h.hexdigest()[:12]


def numpy_float64(T, x, p, q, n_out):
    """y[m] = sum_j T[phase(m)][j] x[n0(m) - K / 2 + 1 + j] in float64, 4096 output frames at a time"""
    K = T.shape[1]
    T = T.astype(np.float64)
    xp = np.concatenate([np.zeros((K, x.shape[1])), x.astype(np.float64), np.zeros((K, x.shape[1]))])
    y = np.zeros((n_out, x.shape[1]))
    for a in range(0, n_out, 4096):
        m = np.arange(a, min(n_out, a + 4096), dtype=np.int64)
        n0 = m * q // p
        idx = (n0 - K // 2 + 1 + K)[:, None] + np.arange(K)[None, :]
        y[m] = np.einsum("mk,mkc->mc", T[m * q - n0 * p], xp[idx])
    return y


def measure(bfir, torch, in_rate, out_rate):
    g = np.gcd(in_rate, out_rate)
    p, q = out_rate // g, in_rate // g
    rng = np.random.default_rng(1)
    x = (rng.random((N_IN, C), dtype=np.float32) * 2 - 1)
    r = bfir.Resampler(in_rate, out_rate, Z, BETA, CUTOFF, 1.0, S, C)
    n_out = r.out_frames(N_IN)
    K = bfir.resample_taps(in_rate, out_rate, Z, BETA, CUTOFF, 1.0, S)
    d_in = torch.from_numpy(x).cuda()
    d_out = torch.zeros((n_out, C), dtype=torch.float32, device="cuda")
    kern, call = [], []
    for rep in range(REPS + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        assert r.run_device(d_in.data_ptr(), N_IN, d_out.data_ptr(), n_out) == n_out
        e1.record(); torch.cuda.synchronize()
        t0 = time.perf_counter(); y = r.run(x); t1 = time.perf_counter()
        if rep:
            kern.append(e0.elapsed_time(e1) * 1e3); call.append((t1 - t0) * 1e6)
    assert d_out.cpu().numpy().tobytes() == y.tobytes()
    T = np.stack([bfir.resample_filter(in_rate, out_rate, ph, Z, BETA, CUTOFF, 1.0, S) for ph in range(p)])
    host = []
    for _ in range(3):
        t0 = time.perf_counter(); ref = numpy_float64(T, x, p, q, n_out); host.append(time.perf_counter() - t0)
    err = float(np.abs(y - ref).max())
    r.close()
    med = lambda v: (float(np.median(v)), float(np.min(v)), float(np.max(v)))
    return ("%d -> %d  p/q %d/%d  K %d  n_out %d  table %d KiB\n"
            "    kernel            %9.1f us  (%.1f .. %.1f)   %.2f Gsamples/s out, %.1f Gfma/s\n"
            "    run, host buffers %9.1f us  (%.1f .. %.1f)\n"
            "    numpy float64     %9.1f ms  (%.1f .. %.1f)   max |gpu - numpy| %.3g\n"
            % ((in_rate, out_rate, p, q, K, n_out, p * K * S // 1024) + med(kern) +
               (n_out * C / med(kern)[0] / 1e3, n_out * C * K / med(kern)[0] / 1e3) + med(call) +
               tuple(1e3 * v for v in med(host)) + (err,)))


def main():
    import torch
    import foo_dsp_bfir_amd as bfir
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "resample_shape.txt")
    lines = ["resample_shape  %s  csrc %s  fp32, Z %d, beta %g, cutoff %g, %d channels x %d frames, %d repetitions\n"
             % (time.strftime("%Y-%m-%d"), csrc_hash(), Z, BETA, CUTOFF, C, N_IN, REPS)]
    for conv in CONVERSIONS:
        lines.append(measure(bfir, torch, *conv))
        print(lines[-1], end="")
    with open(out, "w") as f:
        f.write("".join(lines))


if __name__ == "__main__":
    main()
