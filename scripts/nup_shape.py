"""What two partition lengths (bfir_engine_create_nup) buy against the uniform engine of the same L and taps.

    plugin_65536 / plugin_262144   the plug-in shape (fp64, L = 1024, stereo, float32 frames), Bh = 8, r = 8
    f32_r4 / f32_r16               fp32, 8 channels, L = 512, 131072 taps, Bh = r

Per shape, both engines in one process on one GPU, I/O resident in HBM: Gsamples/s of a long run_device, the per-kernel
event times of bfir_engine_get_profile on the engine's own schedule (fp64: one stream; fp32: three, so the spans of
neighbouring chunks overlap and do not add up to the run time), and the latency of one-block run() calls as median and
maximum -- on the two-level engine the call that completes a tail block is the spike.

Without an argument every step runs in a process of its own, under its own time limit, and the lines go to
profiles/nup_shape.txt; the first step that fails ends the run.  `python scripts/nup_shape.py STEP` runs one step."""
import os, subprocess, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GAIN = 0.0005
# step: (realsize, L, channels, taps, Bh, r, frame format, blocks of the throughput run)
SHAPES = {
    "plugin_65536": (8, 1024, 2, 65536, 8, 8, 8, 32768),
    "plugin_262144": (8, 1024, 2, 262144, 8, 8, 8, 32768),
    "f32_r4": (4, 512, 8, 131072, 4, 4, 8, 16384),
    "f32_r16": (4, 512, 8, 131072, 16, 16, 8, 16384),
}
STEPS = tuple(SHAPES)


def shape(step):
    import torch
    import foo_dsp_bfir_amd as bfir
    s, L, Cn, taps, Bh, r, fmt, nb = SHAPES[step]
    B = -(-taps // L)
    Bt = -(-(taps - Bh * L) // (r * L))
    rng = np.random.default_rng(9)
    dt = np.float64 if s == 8 else np.float32
    h = [(rng.standard_normal(taps) * GAIN).astype(dt) for _ in range(Cn)]
    engines = {"uniform": bfir.Brutefir(L, B, s, Cn, fmt, fmt), "two-level": bfir.BrutefirNup(L, Bh, r, Bt, s, Cn, fmt, fmt)}
    for e in engines.values():
        assert e.set_coeff(h) == 0
    x = torch.from_numpy((rng.random((nb * L, Cn), dtype=np.float32) * 2 - 1)).cuda()
    y = torch.empty_like(x)
    torch.cuda.synchronize()
    print("%s: fp%d, %d channels, L = %d, %d taps: uniform B = %d; two-level Bh = %d, r = %d, Bt = %d (%d partitions per sample)"
          % (step, 8 * s, Cn, L, taps, B, Bh, r, Bt, Bh + Bt))
    rate = {}
    for name, e in engines.items():
        ts = []
        for _ in range(5):
            t0 = time.perf_counter(); e.run_device(x.data_ptr(), y.data_ptr(), nb); assert e.sync() == 0
            ts.append(time.perf_counter() - t0)
        t = float(np.median(ts[1:]))   # the first repetition sizes the work buffers
        rate[name] = nb * L * Cn / t / 1e9
        print("    %-9s %d blocks in %8.2f ms  %7.2f Gsamples/s" % (name, nb, t * 1e3, rate[name]))
    print("    two-level / uniform = %.2f" % (rate["two-level"] / rate["uniform"]))
    for name, e in engines.items():
        for rep in range(2):
            e.set_profiling(rep == 1)
            e.run_device(x.data_ptr(), y.data_ptr(), nb); assert e.sync() == 0
        p = e.profile()
        e.set_profiling(False)
        print("    %-9s kernels, ms (launches): %s" % (name, "  ".join("%s %.3f (%d)" % (k, p[k][0], p[k][1]) for k in p if p[k][1])))
    xb = (rng.random((L, Cn), dtype=np.float32) * 2 - 1)
    yb = np.zeros_like(xb)
    for name, e in engines.items():
        e.reset()
        ts = []
        for i in range(100 + 40 * r):
            t0 = time.perf_counter(); rc, _ = e.run(xb, yb); ts.append(time.perf_counter() - t0)
            assert rc == 0
        ts = np.array(ts[100:]) * 1e6
        print("    %-9s one-block run(): median %.1f us, p90 %.1f us, max %.1f us" % (name, np.median(ts), np.percentile(ts, 90), ts.max()))
        if name == "two-level":
            spike = ts.reshape(-1, r)   # the engine was reset: call i completes a tail block when (i + 1) % r == 0
            print("              calls that complete a tail block: median %.1f us; the others: median %.1f us"
                  % (np.median(spike[:, (r - 100 % r - 1) % r]), np.median(np.delete(spike, (r - 100 % r - 1) % r, axis=1))))
    for e in engines.values():
        e.close()


if __name__ == "__main__":
    if len(sys.argv) > 1:
        if sys.argv[1] not in SHAPES:
            raise SystemExit("unknown step " + sys.argv[1])
        shape(sys.argv[1])
        sys.exit(0)
    out = []
    for step in STEPS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), step], capture_output=True, text=True, timeout=170)
        except subprocess.TimeoutExpired:
            print("step %s ran into its time limit; stopping" % step); break
        sys.stdout.write(p.stdout); sys.stdout.flush()
        if p.returncode != 0:
            print("step %s failed (%d); stopping\n%s" % (step, p.returncode, p.stderr[-2000:])); break
        out.append(p.stdout)
    else:
        with open(os.path.join(ROOT, "profiles", "nup_shape.txt"), "w") as f:
            f.write("# python scripts/nup_shape.py -- one MI355X, one session, every step in a process of its own\n" + "".join(out))
