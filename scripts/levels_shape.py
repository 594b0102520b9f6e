"""What three partition lengths (bfir_engine_create_levels) buy against the best two-level engine and the uniform engine of
the same L and taps.

    f32_L512      fp32, 8 channels, L = 512, 131072 taps: levels (4, 3, 15) x (512, 2048, 8192) against two levels r = 16
    f32_L64       fp32, 2 channels, L = 64, 131072 taps: levels (8, 8, 31) x (64, 512, 4096) against two levels r = 32
    plugin_262144 the plug-in shape (fp64, L = 1024, stereo, float32 frames), 262144 taps: levels (4, 1, 31) x
                  (1024, 4096, 8192) against two levels r = 8

Per shape, the three engines in one process on one GPU, I/O resident in HBM: Gsamples/s of a long run_device, and the
latency of one-block run() calls as median and maximum; on the multi-level engine also the median of the calls that
complete a block of each level.  The two-level and the uniform engine are existing code and so the baseline.

Without an argument every step runs in a process of its own, under its own time limit, and the lines go to
profiles/levels_shape.txt; the first step that fails ends the run.  `python scripts/levels_shape.py STEP` runs one step."""
import os, subprocess, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GAIN = 0.0005
# step: (realsize, L, channels, taps, blocks, ratios, (Bh, r) of the two-level engine, frame format, blocks of the throughput run)
SHAPES = {
    "f32_L512": (4, 512, 8, 131072, (4, 3, 15), (1, 4, 4), (16, 16), 8, 16384),
    "f32_L64": (4, 64, 2, 131072, (8, 8, 31), (1, 8, 8), (32, 32), 8, 65536),
    "plugin_262144": (8, 1024, 2, 262144, (4, 1, 31), (1, 4, 2), (8, 8), 8, 32768),
}
STEPS = tuple(SHAPES)


def shape(step):
    import torch
    import foo_dsp_bfir_amd as bfir
    s, L, Cn, taps, blocks, ratios, (Bh, r), fmt, nb = SHAPES[step]
    B = -(-taps // L)
    Bt = -(-(taps - Bh * L) // (r * L))
    rng = np.random.default_rng(9)
    dt = np.float64 if s == 8 else np.float32
    h = [(rng.standard_normal(taps) * GAIN).astype(dt) for _ in range(Cn)]
    engines = {"uniform": bfir.Brutefir(L, B, s, Cn, fmt, fmt), "two-level": bfir.BrutefirNup(L, Bh, r, Bt, s, Cn, fmt, fmt),
               "levels": bfir.BrutefirLevels(L, blocks, ratios, s, Cn, fmt, fmt)}
    lv = engines["levels"]
    assert lv.max_taps >= taps > lv.D[-1], (lv.max_taps, lv.D)
    for e in engines.values():
        assert e.set_coeff(h) == 0
    x = torch.from_numpy((rng.random((nb * L, Cn), dtype=np.float32) * 2 - 1)).cuda()
    y = torch.empty_like(x)
    torch.cuda.synchronize()
    print("%s: fp%d, %d channels, L = %d, %d taps: uniform B = %d; two-level Bh = %d, r = %d, Bt = %d (%d partitions per sample); "
          "levels %s of %s (%d partitions per sample)"
          % (step, 8 * s, Cn, L, taps, B, Bh, r, Bt, Bh + Bt, "+".join(map(str, blocks)), "/".join(map(str, lv.lengths)), sum(blocks)))
    rate, outs = {}, {}
    for name, e in engines.items():
        ts = []
        for _ in range(5):
            t0 = time.perf_counter(); e.run_device(x.data_ptr(), y.data_ptr(), nb); assert e.sync() == 0
            ts.append(time.perf_counter() - t0)
            if len(ts) == 1:
                outs[name] = y[:64 * L].double().cpu().numpy()   # the first repetition starts from the engine's initial state
        t = float(np.median(ts[1:]))   # ... and sizes the work buffers
        rate[name] = nb * L * Cn / t / 1e9
        print("    %-9s %d blocks in %8.2f ms  %7.2f Gsamples/s" % (name, nb, t * 1e3, rate[name]))
    print("    levels / two-level = %.2f   levels / uniform = %.2f   two-level / uniform = %.2f"
          % (rate["levels"] / rate["two-level"], rate["levels"] / rate["uniform"], rate["two-level"] / rate["uniform"]))
    ref = np.abs(outs["uniform"]).max()
    print("    first 64 blocks against the uniform engine: two-level %.2e, levels %.2e (max |difference| / max |uniform|)"
          % (np.abs(outs["two-level"] - outs["uniform"]).max() / ref, np.abs(outs["levels"] - outs["uniform"]).max() / ref))
    xb = (rng.random((L, Cn), dtype=np.float32) * 2 - 1)
    yb = np.zeros_like(xb)
    rl = lv.lengths[-1] // L
    for name, e in engines.items():
        e.reset()
        ts = []
        for i in range(12 * rl if 12 * rl >= 400 else (400 // rl + 1) * rl):
            t0 = time.perf_counter(); rc, _ = e.run(xb, yb); ts.append(time.perf_counter() - t0)
            assert rc == 0
        ts = np.array(ts[4 * rl:]) * 1e6   # a multiple of every level's block is dropped: call i completes a block of r frames when (i + 1) % r == 0
        print("    %-9s one-block run(): median %.1f us, p90 %.1f us, max %.1f us" % (name, np.median(ts), np.percentile(ts, 90), ts.max()))
        idx = np.arange(ts.size) + 1
        if name == "two-level":
            print("              calls that complete a tail block: median %.1f us; the others: median %.1f us"
                  % (np.median(ts[idx % r == 0]), np.median(ts[idx % r != 0])))
        if name == "levels":
            rs = [Lk // L for Lk in lv.lengths[1:]]
            parts = ["level %d (every %d calls): median %.1f us" % (k + 1, rk, np.median(ts[(idx % rk == 0) & (idx % (rs[k + 1] if k + 1 < len(rs) else 1 << 30) != 0)]))
                     for k, rk in enumerate(rs)]
            print("              calls that complete a block of " + "; ".join(parts) + "; the others: median %.1f us" % np.median(ts[idx % rs[0] != 0]))
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
        with open(os.path.join(ROOT, "profiles", "levels_shape.txt"), "w") as f:
            f.write("# python scripts/levels_shape.py -- one MI355X, one session, every step in a process of its own\n" + "".join(out))
