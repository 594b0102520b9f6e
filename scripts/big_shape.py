"""What long partitions (bfir_engine_create_big) cost against the uniform engine on the same impulse response.

    8 channels, 1048576 taps, frames in the working precision, I/O resident in HBM (run_device)
    fp32   uniform 16384 x 64      big 32768 x 32, 65536 x 16, 131072 x 8, 1048576 x 1
    fp64   uniform 8192 x 128      big 16384 x 64, 65536 x 16

Per engine: Gsamples/s of run_device (windows of eight calls over 2^24 frames, fp64 2^23; median of four after the one that sizes the work buffers) and the
per-kernel event times of bfir_engine_get_profile on the engine's own schedule (fp32: three streams, so the spans of
neighbouring chunks overlap and do not add up to the run time; k_fwd and k_inv of a big engine are two launches each).
The last line of a precision gives every big engine's rate over the uniform engine's of the same session.

Without an argument every step runs in a process of its own, under its own time limit, and the lines go to
profiles/big_shape.txt; the first step that fails ends the run.  `python scripts/big_shape.py STEP` runs one step."""
import os, re, subprocess, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GAIN = 0.0005
CHANNELS, TAPS = 8, 1048576
FRAMES = {4: 1 << 24, 8: 1 << 23}          # per channel and call
CALLS = 8                                  # calls per timed window, one synchronisation at its end
# step: (realsize, kind, L)
SHAPES = {
    "f32_uniform_16384": (4, "uniform", 16384),
    "f32_big_32768": (4, "big", 32768),
    "f32_big_65536": (4, "big", 65536),
    "f32_big_131072": (4, "big", 131072),
    "f32_big_1048576": (4, "big", 1048576),
    "f64_uniform_8192": (8, "uniform", 8192),
    "f64_big_16384": (8, "big", 16384),
    "f64_big_65536": (8, "big", 65536),
}
STEPS = tuple(SHAPES)


def shape(step):
    import torch
    import foo_dsp_bfir_amd as bfir
    s, kind, L = SHAPES[step]
    B, nb = TAPS // L, FRAMES[s] // L
    rng = np.random.default_rng(9)
    dt = np.float64 if s == 8 else np.float32
    h = [(rng.standard_normal(TAPS) * GAIN).astype(dt) for _ in range(CHANNELS)]
    e = (bfir.BrutefirBig if kind == "big" else bfir.Brutefir)(L, B, s, CHANNELS)
    assert e.set_coeff(h) == 0
    x = torch.from_numpy((rng.random((nb * L, CHANNELS), dtype=np.float32) * 2 - 1).astype(dt)).cuda()
    y = torch.empty_like(x)
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            e.run_device(x.data_ptr(), y.data_ptr(), nb)
        assert e.sync() == 0
        ts.append((time.perf_counter() - t0) / CALLS)
    t = float(np.median(ts[1:]))   # the first repetition sizes the work buffers
    for rep in range(2):
        e.set_profiling(rep == 1)
        e.run_device(x.data_ptr(), y.data_ptr(), nb); assert e.sync() == 0
    p = e.profile()
    e.set_profiling(False)
    print("%-18s fp%d %-7s %7d x %-3d %5d blocks in %8.2f ms  %7.2f Gsamples/s   kernels, ms (launches): %s"
          % (step, 8 * s, kind, L, B, nb, t * 1e3, nb * L * CHANNELS / t / 1e9,
             "  ".join("%s %.3f (%d)" % (k, p[k][0], p[k][1]) for k in p if p[k][1])))
    e.close()


if __name__ == "__main__":
    if len(sys.argv) > 1:
        if sys.argv[1] not in SHAPES:
            raise SystemExit("unknown step " + sys.argv[1])
        shape(sys.argv[1])
        sys.exit(0)
    out, rate = [], {}
    for step in STEPS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), step], capture_output=True, text=True, timeout=170)
        except subprocess.TimeoutExpired:
            print("step %s ran into its time limit; stopping" % step); break
        sys.stdout.write(p.stdout); sys.stdout.flush()
        if p.returncode != 0:
            print("step %s failed (%d); stopping\n%s" % (step, p.returncode, p.stderr[-2000:])); break
        out.append(p.stdout)
        m = re.search(r"([\d.]+) Gsamples/s", p.stdout)
        rate[step] = float(m.group(1))
        if step in ("f32_big_1048576", "f64_big_65536"):   # the last of a precision: the ratios to its uniform engine
            pre = step[:3]
            base = [k for k in rate if k.startswith(pre + "_uniform")][0]
            line = "%s big / uniform (%s):  %s\n" % (pre, base, "  ".join(
                "%s %.2f" % (k.split("_")[-1], rate[k] / rate[base]) for k in rate if k.startswith(pre + "_big")))
            sys.stdout.write(line); out.append(line)
    else:
        with open(os.path.join(ROOT, "profiles", "big_shape.txt"), "w") as f:
            f.write("# python scripts/big_shape.py -- one MI355X, one session, every step in a process of its own\n" + "".join(out))
