"""What a crossfaded coefficient change (bfir_engine_set_coeff_fade) costs, on device buffers and on the latency path.

    latency     one run() per block at the plug-in's shape (fp64, L = 1024, B = 64, stereo FLOAT_LE) and its fp32 sibling:
                a call that is a fade block against a plain call of the same engine
    continuous  every block fades (K = the run length; head tracking): 2 -> 2 fp32 matrix, L = 1024, B = 16, and the
                8-channel diagonal engine, L = 4096, B = 32, against (a) the same engine's plain run and (b) today's
                workaround: two plain engines on the same input plus one read-read-write pass over the outputs, counted
                at the measured copy rate of profiles/r03_hbm_stream.txt
    kernels     the engine's own per-kernel event timing (BFIR_PIPE=1: one stream), k_inv_fade against k_inv_pair_ps

Without an argument every step runs in a process of its own, under its own time limit, and the lines go to
profiles/fade_shape.txt; the first step that fails ends the run.  `python scripts/fade_shape.py STEP` runs one step."""
import os, subprocess, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_RATE = 5440e9   # bytes/s read + written, "copy, slabs, 4 in flight, nt" of profiles/r03_hbm_stream.txt
GAIN = 0.002
STEPS = ("latency_f64", "latency_f32", "continuous_matrix", "continuous_diag8", "kernels_diag8", "kernels_stereo")


def latency(s):
    import foo_dsp_bfir_amd as bfir
    L, B, Cn, n = 1024, 64, 2, 300
    rng = np.random.default_rng(s)
    dt = np.float64 if s == 8 else np.float32
    h = [[(rng.standard_normal(B * L) * GAIN).astype(dt) for _ in range(Cn)] for _ in range(2)]
    e = bfir.Brutefir(L, B, s, Cn, 8, 8)
    assert e.set_coeff(h[0]) == 0
    x = (rng.random((L, Cn), dtype=np.float32) * 2 - 1)
    y = np.zeros_like(x)

    def calls(k):
        ts = []
        for _ in range(k):
            t0 = time.perf_counter(); rc, _ = e.run(x, y); ts.append(time.perf_counter() - t0)
            assert rc == 0
        return np.array(ts) * 1e6

    calls(100)
    plain = calls(n)
    assert e.set_coeff_fade(h[1], n + 20) == 0
    calls(20)
    fade = calls(n)
    assert e.fade_remaining() == 0
    print("latency fp%d L=1024 B=64 stereo: plain call %.1f us (p10 %.1f, p90 %.1f), fade-block call %.1f us (p10 %.1f, p90 %.1f), ratio %.2f"
          % (8 * s, np.median(plain), np.percentile(plain, 10), np.percentile(plain, 90), np.median(fade),
             np.percentile(fade, 10), np.percentile(fade, 90), np.median(fade) / np.median(plain)))
    e.close()


def _timed(run, reps=5):
    ts = []
    for _ in range(reps):
        ts.append(run())
    return float(np.median(ts[1:]))   # the first repetition sizes the work buffers


def continuous(matrix):
    import torch
    import foo_dsp_bfir_amd as bfir
    L, B, s, n_in, n_out, nb = (1024, 16, 4, 2, 2, 8192) if matrix else (4096, 32, 4, 8, 8, 2048)
    rng = np.random.default_rng(3)
    taps = lambda: (rng.standard_normal(B * L) * GAIN).astype(np.float32)

    def make():
        if matrix:
            sets = [[[taps() for _ in range(n_in)] for _ in range(n_out)] for _ in range(2)]
            return bfir.BrutefirMatrix(L, B, s, n_in, n_out, 8, 8), sets
        return bfir.Brutefir(L, B, s, n_in, 8, 8), [[taps() for _ in range(n_in)] for _ in range(2)]

    e, sets = make()
    e2, _ = make()
    assert e.set_coeff(sets[0]) == 0 and e2.set_coeff(sets[1]) == 0
    x = torch.from_numpy((rng.random((nb * L, n_in), dtype=np.float32) * 2 - 1)).cuda()
    y = torch.empty((nb * L, n_out), dtype=torch.float32, device="cuda")
    y2 = torch.empty_like(y)
    torch.cuda.synchronize()

    def plain():
        t0 = time.perf_counter(); e.run_device(x.data_ptr(), y.data_ptr(), nb); assert e.sync() == 0
        return time.perf_counter() - t0

    def two():
        t0 = time.perf_counter()
        e.run_device(x.data_ptr(), y.data_ptr(), nb); e2.run_device(x.data_ptr(), y2.data_ptr(), nb)
        assert e.sync() == 0 and e2.sync() == 0
        return time.perf_counter() - t0

    which = [1]

    def fade():
        assert e.set_coeff_fade(sets[which[0]], nb) == 0   # loading the set is not timed (as set_coeff is not in (b))
        which[0] ^= 1
        t0 = time.perf_counter(); e.run_device(x.data_ptr(), y.data_ptr(), nb); assert e.sync() == 0
        assert e.fade_remaining() == 0
        return time.perf_counter() - t0

    t_plain, t_two, t_fade = _timed(plain), _timed(two), _timed(fade)
    t_blend = 3.0 * nb * L * n_out * 4 / COPY_RATE
    name = "2->2 fp32 matrix L=1024 B=16" if matrix else "8-channel fp32 diagonal L=4096 B=32"
    fr = lambda t: nb * L / t / 1e6
    print("continuous %s, %d blocks, every block fades:" % (name, nb))
    print("    (a) plain run                         %8.2f ms  %8.1f Mframes/s" % (t_plain * 1e3, fr(t_plain)))
    print("        fade (K = %d)                   %8.2f ms  %8.1f Mframes/s  %.2f x (a)" % (nb, t_fade * 1e3, fr(t_fade), t_fade / t_plain))
    print("    (b) two plain engines %.2f ms + blend pass at the copy rate %.2f ms = %8.2f ms  %8.1f Mframes/s; fade / (b) = %.2f"
          % (t_two * 1e3, t_blend * 1e3, (t_two + t_blend) * 1e3, fr(t_two + t_blend), t_fade / (t_two + t_blend)))
    e.close(); e2.close()


def kernels(wide):
    import torch
    import foo_dsp_bfir_amd as bfir
    L, B, Cn, nb = (4096, 32, 8, 2048) if wide else (1024, 16, 2, 8192)
    rng = np.random.default_rng(4)
    h = [[(rng.standard_normal(B * L) * GAIN).astype(np.float32) for _ in range(Cn)] for _ in range(2)]
    e = bfir.Brutefir(L, B, 4, Cn, 8, 8)
    assert e.set_coeff(h[0]) == 0
    x = torch.from_numpy((rng.random((nb * L, Cn), dtype=np.float32) * 2 - 1)).cuda()
    y = torch.empty_like(x)
    torch.cuda.synchronize()
    rows = {}
    for name in ("plain", "fade"):
        for rep in range(3):
            if name == "fade":
                assert e.set_coeff_fade(h[(rep + 1) & 1], nb) == 0
            e.set_profiling(rep == 2)
            e.run_device(x.data_ptr(), y.data_ptr(), nb); assert e.sync() == 0
        rows[name] = e.profile()
        e.set_profiling(False)
    print("kernels fp32 %d channels L=%d B=%d, %d blocks per launch, one stream:" % (Cn, L, B, nb))
    for k in ("k_fwd", "k_mac", "k_inv"):
        p, f = rows["plain"][k][0], rows["fade"][k][0]
        print("    %-6s plain %8.3f ms   fade %8.3f ms   x %.2f%s" % (k, p, f, f / p,
              "   (k_inv_pair_ps against k_inv_fade, per block %.3f / %.3f us)" % (p * 1e3 / nb, f * 1e3 / nb) if k == "k_inv" else
              "   (the MAC twice)" if k == "k_mac" else ""))
    e.close()


def run_step(step):
    if step == "latency_f64": latency(8)
    elif step == "latency_f32": latency(4)
    elif step == "continuous_matrix": continuous(True)
    elif step == "continuous_diag8": continuous(False)
    elif step == "kernels_diag8": kernels(True)
    elif step == "kernels_stereo": kernels(False)
    else: raise SystemExit("unknown step " + step)


if __name__ == "__main__":
    if len(sys.argv) > 1:
        run_step(sys.argv[1])
        sys.exit(0)
    out = []
    for step in STEPS:
        env = dict(os.environ)
        if step.startswith("kernels"):
            env["BFIR_PIPE"] = "1"
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), step], capture_output=True, text=True, timeout=150, env=env)
        except subprocess.TimeoutExpired:
            print("step %s ran into its time limit; stopping" % step); break
        sys.stdout.write(p.stdout); sys.stdout.flush()
        if p.returncode != 0:
            print("step %s failed (%d); stopping\n%s" % (step, p.returncode, p.stderr[-2000:])); break
        out.append(p.stdout)
    else:
        with open(os.path.join(ROOT, "profiles", "fade_shape.txt"), "w") as f:
            f.write("# python scripts/fade_shape.py -- one MI355X, one session, every step in a process of its own\n" + "".join(out))
