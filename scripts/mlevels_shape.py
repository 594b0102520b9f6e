"""What the multi-level matrix engine (bfir_engine_create_matrix_levels) costs, against existing code of the same work.
fp32, L = 512, 131072 taps per filter, levels (4, 3, 15) x (512, 2048, 8192), every filter present, I/O resident in HBM.

    2to2   the engine against BrutefirMatrix(512, 256, 4, 2, 2), the same convolution on uniform partitions: Gsamples/s
           (output samples) of a long run_device, and one-block run() latency as median and maximum
    2to3   the fused back end with the lone kernel: the engine's k_inv time from profile() against the summed k_inv (planar
           inverse and ring sum) and k_stage_out time of BrutefirLevels(..., channels = 3), the general back end with the
           same output count and rings
    1to2   the output-side dispatch: the same comparison against BrutefirLevels(..., channels = 1), per output channel

Each comparison has both of its engines in one process and alternates between them; the back-end comparisons repeat the
profiled run and give median and range.  Without an argument every step runs in a process of its own, under its own time limit, and the lines go to
profiles/mlevels_shape.txt with the date and the hash of csrc/; the first step that fails ends the run.
`python scripts/mlevels_shape.py STEP` runs one step."""
import hashlib, os, subprocess, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GAIN = 0.0005
S, L, TAPS, BLOCKS, RATIOS = 4, 512, 131072, (4, 3, 15), (1, 4, 4)
STEPS = {"2to2": (2, 2), "2to3": (2, 3), "1to2": (1, 2)}
NB = 131072                                                              # blocks of the throughput / profile runs


def csrc_hash():
    d = os.path.join(ROOT, "foo-dsp-bfir_amd", "csrc")
    h = hashlib.sha256()
    for name in sorted(os.listdir(d)):
        h.update(name.encode()); h.update(open(os.path.join(d, name), "rb").read())
    return h.hexdigest()[:12]


def _throughput(e, x, y, nb, n_out):
    ts = []
    for _ in range(10):
        t0 = time.perf_counter(); e.run_device(x.data_ptr(), y.data_ptr(), nb); assert e.sync() == 0
        ts.append(time.perf_counter() - t0)
    ts = np.array(ts[1:])                                                # the first repetition sizes the work buffers
    t = float(np.median(ts))
    return t, nb * L * n_out / t / 1e9, (float(ts.min()), float(ts.max()))


def _latency(e, n_in, n_out, rng):
    xb = (rng.random((L, n_in), dtype=np.float32) * 2 - 1)
    rl = 16                                                              # L_2 / L
    e.reset()
    ts = []
    for _ in range(28 * rl):
        t0 = time.perf_counter(); rc, _y = e.run(xb); ts.append(time.perf_counter() - t0)
        assert rc == 0
    ts = np.array(ts[4 * rl:]) * 1e6
    return float(np.median(ts)), float(ts.max())


REPS = 7                                                                 # profiled runs per engine, alternating between the two


def _profiled(e, x, y, nb):
    e.reset()
    e.set_profiling(True)
    e.run_device(x.data_ptr(), y.data_ptr(), nb); assert e.sync() == 0
    prof = e.profile()
    e.set_profiling(False)
    return prof


def _spread(v):
    return "median %.2f, %.2f .. %.2f over %d runs" % (float(np.median(v)), min(v), max(v), len(v))


def step(name):
    import torch
    import foo_dsp_bfir_amd as bfir
    n_in, n_out = STEPS[name]
    rng = np.random.default_rng(9)
    rows = [[(rng.standard_normal(TAPS) * GAIN).astype(np.float32) for _ in range(n_in)] for _ in range(n_out)]
    ml = bfir.BrutefirMatrixLevels(L, BLOCKS, RATIOS, S, n_in, n_out)
    assert ml.max_taps >= TAPS > ml.D[-1] and ml.set_coeff(rows) == 0
    x = torch.from_numpy((rng.random((NB * L, n_in), dtype=np.float32) * 2 - 1)).cuda()
    y = torch.empty((NB * L, n_out), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    print("%s: fp32, %d -> %d, L = %d, %d taps per filter, levels %s of %s (%d partitions per pair and sample)"
          % (name, n_in, n_out, L, TAPS, "+".join(map(str, BLOCKS)), "/".join(map(str, ml.lengths)), sum(BLOCKS)))
    if name == "2to2":
        B = -(-TAPS // L)
        uni = bfir.BrutefirMatrix(L, B, S, n_in, n_out)
        assert uni.set_coeff(rows) == 0
        res = {}
        for label, e in (("matrix-levels", ml), ("matrix B=%d" % B, uni)):
            t, rate, (lo, hi) = _throughput(e, x, y, NB, n_out)
            res[label + " y"] = y[:64 * L].double().cpu().numpy()
            med, mx = _latency(e, n_in, n_out, rng)
            res[label] = rate
            print("    %-14s %d blocks in %8.2f ms (nine runs: %.2f .. %.2f)  %7.2f Gsamples/s   one-block run(): median %.1f us, max %.1f us"
                  % (label, NB, t * 1e3, lo * 1e3, hi * 1e3, rate, med, mx))
        print("    matrix-levels / matrix = %.2f" % (res["matrix-levels"] / res["matrix B=%d" % B]))
        ref = res["matrix B=%d y" % B]
        print("    last repetition's first 64 blocks against the matrix engine: %.2e (max |difference| / max |matrix|)"
              % (np.abs(res["matrix-levels y"] - ref).max() / np.abs(ref).max()))
        uni.close()
    else:
        Cn = 3 if name == "2to3" else 1
        lv = bfir.BrutefirLevels(L, BLOCKS, RATIOS, S, Cn)
        assert lv.set_coeff([rows[0][0]] * Cn) == 0
        xl = torch.from_numpy((rng.random((NB * L, Cn), dtype=np.float32) * 2 - 1)).cuda()
        yl = torch.empty_like(xl)
        torch.cuda.synchronize()
        _throughput(ml, x, y, NB, n_out); _throughput(lv, xl, yl, NB, Cn)     # size the work buffers
        fused, general, ratio = [], [], []
        per = n_out / Cn                                                 # per output channel
        for _ in range(REPS):                                            # the two engines in turn: each ratio is of neighbours in time
            pm, pl = _profiled(ml, x, y, NB), _profiled(lv, xl, yl, NB)
            assert pm["k_stage_out"][1] == 0                             # the fused back end: no staging kernel
            fused.append(pm["k_inv"][0]); general.append(pl["k_inv"][0] + pl["k_stage_out"][0])
            ratio.append(fused[-1] / (general[-1] * per))
        print("    matrix-levels %d -> %d: k_inv ms per run of %d blocks (%d launches): %s"
              % (n_in, n_out, NB, pm["k_inv"][1], _spread(fused)))
        print("    levels, %d channel%s (general back end): k_inv + k_stage_out ms per run (%d + %d launches): %s"
              % (Cn, "s" if Cn > 1 else "", pl["k_inv"][1], pl["k_stage_out"][1], _spread(general)))
        print("    fused / general%s: %s" % ("" if per == 1 else " x %g (per output channel)" % per, _spread(ratio)))
        lv.close()
    ml.close()


if __name__ == "__main__":
    if len(sys.argv) > 1:
        if sys.argv[1] not in STEPS:
            raise SystemExit("unknown step " + sys.argv[1])
        step(sys.argv[1])
        sys.exit(0)
    out = []
    for name in STEPS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), name], capture_output=True, text=True, timeout=170)
        except subprocess.TimeoutExpired:
            print("step %s ran into its time limit; stopping" % name); break
        sys.stdout.write(p.stdout); sys.stdout.flush()
        if p.returncode != 0:
            print("step %s failed (%d); stopping\n%s" % (name, p.returncode, p.stderr[-2000:])); break
        out.append(p.stdout)
    else:
        with open(os.path.join(ROOT, "profiles", "mlevels_shape.txt"), "w") as f:
            f.write("# python scripts/mlevels_shape.py -- one MI355X, one session (%s, csrc %s), every step in a process of its own\n"
                    % (time.strftime("%Y-%m-%d"), csrc_hash()) + "".join(out))
