"""What a crossfaded coefficient change costs on a multi-level matrix engine (bfir_engine_set_coeff_matrix_levels_fade), at
the shape scripts/mlevels_shape.py measures: fp32, 2 -> 2 and 2 -> 3, L = 512, 131072 taps per filter, levels (4, 3, 15) x
(512, 2048, 8192), frames resident in HBM.

    ab       (a) the plain run (no fade) of this build against another build of the library (BFIR_PARENT_LIB=<the parent
             commit's libbfir_hip.so>, loaded through BFIR_LIB_OVERRIDE): the two builds alternate, one process each, REPS
             times, the order within a pair alternating too; the feature adds no memory and no work outside a fade, so the comparison is "equal within the spread of
             the parent's own repeated runs", and that spread is printed
    pairs    (b) every block fading, BFIR_MFADE_DUO=1 (one k_mac_duo launch) against =0 (two k_mac_matrix launches), in
             paired alternating processes: the MAC profile span (BFIR_K_MAC) per chunk and the wall time of a one-block
             fading run().  k_mac_duo is the default only if it is lower on both quantities in every paired run
    uniform  (c) the same fade on BrutefirMatrix(512, 256, ...), the workaround without this feature

Without an argument every step runs in a process of its own, under its own time limit, and the lines go to
profiles/mlevels_fade_shape.txt with the date and the hash of csrc/; the first step that fails ends the run.
`python scripts/mlevels_fade_shape.py STEP` runs one step; `ab` is skipped without BFIR_PARENT_LIB."""
import hashlib, os, subprocess, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GAIN = 0.0005
S, L, TAPS, BLOCKS, RATIOS = 4, 512, 131072, (4, 3, 15), (1, 4, 4)
SHAPES = ((2, 2), (2, 3))
NB = 16384                                                               # blocks per timed run; K = NB: every block fades
REPS = 4
STEPS = ("ab", "pairs", "uniform")
NEW_CALL = "bfir_engine_set_coeff_matrix_levels_fade"


def csrc_hash():
    d = os.path.join(ROOT, "foo-dsp-bfir_amd", "csrc")
    h = hashlib.sha256()
    for name in sorted(os.listdir(d)):
        h.update(name.encode()); h.update(open(os.path.join(d, name), "rb").read())
    return h.hexdigest()[:12]


def _setup(n_in, n_out):
    import torch
    import foo_dsp_bfir_amd as bfir
    from foo_dsp_bfir_amd import _lib
    if os.environ.get("BFIR_LIB_OVERRIDE"):                              # the parent's build lacks the new call
        _lib.SIGNATURES.pop(NEW_CALL, None)
    rng = np.random.default_rng(9)
    sets = [[[(rng.standard_normal(TAPS) * GAIN).astype(np.float32) for _ in range(n_in)] for _ in range(n_out)] for _ in range(2)]
    x = torch.from_numpy((rng.random((NB * L, n_in), dtype=np.float32) * 2 - 1)).cuda()
    y = torch.empty((NB * L, n_out), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return bfir, sets, x, y


def _timed(e, x, y, before=None):
    if before:
        before()
    t0 = time.perf_counter(); e.run_device(x.data_ptr(), y.data_ptr(), NB); assert e.sync() == 0
    return time.perf_counter() - t0


def one():
    """(a) of whichever build BFIR_LIB_OVERRIDE names, 2 -> 2: the median rate and the repetitions' rates, Moutput-samples/s."""
    bfir, sets, x, y = _setup(2, 2)
    ml = bfir.BrutefirMatrixLevels(L, BLOCKS, RATIOS, S, 2, 2)
    assert ml.set_coeff(sets[0]) == 0
    ts = [_timed(ml, x, y) for _ in range(8)][1:]                        # the first repetition sizes the work buffers
    print("%.1f %s" % (NB * L * 2 / float(np.median(ts)) / 1e6, " ".join("%.1f" % (NB * L * 2 / t / 1e6) for t in ts)))
    ml.close()


def ab():
    other = os.environ.get("BFIR_PARENT_LIB")
    if not other or not os.path.exists(other):
        print("ab: BFIR_PARENT_LIB is not set: skipped")
        return
    res = {"parent": [], "this": []}
    for rep in range(REPS):
        for name in (("parent", "this") if rep % 2 == 0 else ("this", "parent")):   # whichever runs second meets a warmer GPU
            env = dict(os.environ)
            env.pop("BFIR_LIB_OVERRIDE", None)
            if name == "parent":
                env["BFIR_LIB_OVERRIDE"] = other
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "one"], capture_output=True, text=True, timeout=120, env=env)
            if p.returncode != 0:
                raise SystemExit("ab: %s failed\n%s" % (name, p.stderr[-1500:]))
            res[name].append(float(p.stdout.split()[0]))
            print("    rep %d %-6s %s" % (rep, name, p.stdout.strip()))
            print("ab: rep %d %s done" % (rep, name), file=sys.stderr, flush=True)
    for name, v in res.items():
        print("    (a) %-6s 2 -> 2, no fade: median %.1f Msamples/s, spread of its %d runs %.1f .. %.1f (%.2f %%)"
              % (name, np.median(v), len(v), min(v), max(v), 100 * (max(v) - min(v)) / np.median(v)))
    d = 100 * (np.median(res["this"]) - np.median(res["parent"])) / np.median(res["parent"])
    sp = 100 * (max(res["parent"]) - min(res["parent"])) / np.median(res["parent"])
    print("    this / parent - 1 = %+.2f %%; the parent's own spread is %.2f %%: %s" % (d, sp, "equal" if abs(d) <= sp else "DIFFERENT"))


def fading(n_in, n_out):
    """One engine under the BFIR_MFADE_DUO of the environment, every block fading: `span_us launches rate one_block_us`."""
    bfir, sets, x, y = _setup(n_in, n_out)
    ml = bfir.BrutefirMatrixLevels(L, BLOCKS, RATIOS, S, n_in, n_out)
    assert ml.set_coeff(sets[0]) == 0
    _timed(ml, x, y)                                                     # sizes the work buffers, fills every delay line
    spans, rates = [], []
    for i in range(4):
        _timed(ml, x, y, lambda: ml.fade_to_rows(sets[1 - i % 2], NB) == 0 or sys.exit("fade_to_rows"))   # the first fade allocates
        assert ml.fade_remaining() == 0
        ml.set_profiling(True)
        t = _timed(ml, x, y, lambda: ml.fade_to_rows(sets[i % 2], NB) == 0 or sys.exit("fade_to_rows"))
        ms, n = ml.profile()["k_mac"]
        ml.set_profiling(False)
        spans.append(1e3 * ms / n); launches = n
        rates.append(NB * L * n_out / t / 1e6)
    # the latency path: one block per run(), all of them inside one long fade, past the calls that fill the levels
    xb = (np.random.default_rng(3).random((L, n_in), dtype=np.float32) * 2 - 1)
    rl = 16
    assert ml.fade_to_rows(sets[1], 32768) == 0
    ts = []
    for _ in range(20 * rl):
        t0 = time.perf_counter(); rc, _y = ml.run(xb); ts.append(time.perf_counter() - t0)
        assert rc == 0
    assert ml.fade_remaining() > 0
    print("%.3f %d %.1f %.2f" % (float(np.median(spans)), launches, float(np.median(rates)), float(np.median(ts[4 * rl:])) * 1e6))
    ml.close()


def pairs():
    lower = True
    for n_in, n_out in SHAPES:
        print("    (b) %d -> %d, every block of %d fading (K = %d), MAC span per chunk [us] | launches | Moutput-samples/s | one-block run() median [us]"
              % (n_in, n_out, NB, NB))
        for rep in range(REPS):
            got = {}
            for duo in ("1", "0"):
                env = dict(os.environ, BFIR_MFADE_DUO=duo)
                env.pop("BFIR_LIB_OVERRIDE", None)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "fading", str(n_in), str(n_out)], capture_output=True,
                                   text=True, timeout=150, env=env)
                if p.returncode != 0:
                    raise SystemExit("pairs: BFIR_MFADE_DUO=%s failed\n%s" % (duo, p.stderr[-1500:]))
                got[duo] = [float(v) for v in p.stdout.split()]
                print("        rep %d BFIR_MFADE_DUO=%s  %9.3f | %6d | %9.1f | %8.2f" % ((rep, duo) + tuple(got[duo])))
                print("pairs: %d -> %d rep %d duo=%s done" % (n_in, n_out, rep, duo), file=sys.stderr, flush=True)
            both = got["1"][0] < got["0"][0] and got["1"][3] < got["0"][3]
            lower = lower and both
            print("        rep %d duo / two launches: span %.3f, one-block run() %.3f: %s"
                  % (rep, got["1"][0] / got["0"][0], got["1"][3] / got["0"][3], "lower on both" if both else "NOT lower on both"))
    print("    k_mac_duo lower on both quantities in every paired run: %s" % ("yes" if lower else "no"))


def uniform():
    bfir, sets, x, y = _setup(2, 2)
    uni = bfir.BrutefirMatrix(L, -(-TAPS // L), S, 2, 2)
    assert uni.set_coeff(sets[0]) == 0
    _timed(uni, x, y)
    ts = [_timed(uni, x, y, lambda: uni.set_coeff_fade(sets[1 - i % 2], NB) == 0 or sys.exit("set_coeff_fade")) for i in range(4)][1:]
    r = [NB * L * 2 / t / 1e6 for t in ts]
    print("    (c) BrutefirMatrix(512, %d, 4, 2, 2), every block of %d fading: median %.1f Moutput-samples/s (%.1f .. %.1f)"
          % (-(-TAPS // L), NB, float(np.median(r)), min(r), max(r)))
    uni.close()


if __name__ == "__main__":
    if len(sys.argv) > 1:
        fn = {"ab": ab, "pairs": pairs, "uniform": uniform, "one": one}.get(sys.argv[1])
        if sys.argv[1] == "fading":
            fading(int(sys.argv[2]), int(sys.argv[3]))
        elif not fn:
            raise SystemExit("unknown step " + sys.argv[1])
        else:
            fn()
        sys.exit(0)
    out = []
    for step in STEPS:
        try:
            # a step's lines are kept for the file; its progress notes (stderr) pass through as they come
            p = subprocess.run([sys.executable, os.path.abspath(__file__), step], stdout=subprocess.PIPE, text=True, timeout=900)
        except subprocess.TimeoutExpired:
            print("step %s ran into its time limit; stopping" % step); break
        sys.stdout.write(p.stdout); sys.stdout.flush()
        if p.returncode != 0:
            print("step %s failed (%d); stopping" % (step, p.returncode)); break
        out.append(p.stdout)
    else:
        with open(os.path.join(ROOT, "profiles", "mlevels_fade_shape.txt"), "w") as f:
            f.write("# python scripts/mlevels_fade_shape.py -- one MI355X, one session (%s, csrc %s), every step in a process of its own\n"
                    % (time.strftime("%Y-%m-%d"), csrc_hash()) + "".join(out))
