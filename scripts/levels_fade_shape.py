"""What a crossfaded coefficient change costs on a multi-level engine (bfir_engine_set_coeff_levels_fade), at the three-level
shape scripts/levels_shape.py measures: fp32, 8 channels, L = 512, 131072 taps, levels (4, 3, 15) x (512, 2048, 8192), frames
resident in HBM.

    rates   (a) Msamples/s of the multi-level engine outside a fade; (b) inside a long fade, K covering the timed span;
            (c) the uniform engine of the same L and taps inside a fade; and the wall time of the set call, which includes
            the catch-up (the tail blocks whose MAC runs again with the new set)
    ab      (a) again, against another build of the library (BFIR_LIB_OVERRIDE=<the parent commit's libbfir_hip.so>): the
            two builds alternate, one process each, REPS times; the spread of each build's own repetitions decides whether
            a difference means anything (the deeper tail delay line must not cost throughput)

Without an argument every step runs in a process of its own, under its own time limit, and the lines go to
profiles/levels_fade_shape.txt; the first step that fails ends the run.  `python scripts/levels_fade_shape.py STEP` runs one
step; `ab` needs BFIR_PARENT_LIB, the path of the other build, and is skipped without it."""
import os, subprocess, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GAIN = 0.0005
S, L, CN, TAPS, BLOCKS, RATIOS, NB = 4, 512, 8, 131072, (4, 3, 15), (1, 4, 4), 16384
REPS = 4
STEPS = ("rates", "ab")


def _setup():
    import torch
    import foo_dsp_bfir_amd as bfir
    rng = np.random.default_rng(9)
    h = [[(rng.standard_normal(TAPS) * GAIN).astype(np.float32) for _ in range(CN)] for _ in range(2)]
    x = torch.from_numpy((rng.random((NB * L, CN), dtype=np.float32) * 2 - 1)).cuda()
    y = torch.empty_like(x)
    torch.cuda.synchronize()
    return bfir, h, x, y


def _timed(e, x, y, before=None):
    """One run_device of NB blocks, `before` (the fade request) outside the timed span.  Seconds."""
    if before:
        before()
    t0 = time.perf_counter(); e.run_device(x.data_ptr(), y.data_ptr(), NB); assert e.sync() == 0
    return time.perf_counter() - t0


def _plain_rate(e, x, y, n=5):
    ts = [_timed(e, x, y) for _ in range(n)]            # the first repetition sizes the work buffers
    return NB * L * CN / float(np.median(ts[1:])) / 1e6, [NB * L * CN / t / 1e6 for t in ts[1:]]


def rates():
    bfir, h, x, y = _setup()
    lv = bfir.BrutefirLevels(L, BLOCKS, RATIOS, S, CN, 8, 8)
    uni = bfir.Brutefir(L, -(-TAPS // L), S, CN, 8, 8)
    assert lv.max_taps >= TAPS > lv.D[-1]
    assert lv.set_coeff(h[0]) == 0 and uni.set_coeff(h[0]) == 0
    print("fp32, %d channels, L = %d, %d taps: levels %s of %s; uniform B = %d; %d blocks per run, frames in HBM"
          % (CN, L, TAPS, "+".join(map(str, BLOCKS)), "/".join(map(str, lv.lengths)), -(-TAPS // L), NB))
    a, _ = _plain_rate(lv, x, y)
    print("    (a) levels, no fade             %9.1f Msamples/s" % a)
    set_ms, fade = [], []
    for i in range(4):                                  # K covers the timed span: every block of the run fades
        def ask():
            t0 = time.perf_counter(); rc = lv.fade_to(h[1 - i % 2], NB); set_ms.append((time.perf_counter() - t0) * 1e3)
            assert rc == 0
        fade.append(_timed(lv, x, y, ask))
        assert lv.fade_remaining() == 0
    b = NB * L * CN / float(np.median(fade[1:])) / 1e6  # the first fade allocates the second filter sets, rings and products
    print("    (b) levels, every block fades   %9.1f Msamples/s   (b) / (a) = %.2f" % (b, b / a))
    print("        the set call (filter upload, catch-up): first %.1f ms (allocates), then median %.1f ms" % (set_ms[0], float(np.median(set_ms[1:]))))
    u, _ = _plain_rate(uni, x, y)
    ufade = []
    for i in range(4):
        ufade.append(_timed(uni, x, y, lambda: uni.set_coeff_fade(h[1 - i % 2], NB) == 0 or sys.exit("set_coeff_fade")))
    c = NB * L * CN / float(np.median(ufade[1:])) / 1e6
    print("    (c) uniform, every block fades  %9.1f Msamples/s   (uniform, no fade: %.1f)   (b) / (c) = %.2f" % (c, u, b / c))
    a2, _ = _plain_rate(lv, x, y)
    print("    (a) again, after the fades      %9.1f Msamples/s" % a2)
    lv.close(); uni.close()


def one():
    """(a) of whichever build BFIR_LIB_OVERRIDE names: one line, the repetitions' rates."""
    bfir, h, x, y = _setup()
    lv = bfir.BrutefirLevels(L, BLOCKS, RATIOS, S, CN, 8, 8)
    assert lv.set_coeff(h[0]) == 0
    med, each = _plain_rate(lv, x, y, 6)
    print("%.1f %s" % (med, " ".join("%.1f" % r for r in each)))
    lv.close()


def ab():
    other = os.environ.get("BFIR_PARENT_LIB")
    if not other or not os.path.exists(other):
        print("ab: BFIR_PARENT_LIB is not set: skipped")
        return
    res = {"parent": [], "this": []}
    for rep in range(REPS):
        for name in ("parent", "this"):
            env = dict(os.environ)
            env.pop("BFIR_LIB_OVERRIDE", None)
            if name == "parent":
                env["BFIR_LIB_OVERRIDE"] = other
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "one"], capture_output=True, text=True, timeout=120, env=env)
            if p.returncode != 0:
                raise SystemExit("ab: %s failed\n%s" % (name, p.stderr[-1500:]))
            res[name].append(float(p.stdout.split()[0]))
            print("    rep %d %-6s %s" % (rep, name, p.stdout.strip()))
    for name, v in res.items():
        print("    (a) %-6s median %.1f Msamples/s, spread of its %d runs %.1f .. %.1f (%.2f %%)"
              % (name, np.median(v), len(v), min(v), max(v), 100 * (max(v) - min(v)) / np.median(v)))
    d = 100 * (np.median(res["this"]) - np.median(res["parent"])) / np.median(res["parent"])
    sp = 100 * (max(res["parent"]) - min(res["parent"])) / np.median(res["parent"])
    print("    this / parent - 1 = %+.2f %%; the parent's own spread is %.2f %%: %s" % (d, sp, "equal" if abs(d) <= sp else "DIFFERENT"))


if __name__ == "__main__":
    if len(sys.argv) > 1:
        fn = {"rates": rates, "ab": ab, "one": one}.get(sys.argv[1])
        if not fn:
            raise SystemExit("unknown step " + sys.argv[1])
        fn()
        sys.exit(0)
    out = []
    for step in STEPS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), step], capture_output=True, text=True, timeout=420)
        except subprocess.TimeoutExpired:
            print("step %s ran into its time limit; stopping" % step); break
        sys.stdout.write(p.stdout); sys.stdout.flush()
        if p.returncode != 0:
            print("step %s failed (%d); stopping\n%s" % (step, p.returncode, p.stderr[-2000:])); break
        out.append(p.stdout)
    else:
        with open(os.path.join(ROOT, "profiles", "levels_fade_shape.txt"), "w") as f:
            f.write("# python scripts/levels_fade_shape.py -- one MI355X, one session, every step in a process of its own\n" + "".join(out))
