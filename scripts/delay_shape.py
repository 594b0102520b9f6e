"""What per-channel delays (bfir_engine_delay_init / _set_delay) cost, and what they save against zero taps in front
of the filters.

    headline   8 channels, L = 4096, 32 partitions, fp32, I/O resident in HBM, four configurations alternated in one
               process: the plain engine; whole-sample delays on both sides; sub-sample delays (h = 16) on both sides;
               and the plain engine on another build of the library -- the parent commit's, named by BFIR_LIB_OVERRIDE
               (this script takes the variable for itself: the branch's library is loaded as usual).  A delayed side
               is one more pass over its frames: expect a visible cost.  The one condition: the plain engine's rate
               lies within the spread of the other build's rate.
    lowlat     8 channels, L = 128, three partition lengths, 16384 taps, 4800-frame delays on the input side against
               the workaround: the same engine with 4800 zero taps in front of every filter.
    pmc        rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE, one pass each and counters only, over one run of the
               headline shape with delays on: the bytes the delay kernels fetch and write against the bytes they must
               move (FETCH_SIZE doubled: gfx950 counts half of a wide read, scripts/summarize_pmc.py).

Without an argument every step runs in a process of its own, under its own time limit, and the lines go to
profiles/delay_shape.txt; the first step that fails ends the run.  `python scripts/delay_shape.py STEP` runs one step."""
import csv
import ctypes as C
import glob
import os
import shutil
import signal
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OTHER_LIB = os.environ.pop("BFIR_LIB_OVERRIDE", None)
GAIN = 0.0005
STEPS = ("headline", "lowlat", "pmc")
REPS = 10
PAIR = ("plain", "plain, other build")


def engine_on(path, bfir, L, B, s, Cn):
    """A Brutefir whose calls go to another build of the library (one without the delay entry points, too)."""
    from foo_dsp_bfir_amd import _lib
    lib = C.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    e = object.__new__(bfir.Brutefir)
    e.L, e.B, e.s, e.C, e.in_format, e.out_format, e.n_engines, e.device, e._lib = L, B, s, Cn, 8, 8, 1, 0, lib
    err = C.c_int(0)
    e._h = lib.bfir_engine_create_batch(1, L, B, s, Cn, 8, 8, 44100, 0, 0, C.byref(err))
    assert e._h, err.value
    return e


def timed(engines, x, y, nb, L, Cn):
    """Every engine REPS times, alternated; {name: Gsamples/s of each repetition} (one untimed pass first)."""
    rates = {k: [] for k in engines}
    names = list(engines)
    for rep in range(REPS + 1):
        # An engine's rate depends on what ran before it (a plain run right after a delayed, memory-bound one measured 3-5 %
        # faster than after another plain run).  The two builds of the plain engine run back to back and swap places every
        # repetition, so each follows the other, and the last engine of the list, equally often; without such a pair the
        # order is reversed every other repetition.
        order = list(names)
        if rep & 1:
            if PAIR[0] in order and PAIR[1] in order:
                i, j = order.index(PAIR[0]), order.index(PAIR[1])
                order[i], order[j] = order[j], order[i]
            else:
                order.reverse()
        for name in order:
            e = engines[name]
            t0 = time.perf_counter()
            e.run_device(x.data_ptr(), y.data_ptr(), nb)
            assert e.sync() == 0
            if rep:
                rates[name].append(nb * L * Cn / (time.perf_counter() - t0) / 1e9)
    return rates


def report(rates):
    for name, r in rates.items():
        print("    %-28s median %7.2f  min %7.2f  max %7.2f Gsamples/s" % (name, np.median(r), min(r), max(r)))


def headline():
    import torch
    import foo_dsp_bfir_amd as bfir
    s, L, B, Cn, nb, h_sub = 4, 4096, 32, 8, 8192, 16
    rng = np.random.default_rng(9)
    h = [(rng.standard_normal(B * L) * GAIN).astype(np.float32) for _ in range(Cn)]
    delays = [0, 1, 48, 480, 1000, 2400, 4095, 4800]
    engines = {"plain": bfir.Brutefir(L, B, s, Cn)}
    if OTHER_LIB:
        engines["plain, other build"] = engine_on(OTHER_LIB, bfir, L, B, s, Cn)
    engines["whole-sample, both sides"] = bfir.Brutefir(L, B, s, Cn)
    engines["sub-sample h = 16, both sides"] = bfir.Brutefir(L, B, s, Cn)
    for e in engines.values():
        assert e.set_coeff(h) == 0
    for side in (0, 1):
        e = engines["whole-sample, both sides"]
        assert e.delay_init(side, 4800) == 0 and e.set_delay(side, delays) == 0
        e = engines["sub-sample h = 16, both sides"]
        assert e.delay_init(side, 4800, 100, h_sub) == 0 and e.set_delay(side, delays, [0, 1, -1, 50, -50, 99, -99, 7]) == 0
    x = torch.from_numpy((rng.random((nb * L, Cn), dtype=np.float32) * 2 - 1)).cuda()
    y = torch.empty_like(x)
    torch.cuda.synchronize()
    print("headline: fp32, %d channels, L = %d, B = %d, %d blocks per call, I/O in HBM, delays %s of up to 4800 frames; %d "
          "repetitions each, alternated" % (Cn, L, B, nb, delays, REPS))
    rates = timed(engines, x, y, nb, L, Cn)
    report(rates)
    p = np.median(rates["plain"])
    print("    whole-sample / plain = %.3f   sub-sample / plain = %.3f" % (np.median(rates["whole-sample, both sides"]) / p,
                                                                          np.median(rates["sub-sample h = 16, both sides"]) / p))
    if OTHER_LIB:
        o = rates["plain, other build"]
        print("    plain / other build = %.3f; the plain median %s the other build's spread [%.2f, %.2f]"
              % (p / np.median(o), "lies within" if min(o) <= p <= max(o) else "is OUTSIDE", min(o), max(o)))
    else:
        print("    no other build given (BFIR_LIB_OVERRIDE): not measured")
    for e in engines.values():
        e.close()


def lowlat():
    import torch
    import foo_dsp_bfir_amd as bfir
    s, L, Cn, taps, d, nb = 4, 128, 8, 16384, 4800, 16384
    blocks, ratios = (8, 8, 14), (1, 4, 4)
    rng = np.random.default_rng(10)
    h = [(rng.standard_normal(taps) * GAIN).astype(np.float32) for _ in range(Cn)]
    hz = [np.r_[np.zeros(d, np.float32), v] for v in h]
    engines = {"plain (no delay)": bfir.BrutefirLevels(L, blocks, ratios, s, Cn), "delay kernels": bfir.BrutefirLevels(L, blocks, ratios, s, Cn),
               "zero taps in front": bfir.BrutefirLevels(L, blocks, ratios, s, Cn)}
    assert engines["plain (no delay)"].set_coeff(h) == 0 and engines["delay kernels"].set_coeff(h) == 0
    assert engines["zero taps in front"].set_coeff(hz) == 0
    e = engines["delay kernels"]
    assert e.delay_init(0, d) == 0 and e.set_delay(0, [d] * Cn) == 0
    x = torch.from_numpy((rng.random((nb * L, Cn), dtype=np.float32) * 2 - 1)).cuda()
    y = torch.empty_like(x)
    torch.cuda.synchronize()
    print("lowlat: fp32, %d channels, L = %d, levels blocks %s ratios %s, %d taps, every channel delayed by %d frames; %d blocks "
          "per call, %d repetitions each, alternated" % (Cn, L, blocks, ratios, taps, d, nb, REPS))
    rates = timed(engines, x, y, nb, L, Cn)
    report(rates)
    print("    delay kernels / zero taps = %.3f   delay kernels / plain = %.3f"
          % (np.median(rates["delay kernels"]) / np.median(rates["zero taps in front"]),
             np.median(rates["delay kernels"]) / np.median(rates["plain (no delay)"])))
    xb = (rng.random((L, Cn), dtype=np.float32) * 2 - 1)
    yb = np.zeros_like(xb)
    for name, e in engines.items():
        e.reset()
        ts = []
        for i in range(400):
            t0 = time.perf_counter(); rc, _ = e.run(xb, yb); ts.append(time.perf_counter() - t0)
            assert rc == 0
        ts = np.array(ts[100:]) * 1e6
        print("    %-28s one-block run(): median %.1f us, p90 %.1f us, max %.1f us" % (name, np.median(ts), np.percentile(ts, 90), ts.max()))
    for e in engines.values():
        e.close()


def pmc_subject():
    """What the counter passes run: one call of 256 headline blocks per delayed configuration."""
    import torch
    import foo_dsp_bfir_amd as bfir
    s, L, B, Cn, nb = 4, 4096, 32, 8, 256
    rng = np.random.default_rng(11)
    h = [(rng.standard_normal(B * L) * GAIN).astype(np.float32) for _ in range(Cn)]
    x = torch.from_numpy((rng.random((nb * L, Cn), dtype=np.float32) * 2 - 1)).cuda()
    y = torch.empty_like(x)
    torch.cuda.synchronize()
    for steps in (0, 100):
        e = bfir.Brutefir(L, B, s, Cn)
        assert e.set_coeff(h) == 0
        for side in (0, 1):
            assert e.delay_init(side, 4800, steps, 16 if steps else 0) == 0
            assert e.set_delay(side, [0, 1, 48, 480, 1000, 2400, 4095, 4800], [0, 1, -1, 50, -50, 99, -99, 7] if steps else None) == 0
        e.run_device(x.data_ptr(), y.data_ptr(), nb)
        assert e.sync() == 0
        e.close()


def run_group(cmd, limit, env=None):
    """cmd in a process group of its own, under a time limit; at the limit the whole group is killed -- a profiler's child
    too -- so that nothing of it keeps the GPU open.  (returncode or None at the limit, stdout, stderr)"""
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, start_new_session=True)
    try:
        out, err = p.communicate(timeout=limit)
        return p.returncode, out, err
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        out, err = p.communicate()
        return None, out, err


PASS_LIMIT, STEP_LIMIT = 120, 280   # a counter pass (the pmc step runs two); a step


def pmc():
    rocprof = shutil.which("rocprofv3")
    if not rocprof:
        print("pmc: rocprofv3 is not on this machine: not measured")
        return
    tmp = tempfile.mkdtemp(prefix="delay_pmc_")
    per = {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):   # counters only, one pass each
        d = os.path.join(tmp, counter)
        rc, out, err = run_group([rocprof, "--pmc", counter, "--output-format", "csv", "-d", d, "-o", "c", "--", sys.executable,
                                  os.path.abspath(__file__), "pmc_subject"], PASS_LIMIT)
        if rc != 0:   # a pass that failed or ran into its limit ends the step: nothing more is started on the GPU
            shutil.rmtree(tmp, ignore_errors=True)
            raise SystemExit("rocprofv3 --pmc %s %s\n%s" % (counter, "ran into its time limit" if rc is None else "failed (%d)" % rc,
                                                            (out + err)[-2000:]))
        for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                if row.get("Counter_Name") == counter and "k_delay" in row["Kernel_Name"]:
                    kind = "k_delay_sub" if "k_delay_sub" in row["Kernel_Name"] else "k_delay_copy"
                    per.setdefault(kind, {}).setdefault(counter, []).append(float(row["Counter_Value"]) * 1024)
    shutil.rmtree(tmp, ignore_errors=True)
    nb, L, Cn, H = 256, 4096, 8, 4800
    piece = nb * L * Cn * 4
    print("pmc: one call of %d headline blocks (8 channels, fp32 frames: %.1f MB per side and pass), delays of up to 4800 "
          "frames on both sides; rocprofv3 --pmc, one counter per pass; FETCH_SIZE doubled" % (nb, piece / 1e6))
    must = {"k_delay_copy": "the delayed piece moves %.1f MB in and %.1f MB out; the history update %.2f MB each way (H = 4800 frames)"
                            % (piece / 1e6, piece / 1e6, H * Cn * 4 / 1e6),
            "k_delay_sub": "the delayed piece moves %.1f MB in and %.1f MB out (H = 4832 frames)" % (piece / 1e6, piece / 1e6)}
    for kind in sorted(per):
        f = [2 * v for v in per[kind].get("FETCH_SIZE", [])]
        w = per[kind].get("WRITE_SIZE", [])
        print("    %-13s %d launches: fetched %s MB, written %s MB" % (kind, max(len(f), len(w)), " ".join("%.2f" % (v / 1e6) for v in f),
                                                                   " ".join("%.2f" % (v / 1e6) for v in w)))
        print("                  %s" % must[kind])
    if not per:
        print("    no delay kernel in the counter files: not measured")


if __name__ == "__main__":
    if len(sys.argv) > 1:
        fn = {"headline": headline, "lowlat": lowlat, "pmc": pmc, "pmc_subject": pmc_subject}.get(sys.argv[1])
        if fn is None:
            raise SystemExit("unknown step " + sys.argv[1])
        fn()
        sys.exit(0)
    out = []
    env = dict(os.environ)
    if OTHER_LIB:
        env["BFIR_LIB_OVERRIDE"] = OTHER_LIB
    for step in STEPS:
        rc, so, se = run_group([sys.executable, os.path.abspath(__file__), step], STEP_LIMIT, env)
        if rc is None:
            print("step %s ran into its time limit; stopping" % step); break
        sys.stdout.write(so); sys.stdout.flush()
        if rc != 0:
            print("step %s failed (%d); stopping\n%s" % (step, rc, se[-2000:])); break
        out.append(so)
    else:
        with open(os.path.join(ROOT, "profiles", "delay_shape.txt"), "w") as f:
            f.write("# python scripts/delay_shape.py -- one MI355X, one session, every step in a process of its own\n" + "".join(out))
