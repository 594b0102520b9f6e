"""The wall time of the coefficient calls of the uniform engines under two builds of the library: this tree's and another
(the parent commit's libbfir_hip.so, loaded through BFIR_LIB_OVERRIDE).  scripts/pairs_shape.py, bank_shape.py,
bankmix_shape.py and the steps of fade_shape.py run RUNS times under each build, alternating, every run a process of its own
under its own time limit; the first that fails ends the measurement.  A row is a line of those scripts (its median where the
script repeats a call itself); per row and build the minimum, median and maximum over the runs, and whether the new median
lies within the other build's minimum .. maximum -- its own spread on the machine of the day is the yardstick for host-bound
calls of tens of microseconds to milliseconds.

    python scripts/coeff_uniform_shape.py OTHER_LIB [RUNS [SUBSTRING_OF_JOB ...]]
"""
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHOW = re.compile(r"^\s+(\S.*?)\s{2,}(?:\d+\.\d+ )+\s+min \S+\s+median (\S+)\s+max \S+ (\w+)\s*$")
TIME = re.compile(r"(\d+(?:\.\d+)?) (ms|us)\b")


def jobs(tmp):
    """(name, argv behind the script, extra environment, seconds)"""
    out = [("pairs_shape.py", [], {}, 180),
           ("bank_shape.py", ["report", "", os.path.join(tmp, "bank.txt")], {}, 240),
           ("bankmix_shape.py", [os.path.join(tmp, "bankmix.txt")], {}, 240)]
    for step in ("latency_f64", "latency_f32", "continuous_matrix", "continuous_diag8", "kernels_diag8", "kernels_stereo"):
        out.append(("fade_shape.py " + step, [step], {"BFIR_PIPE": "1"} if step.startswith("kernels") else {}, 150))
    return out


def rows_of(job, text):
    """{row: (value, unit)} of one run's output."""
    rows = {}
    for ln in text.splitlines():
        m = SHOW.match(ln)
        if m:
            rows["%s: %s" % (job, m.group(1))] = (float(m.group(2)), m.group(3))
        elif job.startswith("fade_shape"):
            label = TIME.sub("#", ln).strip()
            for k, (v, unit) in enumerate(TIME.findall(ln)):
                rows["%s: %s [%d]" % (job, re.sub(r"\d+\.\d+", "#", label)[:60], k)] = (float(v), unit)
    return rows


def main():
    other, runs, only = os.path.abspath(sys.argv[1]), int(sys.argv[2]) if len(sys.argv) > 2 else 5, sys.argv[3:]
    assert os.path.exists(other), other
    got = {}                                                     # row -> build -> [values]
    units, order = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for job, argv, extra, limit in jobs(tmp):
            if only and not any(s in job for s in only):
                continue
            script = os.path.join(ROOT, "scripts", job.split()[0])
            for r in range(runs):
                for build in ("parent", "new"):
                    env = dict(os.environ, **extra)
                    env.pop("BFIR_LIB_OVERRIDE", None)
                    if build == "parent":
                        env["BFIR_LIB_OVERRIDE"] = other
                    t = time.time()
                    p = subprocess.run([sys.executable, script] + argv, capture_output=True, text=True, timeout=limit, env=env)
                    if p.returncode != 0:
                        raise SystemExit("%s (%s, run %d) failed (%d); stopping\n%s" % (job, build, r, p.returncode, p.stderr[-3000:]))
                    print("# %s %s run %d: %.0f s" % (job, build, r, time.time() - t), flush=True)
                    for row, (v, unit) in rows_of(job, p.stdout).items():
                        if row not in got:
                            got[row] = {"parent": [], "new": []}
                            order.append(row)
                        got[row][build].append(v); units[row] = unit
    med = lambda v: sorted(v)[len(v) // 2]
    print("%d runs of each job under each build, alternating parent, new; per row min / median / max over the runs" % runs)
    print("%-100s %-4s %27s   %27s   %s" % ("row", "unit", "parent", "new", "new median within parent's min .. max"))
    outside = []
    for row in order:
        a, b = got[row]["parent"], got[row]["new"]
        inside = min(a) <= med(b) <= max(a)
        if not inside:
            outside.append(row)
        print("%-100s %-4s %8.3f %8.3f %8.3f   %8.3f %8.3f %8.3f   %s" % (row, units[row], min(a), med(a), max(a), min(b), med(b), max(b),
                                                                         "yes" if inside else "NO (%s)" % ("below" if med(b) < min(a) else "above")))
    print("%d rows, %d outside: %s" % (len(order), len(outside), "; ".join(outside) or "none"))


if __name__ == "__main__":
    main()
