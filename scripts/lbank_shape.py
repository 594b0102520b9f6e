"""Coefficient changes from a bank on a multi-level mimo engine (bfir_engine_set_coeff_matrix_levels_pairs_bank,
_pairs_bank_fade; k_lbank_gather) against the same changes from host taps (bfir_engine_set_coeff_matrix_levels_pairs,
_pairs_fade: the yardstick) on scripts/lpairs_shape.py's shape: 64 -> 64, fp32, L = 256, levels 8 x 256, 8 x 2048, 6 x 8192
(ratios 1, 8, 4), 65536 taps per filter.  One source moves: one column, 64 filters out of 4096, per call.  Two engines in one
process, one with a bank of 128 filters, its twin without; after every timed pair of calls both run the same K blocks and the
output bytes are compared -- nothing is printed unless all of them were equal.

    the wall time of the fade call and of the plain call, from the bank and from taps: alternating, seven each, a warm-up of
    each first; min / median / max
    levels_bank_load of the 128 entries in one call
    k_lbank_gather's own time, from a kernel trace made in a run of its own:

        rocprofv3 --kernel-trace --output-format csv -d DIR -o kt -- python scripts/lbank_shape.py trace
        python scripts/lbank_shape.py report DIR [profiles/lbank_shape.txt]

`trace` makes a few gathers and nothing else worth tracing; `report` (without DIR: no kernel time) measures the rest and
writes the file, with the hash of csrc/ it was taken on."""
import csv, glob, hashlib, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import foo_dsp_bfir_amd as bfir

MODE = sys.argv[1] if len(sys.argv) > 1 else "report"
TRACE_DIR = sys.argv[2] if len(sys.argv) > 2 else None
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "lbank_shape.txt")
RUNS = 7
L, TAPS, n, K, NE = 256, 65536, 64, 64, 128
BLOCKS, RATIOS = (8, 8, 6), (1, 8, 4)
rng = np.random.default_rng(1)
lines = []


def csrc_hash():
    d = os.path.join(ROOT, "foo-dsp-bfir_amd", "csrc")
    h = hashlib.sha256()
    for name in sorted(os.listdir(d)):
        h.update(name.encode()); h.update(open(os.path.join(d, name), "rb").read())
    return h.hexdigest()[:12]


def say(s):
    lines.append(s)


def show(name, v, unit):
    say("    %-50s %s   min %.3f  median %.3f  max %.3f %s" % (name, " ".join("%.3f" % f for f in v), min(v), sorted(v)[len(v) // 2], max(v), unit))


def med(v):
    return sorted(v)[len(v) // 2]


bank = [(rng.standard_normal(TAPS) * (0.02 / n)).astype(np.float32) for _ in range(NE)]
first = [[(o + i) % NE for i in range(n)] for o in range(n)]
e = bfir.BrutefirMimoLevels(L, BLOCKS, RATIOS, 4, n, n)
assert e.lbank_create(NE) == 0
torch.cuda.synchronize()
t = time.perf_counter()
assert e.lbank_load(0, bank) == 0
load_ms = (time.perf_counter() - t) * 1e3
col = lambda c: [(o, c) for o in range(n)]
ents = lambda r: [(17 * r + 3 * o + 1) % NE for o in range(n)]

if MODE == "trace":   # the first set from taps: every k_lbank_gather of the trace is one column on all three levels
    assert e.set_coeff([[bank[en] for en in r] for r in first]) == 0
    for r in range(RUNS):
        assert e.set_pairs_bank(col(r), ents(r)) == 0
    e.close()
    sys.exit(0)

assert e.set_bank(first) == 0
twin = bfir.BrutefirMimoLevels(L, BLOCKS, RATIOS, 4, n, n)
assert twin.set_coeff([[bank[en] for en in r] for r in first]) == 0
x = (rng.random((K * L, n), dtype=np.float32) * 2 - 1)
same = []


def blocks():
    (rc, y), (rct, yt) = e.run(x), twin.run(x)
    assert rc == rct == 0
    same.append(y.tobytes() == yt.tobytes())


def timed(f, *a):
    torch.cuda.synchronize()
    t = time.perf_counter()
    assert f(*a) == 0
    return (time.perf_counter() - t) * 1e3


def one(r, fade):
    """Run r: column r from entries ents(r); which of the two calls goes first alternates from one run of a kind to the next."""
    c, en = r % n, ents(r)
    taps = [bank[k] for k in en]
    calls = [(e.fade_to_pairs_bank, (col(c), en, K)) if fade else (e.set_pairs_bank, (col(c), en)),
             (twin.fade_to_pairs, (col(c), taps, K)) if fade else (twin.set_pairs, (col(c), taps))]
    order = (0, 1) if (r // 2) % 2 == 0 else (1, 0)
    ms = [0.0, 0.0]
    for k in order:
        ms[k] = timed(calls[k][0], *calls[k][1])
    blocks()
    assert e.fade_remaining() == twin.fade_remaining() == 0
    return ms


blocks()
one(0, True); one(1, False)                              # warm-up of each (the first fade allocates the second set)
res = {"fade_bank": [], "fade_taps": [], "plain_bank": [], "plain_taps": []}
for r in range(RUNS):
    a, b = one(2 + 2 * r, True)
    res["fade_bank"].append(a); res["fade_taps"].append(b)
    a, b = one(3 + 2 * r, False)
    res["plain_bank"].append(a); res["plain_taps"].append(b)
assert all(same), "the bank engine's output bytes differ from the twin's: %s" % same

geo = bfir.BrutefirMatrixLevels.geometry(L, BLOCKS, RATIOS)
row_bytes = [b * 2 * Lk * 4 for b, Lk in zip(BLOCKS, geo[0])]
say("lbank_shape  %s  csrc %s" % (time.strftime("%Y-%m-%d"), csrc_hash()))
say("%d -> %d fp32, L = %d, levels %s x ratios %s, %d taps; one column (%d pairs) replaced per call; %d runs each, alternating; %d blocks"
    " run on both engines after every pair of calls, %d comparisons of output bytes, all equal"
    % (n, n, L, BLOCKS, RATIOS, TAPS, n, RUNS, K, len(same)))
say("the call itself, wall time:")
show("pairs_bank_fade (3 copies of H, one gather, catch-up)", res["fade_bank"], "ms")
show("pairs_fade from taps (3 copies of H, 192 loads, catch-up)", res["fade_taps"], "ms")
show("pairs_bank (one gather)", res["plain_bank"], "ms")
show("pairs from taps (192 loads)", res["plain_taps"], "ms")
say("the bank call's highest run below the call with taps' lowest: fade %s, plain %s; medians: fade %.2fx, plain %.2fx" %
    ("yes" if max(res["fade_bank"]) < min(res["fade_taps"]) else "no", "yes" if max(res["plain_bank"]) < min(res["plain_taps"]) else "no",
     med(res["fade_taps"]) / med(res["fade_bank"]), med(res["plain_taps"]) / med(res["plain_bank"])))
say("levels_bank_load of %d entries in one call (per level one upload and one transform launch): %.1f ms; the bank is %.1f MiB"
    % (NE, load_ms, NE * sum(row_bytes) / 2.0 ** 20))
say("one gather writes %d rows on three levels, %s = %d KiB per row, %d KiB in all" % (n, " + ".join(str(b) for b in row_bytes),
                                                                                 sum(row_bytes) >> 10, n * sum(row_bytes) >> 10))
if TRACE_DIR:
    dur = []
    for path in glob.glob(os.path.join(TRACE_DIR, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            if "k_lbank_gather" in row["Kernel_Name"]:
                dur.append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    assert dur, "no k_lbank_gather in the kernel trace under %s" % TRACE_DIR
    say("k_lbank_gather over the same %d rows of all levels, from the kernel trace of a run of its own (%d launches):" % (n, len(dur)))
    show("k_lbank_gather", dur, "us")
else:
    say("k_lbank_gather's own time: no kernel trace given")
e.close(); twin.close()
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
open(OUT, "w").write(text)
print(text, end="")
