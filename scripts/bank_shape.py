"""Coefficient changes from a bank (bfir_engine_set_coeff_matrix_pairs_bank, _pairs_bank_fade; k_bank_gather) against the
same changes from host taps (bfir_engine_set_coeff_matrix_pairs, _pairs_fade: the yardstick) on scripts/pairs_shape.py's
shape: a mimo engine 64 -> 64, fp32, L = 1024, B = 16; one source moves: one column, 64 filters out of 4096.  Two engines in
one process, one with a bank of 2048 filters, its twin without; after every timed pair of calls both run the same blocks
and the output bytes are compared -- nothing is printed unless all of them were equal.

    the wall time of the fade call and of the plain call, from the bank and from taps: alternating, seven each, a warm-up of
    each first; min / median / max
    bank_load of 2048 entries in one call, next to 2048 single-row loads projected from the per-row figure of the plain
    pairs call from taps
    a device-to-device hipMemcpyAsync of the bytes one gather moves (64 rows), between events on its stream
    k_bank_gather's own time, from a kernel trace made in a run of its own:

        rocprofv3 --kernel-trace --output-format csv -d DIR -o kt -- python scripts/bank_shape.py trace
        python scripts/bank_shape.py report DIR [profiles/bank_shape.txt]

`trace` makes a few gathers and nothing else worth tracing; `report` (without DIR: no kernel time) measures the rest and
writes the file."""
import csv, ctypes, glob, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import foo_dsp_bfir_amd as bfir

MODE = sys.argv[1] if len(sys.argv) > 1 else "report"
TRACE_DIR = sys.argv[2] if len(sys.argv) > 2 else None
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bank_shape.txt")
RUNS = 7
L, B, n, K, NE = 1024, 16, 64, 4, 2048
rng = np.random.default_rng(1)
lines = []


def say(s):
    lines.append(s)


def filt():
    return (rng.standard_normal(B * L) * (0.02 / n)).astype(np.float32)


def show(name, v, unit):
    say("    %-46s %s   min %.3f  median %.3f  max %.3f %s" % (name, " ".join("%.3f" % f for f in v), min(v), sorted(v)[len(v) // 2], max(v), unit))


def med(v):
    return sorted(v)[len(v) // 2]


bank = [filt() for _ in range(NE)]
e = bfir.BrutefirMimo(L, B, 4, n, n)
assert e.bank_create(NE) == 0
torch.cuda.synchronize()
t = time.perf_counter()
assert e.bank_load(0, bank) == 0
load_ms = (time.perf_counter() - t) * 1e3
col = lambda c: [(o, c) for o in range(n)]
ents = lambda r: [(n * r + o) % NE for o in range(n)]
if MODE != "trace":
    assert e.set_coeff_bank([[(o * n + i) % NE for i in range(n)] for o in range(n)]) == 0

if MODE == "trace":   # the first set from taps: every k_bank_gather of the trace is one column
    assert e.set_coeff([[bank[(o * n + i) % NE] for i in range(n)] for o in range(n)]) == 0
    for r in range(RUNS):
        assert e.set_coeff_pairs_bank(col(r), ents(r)) == 0
    e.close()
    sys.exit(0)

twin = bfir.BrutefirMimo(L, B, 4, n, n)
assert twin.set_coeff([[bank[(o * n + i) % NE] for i in range(n)] for o in range(n)]) == 0
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
    calls = [(e.set_coeff_pairs_bank_fade, (col(c), en, K)) if fade else (e.set_coeff_pairs_bank, (col(c), en)),
             (twin.set_coeff_pairs_fade, (col(c), taps, K)) if fade else (twin.set_coeff_pairs, (col(c), taps))]
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

say("%d -> %d fp32, L = %d, B = %d; one column (%d pairs) replaced per call; %d runs each, alternating; %d blocks run on both engines"
    " after every pair of calls, %d comparisons of output bytes, all equal" % (n, n, L, B, n, RUNS, K, len(same)))
say("the call itself, wall time:")
show("pairs_bank_fade (copy of H, one gather)", res["fade_bank"], "ms")
show("pairs_fade from taps (copy of H, 64 loads)", res["fade_taps"], "ms")
show("pairs_bank (one gather)", res["plain_bank"], "ms")
show("pairs from taps (64 loads)", res["plain_taps"], "ms")
say("the bank call's highest run below the call with taps' lowest: fade %s, plain %s; medians: fade %.2fx, plain %.2fx" %
    ("yes" if max(res["fade_bank"]) < min(res["fade_taps"]) else "no", "yes" if max(res["plain_bank"]) < min(res["plain_taps"]) else "no",
     med(res["fade_taps"]) / med(res["fade_bank"]), med(res["plain_taps"]) / med(res["plain_bank"])))
per_row = med(res["plain_taps"]) / n
say("bank_load of %d entries in one call (one upload, one transform launch): %.1f ms; %d single-row loads at the plain pairs call's"
    " %.4f ms per row: %.1f ms" % (NE, load_ms, NE, per_row, NE * per_row))

# a device-to-device copy of the bytes one gather moves
row_bytes = B * 2 * L * 4
nbytes = n * row_bytes
loaded = sorted({ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln})   # the runtime this process already uses
hip = ctypes.CDLL(loaded[0] if loaded else "libamdhip64.so")
hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
stream = torch.cuda.current_stream()
copies = []
for k in range(RUNS + 1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    assert hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, stream.cuda_stream) == 0   # 3: hipMemcpyDeviceToDevice
    b.record(stream)
    torch.cuda.synchronize()
    if k:
        copies.append(a.elapsed_time(b) * 1e3)
say("the %d rows of one gather are %d KiB; a device-to-device hipMemcpyAsync of as many bytes, between events:" % (n, nbytes >> 10))
show("hipMemcpyAsync", copies, "us")
if TRACE_DIR:
    dur = []
    for path in glob.glob(os.path.join(TRACE_DIR, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            if "k_bank_gather" in row["Kernel_Name"]:
                dur.append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    assert dur, "no k_bank_gather in the kernel trace under %s" % TRACE_DIR
    say("k_bank_gather over the same %d rows, from the kernel trace of a run of its own (%d launches):" % (n, len(dur)))
    show("k_bank_gather", dur, "us")
else:
    say("k_bank_gather's own time: no kernel trace given")
e.close(); twin.close()
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
open(OUT, "w").write(text)
print(text, end="")
