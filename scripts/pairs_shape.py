"""Pair-list crossfades (bfir_engine_set_coeff_matrix_pairs_fade, k_patch_pairs) against whole-matrix crossfades on a mimo
engine: 64 -> 64, fp32, L = 1024, B = 16, frames resident in HBM, default chunk, one stream (BFIR_PIPE=1: a step's events
time that step alone).  One source moves: one column, 64 filters out of 4096, fades over K = 64 blocks.

    a   the MAC step per fading block under the pairs fade (the old set's k_mac_mimo, then k_patch_pairs)
    b   the same under the whole-matrix fade to the same kind of merged set (k_mac_mimo twice): the yardstick
    c   the MAC step per plain block
    and the wall time of the two fade calls themselves (table, copy of H, uploads and transforms).

Alternating runs, seven each, a warm-up of each first; min / median / max.  python scripts/pairs_shape.py [runs]"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import foo_dsp_bfir_amd as bfir

RUNS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
L, B, n, K = 1024, 16, 64, 64
rng = np.random.default_rng(1)


def column():
    return [(rng.standard_normal(B * L) * (0.02 / n)).astype(np.float32) for _ in range(n)]


rows = [column() for _ in range(n)]                     # rows[o][i]
x = torch.from_numpy(rng.random((K * L, n), dtype=np.float32) * 2 - 1).cuda()
y = torch.empty((K * L, n), dtype=torch.float32, device="cuda")
os.environ["BFIR_PIPE"] = "1"                           # read at creation
e = bfir.BrutefirMimo(L, B, 4, n, n)
os.environ.pop("BFIR_PIPE", None)
assert e.set_coeff(rows) == 0


def mac_per_block():
    """K blocks in one call: the MAC step's microseconds per block."""
    e.set_profiling(True)
    e.run_device(x.data_ptr(), y.data_ptr(), K)
    assert e.sync() == 0
    ms, launches = e.profile()["k_mac"]
    e.set_profiling(False)
    return ms / K * 1e3, launches


def pairs_fade(c):
    new = column()
    for o in range(n):
        rows[o][c] = new[o]
    torch.cuda.synchronize()
    t = time.perf_counter()
    assert e.set_coeff_pairs_fade([(o, c) for o in range(n)], new, K) == 0
    call = (time.perf_counter() - t) * 1e3
    per, launches = mac_per_block()
    assert e.fade_remaining() == 0
    return per, call, launches


def whole_fade(c):
    new = column()
    for o in range(n):
        rows[o][c] = new[o]
    torch.cuda.synchronize()
    t = time.perf_counter()
    assert e.set_coeff_fade(rows, K) == 0
    call = (time.perf_counter() - t) * 1e3
    per, launches = mac_per_block()
    assert e.fade_remaining() == 0
    return per, call, launches


def show(name, v, unit):
    print("    %-44s %s   min %.2f  median %.2f  max %.2f %s" % (name, " ".join("%.2f" % f for f in v), min(v), sorted(v)[len(v) // 2], max(v), unit))


mac_per_block(); pairs_fade(0); whole_fade(1)           # warm-up of each
res = {"a": [], "b": [], "c": [], "call_a": [], "call_b": []}
launches = {}
for r in range(RUNS):
    per, call, launches["a"] = pairs_fade((2 * r + 2) % n)
    res["a"].append(per); res["call_a"].append(call)
    per, call, launches["b"] = whole_fade((2 * r + 3) % n)
    res["b"].append(per); res["call_b"].append(call)
    per, launches["c"] = mac_per_block()
    res["c"].append(per)
print("%d -> %d fp32, L = %d, B = %d, one column fading over K = %d blocks, %d runs each, alternating" % (n, n, L, B, K, RUNS))
print("MAC step per block (launches per %d blocks: pairs fade %d, whole-matrix fade %d, plain %d):" % (K, launches["a"], launches["b"], launches["c"]))
show("a  pairs fade (k_mac_mimo + k_patch_pairs)", res["a"], "us")
show("b  whole-matrix fade (k_mac_mimo twice)", res["b"], "us")
show("c  plain block (k_mac_mimo)", res["c"], "us")
print("the fade call itself, wall time:")
show("pairs (table, copy of H, 64 filters)", res["call_a"], "ms")
show("whole matrix (4096 filters)", res["call_b"], "ms")
med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
print("a / b = %.2f at the median, a - c = %.2f us; a below b in every pair of runs: %s; the pairs call faster in every pair: %s" %
      (med["a"] / med["b"], med["a"] - med["c"], "yes" if max(res["a"]) < min(res["b"]) else "no",
       "yes" if max(res["call_a"]) < min(res["call_b"]) else "no"))
# what the call's copy of the whole store costs on its own
H_bytes = n * n * B * 2 * L * 4
a_, b_ = torch.empty(H_bytes, dtype=torch.uint8, device="cuda"), torch.empty(H_bytes, dtype=torch.uint8, device="cuda")
b_.copy_(a_); torch.cuda.synchronize()
copies = []
for _ in range(RUNS):
    t = time.perf_counter()
    b_.copy_(a_); torch.cuda.synchronize()
    copies.append((time.perf_counter() - t) * 1e3)
print("a device-to-device copy of the filter store alone (%d MiB; the pairs call waits for its own before it loads a row):" % (H_bytes >> 20))
show("copy", copies, "ms")
e.close()
