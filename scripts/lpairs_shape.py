"""Pair-list crossfades on a multi-level mimo engine (bfir_engine_set_coeff_matrix_levels_pairs_fade; k_patch_pairs, k_wpatch)
against the whole-matrix crossfade to the same merged set: 64 -> 64, fp32, L = 256, levels 8 x 256, 8 x 2048, 6 x 8192
(ratios 1, 8, 4), 65536 taps per filter, default chunk and streams.  One source moves: one column, 64 filters out of 4096,
fades over K = 64 head blocks.

    a    pairs fade, BFIR_PATCH_FUSED=1: a launch that takes both sets runs k_wpatch
    a'   pairs fade, BFIR_PATCH_FUSED=0: k_mac_mimo, then k_patch_pairs
    b    fade_to_rows with the whole matrix, the listed column replaced: what a caller could do before (k_wduo); the yardstick
    c    no fade

For each: the time of one run_device call of the K fading blocks on frames resident in HBM, and the mean and the longest of
K one-block run() calls (host frames) while fading -- a fade call ahead of each of the two -- and the wall time of the fade
calls themselves.  Every engine sees the same blocks in the same order, so the fades start at the same block on all of them.
Alternating runs, seven per side after a warm-up of each (the rule of profiles/quad_io.txt): lowest / median / highest.

The rules.  The pairs fade's default form must have its highest long call below b's lowest.  BFIR_PATCH_FUSED defaults to 1
only if a's highest lies below a''s lowest in the long call AND in the one-block mean (the rule scripts/mimo_levels_shape.py
states for k_wduo); else it defaults to 0 and k_wpatch stays behind the switch.
python scripts/lpairs_shape.py [runs]"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import foo_dsp_bfir_amd as bfir

RUNS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
L, TAPS, n, K = 256, 65536, 64, 64
BLOCKS, RATIOS = (8, 8, 6), (1, 8, 4)
rng = np.random.default_rng(1)


def taps():
    return (rng.standard_normal(TAPS) * (0.02 / n)).astype(np.float32)


base = [taps() for _ in range(n)]                       # 64 distinct filters: rows[o][i] = base[(o + i) % 64]
rows0 = [[base[(o + i) % n] for i in range(n)] for o in range(n)]
x = torch.from_numpy(rng.random((K * L, n), dtype=np.float32) * 2 - 1).cuda()
xh = x.cpu().numpy()


class Job:
    def __init__(self, kind, fused=None):
        self.kind = kind
        if fused is not None:
            os.environ["BFIR_PATCH_FUSED"] = fused      # read at creation
        self.e = bfir.BrutefirMimoLevels(L, BLOCKS, RATIOS, 4, n, n)
        os.environ.pop("BFIR_PATCH_FUSED", None)
        self.rows = [list(r) for r in rows0]
        assert self.e.set_coeff(self.rows) == 0
        self.y = torch.empty((K * L, n), dtype=torch.float32, device="cuda")
        self.calls = []

    def fade(self, col, new):
        """The fade call of this kind to the set with column `col` replaced; its wall time in seconds."""
        for o in range(n):
            self.rows[o][col] = new[o]
        if self.kind == "none":
            return
        torch.cuda.synchronize()
        t = time.perf_counter()
        if self.kind == "pairs":
            rc = self.e.fade_to_pairs([(o, col) for o in range(n)], new, K)
        else:
            rc = self.e.fade_to_rows(self.rows, K)
        self.calls.append(time.perf_counter() - t)
        assert rc == 0

    def long_call(self):
        t = time.perf_counter()
        self.e.run_device(x.data_ptr(), self.y.data_ptr(), K)
        assert self.e.sync() == 0
        return time.perf_counter() - t

    def one_block_calls(self):
        ts = []
        for b in range(K):
            t = time.perf_counter()
            rc, _ = self.e.run(xh[b * L:(b + 1) * L])
            ts.append(time.perf_counter() - t)
            assert rc == 0
        return ts


def lmh(v, scale):
    v = sorted(v)
    return "%10.3f %10.3f %10.3f" % (v[0] * scale, v[len(v) // 2] * scale, v[-1] * scale)


jobs = {"a   pairs fade, k_wpatch": Job("pairs", "1"), "a'  pairs fade, two launches": Job("pairs", "0"),
        "b   whole-matrix fade_to_rows": Job("rows"), "c   no fade": Job("none")}
for j in jobs.values():                                 # every level running before the first fade
    j.long_call(); j.long_call()
res = {k: ([], [], []) for k in jobs}
col = 0
for r in range(RUNS + 1):
    new1, new2 = [taps() for _ in range(n)], [taps() for _ in range(n)]
    for k, j in jobs.items():
        if r == 0:
            j.calls = []
        j.fade(col % n, new1)
        t = j.long_call()
        assert j.e.fade_remaining() == 0
        j.fade((col + 1) % n, new2)
        ts = j.one_block_calls()
        assert j.e.fade_remaining() == 0
        if r == 0:
            j.calls = []                                # the warm-up's calls (they allocate the second set) do not count
        else:
            res[k][0].append(t); res[k][1].append(sum(ts) / len(ts)); res[k][2].append(max(ts))
    col += 2
    print("round %d of %d done" % (r, RUNS), file=sys.stderr, flush=True)
ya, yb = jobs["a   pairs fade, k_wpatch"].y, jobs["a'  pairs fade, two launches"].y
print("%d -> %d fp32, L = %d, levels %s x ratios %s, %d taps; one column fades over K = %d blocks; %d runs each, alternating" %
      (n, n, L, BLOCKS, RATIOS, TAPS, K, RUNS))
print("a and a' wrote the same bytes in their last long call: %s" % bool(torch.equal(ya, yb)))
print("    %-32s %-34s %-34s %s" % ("", "ms per run_device of %d blocks" % K, "one-block run(), mean us", "one-block run(), longest us"))
for k, (t, m, w) in res.items():
    print("    %-32s %s   %s   %s" % (k, lmh(t, 1e3), lmh(m, 1e6), lmh(w, 1e6)))
print("the fade call itself, wall time in ms (lowest, median, highest of %d calls):" % (2 * RUNS))
for k, j in jobs.items():
    if j.calls:
        print("    %-32s %s" % (k, lmh(j.calls, 1e3)))
a, a2, b = (res[k] for k in list(jobs)[:3])
print("a's highest below a''s lowest: long call %s, one-block mean %s  (both yes: BFIR_PATCH_FUSED defaults to 1)" %
      ("yes" if max(a[0]) < min(a2[0]) else "no", "yes" if max(a[1]) < min(a2[1]) else "no"))
print("highest long call below b's lowest: a %s, a' %s" % ("yes" if max(a[0]) < min(b[0]) else "no", "yes" if max(a2[0]) < min(b[0]) else "no"))
print("highest one-block mean below b's lowest: a %s, a' %s" % ("yes" if max(a[1]) < min(b[1]) else "no", "yes" if max(a2[1]) < min(b[1]) else "no"))
for j in jobs.values():
    j.e.close()
