"""Multi-level mimo engines (bfir_engine_create_mimo_levels) on dense fp32 matrices: 16 -> 16 and 32 -> 32 at L = 256 with
65536 taps per filter.  The levels are 8 x 256, 8 x 2048, 6 x 8192 (ratios 1, 8, 4: 22 partitions per pair, capacity
67584 taps); the uniform engine has 256 partitions of 256.

    engine  the multi-level engine against the uniform mimo engine (bfir_engine_create_mimo) on the same L and taps:
            the time of 4096 blocks in one run_device on device buffers, and the time of a one-block run() (64 calls in a
            row, so every level's block completes among them: mean and longest call).
    fade    every block fading on the multi-level engine, BFIR_MFADE_DUO=1 (k_wduo) against =0 (k_mac_mimo twice): the same
            two quantities.  The rule for the default: k_wduo only if its highest run lies below the other's lowest at
            both shapes.

Alternating runs, seven per side (the rule of profiles/quad_io.txt): lowest / median / highest.
python scripts/mimo_levels_shape.py [engine|fade] [blocks]"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import foo_dsp_bfir_amd as bfir

mode = sys.argv[1] if len(sys.argv) > 1 else "engine"
nb = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
rng = np.random.default_rng(1)
RUNS, ONE = 7, 64
L, TAPS = 256, 65536
BLOCKS, RATIOS = (8, 8, 6), (1, 8, 4)


def filters(n_in, n_out):
    g = 0.02 / n_in
    return [[(rng.standard_normal(TAPS) * g).astype(np.float32) for _ in range(n_in)] for _ in range(n_out)]


class Job:
    """One engine on device buffers; fade: the second filter set, and every timed block fades."""

    def __init__(self, eng, rows, x, n_out, fade=None):
        self.e, self.rows, self.fade = eng, rows, fade
        assert eng.set_coeff(rows) == 0
        self.x, self.y = x, torch.empty((nb * L, n_out), dtype=torch.float32, device="cuda")
        self.xh = x[:ONE * L].cpu().numpy()
        self.flip = False

    def prepare(self):
        if self.fade is not None:                      # a fade over exactly the blocks of this run; the sets take turns
            self.flip = not self.flip
            assert self.e.fade_to_rows(self.fade if self.flip else self.rows, ONE + nb) == 0

    def one_block_calls(self):
        """seconds of every one of ONE one-block run() calls"""
        ts = []
        for b in range(ONE):
            t0 = time.perf_counter()
            rc, _ = self.e.run(self.xh[b * L:(b + 1) * L])
            ts.append(time.perf_counter() - t0)
            assert rc == 0
        return ts

    def long_call(self):
        t0 = time.perf_counter()
        self.e.run_device(self.x.data_ptr(), self.y.data_ptr(), nb)
        assert self.e.sync() == 0
        return time.perf_counter() - t0


def alternate(jobs):
    """{name: ([s per nb blocks], [mean s of a one-block run()], [longest])}: a warm-up of each, then RUNS rounds in turn."""
    out = {k: ([], [], []) for k in jobs}
    for r in range(RUNS + 1):
        for k, j in jobs.items():
            j.prepare()
            ts = j.one_block_calls()
            t = j.long_call()
            if r > 0:
                out[k][0].append(t); out[k][1].append(sum(ts) / len(ts)); out[k][2].append(max(ts))
    return out


def lmh(v, scale):
    v = sorted(v)
    return "%9.3f %9.3f %9.3f" % (v[0] * scale, v[len(v) // 2] * scale, v[-1] * scale)


def show(title, res):
    print(title)
    print("    %-34s %-31s %-31s %s" % ("", "ms per %d blocks (lo med hi)" % nb, "one-block run(), mean us", "one-block run(), longest us"))
    for k, (t, m, x) in res.items():
        print("    %-34s %s   %s   %s" % (k, lmh(t, 1e3), lmh(m, 1e6), lmh(x, 1e6)))


def mimo_levels(n, duo=None):
    if duo is not None:
        os.environ["BFIR_MFADE_DUO"] = duo             # read at creation
    e = bfir.BrutefirMimoLevels(L, BLOCKS, RATIOS, 4, n, n)
    os.environ.pop("BFIR_MFADE_DUO", None)
    return e


for n in (16, 32):
    rows = filters(n, n)
    x = torch.from_numpy(rng.random((nb * L, n), dtype=np.float32) * 2 - 1).cuda()
    if mode == "engine":
        u = Job(bfir.BrutefirMimo(L, TAPS // L, 4, n, n), rows, x, n)
        m = Job(mimo_levels(n), rows, x, n)
        u.long_call(); m.long_call()
        err = float((u.y - m.y).abs().max() / u.y.abs().max())
        u.e.reset(); m.e.reset()
        res = alternate({"uniform mimo, 256 x 256": u, "multi-level mimo, 8 + 8 + 6": m})
        show("%d -> %d dense fp32, L = %d, %d taps (the two engines: %.2g of the maximum apart)" % (n, n, L, TAPS, err), res)
        a, b = res["multi-level mimo, 8 + 8 + 6"], res["uniform mimo, 256 x 256"]
        med = lambda v: sorted(v)[len(v) // 2]
        print("    uniform / multi-level, medians: %.2f x per %d blocks, %.2f x per one-block run()" %
              (med(b[0]) / med(a[0]), nb, med(b[1]) / med(a[1])))
        print("    multi-level highest below the uniform engine's lowest: %s" % ("yes" if max(a[0]) < min(b[0]) else "no"))
    elif mode == "fade":
        rows2 = filters(n, n)
        d1 = Job(mimo_levels(n, "1"), rows, x, n, fade=rows2)
        d0 = Job(mimo_levels(n, "0"), rows, x, n, fade=rows2)
        for j in (d1, d0):                             # every level running before the first fade
            j.long_call()
        res = alternate({"BFIR_MFADE_DUO=1 (k_wduo)": d1, "BFIR_MFADE_DUO=0 (k_mac_mimo twice)": d0})
        same = bool(torch.equal(d1.y, d0.y))
        show("%d -> %d dense fp32, L = %d, %d taps, every block fading (same bytes: %s)" % (n, n, L, TAPS, same), res)
        a, b = res["BFIR_MFADE_DUO=1 (k_wduo)"], res["BFIR_MFADE_DUO=0 (k_mac_mimo twice)"]
        print("    k_wduo's highest below the two launches' lowest: %d blocks %s, one-block run() %s" %
              (nb, "yes" if max(a[0]) < min(b[0]) else "no", "yes" if max(a[1]) < min(b[1]) else "no"))
    else:
        raise SystemExit(__doc__)
    for j in ((u, m) if mode == "engine" else (d1, d0)):
        j.e.close()
    del x
    torch.cuda.empty_cache()
