"""Mimo engines (bfir_engine_create_mimo, k_mac_mimo) on device buffers, dense fp32 matrices.

    wide   16 -> 16 and 32 -> 32 at L = 1024, B = 16 against what the same job takes without them: a grid of 8 x 8
           BrutefirMatrix engines, every one on its own stream with the input groups already split into buffers of their own,
           the partial outputs of an output group summed by one torch reduction.  Alternating runs, seven each (the rule of
           profiles/quad_io.txt); the mimo engine's lowest frames/s has to lie above the grid's highest.
    small  8 -> 8 (L = 1024, B = 16) and 2 -> 2 (L = 4096, B = 32) on a mimo engine with BFIR_MIMO_MAC=1 (k_mac_mimo)
           against =0 (k_mac_matrix), the same way: which kernel such engines get by default.
    mac    the MAC step alone at 32 -> 32 (event-timed, one stream): time per launch and lane-FMA/s.
    pmc    one 32 -> 32 run of one launch, for a counter run (rocprofv3 --pmc FETCH_SIZE ... -- python scripts/mimo_shape.py pmc).

Frames/s = input frames per second.  python scripts/mimo_shape.py [wide|small|mac|pmc] [blocks]"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import foo_dsp_bfir_amd as bfir

mode = sys.argv[1] if len(sys.argv) > 1 else "wide"
nb = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
rng = np.random.default_rng(1)
RUNS, CALLS = 7, 3


def filters(L, B, n_in, n_out):
    g = 0.02 / n_in
    return [[(rng.standard_normal(B * L) * g).astype(np.float32) for _ in range(n_in)] for _ in range(n_out)]


def frames(L, n):
    return torch.from_numpy(rng.random((nb * L, n), dtype=np.float32) * 2 - 1).cuda()


class Mimo:
    def __init__(self, L, B, n_in, n_out, rows, x, mac=None):
        if mac is not None:
            os.environ["BFIR_MIMO_MAC"] = mac          # read at creation
        self.e = bfir.BrutefirMimo(L, B, 4, n_in, n_out)
        os.environ.pop("BFIR_MIMO_MAC", None)
        assert self.e.set_coeff(rows) == 0
        self.x, self.y = x, torch.empty((nb * L, n_out), dtype=torch.float32, device="cuda")

    def go(self):
        self.e.run_device(self.x.data_ptr(), self.y.data_ptr(), nb)

    def wait(self):
        assert self.e.sync() == 0


class Grid:
    """The workaround: engine (go, gi) convolves input group gi with block (go, gi) of the matrix into partial[go][gi]."""

    def __init__(self, L, B, n_in, n_out, rows, x):
        self.n_gi, self.n_go = n_in // 8, n_out // 8
        self.xs = [x[:, 8 * g:8 * g + 8].contiguous() for g in range(self.n_gi)]
        self.part = [torch.empty((self.n_gi, nb * L, 8), dtype=torch.float32, device="cuda") for _ in range(self.n_go)]
        self.y = torch.empty((nb * L, n_out), dtype=torch.float32, device="cuda")
        self.engines = []
        for go in range(self.n_go):
            for gi in range(self.n_gi):
                e = bfir.BrutefirMatrix(L, B, 4, 8, 8)
                assert e.set_coeff([r[8 * gi:8 * gi + 8] for r in rows[8 * go:8 * go + 8]]) == 0
                self.engines.append((e, go, gi))
        torch.cuda.synchronize()

    def go(self):
        for e, go, gi in self.engines:
            e.run_device(self.xs[gi].data_ptr(), self.part[go][gi].data_ptr(), nb)

    def wait(self):
        for e, _, _ in self.engines:
            assert e.sync() == 0
        for go in range(self.n_go):
            torch.sum(self.part[go], dim=0, out=self.y[:, 8 * go:8 * go + 8])
        torch.cuda.synchronize()


def one_run(job):
    t0 = time.perf_counter()
    for _ in range(CALLS):
        job.go(); job.wait()
    return (time.perf_counter() - t0) / CALLS


def alternate(L, jobs):
    """{name: [frames/s of every run]}: a warm-up of each, then RUNS rounds of every job in turn."""
    for j in jobs.values():
        one_run(j)
    out = {k: [] for k in jobs}
    for _ in range(RUNS):
        for k, j in jobs.items():
            out[k].append(nb * L / one_run(j))
    return out


def show(title, res):
    print(title)
    for k, v in res.items():
        print("    %-28s %s   min %.1f  median %.1f  max %.1f Mframes/s" % (k, " ".join("%.1f" % (f / 1e6) for f in v), min(v) / 1e6,
                                                                          sorted(v)[len(v) // 2] / 1e6, max(v) / 1e6))


if mode == "wide":
    L, B = 1024, 16
    for n in (16, 32):
        rows, x = filters(L, B, n, n), frames(L, n)
        m, g = Mimo(L, B, n, n, rows, x), Grid(L, B, n, n, rows, x)
        m.go(); m.wait(); g.go(); g.wait()
        err = float((m.y - g.y).abs().max() / g.y.abs().max())
        res = alternate(L, {"mimo engine": m, "grid of 8 x 8 engines": g})
        show("%d -> %d dense fp32, L = %d, B = %d, %d blocks per call (mimo against grid: %.2g of the maximum apart)" % (n, n, L, B, nb, err), res)
        print("    mimo lowest above the grid's highest: %s" % ("yes" if min(res["mimo engine"]) > max(res["grid of 8 x 8 engines"]) else "no"))
        m.e.close()
        for e, _, _ in g.engines:
            e.close()
        del m, g, x
        torch.cuda.empty_cache()
elif mode == "small":
    for L, B, n in ((1024, 16, 8), (4096, 32, 2)):
        rows, x = filters(L, B, n, n), frames(L, n)
        a, b = Mimo(L, B, n, n, rows, x, "1"), Mimo(L, B, n, n, rows, x, "0")
        a.go(); a.wait(); b.go(); b.wait()
        same = bool(torch.equal(a.y, b.y))
        res = alternate(L, {"BFIR_MIMO_MAC=1 (k_mac_mimo)": a, "BFIR_MIMO_MAC=0 (k_mac_matrix)": b})
        show("%d -> %d dense fp32, L = %d, B = %d, %d blocks per call (same bytes: %s)" % (n, n, L, B, nb, same), res)
        a.e.close(); b.e.close()
        del a, b, x
        torch.cuda.empty_cache()
elif mode in ("mac", "pmc"):
    L, B, n = 1024, 16, 32
    os.environ["BFIR_PIPE"] = "1"                      # one stream: a kernel's events time that kernel alone
    m = Mimo(L, B, n, n, filters(L, B, n, n), frames(L, n))
    os.environ.pop("BFIR_PIPE", None)
    m.go(); m.wait()
    if mode == "mac":
        m.e.set_profiling(True)
        for _ in range(RUNS):
            m.go(); m.wait()
        ms, launches = m.e.profile()["k_mac"]
        per = ms / launches
        fma = 4.0 * n * n * B * L * (nb * RUNS / launches)     # lane-FMAs of a launch: four per complex MAC, N / 2 = L bins
        print("k_mac_mimo at %d -> %d, L = %d, B = %d: %d launches of %d blocks, %.3f ms each, %.1f T lane-FMA/s" %
              (n, n, L, B, launches, nb * RUNS // launches, per, fma / (per * 1e-3) / 1e12))
        print("    H is %.0f MiB; the delay-line window of a launch %.0f MiB; its products %.0f MiB" %
              (n * n * B * 2 * L * 4 / 2**20, n * (nb * RUNS // launches + B - 1) * 2 * L * 4 / 2**20, n * (nb * RUNS // launches) * 2 * L * 4 / 2**20))
    else:
        m.go(); m.wait()
    m.e.close()
else:
    raise SystemExit(__doc__)
