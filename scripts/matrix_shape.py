"""Throughput of matrix engines (n inputs -> m outputs, one filter per pair) on device buffers, and of the workaround a
diagonal engine needs for the same problem (n_in * n_out channels fed copies of the inputs, outputs summed by the caller;
the sum itself is not timed).  Frames/s = input frames per second; every shape runs the same number of blocks."""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import foo_dsp_bfir_amd as bfir

rng = np.random.default_rng(1)
nb = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
GAIN = 0.002


def timed(e, d_in, d_out, n):
    for _ in range(2):
        e.run_device(d_in.data_ptr(), d_out.data_ptr(), n); e.sync()
    t0 = time.perf_counter()
    for _ in range(4):
        e.run_device(d_in.data_ptr(), d_out.data_ptr(), n)
    assert e.sync() == 0
    return (time.perf_counter() - t0) / 4


def matrix(L, B, s, n_in, n_out, nz):
    dt = np.float64 if s == 8 else np.float32
    rows = [[(rng.standard_normal(B * L) * GAIN).astype(dt) if nz(o, i) else None for i in range(n_in)] for o in range(n_out)]
    e = bfir.BrutefirMatrix(L, B, s, n_in, n_out, 8, 8)
    assert e.set_coeff(rows) == 0
    x = torch.from_numpy((rng.random((nb * L, n_in), dtype=np.float32) * 2 - 1)).cuda()
    y = torch.empty((nb * L, n_out), dtype=torch.float32, device="cuda")
    dtm = timed(e, x, y, nb)
    e.close()
    return dtm


def workaround(L, B, s, n_in, n_out):
    dt = np.float64 if s == 8 else np.float32
    C = n_in * n_out
    e = bfir.Brutefir(L, B, s, C, 8, 8)
    assert e.set_coeff([(rng.standard_normal(B * L) * GAIN).astype(dt) for _ in range(C)]) == 0
    x = torch.from_numpy((rng.random((nb * L, C), dtype=np.float32) * 2 - 1)).cuda()
    y = torch.empty_like(x)
    dtm = timed(e, x, y, nb)
    e.close()
    return dtm


def report(name, dtm, L, macs_per_block):
    print("%-44s %7.2f Mframes/s  (%d blocks in %.2f ms, %.1f G complex MAC/s incl. FFTs)"
          % (name, nb * L / dtm / 1e6, nb, dtm * 1e3, nb * macs_per_block / dtm / 1e9))


L, B = 4096, 32
report("2->2 fp32 L=4096 B=32 (matrix)", matrix(L, B, 4, 2, 2, lambda o, i: True), L, 4 * B * L)
report("2->2 fp32 L=4096 B=32 (4-channel workaround)", workaround(L, B, 4, 2, 2), L, 4 * B * L)
L, B = 1024, 16
report("8->8 dense fp32 L=1024 B=16", matrix(L, B, 4, 8, 8, lambda o, i: True), L, 64 * B * L)
report("8->8 tridiagonal fp32 L=1024 B=16", matrix(L, B, 4, 8, 8, lambda o, i: abs(o - i) <= 1), L, 22 * B * L)
L, B = 1024, 64
report("2->2 fp64 L=1024 B=64 (matrix)", matrix(L, B, 8, 2, 2, lambda o, i: True), L, 4 * B * L)
report("2->2 fp64 L=1024 B=64 (4-channel workaround)", workaround(L, B, 8, 2, 2), L, 4 * B * L)
