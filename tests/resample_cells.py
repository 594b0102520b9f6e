"""The resampler's definition restated for its tests (include/bfir_hip.h, "sampling-rate conversion"), the cells the GPU test
runs, and the bound it applies.  Nothing here loads the library but `table`, which asks it for its own rounded taps.

Geometry is exact (Python integers and Fractions); taps are evaluated in np.longdouble where that is wider than double, else
in float64."""
import math
import os
import re
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "foo-dsp-bfir_amd", "csrc", "resample.hip")

LD = np.longdouble if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps else np.float64
PI = LD("3.141592653589793238462643383279502884") if LD is not np.float64 else np.float64(np.pi)
U = {4: 2.0 ** -24, 8: 2.0 ** -53}          # unit roundoff of the working precision / of the frame type
DTYPE = {4: np.float32, 8: np.float64}

# out_rate / in_rate = p / q as the issue writes its ratios
AUDIO_RATIOS = [(160, 147), (147, 160), (2, 1), (1, 2), (320, 147), (147, 320)]
RATIOS = AUDIO_RATIOS + [(7, 3)]


# ---- the definition -----------------------------------------------------------------------------------------------------
def geometry(in_rate, out_rate, Z, cutoff):
    """(p, q, rho, W, Wc, K) with rho and W as Fractions of the cutoff's exact double value."""
    g = math.gcd(in_rate, out_rate)
    p, q = out_rate // g, in_rate // g
    rho = min(Fraction(1), Fraction(p, q)) * Fraction(float(cutoff))
    W = Fraction(Z) / rho
    Wc = math.ceil(W)
    return p, q, rho, W, Wc, 2 * Wc


def n_out(n_in, p, q):
    return -((-n_in * p) // q)


def position(m, p, q):
    """(n0, phase) of output frame m; m a Python int or an int64 array."""
    mq = m * q
    n0 = mq // p
    return n0, mq - n0 * p


def n_in_for(n_frames_out, p, q):
    """the smallest n_in that gives this many output frames"""
    n = max(0, (n_frames_out - 1) * q // p)
    while n_out(n, p, q) < n_frames_out:
        n += 1
    assert n_out(n, p, q) == n_frames_out, (n_frames_out, p, q)
    return n


def _i0(x):
    """I_0 of an array: sum of ((x / 2)^n / n!)^2 until no term changes its sum"""
    half, total, term, n = x / LD(2), np.ones_like(x), np.ones_like(x), LD(1)
    while True:
        term = term * half / n
        nxt = total + term * term
        if np.all(nxt == total):
            return nxt
        total, n = nxt, n + LD(1)


def model_taps(in_rate, out_rate, Z, beta, cutoff, gain):
    """[p, K]: every tap of every phase in LD."""
    p, q, rho, W, Wc, K = geometry(in_rate, out_rate, Z, cutoff)
    num = (Wc - 1 - np.arange(K, dtype=np.int64))[None, :] * p + np.arange(p, dtype=np.int64)[:, None]
    u = num.astype(LD) / LD(p)
    rho_l = (LD(p) / LD(q) if p < q else LD(1)) * LD(float(cutoff))
    W_l = LD(Z) / rho_l
    inside = np.abs(u) < W_l
    x = PI * rho_l * u
    safe = np.where(x == 0, LD(1), x)
    sinc = np.where(x == 0, LD(1), np.sin(safe) / safe)
    r = np.where(inside, u / W_l, LD(0))
    win = _i0(LD(beta) * np.sqrt(LD(1) - r * r)) / _i0(np.array([LD(beta)]))[0]
    return np.where(inside, LD(gain) * rho_l * sinc * win, LD(0))


def table(bfir, cell):
    """[p, K] of the library's own taps, in the cell's working precision"""
    p = geometry(cell["in_rate"], cell["out_rate"], cell["Z"], cell["cutoff"])[0]
    return np.stack([bfir.resample_filter(cell["in_rate"], cell["out_rate"], ph, cell["Z"], cell["beta"], cell["cutoff"],
                                          cell["gain"], cell["s"]) for ph in range(p)])


def gather(x, frames, p, q, Wc):
    """[len(frames), K, C]: the input samples each output frame's taps meet, zero outside the input; and the phases."""
    frames = np.asarray(frames, dtype=np.int64)
    n0, phase = position(frames, p, q)
    idx = (n0 - Wc + 1)[:, None] + np.arange(2 * Wc, dtype=np.int64)[None, :]
    ok = (idx >= 0) & (idx < x.shape[0])
    return np.where(ok[:, :, None], x[np.clip(idx, 0, x.shape[0] - 1)], 0), phase


def reference(T, x, frames, p, q, Wc):
    """The direct form of the taps T on frames `frames` in LD, and sum |T_j| |x_j| beside it: (ref, amp), [len(frames), C]."""
    frames = np.asarray(frames, dtype=np.int64)
    ref, amp = np.zeros((frames.size, x.shape[1]), LD), np.zeros((frames.size, x.shape[1]), LD)
    step = max(1, (1 << 21) // (2 * Wc * x.shape[1]))            # a couple of million products at a time
    for a in range(0, frames.size, step):
        X, phase = gather(x, frames[a:a + step], p, q, Wc)
        Tm = T[phase].astype(LD)[:, :, None]
        X = X.astype(LD)
        ref[a:a + step] = (Tm * X).sum(axis=1)
        amp[a:a + step] = (np.abs(Tm) * np.abs(X)).sum(axis=1)
    return ref, amp


def bound(s, K, ref, amp):
    """(K + 2) u_R sum |T_j| |x_j| + u_F |ref|: K fused multiply-adds in working precision, the source widened exactly, the
    sum rounded once to the frame type (frames have the working precision's width: u_F = u_R)."""
    return ((K + 2) * U[s] * amp + U[s] * np.abs(ref)).astype(np.float64)


def emulate(T, x, frames, p, q, Wc, s, drop_last=False, shift=0, step=None):
    """k_resample in working precision on the CPU: taps j ascending, one multiply-add per tap.  fp32: the product of two floats
    is exact in double and its sum with a float is rounded to float from there; fp64: multiply, then add.  The mutations:
    drop_last leaves out tap K - 1, shift moves the window's first frame, step = p advances the position by p / p input frames
    per output frame instead of q / p."""
    R = DTYPE[s]
    K = 2 * Wc
    n0, phase = position(np.asarray(frames, dtype=np.int64), p, q if step is None else step)
    idx = (n0 - Wc + 1 + shift)[:, None] + np.arange(K, dtype=np.int64)[None, :]
    ok = (idx >= 0) & (idx < x.shape[0])
    X = np.where(ok[:, :, None], x[np.clip(idx, 0, x.shape[0] - 1)], 0).astype(R)
    Tm = T[phase].astype(R)
    acc = np.zeros((len(frames), x.shape[1]), R)
    for j in range(K - (1 if drop_last else 0)):
        if R is np.float32:
            acc = (Tm[:, j, None].astype(np.float64) * X[:, j].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
        else:
            acc = Tm[:, j, None] * X[:, j] + acc
    return acc


# ---- the kernel's launch geometry, restated from the constants of csrc/resample.hip ----------------------------------------
def limits():
    src = open(SOURCE).read()
    grab = lambda name: re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, src).group(1)
    num = lambda t: int(eval(re.sub(r"(\d+)L\b", r"\1", t)))
    return {"tile": num(grab("kResTile")), "lds": num(grab("kResLds")), "max_taps": num(grab("kResMaxTaps")),
            "max_table": num(grab("kResMaxTable"))}


def source_instances():
    """the (R, F) pairs of k_resample the source launches"""
    src = open(SOURCE).read()
    return set(re.findall(r"hipLaunchKernelGGL\(\(k_resample<(\w+), (\w+)>\)", src))


def out_bytes(tile, C, s):
    return (tile * C * s + 15) & ~15


def width(tile, p, q, K):
    return (tile * q + p - 1) // p + K


def tile_of(p, q, K, C, s, lim=None):
    lim = lim or limits()
    tile = lim["tile"]
    while tile > 1 and out_bytes(tile, C, s) + width(tile, p, q, K) * s > lim["lds"]:
        tile >>= 1
    return tile


def lds_of(p, q, K, C, s, lim=None):
    t = tile_of(p, q, K, C, s, lim)
    return out_bytes(t, C, s) + width(t, p, q, K) * s


# ---- the cells --------------------------------------------------------------------------------------------------------------
def _cell(cid, ratio, s, C, Z=16, beta=9.0, cutoff=0.95, gain=1.0, n_in=None, tiles=None, **kw):
    """ratio = (out, in).  n_in, or `tiles` = (a, b): n_out = a * tile + b frames."""
    c = dict(id="%s-s%d" % (cid, s), out_rate=ratio[0], in_rate=ratio[1], s=s, C=C, Z=Z, beta=beta, cutoff=cutoff, gain=gain, **kw)
    p, q, _, _, Wc, K = geometry(c["in_rate"], c["out_rate"], Z, cutoff)
    c.update(p=p, q=q, Wc=Wc, K=K, tile=tile_of(p, q, K, C, s), instance=("float", "float") if s == 4 else ("double", "double"))
    c["n_in"] = n_in if tiles is None else n_in_for(tiles[0] * c["tile"] + tiles[1], p, q)
    c["n_out"] = n_out(c["n_in"], p, q)
    return c


def _cells():
    out = []
    for s in (4, 8):
        out.append(_cell("a-all-edge", (160, 147), s, 3, n_in=5))
        for name, tiles in (("one-tile", (1, 0)), ("one-tile-plus-1", (1, 1)), ("three-tiles-minus-1", (3, -1))):
            out.append(_cell("b-up-" + name, (160, 147), s, 2, Z=32, tiles=tiles))
            out.append(_cell("b-down-" + name, (147, 160), s, 2, beta=0.0, tiles=tiles))
        out.append(_cell("d-two-taps", (3, 2), s, 2, Z=1, beta=0.0, cutoff=1.0, n_in=700))
        # no whole number of 16-byte units (8 channels always are one); run_device with both pointers off a 16-byte boundary by
        # `offset` bytes: 4 for float frames, the sample's own 8 for double frames (4 would not be a pointer to a double)
        for C in (1, 3, 8):
            out.append(_cell("h-unaligned-C%d" % C, (160, 147), s, C, n_in=300, offset=4 if s == 4 else 8))
    out.append(_cell("c-largest-window", (1, 8), 8, 8, Z=128, cutoff=0.5, tiles=(2, 0)))
    # the same window over a span twice as wide per output frame: a whole tile's request does not fit, the tile is halved;
    # and a tile of 8 (most lanes only stage)
    out.append(_cell("c-halved-tile", (1, 16), 8, 8, Z=64, cutoff=0.5, tiles=(2, 1)))
    out.append(_cell("c-small-tile", (1, 1000), 4, 2, Z=2, cutoff=1.0, tiles=(2, 1)))
    return out


CELLS = _cells()
# the impulse cells: one unit sample at frame k of channel 1, noise at 1/8 amplitude in the other two
IMPULSE_CELLS = [_cell("e-impulse-%d-%d" % r, r, s, 3, n_in=600, k=300) for r in ((320, 147), (147, 320)) for s in (4, 8)]
# 64-bit indices: (n_out - 1) q >= 2^32
_BIG_OUT = -(-(1 << 32) // 320) + 1 + 700
BIG_CELL = _cell("f-64-bit", (147, 320), 4, 1, n_in=n_in_for(_BIG_OUT, 147, 320))
FILTERED = CELLS + IMPULSE_CELLS + [BIG_CELL]


def audio(cell):
    """the cell's input frames: uniform noise in [-1, 1) in the frame type, the same on every machine"""
    rng = np.random.default_rng(sum(map(ord, cell["id"])))
    return (rng.random((cell["n_in"], cell["C"])) * 2.0 - 1.0).astype(DTYPE[cell["s"]])
