"""Bank mixes on a multi-level mimo engine (bfir_engine_set_coeff_matrix_levels_pairs_bank_mix, _pairs_bank_mix_fade;
k_lbank_mix) on scripts/lbank_shape.py's shape: 64 -> 64, fp32, L = 256, levels 8 x 256, 8 x 2048, 6 x 8192 (ratios 1, 8, 4),
65536 taps per filter.  One source moves: one column, 64 filters out of 4096, per call.  Timed, plain and faded:

    pairs_bank                   one entry per pair (the yardstick, k_lbank_gather)
    pairs_bank_mix, 1 / 2 / 4    that many (entry, weight) terms per pair
    the sum on the host          the only route without the mix calls: sum w_j h_j formed in NumPy in float32, then
                                 set_coeff_matrix_levels_pairs[_fade] with the 64 sums as taps; the sum is part of the time

Two engines in one process, one with a bank of 128 filters, its twin without.  Every timed call on the bank engine is paired
with the host route for the same terms on the twin; after every pair both run the same K blocks and the outputs are compared:
byte for byte where the call names one entry at weight 1 (those runs come first, while both engines hold the same bytes), else
the largest difference relative to the largest output, which must stay within 1e-5 (the project's fp32 bound).  Wall time
of the call, alternating order, seven runs each, a warm-up of each first; nothing is written unless every comparison held.

    python scripts/lbankmix_shape.py [profiles/lbankmix_shape.txt]"""
import hashlib, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import foo_dsp_bfir_amd as bfir

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lbankmix_shape.txt")
RUNS = 7
L, TAPS, n, K, NE = 256, 65536, 64, 64, 128
BLOCKS, RATIOS = (8, 8, 6), (1, 8, 4)
WEIGHTS = {1: (1.0,), 2: (0.75, 0.25), 4: (0.4, 0.3, 0.2, 0.1)}
VARIANTS = ("bank", 1, 2, 4)
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
assert e.lbank_create(NE) == 0 and e.lbank_load(0, bank) == 0
assert e.set_bank(first) == 0
twin = bfir.BrutefirMimoLevels(L, BLOCKS, RATIOS, 4, n, n)
assert twin.set_coeff([[bank[en] for en in r] for r in first]) == 0
x = (rng.random((K * L, n), dtype=np.float32) * 2 - 1)
col = lambda c: [(o, c) for o in range(n)]
same, far = [], []


def terms(r, nt):
    return [[((17 * r + 3 * o + 1 + 11 * j) % NE, WEIGHTS[nt][j]) for j in range(nt)] for o in range(n)]


def blocks(exact):
    (rc, y), (rct, yt) = e.run(x), twin.run(x)
    assert rc == rct == 0
    if exact:
        same.append(y.tobytes() == yt.tobytes())
    else:
        far.append(float(np.abs(y - yt).max() / np.abs(yt).max()))


def timed(f):
    torch.cuda.synchronize()
    t = time.perf_counter()
    assert f() == 0
    return (time.perf_counter() - t) * 1e3


def host_route(c, tm, fade):
    """The sums on the host, then the call with taps."""
    sums = []
    for row in tm:
        h = np.float32(row[0][1]) * bank[row[0][0]]
        for en, w in row[1:]:
            h = h + np.float32(w) * bank[en]
        sums.append(h)
    return twin.fade_to_pairs(col(c), sums, K) if fade else twin.set_pairs(col(c), sums)


def one(r, v, fade):
    """Run r of variant v: column r from terms(r, .); which of the two calls goes first alternates from run to run."""
    c = r % n
    tm = terms(r, 1 if v == "bank" else v)
    if v == "bank":
        ents = [row[0][0] for row in tm]
        mine = (lambda: e.fade_to_pairs_bank(col(c), ents, K)) if fade else (lambda: e.set_pairs_bank(col(c), ents))
    else:
        mine = (lambda: e.fade_to_pairs_bank_mix(col(c), tm, K)) if fade else (lambda: e.set_pairs_bank_mix(col(c), tm))
    calls = [mine, lambda: host_route(c, tm, fade)]
    ms = [0.0, 0.0]
    for k in ((0, 1) if (r // 2) % 2 == 0 else (1, 0)):
        ms[k] = timed(calls[k])
    blocks(v in ("bank", 1))
    assert e.fade_remaining() == twin.fade_remaining() == 0
    return ms


blocks(True)
res = {(v, fade, who): [] for v in VARIANTS for fade in (False, True) for who in ("mine", "host")}
r = 0
# The calls that name one entry at weight 1 come first: until the first mix of several entries the two engines hold the same
# bytes on every level and put out the same bytes; behind it they differ by the roundings of the sums, in the stores and in
# what the levels' rings still play, and only the distance is taken.
for phase in (("bank", 1), (2, 4)):
    for rep in range(RUNS + 1):                          # the first of each is the warm-up (the first fade allocates the second set)
        for fade in (True, False):
            for v in phase:
                a, b = one(r, v, fade)
                r += 1
                if rep > 0:
                    res[(v, fade, "mine")].append(a); res[(v, fade, "host")].append(b)
assert all(same), "a one-entry call's output bytes differ from the host route's: %s" % same
assert max(far) <= 1e-5, "a mix is further from the host-formed sum than 1e-5 of the largest output: %s" % far

say("lbankmix_shape  %s  csrc %s" % (time.strftime("%Y-%m-%d"), csrc_hash()))
say("%d -> %d fp32, L = %d, levels %s x ratios %s, %d taps; one column (%d pairs) replaced per call; %d runs each, alternating; %d blocks"
    " run on both engines after every pair of calls" % (n, n, L, BLOCKS, RATIOS, TAPS, n, RUNS, K))
say("one-entry calls against the host route: %d comparisons of output bytes, all equal; mixes of 2 and 4 entries against the"
    " host-formed sum: %d comparisons, largest difference %.3g of the largest output" % (len(same), len(far), max(far)))
NAMES = {"bank": "pairs_bank (one gather)", 1: "pairs_bank_mix, 1 term", 2: "pairs_bank_mix, 2 terms", 4: "pairs_bank_mix, 4 terms"}
for fade in (False, True):
    say("the %s call itself, wall time:" % ("faded" if fade else "plain"))
    for v in VARIANTS:
        show(NAMES[v] + (", fade" if fade else ""), res[(v, fade, "mine")], "ms")
    for v in VARIANTS[1:]:
        show("host sum of %d, then pairs%s from taps" % (v, "_fade" if fade else ""), res[(v, fade, "host")], "ms")
for fade in (False, True):
    m = {v: med(res[(v, fade, "mine")]) for v in VARIANTS}
    h4 = res[(4, fade, "host")]
    say("%s: medians against pairs_bank: 1 term %.2fx, 2 terms %.2fx, 4 terms %.2fx; the host route with 4 terms against the 4-term mix"
        " %.2fx; the 4-term mix's highest run below the host route's lowest: %s"
        % ("faded" if fade else "plain", m[1] / m["bank"], m[2] / m["bank"], m[4] / m["bank"], med(h4) / m[4],
           "yes" if max(res[(4, fade, "mine")]) < min(h4) else "no"))
e.close(); twin.close()
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
open(OUT, "w").write(text)
print(text, end="")
