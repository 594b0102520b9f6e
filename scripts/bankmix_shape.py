"""Coefficient changes as bank mixes (bfir_engine_set_coeff_matrix_pairs_bank_mix, _pairs_bank_mix_fade; k_bank_mix) on
scripts/bank_shape.py's shape: a mimo engine 64 -> 64, fp32, L = 1024, B = 16, a bank of 2048 filters; one source moves: one
column, 64 filters out of 4096, every one a weighted sum of 1, 2 or 4 bank entries.  Two engines in one process:

    e      holds the bank and takes the mix calls, and the one-entry bank calls (_pairs_bank, _pairs_bank_fade) as the
           yardstick: the gather of the same library in the same session
    twin   has no bank and takes the same filters from host taps (_pairs, _pairs_fade), the sum w_1 h_1 + ... formed on the host
           in float32 inside the timed region: what a caller does today

The calls alternate (which engine goes first changes from run to run), seven runs of each kind after a warm-up of each; min /
median / max of the wall time of the call.  After every timed pair both engines run the same blocks: for the yardstick the
output bytes must be equal, for the mixes (the twin rounds the sum of the TAPS, the mix the sum of the SPECTRA) the largest
difference relative to the largest output must stay below 2e-5, twice the fp32 tolerance of the tests -- nothing is printed
unless all of that held.  Behind a mix the column is set back to single entries on both engines (not timed), so the two
stores hold the same bytes whenever the yardstick runs.  No threshold on the times: they are recorded.

    python scripts/bankmix_shape.py [profiles/bankmix_shape.txt]"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import foo_dsp_bfir_amd as bfir

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bankmix_shape.txt")
RUNS = 7
L, B, n, K, NE = 1024, 16, 64, 4, 2048
TERMS = (1, 2, 4)
rng = np.random.default_rng(1)
lines = []


def say(s):
    lines.append(s)


def show(name, v, unit):
    say("    %-52s %s   min %.3f  median %.3f  max %.3f %s" % (name, " ".join("%.3f" % f for f in v), min(v), sorted(v)[len(v) // 2], max(v), unit))


def med(v):
    return sorted(v)[len(v) // 2]


bank = [(rng.standard_normal(B * L) * (0.02 / n)).astype(np.float32) for _ in range(NE)]
e, twin = bfir.BrutefirMimo(L, B, 4, n, n), bfir.BrutefirMimo(L, B, 4, n, n)
assert e.bank_create(NE) == 0 and e.bank_load(0, bank) == 0
first = [[(o * n + i) % NE for i in range(n)] for o in range(n)]
assert e.set_coeff_bank(first) == 0
assert twin.set_coeff([[bank[en] for en in r] for r in first]) == 0
x = (rng.random((K * L, n), dtype=np.float32) * 2 - 1)
col = lambda c: [(o, c) for o in range(n)]
same, errs = [], []


def blocks(exact):
    (rc, y), (rct, yt) = e.run(x), twin.run(x)
    assert rc == rct == 0
    if exact:
        same.append(y.tobytes() == yt.tobytes())
    else:
        errs.append(float(np.abs(y.astype(np.float64) - yt).max() / np.abs(yt).max()))


def timed(f):
    torch.cuda.synchronize()
    t = time.perf_counter()
    assert f() == 0
    return (time.perf_counter() - t) * 1e3


def terms_of(r, nt):
    """Column r's 64 mixes of nt terms: neighbouring entries, weights that sum to about one with mixed magnitudes."""
    g = np.random.default_rng(1000 * nt + r)
    out = []
    for o in range(n):
        w = g.uniform(0.1, 1.0, nt)
        w = w / w.sum() * (1.0 if nt > 1 else 0.7)
        out.append([((n * r + o + 97 * j) % NE, float(w[j])) for j in range(nt)])
    return out


def one(r, nt, fade):
    """Run r: column r % n; nt = 0: the one-entry bank call against the same taps.  (ms of e's call, ms of twin's call)"""
    c = r % n
    if nt == 0:
        en = [(n * r + o) % NE for o in range(n)]
        f_e = (lambda: e.set_coeff_pairs_bank_fade(col(c), en, K)) if fade else (lambda: e.set_coeff_pairs_bank(col(c), en))

        def f_t():
            taps = [bank[k] for k in en]
            return twin.set_coeff_pairs_fade(col(c), taps, K) if fade else twin.set_coeff_pairs(col(c), taps)
    else:
        tm = terms_of(r, nt)
        f_e = (lambda: e.set_coeff_pairs_bank_mix_fade(col(c), tm, K)) if fade else (lambda: e.set_coeff_pairs_bank_mix(col(c), tm))

        def f_t():   # the sum on the host, in the engine's precision, then the call with taps
            taps = []
            for t in tm:
                h = np.float32(t[0][1]) * bank[t[0][0]]
                for en, w in t[1:]:
                    h = h + np.float32(w) * bank[en]
                taps.append(h)
            return twin.set_coeff_pairs_fade(col(c), taps, K) if fade else twin.set_coeff_pairs(col(c), taps)
    calls = [f_e, f_t]
    ms = [0.0, 0.0]
    for k in ((0, 1) if (r // 2) % 2 == 0 else (1, 0)):
        ms[k] = timed(calls[k])
    blocks(nt == 0)
    assert e.fade_remaining() == twin.fade_remaining() == 0
    if nt:   # not timed: the column back to single entries, so that the two stores hold the same bytes for the yardstick's runs
        en = [first[o][c] for o in range(n)]
        assert e.set_coeff_pairs_bank(col(c), en) == 0 and twin.set_coeff_pairs(col(c), [bank[k] for k in en]) == 0
    return ms


blocks(True)
kinds = [(nt, fade) for nt in (0,) + TERMS for fade in (True, False)]
for j, (nt, fade) in enumerate(kinds):                  # warm-up of each (the first fade allocates the second set)
    one(j, nt, fade)
res = {k: ([], []) for k in kinds}
for r in range(RUNS):
    for j, k in enumerate(kinds):
        a, b = one(len(kinds) * (r + 1) + j, *k)
        res[k][0].append(a); res[k][1].append(b)
assert all(same), "the one-entry bank call's output bytes differ from the twin's: %s" % same
assert max(errs) < 2e-5, "a mix differs from the host-formed sum by %.3g of the largest output" % max(errs)

say("%d -> %d fp32, L = %d, B = %d, a bank of %d filters; one column (%d pairs) replaced per call; %d runs each, alternating; %d blocks"
    " run on both engines after every pair of calls: %d comparisons of output bytes (one-entry calls), all equal; %d comparisons of"
    " mixes with the host-formed sum, largest difference %.2e of the largest output" % (n, n, L, B, NE, n, RUNS, K, len(same), len(errs), max(errs)))
say("the call itself, wall time; `from taps`: the sum formed on the host in float32, then the call with taps:")
for fade in (False, True):
    f = "_fade" if fade else ""
    show("pairs_bank%s (one gather, the yardstick)" % f, res[(0, fade)][0], "ms")
    show("pairs%s from taps, the same entries" % f, res[(0, fade)][1], "ms")
    for nt in TERMS:
        show("pairs_bank_mix%s, %d term%s" % (f, nt, "" if nt == 1 else "s"), res[(nt, fade)][0], "ms")
        show("pairs%s from taps, %d term%s summed on the host" % (f, nt, "" if nt == 1 else "s"), res[(nt, fade)][1], "ms")
say("medians, call with taps / mix call: " + "; ".join(
    "%s %d term%s %.2fx" % ("fade" if fade else "plain", nt, "" if nt == 1 else "s", med(res[(nt, fade)][1]) / med(res[(nt, fade)][0]))
    for fade in (False, True) for nt in TERMS))
say("the four-term mix call's highest run below the call with taps' lowest: plain %s, fade %s" % tuple(
    "yes" if max(res[(4, fade)][0]) < min(res[(4, fade)][1]) else "no" for fade in (False, True)))
say("medians, mix call / one-entry bank call: " + "; ".join(
    "%s %d term%s %.2fx" % ("fade" if fade else "plain", nt, "" if nt == 1 else "s", med(res[(nt, fade)][0]) / med(res[(0, fade)][0]))
    for fade in (False, True) for nt in TERMS))
e.close(); twin.close()
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
open(OUT, "w").write(text)
print(text, end="")
