"""A digest of what the coefficient calls of the uniform engines leave behind, to compare two builds of the library byte for
byte: the calls of tests/test_coeff_routes_gpu.py -- five routes to one merged set on three shapes, at once and as a fade over
three blocks -- and a diagonal set_coeff / set_coeff_fade on an L = 512, B = 3, 4-channel fp32 engine.  One sha256 per
(route, store) and per (route, output), one line each.

    python scripts/coeff_routes_digest.py                  the build in the tree (or the one BFIR_LIB_OVERRIDE names)
    python scripts/coeff_routes_digest.py compare OTHER    this build and the library OTHER, each in a fresh child process
                                                           under its own time limit; the two listings line for line
"""
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 240   # seconds per child


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def listing():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import foo_dsp_bfir_amd as bfir
    import test_coeff_routes_gpu as T
    bfir.load()
    for cid in T.SHAPES:
        P = T.plan(cid)
        for K in (None, T.FADE):
            for name in T.ROUTES:
                r = T.route(bfir, cid, P, name, K)
                tag = "%s %s %s" % (cid, "plain" if K is None else "fade%d" % K, name)
                print("%-48s store  %s" % (tag, sha(r["store"])))
                print("%-48s output %s" % (tag, sha(np.concatenate([r["before"], r["during"], r["behind"]]))))
    # the diagonal engine: a set, a plain change, a fade to a third set run to its end and past it
    L, B, Cn, K = 512, 3, 4, 3
    rng = np.random.default_rng(512)
    sets = [[(rng.standard_normal(B * L - 5) * 0.01).astype(np.float32) for c in range(Cn)] for _ in range(3)]
    x = (rng.random((12 * L, Cn), dtype=np.float32) * 2 - 1)
    e = bfir.Brutefir(L, B, 4, Cn)
    ys = []

    def step(tag, lo, hi):
        rc, y = e.run(x[lo * L:hi * L])
        assert rc == 0
        ys.append(y)
        store = np.concatenate([e.coeff_block(c, b) for c in range(Cn) for b in range(B)])
        print("%-48s store  %s" % ("diagonal-f32 " + tag, sha(store)))
        print("%-48s output %s" % ("diagonal-f32 " + tag, sha(y)))
    assert e.set_coeff(sets[0]) == 0
    step("set_coeff", 0, 3)
    assert e.set_coeff(sets[1], n_coeffs=Cn - 1, coeff_blocks=B - 1) == 0   # the last channel gets zeros
    step("set_coeff n_coeffs=3 coeff_blocks=2", 3, 5)
    assert e.set_coeff_fade(sets[2], K, n_coeffs=Cn - 1) == 0 and e.fade_remaining() == K
    step("set_coeff_fade in the fade", 5, 7)
    step("set_coeff_fade behind the fade", 7, 12)
    assert e.fade_remaining() == 0
    e.close()


def child(lib):
    env = dict(os.environ)
    env.pop("BFIR_LIB_OVERRIDE", None)
    if lib:
        env["BFIR_LIB_OVERRIDE"] = os.path.abspath(lib)
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=LIMIT, env=env)
    if p.returncode != 0:
        raise SystemExit("the listing of %s failed (%d):\n%s" % (lib or "this build", p.returncode, p.stderr[-3000:]))
    return p.stdout.splitlines()


if __name__ == "__main__":
    if len(sys.argv) == 1:
        listing()
        sys.exit(0)
    assert sys.argv[1] == "compare" and len(sys.argv) == 3, __doc__
    other, this = child(sys.argv[2]), child(None)
    diff = [(a, b) for a, b in zip(other, this) if a != b]
    for a, b in diff:
        print("DIFFERENT\n  other %s\n  this  %s" % (a, b))
    print("\n".join(this))
    print("# %d lines from each build, %s" % (len(this), "identical line for line" if not diff and len(other) == len(this) else "NOT identical"))
    sys.exit(0 if not diff and len(other) == len(this) else 1)
