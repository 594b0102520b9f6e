"""Generates tests/golden/kaiser_window_ref.json from the REFERENCE's own firwindow.c, compiled in place into the
untracked oracle/_ref/ (gcc -O1 -D_finite=isfinite; the source never enters the repo).

firwindow_kaiser (brutefir/firwindow.c:89-210) windows the sub-sample delay filters of the reference's delay class
(delay::sample_sinc, brutefir/delay.cpp:278-306).  Every case is one call with a non-zero offset n / steps, applied
(i) to an array of ones -- the weights alone, each applied twice as the reference applies them -- and (ii) to the sinc
samples of delay.cpp:290-302 (computed here with the C library's sin, rounded to float first for realsize 4).  Arrays
are stored as base64 of their little-endian bytes.  tests/test_delay.py checks bfir_subdelay_filter against (ii) on any
machine.

    python tests/golden/make_kaiser_golden.py <path of the reference's brutefir directory>
"""
import base64
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LENGTHS = (3, 9, 33, 63)
STEPS = (2, 10, 100)
BETAS = (9.0, 4.5)


def build(ref_dir):
    out_dir = os.path.join(ROOT, "oracle", "_ref")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libref_firwindow.so")
    subprocess.run(["gcc", "-O1", "-D_finite=isfinite", "-shared", "-fPIC", "-o", so, os.path.join(ref_dir, "firwindow.c"), "-lm"],
                   check=True)
    lib = C.CDLL(so)
    lib.firwindow_kaiser.restype = None
    lib.firwindow_kaiser.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int]
    return lib


def sinc_samples(length, offset, realsize):
    """delay.cpp:290-302"""
    h = length >> 1
    out = np.zeros(length, np.float32 if realsize == 4 else np.float64)
    for n in range(length):
        x = math.pi * (float(n - h) - offset)
        out[n] = 1.0 if x == 0.0 else math.sin(x) / x
    return out


def b64(a):
    return base64.b64encode(a.astype(a.dtype.newbyteorder("<")).tobytes()).decode()


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    lib = build(sys.argv[1])
    cases = []
    for length in LENGTHS:
        for steps in STEPS:
            for n in sorted({1, -1, steps - 1, -(steps - 1)}):
                offset = float(n) / steps   # delay.cpp:246, :255
                for beta in BETAS:
                    for realsize in (4, 8):
                        ones = np.ones(length, np.float32 if realsize == 4 else np.float64)
                        lib.firwindow_kaiser(ones.ctypes.data, length, offset, beta, realsize)
                        taps = sinc_samples(length, offset, realsize)
                        lib.firwindow_kaiser(taps.ctypes.data, length, offset, beta, realsize)
                        cases.append(dict(len=length, n=n, steps=steps, beta=beta, realsize=realsize, ones=b64(ones), sinc=b64(taps)))
    out = os.path.join(HERE, "kaiser_window_ref.json")
    json.dump(dict(source="firwindow_kaiser of brutefir/firwindow.c:89-210 compiled in place with gcc -O1 -D_finite=isfinite; "
                          "offset = n / steps; `ones`: applied to ones, `sinc`: applied to the sinc samples of "
                          "brutefir/delay.cpp:290-302; base64 of little-endian float32 (realsize 4) / float64 (realsize 8)",
                   cases=cases), open(out, "w"), indent=0)
    print("wrote", out, len(cases), "cases,", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
