"""The transform-size matrix: one row per (kernel family, realsize, L) the engine supports, the channel count, frame
formats and switches that make the engine take that family, and what its creation log line must then report.

Plain data, importable without a GPU: tests/test_size_matrix.py checks on the CPU that CELLS covers exactly the set
the sources in csrc/ support; tests/test_size_matrix_gpu.py runs every row on the device."""
import os
import re

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "foo-dsp-bfir_amd", "csrc")

FLOAT_LE, FLOAT64_LE = 8, 10

# every switch that can move an engine to another family: a cell sets each of them, to a value or to None (unset)
PATH_SWITCHES = ("BFIR_PAIR", "BFIR_PAIR_TIME", "BFIR_DIRECT", "BFIR_RUN64", "BFIR_F64_PAIRS", "BFIR_MAC_SYS",
                 "BFIR_MAC_BATCHED")

B = 3                     # partitions; taps = B*L - 7 (ragged last partition)
RAGGED = 7


# ---- what the sources support -----------------------------------------------------------------------------------
def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _macro_list(src, name):
    m = re.search(r"#define\s+%s\(F\)\s*\\?\s*((?:F\(\d+\)\s*)+)" % name, src)
    assert m, name
    return [int(v) for v in re.findall(r"F\((\d+)\)", m.group(1))]


def _const(src, name):
    m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, src)
    assert m, name
    return int(m.group(1))


def source_limits():
    """The size lists and limits in csrc/ that decide which kernels an engine of size L can run."""
    k, p = _read("kernels.hip"), _read("pair.hip")
    lds = re.search(r"filter_length\s*/\s*32\)\s*\*\s*2\s*\*\s*\(size_t\)realsize\s*>\s*(\d+)\s*\*\s*1024", k)
    run_max = re.search(r"bool run64_supported\(.*?filter_length <= (\d+);", k, re.S)
    assert lds and run_max
    return {
        "log2m": _macro_list(k, "BFIR_FOR_LOG2M"),
        "pair_log2n": _macro_list(p, "BFIR_FOR_PAIR_LOG2N"),
        "run64_min_log2m": _const(k, "BFIR_RUN64_MIN_LOG2M"),
        "run64_max_len": int(run_max.group(1)),
        "pairs64_max_log2m": _const(k, "BFIR_PAIRS64_MAX_LOG2M"),
        "lds_bytes": int(lds.group(1)) * 1024,
    }


def supported_lengths(lim, s):
    """Partition lengths L an engine of realsize s accepts: one transform of L complex points must fit the LDS bound."""
    return [1 << lg for lg in lim["log2m"] if ((1 << lg) + (1 << lg) // 32) * 2 * s <= lim["lds_bytes"]]


def refused_lengths(lim, s):
    """Powers of two next to the supported range, and sizes of the list that the LDS bound refuses."""
    out = [1 << (min(lim["log2m"]) - 1), 1 << (max(lim["log2m"]) + 1)]
    return sorted(set(out) | {1 << lg for lg in lim["log2m"]} - set(supported_lengths(lim, s)))


def supported_set(lim):
    """{(family, realsize, L)} the build supports (the engine's choice in engine.hip, bfir_engine_create_batch)."""
    f32, f64 = supported_lengths(lim, 4), supported_lengths(lim, 8)
    pair = [1 << (n - 1) for n in lim["pair_log2n"]]               # the pair plans are 2L points
    run_lo = 1 << lim["run64_min_log2m"]
    run = [L for L in f64 if run_lo <= L <= lim["run64_max_len"]]
    run_pairs = [L for L in run if L <= 1 << lim["pairs64_max_log2m"]]
    fams = {
        "staging_grouped": (4, [L for L in f32 if 2 * L < 512]),     # fp32 spectra are (re, im) pairs from N = 512
        "staging_pairs": (4, [L for L in f32 if 2 * L >= 512]),
        "direct_one": (4, f32),
        "direct_mixed": (4, f32),
        "pair": (4, pair),
        "time_pair": (4, pair),
        "staging64": (8, f64),
        "direct64": (8, f64),
        "run64_pairs": (8, run_pairs),
        "run64_grouped": (8, run),
        "plugin": (8, f64),
    }
    return {(f, s, L) for f, (s, Ls) in fams.items() for L in Ls}


# ---- the matrix ---------------------------------------------------------------------------------------------------
def _cell(family, s, L, C, fin, fout, env, path, layout, run):
    e = {k: None for k in PATH_SWITCHES}
    e.update(env)
    sw = "".join("-%s=%s" % (k[5:], v) for k, v in sorted(env.items()))
    return {"id": "%s-s%d-L%d-C%d-%d.%d%s" % (family, s, L, C, fin, fout, sw), "family": family, "s": s, "L": L, "C": C,
            "in_fmt": fin, "out_fmt": fout, "env": e, "path": path, "layout": layout, "run": run}


def _build_cells():
    F32 = [1 << lg for lg in range(4, 15)]
    F64 = [1 << lg for lg in range(4, 14)]
    PAIR = [512, 1024, 2048, 4096, 8192]
    cells = []
    add = lambda *a: cells.append(_cell(*a))
    for L in F32:
        lay = "pairs" if L >= 256 else "grouped"
        if L < 256:                   # grouped spectra: float frames of three channels go through the staging kernels
            add("staging_grouped", 4, L, 3, FLOAT_LE, FLOAT_LE, {}, "staging", "grouped", "off")
        else:                         # BFIR_PAIR=0 also turns off direct mode; 256 / 16384 have no pair kernels at all
            add("staging_pairs", 4, L, 2, FLOAT_LE, FLOAT_LE, {"BFIR_PAIR": 0}, "staging", "pairs", "off")
            if L not in PAIR:
                add("staging_pairs", 4, L, 2, FLOAT_LE, FLOAT_LE, {}, "staging", "pairs", "off")
                add("staging_pairs", 4, L, 3, FLOAT_LE, FLOAT_LE, {}, "staging", "pairs", "off")
        # one channel: contiguous samples, direct mode (the time-pair kernels would take it at the pair sizes)
        add("direct_one", 4, L, 1, FLOAT_LE, FLOAT_LE, {"BFIR_PAIR_TIME": 0}, "direct", lay, "off")
        # float / double frames around fp32 arithmetic: direct mode with a double-frame side (the pair path needs
        # FLOAT_LE on both sides).  Two channels per workgroup (CPW = 2) never occur on fp32 engines: they need the
        # grouped layout (k_fwd / k_inv: !il) and fp32 engines keep (re, im) pairs from 256 points, while CPW = 2 needs
        # 64 threads per transform (1024 points and up).
        add("direct_mixed", 4, L, 2, FLOAT_LE, FLOAT64_LE, {"BFIR_DIRECT": 1}, "direct", lay, "off")
        add("direct_mixed", 4, L, 2, FLOAT64_LE, FLOAT_LE, {"BFIR_DIRECT": 1}, "direct", lay, "off")
    for L in PAIR:
        for C in (2, 8):
            add("pair", 4, L, C, FLOAT_LE, FLOAT_LE, {}, "pair", "pairs", "off")
        for C in (1, 3):
            add("time_pair", 4, L, C, FLOAT_LE, FLOAT_LE, {}, "time-pair", "pairs", "off")
    for L in F64:
        run = 1024 <= L <= 8192
        add("staging64", 8, L, 3, FLOAT_LE, FLOAT_LE, {"BFIR_DIRECT": 0}, "staging", "grouped", "off")
        for C in (2, 3):              # one transform per workgroup (CPW = 2 with C = 2 where direct_stereo_fits<double>),
            # double and float frames
            add("direct64", 8, L, C, FLOAT64_LE, FLOAT64_LE, {"BFIR_RUN64": 0}, "direct", "grouped", "off")
            add("direct64", 8, L, C, FLOAT_LE, FLOAT_LE, {"BFIR_RUN64": 0, "BFIR_DIRECT": 1}, "direct", "grouped", "off")
        if 1024 <= L <= 4096:
            for C in (2, 3):
                add("run64_pairs", 8, L, C, FLOAT64_LE, FLOAT64_LE, {}, "direct", "pairs", "on")
        if run:
            for C in (2, 3):
                add("run64_grouped", 8, L, C, FLOAT64_LE, FLOAT64_LE, {"BFIR_F64_PAIRS": 0}, "direct", "grouped", "on")
            add("run64_grouped", 8, L, 3, FLOAT_LE, FLOAT_LE, {"BFIR_F64_PAIRS": 0}, "direct", "grouped", "on")
        # the plug-in's shape: fp64 arithmetic, float32 stereo frames -- staging below the run kernels' sizes except
        # where two channels per workgroup fit (none below 1024 points)
        for C in (2, 3):              # odd channel counts: the run kernels on float frames also where CPW = 2 fits
            add("plugin", 8, L, C, FLOAT_LE, FLOAT_LE, {}, "direct" if run else "staging",
                "pairs" if 1024 <= L <= 4096 else "grouped", "on" if run else "off")
    return cells


CELLS = _build_cells()

# creation must fail: (realsize, L, error name in foo_dsp_bfir_amd._lib)
REFUSALS = [(8, 16384, "ERR_UNSUPPORTED"), (4, 8, "ERR_UNSUPPORTED"), (8, 8, "ERR_UNSUPPORTED"),
            (4, 32768, "ERR_UNSUPPORTED"), (8, 32768, "ERR_UNSUPPORTED")]


# ---- test data and the float64 reference ------------------------------------------------------------------------
def flat_ir(rng, channels, taps):
    """Distinct float64 impulse responses with a flat envelope (every partition, the ragged tail included, carries
    the weight of the first), sum |h| = 1 per channel.  oracle.synth_ir decays by e^-6 over the taps instead."""
    out = []
    for _ in range(channels):
        h = rng.uniform(-1.0, 1.0, taps)
        out.append(h / np.abs(h).sum())
    return out


def amplitudes(n_blocks, L, C, time_pairs):
    """[frames, C] gains: within each channel pair the odd channel runs at 1/8; with time pairs, odd blocks too."""
    g = np.ones((n_blocks * L, C))
    g[:, 1::2] = 0.125
    if time_pairs:
        g = np.ones((n_blocks * L, C))
        for t in range(1, n_blocks, 2):
            g[t * L:(t + 1) * L] = 0.125
    return g


FFT_CONV_ABOVE = 4e7      # n_x * n_h above which the float64 FFT convolution replaces the long-double direct form


def fft_conv(x, h):
    """Linear convolution of float64 x and h, first x.size outputs, by float64 FFT."""
    import scipy.fft
    x, h = np.asarray(x, np.float64), np.asarray(h, np.float64)
    n = scipy.fft.next_fast_len(x.size + h.size - 1, real=True)
    return scipy.fft.irfft(scipy.fft.rfft(x, n) * scipy.fft.rfft(h, n), n)[:x.size]


def reference_conv(orc, x, h):
    """High-precision y = x * h: the oracle's long-double direct form where that is cheap, float64 FFT above."""
    if x.size * h.size <= FFT_CONV_ABOVE:
        return orc.direct_conv(x, h)
    return fft_conv(x, h)


def grouped_spectrum(taps_block, L, scale):
    """The reference's partition spectrum (coeffs2cbuf): R2HC of [0 .. 0 | taps * scale] over N = 2L reals, times
    1/N, in the grouped layout (bins four at a time: 4 re | 4 im, Re X_{N/2} in the slot of Im X_0), float64."""
    N = 2 * L
    r = np.zeros(N)
    r[L:L + taps_block.size] = np.asarray(taps_block, np.float64) * scale
    X = np.fft.rfft(r) / N
    out = np.concatenate([X[:L].real.reshape(-1, 4), X[:L].imag.reshape(-1, 4)], axis=1).ravel()
    out[4] = X[L].real
    return out


def halfcomplex(X, n):
    """FFTW half-complex order of the rfft X of n reals: Re X_0 .. Re X_{n/2}, Im X_{n/2-1} .. Im X_1."""
    out = np.empty(n)
    out[:n // 2 + 1] = X.real
    out[n // 2 + 1:] = X.imag[1:n // 2][::-1]
    return out


def hc2r(hc):
    """FFTW_HC2R (unnormalised inverse) of half-complex hc in float64, from the definition's rfft form."""
    hc = np.asarray(hc, np.float64)
    n = hc.size
    X = np.zeros(n // 2 + 1, complex)
    X.real = hc[:n // 2 + 1]
    X.imag[1:n // 2] = hc[n // 2 + 1:][::-1]
    return np.fft.irfft(X, n) * n
