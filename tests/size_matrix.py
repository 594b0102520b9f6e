"""The transform-size matrix: one row per (kernel family, realsize, L) the engine supports, the channel count, frame
formats and switches that make the engine take that family, and what its creation log line must then report.

NUP_CELLS, FADE_CELLS, MATRIX_CELLS, LEVELS_CELLS, LFADE_CELLS, MLEVELS_CELLS and MFADE_CELLS are the same for the engine
kinds built on top of the plain diagonal engine: two-level engines (csrc/nup.hip and the tail level in engine.hip),
crossfaded coefficient changes (csrc/fade.hip), matrix engines (csrc/matrix.hip), multi-level engines (csrc/levels.hip),
crossfaded coefficient changes on two-level and multi-level engines (csrc/lfade.hip), multi-level matrix engines
(csrc/mlevels.hip) and their crossfades (csrc/mfade.hip).

DELAY_SUB_CELLS, DELAY_MID_CELLS, DELAY_COPY_CELLS and DELAY_KIND_CELLS are the matrix of the per-channel delays
(csrc/delay.hip): every instance, tile shape and history edge of k_delay_sub and k_delay_copy, on every kind of engine
(tests/test_delay_matrix.py on the CPU, tests/test_delay_matrix_gpu.py on the device).

Plain data, importable without a GPU: tests/test_size_matrix.py checks on the CPU that the lists cover exactly the set
the sources in csrc/ support; tests/test_size_matrix_gpu.py and tests/test_size_matrix_kinds_gpu.py run every row on
the device."""
import os
import re
import zlib

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "foo-dsp-bfir_amd", "csrc")

FLOAT_LE, FLOAT64_LE = 8, 10

# every switch that can move an engine to another family: a cell sets each of them, to a value or to None (unset)
# (BFIR_MFADE_DUO, read at creation: unset is the default, k_mac_duo; 0 runs k_mac_matrix twice)
PATH_SWITCHES = ("BFIR_PAIR", "BFIR_PAIR_TIME", "BFIR_DIRECT", "BFIR_RUN64", "BFIR_F64_PAIRS", "BFIR_MAC_SYS",
                 "BFIR_MAC_BATCHED", "BFIR_MFADE_DUO")

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
    k, p, kh = _read("kernels.hip"), _read("pair.hip"), _read("kernels.h")
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
        "nup_log2n": _macro_list(_read("nup.hip"), "BFIR_FOR_NUP_LOG2N"),
        "fade_log2n": _macro_list(_read("fade.hip"), "BFIR_FOR_FADE_LOG2N"),
        "mat_small_max": _const(kh, "BFIR_MAT_SMALL_MAX"),
        "levels_log2n": _macro_list(_read("levels.hip"), "BFIR_FOR_LEVELS_LOG2N"),
        "lfade_log2n": _macro_list(_read("lfade.hip"), "BFIR_FOR_LFADE_LOG2N"),
        "level_rings": _const(kh, "BFIR_LEVEL_RINGS"),
        "lone_log2n": _macro_list(_read("mlevels.hip"), "BFIR_FOR_LONE_LOG2N"),
        "max_levels": _max_levels(),
    }


def _max_levels():
    """BFIR_MAX_LEVELS of the public header."""
    with open(os.path.join(os.path.dirname(os.path.dirname(CSRC)), "include", "bfir_hip.h")) as f:
        m = re.search(r"#define\s+BFIR_MAX_LEVELS\s+(\d+)", f.read())
    assert m
    return int(m.group(1))


def reachable_instances(lim, log2n, nr_min):
    """{(LOG2N, NR)} of k_inv_levels (nr_min = 2: one ring of a non-fading chunk is k_inv_nup's), k_inv_lfade (nr_min = 1) or
    k_inv_lone (nr_min = 0: the chunks before any level contributes) that an engine can launch, and the instances the
    sources build.  NR counts the contributing tails; bfir_engine_create_levels wants ratios >= 2 and every L_k supported, so
    NR tails on a head of L = 2^(LOG2N - 1) need 2^(LOG2N - 1) 2^NR <= the largest supported fp32 length."""
    top = max(supported_lengths(lim, 4))
    built = {(lg, nr) for lg in log2n for nr in range(nr_min, lim["level_rings"] + 1)}
    return {(lg, nr) for lg, nr in built if (1 << (lg - 1)) << nr <= top}, built


def fade_fused_rule():
    """The right-hand side of `e->fade_fused = ...;` in engine.hip: which engines k_inv_fade serves."""
    m = re.search(r"e->fade_fused\s*=\s*([^;]+);", _read("engine.hip"))
    assert m
    return " ".join(m.group(1).split())


def fade_is_fused(lim, s, L, out_fmt):
    """fade_fused_rule() restated: fp32 spectra kept as (re, im) pairs (2L >= 512: choose_path), FLOAT_LE output frames
    and a pair plan of 2L points (pair_supported)."""
    return s == 4 and 2 * L >= 512 and out_fmt == FLOAT_LE and L in [1 << (n - 1) for n in lim["pair_log2n"]]


def back_fused_rule():
    """The right-hand side of `e->back_fused = ...;` in engine.hip: which split engines take the fused back ends."""
    m = re.search(r"e->back_fused\s*=\s*([^;]+);", _read("engine.hip"))
    assert m
    return " ".join(m.group(1).split())


def matrix_back_is_fused(lim, s, L, out_fmt):
    """back_fused_rule() restated for a matrix head: by its output side alone, the conditions of fade_is_fused -- whatever
    the input count, the input format or the parity of the output count."""
    return fade_is_fused(lim, s, L, out_fmt)


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
        # two-level engines: the head's L with a tail of 2L (the smallest ratio) that the level below takes as well; the
        # fused back end where k_inv_nup has an instance of 2L points
        "nup_fused": (4, [1 << (n - 1) for n in lim["nup_log2n"]]),
        "nup_general32": (4, [L for L in f32 if 2 * L in f32]),
        "nup_general64": (8, [L for L in f64 if 2 * L in f64]),
        "fade_fused": (4, [1 << (n - 1) for n in lim["fade_log2n"]]),
        "fade_general32": (4, f32),
        "fade_general64": (8, f64),
        "matrix32": (4, f32),
        "matrix64": (8, f64),
        # multi-level engines: the head's L with three levels of ratio 2 (the smallest) that the precision takes; the fused
        # back end where k_inv_levels has an instance of 2L points
        "levels_fused": (4, [L for L in [1 << (n - 1) for n in lim["levels_log2n"]] if 4 * L in f32]),
        "levels_general32": (4, [L for L in f32 if 4 * L in f32]),
        "levels_general64": (8, [L for L in f64 if 4 * L in f64]),
        # fades on split engines: from two levels (a tail of 2L) up
        "lfade_fused": (4, [L for L in [1 << (n - 1) for n in lim["lfade_log2n"]] if 2 * L in f32]),
        "lfade_general32": (4, [L for L in f32 if 2 * L in f32]),
        "lfade_general64": (8, [L for L in f64 if 2 * L in f64]),
        # multi-level matrix engines and their fades, from two levels up: the fused back end where the head has a pair plan
        # (k_inv_nup / k_inv_levels / k_inv_lone, k_inv_lfade), the general one at every head that takes a tail
        "mlevels_fused": (4, [L for L in pair if 2 * L in f32]),
        "mlevels_general32": (4, [L for L in f32 if 2 * L in f32]),
        "mlevels_general64": (8, [L for L in f64 if 2 * L in f64]),
        "mfade_fused": (4, [L for L in pair if 2 * L in f32]),
        "mfade_general32": (4, [L for L in f32 if 2 * L in f32]),
        "mfade_general64": (8, [L for L in f64 if 2 * L in f64]),
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


# ---- the engine kinds on top of the plain diagonal engine ---------------------------------------------------------------
# Same recipe as above for all of them: flat_ir filters (a distinct one per channel or per (output, input) pair) cast to the
# working precision, uniform noise with the odd channels (inputs) at 1/8, the float64 / long-double reference, the
# per-block, per-channel norm of block_errors and the tolerance of tolerance() -- the project's own, nothing new.
def _kind_cell(family, s, L, C, fin, fout, tag, **more):
    cell = {"id": "%s-s%d-L%d-C%d-%d.%d%s" % (family, s, L, C, fin, fout, tag), "family": family, "s": s, "L": L, "C": C,
            "in_fmt": fin, "out_fmt": fout, "env": {k: None for k in PATH_SWITCHES}}
    cell.update(more)
    return cell


def _nup_cell(family, s, L, C, fin, fout, back, r=2, Bt=2):
    """Bh = r; taps end RAGGED short of the last tail partition; nb blocks make the tail's delay line and its time ring
    wrap (tests/test_nup_gpu.py: nb >= Bh + r (Bt + 2) + 3)."""
    Bh = r
    return _kind_cell(family, s, L, C, fin, fout, "-r%dx%d" % (r, Bt), Bh=Bh, r=r, Bt=Bt, back=back,
                      taps=Bh * L + (Bt - 1) * r * L + r * L - RAGGED, nb=Bh + r * (Bt + 2) + 3)


def _build_nup_cells():
    cells = []
    add = lambda *a, **k: cells.append(_nup_cell(*a, **k))
    for L in (512, 1024, 2048, 4096, 8192):       # k_inv_nup: fp32, float frames, an even channel count
        for C in (2, 8):
            add("nup_fused", 4, L, C, FLOAT_LE, FLOAT_LE, "fused")
    add("nup_fused", 4, 512, 2, FLOAT_LE, FLOAT_LE, "fused", r=32, Bt=1)      # a large ratio: tail partitions of 16384
    for L in [1 << lg for lg in range(4, 14)]:    # k_nup_combine<float>: an odd count anywhere, any count below the pair plans
        add("nup_general32", 4, L, 3, FLOAT_LE, FLOAT_LE, "general")
        if L < 512:
            add("nup_general32", 4, L, 2, FLOAT_LE, FLOAT_LE, "general")
    for L in [1 << lg for lg in range(4, 13)]:    # k_nup_combine<double>
        for C in (2, 3):
            add("nup_general64", 8, L, C, FLOAT64_LE, FLOAT64_LE, "general")
        if L in (64, 1024, 4096):                 # the plug-in's shape: fp64 arithmetic, float32 stereo frames
            add("nup_general64", 8, L, 2, FLOAT_LE, FLOAT_LE, "general")
    return cells


FADE_K = 3                # blocks of the fade; with chunks of 2 it is cut into 2 + 1, so the second part starts at m0 = 2L


def _build_fade_cells():
    """B partitions, ragged taps; t0 = B + 1 blocks, the fade, K + B + 2 more.  The new set has 1/8 of the old set's gain
    in half of the cells and 8 times in the other half (gains (1, 1/8) and (1/8, 1): the loud set is the same size in
    both), so a leak between the halves of Z = Y_old + i Y_new shows at either end of the ramp."""
    cells = []

    def add(family, s, L, C, fin, fout):
        lg = L.bit_length() - 1
        new_gain = 0.125 if (lg + C) % 2 == 0 else 8.0
        cells.append(_kind_cell(family, s, L, C, fin, fout, "-g%g" % new_gain, new_gain=new_gain, t0=B + 1,
                                nb=B + 1 + FADE_K + B + 2, taps=B * L - RAGGED))
    for L in (512, 1024, 2048, 4096, 8192):       # k_inv_fade: channel pairs and pairs in time
        for C in (2, 3):
            add("fade_fused", 4, L, C, FLOAT_LE, FLOAT_LE)
    for L in (16, 32, 64, 128, 256, 16384):       # k_fade_blend<float>: outside the pair plans
        for C in (2, 3):
            add("fade_general32", 4, L, C, FLOAT_LE, FLOAT_LE)
    for L in (512, 1024, 2048, 4096, 8192):       # ... and inside them where the output frames are not FLOAT_LE
        add("fade_general32", 4, L, 2, FLOAT_LE, FLOAT64_LE)
    for L in [1 << lg for lg in range(4, 14)]:    # k_fade_blend<double>
        add("fade_general64", 8, L, 2, FLOAT64_LE, FLOAT64_LE)
        if L in (64, 1024, 4096):
            add("fade_general64", 8, L, 3, FLOAT_LE, FLOAT_LE)
    return cells


MATRIX_CALLS = (3, 11)    # blocks per call: the one-block-per-lane MAC (<= BFIR_MAT_SMALL_MAX), then time tiles 8 + 3 / 4 + 4 + 3


def _build_matrix_cells():
    """B partitions, ragged taps, one NULL filter; every matrix engine here is in direct mode (an odd count on one side, or
    fp64)."""
    cells = []

    def add(family, s, L, n_in, n_out, fmt):
        lg = L.bit_length() - 1
        layout = "pairs" if (L >= 256 if s == 4 else 1024 <= L <= 4096) else "grouped"
        cells.append(_kind_cell(family, s, L, n_in, fmt, fmt, "-to%d" % n_out, n_in=n_in, n_out=n_out,
                                null=(lg % n_out, lg % n_in), path="direct", layout=layout, nb=sum(MATRIX_CALLS),
                                taps=B * L - RAGGED))
    for L in [1 << lg for lg in range(4, 15)]:
        add("matrix32", 4, L, 2, 3, FLOAT_LE)     # an output tile of 4 with one row unused
        if L in (16, 256, 4096):
            add("matrix32", 4, L, 3, 5, FLOAT_LE)  # two output tiles, the second ragged
    for L in [1 << lg for lg in range(4, 14)]:
        add("matrix64", 8, L, 2, 3, FLOAT64_LE)   # output tiles of 2, the second ragged
        if L == 1024:
            add("matrix64", 8, L, 2, 2, FLOAT_LE)
    return cells


# Multi-level engines (csrc/levels.hip) and fades on two-level and multi-level engines (csrc/lfade.hip): the smallest
# geometry bfir_engine_create_levels accepts, ratios of 2 throughout and every D_k = L_k, so a cell costs as little as its
# transform sizes allow.  Two levels are BrutefirNup(L, 2, 2, 2).
LEVEL_BLOCKS = {2: (2, 2), 3: (2, 1, 2), 4: (2, 1, 1, 2)}


def level_geometry(L, blocks, ratios):
    """([L_k], [D_k] with D_n = capacity appended) in samples."""
    Ls, D = [], [0]
    for b, r in zip(blocks, ratios):
        Ls.append(L if not Ls else Ls[-1] * r)
        D.append(D[-1] + b * Ls[-1])
    return Ls, D


def _levels_cell(family, s, L, C, fin, fout, n, fade=None, K=FADE_K, pre="", post="", **extra):
    """n levels; taps end RAGGED short of the capacity (the last level's last partition is ragged).  Without a fade,
    nb = D_last / L + r_last (blocks_last + 2) + 3 blocks: the deepest delay line and its ring both wrap.  With one (fade,
    added to lg + C in the gain rule of FADE_CELLS) it starts at t0 = D_last / L + r_last + 1, where every ring contributes
    (NR of k_inv_lfade = n - 1) and which is odd, so inside a block of every level: every level catches up; K = FADE_K blocks
    and 2 r_last + 1 more.  C counts both sides of a matrix cell in the gain rule (extra: n_in, n_out; the cell's C is n_in)."""
    blocks, ratios = LEVEL_BLOCKS[n], (1,) + (2,) * (n - 1)
    Ls, D = level_geometry(L, blocks, ratios)
    r_last = Ls[-1] // L
    more = {"blocks": blocks, "ratios": ratios, "taps": D[-1] - RAGGED}
    tag = pre + "-%dlv" % n
    if fade is None:
        more["nb"] = D[-2] // L + r_last * (blocks[-1] + 2) + 3
        more["back"] = "fused" if family.endswith("levels_fused") else "general"
    else:
        lg = L.bit_length() - 1
        more["new_gain"] = 0.125 if (lg + C + fade) % 2 == 0 else 8.0
        more["t0"] = D[-2] // L + r_last + 1
        more["nb"] = more["t0"] + K + 2 * r_last + 1
        tag += "-g%g" % more["new_gain"]
    more.update(extra)
    return _kind_cell(family, s, L, extra.get("n_in", C), fin, fout, tag + post, **more)


def _build_levels_cells():
    cells = []
    add = lambda *a: cells.append(_levels_cell(*a))
    for n, Ls in ((3, (512, 1024, 2048, 4096)), (4, (512, 1024, 2048))):    # k_inv_levels: fp32, float frames, an even count;
        for L in Ls:                                  # a run of n levels passes through 0 .. n - 1 contributing rings
            add("levels_fused", 4, L, 2, FLOAT_LE, FLOAT_LE, n)
        add("levels_fused", 4, Ls[1], 8, FLOAT_LE, FLOAT_LE, n)
    for L in [1 << lg for lg in range(4, 13)]:        # k_levels_combine<float>: an odd count anywhere, any count below the pair plans
        add("levels_general32", 4, L, 3, FLOAT_LE, FLOAT_LE, 3)
        if L < 512:
            add("levels_general32", 4, L, 2, FLOAT_LE, FLOAT_LE, 3)
        if L in (16, 256, 2048):                      # four levels: the smallest and the largest head there is, one between
            add("levels_general32", 4, L, 3, FLOAT_LE, FLOAT_LE, 4)
    for L in [1 << lg for lg in range(4, 12)]:        # k_levels_combine<double>
        for C in (2, 3):
            add("levels_general64", 8, L, C, FLOAT64_LE, FLOAT64_LE, 3)
        if L in (16, 1024):                           # four levels: the smallest and the largest head there is
            add("levels_general64", 8, L, 2, FLOAT64_LE, FLOAT64_LE, 4)
        if L in (64, 1024):                           # the plug-in's shape: fp64 arithmetic, float32 stereo frames
            add("levels_general64", 8, L, 2, FLOAT_LE, FLOAT_LE, 3)
    return cells


def _build_lfade_cells():
    cells = []
    add = lambda *a: cells.append(_levels_cell(*a))
    # k_inv_lfade<LOG2N, NR>: NR = n - 1 rings at every size n levels fit, any channel count.  C alternates with the size, so
    # lg + C is the same all along a row; half the index in the row takes its place in the gain rule: the direction changes
    # every second size, and each channel count meets both
    for n, Ls in ((2, (512, 1024, 2048, 4096, 8192)), (3, (512, 1024, 2048, 4096)), (4, (512, 1024, 2048))):
        for i, L in enumerate(Ls):
            add("lfade_fused", 4, L, 2 + (i + n) % 2, FLOAT_LE, FLOAT_LE, n, i // 2)
    for L in (16, 32, 64, 128, 256):                  # k_lfade_sum<float>: below the pair plans
        lg = L.bit_length() - 1
        add("lfade_general32", 4, L, 2, FLOAT_LE, FLOAT_LE, 3, 0)
        add("lfade_general32", 4, L, 3, FLOAT_LE, FLOAT_LE, 4 if lg % 2 == 0 else 2, 0)
    for L, n in ((512, 2), (1024, 3), (2048, 4), (4096, 3), (8192, 2)):     # ... and inside them where the output frames are not FLOAT_LE
        add("lfade_general32", 4, L, 2, FLOAT_LE, FLOAT64_LE, n, 0)
    for L in [1 << lg for lg in range(4, 12)]:        # k_lfade_sum<double>
        add("lfade_general64", 8, L, 2, FLOAT64_LE, FLOAT64_LE, 3, 0)
        if L in (64, 1024):
            add("lfade_general64", 8, L, 3, FLOAT_LE, FLOAT_LE, 3, 0)
    add("lfade_general64", 8, 4096, 2, FLOAT64_LE, FLOAT64_LE, 2, 0)       # a tail of 8192, the largest fp64 transform
    add("lfade_general64", 8, 1024, 3, FLOAT64_LE, FLOAT64_LE, 4, 0)       # four levels, 8192 again
    return cells


# Multi-level matrix engines (csrc/mlevels.hip and the matrix levels in engine.hip) and their crossfades (csrc/mfade.hip,
# csrc/lfade.hip): the geometry of _levels_cell, n_in inputs to n_out outputs, every (output, input) pair a filter of its
# own length.
MFADE_WIDE_K = 11         # the whole fade in one launch: time tiles 8 + 3 (fp32), 4 + 4 + 3 (fp64), as MATRIX_CALLS[1]


def matrix_level_lengths(L, blocks, ratios, n_in, n_out, null, new=False):
    """[o][i] tap counts (None at the NULL pair).  Filter j, row-major over the pairs that are not NULL, belongs to level
    order[j % n], order = [n - 1, 0, 1, .., n - 2], and ends RAGGED + j // n taps short of the end of that level's last
    partition: the first filter has the D[-1] - RAGGED taps of the diagonal cells, and with n or more filters one ends in
    every level.  new: the second set of a fade -- the same table with the input columns mirrored (the outputs, where there is
    one input), the NULL pair with them, and every filter that short of the end of its level's FIRST partition.  Where the
    mirror leaves the NULL pair where it was (the middle column of three) or some level's partition counts as they were (a
    level of one partition under a table that is its own mirror image), the outputs are mirrored as well."""
    n = len(blocks)
    Ls, D = level_geometry(L, blocks, ratios)
    order = [n - 1] + list(range(n - 1))
    table, j = [], 0
    for o in range(n_out):
        row = []
        for i in range(n_in):
            if (o, i) == null:
                row.append(None)
                continue
            row.append((order[j % n], j // n))
            j += 1
        table.append(row)
    lens = lambda tab, first: [[None if e is None else (D[e[0]] + Ls[e[0]] if first else D[e[0] + 1]) - RAGGED - e[1] for e in r]
                               for r in tab]
    old = lens(table, False)
    if not new:
        return old
    table = [r[::-1] for r in table] if n_in > 1 else table[::-1]
    if n_in > 1 and not sets_differ(L, blocks, ratios, old, lens(table, True)):
        table = table[::-1]
    return lens(table, True)


def level_counts(L, blocks, ratios, lens):
    """[level][o][i]: partitions of h_{o,i} on the level, as bfir_engine_set_coeff_matrix_levels splits the filters."""
    Ls, D = level_geometry(L, blocks, ratios)
    return [[[0 if n is None else -(-max(0, min(n - D[k], blocks[k] * Ls[k])) // Ls[k]) for n in r] for r in lens]
            for k in range(len(Ls))]


def sets_differ(L, blocks, ratios, old, new):
    """The two sets of a fade have their NULL pair (if any) in different places and different partition counts at every level."""
    where = lambda lens: [(o, i) for o, r in enumerate(lens) for i, n in enumerate(r) if n is None]
    co, cn = level_counts(L, blocks, ratios, old), level_counts(L, blocks, ratios, new)
    return (not where(old) or where(old) != where(new)) and all(a != b for a, b in zip(co, cn))


def _mlevels_cell(family, s, L, n_in, n_out, fin, fout, n, fade=None, K=FADE_K, wide=False):
    """_levels_cell with a matrix: one NULL pair where there are three pairs or more, by the rule of MATRIX_CELLS and one step
    on where that is filter 0; lens (and lens_new, the fade's second set) from matrix_level_lengths.  A fade cell's gain rule
    counts both sides.  wide: K = MFADE_WIDE_K blocks of fade in one call with chunks that long."""
    lg = L.bit_length() - 1
    null = None
    if n_in * n_out >= 3:
        null = (lg % n_out, lg % n_in)
        if null == (0, 0):
            null = (0, 1) if n_in > 1 else (1, 0)
    extra = {"n_in": n_in, "n_out": n_out, "null": null}
    if fade is not None:
        extra.update(chunk=K if wide else 2, wide=wide)
    cell = _levels_cell(family, s, L, n_in + n_out, fin, fout, n, fade, K, "-to%d" % n_out, "-wide" if wide else "", **extra)
    cell["lens"] = matrix_level_lengths(L, cell["blocks"], cell["ratios"], n_in, n_out, null)
    if fade is not None:
        cell["K"] = K
        cell["lens_new"] = matrix_level_lengths(L, cell["blocks"], cell["ratios"], n_in, n_out, null, new=True)
    return cell


PAIR_PLANS = (512, 1024, 2048, 4096, 8192)


def _build_mlevels_cells():
    cells = []
    add = lambda *a: cells.append(_mlevels_cell(*a))
    # the fused back end: k_inv_pair / k_inv_nup / k_inv_levels on the output pair, frames 3 floats apart, and k_inv_lone<LOG2N, NR>
    # on the third output -- a run of n levels passes through 0 .. n - 1 contributing rings
    for n, Ls in ((2, PAIR_PLANS), (3, PAIR_PLANS[:4]), (4, PAIR_PLANS[:3])):
        for L in Ls:
            add("mlevels_fused", 4, L, 2, 3, FLOAT_LE, FLOAT_LE, n)
        add("mlevels_fused", 4, Ls[1], 2, 2, FLOAT_LE, FLOAT_LE, n)    # pair front end, frame stride 0
        add("mlevels_fused", 4, Ls[1], 1, 2, FLOAT_LE, FLOAT_LE, n)    # direct front end on the fused back end
        add("mlevels_fused", 4, Ls[1], 2, 1, FLOAT_LE, FLOAT_LE, n)    # the lone kernel alone, NO = 1 in the MAC
    add("mlevels_fused", 4, 512, 3, 5, FLOAT_LE, FLOAT_LE, 3)          # two output pairs and the lone one, a ragged second MAC tile
    # the general back end, fp32: below the pair plans ...
    for L in (16, 32, 64, 128, 256):
        add("mlevels_general32", 4, L, 2, 3, FLOAT_LE, FLOAT_LE, 3)
        add("mlevels_general32", 4, L, 3, 2, FLOAT_LE, FLOAT_LE, 3)
        if L in (16, 256):                            # four levels: the smallest head and the largest below the pair plans
            add("mlevels_general32", 4, L, 2, 3, FLOAT_LE, FLOAT_LE, 4)
    for L in PAIR_PLANS:                              # ... and inside them where the output frames are not FLOAT_LE; 8192 x 16384
        add("mlevels_general32", 4, L, 2, 3, FLOAT_LE, FLOAT64_LE, 2)
    for L in [1 << lg for lg in range(4, 12)]:        # fp64
        add("mlevels_general64", 8, L, 2, 3, FLOAT64_LE, FLOAT64_LE, 3)
        if L in (16, 1024):                           # four levels: the smallest and the largest head there is
            add("mlevels_general64", 8, L, 2, 3, FLOAT64_LE, FLOAT64_LE, 4)
        if L in (64, 1024):                           # the plug-in's shape: fp64 arithmetic, float32 stereo frames
            add("mlevels_general64", 8, L, 2, 2, FLOAT_LE, FLOAT_LE, 3)
    add("mlevels_general64", 8, 4096, 2, 3, FLOAT64_LE, FLOAT64_LE, 2)  # a tail of 8192, the largest fp64 transform
    return cells


def _build_mfade_cells():
    cells = []
    add = lambda *a, **k: cells.append(_mlevels_cell(*a, **k))
    io = lambda Cn: (2, 3) if Cn == 2 else (3, 2)     # the channel count of an LFADE cell -> (n_in, n_out): 2 -> 3 or 3 -> 2
    # k_inv_lfade<LOG2N, NR = n - 1> with an odd and an even output count alternating along a row, as lfade_fused alternates C
    for n, Ls in ((2, PAIR_PLANS), (3, PAIR_PLANS[:4]), (4, PAIR_PLANS[:3])):
        for i, L in enumerate(Ls):
            add("mfade_fused", 4, L, *io(2 + (i + n) % 2), FLOAT_LE, FLOAT_LE, n, i // 2)
    for L in (16, 32, 64, 128, 256):                  # k_lfade_sum<float>: below the pair plans
        lg = L.bit_length() - 1
        add("mfade_general32", 4, L, 2, 3, FLOAT_LE, FLOAT_LE, 3, 0)
        add("mfade_general32", 4, L, 3, 2, FLOAT_LE, FLOAT_LE, 4 if lg % 2 == 0 else 2, 0)
    for L, n in ((512, 2), (1024, 3), (2048, 4), (4096, 3), (8192, 2)):     # ... and inside them where the output frames are not FLOAT_LE
        add("mfade_general32", 4, L, 2, 3, FLOAT_LE, FLOAT64_LE, n, 0)
    for L in [1 << lg for lg in range(4, 12)]:        # k_lfade_sum<double>
        add("mfade_general64", 8, L, 2, 3, FLOAT64_LE, FLOAT64_LE, 3, 0)
        if L in (64, 1024):
            add("mfade_general64", 8, L, 3, 2, FLOAT_LE, FLOAT_LE, 3, 0)
    add("mfade_general64", 8, 4096, 2, 3, FLOAT64_LE, FLOAT64_LE, 2, 0)     # a tail of 8192, the largest fp64 transform
    add("mfade_general64", 8, 1024, 3, 2, FLOAT64_LE, FLOAT64_LE, 4, 0)     # four levels, 8192 again
    # the time-tiled k_mac_duo: one cell per (T, ILV, NO) at the smallest head with that layout, three levels.  The head's one
    # fading launch has MFADE_WIDE_K blocks; the tails' have one to four (the block a call began inside runs alone), so TT = 1:
    # with one output, the only NO = 1 launches of the fp32 latency form
    for s, L, n_out, fmt in ((4, 16, 1, FLOAT_LE), (4, 16, 3, FLOAT_LE), (4, 256, 1, FLOAT_LE), (4, 256, 3, FLOAT_LE),
                             (8, 16, 3, FLOAT64_LE), (8, 1024, 3, FLOAT64_LE)):
        add("mfade_general32" if s == 4 else "mfade_general64", s, L, 2, n_out, fmt, fmt, 3, 0, K=MFADE_WIDE_K, wide=True)
    return cells


NUP_CELLS = _build_nup_cells()
FADE_CELLS = _build_fade_cells()
MATRIX_CELLS = _build_matrix_cells()
LEVELS_CELLS = _build_levels_cells()
LFADE_CELLS = _build_lfade_cells()
MLEVELS_CELLS = _build_mlevels_cells()
MFADE_CELLS = _build_mfade_cells()
KIND_CELLS = NUP_CELLS + FADE_CELLS + MATRIX_CELLS + LEVELS_CELLS + LFADE_CELLS + MLEVELS_CELLS + MFADE_CELLS

# bfir_engine_create_nup must fail: (realsize, L, tail_ratio, error name) -- the tail's partition is past the range
NUP_REFUSALS = [(4, 16384, 2, "ERR_UNSUPPORTED"), (8, 8192, 2, "ERR_UNSUPPORTED")]

# bfir_engine_create_levels must fail: (realsize, L, levels, error name) -- the first shape past each limit
LEVELS_REFUSALS = [(4, 8192, 3, "ERR_UNSUPPORTED"), (4, 4096, 4, "ERR_UNSUPPORTED"), (8, 4096, 3, "ERR_UNSUPPORTED")]

# bfir_engine_create_matrix_levels must fail, 2 -> 3: the same three shapes (check_levels_args serves both kinds)
MLEVELS_REFUSALS = list(LEVELS_REFUSALS)


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


# ---- data, references and the norm of the engine-kind cells ---------------------------------------------------------
def tolerance(cell, TOL):
    """The project's own (conftest.TOL): 1e-5 for fp32 arithmetic or float32 output frames, TOL[8] otherwise."""
    return 1e-5 if (cell["s"] == 4 or cell["out_fmt"] == FLOAT_LE) else TOL[cell["s"]]


def block_errors(y, ref, L):
    """[C, n_blocks] max |y - ref| of each output block of each channel over that channel's own max |ref|."""
    y, ref = np.asarray(y, np.float64), np.asarray(ref, np.float64)
    nb, Cn = ref.shape[0] // L, ref.shape[1]
    d = np.abs(y - ref).reshape(nb, L, Cn).max(axis=1).T
    return d / np.maximum(np.abs(ref).max(axis=0), 1e-300)[:, None]


def _rng(cell):
    return np.random.default_rng(zlib.crc32(cell["id"].encode()))


def _noise(orc, rng, cell):
    """The frames sent: uniform noise, odd channels at 1/8, in the input format."""
    nb, L, Cn = cell["nb"], cell["L"], cell["C"]
    return (rng.uniform(-1.0, 1.0, (nb * L, Cn)) * amplitudes(nb, L, Cn, False)).astype(orc.fmt_dtype(cell["in_fmt"]))


def reference(orc, x, h):
    """[frames, C] float64: reference_conv per channel, from the float64 value of the frames and taps actually sent."""
    x64 = np.asarray(x, np.float64)
    return np.stack([reference_conv(orc, x64[:, c], np.asarray(h[c], np.float64)) for c in range(len(h))], axis=1)


def nup_data(orc, cell):
    """(h, x) of a two-level or multi-level cell: taps in the working precision, frames in the input format."""
    rng = _rng(cell)
    h = [v.astype(orc.real_dtype(cell["s"])) for v in flat_ir(rng, cell["C"], cell["taps"])]
    return h, _noise(orc, rng, cell)


def fade_data(orc, cell):
    """(h_old, h_new, x) of a fade cell (FADE_CELLS, LFADE_CELLS)."""
    rng = _rng(cell)
    dt = orc.real_dtype(cell["s"])
    g_old, g_new = (1.0, 0.125) if cell["new_gain"] < 1.0 else (0.125, 1.0)
    h_old = [(v * g_old).astype(dt) for v in flat_ir(rng, cell["C"], cell["taps"])]
    h_new = [(v * g_new).astype(dt) for v in flat_ir(rng, cell["C"], cell["taps"])]
    return h_old, h_new, _noise(orc, rng, cell)


def fade_reference(orc, cell, h_old, h_new, x):
    """float64: y_old before block t0, y_old (1 - f m) + y_new f m with f = 1 / (K L - 1), m = (t - t0) L + n over the K
    blocks of the fade, y_new after it; y_old / y_new the reference convolutions of the whole stream (of a matrix cell, whose
    sets are rows of filters: matrix_reference_conv)."""
    L, t0, K = cell["L"], cell["t0"], cell.get("K", FADE_K)
    conv = matrix_reference_conv if "n_out" in cell else lambda o, rows, xx: reference(o, xx, rows)
    y_old, y_new = conv(orc, h_old, x), conv(orc, h_new, x)
    y = y_old.copy()
    y[(t0 + K) * L:] = y_new[(t0 + K) * L:]
    fm = (np.arange(K * L) / (K * L - 1.0))[:, None]
    a, b = t0 * L, (t0 + K) * L
    y[a:b] = y_old[a:b] * (1.0 - fm) + y_new[a:b] * fm
    return y


def matrix_data(orc, cell):
    """(rows, x) of a matrix cell: rows[o][i] the taps of h_{o,i}, None at cell["null"]."""
    rng = _rng(cell)
    dt = orc.real_dtype(cell["s"])
    rows = [[v.astype(dt) for v in flat_ir(rng, cell["n_in"], cell["taps"])] for _ in range(cell["n_out"])]
    o, i = cell["null"]
    rows[o][i] = None
    return rows, _noise(orc, rng, cell)


def matrix_reference_conv(orc, rows, x):
    """[frames, n_out] float64: output o is the sum over the inputs of reference_conv(x_i, h_{o,i})."""
    x64 = np.asarray(x, np.float64)
    out = np.zeros((x64.shape[0], len(rows)))
    for o, row in enumerate(rows):
        for i, h in enumerate(row):
            if h is not None:
                out[:, o] += reference_conv(orc, x64[:, i], np.asarray(h, np.float64))
    return out


def _matrix_rows(orc, rng, cell, lens, gain=1.0):
    """rows[o][i]: a flat_ir filter of lens[o][i] taps times gain in the working precision, None where lens has None."""
    dt = orc.real_dtype(cell["s"])
    return [[None if n is None else (flat_ir(rng, 1, n)[0] * gain).astype(dt) for n in row] for row in lens]


def mlevels_data(orc, cell):
    """(rows, x) of a multi-level matrix cell: every pair its own filter of its own length (cell["lens"]), sum |h| = 1."""
    rng = _rng(cell)
    return _matrix_rows(orc, rng, cell, cell["lens"]), _noise(orc, rng, cell)


def mfade_data(orc, cell):
    """(rows_old, rows_new, x) of a fade cell of a multi-level matrix engine: the gains of fade_data, the lengths of the two
    sets from cell["lens"] and cell["lens_new"]."""
    rng = _rng(cell)
    g_old, g_new = (1.0, 0.125) if cell["new_gain"] < 1.0 else (0.125, 1.0)
    rows_old = _matrix_rows(orc, rng, cell, cell["lens"], g_old)
    rows_new = _matrix_rows(orc, rng, cell, cell["lens_new"], g_new)
    return rows_old, rows_new, _noise(orc, rng, cell)


def partition_counts(cell, lens):
    """level_counts of a cell's geometry."""
    return level_counts(cell["L"], cell["blocks"], cell["ratios"], lens)


# ---- the delay kernels (csrc/delay.hip; run_blocks_delayed in engine.hip) ---------------------------------------------
# DELAY_SUB_CELLS, DELAY_COPY_CELLS, DELAY_KIND_CELLS and DELAY_MID_CELLS name every instance, tile shape and history edge
# of k_delay_sub and k_delay_copy; tests/test_delay_matrix.py checks them against the sources on the CPU and
# tests/test_delay_matrix_gpu.py runs them.
DELAY_IN, DELAY_OUT = 0, 1
FMT_NAMES = {1: "S8", 2: "S16_LE", 3: "S16_BE", 4: "S24_LE", 5: "S24_BE", 6: "S32_LE", 7: "S32_BE", 8: "FLOAT_LE",
             9: "FLOAT_BE", 10: "FLOAT64_LE", 11: "FLOAT64_BE"}
FMT_BYTES = {1: 1, 2: 2, 3: 2, 4: 3, 5: 3, 6: 4, 7: 4, 8: 4, 9: 4, 10: 8, 11: 8}


def delay_limits():
    """What delay.hip, kernels.h, engine.hip and the public header fix for the delay kernels."""
    with open(os.path.join(os.path.dirname(os.path.dirname(CSRC)), "include", "bfir_hip.h")) as f:
        mc = re.search(r"#define\s+BFIR_MAXCHANNELS\s+(\d+)", f.read())
    init = re.search(r"bfir_engine_delay_init\(.*?\n\}", _read("engine.hip"), re.S)
    assert mc and init
    hl = re.search(r"half_filter_length\s*<\s*(\d+)\s*\|\|\s*half_filter_length\s*>\s*(\d+)", init.group(0))
    assert hl
    return {"sub_tile": _const(_read("delay.hip"), "kSubTile"), "delay_ch": _const(_read("kernels.h"), "BFIR_DELAY_CH"),
            "h_min": int(hl.group(1)), "h_max": int(hl.group(2)), "max_channels": int(mc.group(1))}


def delay_source_instances():
    """({(R, F)} of k_delay_sub, {(unit bytes, VEC)} of k_delay_copy) that delay.hip launches: its hipLaunchKernelGGL lines
    and the unit types launch_delay_copy hands to delay_copy_t."""
    src = _read("delay.hip")
    sub = set(re.findall(r"hipLaunchKernelGGL\(\(k_delay_sub<(\w+),\s*(\w+)>\)", src))
    vecs = {v == "true" for v in re.findall(r"hipLaunchKernelGGL\(\(k_delay_copy<T,\s*(\w+)>\)", src)}
    body = re.search(r"void launch_delay_copy\(.*?\n\}", src, re.S)
    assert body
    units = {int(b) // 8 for b in re.findall(r"delay_copy_t<uint(\d+)_t>", body.group(0))}
    return sub, {(u, v) for u in units for v in vecs}


def _align(addr):
    """The largest power of two up to 16 that divides addr."""
    return 16 if addr % 16 == 0 else addr & -addr


def delay_copy_instance(sample_bytes, ptr_align, dst_align):
    """launch_delay_copy restated: (unit bytes, VEC) from the sample size, the alignment every buffer of the launch has
    (sources, histories and destinations) and the alignment both destinations have."""
    unit = sample_bytes if sample_bytes in (8, 4, 2) and ptr_align % sample_bytes == 0 else 1
    return unit, dst_align % 16 == 0


def delay_sub_instance(realsize, sample_bytes):
    """launch_delay_sub restated: (R, F) of the k_delay_sub instance."""
    name = {4: "float", 8: "double"}
    return name[realsize], name[sample_bytes]


def delay_sub_lds(C, h, realsize, sample_bytes, lim=None):
    """Bytes of LDS launch_delay_sub asks for: the tile's output frames at the full channel count, then C source spans."""
    lim = lim or delay_limits()
    return lim["sub_tile"] * lim["delay_ch"] * sample_bytes + C * (lim["sub_tile"] + 2 * h) * realsize


def delay_sub_grid(n_frames, lim=None):
    lim = lim or delay_limits()
    return -(-n_frames // lim["sub_tile"])


def uneven_calls(nb):
    """Blocks per call 2, 1, 3, 2, 1, 3, ... summing to nb (tests/test_delay_gpu.py takes its "uneven" pattern from here)."""
    out, k = [], 0
    while sum(out) < nb:
        out.append(min((2, 1, 3)[k % 3], nb - sum(out)))
        k += 1
    return out


def delay_n_blocks(reach, L):
    """Blocks that play a history of `reach` frames in and out (_n_blocks of tests/test_delay_gpu.py is this function)."""
    return 2 * -(-reach // L) + 3


def _sub_geometries(s):
    """name -> (L, C, h, step_count, kaiser_beta, delays, subdelays, max_delay, calls, chunks), the edge of each in the
    comment; every one with two channels or more has a channel with subdelay 0, the unfiltered shift by d + h."""
    top = max(supported_lengths(source_limits(), s))
    b_total = delay_n_blocks(1000 + 256, 16)
    return {
        # every piece (16 frames) is shorter than the span (2 h = 256) and the history; a rectangular window
        "a": (16, 1, 128, 2, 0.0, (0,), (1,), 0, [1] * 20, (None,)),
        # 640 frames in one launch: three tiles, the last ragged; the largest LDS request; delays longer than most pieces
        "b": (16, 8, 128, 1000, 9.0, (0, 1000, 17, 999, 1000, 0, 16, 500), (999, -999, 1, -1, 0, -999, 1, 0), 1000,
              uneven_calls(60) + [40] + uneven_calls(b_total - 100), (None,)),
        # three taps that all count; 12-byte frames (fp32), an odd number of blocks
        "c": (64, 3, 1, 2, 0.0, (5, 0, 70), (1, -1, 0), 70, uneven_calls(delay_n_blocks(70 + 2, 64)), (None,)),
        # a block is exactly one tile; pieces of 3, 3 and 1 blocks
        "d": (256, 5, 31, 10, 2.0, (0, 255, 256, 300, 1), (3, -7, 0, 9, -1), 300, [7], (1, 3)),
        # 20 and 12 workgroups: the XCD remap with a remainder
        "e": (1024, 2, 8, 10, 9.0, (100, 1500), (3, 0), 1500, [5, 3], (None,)),
        # the largest transform of the precision
        "f": (top, 1, 4, 10, 9.0, (7,), (-3,), 7, [2], (None,)),
    }


SUB_TYPE_PAIRS = [(4, FLOAT_LE), (4, FLOAT64_LE), (8, FLOAT_LE), (8, FLOAT64_LE)]


def _sub_cell(prefix, side, s, fmt, name, geo, **more):
    L, C, h, steps, beta, delays, subs, max_delay, calls, chunks = geo
    cell = {"id": "%s-%s-s%d-%s-%s" % (prefix, "in" if side == DELAY_IN else "out", s, FMT_NAMES[fmt], name),
            "side": side, "s": s, "fmt": fmt, "geo": name, "L": L, "C": C, "h": h, "steps": steps, "beta": beta,
            "delays": tuple(delays), "subs": tuple(subs), "max_delay": max_delay, "calls": list(calls), "chunks": tuple(chunks),
            "instance": delay_sub_instance(s, FMT_BYTES[fmt])}
    cell.update(more)
    return cell


def _build_delay_sub_cells():
    return [_sub_cell("dsub", side, s, fmt, name, geo) for side in (DELAY_IN, DELAY_OUT) for s, fmt in SUB_TYPE_PAIRS
            for name, geo in _sub_geometries(s).items()]


def delay_sub_chunk(cell, chunk):
    """The blocks per launch a stage cell runs with: one of cell["chunks"], None standing for the cell's longest call."""
    return max(cell["calls"]) if chunk is None else chunk


def delay_sub_sees_last_tap(taps_fn, cell):
    """Whether a stage that drops tap 2 h must leave delay_sub_bound on every filtered channel of the cell.  It adds
    |f[2h]| |u[n - d - 2h]| to the error.  Against the arithmetic term of the bound alone any tap that the working
    precision resolves shows (asserted, not assumed: the beta 0 and 2.0 cells in both precisions, the fp64 cells at beta
    9).  Where the frame type is narrower than R the bound also allows u_F |ref|: of N samples of uniform noise (8192 and
    more in the cells near this limit, e and f) about N / 64 have |u[n - d - 2h]| > 1/2 and |ref| < 1/32, so a tap of u_F / 16 or more leaves the bound there;
    a smaller one is hidden by the frame's own rounding and nothing read from such frames can be asked to see it."""
    if cell["s"] == 4:
        return cell["beta"] in (0.0, 2.0)
    u_f = 2.0 ** -24 if cell["fmt"] == FLOAT_LE else 0.0
    last = [abs(float(np.asarray(taps_fn(cell["h"], sd, cell["steps"], cell["beta"], cell["s"]))[-1]))
            for sd in delay_sub_steps(cell)[0][1] if sd]
    return min(last) >= u_f / 16


def delay_sub_launches(cell, chunk):
    """Frames of every k_delay_sub launch of the cell: run_blocks_delayed cuts a call into pieces of at most `chunk` blocks
    (None: delay_sub_chunk(cell, None), the cell's longest call, which the device test sets with set_chunk: every call is
    one piece whatever the automatic chunk would be)."""
    chunk = delay_sub_chunk(cell, chunk)
    out = []
    for n in cell["calls"]:
        while n > 0:
            tc = min(chunk, n)
            out.append(tc * cell["L"])
            n -= tc
    return out


def delay_sub_steps(cell):
    """[(delays, subdelays, blocks, reset before)] of a cell: one setting for all its calls, or the cell's own steps."""
    return cell.get("steps_list") or [(cell["delays"], cell["subs"], sum(cell["calls"]), False)]


def _build_delay_mid_cells():
    """Geometry c with the setting changed between calls: sub to another sub, sub to none, none to sub, a longer delay that
    repeats history, reset() in the middle, one more change.  One call per step."""
    steps = [((5, 0, 70), (1, -1, 0), 3, False), ((5, 0, 70), (-1, 1, 0), 2, False), ((6, 1, 70), (0, 0, 0), 2, False),
             ((6, 1, 3), (1, 0, -1), 2, False), ((70, 64, 3), (1, 0, -1), 2, False), ((70, 64, 3), (1, 0, -1), 3, True),
             ((0, 0, 0), (0, 1, 1), 2, False)]
    cells = []
    for side in (DELAY_IN, DELAY_OUT):
        for s, fmt in SUB_TYPE_PAIRS:
            geo = list(_sub_geometries(s)["c"])
            geo[8] = [n for _, _, n, _ in steps]
            cells.append(_sub_cell("dmid", side, s, fmt, "c", geo, steps_list=steps))
    return cells


INT_FMTS = (1, 2, 3, 4, 5, 6, 7)
COPY_SHAPE = (16, 3, 2, (0, 7, 37))           # L, C, B, delays
ALIGN_FMTS = (FLOAT_LE, FLOAT64_LE, 2, 4, 1)  # FLOAT_LE, FLOAT64_LE, S16_LE, S24_LE, S8
DITHER_FMTS = (2, 4, 6)                       # S16_LE, S24_LE, S32_LE


def _build_delay_copy_cells():
    """Whole samples.  kind "format": run() through the engine's own aligned buffers; "dither": a dithered integer output,
    delayed behind the dither; "align": run_device with the caller's pointer on the delayed side `offset` bytes past a
    16-byte boundary -- the engine proper works between that side's aligned scratch and the other side's aligned pointer, which
    chunk_aligned accepts for every format here, so the other side stays undelayed.  `instance` is what launch_delay_copy
    then picks: an input-side launch stores to the scratch and the history (VEC) and reads the caller's pointer, an
    output-side launch stores to the caller's pointer."""
    L, C, B, delays = COPY_SHAPE
    cells = []

    def add(kind, side, fmt, offset, s=4, **more):
        sb = FMT_BYTES[fmt]
        inst = delay_copy_instance(sb, _align(offset), 16 if side == DELAY_IN else _align(offset))
        cell = {"id": "dcopy-%s-%s-%s%s" % (kind, "in" if side == DELAY_IN else "out", FMT_NAMES[fmt], "+%d" % offset if offset else ""),
                "kind": kind, "side": side, "s": s, "fmt": fmt, "offset": offset, "L": L, "C": C, "B": B, "delays": delays,
                "max_delay": max(delays), "calls": uneven_calls(delay_n_blocks(max(delays), L)), "instance": inst}
        cell.update(more)
        cells.append(cell)
    for side in (DELAY_IN, DELAY_OUT):
        for fmt in sorted(FMT_NAMES):
            add("format", side, fmt, 0, s=8 if fmt in (10, 11) else 4)
    for fmt in DITHER_FMTS:
        add("dither", DELAY_OUT, fmt, 0)
    for side in (DELAY_IN, DELAY_OUT):
        for fmt in ALIGN_FMTS:
            for offset in sorted({FMT_BYTES[fmt], 1}, reverse=True):      # one sample, one byte
                add("align", side, fmt, offset, s=8 if fmt == FLOAT64_LE else 4)
    return cells


KIND_L = 64
DELAY_KINDS = {   # kind -> (inputs, outputs); BrutefirMatrix 3 -> 2, BrutefirNup, BrutefirLevels of three levels, BrutefirMatrixLevels 2 -> 3
    "matrix": (3, 2), "nup": (3, 3), "levels": (3, 3), "mlevels": (2, 3)}
KIND_SUB = (4, 10, 9.0, (5, 70, 0), (3, 0, -7), 70)      # h, step_count, beta, delays, subdelays (one 0), max_delay
KIND_FADE = (5, 3, (3, 0, 40), (100, 31, 0), 100)        # t0, fade blocks, delays before / from the second fade block, max_delay


def _build_delay_kind_cells():
    """L = 64, fp32, FLOAT_LE.  Per kind a sub-sample stage on each side, and per kind and for the plain engine a fade that
    runs while the input side is delayed by whole samples: t0 blocks, the kind's fade call over 3 head blocks, one block, the
    delays changed by set_delay, the rest."""
    h, steps, beta, delays, subs, max_delay = KIND_SUB
    cells = []
    for kind, (n_in, n_out) in DELAY_KINDS.items():
        for side in (DELAY_IN, DELAY_OUT):
            C = n_in if side == DELAY_IN else n_out
            nb = delay_n_blocks(max_delay + 2 * h, KIND_L) + 8          # long enough for every level to sound
            geo = (KIND_L, C, h, steps, beta, delays[:C], subs[:C], max_delay, uneven_calls(nb), (None,))
            cells.append(_sub_cell("dkind-" + kind, side, 4, FLOAT_LE, "sub", geo, kind=kind, n_in=n_in, n_out=n_out))
    t0, K, d0, d1, max_delay = KIND_FADE
    for kind, (n_in, n_out) in list(DELAY_KINDS.items()) + [("plain", (2, 2))]:
        nb = t0 + K + 9
        cells.append({"id": "dkind-%s-fade" % kind, "kind": kind, "fade": True, "side": DELAY_IN, "s": 4, "fmt": FLOAT_LE,
                      "L": KIND_L, "C": n_in, "n_in": n_in, "n_out": n_out, "t0": t0, "K": K, "nb": nb,
                      "delays": d0[:n_in], "delays_after": d1[:n_in], "max_delay": max_delay,
                      "instance": delay_copy_instance(4, 16, 16)})
    return cells


DELAY_SUB_CELLS = _build_delay_sub_cells()
DELAY_MID_CELLS = _build_delay_mid_cells()
DELAY_COPY_CELLS = _build_delay_copy_cells()
DELAY_KIND_CELLS = _build_delay_kind_cells()
DELAY_STAGE_CELLS = DELAY_SUB_CELLS + DELAY_MID_CELLS + [c for c in DELAY_KIND_CELLS if not c.get("fade")]
DELAY_CELLS = DELAY_SUB_CELLS + DELAY_MID_CELLS + DELAY_COPY_CELLS + DELAY_KIND_CELLS


# ---- the float64 model of the sub-sample stage and its error bound ----------------------------------------------------
def frame_dtype(fmt):
    return np.dtype("<f4") if fmt == FLOAT_LE else np.dtype("<f8")


def _shifted(v, d):
    w = np.zeros_like(v)
    if d < v.shape[0]:
        w[d:] = v[:v.shape[0] - d]
    return w


def delay_sub_reference(taps_fn, u, L, s, h, steps, beta, per_block):
    """The stage on the stream u [frames, C] that starts from silence, with per_block[t] = (delays, subdelays) in force in
    block t.  (ref, amp, filtered), each [frames, C]: ref_c[n] = sum_k f[k] u_c[n - d_c - k] over the taps
    f = taps_fn(h, subdelay, steps, beta, s) in their float64 value, summed in long double and rounded once to float64;
    amp_c[n] = sum_k |f[k]| |u_c[n - d_c - k]|; on a channel without a filter ref is u_c[n - d_c - h] itself, amp 0 and
    filtered False."""
    u = np.asarray(u)
    n, C = u.shape
    ref, amp, filt = np.zeros((n, C)), np.zeros((n, C)), np.zeros((n, C), bool)
    for c in range(C):
        uc = u[:, c].astype(np.longdouble)
        cache = {}
        for t in range(n // L):
            d, sd = per_block[t][0][c], per_block[t][1][c]
            if (d, sd) not in cache:
                if sd == 0:
                    cache[(d, sd)] = (_shifted(uc, d + h).astype(np.float64), np.zeros(n))
                else:
                    f = np.asarray(taps_fn(h, sd, steps, beta, s)).astype(np.longdouble)
                    cache[(d, sd)] = (_shifted(np.convolve(uc, f)[:n], d).astype(np.float64),
                                      _shifted(np.convolve(np.abs(uc), np.abs(f))[:n], d).astype(np.float64))
            r, a = cache[(d, sd)]
            ref[t * L:(t + 1) * L, c], amp[t * L:(t + 1) * L, c], filt[t * L:(t + 1) * L, c] = \
                r[t * L:(t + 1) * L], a[t * L:(t + 1) * L], sd != 0
    return ref, amp, filt


def delay_sub_bound(s, fmt, h, ref, amp):
    """|y - ref| <= (n_taps + 2) u_R amp + u_F |ref|: an n_taps-term fma chain in working precision (unit roundoff u_R)
    whose first term passes n_taps roundings, the rounding of the source to R on load and of the sum on store (+ 2), and the
    store to a frame type narrower than R (unit roundoff u_F, else 0).  Derived, not measured."""
    u_r = 2.0 ** -24 if s == 4 else 2.0 ** -53
    u_f = 2.0 ** -24 if (s == 8 and fmt == FLOAT_LE) else 0.0
    return (2 * h + 1 + 2) * u_r * amp + u_f * np.abs(ref)


def delay_sub_model(taps_fn, cell, u):
    """(ref, amp, filtered) of a stage cell on the stream u: delay_sub_reference with the cell's setting per block; after a
    reset() the stream starts from silence again."""
    L = cell["L"]
    parts, pos, seg, per_block = [], 0, 0, []
    for delays, subs, nb, reset in delay_sub_steps(cell):
        if reset:
            parts.append((seg, pos, per_block))
            seg, per_block = pos, []
        per_block += [(delays, subs)] * nb
        pos += nb
    parts.append((seg, pos, per_block))
    outs = [delay_sub_reference(taps_fn, u[a * L:b * L], L, cell["s"], cell["h"], cell["steps"], cell["beta"], pb)
            for a, b, pb in parts]
    return tuple(np.concatenate([o[k] for o in outs]) for k in range(3))


def delay_sub_audio(orc, cell):
    """The frames a stage cell sends: orc.synth_audio in the frame type."""
    side_c = cell["C"]
    return orc.synth_audio(_rng(cell), sum(cell["calls"]) * cell["L"], side_c, frame_dtype(cell["fmt"]))
