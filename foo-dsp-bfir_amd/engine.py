"""Host-side mirror of the reference's `brutefir` class over the C ABI.

Method names, argument meaning and return codes follow
brutefir/brutefir.hpp:15-128 so the parity tests read like the reference's
callers (foo_dsp_bfir/foo_dsp_bfir.cpp:279-345, brutefir/preprocessor.cpp:287-333).
Everything is computed by libbfir_hip.so on the GPU."""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import (BfirError, Overflow, SAMPLE_FORMAT_FLOAT64_LE, SAMPLE_FORMAT_FLOAT_LE)


def _real_dtype(realsize):
    return np.float32 if realsize == 4 else np.float64


# raw sample element types (brutefir/global.h:24-34); 24-bit samples are 3 raw bytes
_FMT_DTYPES = {1: np.dtype("i1"), 2: np.dtype("<i2"), 3: np.dtype(">i2"), 4: None, 5: None,
               6: np.dtype("<i4"), 7: np.dtype(">i4"), 8: np.dtype("<f4"), 9: np.dtype(">f4"),
               10: np.dtype("<f8"), 11: np.dtype(">f8")}


def raw_frames(fmt, shape_frames_channels):
    """Zeroed interleaved raw buffer [..., frames, C] (plus a trailing 3 for 24-bit formats)."""
    d = _FMT_DTYPES[fmt]
    shape = tuple(shape_frames_channels)
    return np.zeros(shape + (3,), np.uint8) if d is None else np.zeros(shape, d)


def pinned_frames(fmt, shape_frames_channels):
    """raw_frames in page-locked host memory (bfir_pinned_malloc): `Brutefir.run` on such arrays skips the staging copies.
    The array keeps its allocation alive; it is released when the array is collected."""
    import weakref
    d = _FMT_DTYPES[fmt]
    shape = tuple(shape_frames_channels) + ((3,) if d is None else ())
    dt = np.dtype(np.uint8) if d is None else d
    n = int(np.prod(shape)) * dt.itemsize
    lib = _lib.load()
    p = lib.bfir_pinned_malloc(n)
    if not p:
        raise BfirError(_lib.ERR_HIP, "bfir_pinned_malloc")
    buf = (C.c_char * n).from_address(p)
    a = np.frombuffer(buf, dtype=dt).reshape(shape)
    weakref.finalize(buf, lib.bfir_pinned_free, p)
    a[...] = 0
    return a


def subdelay_filter(half_filter_length, subdelay, step_count, kaiser_beta=9.0, realsize=8):
    """bfir_subdelay_filter: the 2 * half_filter_length + 1 taps of the filter that delays by half_filter_length +
    subdelay / step_count samples (delay::sample_sinc + firwindow_kaiser).  Host arithmetic: no device needed."""
    taps = np.zeros(2 * max(0, int(half_filter_length)) + 1, dtype=_real_dtype(realsize) if realsize in (4, 8) else np.float64)
    rc = _lib.load().bfir_subdelay_filter(int(half_filter_length), int(subdelay), int(step_count), float(kaiser_beta),
                                          int(realsize), taps.ctypes.data)
    if rc != 0:
        raise BfirError(rc, "bfir_subdelay_filter")
    return taps


class Brutefir:
    """brutefir(filter_length, filter_blocks, realsize, channels, in_format,
    out_format, sampling_rate, apply_dither)  -- brutefir/brutefir.hpp:18-25.

    n_engines > 1 builds a batch of independent, identically shaped engines
    that share launches (BASELINE.json configs[3])."""

    def __init__(self, filter_length, filter_blocks, realsize, channels,
                 in_format=None, out_format=None, sampling_rate=44100, apply_dither=False,
                 device=0, n_engines=1):
        dflt = SAMPLE_FORMAT_FLOAT_LE if realsize == 4 else SAMPLE_FORMAT_FLOAT64_LE
        self.L, self.B, self.s, self.C = filter_length, filter_blocks, realsize, channels
        self.in_format = dflt if in_format is None else in_format
        self.out_format = dflt if out_format is None else out_format
        self.n_engines, self.device = n_engines, device
        self.sampling_rate = sampling_rate
        self._lib = _lib.load()
        err = C.c_int(0)
        self._h = self._lib.bfir_engine_create_batch(
            n_engines, filter_length, filter_blocks, realsize, channels, self.in_format,
            self.out_format, sampling_rate, int(bool(apply_dither)), device, C.byref(err))
        if not self._h:
            raise BfirError(err.value, "bfir_engine_create")

    # -- lifetime ---------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.bfir_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    # -- brutefir public interface -----------------------------------------
    def is_initialized(self):
        return bool(self._lib.bfir_engine_is_initialized(self._h))

    def set_coeff(self, coeffs, n_coeffs=None, length=None, coeff_blocks=None, scale=1.0,
                  engine_index=0):
        """set_coeff(void **coeffs, n_coeffs, length, coeff_blocks, scale)
        (brutefir/brutefir.cpp:179-228).  Returns 0 or -2.

        A file name in place of the arrays is the reference's other overload, set_coeff(filename, coeff_blocks, scale)
        (set_coeff_file below): its second and third positional arguments are coeff_blocks and scale."""
        if isinstance(coeffs, (str, bytes, os.PathLike)):
            blocks = coeff_blocks if coeff_blocks is not None else n_coeffs
            return self.set_coeff_file(coeffs, blocks, scale if length is None else length)
        rd = _real_dtype(self.s)
        arrs = [np.ascontiguousarray(c, dtype=rd) for c in coeffs]
        n_coeffs = len(arrs) if n_coeffs is None else n_coeffs
        length = arrs[0].size if length is None else length
        coeff_blocks = self.B if coeff_blocks is None else coeff_blocks
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        return self._lib.bfir_engine_set_coeff_at(self._h, engine_index, ptrs, n_coeffs, length,
                                                  coeff_blocks, float(scale))

    def set_coeff_file(self, filename, coeff_blocks=None, scale=1.0):
        """set_coeff(const wchar_t *filename, coeff_blocks, scale) (brutefir/brutefir.cpp:89-165): one filter per channel
        from a sound file with the engine's channel count and sampling rate, at most coeff_blocks * filter_length frames of
        it.  Returns the number of filters, -1 for an incompatible (or unreadable) file, -2 when loading failed.  A file at
        another rate goes through buffer.resample_snd_file first."""
        from . import buffer
        coeff_blocks = self.B if coeff_blocks is None else int(coeff_blocks)
        if not buffer.check_snd_file(filename, self.C, self.sampling_rate):
            return -1
        got = buffer.load_snd_coeff(filename, self.s, coeff_blocks * self.L)
        if got is None:
            return -2
        coeffs, length = got
        n = min(len(coeffs), self.C)
        if Brutefir.set_coeff(self, coeffs[:n], n, length, coeff_blocks, scale) != 0:
            return -2
        return n

    def set_coeff_fade(self, coeffs, fade_blocks, n_coeffs=None, length=None, coeff_blocks=None, scale=1.0):
        """bfir_engine_set_coeff_fade: load a second filter set and fade to it over the next `fade_blocks` blocks
        (the linear ramp of fftw_convolver::convolver_crossfade_inplace, brutefir/fftw_convolver.cpp:275-321).
        Returns 0 or an ERR_* code; on ERR_COEFF the engine keeps running the old filters."""
        rd = _real_dtype(self.s)
        arrs = [np.ascontiguousarray(c, dtype=rd) for c in coeffs]
        n_coeffs = len(arrs) if n_coeffs is None else n_coeffs
        length = arrs[0].size if length is None else length
        coeff_blocks = self.B if coeff_blocks is None else coeff_blocks
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        return self._lib.bfir_engine_set_coeff_fade(self._h, ptrs, n_coeffs, length, coeff_blocks, float(scale),
                                                    int(fade_blocks))

    def fade_remaining(self):
        """Blocks of a pending or running fade still to be processed; 0 = none."""
        return self._lib.bfir_engine_fade_remaining(self._h)

    def run(self, inbuf, outbuf=None):
        """run(void *inbuf, void *outbuf) for every L-frame block in `inbuf`
        (host arrays).  inbuf: [n_blocks*L, C] (one engine) or
        [n_engines, n_blocks*L, C].  Returns (rc, outbuf)."""
        d_in = _FMT_DTYPES[self.in_format]
        x = np.ascontiguousarray(inbuf, dtype=np.uint8 if d_in is None else d_in)
        shape = x.shape[:-1] if d_in is None else x.shape        # 24-bit: [..., frames, C, 3]
        frames = shape[-2]
        assert shape[-1] == self.C and frames % self.L == 0
        assert int(np.prod(shape)) == self.n_engines * frames * self.C
        if outbuf is None:
            outbuf = raw_frames(self.out_format, shape)
        rc = self._lib.bfir_engine_run(self._h, x.ctypes.data, outbuf.ctypes.data, frames // self.L)
        return rc, outbuf

    def run_device(self, d_in, d_out, n_blocks, in_stride_bytes=0, out_stride_bytes=0, stream=None):
        """Asynchronous run on device pointers (ints).  Raises on a bad call;
        the NaN verdict comes from sync()."""
        rc = self._lib.bfir_engine_run_device(self._h, d_in, in_stride_bytes, d_out, out_stride_bytes,
                                              n_blocks, stream)
        if rc != 0:
            raise BfirError(rc, "bfir_engine_run_device")

    def sync(self):
        return self._lib.bfir_engine_sync(self._h)

    def reset(self):
        self._lib.bfir_engine_reset(self._h)

    def overflow(self, channel):
        of = Overflow()
        rc = self._lib.bfir_engine_get_overflow(self._h, channel, C.byref(of))
        if rc != 0:
            raise BfirError(rc, "bfir_engine_get_overflow")
        return of

    def check_overflows(self):
        """brutefir::check_overflows (brutefir.cpp:370-388): list of
        (channel, n_overflows, peak_dB) when any channel overflowed."""
        ofs = [self.overflow(n) for n in range(self.C * self.n_engines)]
        if not any(o.n_overflows for o in ofs):
            return []
        out = []
        for n, o in enumerate(ofs):
            peak = max(o.largest, float(o.intlargest))
            db = float("-inf") if peak == 0.0 else 20.0 * np.log10(peak / o.max)
            out.append((n, o.n_overflows, db))
        return out

    # -- per-channel delays (the reference's delay class, brutefir/delay.hpp) ----
    def _side_channels(self, side):
        return self.C if side == _lib.DELAY_INPUT else getattr(self, "n_out", self.C)

    def delay_init(self, side, max_delay, step_count=0, half_filter_length=0, kaiser_beta=9.0):
        """bfir_engine_delay_init: per-channel delays of up to max_delay frames on the input (side 0) or output (side 1)
        frames; step_count >= 2 adds the sub-sample stage (2 * half_filter_length + 1 tap filters, steps of 1 / step_count
        sample, half_filter_length frames of latency).  Returns 0 or an ERR_* code."""
        return self._lib.bfir_engine_delay_init(self._h, int(side), int(max_delay), int(step_count), int(half_filter_length),
                                                float(kaiser_beta))

    def set_delay(self, side, delay, subdelay=None):
        """bfir_engine_set_delay: delay[c] frames (and subdelay[c] steps) for every channel of the side, from the next block
        on, as a hard cut.  Returns 0 or an ERR_* code; a refused call changes nothing."""
        d = [int(v) for v in delay]
        sd = [0] * len(d) if subdelay is None else [int(v) for v in subdelay]
        assert len(sd) == len(d)
        n = len(d)
        return self._lib.bfir_engine_set_delay(self._h, int(side), (C.c_int * max(1, n))(*d), (C.c_int * max(1, n))(*sd), n)

    def get_delay(self, side):
        """(delays, subdelays) of the side as lists; raises on an error (a side never initialised: ERR_STATE)."""
        n = self._side_channels(side)
        d, sd = (C.c_int * n)(), (C.c_int * n)()
        rc = self._lib.bfir_engine_get_delay(self._h, int(side), d, sd, n)
        if rc != 0:
            raise BfirError(rc, "bfir_engine_get_delay")
        return list(d), list(sd)

    def delay_latency(self, side):
        """Frames of fixed latency the side's sub-sample stage adds (half_filter_length, or 0 without one)."""
        return self._lib.bfir_engine_delay_latency(self._h, int(side))

    # -- tuning / introspection --------------------------------------------
    def set_chunk(self, blocks_per_launch):
        rc = self._lib.bfir_engine_set_chunk(self._h, blocks_per_launch)
        if rc != 0:
            raise BfirError(rc, "bfir_engine_set_chunk")

    def set_profiling(self, on):
        self._lib.bfir_engine_set_profiling(self._h, int(bool(on)))

    def profile(self):
        """{kernel name: (total_ms, launches)} measured with HIP events."""
        out = {}
        for k, name in enumerate(_lib.KERNEL_NAMES):
            ms, n = C.c_double(0), C.c_int64(0)
            self._lib.bfir_engine_get_profile(self._h, k, C.byref(ms), C.byref(n))
            out[name] = (ms.value, n.value)
        return out

    def coeff_block(self, channel, block):
        dst = np.zeros(2 * self.L, dtype=_real_dtype(self.s))
        rc = self._lib.bfir_engine_read_coeff(self._h, channel, block, dst.ctypes.data)
        if rc != 0:
            raise BfirError(rc, "bfir_engine_read_coeff")
        return dst


class BrutefirBig(Brutefir):
    """Brutefir on long partitions (bfir_engine_create_big): filter_length 32768 ... 1048576 (realsize 8: from 16384), the
    lengths past one workgroup's transform.  One engine; everything else is Brutefir's -- every sample format, dither,
    set_coeff, set_coeff_fade, the delays, coeff_block in the reference's layout and natural bin order."""

    def __init__(self, filter_length, filter_blocks, realsize, channels,
                 in_format=None, out_format=None, sampling_rate=44100, apply_dither=False, device=0):
        dflt = SAMPLE_FORMAT_FLOAT_LE if realsize == 4 else SAMPLE_FORMAT_FLOAT64_LE
        self.L, self.B, self.s, self.C = filter_length, filter_blocks, realsize, channels
        self.in_format = dflt if in_format is None else in_format
        self.out_format = dflt if out_format is None else out_format
        self.n_engines, self.device = 1, device
        self.sampling_rate = sampling_rate
        self._lib = _lib.load()
        err = C.c_int(0)
        self._h = self._lib.bfir_engine_create_big(
            filter_length, filter_blocks, realsize, channels, self.in_format,
            self.out_format, sampling_rate, int(bool(apply_dither)), device, C.byref(err))
        if not self._h:
            raise BfirError(err.value, "bfir_engine_create_big")


class BrutefirMatrix(Brutefir):
    """n_in inputs -> n_out outputs with one filter per (output, input) pair (bfir_engine_create_matrix):
    y_o = sum_i h_{o,i} * x_i.  Frames are FLOAT_LE or FLOAT64_LE; the default is the working precision's.

    run / run_device / sync / reset / set_chunk / set_profiling / profile / close are Brutefir's; overflow(o) is
    output o's."""

    _create = "bfir_engine_create_matrix"   # the entry point of the kind (BrutefirMimo: the wider one)

    def __init__(self, filter_length, filter_blocks, realsize, n_in, n_out, in_format=None, out_format=None, device=0):
        dflt = SAMPLE_FORMAT_FLOAT_LE if realsize == 4 else SAMPLE_FORMAT_FLOAT64_LE
        self.L, self.B, self.s = filter_length, filter_blocks, realsize
        self.n_in, self.n_out = n_in, n_out
        self.C = n_in
        self.in_format = dflt if in_format is None else in_format
        self.out_format = dflt if out_format is None else out_format
        self.n_engines, self.device = 1, device
        self._lib = _lib.load()
        err = C.c_int(0)
        self._h = getattr(self._lib, self._create)(filter_length, filter_blocks, realsize, n_in, n_out,
                                                   self.in_format, self.out_format, device, C.byref(err))
        if not self._h:
            raise BfirError(err.value, self._create)

    def set_coeff(self, rows, length=None, coeff_blocks=None, scale=1.0):
        """rows[o][i]: taps of h_{o,i} (working precision) or None = no path from input i to output o.
        Returns 0 or ERR_COEFF (a NaN / Inf tap)."""
        assert len(rows) == self.n_out and all(len(r) == self.n_in for r in rows)
        rd = _real_dtype(self.s)
        arrs = [None if h is None else np.ascontiguousarray(h, dtype=rd) for r in rows for h in r]
        given = [a for a in arrs if a is not None]
        length = (given[0].size if given else 0) if length is None else length
        coeff_blocks = self.B if coeff_blocks is None else coeff_blocks
        ptrs = (C.c_void_p * len(arrs))(*[None if a is None else a.ctypes.data for a in arrs])
        return self._lib.bfir_engine_set_coeff_matrix(self._h, ptrs, length, coeff_blocks, float(scale))

    def set_coeff_fade(self, rows, fade_blocks, length=None, coeff_blocks=None, scale=1.0):
        """bfir_engine_set_coeff_matrix_fade: rows as set_coeff; a filter that is None in one set and present in the
        other fades in or out over the next `fade_blocks` blocks."""
        assert len(rows) == self.n_out and all(len(r) == self.n_in for r in rows)
        rd = _real_dtype(self.s)
        arrs = [None if h is None else np.ascontiguousarray(h, dtype=rd) for r in rows for h in r]
        given = [a for a in arrs if a is not None]
        length = (given[0].size if given else 0) if length is None else length
        coeff_blocks = self.B if coeff_blocks is None else coeff_blocks
        ptrs = (C.c_void_p * len(arrs))(*[None if a is None else a.ctypes.data for a in arrs])
        return self._lib.bfir_engine_set_coeff_matrix_fade(self._h, ptrs, length, coeff_blocks, float(scale),
                                                           int(fade_blocks))

    def _pair_args(self, pairs, filters, length, coeff_blocks):
        """The list arguments of the two pairs calls; the arrays are returned too, to keep them alive over the call."""
        assert len(pairs) == len(filters)
        rd = _real_dtype(self.s)
        arrs = [None if h is None else np.ascontiguousarray(h, dtype=rd) for h in filters]
        given = [a for a in arrs if a is not None]
        length = (given[0].size if given else 0) if length is None else length
        coeff_blocks = self.B if coeff_blocks is None else coeff_blocks
        assert all(a.size >= length for a in given), "every filter of a pairs call holds `length` taps"
        outs = (C.c_int * len(pairs))(*[int(o) for o, _ in pairs])
        ins = (C.c_int * len(pairs))(*[int(i) for _, i in pairs])
        ptrs = (C.c_void_p * len(arrs))(*[None if a is None else a.ctypes.data for a in arrs])
        return (len(pairs), outs, ins, ptrs, length, coeff_blocks), arrs

    def set_coeff_pairs(self, pairs, filters, length=None, coeff_blocks=None, scale=1.0):
        """bfir_engine_set_coeff_matrix_pairs: filters[k] (taps in working precision, or None = the path is removed)
        replaces h_{o,i} for pairs[k] = (o, i); every other pair keeps its filter.  Returns 0 or an ERR_* code."""
        args, _keep = self._pair_args(pairs, filters, length, coeff_blocks)
        return self._lib.bfir_engine_set_coeff_matrix_pairs(self._h, *args, float(scale))

    def set_coeff_pairs_fade(self, pairs, filters, fade_blocks, length=None, coeff_blocks=None, scale=1.0):
        """bfir_engine_set_coeff_matrix_pairs_fade: the same change, crossfaded over the next `fade_blocks` blocks."""
        args, _keep = self._pair_args(pairs, filters, length, coeff_blocks)
        return self._lib.bfir_engine_set_coeff_matrix_pairs_fade(self._h, *args, float(scale), int(fade_blocks))

    # A coefficient bank: filters transformed once and kept on the device, then named by index.  The calls below are
    # set_coeff / set_coeff_fade / set_coeff_pairs / set_coeff_pairs_fade with a bank index (or None = no path) in place
    # of every filter; they take no taps and copy rows on the device in one kernel launch.  On the multi-level classes the
    # library answers every one of these with ERR_UNSUPPORTED: their banks, one store per level, are the lbank_* methods and
    # set_bank / fade_to_rows_bank / set_pairs_bank / fade_to_pairs_bank of BrutefirMatrixLevels.

    def bank_create(self, n):
        """bfir_engine_bank_create: a bank of n empty entries on the engine's device.  Returns 0 or an ERR_* code
        (ERR_STATE: the engine has one)."""
        return self._lib.bfir_engine_bank_create(self._h, int(n))

    def bank_destroy(self):
        """bfir_engine_bank_destroy: frees the bank; the engine's active filters are copies and stay."""
        return self._lib.bfir_engine_bank_destroy(self._h)

    def bank_entries(self):
        """bfir_engine_bank_entries: the entry count, 0 without a bank (< 0: an ERR_* code)."""
        return self._lib.bfir_engine_bank_entries(self._h)

    def bank_blocks(self, entry):
        """bfir_engine_bank_blocks: the partition count entry `entry` was loaded with, 0 = empty (< 0: an ERR_* code)."""
        return self._lib.bfir_engine_bank_blocks(self._h, int(entry))

    def bank_load(self, first, filters, length=None, coeff_blocks=None, scale=1.0):
        """bfir_engine_bank_load: filters[k] (taps in working precision, or None = the entry becomes empty) into entry
        first + k, all in one upload and one transform launch; length / coeff_blocks / scale as set_coeff, and the entry's
        partition count is min(coeff_blocks, B).  Returns 0 or an ERR_* code (ERR_COEFF: a NaN / Inf tap, the bank is
        unchanged)."""
        rd = _real_dtype(self.s)
        arrs = [None if h is None else np.ascontiguousarray(h, dtype=rd) for h in filters]
        given = [a for a in arrs if a is not None]
        length = (given[0].size if given else 0) if length is None else length
        coeff_blocks = self.B if coeff_blocks is None else coeff_blocks
        assert all(a.size >= length for a in given), "every filter of a bank_load call holds `length` taps"
        ptrs = (C.c_void_p * max(1, len(arrs)))(*[None if a is None else a.ctypes.data for a in arrs])
        return self._lib.bfir_engine_bank_load(self._h, int(first), len(arrs), ptrs, length, coeff_blocks, float(scale))

    def bank_read(self, entry, block):
        """bfir_engine_bank_read: partition spectrum `block` of a bank entry, as coeff_block gives the engine's; zeros at
        and past the entry's partition count."""
        dst = np.zeros(2 * self.L, dtype=_real_dtype(self.s))
        rc = self._lib.bfir_engine_bank_read(self._h, int(entry), int(block), dst.ctypes.data)
        if rc != 0:
            raise BfirError(rc, "bfir_engine_bank_read")
        return dst

    @staticmethod
    def _bank_ints(entries):
        return (C.c_int * max(1, len(entries)))(*[-1 if en is None else int(en) for en in entries])

    def set_coeff_bank(self, rows):
        """bfir_engine_set_coeff_matrix_bank: rows[o][i] is the bank entry of h_{o,i}, or None = no path.  The engine is left
        as set_coeff with the entries' taps leaves it, every filter at its entry's partition count.  Returns 0 or an ERR_*
        code (ERR_STATE: no bank, or an empty entry)."""
        assert len(rows) == self.n_out and all(len(r) == self.n_in for r in rows)
        return self._lib.bfir_engine_set_coeff_matrix_bank(self._h, self._bank_ints([en for r in rows for en in r]))

    def set_coeff_bank_fade(self, rows, fade_blocks):
        """bfir_engine_set_coeff_matrix_bank_fade: set_coeff_fade to the set rows names, over the next `fade_blocks`
        blocks."""
        assert len(rows) == self.n_out and all(len(r) == self.n_in for r in rows)
        return self._lib.bfir_engine_set_coeff_matrix_bank_fade(self._h, self._bank_ints([en for r in rows for en in r]),
                                                                int(fade_blocks))

    def _pair_bank_args(self, pairs, entries):
        assert len(pairs) == len(entries)
        outs = (C.c_int * max(1, len(pairs)))(*[int(o) for o, _ in pairs])
        ins = (C.c_int * max(1, len(pairs)))(*[int(i) for _, i in pairs])
        return len(pairs), outs, ins, self._bank_ints(entries)

    def set_coeff_pairs_bank(self, pairs, entries):
        """bfir_engine_set_coeff_matrix_pairs_bank: bank entry entries[k] (or None = the path is removed) replaces h_{o,i}
        for pairs[k] = (o, i); every other pair keeps its filter.  Returns 0 or an ERR_* code."""
        return self._lib.bfir_engine_set_coeff_matrix_pairs_bank(self._h, *self._pair_bank_args(pairs, entries))

    def set_coeff_pairs_bank_fade(self, pairs, entries, fade_blocks):
        """bfir_engine_set_coeff_matrix_pairs_bank_fade: the same change, crossfaded over the next `fade_blocks` blocks."""
        return self._lib.bfir_engine_set_coeff_matrix_pairs_bank_fade(self._h, *self._pair_bank_args(pairs, entries),
                                                                      int(fade_blocks))

    # Bank mixes: a filter as a weighted sum of up to four bank entries, formed on the device while the rows are copied
    # (k_bank_mix).  `terms` holds, per listed row, a list of up to four (entry, weight) tuples, or None / [] = no path;
    # shorter lists are padded with (-1, 0.0) up to the call's longest.  One term of weight 1.0 is the bank call above.

    @staticmethod
    def _mix_args(terms):
        """(n_terms, entries, weights) of the C calls from per-row lists of (entry, weight)."""
        rows = [list(t) if t else [] for t in terms]
        n_terms = max([1] + [len(r) for r in rows])
        flat = [t for r in rows for t in r + [(-1, 0.0)] * (n_terms - len(r))]
        ents = (C.c_int * max(1, len(flat)))(*[-1 if en is None else int(en) for en, _ in flat])
        wts = (C.c_double * max(1, len(flat)))(*[float(w) for _, w in flat])
        return n_terms, ents, wts

    def set_coeff_bank_mix(self, terms):
        """bfir_engine_set_coeff_matrix_bank_mix: terms[o][i] is the list of (entry, weight) of h_{o,i}.  Every stored real is
        fl(w_1 h_1), then fl(. + fl(w_m h_m)) in listed order over the live terms (entry >= 0, weight != 0 in the working
        precision) whose entry reaches the partition; the filter's partition count is the largest among its live terms.
        Returns 0 or an ERR_* code."""
        assert len(terms) == self.n_out and all(len(r) == self.n_in for r in terms)
        return self._lib.bfir_engine_set_coeff_matrix_bank_mix(self._h, *self._mix_args([t for r in terms for t in r]))

    def set_coeff_bank_mix_fade(self, terms, fade_blocks):
        """bfir_engine_set_coeff_matrix_bank_mix_fade: set_coeff_fade to the mixed set, over the next `fade_blocks` blocks."""
        assert len(terms) == self.n_out and all(len(r) == self.n_in for r in terms)
        return self._lib.bfir_engine_set_coeff_matrix_bank_mix_fade(self._h, *self._mix_args([t for r in terms for t in r]),
                                                                    int(fade_blocks))

    def _pair_mix_args(self, pairs, terms):
        assert len(pairs) == len(terms)
        outs = (C.c_int * max(1, len(pairs)))(*[int(o) for o, _ in pairs])
        ins = (C.c_int * max(1, len(pairs)))(*[int(i) for _, i in pairs])
        return (len(pairs), outs, ins) + self._mix_args(terms)

    def set_coeff_pairs_bank_mix(self, pairs, terms):
        """bfir_engine_set_coeff_matrix_pairs_bank_mix: the mix terms[k] (None / [] = the path is removed) replaces h_{o,i}
        for pairs[k] = (o, i); every other pair keeps its filter.  Returns 0 or an ERR_* code."""
        return self._lib.bfir_engine_set_coeff_matrix_pairs_bank_mix(self._h, *self._pair_mix_args(pairs, terms))

    def set_coeff_pairs_bank_mix_fade(self, pairs, terms, fade_blocks):
        """bfir_engine_set_coeff_matrix_pairs_bank_mix_fade: the same change, crossfaded over the next `fade_blocks` blocks."""
        return self._lib.bfir_engine_set_coeff_matrix_pairs_bank_mix_fade(self._h, *self._pair_mix_args(pairs, terms),
                                                                          int(fade_blocks))

    def run(self, inbuf, outbuf=None):
        """inbuf: [n_blocks*L, n_in] frames in the input format.  Returns (rc, outbuf [n_blocks*L, n_out])."""
        x = np.ascontiguousarray(inbuf, dtype=_FMT_DTYPES[self.in_format])
        frames = x.shape[0]
        assert x.ndim == 2 and x.shape[1] == self.n_in and frames % self.L == 0
        if outbuf is None:
            outbuf = raw_frames(self.out_format, (frames, self.n_out))
        assert outbuf.shape == (frames, self.n_out) and outbuf.dtype == _FMT_DTYPES[self.out_format]
        rc = self._lib.bfir_engine_run(self._h, x.ctypes.data, outbuf.ctypes.data, frames // self.L)
        return rc, outbuf

    def check_overflows(self):
        ofs = [self.overflow(o) for o in range(self.n_out)]
        if not any(o.n_overflows for o in ofs):
            return []
        return [(n, o.n_overflows, float("-inf") if o.largest == 0.0 else 20.0 * np.log10(o.largest / o.max))
                for n, o in enumerate(ofs)]

    def coeff_block(self, output, input, block):
        dst = np.zeros(2 * self.L, dtype=_real_dtype(self.s))
        rc = self._lib.bfir_engine_read_coeff_matrix(self._h, output, input, block, dst.ctypes.data)
        if rc != 0:
            raise BfirError(rc, "bfir_engine_read_coeff_matrix")
        return dst


class BrutefirMimo(BrutefirMatrix):
    """BrutefirMatrix with up to 64 inputs and outputs (bfir_engine_create_mimo): the same methods, and the same bytes
    wherever both exist.  No delays: delay_init raises BfirError(ERR_UNSUPPORTED)."""

    _create = "bfir_engine_create_mimo"

    def delay_init(self, side, max_delay, step_count=0, half_filter_length=0, kaiser_beta=9.0):
        rc = super().delay_init(side, max_delay, step_count, half_filter_length, kaiser_beta)
        raise BfirError(rc, "bfir_engine_delay_init")


class BrutefirNup(Brutefir):
    """Two partition lengths in one engine (bfir_engine_create_nup): taps [0, D), D = head_blocks * filter_length, run on
    partitions of filter_length, the rest on tail_blocks partitions of tail_ratio * filter_length.  Same convolution, same
    zero latency and the same filter_length-frame blocks as Brutefir(filter_length, ceil(taps / filter_length), ...), with
    head_blocks + tail_blocks partitions of MAC work per sample instead.  head_blocks >= tail_ratio, a power of two >= 2.
    Frames are FLOAT_LE or FLOAT64_LE; the default is the working precision's.

    run / run_device / sync / reset / overflow / check_overflows / set_chunk / set_profiling / profile / close are
    Brutefir's; reset() discards all signal state (the engine then behaves as newly created with the same filters)."""

    def __init__(self, filter_length, head_blocks, tail_ratio, tail_blocks, realsize, channels, in_format=None,
                 out_format=None, device=0):
        dflt = SAMPLE_FORMAT_FLOAT_LE if realsize == 4 else SAMPLE_FORMAT_FLOAT64_LE
        self.L, self.B, self.s, self.C = filter_length, head_blocks, realsize, channels
        self.head_blocks, self.tail_ratio, self.tail_blocks = head_blocks, tail_ratio, tail_blocks
        self.D = head_blocks * filter_length
        self.max_taps = self.D + tail_blocks * tail_ratio * filter_length
        self.in_format = dflt if in_format is None else in_format
        self.out_format = dflt if out_format is None else out_format
        self.n_engines, self.device = 1, device
        self._lib = _lib.load()
        err = C.c_int(0)
        self._h = self._lib.bfir_engine_create_nup(filter_length, head_blocks, tail_ratio, tail_blocks, realsize, channels,
                                                   self.in_format, self.out_format, device, C.byref(err))
        if not self._h:
            raise BfirError(err.value, "bfir_engine_create_nup")

    def set_coeff(self, coeffs, scale=1.0):
        """coeffs[c]: the taps of channel c, at most max_taps of them; split at D between the two levels.
        Returns 0 or an ERR_* code (ERR_COEFF: a NaN / Inf tap, the engine is uninitialised)."""
        rd = _real_dtype(self.s)
        arrs = [np.ascontiguousarray(c, dtype=rd) for c in coeffs]
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        return self._lib.bfir_engine_set_coeff_nup(self._h, ptrs, len(arrs), arrs[0].size, float(scale))

    def set_coeff_fade(self, *args, **kwargs):
        raise BfirError(_lib.ERR_UNSUPPORTED, "bfir_engine_set_coeff_fade")

    def fade_to(self, coeffs, fade_blocks, scale=1.0):
        """bfir_engine_set_coeff_nup_fade: fade to coeffs (as set_coeff takes them) over the next `fade_blocks` blocks of filter_length
        frames, every level consistently (the ramp of fftw_convolver::convolver_crossfade_inplace).  Returns 0 or an ERR_*
        code: ERR_COEFF (a NaN / Inf tap) leaves the engine running the old filters, ERR_UNSUPPORTED means the new set reaches
        a level the old one does not (load the first set zero-padded to the longest length that will be faded to)."""
        rd = _real_dtype(self.s)
        arrs = [np.ascontiguousarray(c, dtype=rd) for c in coeffs]
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        return self._lib.bfir_engine_set_coeff_nup_fade(self._h, ptrs, len(arrs), arrs[0].size, float(scale), int(fade_blocks))

    def fade_remaining(self):
        """Head blocks of a pending or running fade_to still to be processed; 0 = none."""
        return self._lib.bfir_engine_fade_remaining_levels(self._h)

    def coeff_block(self, level, channel, block):
        """Partition spectrum `block` of `channel` on level 0 (head, 2 L reals) or 1 (tail, 2 tail_ratio L reals)."""
        n = 2 * self.L * (self.tail_ratio if level else 1)
        dst = np.zeros(n, dtype=_real_dtype(self.s))
        rc = self._lib.bfir_engine_read_coeff_nup(self._h, level, channel, block, dst.ctypes.data)
        if rc != 0:
            raise BfirError(rc, "bfir_engine_read_coeff_nup")
        return dst


class BrutefirLevels(Brutefir):
    """Three or four partition lengths in one engine (bfir_engine_create_levels): level k has blocks[k] partitions of
    L_k = ratios[k] * L_(k-1) (L_0 = filter_length, ratios[0] = 1, the others powers of two >= 2) and convolves taps
    [D[k], D[k + 1]), D[0] = 0 and D[k + 1] = D[k] + blocks[k] * L_k; D[k] >= L_k for k >= 1.  Same convolution, same zero
    latency and the same filter_length-frame blocks as Brutefir(filter_length, ceil(taps / filter_length), ...), with
    sum(blocks) partitions of MAC work per sample instead.  Two levels are allowed and give BrutefirNup's bytes.
    Frames are FLOAT_LE or FLOAT64_LE; the default is the working precision's.

    run / run_device / sync / reset / overflow / check_overflows / set_chunk / set_profiling / profile / close are
    Brutefir's; reset() discards all signal state of all levels."""

    def __init__(self, filter_length, blocks, ratios, realsize, channels, in_format=None, out_format=None, device=0):
        dflt = SAMPLE_FORMAT_FLOAT_LE if realsize == 4 else SAMPLE_FORMAT_FLOAT64_LE
        blocks, ratios = [int(b) for b in blocks], [int(r) for r in ratios]
        assert len(blocks) == len(ratios)
        self.L, self.B, self.s, self.C = filter_length, blocks[0] if blocks else 0, realsize, channels
        self.blocks, self.ratios = tuple(blocks), tuple(ratios)
        self.lengths, self.D = [], [0]
        for b, r in zip(blocks, ratios):
            self.lengths.append(filter_length if not self.lengths else self.lengths[-1] * r)
            self.D.append(self.D[-1] + b * self.lengths[-1])
        self.max_taps = self.D.pop()
        self.in_format = dflt if in_format is None else in_format
        self.out_format = dflt if out_format is None else out_format
        self.n_engines, self.device = 1, device
        self._lib = _lib.load()
        err = C.c_int(0)
        n = len(blocks)
        self._h = self._lib.bfir_engine_create_levels(filter_length, n, (C.c_int * n)(*blocks), (C.c_int * n)(*ratios), realsize,
                                                      channels, self.in_format, self.out_format, device, C.byref(err))
        if not self._h:
            raise BfirError(err.value, "bfir_engine_create_levels")

    def set_coeff(self, coeffs, scale=1.0):
        """coeffs[c]: the taps of channel c, at most max_taps of them; split at every D[k] between the levels.
        Returns 0 or an ERR_* code (ERR_COEFF: a NaN / Inf tap, the engine is uninitialised)."""
        rd = _real_dtype(self.s)
        arrs = [np.ascontiguousarray(c, dtype=rd) for c in coeffs]
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        return self._lib.bfir_engine_set_coeff_levels(self._h, ptrs, len(arrs), arrs[0].size, float(scale))

    def set_coeff_fade(self, *args, **kwargs):
        raise BfirError(_lib.ERR_UNSUPPORTED, "bfir_engine_set_coeff_fade")

    def fade_to(self, coeffs, fade_blocks, scale=1.0):
        """bfir_engine_set_coeff_levels_fade: fade to coeffs (as set_coeff takes them) over the next `fade_blocks` blocks of filter_length
        frames, every level consistently (the ramp of fftw_convolver::convolver_crossfade_inplace).  Returns 0 or an ERR_*
        code: ERR_COEFF (a NaN / Inf tap) leaves the engine running the old filters, ERR_UNSUPPORTED means the new set reaches
        a level the old one does not (load the first set zero-padded to the longest length that will be faded to)."""
        rd = _real_dtype(self.s)
        arrs = [np.ascontiguousarray(c, dtype=rd) for c in coeffs]
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        return self._lib.bfir_engine_set_coeff_levels_fade(self._h, ptrs, len(arrs), arrs[0].size, float(scale), int(fade_blocks))

    def fade_remaining(self):
        """Head blocks of a pending or running fade_to still to be processed; 0 = none."""
        return self._lib.bfir_engine_fade_remaining_levels(self._h)

    def coeff_block(self, level, channel, block):
        """Partition spectrum `block` of `channel` on `level`: 2 L_level reals."""
        n = 2 * self.lengths[level] if 0 <= level < len(self.lengths) else 2 * self.L
        dst = np.zeros(n, dtype=_real_dtype(self.s))
        rc = self._lib.bfir_engine_read_coeff_levels(self._h, level, channel, block, dst.ctypes.data)
        if rc != 0:
            raise BfirError(rc, "bfir_engine_read_coeff_levels")
        return dst


class BrutefirMatrixLevels(BrutefirMatrix):
    """BrutefirMatrix on the partition lengths of BrutefirLevels (bfir_engine_create_matrix_levels): n_in inputs -> n_out
    outputs, one filter per (output, input) pair, every filter split at every D[k] between two to four levels -- long
    impulse responses in a crossover, room-correction or reverb matrix at a short block length, with sum(blocks)
    partitions of MAC work per pair and sample instead of ceil(taps / filter_length).  blocks, ratios, lengths, D and
    max_taps are BrutefirLevels'.  Frames are FLOAT_LE or FLOAT64_LE; the default is the working precision's.

    run / run_device / sync / reset / overflow / check_overflows / set_chunk / set_profiling / profile / close are
    BrutefirMatrix's; reset() discards all signal state of all levels.  The crossfade of this kind is fade_to_rows."""

    _create = "bfir_engine_create_matrix_levels"   # the entry point of the kind (BrutefirMimoLevels: the wider one)

    def __init__(self, filter_length, blocks, ratios, realsize, n_in, n_out, in_format=None, out_format=None, device=0):
        dflt = SAMPLE_FORMAT_FLOAT_LE if realsize == 4 else SAMPLE_FORMAT_FLOAT64_LE
        blocks, ratios = [int(b) for b in blocks], [int(r) for r in ratios]
        assert len(blocks) == len(ratios)
        self.L, self.B, self.s = filter_length, blocks[0] if blocks else 0, realsize
        self.n_in, self.n_out = n_in, n_out
        self.C = n_in
        self.blocks, self.ratios = tuple(blocks), tuple(ratios)
        self.lengths, self.D, self.max_taps = self.geometry(filter_length, blocks, ratios)
        self.in_format = dflt if in_format is None else in_format
        self.out_format = dflt if out_format is None else out_format
        self.n_engines, self.device = 1, device
        self._lib = _lib.load()
        err = C.c_int(0)
        n = len(blocks)
        self._h = getattr(self._lib, self._create)(filter_length, n, (C.c_int * max(1, n))(*blocks),
                                                   (C.c_int * max(1, n))(*ratios), realsize, n_in, n_out, self.in_format,
                                                   self.out_format, device, C.byref(err))
        if not self._h:
            raise BfirError(err.value, self._create)

    @staticmethod
    def geometry(filter_length, blocks, ratios):
        """([L_k], [D_k], capacity in taps) of the levels, as BrutefirLevels keeps them in lengths, D and max_taps."""
        lengths, D = [], [0]
        for b, r in zip(blocks, ratios):
            lengths.append(filter_length if not lengths else lengths[-1] * r)
            D.append(D[-1] + b * lengths[-1])
        return lengths, D[:-1], D[-1]

    def set_coeff(self, rows, scale=1.0):
        """rows[o][i]: the taps of h_{o,i} (working precision), each of its own length up to max_taps, or None = no path
        from input i to output o.  Returns 0 or an ERR_* code (ERR_COEFF: a NaN / Inf tap, the engine is uninitialised)."""
        assert len(rows) == self.n_out and all(len(r) == self.n_in for r in rows)
        rd = _real_dtype(self.s)
        arrs = [None if h is None else np.ascontiguousarray(h, dtype=rd) for r in rows for h in r]
        ptrs = (C.c_void_p * len(arrs))(*[None if a is None else a.ctypes.data for a in arrs])
        lens = (C.c_int * len(arrs))(*[0 if a is None else a.size for a in arrs])
        return self._lib.bfir_engine_set_coeff_matrix_levels(self._h, ptrs, lens, float(scale))

    def set_coeff_fade(self, *args, **kwargs):
        raise BfirError(_lib.ERR_UNSUPPORTED, "bfir_engine_set_coeff_fade")

    def fade_to(self, *args, **kwargs):
        raise BfirError(_lib.ERR_UNSUPPORTED, "bfir_engine_set_coeff_levels_fade")

    def fade_to_rows(self, rows, fade_blocks, scale=1.0):
        """bfir_engine_set_coeff_matrix_levels_fade: fade to rows (as set_coeff takes them: per-filter lengths, None = no
        path) over the next `fade_blocks` blocks of filter_length frames, every level and every output consistently (the ramp
        of fftw_convolver::convolver_crossfade_inplace).  A filter that is None or shorter in one set fades in or out.
        Returns 0 or an ERR_* code: ERR_COEFF (a NaN / Inf tap) leaves the engine running the old filters, ERR_UNSUPPORTED
        means the new set has taps on a level on which no filter of the old set has any (load the first set zero-padded).
        fade_to and set_coeff_fade, the calls of the other kinds, keep raising ERR_UNSUPPORTED on this class."""
        assert len(rows) == self.n_out and all(len(r) == self.n_in for r in rows)
        rd = _real_dtype(self.s)
        arrs = [None if h is None else np.ascontiguousarray(h, dtype=rd) for r in rows for h in r]
        ptrs = (C.c_void_p * len(arrs))(*[None if a is None else a.ctypes.data for a in arrs])
        lens = (C.c_int * len(arrs))(*[0 if a is None else a.size for a in arrs])
        return self._lib.bfir_engine_set_coeff_matrix_levels_fade(self._h, ptrs, lens, float(scale), int(fade_blocks))

    def _level_pair_args(self, pairs, filters):
        """The list arguments of set_pairs / fade_to_pairs; the arrays are returned too, to keep them alive over the call."""
        assert len(pairs) == len(filters)
        rd = _real_dtype(self.s)
        arrs = [None if h is None else np.ascontiguousarray(h, dtype=rd) for h in filters]
        outs = (C.c_int * len(pairs))(*[int(o) for o, _ in pairs])
        ins = (C.c_int * len(pairs))(*[int(i) for _, i in pairs])
        ptrs = (C.c_void_p * len(arrs))(*[None if a is None else a.ctypes.data for a in arrs])
        lens = (C.c_int * len(arrs))(*[0 if a is None else a.size for a in arrs])
        return (len(pairs), outs, ins, ptrs, lens), arrs

    def set_pairs(self, pairs, filters, scale=1.0):
        """bfir_engine_set_coeff_matrix_levels_pairs: filters[k] (taps in working precision, each of its own length up to
        max_taps, or None = the path is removed) replaces h_{o,i} for pairs[k] = (o, i); every other pair keeps its filter
        on every level.  Returns 0 or an ERR_* code (ERR_STATE while a fade is pending or running).  The inherited
        set_coeff_pairs / set_coeff_pairs_fade, the calls of the uniform kinds, keep returning ERR_UNSUPPORTED."""
        args, _keep = self._level_pair_args(pairs, filters)
        return self._lib.bfir_engine_set_coeff_matrix_levels_pairs(self._h, *args, float(scale))

    def fade_to_pairs(self, pairs, filters, fade_blocks, scale=1.0):
        """bfir_engine_set_coeff_matrix_levels_pairs_fade: the same change, crossfaded over the next `fade_blocks` blocks as
        fade_to_rows fades to the merged set; the fading blocks agree with that fade within rounding, not bitwise."""
        args, _keep = self._level_pair_args(pairs, filters)
        return self._lib.bfir_engine_set_coeff_matrix_levels_pairs_fade(self._h, *args, float(scale), int(fade_blocks))

    # The bank of a multi-level engine: one store per level, every filter transformed once through the level split and then
    # named by index.  set_bank / fade_to_rows_bank / set_pairs_bank / fade_to_pairs_bank are set_coeff / fade_to_rows /
    # set_pairs / fade_to_pairs with a bank index (or None = no path) in place of every filter; they take no taps and copy
    # the rows of all levels on the device in one kernel launch.

    def lbank_create(self, n):
        """bfir_engine_levels_bank_create: a bank of n empty entries, a store on every level.  Returns 0 or an ERR_* code
        (ERR_STATE: the engine has one)."""
        return self._lib.bfir_engine_levels_bank_create(self._h, int(n))

    def lbank_destroy(self):
        """bfir_engine_levels_bank_destroy: frees the bank; the engine's active filters are copies and stay."""
        return self._lib.bfir_engine_levels_bank_destroy(self._h)

    def lbank_entries(self):
        """bfir_engine_levels_bank_entries: the entry count, 0 without a bank (< 0: an ERR_* code)."""
        return self._lib.bfir_engine_levels_bank_entries(self._h)

    def lbank_length(self, entry):
        """bfir_engine_levels_bank_length: the taps entry `entry` was loaded with, 0 = empty (< 0: an ERR_* code)."""
        return self._lib.bfir_engine_levels_bank_length(self._h, int(entry))

    def lbank_blocks(self, entry, level):
        """bfir_engine_levels_bank_blocks: the entry's partition count on `level` (< 0: an ERR_* code)."""
        return self._lib.bfir_engine_levels_bank_blocks(self._h, int(entry), int(level))

    def lbank_load(self, first, filters, scale=1.0):
        """bfir_engine_levels_bank_load: filters[k] (taps in working precision, each of its own length up to max_taps as
        set_coeff takes them, or None = the entry becomes empty) into entry first + k, split between the levels, one upload
        and one transform launch per level.  Returns 0 or an ERR_* code (ERR_COEFF: a NaN / Inf tap, the bank is unchanged)."""
        rd = _real_dtype(self.s)
        arrs = [None if h is None else np.ascontiguousarray(h, dtype=rd) for h in filters]
        ptrs = (C.c_void_p * max(1, len(arrs)))(*[None if a is None else a.ctypes.data for a in arrs])
        lens = (C.c_int * max(1, len(arrs)))(*[0 if a is None else a.size for a in arrs])
        return self._lib.bfir_engine_levels_bank_load(self._h, int(first), len(arrs), ptrs, lens, float(scale))

    def lbank_read(self, entry, level, block):
        """bfir_engine_levels_bank_read: partition spectrum `block` of a bank entry on `level`, as coeff_block gives the
        engine's; zeros at and past the entry's partition count there."""
        n = 2 * self.lengths[level] if 0 <= level < len(self.lengths) else 2 * self.L
        dst = np.zeros(n, dtype=_real_dtype(self.s))
        rc = self._lib.bfir_engine_levels_bank_read(self._h, int(entry), int(level), int(block), dst.ctypes.data)
        if rc != 0:
            raise BfirError(rc, "bfir_engine_levels_bank_read")
        return dst

    def set_bank(self, rows):
        """bfir_engine_set_coeff_matrix_levels_bank: rows[o][i] is the bank entry of h_{o,i}, or None = no path.  The engine
        is left as set_coeff with the entries' taps leaves it.  Returns 0 or an ERR_* code (ERR_STATE: no bank, or an empty
        entry)."""
        assert len(rows) == self.n_out and all(len(r) == self.n_in for r in rows)
        return self._lib.bfir_engine_set_coeff_matrix_levels_bank(self._h, self._bank_ints([en for r in rows for en in r]))

    def fade_to_rows_bank(self, rows, fade_blocks):
        """bfir_engine_set_coeff_matrix_levels_bank_fade: fade_to_rows to the set rows names."""
        assert len(rows) == self.n_out and all(len(r) == self.n_in for r in rows)
        return self._lib.bfir_engine_set_coeff_matrix_levels_bank_fade(
            self._h, self._bank_ints([en for r in rows for en in r]), int(fade_blocks))

    def set_pairs_bank(self, pairs, entries):
        """bfir_engine_set_coeff_matrix_levels_pairs_bank: bank entry entries[k] (or None = the path is removed) replaces
        h_{o,i} for pairs[k] = (o, i) on every level; every other pair keeps its filter.  Returns 0 or an ERR_* code
        (ERR_STATE while a fade is pending or running)."""
        return self._lib.bfir_engine_set_coeff_matrix_levels_pairs_bank(self._h, *self._pair_bank_args(pairs, entries))

    def fade_to_pairs_bank(self, pairs, entries, fade_blocks):
        """bfir_engine_set_coeff_matrix_levels_pairs_bank_fade: the same change, crossfaded as fade_to_pairs."""
        return self._lib.bfir_engine_set_coeff_matrix_levels_pairs_bank_fade(self._h, *self._pair_bank_args(pairs, entries),
                                                                             int(fade_blocks))

    # Mixes over the levels bank: set_bank / fade_to_rows_bank / set_pairs_bank / fade_to_pairs_bank with, per row, a list of
    # up to four (entry, weight) tuples (or None / [] = no path) in place of one entry, as set_coeff_bank_mix takes them.  The
    # sums are formed on the device on every level in one kernel launch (k_lbank_mix); one term of weight 1.0 is the bank
    # call.  The inherited set_coeff_bank_mix* methods, the calls of the uniform kinds, keep returning ERR_UNSUPPORTED.

    def set_bank_mix(self, terms):
        """bfir_engine_set_coeff_matrix_levels_bank_mix: terms[o][i] is the list of (entry, weight) of h_{o,i}.  On every
        level every stored real is fl(w_1 h_1), then fl(. + fl(w_m h_m)) in listed order over the live terms (entry >= 0,
        weight != 0 in the working precision) whose entry reaches the partition; the filter's partition count on a level is
        the largest among its live terms there.  Returns 0 or an ERR_* code."""
        assert len(terms) == self.n_out and all(len(r) == self.n_in for r in terms)
        return self._lib.bfir_engine_set_coeff_matrix_levels_bank_mix(self._h, *self._mix_args([t for r in terms for t in r]))

    def fade_to_rows_bank_mix(self, terms, fade_blocks):
        """bfir_engine_set_coeff_matrix_levels_bank_mix_fade: fade_to_rows to the mixed set."""
        assert len(terms) == self.n_out and all(len(r) == self.n_in for r in terms)
        return self._lib.bfir_engine_set_coeff_matrix_levels_bank_mix_fade(
            self._h, *self._mix_args([t for r in terms for t in r]), int(fade_blocks))

    def set_pairs_bank_mix(self, pairs, terms):
        """bfir_engine_set_coeff_matrix_levels_pairs_bank_mix: the mix terms[k] (None / [] = the path is removed) replaces
        h_{o,i} for pairs[k] = (o, i) on every level; every other pair keeps its filter.  Returns 0 or an ERR_* code
        (ERR_STATE while a fade is pending or running)."""
        return self._lib.bfir_engine_set_coeff_matrix_levels_pairs_bank_mix(self._h, *self._pair_mix_args(pairs, terms))

    def fade_to_pairs_bank_mix(self, pairs, terms, fade_blocks):
        """bfir_engine_set_coeff_matrix_levels_pairs_bank_mix_fade: the same change, crossfaded as fade_to_pairs."""
        return self._lib.bfir_engine_set_coeff_matrix_levels_pairs_bank_mix_fade(self._h, *self._pair_mix_args(pairs, terms),
                                                                                 int(fade_blocks))

    def fade_remaining(self):
        """Head blocks of a pending or running fade_to_rows / fade_to_pairs still to be processed; 0 = none."""
        return self._lib.bfir_engine_fade_remaining_levels(self._h)

    def coeff_block(self, level, output, input, block):
        """Partition spectrum `block` of h_{output,input} on `level`: 2 L_level reals."""
        n = 2 * self.lengths[level] if 0 <= level < len(self.lengths) else 2 * self.L
        dst = np.zeros(n, dtype=_real_dtype(self.s))
        rc = self._lib.bfir_engine_read_coeff_matrix_levels(self._h, level, output, input, block, dst.ctypes.data)
        if rc != 0:
            raise BfirError(rc, "bfir_engine_read_coeff_matrix_levels")
        return dst


class BrutefirMimoLevels(BrutefirMatrixLevels):
    """BrutefirMatrixLevels with up to 64 inputs and outputs (bfir_engine_create_mimo_levels): the same methods, and the
    same bytes wherever both exist.  No delays: delay_init raises BfirError(ERR_UNSUPPORTED)."""

    _create = "bfir_engine_create_mimo_levels"

    def delay_init(self, side, max_delay, step_count=0, half_filter_length=0, kaiser_beta=9.0):
        rc = super().delay_init(side, max_delay, step_count, half_filter_length, kaiser_beta)
        raise BfirError(rc, "bfir_engine_delay_init")
