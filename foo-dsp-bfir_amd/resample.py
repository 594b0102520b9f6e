"""Sampling-rate conversion of an impulse response on the GPU (csrc/resample.hip): band-limited interpolation on the exact
rational grid out_rate / in_rate = p / q, a Kaiser-windowed sinc of K taps for each of the p phases.  The definition is in
include/bfir_hip.h; this is the arithmetic buffer::resample_snd_file (brutefir/buffer.cpp:225-330) hands to libsamplerate."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import BfirError

# the defaults of the file mirror (buffer.resample_snd_file): they preserve the waveform, as libsamplerate does
ZERO_CROSSINGS, KAISER_BETA, CUTOFF, GAIN = 64, 9.0, 0.95, 1.0


def _real_dtype(realsize):
    return np.float32 if realsize == 4 else np.float64


def resample_taps(in_rate, out_rate, zero_crossings=ZERO_CROSSINGS, kaiser_beta=KAISER_BETA, cutoff=CUTOFF, gain=GAIN,
                  realsize=8):
    """K, the taps per phase (bfir_resample_filter with taps == NULL).  Host arithmetic: no device needed."""
    k = C.c_int(0)
    rc = _lib.load().bfir_resample_filter(int(in_rate), int(out_rate), int(zero_crossings), float(kaiser_beta), float(cutoff),
                                          float(gain), int(realsize), 0, None, C.byref(k))
    if rc != 0:
        raise BfirError(rc, "bfir_resample_filter")
    return k.value


def resample_filter(in_rate, out_rate, phase, zero_crossings=ZERO_CROSSINGS, kaiser_beta=KAISER_BETA, cutoff=CUTOFF, gain=GAIN,
                    realsize=8):
    """bfir_resample_filter: the K taps of one phase, 0 <= phase < p, rounded once to realsize precision; tap j meets input
    frame n0 - K / 2 + 1 + j.  Host arithmetic: no device needed."""
    k = resample_taps(in_rate, out_rate, zero_crossings, kaiser_beta, cutoff, gain, realsize)
    taps = np.zeros(k, dtype=_real_dtype(realsize))
    rc = _lib.load().bfir_resample_filter(int(in_rate), int(out_rate), int(zero_crossings), float(kaiser_beta), float(cutoff),
                                          float(gain), int(realsize), int(phase), taps.ctypes.data, None)
    if rc != 0:
        raise BfirError(rc, "bfir_resample_filter")
    return taps


class Resampler:
    """bfir_resampler: the phase table resident on the device, for interleaved [frames, channels] float32 (realsize 4) or
    float64 (realsize 8) frames.  Raises BfirError (ERR_NO_DEVICE without a GPU: there is no CPU stand-in)."""

    def __init__(self, in_rate, out_rate, zero_crossings=ZERO_CROSSINGS, kaiser_beta=KAISER_BETA, cutoff=CUTOFF, gain=GAIN,
                 realsize=4, channels=1, device=0):
        self._lib = _lib.load()
        self.realsize, self.channels = realsize, channels
        err = C.c_int(0)
        self._h = self._lib.bfir_resampler_create(int(in_rate), int(out_rate), int(zero_crossings), float(kaiser_beta),
                                                  float(cutoff), float(gain), int(realsize), int(channels), int(device),
                                                  C.byref(err))
        if not self._h:
            raise BfirError(err.value, "bfir_resampler_create")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bfir_resampler_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def out_frames(self, n_in):
        """ceil(n_in p / q)."""
        n = self._lib.bfir_resampler_out_frames(self._h, int(n_in))
        if n < 0:
            raise BfirError(int(n), "bfir_resampler_out_frames")
        return n

    def run(self, frames, max_out=None, out=None):
        """frames: [n_in, channels] host array -> the first min(max_out, n_out) converted frames, [n, channels]."""
        x = np.ascontiguousarray(frames, dtype=_real_dtype(self.realsize))
        assert x.ndim == 2 and x.shape[1] == self.channels
        n = self.out_frames(x.shape[0])
        n = n if max_out is None else min(n, int(max_out))
        if out is None:
            out = np.zeros((n, self.channels), x.dtype)
        assert out.dtype == x.dtype and out.flags.c_contiguous and out.size >= n * self.channels
        got = self._lib.bfir_resampler_run(self._h, x.ctypes.data, x.shape[0], out.ctypes.data, n)
        if got < 0:
            raise BfirError(int(got), "bfir_resampler_run")
        assert got == n
        return out

    def run_device(self, d_in, n_in, d_out, max_out):
        """The same on device pointers (ints), queued on the device's null stream; returns the frames it writes."""
        got = self._lib.bfir_resampler_run_device(self._h, d_in, int(n_in), d_out, int(max_out))
        if got < 0:
            raise BfirError(int(got), "bfir_resampler_run_device")
        return got
