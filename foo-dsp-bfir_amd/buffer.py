"""Host-side mirror of the reference's `namespace buffer` (brutefir/buffer.hpp, buffer.cpp:23-443) and of
coeff::load_snd_coeff (coeff.cpp:245-277): sound files in and out of interleaved buffers, and the conversion of an impulse
file to the stream's sampling rate on the GPU (resample.Resampler), cached as the reference caches it.

Files go through wavio: RIFF/WAVE only, other containers are refused (a failed call, not an exception).

Two deviations from the reference, both in resample_snd_file:
  * ratio direction -- the reference sets src_ratio = file rate / target rate (buffer.cpp:299), which libsamplerate reads
    as output rate / input rate: it converts the wrong way.  Here the file is converted from its own rate to the target.
  * output length -- the reference caps the output at the source's frame count (buffer.cpp:292-298), which cuts an
    up-converted impulse short.  Here all ceil(n p / q) frames are written.
Because of both, a cache directory must not be shared with the reference for ir- files."""
import os

import numpy as np

from . import resample, wavio
from ._lib import BfirError
from .equalizer import djb_hash


def _dtype(realsize):
    return np.float32 if realsize == 4 else np.float64


def _read(filename):
    try:
        return wavio.read_wav(os.fspath(filename))
    except Exception:          # unreadable, another container, a truncated header: the reference's sf_open fails
        return None


def get_snd_file_params(filename):
    """buffer.cpp:152-177: (n_channels, n_frames, sampling_rate), or None where the file cannot be read."""
    got = _read(filename)
    if got is None:
        return None
    frames, rate = got
    return frames.shape[1], frames.shape[0], rate


def check_snd_file(filename, n_channels, sampling_rate):
    """buffer.cpp:190-211: the file has exactly this many channels and this sampling rate."""
    params = get_snd_file_params(filename)
    return params is not None and params[0] == n_channels and params[2] == sampling_rate


def load_from_snd_file(filename, realsize, max_frames=-1, pad=False):
    """buffer.cpp:37-95: (buffer [rows, n_channels] in realsize precision, n_frames), or None.  n_frames is the file's frame
    count, or max_frames where the file has more (-1: no limit); rows is n_frames, or max_frames when `pad` (the rest zero,
    buffer.cpp:60-71)."""
    got = _read(filename)
    if got is None or (pad and max_frames < 0):
        return None
    frames = got[0]
    n_frames = frames.shape[0] if max_frames == -1 else min(int(max_frames), frames.shape[0])
    if n_frames < 0:
        return None
    buf = np.zeros((int(max_frames) if pad else n_frames, frames.shape[1]), _dtype(realsize))
    buf[:n_frames] = frames[:n_frames]
    return buf, n_frames


def save_to_snd_file(filename, buffer, realsize, sampling_rate):
    """buffer.cpp:106-139: interleaved [n_frames, n_channels] -> WAV, IEEE float (realsize 4) or double (8), little endian.
    Like the reference's it reports nothing."""
    try:
        wavio.write_wav_float(os.fspath(filename), np.ascontiguousarray(buffer, dtype=_dtype(realsize)), int(sampling_rate))
    except OSError:
        pass


def deinterlace(buffer):
    """buffer.cpp:343-384: [n_frames, n_channels] -> one contiguous array per channel."""
    b = np.asarray(buffer)
    return [np.ascontiguousarray(b[:, c]) for c in range(b.shape[1])]


def interlace(buffers, n_channels=None):
    """buffer.cpp:397-443: the first n_channels (default: all) per-channel arrays -> [n_frames, n_channels]."""
    bufs = list(buffers)[:n_channels]
    return np.ascontiguousarray(np.stack(bufs, axis=1))


def load_snd_coeff(filename, realsize, max_length):
    """coeff::load_snd_coeff (coeff.cpp:245-277): (one array per channel, length), at most max_length frames; or None."""
    got = load_from_snd_file(filename, realsize, max_length, False)
    if got is None:
        return None
    buf, n_frames = got
    return deinterlace(buf), n_frames


def cache_name(filename, n_channels, sampling_rate):
    """buffer.cpp:243-251: ir-<hex DJB hash of the file name's bytes>-<channels>-<rate>.wav."""
    raw = bytes(filename) if isinstance(filename, (bytes, bytearray)) else os.fsencode(os.fspath(filename))
    return "ir-%x-%d-%d.wav" % (djb_hash(raw), n_channels, sampling_rate)


def resample_snd_file(filename, n_channels, sampling_rate, cache_dir, zero_crossings=resample.ZERO_CROSSINGS,
                      kaiser_beta=resample.KAISER_BETA, cutoff=resample.CUTOFF, gain=resample.GAIN, device=0):
    """buffer.cpp:225-330: the file's first n_channels channels at `sampling_rate`, as a float WAV in cache_dir; returns its
    path, or "" on failure.  An existing cache file is reused untouched; a file with fewer channels than asked is refused;
    the conversion runs in realsize 4, as the reference's does.  The defaults preserve the waveform; a caller who wants the
    filter's frequency response preserved instead passes gain = file rate / sampling_rate."""
    dst = os.path.join(os.fspath(cache_dir), cache_name(filename, n_channels, sampling_rate))
    if os.path.exists(dst):
        return dst
    realsize = 4
    params = get_snd_file_params(filename)
    if params is None or params[0] < n_channels:
        return ""
    got = load_from_snd_file(filename, realsize, -1, False)
    if got is None:
        return ""
    src = got[0]
    if src.shape[1] > n_channels:                      # deinterlace, re-interlace without the extra channels (:280-289)
        src = interlace(deinterlace(src), n_channels)
    try:
        r = resample.Resampler(params[2], sampling_rate, zero_crossings, kaiser_beta, cutoff, gain, realsize, n_channels, device)
        try:
            out = r.run(src)
        finally:
            r.close()
    except BfirError:
        return ""
    try:
        wavio.write_wav_float(dst, out, int(sampling_rate))
    except OSError:
        return ""
    return dst
