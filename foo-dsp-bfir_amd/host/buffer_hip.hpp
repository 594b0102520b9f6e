// buffer_hip.hpp -- the reference's namespace buffer (brutefir/buffer.hpp, buffer.cpp:23-443): sound files in and out of
// interleaved buffers, and the conversion of an impulse file to the stream's sampling rate, on the GPU (bfir_resampler,
// include/bfir_hip.h) where the reference calls libsamplerate.  File names are narrow strings (the reference narrows its
// wchar_t names with util::wstr2str before hashing them, buffer.cpp:244).  Files go through wav_io: RIFF/WAVE with IEEE
// float samples only, other containers are refused.  Buffers come from bfir_aligned_malloc; the caller frees them with
// bfir_aligned_free, as the reference frees its own with _aligned_free.
//
// Two deviations from the reference, both in resample_snd_file:
//   * ratio direction -- the reference sets src_ratio = file rate / target rate (buffer.cpp:299), which libsamplerate reads
//     as output rate / input rate: it converts the wrong way.  Here the file is converted from its own rate to the target.
//   * output length -- the reference caps the output at the source's frame count (buffer.cpp:292-298), which cuts an
//     up-converted impulse short.  Here all ceil(n p / q) frames are written.
// Because of both, a cache directory must not be shared with the reference for ir- files.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bfir_types.hpp"
#include "equalizer_hip.hpp"
#include "wav_io.hpp"

namespace buffer {

// buffer.cpp:152-177
inline bool get_snd_file_params(const char *filename, int *n_channels, int *n_frames, int *sampling_rate)
{
    std::vector<uint8_t> raw;
    int realsize = 0;
    return wav_io::load_float(filename, &raw, n_channels, n_frames, &realsize, sampling_rate);
}

// buffer.cpp:190-211
inline bool check_snd_file(const char *filename, int n_channels, int sampling_rate)
{
    int ch = 0, frames = 0, rate = 0;
    return get_snd_file_params(filename, &ch, &frames, &rate) && ch == n_channels && rate == sampling_rate;
}

// buffer.cpp:37-95: the file's frames in realsize precision, at most max_frames of them (-1: all); `pad`: a buffer of
// max_frames frames, the rest zero.  NULL where the file cannot be read.
inline void *load_from_snd_file(const char *filename, int *n_channels, int *n_frames, int realsize, int max_frames, bool pad)
{
    std::vector<uint8_t> raw;
    int file_frames = 0, file_size = 0, rate = 0;
    if ((realsize != 4 && realsize != 8) || (pad && max_frames < 0)) return nullptr;
    if (!wav_io::load_float(filename, &raw, n_channels, &file_frames, &file_size, &rate)) return nullptr;
    *n_frames = max_frames == -1 ? file_frames : max_frames > file_frames ? file_frames : max_frames;
    if (*n_frames < 0) return nullptr;
    const size_t rows = pad ? (size_t)max_frames : (size_t)*n_frames, n = (size_t)*n_frames * *n_channels;
    const size_t bytes = rows * *n_channels * realsize;
    void *buf = bfir_aligned_malloc(bytes ? bytes : 16, 16);
    if (!buf) return nullptr;
    memset(buf, 0, bytes);
    if (file_size == realsize) memcpy(buf, raw.data(), n * realsize);
    else if (realsize == 4) for (size_t i = 0; i < n; i++) ((float *)buf)[i] = (float)((const double *)raw.data())[i];
    else for (size_t i = 0; i < n; i++) ((double *)buf)[i] = (double)((const float *)raw.data())[i];
    return buf;
}

// buffer.cpp:106-139; like the reference's it reports nothing
inline void save_to_snd_file(const char *filename, void *buf, int n_channels, int n_frames, int realsize, int sampling_rate)
{
    (void)wav_io::save_float(filename, buf, n_channels, n_frames, realsize, sampling_rate);
}

// buffer.cpp:343-384: one buffer per channel, and the table of them
inline void **deinterlace(void *buf, int n_channels, int n_frames, int realsize)
{
    void **bufs = (void **)bfir_aligned_malloc(sizeof(void *) * (size_t)n_channels, 16);
    for (int c = 0; c < n_channels; c++) {
        bufs[c] = bfir_aligned_malloc((size_t)n_frames * realsize + 16, 16);
        for (int f = 0; f < n_frames; f++)
            memcpy((uint8_t *)bufs[c] + (size_t)f * realsize, (const uint8_t *)buf + ((size_t)f * n_channels + c) * realsize, realsize);
    }
    return bufs;
}

// buffer.cpp:397-443: the first n_channels buffers as frames
inline void *interlace(void **bufs, int n_channels, int n_frames, int realsize)
{
    void *buf = bfir_aligned_malloc((size_t)n_channels * n_frames * realsize + 16, 16);
    for (int c = 0; c < n_channels; c++)
        for (int f = 0; f < n_frames; f++)
            memcpy((uint8_t *)buf + ((size_t)f * n_channels + c) * realsize, (const uint8_t *)bufs[c] + (size_t)f * realsize, realsize);
    return buf;
}

// buffer.cpp:243-251: ir-<hex DJB hash of the file name>-<channels>-<rate>.wav
inline std::string cache_name(const char *filename, int n_channels, int sampling_rate)
{
    char name[96];
    snprintf(name, sizeof(name), "ir-%x-%d-%d.wav", equalizer::djb_hash(filename, strlen(filename)), n_channels, sampling_rate);
    return name;
}

// buffer.cpp:225-330: the file's first n_channels channels at sampling_rate, as a float WAV in cache_dir (the reference's
// bfir_path::append_temp_path); its path, or the empty string on failure.  An existing cache file is reused untouched, a
// file with fewer channels than asked is refused, the conversion runs in realsize 4.  The defaults preserve the waveform,
// as libsamplerate does; a caller who wants the filter's frequency response preserved passes gain = file rate /
// sampling_rate.
inline std::string resample_snd_file(const char *filename, int n_channels, int sampling_rate, const std::string &cache_dir,
                                     int zero_crossings = 64, double kaiser_beta = 9.0, double cutoff = 0.95, double gain = 1.0,
                                     int device = 0)
{
    const std::string dst = cache_dir + "/" + cache_name(filename, n_channels, sampling_rate);
    FILE *probe = fopen(dst.c_str(), "rb");
    if (probe) { fclose(probe); return dst; }
    const int realsize = 4;
    int src_channels = 0, src_frames = 0, src_rate = 0;
    if (!get_snd_file_params(filename, &src_channels, &src_frames, &src_rate) || src_channels < n_channels) return std::string();
    void *src = load_from_snd_file(filename, &src_channels, &src_frames, realsize, -1, false);
    if (!src) return std::string();
    if (src_channels > n_channels) {   // deinterlace, re-interlace without the extra channels (:280-289)
        void **tmp = deinterlace(src, src_channels, src_frames, realsize);
        bfir_aligned_free(src);
        src = interlace(tmp, n_channels, src_frames, realsize);
        for (int c = 0; c < src_channels; c++) bfir_aligned_free(tmp[c]);
        bfir_aligned_free(tmp);
    }
    bool ok = false;
    int err = 0;
    bfir_resampler *r = bfir_resampler_create(src_rate, sampling_rate, zero_crossings, kaiser_beta, cutoff, gain, realsize,
                                              n_channels, device, &err);
    if (r) {
        const int64_t n_out = bfir_resampler_out_frames(r, src_frames);
        if (n_out >= 0 && n_out <= INT32_MAX) {
            std::vector<float> out((size_t)n_out * n_channels + 1);
            ok = bfir_resampler_run(r, src, src_frames, out.data(), n_out) == n_out &&
                 wav_io::save_float(dst, out.data(), n_channels, (int)n_out, realsize, sampling_rate);
        }
        bfir_resampler_destroy(r);
    }
    bfir_aligned_free(src);
    return ok ? dst : std::string();
}

}  // namespace buffer
