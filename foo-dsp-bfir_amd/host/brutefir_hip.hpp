// brutefir_hip.hpp -- the reference's engine class (brutefir/brutefir.hpp:15-128)
// over the fused GPU engine: same public interface, same return codes, so
// foo_dsp_bfir.cpp:279-345 and preprocessor.cpp:287-333 call it unchanged.
// All block processing happens in bfir_engine_run (include/bfir_hip.h).
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cwchar>
#include <string>

#include "bfir_types.hpp"
#include "coeff_hip.hpp"

class brutefir {
public:
    // brutefir.cpp:21-44.  On failure the object stays uninitialised (is_initialized()
    // false, run() returns an error), as the reference's does.
    brutefir(int filter_length, int filter_blocks, int realsize, int channels, int in_format,
             int out_format, int sampling_rate, bool apply_dither, int device = 0)
        : m_channels(channels), m_filter_length(filter_length), m_realsize(realsize), m_rate(sampling_rate)
    {
        int err = 0;
        m_e = bfir_engine_create(filter_length, filter_blocks, realsize, channels, in_format, out_format,
                                 sampling_rate, apply_dither ? 1 : 0, device, &err);
        m_err = err;
        memset(m_last, 0, sizeof(m_last));
    }
    // Long partitions (bfir_engine_create_big): filter_blocks partitions of 32768 ... 1048576 samples (realsize 8: from
    // 16384), the lengths past bfir_engine_create's.  Everything else is the first constructor's: every sample format, dither,
    // both set_coeff overloads.
    struct long_partitions { int filter_blocks; };
    brutefir(int filter_length, long_partitions big, int realsize, int channels, int in_format, int out_format,
             int sampling_rate, bool apply_dither, int device = 0)
        : m_channels(channels), m_filter_length(filter_length), m_realsize(realsize), m_rate(sampling_rate)
    {
        int err = 0;
        m_e = bfir_engine_create_big(filter_length, big.filter_blocks, realsize, channels, in_format, out_format,
                                     sampling_rate, apply_dither ? 1 : 0, device, &err);
        m_err = err;
        memset(m_last, 0, sizeof(m_last));
    }
    // Two partition lengths (bfir_engine_create_nup): taps [0, head_blocks * filter_length) on partitions of filter_length,
    // the rest on tail_blocks partitions of tail_ratio * filter_length; run() keeps its filter_length-frame blocks.
    // Float frames only, no dither.  Coefficients: the set_coeff(coeffs, n_coeffs, length, scale) overload.
    struct two_level { int head_blocks, tail_ratio, tail_blocks; };
    brutefir(int filter_length, two_level levels, int realsize, int channels, int in_format, int out_format, int device = 0)
        : m_channels(channels)
    {
        int err = 0;
        m_e = bfir_engine_create_nup(filter_length, levels.head_blocks, levels.tail_ratio, levels.tail_blocks, realsize,
                                     channels, in_format, out_format, device, &err);
        m_err = err;
        memset(m_last, 0, sizeof(m_last));
    }
    // Three or four partition lengths (bfir_engine_create_levels): level k has blocks[k] partitions of ratios[k] times the
    // length of level k - 1 (ratios[0] = 1).  Coefficients: set_coeff_levels(coeffs, n_coeffs, length, scale).
    struct multi_level { int n_levels; int blocks[BFIR_MAX_LEVELS]; int ratios[BFIR_MAX_LEVELS]; };
    brutefir(int filter_length, const multi_level &levels, int realsize, int channels, int in_format, int out_format, int device = 0)
        : m_channels(channels)
    {
        int err = 0;
        m_e = bfir_engine_create_levels(filter_length, levels.n_levels, levels.blocks, levels.ratios, realsize, channels, in_format,
                                        out_format, device, &err);
        m_err = err;
        memset(m_last, 0, sizeof(m_last));
    }
    // The matrix form of the above (bfir_engine_create_matrix_levels): n_inputs -> n_outputs, one filter per (output, input)
    // pair, every filter on the same two to four partition lengths.  Frames are n_inputs samples in and n_outputs samples
    // out.  Coefficients: set_coeff_matrix_levels(coeffs, lengths, scale).
    struct matrix_io { int n_inputs, n_outputs; };
    brutefir(int filter_length, const multi_level &levels, int realsize, matrix_io io, int in_format, int out_format, int device = 0)
        : m_channels(io.n_outputs)
    {
        int err = 0;
        m_e = bfir_engine_create_matrix_levels(filter_length, levels.n_levels, levels.blocks, levels.ratios, realsize, io.n_inputs,
                                               io.n_outputs, in_format, out_format, device, &err);
        m_err = err;
        memset(m_last, 0, sizeof(m_last));
    }
    // A mimo engine (bfir_engine_create_mimo): n_inputs -> n_outputs with up to BFIR_MIMO_MAXCHANNELS of each, one filter
    // per (output, input) pair on uniform partitions.  Float frames only, no dither, no delays.  Coefficients:
    // set_coeff_matrix(coeffs, length, coeff_blocks, scale).
    struct mimo_io { int n_inputs, n_outputs; };
    brutefir(int filter_length, int filter_blocks, int realsize, mimo_io io, int in_format, int out_format, int device = 0)
        : m_channels(io.n_outputs)
    {
        int err = 0;
        m_e = bfir_engine_create_mimo(filter_length, filter_blocks, realsize, io.n_inputs, io.n_outputs, in_format, out_format,
                                      device, &err);
        m_err = err;
        memset(m_last, 0, sizeof(m_last));
    }
    // A multi-level mimo engine (bfir_engine_create_mimo_levels): the matrix form on two to four partition lengths with up
    // to BFIR_MIMO_MAXCHANNELS inputs and outputs.  Float frames only, no dither, no delays.  Coefficients:
    // set_coeff_matrix_levels(coeffs, lengths, scale).
    brutefir(int filter_length, const multi_level &levels, int realsize, mimo_io io, int in_format, int out_format, int device = 0)
        : m_channels(io.n_outputs)
    {
        int err = 0;
        m_e = bfir_engine_create_mimo_levels(filter_length, levels.n_levels, levels.blocks, levels.ratios, realsize, io.n_inputs,
                                             io.n_outputs, in_format, out_format, device, &err);
        m_err = err;
        memset(m_last, 0, sizeof(m_last));
    }
    ~brutefir() { bfir_engine_destroy(m_e); }
    brutefir(const brutefir &) = delete;
    brutefir &operator=(const brutefir &) = delete;

    bool is_initialized() { return m_e && bfir_engine_is_initialized(m_e); }

    // brutefir.cpp:88-165: one filter per channel from a sound file with the engine's channel count and sampling rate, at
    // most coeff_blocks * filter_length frames of it and at most n_channels filters.  The number of filters; -1 for an
    // incompatible (or unreadable) file, or an engine built by another constructor than the first; -2 when loading failed.
    // A file at another rate goes through buffer::resample_snd_file first (foo_dsp_bfir.cpp:181-233).
    int set_coeff(const char *filename, int coeff_blocks, double scale)
    {
        if (!m_e || !filename) return -1;
        if (!buffer::check_snd_file(filename, m_channels, m_rate)) return -1;
        int length = 0, n_coeffs = 0;
        void **coeffs = coeff::load_snd_coeff(filename, &length, m_realsize, coeff_blocks * m_filter_length, &n_coeffs);
        if (!coeffs) return -2;
        const int n_files = n_coeffs;
        if (n_coeffs > m_channels) n_coeffs = m_channels;
        const int rc = bfir_engine_set_coeff(m_e, (const void *const *)coeffs, n_coeffs, length, coeff_blocks, scale);
        for (int n = 0; n < n_files; n++) bfir_aligned_free(coeffs[n]);
        bfir_aligned_free(coeffs);
        return rc == 0 ? n_coeffs : -2;
    }
    // the reference's wide-character signature: the name narrowed as util::wstr2str does (buffer.cpp:244)
    int set_coeff(const wchar_t *filename, int coeff_blocks, double scale)
    {
        if (!filename) return -1;
        std::string narrow(wcslen(filename) * MB_CUR_MAX + 1, '\0');
        const size_t n = wcstombs(&narrow[0], filename, narrow.size());
        if (n == (size_t)-1) return -1;
        narrow.resize(n);
        return set_coeff(narrow.c_str(), coeff_blocks, scale);
    }

    // brutefir.cpp:179-228: 0, or -2 when a tap is NaN/Inf.
    int set_coeff(void **coeffs, int n_coeffs, int length, int coeff_blocks, double scale)
    {
        if (!m_e) return -1;
        return bfir_engine_set_coeff(m_e, (const void *const *)coeffs, n_coeffs, length, coeff_blocks, scale);
    }

    // The same with a crossfade over the next fade_blocks blocks instead of a hard cut: the blend of
    // fftw_convolver::convolver_crossfade_inplace (fftw_convolver.cpp:275-321) at the engine level.  0, -2 (a NaN/Inf tap:
    // the old filters stay), or a BFIR_ERR_* code (bfir_engine_set_coeff_fade).
    int set_coeff_fade(void **coeffs, int n_coeffs, int length, int coeff_blocks, double scale, int fade_blocks)
    {
        if (!m_e) return -1;
        return bfir_engine_set_coeff_fade(m_e, (const void *const *)coeffs, n_coeffs, length, coeff_blocks, scale, fade_blocks);
    }
    // blocks of a pending or running fade still to be processed; 0 = none
    int fade_remaining() { return m_e ? bfir_engine_fade_remaining(m_e) : -1; }

    // A two-level engine's filters: `length` taps per channel, split between the levels (bfir_engine_set_coeff_nup).
    int set_coeff(void **coeffs, int n_coeffs, int length, double scale)
    {
        if (!m_e) return -1;
        return bfir_engine_set_coeff_nup(m_e, (const void *const *)coeffs, n_coeffs, length, scale);
    }

    // A multi-level engine's filters: `length` taps per channel, split between the levels (bfir_engine_set_coeff_levels).
    int set_coeff_levels(void **coeffs, int n_coeffs, int length, double scale)
    {
        if (!m_e) return -1;
        return bfir_engine_set_coeff_levels(m_e, (const void *const *)coeffs, n_coeffs, length, scale);
    }

    // A mimo engine's filters: coeffs[o * n_inputs + i] the `length` taps of h_{o,i} or null (no path), at most coeff_blocks
    // partitions of each (bfir_engine_set_coeff_matrix); and partition spectrum `block` of h_{output,input}.
    int set_coeff_matrix(void **coeffs, int length, int coeff_blocks, double scale)
    {
        if (!m_e) return -1;
        return bfir_engine_set_coeff_matrix(m_e, (const void *const *)coeffs, length, coeff_blocks, scale);
    }
    int read_coeff_matrix(int output, int input, int block, void *dst)
    {
        if (!m_e) return -1;
        return bfir_engine_read_coeff_matrix(m_e, output, input, block, dst);
    }
    // A list of a mimo engine's pairs replaced: coeffs[k] the new h_{outputs[k],inputs[k]} or null (the path is removed), every
    // other pair keeps its filter (bfir_engine_set_coeff_matrix_pairs); and the same change crossfaded over the next
    // fade_blocks blocks (bfir_engine_set_coeff_matrix_pairs_fade).
    int set_coeff_matrix_pairs(int n_pairs, const int *outputs, const int *inputs, void **coeffs, int length, int coeff_blocks,
                               double scale)
    {
        if (!m_e) return -1;
        return bfir_engine_set_coeff_matrix_pairs(m_e, n_pairs, outputs, inputs, (const void *const *)coeffs, length, coeff_blocks,
                                                  scale);
    }
    int set_coeff_matrix_pairs_fade(int n_pairs, const int *outputs, const int *inputs, void **coeffs, int length, int coeff_blocks,
                                    double scale, int fade_blocks)
    {
        if (!m_e) return -1;
        return bfir_engine_set_coeff_matrix_pairs_fade(m_e, n_pairs, outputs, inputs, (const void *const *)coeffs, length,
                                                       coeff_blocks, scale, fade_blocks);
    }

    // A mimo engine's coefficient bank: filters transformed once and kept on the device (bfir_engine_bank_create, _destroy,
    // _entries, _blocks, _load, _read), then named by index.  coeffs[k] of bank_load: the `length` taps of entry first + k, or
    // null (the entry becomes empty); an entry keeps the partition count min(coeff_blocks, filter_blocks) it was loaded with.
    int bank_create(int n_entries) { return m_e ? bfir_engine_bank_create(m_e, n_entries) : -1; }
    int bank_destroy() { return m_e ? bfir_engine_bank_destroy(m_e) : -1; }
    int bank_entries() { return m_e ? bfir_engine_bank_entries(m_e) : -1; }
    int bank_blocks(int entry) { return m_e ? bfir_engine_bank_blocks(m_e, entry) : -1; }
    int bank_load(int first, int n, void **coeffs, int length, int coeff_blocks, double scale)
    {
        if (!m_e) return -1;
        return bfir_engine_bank_load(m_e, first, n, (const void *const *)coeffs, length, coeff_blocks, scale);
    }
    int bank_read(int entry, int block, void *dst) { return m_e ? bfir_engine_bank_read(m_e, entry, block, dst) : -1; }
    // The four coefficient changes of a mimo engine with bank entries in place of taps: entries[o * n_inputs + i] (the whole
    // matrix) or entries[k] for the pair (outputs[k], inputs[k]) is a bank index, or -1 = no path
    // (bfir_engine_set_coeff_matrix_bank, _bank_fade, _pairs_bank, _pairs_bank_fade).
    int set_coeff_matrix_bank(const int *entries) { return m_e ? bfir_engine_set_coeff_matrix_bank(m_e, entries) : -1; }
    int set_coeff_matrix_bank_fade(const int *entries, int fade_blocks)
    {
        return m_e ? bfir_engine_set_coeff_matrix_bank_fade(m_e, entries, fade_blocks) : -1;
    }
    int set_coeff_matrix_pairs_bank(int n_pairs, const int *outputs, const int *inputs, const int *entries)
    {
        return m_e ? bfir_engine_set_coeff_matrix_pairs_bank(m_e, n_pairs, outputs, inputs, entries) : -1;
    }
    int set_coeff_matrix_pairs_bank_fade(int n_pairs, const int *outputs, const int *inputs, const int *entries, int fade_blocks)
    {
        return m_e ? bfir_engine_set_coeff_matrix_pairs_bank_fade(m_e, n_pairs, outputs, inputs, entries, fade_blocks) : -1;
    }
    // The same four with a weighted sum of up to BFIR_BANK_MIX_TERMS entries in place of one: listed row k has the terms
    // (entries[k * n_terms + j], weights[k * n_terms + j]), j < n_terms; entry -1 or weight 0: the term takes no part
    // (bfir_engine_set_coeff_matrix_bank_mix, _bank_mix_fade, _pairs_bank_mix, _pairs_bank_mix_fade).
    int set_coeff_matrix_bank_mix(int n_terms, const int *entries, const double *weights)
    {
        return m_e ? bfir_engine_set_coeff_matrix_bank_mix(m_e, n_terms, entries, weights) : -1;
    }
    int set_coeff_matrix_bank_mix_fade(int n_terms, const int *entries, const double *weights, int fade_blocks)
    {
        return m_e ? bfir_engine_set_coeff_matrix_bank_mix_fade(m_e, n_terms, entries, weights, fade_blocks) : -1;
    }
    int set_coeff_matrix_pairs_bank_mix(int n_pairs, const int *outputs, const int *inputs, int n_terms, const int *entries,
                                        const double *weights)
    {
        return m_e ? bfir_engine_set_coeff_matrix_pairs_bank_mix(m_e, n_pairs, outputs, inputs, n_terms, entries, weights) : -1;
    }
    int set_coeff_matrix_pairs_bank_mix_fade(int n_pairs, const int *outputs, const int *inputs, int n_terms, const int *entries,
                                             const double *weights, int fade_blocks)
    {
        return m_e ? bfir_engine_set_coeff_matrix_pairs_bank_mix_fade(m_e, n_pairs, outputs, inputs, n_terms, entries, weights,
                                                                      fade_blocks)
                   : -1;
    }

    // A multi-level matrix engine's filters: coeffs[o * n_inputs + i] the taps of h_{o,i} or null (no path), lengths[o *
    // n_inputs + i] its tap count, each filter split between the levels (bfir_engine_set_coeff_matrix_levels).
    int set_coeff_matrix_levels(void **coeffs, const int *lengths, double scale)
    {
        if (!m_e) return -1;
        return bfir_engine_set_coeff_matrix_levels(m_e, (const void *const *)coeffs, lengths, scale);
    }
    // partition spectrum `block` of h_{output,input} on `level` (2 L_level reals, grouped layout)
    int read_coeff_matrix_levels(int level, int output, int input, int block, void *dst)
    {
        if (!m_e) return -1;
        return bfir_engine_read_coeff_matrix_levels(m_e, level, output, input, block, dst);
    }

    // The same two with a crossfade over the next fade_blocks blocks of filter_length frames, every level consistently
    // (bfir_engine_set_coeff_nup_fade / _levels_fade): 0, -2 (a NaN/Inf tap: the old filters stay), or a BFIR_ERR_* code.
    int set_coeff_nup_fade(void **coeffs, int n_coeffs, int length, double scale, int fade_blocks)
    {
        if (!m_e) return -1;
        return bfir_engine_set_coeff_nup_fade(m_e, (const void *const *)coeffs, n_coeffs, length, scale, fade_blocks);
    }
    int set_coeff_levels_fade(void **coeffs, int n_coeffs, int length, double scale, int fade_blocks)
    {
        if (!m_e) return -1;
        return bfir_engine_set_coeff_levels_fade(m_e, (const void *const *)coeffs, n_coeffs, length, scale, fade_blocks);
    }
    // ... and a multi-level matrix engine's, coeffs / lengths as set_coeff_matrix_levels takes them
    // (bfir_engine_set_coeff_matrix_levels_fade): a filter that is null or shorter in one set fades in or out.
    int set_coeff_matrix_levels_fade(void **coeffs, const int *lengths, double scale, int fade_blocks)
    {
        if (!m_e) return -1;
        return bfir_engine_set_coeff_matrix_levels_fade(m_e, (const void *const *)coeffs, lengths, scale, fade_blocks);
    }
    // A list of a multi-level matrix or mimo engine's pairs replaced: coeffs[k] the new h_{outputs[k],inputs[k]} with
    // lengths[k] taps, or null (the path is removed); every other pair keeps its filter on every level
    // (bfir_engine_set_coeff_matrix_levels_pairs); and the same change crossfaded over the next fade_blocks blocks
    // (bfir_engine_set_coeff_matrix_levels_pairs_fade).
    int set_coeff_matrix_levels_pairs(int n_pairs, const int *outputs, const int *inputs, void **coeffs, const int *lengths,
                                      double scale)
    {
        if (!m_e) return -1;
        return bfir_engine_set_coeff_matrix_levels_pairs(m_e, n_pairs, outputs, inputs, (const void *const *)coeffs, lengths, scale);
    }
    int set_coeff_matrix_levels_pairs_fade(int n_pairs, const int *outputs, const int *inputs, void **coeffs, const int *lengths,
                                           double scale, int fade_blocks)
    {
        if (!m_e) return -1;
        return bfir_engine_set_coeff_matrix_levels_pairs_fade(m_e, n_pairs, outputs, inputs, (const void *const *)coeffs, lengths,
                                                              scale, fade_blocks);
    }
    // A multi-level matrix or mimo engine's coefficient bank, one store per level: filters split between the levels and
    // transformed once (bfir_engine_levels_bank_create, _destroy, _entries, _length, _blocks, _load, _read), then named by
    // index.  coeffs[k] of levels_bank_load: the lengths[k] taps of entry first + k, or null (the entry becomes empty).
    int levels_bank_create(int n_entries) { return m_e ? bfir_engine_levels_bank_create(m_e, n_entries) : -1; }
    int levels_bank_destroy() { return m_e ? bfir_engine_levels_bank_destroy(m_e) : -1; }
    int levels_bank_entries() { return m_e ? bfir_engine_levels_bank_entries(m_e) : -1; }
    int levels_bank_length(int entry) { return m_e ? bfir_engine_levels_bank_length(m_e, entry) : -1; }
    int levels_bank_blocks(int entry, int level) { return m_e ? bfir_engine_levels_bank_blocks(m_e, entry, level) : -1; }
    int levels_bank_load(int first, int n, void **coeffs, const int *lengths, double scale)
    {
        if (!m_e) return -1;
        return bfir_engine_levels_bank_load(m_e, first, n, (const void *const *)coeffs, lengths, scale);
    }
    int levels_bank_read(int entry, int level, int block, void *dst)
    {
        return m_e ? bfir_engine_levels_bank_read(m_e, entry, level, block, dst) : -1;
    }
    // The four coefficient changes of such an engine with bank entries in place of taps: entries[o * n_inputs + i] (the whole
    // matrix) or entries[k] for the pair (outputs[k], inputs[k]) is a bank index, or -1 = no path
    // (bfir_engine_set_coeff_matrix_levels_bank, _bank_fade, _pairs_bank, _pairs_bank_fade).
    int set_coeff_matrix_levels_bank(const int *entries) { return m_e ? bfir_engine_set_coeff_matrix_levels_bank(m_e, entries) : -1; }
    int set_coeff_matrix_levels_bank_fade(const int *entries, int fade_blocks)
    {
        return m_e ? bfir_engine_set_coeff_matrix_levels_bank_fade(m_e, entries, fade_blocks) : -1;
    }
    int set_coeff_matrix_levels_pairs_bank(int n_pairs, const int *outputs, const int *inputs, const int *entries)
    {
        return m_e ? bfir_engine_set_coeff_matrix_levels_pairs_bank(m_e, n_pairs, outputs, inputs, entries) : -1;
    }
    int set_coeff_matrix_levels_pairs_bank_fade(int n_pairs, const int *outputs, const int *inputs, const int *entries,
                                                int fade_blocks)
    {
        return m_e ? bfir_engine_set_coeff_matrix_levels_pairs_bank_fade(m_e, n_pairs, outputs, inputs, entries, fade_blocks) : -1;
    }
    // The same four with up to BFIR_BANK_MIX_TERMS (entry, weight) terms per row in place of one entry: entries[k * n_terms + j]
    // and weights[k * n_terms + j] belong to row k, and every level's row is the weighted sum of the entries' rows there, formed
    // on the device (bfir_engine_set_coeff_matrix_levels_bank_mix, _bank_mix_fade, _pairs_bank_mix, _pairs_bank_mix_fade).
    int set_coeff_matrix_levels_bank_mix(int n_terms, const int *entries, const double *weights)
    {
        return m_e ? bfir_engine_set_coeff_matrix_levels_bank_mix(m_e, n_terms, entries, weights) : -1;
    }
    int set_coeff_matrix_levels_bank_mix_fade(int n_terms, const int *entries, const double *weights, int fade_blocks)
    {
        return m_e ? bfir_engine_set_coeff_matrix_levels_bank_mix_fade(m_e, n_terms, entries, weights, fade_blocks) : -1;
    }
    int set_coeff_matrix_levels_pairs_bank_mix(int n_pairs, const int *outputs, const int *inputs, int n_terms, const int *entries,
                                               const double *weights)
    {
        return m_e ? bfir_engine_set_coeff_matrix_levels_pairs_bank_mix(m_e, n_pairs, outputs, inputs, n_terms, entries, weights) : -1;
    }
    int set_coeff_matrix_levels_pairs_bank_mix_fade(int n_pairs, const int *outputs, const int *inputs, int n_terms,
                                                    const int *entries, const double *weights, int fade_blocks)
    {
        return m_e ? bfir_engine_set_coeff_matrix_levels_pairs_bank_mix_fade(m_e, n_pairs, outputs, inputs, n_terms, entries, weights,
                                                                             fade_blocks)
                   : -1;
    }
    // head blocks of such a fade still to be processed; 0 = none
    int fade_remaining_levels() { return m_e ? bfir_engine_fade_remaining_levels(m_e) : -1; }

    // Per-channel delays on the input (side BFIR_DELAY_INPUT) or output (BFIR_DELAY_OUTPUT) frames: what the reference's delay
    // class does on its host buffers (brutefir/delay.hpp: delay_allocate_buffer + subsample_init, update, subsample_update).
    // delay_init once per side (step_count 0: whole samples only), then set_delay with one entry per channel of the side --
    // the inputs / outputs of a matrix engine -- from the next block on, as a hard cut.  0 or a BFIR_ERR_* code.
    int delay_init(int side, int max_delay, int step_count = 0, int half_filter_length = 0, double kaiser_beta = 9.0)
    {
        if (!m_e) return -1;
        return bfir_engine_delay_init(m_e, side, max_delay, step_count, half_filter_length, kaiser_beta);
    }
    int set_delay(int side, const int *delay, const int *subdelay, int n_channels)
    {
        if (!m_e) return -1;
        return bfir_engine_set_delay(m_e, side, delay, subdelay, n_channels);
    }
    int get_delay(int side, int *delay, int *subdelay, int n_channels)
    {
        if (!m_e) return -1;
        return bfir_engine_get_delay(m_e, side, delay, subdelay, n_channels);
    }
    // frames of fixed latency the side's sub-sample stage adds (half_filter_length, or 0 without one)
    int delay_latency(int side) { return m_e ? bfir_engine_delay_latency(m_e, side) : -1; }
    // the taps of one sub-sample filter (delay::sample_sinc): host arithmetic, no engine needed
    static int subdelay_filter(int half_filter_length, int subdelay, int step_count, double kaiser_beta, int realsize, void *taps)
    {
        return bfir_subdelay_filter(half_filter_length, subdelay, step_count, kaiser_beta, realsize, taps);
    }

    // brutefir.cpp:244-343: one block of filter_length interleaved frames; 0 or -1.
    int run(void *inbuf, void *outbuf) { return run_blocks(inbuf, outbuf, 1); }

    // n consecutive blocks in one call: what the offline drivers' loops
    // (preprocessor.cpp:145, 329-333) amount to.
    int run_blocks(void *inbuf, void *outbuf, int n_blocks)
    {
        if (!m_e) return -1;
        int rc = bfir_engine_run(m_e, inbuf, outbuf, n_blocks);
        return rc == 0 ? 0 : -1;
    }

    // brutefir.cpp:346-367
    void reset()
    {
        if (m_e) bfir_engine_reset(m_e);
        memset(m_last, 0, sizeof(m_last));
    }

    // brutefir.cpp:370-388 + print_overflows :585-629: report when any channel changed.
    void check_overflows()
    {
        if (!m_e) return;
        bfir_overflow of[BFIR_MIMO_MAXCHANNELS];
        bool changed = false, any = false;
        for (int n = 0; n < m_channels; n++) {
            bfir_engine_get_overflow(m_e, n, &of[n]);
            changed |= memcmp(&of[n], &m_last[n], sizeof(bfir_overflow)) != 0;
            any |= of[n].n_overflows > 0;
        }
        if (!changed) return;
        memcpy(m_last, of, sizeof(bfir_overflow) * m_channels);
        if (!any) return;
        for (int n = 0; n < m_channels; n++) {
            double peak = of[n].largest;
            if (peak < (double)of[n].intlargest) peak = (double)of[n].intlargest;
            char line[96];
            if (peak != 0.0) {
                double db = 20.0 * log10(peak / of[n].max);
                if (db == 0.0) db = -0.0;
                snprintf(line, sizeof(line), "peak: %d/%u/%+.2f ", n, of[n].n_overflows, db);
            } else {
                snprintf(line, sizeof(line), "peak: %d/%u/-Inf ", n, of[n].n_overflows);
            }
            if (m_log) m_log(line);
        }
    }

    // pinfo-style sink for check_overflows (brutefir/pinfo.c:17-39)
    void set_log(bfir_log_fn fn) { m_log = fn; bfir_set_log_callback(fn); }
    int create_error() const { return m_err; }
    bfir_engine *handle() { return m_e; }

private:
    bfir_engine *m_e = nullptr;
    int m_channels = 0, m_err = 0;
    int m_filter_length = 0, m_realsize = 0, m_rate = -1;   // of the first constructor: what the file form of set_coeff needs
    bfir_overflow m_last[BFIR_MIMO_MAXCHANNELS];   // the widest kind: the outputs of a mimo engine
    bfir_log_fn m_log = nullptr;
};
