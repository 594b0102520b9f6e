/*
 * bfir_hip.h -- C ABI of the MI355X (gfx950) partitioned-FIR convolution engine.
 *
 * This is the drop-in boundary for the hot path of vsu/foo-dsp-bfir: the
 * entry points are what a binding of the reference's convolver path would
 * bind.  Plain pointers and sizes only; no C++ or torch types.  Citations are
 * path:line in the reference tree (brutefir/...).
 *
 * Two levels:
 *   bfir_engine_*     one call = brutefir::run for n consecutive blocks
 *                     (brutefir/brutefir.cpp:244-343), fused on the GPU with
 *                     the partition spectra and the delay line resident in
 *                     HBM.  This is the measured path.
 *   bfir_convolver_*  one call = one fftw_convolver method
 *                     (brutefir/fftw_convolver.hpp:28-166) on host buffers,
 *                     run by the same kernels.  Plumbing/parity path for
 *                     callers that keep the reference's per-stage sequence.
 *
 * Library: libbfir_hip.so (hipcc --offload-arch=gfx950).  There is no CPU
 * fallback: without a HIP device every create call fails with
 * BFIR_ERR_NO_DEVICE.
 */
#ifndef BFIR_HIP_H
#define BFIR_HIP_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* limits and sample format codes: brutefir/global.h:21-34 */
#define BFIR_MAXCHANNELS 8
#define BFIR_MIMO_MAXCHANNELS 64 /* inputs / outputs of bfir_engine_create_mimo: the GPU's width, not the plug-in's */
#define BFIR_SAMPLE_FORMAT_S8 1
#define BFIR_SAMPLE_FORMAT_S16_LE 2
#define BFIR_SAMPLE_FORMAT_S16_BE 3
#define BFIR_SAMPLE_FORMAT_S24_LE 4
#define BFIR_SAMPLE_FORMAT_S24_BE 5
#define BFIR_SAMPLE_FORMAT_S32_LE 6
#define BFIR_SAMPLE_FORMAT_S32_BE 7
#define BFIR_SAMPLE_FORMAT_FLOAT_LE 8
#define BFIR_SAMPLE_FORMAT_FLOAT_BE 9
#define BFIR_SAMPLE_FORMAT_FLOAT64_LE 10
#define BFIR_SAMPLE_FORMAT_FLOAT64_BE 11

/* mixmodes: brutefir/fftw_convolver.hpp:14-16 */
#define BFIR_MIXMODE_INPUT 1
#define BFIR_MIXMODE_INPUT_ADD 2
#define BFIR_MIXMODE_OUTPUT 3

/* error codes (negative).  -1 and -2 keep the reference's meaning where a
 * reference function returns them (run: -1, set_coeff: -2). */
#define BFIR_OK 0
#define BFIR_ERR_NONFINITE (-1)   /* brutefir::run, brutefir.cpp:316-321 */
#define BFIR_ERR_COEFF (-2)       /* brutefir::set_coeff, brutefir.cpp:217-222 */
#define BFIR_ERR_ARG (-3)
#define BFIR_ERR_NO_DEVICE (-4)
#define BFIR_ERR_HIP (-5)
#define BFIR_ERR_STATE (-6)       /* engine not initialised (no coefficients) */
#define BFIR_ERR_UNSUPPORTED (-7) /* sample format / size outside this build */
#define BFIR_ERR_IO (-8)          /* a file could not be opened (convolver_debug_dump_cbuf) */

/* bfoverflow_t, brutefir/global.h:96-102 (same layout) */
typedef struct bfir_overflow {
    unsigned int n_overflows;
    int32_t intlargest;
    double largest;
    double max;
} bfir_overflow;

/* sample_format_t + buffer_format_t, brutefir/global.h:39-54 (same layout) */
typedef struct bfir_sample_format {
    bool isfloat;
    bool swap;
    int bytes;
    int sbytes;
    double scale;
    int format;
} bfir_sample_format;

typedef struct bfir_buffer_format {
    bfir_sample_format sf;
    int sample_spacing; /* in samples */
    int byte_offset;    /* in bytes */
} bfir_buffer_format;

/* log callback, same shape as pinfo's (brutefir/pinfo.c:17-39) */
typedef void (*bfir_log_fn)(const char *msg);
void bfir_set_log_callback(bfir_log_fn fn);

const char *bfir_strerror(int err);
int bfir_device_count(void);
const char *bfir_version(void);

/* ------------------------------------------------------------------ */
/* engine level                                                        */
/* ------------------------------------------------------------------ */
typedef struct bfir_engine bfir_engine;

/* brutefir::brutefir (brutefir/brutefir.hpp:18-25, brutefir.cpp:21-44).
 * filter_length: partition length L (power of two, 16..16384; 8192 max for
 * realsize 8); filter_blocks: B; realsize: 4 or 8; channels: 1..8;
 * in/out_format: any BFIR_SAMPLE_FORMAT_* code (FLOAT_LE / FLOAT64_LE take the
 * vectorised staging kernels, the others a byte-wise one); apply_dither acts on
 * integer output formats only (fftw_convolver.cpp:421, 444): HP-TPDF dither with
 * the reference's random table (dither.cpp:21-110; sampling_rate sizes it) and
 * error feedback, one lane per channel.  device: HIP ordinal.
 * Returns NULL and sets *err on failure. */
bfir_engine *bfir_engine_create(int filter_length, int filter_blocks, int realsize, int channels,
                                int in_format, int out_format, int sampling_rate, int apply_dither,
                                int device, int *err);

/* n_engines independent, identically shaped engines run by shared launches
 * (BASELINE.json configs[3]).  Engine e owns global channels e*C .. e*C+C-1. */
bfir_engine *bfir_engine_create_batch(int n_engines, int filter_length, int filter_blocks,
                                      int realsize, int channels, int in_format, int out_format,
                                      int sampling_rate, int apply_dither, int device, int *err);

/* Long partitions ("big" engines): a diagonal engine whose partition does not fit one workgroup's transform -- the
 * playback configurations written as a few partitions of 65536 or more.  filter_length is a power of two, 32768 ...
 * 1048576 with realsize 4 and 16384 ... 1048576 with realsize 8; a power of two outside that range is
 * BFIR_ERR_UNSUPPORTED (16 ... 16384 / 8192 are bfir_engine_create's), anything else BFIR_ERR_ARG as there.  One engine
 * (no batch), 1 <= channels <= BFIR_MAXCHANNELS, all eleven sample formats, HP-TPDF dither with integer outputs.
 * Every transform runs as two passes over the workgroup FFT (bigconv.hip) and the spectra are kept in a transposed bin
 * order, which only bfir_engine_read_coeff undoes: it hands out the reference's grouped layout in natural bin order, like
 * every other kind.  bfir_engine_set_coeff, _set_coeff_at, _read_coeff, run, run_device, sync, reset, get_overflow,
 * set_chunk, set_profiling, get_profile, is_initialized, destroy, set_coeff_fade, fade_remaining and the delay calls work
 * on it as on an engine from bfir_engine_create; the matrix, nup and levels calls return BFIR_ERR_UNSUPPORTED.  A launch
 * (bfir_engine_set_chunk) whose delay line would pass 2^31 samples per channel is refused with BFIR_ERR_UNSUPPORTED
 * before anything is queued; the default never gets there. */
bfir_engine *bfir_engine_create_big(int filter_length, int filter_blocks, int realsize, int channels,
                                    int in_format, int out_format, int sampling_rate, int apply_dither,
                                    int device, int *err);

/* n_inputs -> n_outputs, one filter per (output, input) pair: output o is the sum over the inputs i of input i
 * convolved with h_{o,i} (a BruteFIR filter graph folded into one matrix).  1 <= n_inputs, n_outputs <=
 * BFIR_MAXCHANNELS.  Frames: n_inputs-channel frames in, n_outputs-channel frames out, FLOAT_LE or FLOAT64_LE each
 * (other formats: BFIR_ERR_UNSUPPORTED).  No dither (float outputs only), one engine (no batch).  Every other
 * bfir_engine_* entry point works on it; get_overflow's `channel` is an output.  bfir_engine_set_coeff, _set_coeff_at
 * and _read_coeff return BFIR_ERR_UNSUPPORTED on a matrix engine, the two matrix calls below the same on others. */
bfir_engine *bfir_engine_create_matrix(int filter_length, int filter_blocks, int realsize, int n_inputs,
                                       int n_outputs, int in_format, int out_format, int device, int *err);

/* A matrix engine as bfir_engine_create_matrix defines it, of up to BFIR_MIMO_MAXCHANNELS inputs and outputs ("mimo"):
 * uniform partitions of the lengths bfir_engine_create takes for realsize, FLOAT_LE / FLOAT64_LE frames, no dither, one
 * engine.  coeffs[o * n_inputs + i], NULL = no path.  Checked before the device is touched: a count outside 1 ...
 * BFIR_MIMO_MAXCHANNELS is BFIR_ERR_ARG; an integer or big-endian frame format and a partition length outside the range
 * are BFIR_ERR_UNSUPPORTED; valid arguments without a GPU give BFIR_ERR_NO_DEVICE.
 * With unchanged meaning on it: bfir_engine_set_coeff_matrix, _read_coeff_matrix, _set_coeff_matrix_fade, _fade_remaining,
 * _run, _run_device, _sync, _reset, _get_overflow (channel = output, 0 ... n_outputs - 1), _set_chunk, _set_profiling,
 * _get_profile, _is_initialized, _destroy.  BFIR_ERR_UNSUPPORTED on it: the diagonal, nup, levels and matrix-levels
 * coefficient and fade calls, and the four delay calls (the delay table holds BFIR_MAXCHANNELS channels).  A launch
 * (bfir_engine_set_chunk) past the MAC kernel's grid is refused with BFIR_ERR_UNSUPPORTED before anything is allocated or
 * queued; the default never gets there.
 * Every output sample is one fma chain per (output, bin, block) -- inputs in index order, partitions in order, a filter
 * with fewer partitions or none skipped, never multiplied by zero -- so two byte identities hold:
 *   1. with both counts <= BFIR_MAXCHANNELS the output bytes are those of bfir_engine_create_matrix with the same arguments;
 *   2. a matrix whose filters form blocks of at most 8 x 8 on the diagonal, with even block boundaries (channels that share
 *      a transform on the pair path stay together), gives for each block the bytes of a bfir_engine_create_matrix engine
 *      run on that block's channels; a diagonal matrix therefore the bytes of bfir_engine_create on each group of 8.
 * As on every matrix engine the bytes do not depend on bfir_engine_set_chunk or on how the blocks arrive.
 * BFIR_MIMO_MAC=0|1, read at creation, forbids or forces the wide MAC kernel (k_mac_mimo) on an engine whose counts are
 * both <= 8, where the matrix engine's kernel can run instead: the same bits, the default is the matrix engine's. */
bfir_engine *bfir_engine_create_mimo(int filter_length, int filter_blocks, int realsize, int n_inputs, int n_outputs,
                                     int in_format, int out_format, int device, int *err);

/* Two partition lengths in one engine ("nup": non-uniform partitioning): a long impulse response at a small block length
 * without a partition count that grows with it.  The head level convolves taps [0, D), D = head_blocks * filter_length,
 * in partitions of filter_length = L; the tail level the taps from D on in tail_blocks partitions of tail_ratio * L.  The
 * engine computes the linear convolution a uniform engine of partition L computes, with no added latency and L-frame
 * blocks at its interface:  y[n] = y_head[n] + z[n - D],  z the tail's output in blocks of tail_ratio * L from sample 0
 * (z[m] = 0 for m < 0).  A tail block is transformed when its last L-block has arrived and first read head_blocks -
 * tail_ratio + 1 blocks later, hence head_blocks >= tail_ratio.  The output sample is one addition in working precision,
 * head first, each term after the output scale; format conversion, overflow statistics and the NaN guard (sample 0 of
 * every L-block) act on the sum.  The output does not depend on how the blocks arrive (one call or many, host or
 * device pointers, any bfir_engine_set_chunk).  While the filters do not reach past D the tail does no work and the
 * output is, bit for bit, that of bfir_engine_create(L, head_blocks, ...) run in direct mode or on channel pairs.
 * A diagonal engine, 1 <= channels <= BFIR_MAXCHANNELS; an odd channel count runs one channel per transform.
 * BFIR_ERR_ARG: tail_ratio not a power of two or below 2, head_blocks < tail_ratio, tail_blocks < 1.
 * BFIR_ERR_UNSUPPORTED: filter_length or tail_ratio * filter_length outside what bfir_engine_create takes for realsize; a
 * frame format other than FLOAT_LE / FLOAT64_LE.  Arguments are checked before the device.
 * run, run_device, sync, get_overflow, set_chunk, is_initialized, set_profiling, get_profile (the sum of both levels) and
 * destroy work on it unchanged in meaning, in blocks of L frames.  bfir_engine_reset discards ALL signal state of such an
 * engine -- both delay lines, both time histories, the tail's partial input block and its queued output -- and zeroes
 * the counters; the engine then behaves as newly created with the same coefficients.  (The plain engine keeps
 * input_timecbuf across a reset, a quirk of the reference with no two-level meaning.)
 * bfir_engine_set_coeff, _set_coeff_at, _read_coeff, the matrix calls and the uniform fade calls (the fade of such an engine is
 * bfir_engine_set_coeff_nup_fade) return BFIR_ERR_UNSUPPORTED on
 * it; the three nup calls the same on every other kind of engine. */
bfir_engine *bfir_engine_create_nup(int filter_length, int head_blocks, int tail_ratio, int tail_blocks, int realsize,
                                    int channels, int in_format, int out_format, int device, int *err);
/* coeffs[n]: `length` taps in working precision, length <= D + tail_blocks * tail_ratio * L (more: BFIR_ERR_ARG); split
 * at D, ragged ends zero-filled as coeff::preprocess_coeff does.  A NaN/Inf tap: BFIR_ERR_COEFF and the engine is
 * uninitialised.  Mid-stream both delay lines are kept: the head uses the new filters from the next block, the tail from
 * the next tail block that completes, and tail output already queued still plays -- the change reaches the output tap by
 * tap within head_blocks + tail_ratio blocks.  A tail that had no taps starts with the next tail block that begins, on an
 * empty delay line. */
int bfir_engine_set_coeff_nup(bfir_engine *e, const void *const *coeffs, int n_coeffs, int length, double scale);
/* partition spectrum `block` of `channel`: level 0 = head (2 L reals), 1 = tail (2 tail_ratio L reals); grouped layout */
int bfir_engine_read_coeff_nup(bfir_engine *e, int level, int channel, int block, void *dst);

/* Three or four partition lengths in one engine: the two-level engine above with more tails.  Level k (0 <= k < n_levels)
 * has blocks[k] partitions of L_k, L_0 = filter_length and L_k = ratios[k] * L_(k-1) (ratios[0] must be 1), and convolves
 * taps [D_k, D_(k+1)), D_0 = 0 and D_k = D_(k-1) + blocks[k-1] * L_(k-1).  With z_k level k's overlap-save output in blocks
 * of L_k from sample 0 (z_k[m] = 0 for m < 0) the engine computes
 *   y[n] = ((y_0[n] + z_1[n - D_1]) + z_2[n - D_2]) + z_3[n - D_3]
 * -- the uniform engine's convolution, L_0-frame blocks at the interface, no added latency -- the additions in working
 * precision and in that order, each term after the output scale; format conversion, overflow statistics and the NaN guard
 * act on the sum.  A level whose tap range holds no taps does no work and adds nothing: filters that end at or before D_2
 * give the bytes of bfir_engine_create_nup(L_0, blocks[0], ratios[1], blocks[1], ...), n_levels = 2 the same.
 * Everything else is as for two levels: 1 <= channels <= BFIR_MAXCHANNELS, an odd count one channel per transform; the
 * output does not depend on how the blocks arrive; bfir_engine_reset discards all signal state of all levels.
 * BFIR_ERR_ARG: n_levels outside 2 .. BFIR_MAX_LEVELS; a null array; ratios[0] != 1; a ratios[k], k >= 1, that is not a
 * power of two >= 2; a blocks[k] < 1; D_k < L_k for some k >= 1 (a block of level k must be complete before it is read:
 * for two levels, head_blocks >= tail_ratio).  BFIR_ERR_UNSUPPORTED: an L_k outside what bfir_engine_create takes for
 * realsize; a frame format other than FLOAT_LE / FLOAT64_LE.  Arguments are checked before the device.
 * Such an engine is a kind of its own: bfir_engine_set_coeff, _set_coeff_at, _read_coeff, the matrix calls, the uniform fade calls
 * (its fade is bfir_engine_set_coeff_levels_fade)
 * and the three nup calls return BFIR_ERR_UNSUPPORTED on it, the three levels calls the same on every other kind of
 * engine (one from bfir_engine_create_nup included). */
#define BFIR_MAX_LEVELS 4
bfir_engine *bfir_engine_create_levels(int filter_length, int n_levels, const int *blocks, const int *ratios,
                                       int realsize, int channels, int in_format, int out_format, int device, int *err);
/* coeffs[n]: `length` taps in working precision, length <= D_(n_levels) (more: BFIR_ERR_ARG); split at every D_k, ragged
 * ends zero-filled.  A NaN/Inf tap: BFIR_ERR_COEFF and the engine is uninitialised.  Mid-stream every delay line is kept:
 * the head uses the new filters from the next block, level k from its next block that completes, and ring contents
 * already written still play.  A level that gains taps starts with its next block that begins, on an empty delay line; a
 * level that loses its taps stops, and its queued output plays out. */
int bfir_engine_set_coeff_levels(bfir_engine *e, const void *const *coeffs, int n_coeffs, int length, double scale);
/* partition spectrum `block` of `channel` on level `level`: 2 L_level reals, grouped layout */
int bfir_engine_read_coeff_levels(bfir_engine *e, int level, int channel, int block, void *dst);

/* The matrix form of the engine above: n_inputs inputs, n_outputs outputs, one filter h_{o,i} per (output, input) pair, every
 * filter convolved on the same two to four partition lengths:
 *   y_o[n] = ((y_0,o[n] + z_1,o[n - D_1]) + z_2,o[n - D_2]) + z_3,o[n - D_3],
 * y_0,o and z_k,o the sums over the inputs that bfir_engine_create_matrix(L_k, blocks[k], ...) computes from taps
 * [D_k, D_(k+1)) of every filter.  n_levels is 2 .. BFIR_MAX_LEVELS (there is no separate two-level call); blocks, ratios,
 * realsize, the frame formats and their errors are those of bfir_engine_create_levels, 1 <= n_inputs, n_outputs <=
 * BFIR_MAXCHANNELS (else BFIR_ERR_ARG).  Arguments are checked before the device: BFIR_ERR_NO_DEVICE only for valid ones.
 * Filters that all end at or before D_1 give the bytes of bfir_engine_create_matrix(L_0, blocks[0], ...).  While some level
 * beyond the first has taps and the rows of outputs 2p and 2p + 1 read every input, the bytes of those two outputs do not
 * depend on whether further outputs exist.  The output does not depend on bfir_engine_set_chunk or on how the blocks arrive.  Frames: n_inputs samples in,
 * n_outputs samples out; bfir_engine_get_overflow(e, o, ..) is output o's; bfir_engine_reset discards all signal state.
 * Such an engine is a kind of its own: every other bfir_engine_set_coeff*, _read_coeff* and fade call returns
 * BFIR_ERR_UNSUPPORTED on it, and the three calls below the same on every other kind of engine.  Its crossfade is
 * bfir_engine_set_coeff_matrix_levels_fade; bfir_engine_fade_remaining_levels reports it (0 while none is pending). */
bfir_engine *bfir_engine_create_matrix_levels(int filter_length, int n_levels, const int *blocks, const int *ratios,
                                              int realsize, int n_inputs, int n_outputs, int in_format, int out_format,
                                              int device, int *err);
/* coeffs[o * n_inputs + i]: the taps of h_{o,i} in working precision, or NULL = no path from input i to output o;
 * lengths[o * n_inputs + i]: that filter's tap count, 0 .. D_(n_levels) (outside: BFIR_ERR_ARG; 0 taps are no path).  Each
 * filter is split at every D_k, ragged ends zero-filled; a filter that ends at or before D_k has no partitions on level k
 * and is skipped there, never multiplied by zero, and a level on which no filter has taps does no work at all.  An input is
 * read if any filter of its column has taps on any level; a NaN on an input that is not read reaches no output and no
 * verdict (while there is one, every level transforms one channel at a time).  A NaN/Inf tap: BFIR_ERR_COEFF, nothing is
 * uploaded and the engine is uninitialised.  Mid-stream the rules of bfir_engine_set_coeff_levels hold per level. */
int bfir_engine_set_coeff_matrix_levels(bfir_engine *e, const void *const *coeffs, const int *lengths, double scale);
/* partition spectrum `block` of h_{output,input} on level `level`: 2 L_level reals, grouped layout */
int bfir_engine_read_coeff_matrix_levels(bfir_engine *e, int level, int output, int input, int block, void *dst);

/* bfir_engine_create_matrix_levels with the channel cap of bfir_engine_create_mimo: n_inputs -> n_outputs with up to
 * BFIR_MIMO_MAXCHANNELS of each, every filter on the same two to four partition lengths -- long room responses at a short
 * block length through one wide matrix (the reference stops at BF_MAXCHANNELS, brutefir/global.h:21, and at uniform
 * partitions, brutefir/brutefir.cpp:738-810).  The head and every tail level are mimo engines; FLOAT_LE / FLOAT64_LE frames,
 * no dither, one engine.  Checked before the device is touched, in this order: a count outside 1 ... BFIR_MIMO_MAXCHANNELS
 * is BFIR_ERR_ARG; whatever bfir_engine_create_levels refuses about filter_length, n_levels, blocks, ratios and realsize
 * keeps its code; an integer or big-endian frame format is BFIR_ERR_UNSUPPORTED; valid arguments without a GPU give
 * BFIR_ERR_NO_DEVICE.  Device memory that does not suffice: BFIR_ERR_HIP, everything already allocated freed.  The filters
 * alone take
 *   n_inputs * n_outputs * 2 * realsize * D_(n_levels)  bytes,  D_(n_levels) = sum_k blocks[k] * L_k  the capacity in taps,
 * and twice that from the first crossfade on (64 x 64, fp32, 65536 taps: 2 GiB per set); beside them every level keeps a
 * delay line of n_inputs * (2 chunk_k + blocks[k] + ceil(D_k / L_k) + 1) spectra and two product buffers of n_outputs *
 * chunk_k spectra of 2 L_k reals, chunk_k = ceil(blocks per launch / (L_k / L_0)).
 * With unchanged meaning on it: bfir_engine_set_coeff_matrix_levels, _read_coeff_matrix_levels,
 * _set_coeff_matrix_levels_fade, _fade_remaining_levels, _run, _run_device, _sync, _reset, _get_overflow (channel = output,
 * 0 ... n_outputs - 1), _set_chunk, _set_profiling, _get_profile, _is_initialized, _destroy.  BFIR_ERR_UNSUPPORTED on it:
 * every other coefficient, read and fade call, and the four delay calls (the delay table holds BFIR_MAXCHANNELS channels).
 * A launch (bfir_engine_set_chunk) past the grid of any level's MAC kernel, the one of a fading launch included, is refused
 * with BFIR_ERR_UNSUPPORTED before anything is allocated or queued; the default never gets there.
 * A level's MAC is k_mac_mimo where either count passes BFIR_MAXCHANNELS; within it the matrix engine's kernel unless
 * BFIR_MIMO_MAC=1 (the same bits).  The chain of bfir_engine_create_mimo holds per level, so:
 *   1. with both counts <= BFIR_MAXCHANNELS the output bytes are those of bfir_engine_create_matrix_levels with the same
 *      arguments, plain and through a crossfade;
 *   2. filters that all end at or before D_1 give the bytes of bfir_engine_create_mimo(L_0, blocks[0], ...);
 *   3. a matrix whose filters form blocks of at most 8 x 8 on the diagonal, every block with even input and output counts
 *      and every block with taps on the same levels, gives for each block the bytes of a bfir_engine_create_matrix_levels
 *      engine run on that block's channels and lengths (a block without taps on a level that another block reaches has that
 *      level's zeros ADDED to its samples, which turns a sample of -0.0 into +0.0);
 *   4. the bytes do not depend on bfir_engine_set_chunk, on how the blocks arrive (one call, many, one block at a time on
 *      the latency path, host or device pointers), or on BFIR_MFADE_DUO.
 * BFIR_MFADE_DUO=0|1, read at creation: a launch of a level that needs both filter sets of a crossfade runs the level's MAC
 * twice (0) or both sets in one pass over the delay line (1: k_mac_duo, or k_wduo on a level whose MAC is k_mac_mimo).  The
 * default is 1 on every level: the one pass was the faster form in the measurements of both kernels. */
bfir_engine *bfir_engine_create_mimo_levels(int filter_length, int n_levels, const int *blocks, const int *ratios,
                                            int realsize, int n_inputs, int n_outputs, int in_format, int out_format,
                                            int device, int *err);

void bfir_engine_destroy(bfir_engine *e);

/* brutefir::is_initialized */
int bfir_engine_is_initialized(const bfir_engine *e);

/* brutefir::set_coeff(void **coeffs, int n_coeffs, int length,
 * int coeff_blocks, double scale)  (brutefir.cpp:179-228) with
 * coeff::preprocess_coeff (coeff.cpp:292-354) and convolver_coeffs2cbuf
 * (fftw_convolver.cpp:474-537) done on the device.  coeffs[n]: host array of
 * `length` taps in working precision (float for realsize 4, double for 8).
 * Returns 0, or BFIR_ERR_COEFF on a NaN/Inf tap. */
int bfir_engine_set_coeff(bfir_engine *e, const void *const *coeffs, int n_coeffs, int length,
                          int coeff_blocks, double scale);
/* coeffs[o * n_inputs + i]: taps of h_{o,i} in working precision, or NULL = no path from input i to output o
 * (skipped, not multiplied by zero).  length / coeff_blocks / scale as bfir_engine_set_coeff.  A NaN/Inf tap:
 * BFIR_ERR_COEFF and the engine is uninitialised.  Mid-stream the delay line is kept and the next block uses the
 * new filters. */
int bfir_engine_set_coeff_matrix(bfir_engine *e, const void *const *coeffs, int length, int coeff_blocks,
                                 double scale);
/* bfir_engine_set_coeff for engine `engine_index` of a batch */
int bfir_engine_set_coeff_at(bfir_engine *e, int engine_index, const void *const *coeffs,
                             int n_coeffs, int length, int coeff_blocks, double scale);

/* Crossfaded coefficient change: the engine-level form of fftw_convolver::convolver_crossfade_inplace
 * (brutefir/fftw_convolver.cpp:275-321), which convolves one block with both filter sets and blends the two time signals
 * with a linear ramp.  Load a second filter set and fade to it over the next fade_blocks blocks the engine processes;
 * arguments as bfir_engine_set_coeff, fade_blocks >= 1.  With K = fade_blocks, L = filter_length, t0 the first block
 * processed after the call and y_old / y_new the blocks the old and the new filters give on the same delay line (working
 * precision, after the output scale), sample n of block t0 <= t < t0 + K is, with m = (t - t0) L + n,
 *     y_old[n] * (1.0 - f * (real)m) + y_new[n] * f * (real)m,    f = 1 / (real)(K L - 1)
 * -- with K = 1 the reference's loop (:298-304), C's promotions included (fp32: the first product and the sum are double);
 * before t0 the output is y_old, from t0 + K on y_new.  fp64 uses the same roles, old faded out and new faded in: the
 * reference's fp64 branch (:308-314) reads its operands from the wrong halves of buffer_cbuf, which
 * bfir_convolver_crossfade_inplace reproduces on purpose and the engine does not.  Overflow statistics, the NaN guard and
 * the format conversion act on the blended sample.  The fade does not depend on how the blocks arrive (one call or many,
 * host or device pointers, any bfir_engine_set_chunk).
 * Returns BFIR_ERR_STATE on an engine without coefficients and while another fade is pending or running (poll
 * bfir_engine_fade_remaining); BFIR_ERR_ARG for fade_blocks < 1 or K L > 2^24 (m must be exact as a float);
 * BFIR_ERR_UNSUPPORTED on a batch, on an engine that dithers its output (apply_dither with an integer format), and for
 * the call that does not match the engine's kind (matrix / diagonal); BFIR_ERR_COEFF on a NaN/Inf tap -- unlike
 * bfir_engine_set_coeff the engine then stays initialised and keeps running the old filters.
 * A plain bfir_engine_set_coeff* during a fade cancels it and cuts hard; bfir_engine_reset ends it at once with the new
 * set active; bfir_engine_read_coeff* reads the active set: the old one until the fade's last block has been queued. */
int bfir_engine_set_coeff_fade(bfir_engine *e, const void *const *coeffs, int n_coeffs, int length,
                               int coeff_blocks, double scale, int fade_blocks);
/* The same for a matrix engine; coeffs[o * n_inputs + i] or NULL as bfir_engine_set_coeff_matrix.  A filter that is NULL
 * in one set and present in the other fades in or out.  The fade's blocks take the channel-pair path only if every input
 * feeds an output under BOTH sets; after the fade the new set decides. */
int bfir_engine_set_coeff_matrix_fade(bfir_engine *e, const void *const *coeffs, int length,
                                      int coeff_blocks, double scale, int fade_blocks);
/* A LIST of pairs of a matrix engine replaced (bfir_engine_create_matrix, bfir_engine_create_mimo): coeffs[k], k < n_pairs,
 * is the new h_{outputs[k], inputs[k]}, `length` taps in working precision, or NULL = the path is removed; length /
 * coeff_blocks / scale as bfir_engine_set_coeff_matrix.  The MERGED set is the active set with exactly the listed pairs
 * replaced: every other pair keeps its spectra and its partition count byte for byte, and only the listed filters are
 * uploaded and transformed.  One moving source of a 64 x 64 renderer is one column: 64 filters out of 4096.
 * The plain call leaves the engine, byte for byte, as bfir_engine_set_coeff_matrix with the merged set would: filter store,
 * partition counts and the choice between the channel-pair and the direct path.  The delay line is kept.  During a fade it
 * cancels the fade (the old set stays active) and then patches the old set.
 * The fade call is bfir_engine_set_coeff_matrix_fade with the merged set as the new set -- the same blocks t0 .. t0 + K - 1,
 * blend and f, bfir_engine_fade_remaining, bfir_engine_read_coeff_matrix reading the old set until the fade's last block
 * is queued, a plain set call cancelling it, bfir_engine_reset ending it with the merged set active, the pair-path rule --
 * with one difference: during the fade y_new is NOT the new set's own fma chain.  Its spectra are the old set's products
 * plus the listed pairs' difference,
 *     Y2[o] = Y[o] + sum over the listed (o, i), in input order, of
 *             ( sum_{p < nb_new} X_i[t - p] H2_{o,i,p}  -  sum_{p < nb_old} X_i[t - p] H_{o,i,p} ),
 * the new filter's terms first, then the old filter's, in one fma chain behind Y[o].  So the fading blocks agree with those
 * of bfir_engine_set_coeff_matrix_fade to the merged set within rounding, NOT bitwise; an output without a listed pair is
 * blended with itself (y_new = y_old bitwise).  Before t0 the bytes are those of an engine that was never patched; from
 * t0 + K on those of an engine that faded to the merged set with bfir_engine_set_coeff_matrix_fade.  As every fade, the
 * output does not depend on how the blocks arrive.  A listed pair without a filter in either set is never loaded: nothing is
 * multiplied by zero, an input no filter reads keeps its NaN to itself.
 * All refusals come before the device is touched and change nothing.  BFIR_ERR_ARG: a null e, outputs, inputs or coeffs;
 * n_pairs < 1; an index outside the matrix; the same pair listed twice; length < 0; coeff_blocks < 1; for the fade,
 * fade_blocks < 1 or K L > 2^24.  BFIR_ERR_STATE: an engine without coefficients; for the fade, a fade pending or running.
 * BFIR_ERR_UNSUPPORTED: an engine of any other kind (diagonal, batch, two-level, multi-level, multi-level matrix or mimo);
 * for the fade, an engine that dithers its output.  BFIR_ERR_COEFF: a NaN/Inf tap, found before anything is uploaded -- the
 * engine keeps its filters and, unlike after bfir_engine_set_coeff_matrix, stays initialised. */
int bfir_engine_set_coeff_matrix_pairs(bfir_engine *e, int n_pairs, const int *outputs, const int *inputs,
                                       const void *const *coeffs, int length, int coeff_blocks, double scale);
int bfir_engine_set_coeff_matrix_pairs_fade(bfir_engine *e, int n_pairs, const int *outputs, const int *inputs,
                                            const void *const *coeffs, int length, int coeff_blocks, double scale,
                                            int fade_blocks);

/* Coefficient banks (bfir_engine_create_matrix, bfir_engine_create_mimo; both precisions): filter sets that stay on the
 * device, transformed once, and are switched by index -- BruteFIR's model of coefficient sets loaded at start and a filter
 * pointed at another set at run time (the `cfc` command).  A bank is a store of n_entries filters in the form of the
 * engine's own filter store ([n_entries][filter_blocks][2 filter_length] spectra in the engine's precision and spectrum
 * layout) on the engine's device.  The four bfir_engine_set_coeff_matrix_*bank* calls below are the four calls with taps
 * with a bank index in place of every filter: where those upload and transform, these copy rows on the device, all listed
 * rows in ONE kernel launch (k_bank_gather), and take no host taps.  Every entry keeps the partition count it was loaded
 * with, so the filters of one call may have different counts (which the calls with taps, with one coeff_blocks per call,
 * cannot give).  The engine's sets are COPIES: loading over an entry, or destroying the bank, changes nothing in the engine.
 * Multi-level kinds (bfir_engine_create_matrix_levels, _mimo_levels) have no banks of this group: theirs, one store per
 * level, are the bfir_engine_levels_bank_* calls further below.  Every call of this group returns BFIR_ERR_UNSUPPORTED on an engine of any kind but the two above, and
 * BFIR_ERR_ARG for a null e.
 *
 * bfir_engine_bank_create allocates the store; every entry is empty (partition count 0) and the store is not cleared.
 * BFIR_ERR_ARG: n_entries < 1.  BFIR_ERR_STATE: the engine has a bank.  BFIR_ERR_HIP: the allocation failed; there is then
 * no bank.
 * bfir_engine_bank_destroy waits for queued work and frees the bank (no bank: BFIR_OK, nothing happens);
 * bfir_engine_destroy does the same.  The engine's active filters and a running fade are untouched.
 * bfir_engine_bank_entries: the entry count, 0 without a bank.  bfir_engine_bank_blocks: the partition count of an entry,
 * 0 = empty; BFIR_ERR_ARG for an entry outside the bank (any entry, without one). */
int bfir_engine_bank_create(bfir_engine *e, int n_entries);
int bfir_engine_bank_destroy(bfir_engine *e);
int bfir_engine_bank_entries(const bfir_engine *e);
int bfir_engine_bank_blocks(const bfir_engine *e, int entry);
/* Entries first .. first + n - 1 written: coeffs[k] is `length` taps in working precision, or NULL = the entry becomes empty;
 * length / coeff_blocks / scale as bfir_engine_set_coeff_matrix, and the entry's partition count is min(coeff_blocks,
 * filter_blocks).  All n filters go up in one upload and one transform launch, after queued work has finished.  Calls may
 * differ in length, coeff_blocks and scale.  An entry's spectra are, byte for byte, those bfir_engine_set_coeff_matrix
 * gives a filter of the same taps, coeff_blocks and scale.
 * BFIR_ERR_ARG: a null coeffs, n < 1, first < 0, length < 0, coeff_blocks < 1, first + n past the bank.  BFIR_ERR_STATE: no
 * bank (checked before the range).  BFIR_ERR_COEFF: a NaN/Inf tap in any filter, found before anything is uploaded -- the
 * bank is unchanged. */
int bfir_engine_bank_load(bfir_engine *e, int first, int n, const void *const *coeffs, int length, int coeff_blocks,
                          double scale);
/* Partition spectrum `block` of an entry (2 filter_length reals) in the form bfir_engine_read_coeff_matrix gives.  A block at
 * or past the entry's partition count reads as zeros (every block of an empty entry): what a set call writes there.
 * BFIR_ERR_ARG: a null dst, block outside 0 .. filter_blocks - 1, an entry outside the bank.  BFIR_ERR_STATE: no bank
 * (checked before the entry). */
int bfir_engine_bank_read(bfir_engine *e, int entry, int block, void *dst);
/* bfir_engine_set_coeff_matrix, _matrix_fade, _matrix_pairs and _matrix_pairs_fade with bank entries: entries[o * n_inputs +
 * i] (the whole matrix) or entries[k] for the pair (outputs[k], inputs[k]) is a bank index, or -1 = no path (the NULL of
 * the calls with taps; in a pairs call the path is removed).  A row of the engine's store written from an entry of count c
 * holds the entry's first c partitions and zeros up to filter_blocks, and its partition count is c: the row, the count
 * and so every output byte are those of the call with taps for the same taps, coeff_blocks = c and scale.  One entry may be
 * named for any number of pairs.  Everything else is the contract of the call with taps:
 *   _bank        a fade in progress is cancelled, the delay line is kept, the engine becomes initialised;
 *   _bank_fade   bfir_engine_set_coeff_matrix_fade, the new set gathered from the bank;
 *   _pairs_bank  bfir_engine_set_coeff_matrix_pairs, merged-set semantics included: every pair not listed keeps its
 *                spectra and its count; during a fade the fade is cancelled and the old set patched;
 *   _pairs_bank_fade  bfir_engine_set_coeff_matrix_pairs_fade, merged-set semantics and the patched y_new (NOT bitwise
 *                the whole-matrix fade's) included; nb_new of a listed pair is its entry's count.
 * With entries of different counts in one call the result is that of the merged set with every filter at its own count: the
 * plain calls give the bytes of one call with taps per distinct count.
 * All refusals come before the device is touched and change nothing, in this order.  BFIR_ERR_UNSUPPORTED: the engine's
 * kind; for the fade calls a batch or an engine that dithers its output.  BFIR_ERR_ARG: a null entries, outputs or inputs;
 * n_pairs < 1.  BFIR_ERR_STATE: no bank.  BFIR_ERR_ARG: a pair outside the matrix; the same pair listed twice; an index
 * outside -1 .. n_entries - 1.  BFIR_ERR_STATE: a named entry is empty.  For the fade calls BFIR_ERR_ARG: fade_blocks < 1 or
 * K L > 2^24, then BFIR_ERR_STATE: an engine without coefficients, a fade pending or running.  For _pairs_bank
 * BFIR_ERR_STATE: an engine without coefficients.
 * The calls wait for queued work, upload the table of the listed rows and the counts, launch the gather once on the
 * engine's stream and wait for it; they allocate nothing but the table when it grows (and, as every fade, the second set
 * at the engine's first fade). */
int bfir_engine_set_coeff_matrix_bank(bfir_engine *e, const int *entries);
int bfir_engine_set_coeff_matrix_bank_fade(bfir_engine *e, const int *entries, int fade_blocks);
int bfir_engine_set_coeff_matrix_pairs_bank(bfir_engine *e, int n_pairs, const int *outputs, const int *inputs,
                                            const int *entries);
int bfir_engine_set_coeff_matrix_pairs_bank_fade(bfir_engine *e, int n_pairs, const int *outputs, const int *inputs,
                                                 const int *entries, int fade_blocks);
/* Bank mixes: the four calls above with up to BFIR_BANK_MIX_TERMS terms (entry, weight) in place of one entry, so that a
 * filter BETWEEN measured entries (two neighbours on an arc, three on a triangle, four on a bilinear grid) or an entry AT A
 * LEVEL (distance attenuation, a volume, a polarity flip, a mute: a "sum" of one term) is still named by index.  The
 * transform is linear: the weighted sum of entry spectra is the spectrum of the same weighted sum of the taps, and no
 * transform runs.  One kernel launch (k_bank_mix) writes all listed rows; the MAC, the fades and the swap are untouched, and
 * after the call the store is a store like any other.
 * entries[k * n_terms + j] and weights[k * n_terms + j], j < n_terms <= BFIR_BANK_MIX_TERMS, belong to listed row k: k = o *
 * n_inputs + i in the whole-matrix calls, the pair (outputs[k], inputs[k]) in the pairs calls.  Every weight is converted
 * once to the working precision R (float or double; 1e-60 on a float engine converts to 0 and is handled like 0).  A term
 * is LIVE iff its entry is >= 0 and its converted weight is not zero; c_j is the partition count of a live term's entry.
 *   The row's partition count is c = max c_j over its live terms.  Without a live term the pair has no path: count 0, a
 *   row of zeros, the -1 of the calls above (in a pairs call the path is removed).  A mute is a removed path, nothing is
 *   multiplied by zero.
 *   With j_1 < j_2 < ... the live terms with c_j > p, in listed order, every stored real of partition p < c is
 *       r = fl(w_j1 * h_j1);  r = fl(r + fl(w_jm * h_jm)), m = 2, 3, ...
 *   every multiply and every add rounded on its own in R (no fma), the first product starting the sum (no 0 + ..., a
 *   product of -0 stays -0).  A term whose entry is shorter than p takes no part in partition p, and what that entry's
 *   store holds past its count is never read.  Partitions c .. filter_blocks - 1 are written as zeros.  Real and imaginary
 *   parts, DC and Nyquist and both spectrum layouts are all stored reals: the operation is elementwise.
 * So n_terms = 1 with weight 1 writes every byte of the call above for the same entry, and a restatement in IEEE single or
 * double arithmetic from bfir_engine_bank_read is exact to the bit wherever no product or sum is subnormal.
 * Everything not said here is the contract of the corresponding call above, word for word: the merged-set semantics of
 * the pairs calls; the plain call cancels a fade and keeps the delay line; the whole-matrix plain call initialises the
 * engine; the fades are bfir_engine_set_coeff_matrix_fade / _pairs_fade with the mixed set as the new set (the patched
 * y_new of a pairs fade with nb_new = the row's count c); bfir_engine_fade_remaining, bfir_engine_reset and the pair-path
 * rule behave as there.
 * All refusals come before the device is touched and change nothing, in this order.  BFIR_ERR_ARG: a null e.
 * BFIR_ERR_UNSUPPORTED: the engine's kind (the kinds of the calls above); for the fade calls a batch or an engine that
 * dithers its output.  BFIR_ERR_ARG: a null entries, weights, outputs or inputs; n_pairs < 1; n_terms outside 1 ..
 * BFIR_BANK_MIX_TERMS.  BFIR_ERR_STATE: no bank.  BFIR_ERR_ARG: a pair outside the matrix; the same pair listed twice; an
 * index outside -1 .. n_entries - 1, live or not; a weight that is NaN or infinite, or becomes infinite in the working
 * precision.  BFIR_ERR_STATE: a live term names an empty entry (a term of weight 0 may name one).  For the fade calls
 * BFIR_ERR_ARG: fade_blocks < 1 or K L > 2^24, then BFIR_ERR_STATE: an engine without coefficients, a fade pending or
 * running.  For _pairs_bank_mix BFIR_ERR_STATE: an engine without coefficients.
 * The calls wait for queued work, upload one table, launch k_bank_mix once on the engine's stream and wait for it; they
 * allocate nothing but that table when it grows (and, as every fade, the second set at the engine's first fade).
 * Out of scope: mixes on the multi-level kinds (BFIR_ERR_UNSUPPORTED there) -- theirs, over the bank of
 * bfir_engine_levels_bank_*, are the bfir_engine_set_coeff_matrix_levels_*bank_mix* calls further below; a gain change that
 * keeps a pair's current entry without naming it; more than BFIR_BANK_MIX_TERMS terms; complex weights (phase or delay
 * interpolation). */
#define BFIR_BANK_MIX_TERMS 4
int bfir_engine_set_coeff_matrix_bank_mix(bfir_engine *e, int n_terms, const int *entries, const double *weights);
int bfir_engine_set_coeff_matrix_bank_mix_fade(bfir_engine *e, int n_terms, const int *entries, const double *weights,
                                               int fade_blocks);
int bfir_engine_set_coeff_matrix_pairs_bank_mix(bfir_engine *e, int n_pairs, const int *outputs, const int *inputs,
                                                int n_terms, const int *entries, const double *weights);
int bfir_engine_set_coeff_matrix_pairs_bank_mix_fade(bfir_engine *e, int n_pairs, const int *outputs, const int *inputs,
                                                     int n_terms, const int *entries, const double *weights,
                                                     int fade_blocks);
/* Blocks of a pending or running fade still to be processed; 0 = none.  < 0: error. */
int bfir_engine_fade_remaining(const bfir_engine *e);

/* The same crossfade (fftw_convolver::convolver_crossfade_inplace, brutefir/fftw_convolver.cpp:275-321, stretched over
 * fade_blocks blocks of the head length L) on an engine from bfir_engine_create_nup: `length` taps per channel, split at D
 * as bfir_engine_set_coeff_nup splits them.  With a_f the engine's block counter at the call and K = fade_blocks, sample m =
 * 0 .. K L - 1 of the fade, at absolute sample a_f L + m, is blend(S_old[m], S_new[m]) with the blend, f and d of
 * bfir_engine_set_coeff_fade and S_x = ((y_head,x + z_1,x) + z_2,x) + z_3,x: the sums of the levels under the filters active
 * at the call (x = old) and under the filters of the call (x = new), in working precision, head first, levels in order.
 * Both sets act on the whole signal history: there is no transient.  Format conversion, overflow statistics and the NaN
 * guard act on the blended sample.  Before block a_f the engine is an engine that never faded, from block a_f + K on one
 * that has had the new filters all along; the output does not depend on how the blocks arrive.
 * BFIR_ERR_ARG: a null engine or `coeffs`, negative counts, `length` above the engine's capacity, fade_blocks < 1 or
 * K L > 2^24.  BFIR_ERR_STATE: no coefficients yet, or a fade is pending or running (poll
 * bfir_engine_fade_remaining_levels).  BFIR_ERR_COEFF: a NaN or Inf tap at any level, refused before anything is uploaded
 * at any level: the engine stays initialised and keeps running the old filters (unlike bfir_engine_set_coeff_nup).
 * BFIR_ERR_UNSUPPORTED: an engine of another kind; or the new set reaches a level the old set does not -- that level runs
 * no forward transforms and so has no delay line to fade on; nothing changes.  The way round it: load the first set
 * zero-padded to the longest length that will ever be faded to (a level is active by `length`, not by the tap values).
 * A new set that is shorter is allowed: the level runs through the fade with no partitions for the new set and then stops
 * as a bfir_engine_set_coeff_nup of that length would stop it.
 * bfir_engine_set_coeff_nup / _levels during a fade ends it (fade_remaining 0) and behaves as it does mid-stream;
 * bfir_engine_reset ends it with the new set active at every level and all signal state gone; bfir_engine_read_coeff_nup /
 * _levels reads the head's old set while the fade remains (which set the other levels read is unspecified) and the new set
 * at every level once it is done.
 * Memory: the first fade allocates, per level, a second filter set, a second time ring and a second product buffer. */
int bfir_engine_set_coeff_nup_fade(bfir_engine *e, const void *const *coeffs, int n_coeffs, int length, double scale,
                                   int fade_blocks);
/* ... and on an engine from bfir_engine_create_levels (two levels included): the crossfade of
 * fftw_convolver::convolver_crossfade_inplace (brutefir/fftw_convolver.cpp:275-321) as bfir_engine_set_coeff_nup_fade
 * defines it above, the taps split at every D_k as bfir_engine_set_coeff_levels splits them. */
int bfir_engine_set_coeff_levels_fade(bfir_engine *e, const void *const *coeffs, int n_coeffs, int length, double scale,
                                      int fade_blocks);
/* ... and on an engine from bfir_engine_create_matrix_levels: the same crossfade (fftw_convolver::convolver_crossfade_inplace,
 * brutefir/fftw_convolver.cpp:275-321, stretched over fade_blocks head blocks) per output.  coeffs / lengths are
 * [o * n_inputs + i] as bfir_engine_set_coeff_matrix_levels takes them (NULL or 0 taps: no path).  With a_f the block counter
 * at the call and K = fade_blocks, sample m = 0 .. K L - 1 of output o is fade_blend(S_old,o[m], S_new,o[m], f, m) with the
 * blend, f and d of bfir_engine_set_coeff_fade and S_x,o = ((y_0,o + z_1,o) + z_2,o) + z_3,o under the filters active at the
 * call (old) and those of the call (new), each term the sum over the inputs that the matrix engine of that level computes.
 * Both sets act on the whole signal history: there is no transient.  Overflow statistics, the NaN guard and the frame store
 * act on the blended sample.
 * Errors.  BFIR_ERR_ARG: a null engine, `coeffs` or `lengths`; a length outside 0 .. D_(n_levels); fade_blocks < 1; K L >
 * 2^24.  BFIR_ERR_STATE: no coefficients yet, or a fade is pending or running.  BFIR_ERR_COEFF: a NaN / Inf tap in any filter
 * at any level, refused before anything is uploaded; the engine stays initialised on the old set.  BFIR_ERR_UNSUPPORTED: every
 * other kind of engine (this kind keeps refusing the five other fade calls); and a new set with taps on a level on which no
 * filter of the old set has any -- per level, not per filter; nothing changes.  The way round it: load the first set
 * zero-padded, as for bfir_engine_set_coeff_levels_fade.
 * Per-filter reach.  A filter that is NULL or shorter in one set and present or longer in the other fades in or out; on a
 * level it has partition count 0 in the set where it does not reach that level and is skipped there, never multiplied by
 * zero.  A new set that reaches no active tail level at all stops that level after the fade, as a
 * bfir_engine_set_coeff_matrix_levels of those lengths would.  If neither set has taps beyond D_1 the fade is the one of
 * bfir_engine_set_coeff_matrix_fade on bfir_engine_create_matrix(L_0, blocks[0], ...).
 * Front end: the rule of bfir_engine_set_coeff_matrix_fade.  During the fade a level pairs channels only while every input
 * is read under BOTH sets (an input is read if any filter of its column has taps on any level of that set); after the fade
 * the new set decides.  A level that changes mode does so as after a bfir_engine_set_coeff_matrix_levels mid-stream.
 * Byte identities.  Blocks before a_f are those of an engine that never faded.  If both sets read every input, or the engine
 * cannot pair channels at all, blocks from a_f + K on are those of an engine that has had the new filters all along; else
 * they agree with it to rounding (pair and direct transforms round differently).  The output does not depend on
 * bfir_engine_set_chunk or on how the blocks arrive.
 * bfir_engine_set_coeff_matrix_levels during a fade ends it and cuts hard; bfir_engine_reset ends it with the new set active
 * at every level; bfir_engine_read_coeff_matrix_levels reads the head's old set while the fade remains and the new set
 * afterwards.  Memory: the first fade allocates, per level, a second filter set with its per-filter partition counts, a
 * second time ring and a second product buffer, sized by n_outputs where the first ones are. */
int bfir_engine_set_coeff_matrix_levels_fade(bfir_engine *e, const void *const *coeffs, const int *lengths, double scale,
                                             int fade_blocks);
/* A LIST of pairs of a multi-level matrix or mimo engine replaced (bfir_engine_create_matrix_levels, _create_mimo_levels;
 * bfir_engine_set_coeff_matrix_pairs and _pairs_fade keep refusing these kinds): coeffs[k], k < n_pairs, is the new
 * h_{outputs[k], inputs[k]} with lengths[k] taps of its own, 0 .. D_(n_levels); a NULL pointer or 0 taps removes the path.
 * The taps are split at every D_k as bfir_engine_set_coeff_matrix_levels splits them.  The MERGED set is the active set with
 * exactly the listed pairs replaced: on every level every other pair keeps its spectra and its partition count, and only
 * the listed filters are uploaded and transformed.  One moving source of a 64 x 64 renderer is one column: 64 filters out
 * of 4096.
 * The plain call leaves every level as bfir_engine_set_coeff_matrix_levels with the merged set, made at the same block,
 * would: the filter store (byte for byte over the partitions below each pair's count, zeros past it), the counts, which
 * levels are active -- a level the merged set newly reaches starts with its next block that begins, one it no longer
 * reaches stops -- and the choice between the channel-pair and the direct path.  Every delay line is kept.  Unlike the
 * uniform kind's call it does not cut a fade: while one is pending or running it returns BFIR_ERR_STATE, because a tail
 * level that has passed its last old block already runs the new set and there is no single active set to patch.
 * The fade call is bfir_engine_set_coeff_matrix_levels_fade to the merged set -- the same blocks a_f .. a_f + K - 1, blend
 * and f, bfir_engine_fade_remaining_levels, bfir_engine_reset ending it with the merged set active at every level, a
 * whole-matrix set call cutting it, the per-level refusal, the stop of a level the merged set leaves, the front-end rule --
 * with one difference, the one bfir_engine_set_coeff_matrix_pairs_fade has: on every level the new set's product spectra
 * are NOT the new set's own fma chain but the old set's products plus the listed pairs' difference,
 *     Y2[o] = Y[o] + sum over the listed (o, i), in input order, of
 *             ( sum_{p < nb_new} X_i[t - p] H2_{o,i,p}  -  sum_{p < nb_old} X_i[t - p] H_{o,i,p} ),
 * the new filter's partitions first, then the old filter's negated, in one fma chain behind Y[o], with that level's counts.
 * This holds for every launch that takes both sets: the head while it fades, a tail level up to its last old block, and
 * the blocks a tail level had already run when the call was made.  An output without a listed pair is blended with itself.
 * Identities (r_max = L_last / L_0):
 *   - blocks before a_f are those of an engine that was never patched;
 *   - blocks from a_f + K + r_max on are bitwise those of an engine that faded to the merged set with
 *     bfir_engine_set_coeff_matrix_levels_fade at a_f, under that call's own condition (both sets read every input, or the
 *     engine cannot pair channels): a tail level runs the merged set's own chain from the block after its last old one, and
 *     the head first reads that block at most r_k - 1 blocks past the fade's end;
 *   - the fading blocks and the r_max blocks behind them agree with that engine within rounding, NOT bitwise;
 *   - the output does not depend on bfir_engine_set_chunk, on how the blocks arrive, or on BFIR_PATCH_FUSED.
 * BFIR_PATCH_FUSED=0|1, read at creation, multi-level kinds only: on a level whose MAC is k_mac_mimo a launch that takes both
 * sets runs the old set's MAC and the patch as two launches (0) or as one, k_wpatch (1); the same bits.  The default is 0:
 * the two launches measured faster ("Pair lists on multi-level engines").  Levels on k_mac_matrix and uniform engines always take the two launches.
 * A listed pair without a filter in either set is never loaded: nothing is multiplied by zero, an input no filter reads
 * keeps its NaN to itself.
 * All refusals come before the device is touched and change nothing.  BFIR_ERR_ARG: a null e, outputs, inputs, coeffs or
 * lengths; n_pairs < 1; an index outside the matrix; the same pair listed twice; a length outside 0 .. D_(n_levels); for the
 * fade, fade_blocks < 1 or K L > 2^24.  BFIR_ERR_STATE: an engine without coefficients, or a fade pending or running (both
 * calls).  BFIR_ERR_UNSUPPORTED: every other kind of engine; for the fade, a merged set with taps on a level no filter of the
 * old set reaches.  BFIR_ERR_COEFF: a NaN/Inf tap, found before anything is uploaded -- the engine keeps its filters and
 * stays initialised. */
int bfir_engine_set_coeff_matrix_levels_pairs(bfir_engine *e, int n_pairs, const int *outputs, const int *inputs,
                                              const void *const *coeffs, const int *lengths, double scale);
int bfir_engine_set_coeff_matrix_levels_pairs_fade(bfir_engine *e, int n_pairs, const int *outputs, const int *inputs,
                                                   const void *const *coeffs, const int *lengths, double scale,
                                                   int fade_blocks);

/* Coefficient banks of the multi-level matrix kinds (bfir_engine_create_matrix_levels, bfir_engine_create_mimo_levels; both
 * precisions): the banks of bfir_engine_bank_create for engines whose filters are split between levels.  The bank is one
 * store per level on the engine's device: level k holds [n_entries][blocks[k]][2 L_k] spectra in that level's precision and
 * spectrum layout, an entry being a row of that level's filter store that lives elsewhere.  The bank takes n_entries * 2 *
 * realsize * D_(n_levels) bytes (D_(n_levels) = the sum of blocks[k] L_k, the taps the engine holds per filter).  The four
 * bfir_engine_set_coeff_matrix_levels_*bank* calls are bfir_engine_set_coeff_matrix_levels, _levels_fade, _levels_pairs and
 * _levels_pairs_fade with a bank index in place of every filter: where those upload and transform level by level and row by
 * row, these copy rows on the device, all listed rows of ALL levels in ONE kernel launch (k_lbank_gather), and take no host
 * taps.  The engine's sets are COPIES: loading over an entry, or destroying the bank, changes nothing in the engine.  Every
 * call of this group returns BFIR_ERR_UNSUPPORTED on an engine of any kind but the two above (the ten bfir_engine_bank_* /
 * _set_coeff_matrix_*bank* calls above keep refusing these two), and BFIR_ERR_ARG for a null e.
 *
 * bfir_engine_levels_bank_create allocates the stores of all levels; every entry is empty (length 0) and the stores are not
 * cleared.  BFIR_ERR_ARG: n_entries < 1.  BFIR_ERR_STATE: the engine has a bank.  BFIR_ERR_HIP: an allocation failed; what
 * was allocated is freed and there is then no bank.
 * bfir_engine_levels_bank_destroy waits for queued work and frees the bank (no bank: BFIR_OK, nothing happens);
 * bfir_engine_destroy does the same.  The engine's active filters and a running fade are untouched.
 * bfir_engine_levels_bank_entries: the entry count, 0 without a bank.  bfir_engine_levels_bank_length: the taps an entry was
 * loaded with, 0 = empty.  bfir_engine_levels_bank_blocks: its partition count on `level` (0 .. n_levels - 1), 0 = the entry
 * does not reach that level.  Both: BFIR_ERR_ARG for an entry outside the bank (any entry, without one) or a level outside the
 * engine. */
int bfir_engine_levels_bank_create(bfir_engine *e, int n_entries);
int bfir_engine_levels_bank_destroy(bfir_engine *e);
int bfir_engine_levels_bank_entries(const bfir_engine *e);
int bfir_engine_levels_bank_length(const bfir_engine *e, int entry);
int bfir_engine_levels_bank_blocks(const bfir_engine *e, int entry, int level);
/* Entries first .. first + n - 1 written: coeffs[k] is lengths[k] taps in working precision, 0 .. D_(n_levels) as
 * bfir_engine_set_coeff_matrix_levels takes them; NULL or 0 taps = the entry becomes empty.  The n filters are split at every
 * D_k as that call splits them and every level they reach gets ONE upload and ONE transform launch for all n, after queued
 * work has finished; a level none of them reaches is not transformed into.  An entry holds, on every level, byte for byte the
 * partitions bfir_engine_set_coeff_matrix_levels gives a filter of the same taps, length and scale, and the host keeps its
 * length and its partition count on every level.  Calls may differ in scale.
 * BFIR_ERR_ARG: a null coeffs or lengths, n < 1, first < 0, a length outside 0 .. D_(n_levels), first + n past the bank.
 * BFIR_ERR_STATE: no bank (checked before the range).  BFIR_ERR_COEFF: a NaN/Inf tap in any filter, found before anything is
 * uploaded -- the bank is unchanged. */
int bfir_engine_levels_bank_load(bfir_engine *e, int first, int n, const void *const *coeffs, const int *lengths, double scale);
/* Partition spectrum `block` of an entry on `level` (2 L_level reals) in the form bfir_engine_read_coeff_matrix_levels gives.
 * A block at or past the entry's partition count on that level reads as zeros: what a set call writes there.
 * BFIR_ERR_ARG: a null dst, a level outside the engine, block outside 0 .. blocks[level] - 1, an entry outside the bank.
 * BFIR_ERR_STATE: no bank (checked before the entry). */
int bfir_engine_levels_bank_read(bfir_engine *e, int entry, int level, int block, void *dst);
/* bfir_engine_set_coeff_matrix_levels, _levels_fade, _levels_pairs and _levels_pairs_fade with bank entries: entries[o *
 * n_inputs + i] (the whole matrix) or entries[k] for the pair (outputs[k], inputs[k]) is a bank index, or -1 = no path (in a
 * pairs call the path is removed).  A row written from an entry holds, on level k, the entry's first count_k partitions and
 * zeros up to blocks[k], and its partition count there is count_k: the row, the counts and so every output byte are those of
 * the call with taps for the same taps, length and scale.  One entry may be named for any number of pairs.  Everything else
 * is the contract of the call with taps: the plain whole-matrix call cuts a fade; the plain pairs call returns
 * BFIR_ERR_STATE while a fade is pending or running; the fades refuse, per level, a new set that reaches a level the active
 * set does not; a newly reached level starts and a left one stops; the pairs fade keeps the merged-set semantics and the
 * patched y_new; bfir_engine_fade_remaining_levels and bfir_engine_reset behave as with taps.
 * All refusals come before the device is touched and change nothing, in this order.  BFIR_ERR_UNSUPPORTED: the engine's
 * kind.  BFIR_ERR_ARG: a null entries, outputs or inputs; n_pairs < 1.  BFIR_ERR_STATE: no bank.  BFIR_ERR_ARG: a pair outside
 * the matrix; the same pair listed twice; an index outside -1 .. n_entries - 1.  BFIR_ERR_STATE: a named entry is empty.
 * BFIR_ERR_UNSUPPORTED: a gather the kernel cannot make (a misaligned store, a partition that is not whole 16 bytes, more
 * than 65535 rows, a grid past the launch limits) -- never a skipped launch.  For the fade calls BFIR_ERR_ARG: fade_blocks < 1
 * or K L > 2^24, then BFIR_ERR_STATE: an engine without coefficients, a fade pending or running; for _pairs_bank
 * BFIR_ERR_STATE likewise.  For the fade calls then BFIR_ERR_UNSUPPORTED: the new set reaches a level the active one does
 * not, or a launch of the fade on an active level that does not fit its kernel's grid.
 * The calls wait for queued work, upload ONE table of the listed rows (row, entry, the count on every level) and the counts,
 * launch the gather once on the engine's stream for all levels and wait for it once; a pairs fade queues every active
 * level's copy of its store in front of the gather, and a level the fade with taps skips is skipped by the gather too.  They
 * transform nothing and allocate nothing but the table when it grows (and, as every fade, the second set at the engine's
 * first fade). */
int bfir_engine_set_coeff_matrix_levels_bank(bfir_engine *e, const int *entries);
int bfir_engine_set_coeff_matrix_levels_bank_fade(bfir_engine *e, const int *entries, int fade_blocks);
int bfir_engine_set_coeff_matrix_levels_pairs_bank(bfir_engine *e, int n_pairs, const int *outputs, const int *inputs,
                                                   const int *entries);
int bfir_engine_set_coeff_matrix_levels_pairs_bank_fade(bfir_engine *e, int n_pairs, const int *outputs, const int *inputs,
                                                        const int *entries, int fade_blocks);
/* Bank mixes on the multi-level kinds: the four calls above with up to BFIR_BANK_MIX_TERMS terms (entry, weight) in place
 * of one entry, on engines from bfir_engine_create_matrix_levels and bfir_engine_create_mimo_levels in both precisions.  The
 * entries are those of the engine's levels bank (bfir_engine_levels_bank_create, _load).  The transform of every level is
 * linear, so no transform runs: one kernel launch (k_lbank_mix) writes the listed rows of all levels.
 * entries[k * n_terms + j] and weights[k * n_terms + j], j < n_terms <= BFIR_BANK_MIX_TERMS, belong to listed row k: k = o *
 * n_inputs + i in the whole-matrix calls, the pair (outputs[k], inputs[k]) in the pairs calls -- the layout of the uniform
 * mix calls (bfir_engine_set_coeff_matrix_bank_mix).
 * The operation is k_bank_mix's, applied per level.  Every weight is converted once to the working precision R.  A term is
 * LIVE iff its entry is >= 0 and its converted weight is not zero.  On level k, c_j,k is the partition count of a live
 * term's entry on that level (bfir_engine_levels_bank_blocks), and the row's count there is c_k = max c_j,k over its live
 * terms.  With j_1 < j_2 < ... the live terms with c_j,k > p, in listed order, every stored real of partition p < c_k is
 *       r = fl(w_j1 * h_j1);  r = fl(r + fl(w_jm * h_jm)), m = 2, 3, ...
 *   every multiply and every add rounded on its own in R (no fma), the first product starting the sum (no 0 + ..., a
 *   product of -0 stays -0).  Partitions c_k .. blocks[k] - 1 are zeros.  A term whose entry does not reach level k, or is
 *   shorter there than p, takes no part, and what its store holds past its count is never read.  A row without a live term
 *   is no path: count 0 on every level, zeros; in a pairs call the path is removed.  Nothing is multiplied by zero.
 * So n_terms = 1 with weight 1 writes every byte of the call above for the same entry, and a restatement in IEEE single or
 * double arithmetic from bfir_engine_levels_bank_read is exact to the bit wherever no product or sum is subnormal.
 * Everything else is the contract of the corresponding _levels_*bank* call above, word for word: the plain whole-matrix call
 * cuts a fade and initialises the engine; the plain pairs call returns BFIR_ERR_STATE while a fade is pending or running; the
 * fades refuse, per level, a new set that reaches a level the active set does not, "reaches" decided by the mixed rows'
 * counts c_k; a newly reached level starts and a left one stops; the pairs fade keeps the merged-set semantics and the
 * patched y_new, with nb_new = c_k; the front-end pairing rule, bfir_engine_fade_remaining_levels and bfir_engine_reset
 * behave as there.
 * All refusals come before the device is touched and change nothing, in this order.  BFIR_ERR_ARG: a null e.
 * BFIR_ERR_UNSUPPORTED: any kind but the two.  BFIR_ERR_ARG: a null entries, weights, outputs or inputs; n_pairs < 1; n_terms
 * outside 1 .. BFIR_BANK_MIX_TERMS.  BFIR_ERR_STATE: no bank.  BFIR_ERR_ARG: a pair outside the matrix; the same pair listed
 * twice; an index outside -1 .. n_entries - 1, live or not; a weight that is NaN or infinite, or becomes infinite in the
 * working precision.  BFIR_ERR_STATE: a live term names an empty entry (length 0; a dead term may name one).
 * BFIR_ERR_UNSUPPORTED: a launch the kernel cannot make (a misaligned store, a partition that is not whole 16 bytes, more
 * than 65535 rows, a grid past the launch limits) -- a launch is never skipped.  Then the refusals of the call with taps, in
 * its own order: for the fade calls BFIR_ERR_ARG: fade_blocks < 1 or K L > 2^24, then BFIR_ERR_STATE: an engine without
 * coefficients, a fade pending or running; for _pairs_bank_mix BFIR_ERR_STATE likewise; for the fade calls then
 * BFIR_ERR_UNSUPPORTED: the mixed set reaches a level the active one does not, or a launch of the fade on an active level
 * that does not fit its kernel's grid.
 * Cost: the calls wait for queued work, upload ONE table (per listed row: the row, its live terms, and per term the entry,
 * the weight and the count on every level) and the counts, launch k_lbank_mix once on the engine's stream for all levels
 * and wait for it once.  They transform nothing and allocate nothing but the table when it grows (and, as every fade, the
 * second set at the engine's first fade).
 * The four uniform mix calls keep returning BFIR_ERR_UNSUPPORTED on the multi-level kinds, and these four on the uniform. */
int bfir_engine_set_coeff_matrix_levels_bank_mix(bfir_engine *e, int n_terms, const int *entries, const double *weights);
int bfir_engine_set_coeff_matrix_levels_bank_mix_fade(bfir_engine *e, int n_terms, const int *entries, const double *weights,
                                                      int fade_blocks);
int bfir_engine_set_coeff_matrix_levels_pairs_bank_mix(bfir_engine *e, int n_pairs, const int *outputs, const int *inputs,
                                                       int n_terms, const int *entries, const double *weights);
int bfir_engine_set_coeff_matrix_levels_pairs_bank_mix_fade(bfir_engine *e, int n_pairs, const int *outputs, const int *inputs,
                                                            int n_terms, const int *entries, const double *weights,
                                                            int fade_blocks);
/* Head blocks of a pending or running fade (fftw_convolver.cpp:275-321 over fade_blocks blocks) of an engine from
 * bfir_engine_create_nup, _levels or _matrix_levels still to be processed; 0 = none.  BFIR_ERR_UNSUPPORTED on every other kind
 * of engine. */
int bfir_engine_fade_remaining_levels(const bfir_engine *e);

/* brutefir::run (brutefir.cpp:244-343) for n_blocks consecutive blocks.
 * inbuf/outbuf: HOST memory, n_blocks * filter_length interleaved frames in
 * the input/output format (for a batch: engine after engine, each
 * n_blocks*L frames).  Staged through pinned buffers with hipMemcpyAsync on
 * side streams, overlapped with compute.  Returns 0 or BFIR_ERR_NONFINITE. */
int bfir_engine_run(bfir_engine *e, const void *inbuf, void *outbuf, int n_blocks);

/* The same on DEVICE memory, asynchronous on `hip_stream` (a hipStream_t;
 * NULL = the engine's own stream).  Engine k reads d_in + k*in_stride_bytes
 * and writes d_out + k*out_stride_bytes.  The NaN verdict is delivered by
 * bfir_engine_sync.  Strides, counts and lengths that can pass 2^31 are int64_t,
 * never `long`: the reference's platform is MSVC (brutefir/brutefir.vcxproj:66-70),
 * where `long` has 32 bits, and one 8-channel stream of a day's audio is a 32 GiB stride. */
int bfir_engine_run_device(bfir_engine *e, const void *d_in, int64_t in_stride_bytes, void *d_out,
                           int64_t out_stride_bytes, int n_blocks, void *hip_stream);
/* Wait for all queued work; 0, or BFIR_ERR_NONFINITE if any block since the
 * last sync produced a non-finite first sample. */
int bfir_engine_sync(bfir_engine *e);

/* brutefir::reset (brutefir.cpp:346-367) */
void bfir_engine_reset(bfir_engine *e);

/* copy of brutefir's overflow[channel] (brutefir.cpp:326-334) */
int bfir_engine_get_overflow(bfir_engine *e, int channel, bfir_overflow *of);

/* ------------------------------------------------------------------ */
/* per-channel input and output delays, whole-sample and sub-sample:   */
/* the reference's delay class (brutefir/delay.hpp, delay.cpp) with    */
/* firwindow_kaiser (brutefir/firwindow.c)                             */
/* ------------------------------------------------------------------ */
#define BFIR_DELAY_INPUT  0
#define BFIR_DELAY_OUTPUT 1

/* delay::sample_sinc + firwindow_kaiser (delay.cpp:278-306, firwindow.c:89-210): the 2h+1 taps, h = half_filter_length, of
 * the filter that delays by h + subdelay/step_count samples, in realsize precision (float or double at `taps`).  Pure host
 * arithmetic, no device.  subdelay 0: a unit tap at index h, no window (delay.cpp:229-240).  Otherwise tap n is
 * sinc(pi ((n - h) - subdelay/step_count)), rounded to float first for realsize 4, times the Kaiser weights exactly as
 * firwindow_kaiser applies them for a non-zero offset: every tap is multiplied by its weight twice (firwindow.c:129-130,
 * 153-158).  Two deviations from the reference: kaiser_beta is honoured (delay::sample_sinc ignores its argument and passes
 * the literal 9, delay.cpp:304: pass 9.0 for the reference's filters), and |subdelay| >= step_count is BFIR_ERR_ARG (the
 * reference silently skips the filter, delay.cpp:158-161).  BFIR_ERR_ARG also: a null `taps`, step_count < 2,
 * half_filter_length outside 1 .. 128, a realsize that is not 4 or 8. */
int bfir_subdelay_filter(int half_filter_length, int subdelay, int step_count, double kaiser_beta,
                         int realsize, void *taps);

/* delay_allocate_buffer + delay::subsample_init (delay.cpp:56-140, 182-265) for one side of an engine: side
 * BFIR_DELAY_INPUT delays the caller's frames before the engine proper reads them, BFIR_DELAY_OUTPUT what the engine
 * proper writes before the caller receives it.  An engine on which this was never called runs exactly the code it ran
 * before these calls existed.
 * With u_c[n] channel c of the side's frame stream, n counted from creation or the last bfir_engine_reset (u_c[n] = 0 for
 * n < 0), w the delayed stream, and d_c, s_c the values in force when the block that holds n is processed:
 *   step_count == 0 (no sub-sample stage; half_filter_length and kaiser_beta are ignored):
 *     w_c[n] = u_c[n - d_c], a copy of the raw sample bytes, so every sample format (1, 2, 3, 4 or 8 bytes) is served;
 *   step_count >= 2:
 *     w_c[n] = sum over k = 0 .. 2h of f_{s_c}[k] u_c[n - d_c - k], f from bfir_subdelay_filter(h, s_c, step_count,
 *     kaiser_beta, realsize): a delay of d_c + h + s_c/step_count samples.  Taps and accumulation in the engine's working
 *     precision, k ascending; samples are converted from the frame type on load and rounded once on store.  A channel
 *     with s_c = 0 is copied from u_c[n - d_c - h], not multiplied: its bytes, NaNs included, are a pure shift.
 * On the output side format conversion, overflow statistics and the NaN guard act on u, before the delay.
 * bfir_engine_set_delay applies from the next block processed and is a hard cut: the read position jumps, and the history
 * is that of u, so a longer delay repeats samples already played -- a deviation from the reference, which emits silence
 * while its buffer refills (delay.cpp:585-596).  The result does not depend on how the blocks arrive (one call or many,
 * host or device pointers, the latency path, any bfir_engine_set_chunk).  bfir_engine_reset zeroes the histories of both
 * sides and keeps the settings.  delay_init may be called again: it waits for queued work, discards that side's history
 * and sets that side's delays to 0.  Works on every kind of engine but a batch, fades included; a dithered integer output
 * takes whole-sample delays.
 * BFIR_ERR_ARG: a null engine; a side other than 0 / 1; max_delay < 0 or > 2^24; step_count negative or 1;
 * half_filter_length outside 1 .. 128 when step_count >= 2.  BFIR_ERR_UNSUPPORTED: a batch (n_engines > 1); step_count >= 2
 * on a side whose frames are not FLOAT_LE / FLOAT64_LE.  BFIR_ERR_HIP: the device is out of memory; the side is then off.
 * Memory per side: two histories of max_delay + 2h frames and one scratch buffer of one launch's frames -- the blocks per
 * launch of bfir_engine_set_chunk times filter_length frames, whatever the length of a call: with the automatic setting and
 * calls that long, 4096 blocks of the 8-channel, 4096-sample fp32 shape, 512 MiB per delayed side; a call of n blocks never
 * makes it larger than n blocks. */
int bfir_engine_delay_init(bfir_engine *e, int side, int max_delay, int step_count,
                           int half_filter_length, double kaiser_beta);

/* delay::update / change_delay (delay.cpp:27-54, 552-600) + subsample_update (:148-180) for all channels of a side:
 * delay[c] frames, 0 .. max_delay, and subdelay[c] steps, |subdelay[c]| < step_count (a null subdelay: all 0; non-zero on
 * a side without the stage: BFIR_ERR_ARG).  n_channels must be the side's channel count: the inputs / outputs of a matrix
 * engine, else the channels.  Waits for queued work.  BFIR_ERR_STATE on a side never initialised; a refused call changes
 * nothing.  get_delay returns what was set (both arrays required). */
int bfir_engine_set_delay(bfir_engine *e, int side, const int *delay, const int *subdelay, int n_channels);
int bfir_engine_get_delay(const bfir_engine *e, int side, int *delay, int *subdelay, int n_channels);

/* frames of fixed latency the side's sub-sample stage adds (h, or 0 without one); < 0: error */
int bfir_engine_delay_latency(const bfir_engine *e, int side);

/* tuning: blocks per launch; 0 (the default) = automatic: the work of 4096 blocks of the 8-channel, 4096-sample
 * headline shape (4096 ... 32768 blocks), less when the delay line of that many blocks would pass 4 GiB, at most 512
 * on the host-pointer path; takes effect on the next run */
int bfir_engine_set_chunk(bfir_engine *e, int blocks_per_launch);

/* per-kernel timing with HIP events on the stream the kernels run on */
enum { BFIR_K_STAGE_IN = 0, BFIR_K_FWD = 1, BFIR_K_MAC = 2, BFIR_K_INV = 3, BFIR_K_STAGE_OUT = 4,
       BFIR_K_COUNT = 5 };
int bfir_engine_set_profiling(bfir_engine *e, int enable);
int bfir_engine_get_profile(bfir_engine *e, int kernel, double *total_ms, int64_t *launches);

/* copy partition spectrum `block` of global channel `channel` to host (n_fft reals) */
int bfir_engine_read_coeff(bfir_engine *e, int channel, int block, void *dst);
/* partition spectrum `block` of h_{output,input} of a matrix engine, grouped layout, as bfir_engine_read_coeff */
int bfir_engine_read_coeff_matrix(bfir_engine *e, int output, int input, int block, void *dst);

/* ------------------------------------------------------------------ */
/* stage level: fftw_convolver methods on host buffers                 */
/* ------------------------------------------------------------------ */
typedef struct bfir_convolver bfir_convolver;

/* fftw_convolver::fftw_convolver (fftw_convolver.cpp:51-138) */
bfir_convolver *bfir_convolver_create(int length, int realsize, int device, int *err);
void bfir_convolver_destroy(bfir_convolver *c);
/* convolver_cbufsize (:468-472) */
int bfir_convolver_cbufsize(const bfir_convolver *c);
/* convolver_raw2cbuf (:156-185); float formats without byte swap */
int bfir_convolver_raw2cbuf(bfir_convolver *c, const void *rawbuf, void *cbuf, void *next_cbuf,
                            const bfir_buffer_format *bf);
/* convolver_time2freq (:187-212): FFTW_R2HC, half-complex output */
int bfir_convolver_time2freq(bfir_convolver *c, const void *input_cbuf, void *output_cbuf);
/* convolver_mixnscale (:214-229) */
int bfir_convolver_mixnscale(bfir_convolver *c, void *const *input_cbufs, void *output_cbuf,
                             const double *scales, int n_bufs, int mixmode);
/* convolver_convolve_inplace / convolve / convolve_add (:231-273) */
int bfir_convolver_convolve_inplace(bfir_convolver *c, void *cbuf, const void *coeffs);
int bfir_convolver_convolve(bfir_convolver *c, const void *input_cbuf, const void *coeffs,
                            void *output_cbuf);
int bfir_convolver_convolve_add(bfir_convolver *c, const void *input_cbuf, const void *coeffs,
                                void *output_cbuf);
/* convolver_freq2time (:350-375): FFTW_HC2R */
int bfir_convolver_freq2time(bfir_convolver *c, const void *input_cbuf, void *output_cbuf);
/* convolver_cbuf2raw (:405-466) with apply_dither false (or a float format): any sample format */
int bfir_convolver_cbuf2raw(bfir_convolver *c, const void *cbuf, void *outbuf,
                            const bfir_buffer_format *bf, bfir_overflow *overflow);

/* class dither (brutefir/dither.hpp:13-77, dither.cpp) and dither_state_t (global.h:63-69, same
 * layout).  The constructor fills dither_state[0 .. n_channels) as the reference's does. */
typedef struct bfir_dither bfir_dither;
typedef struct bfir_dither_state {
    int randtab_ptr;
    int8_t *randtab;
    float sf[2];
    double sd[2];
} bfir_dither_state;
bfir_dither *bfir_dither_create(int n_channels, int sample_rate, int realsize, int max_size,
                                int max_samples_per_loop, bfir_dither_state *dither_state, int device, int *err);
void bfir_dither_destroy(bfir_dither *d);
int bfir_dither_table_size(const bfir_dither *d);
const int8_t *bfir_dither_table(const bfir_dither *d);   /* host copy of dither_randtab */
/* dither::dither_preloop_real2int_hp_tpdf (dither.cpp:127-139) */
void bfir_dither_preloop_real2int_hp_tpdf(bfir_dither *d, bfir_dither_state *state, int samples_per_loop);
/* convolver_cbuf2raw with apply_dither true on an integer format (:421-431, :444-454): the preloop
 * for n_fft2 samples, then real2raw{f,d}_hp_tpdf with the caller's dither_state and overflow */
int bfir_convolver_cbuf2raw_dither(bfir_convolver *c, bfir_dither *d, const void *cbuf, void *outbuf,
                                   const bfir_buffer_format *bf, bfir_dither_state *dither_state,
                                   bfir_overflow *overflow);
/* convolver_coeffs2cbuf (:474-537).  Returns optional_dest, or (when it is
 * NULL) a 16-byte aligned host block the CALLER frees with bfir_aligned_free
 * (the reference caller frees it with _aligned_free, brutefir.cpp:844-854);
 * NULL on a NaN/Inf tap. */
void *bfir_convolver_coeffs2cbuf(bfir_convolver *c, const void *coeffs, int n_coeffs, double scale,
                                 void *optional_dest);
/* Methods of the class that nothing in the reference tree calls.
 * convolver_mixnscale above takes any n_bufs <= 32 (mixing matrix rows,
 * :908-1156, :1187-1419). */
/* convolver_runtime_coeffs2cbuf (:539-567): n_fft2 taps at src -> spectrum at dest */
int bfir_convolver_runtime_coeffs2cbuf(bfir_convolver *c, const void *src, void *dest);
/* convolver_dirac_convolve / _inplace (:323-348) */
int bfir_convolver_dirac_convolve(bfir_convolver *c, const void *input_cbuf, void *output_cbuf);
int bfir_convolver_dirac_convolve_inplace(bfir_convolver *c, void *cbuf);
/* convolver_convolve_eval (:377-403); buffer_cbuf is 1.5 cbufs, zeroed before the first call */
int bfir_convolver_convolve_eval(bfir_convolver *c, const void *input_cbuf, void *buffer_cbuf,
                                 void *output_cbuf);
/* convolver_crossfade_inplace (:275-321); buffer_cbuf is 1.5 cbufs */
int bfir_convolver_crossfade_inplace(bfir_convolver *c, void *input_cbuf, void *crossfade_cbuf,
                                     void *buffer_cbuf);
/* convolver_verify_cbuf (:569-602): 1 = all finite, 0 = NaN/Inf found, < 0 = error */
int bfir_convolver_verify_cbuf(bfir_convolver *c, void *const *cbufs, int n_cbufs);
/* convolver_debug_dump_cbuf (:604-651): every cbuf converted back to its coefficient list and written as one
 * "%.16e" line per tap (n_fft2 lines per cbuf).  BFIR_ERR_IO when the file cannot be opened (the reference
 * logs and returns). */
int bfir_convolver_debug_dump_cbuf(bfir_convolver *c, const char *filename, void *const *cbufs, int n_cbufs);
/* ------------------------------------------------------------------ */
/* FFT plans of any power-of-two size and the equalizer render          */
/*                                                     */
/* ------------------------------------------------------------------ */
typedef struct bfir_fft_plan bfir_fft_plan;

/* fftw_convolver::create_fft_plan(order, invert, inplace) (fftw_convolver.cpp:653-675):
 * FFTW_R2HC (invert 0) or FFTW_HC2R (invert 1) of 2^order reals, 1 <= order <= 25.
 * Sizes beyond one workgroup's LDS run as a four-step FFT, sizes below 32 reals as direct sums. */
bfir_fft_plan *bfir_fft_plan_create(int order, int invert, int inplace, int realsize, int device, int *err);
void bfir_fft_plan_destroy(bfir_fft_plan *p);
/* fftw[f]_execute_r2r(plan, in, out) on host buffers of 2^order reals; in == out allowed
 * (replaces the direct FFTW calls at equalizer.cpp:262, 357). */
int bfir_fft_plan_execute(bfir_fft_plan *p, const void *in, void *out);
int64_t bfir_fft_plan_length(const bfir_fft_plan *p);
/* equalizer::render_f / render_d (equalizer.cpp:211-299, 301-394): band tables as
 * equalizer::generate leaves them (:113-118) -> taps/2-sample impulse response in ir_out.
 * ifftplan: an HC2R plan of `taps` reals. */
int bfir_equalizer_render(bfir_fft_plan *ifftplan, int band_count, const double *freq, const double *mag,
                          const double *phase, void *ir_out);

/* ------------------------------------------------------------------ */
/* fftw_convolver::convolver_td_* (fftw_convolver.hpp:157-166): the     */
/* one-block convolver of the reference's delay class (delay.cpp:174)   */
/* ------------------------------------------------------------------ */
typedef struct bfir_td_conv bfir_td_conv;
/* convolver_td_block_length (fftw_convolver.cpp:697-706): n_coeffs rounded up to a power of two; -1 for
 * n_coeffs < 2 (the reference's log2_roof(1) is -1 and it shifts by it: undefined there, refused here) */
int bfir_td_block_length(int n_coeffs);
/* convolver_td_new (:708-757): the spectrum of [blocklen zeros | taps | zeros], times 1 / (2 blocklen),
 * resident on the device (td_conv_t; bfir_td_coeffs returns the host copy of td_conv_t.coeffs,
 * 2 * blocklen reals in FFTW's half-complex order).  The reference never frees a td_conv_t. */
bfir_td_conv *bfir_td_new(const void *coeffs, int n_coeffs, int realsize, int device, int *err);
void bfir_td_destroy(bfir_td_conv *tdc);
int bfir_td_blocklen(const bfir_td_conv *tdc);
const void *bfir_td_coeffs(const bfir_td_conv *tdc);
/* convolver_td_convolve (:759-777): R2HC, convolve_inplace_ordered (:819-856), HC2R in place on the
 * caller's 2 * blocklen reals */
int bfir_td_convolve(bfir_td_conv *tdc, void *overlap_block);

/* ------------------------------------------------------------------ */
/* sampling-rate conversion of an impulse response: the arithmetic     */
/* buffer::resample_snd_file (buffer.cpp:225-330) hands to             */
/* libsamplerate (src_simple, SRC_SINC_BEST_QUALITY)                   */
/* ------------------------------------------------------------------ */
/* libsamplerate's filter tables are not part of the reference tree, so this stage is defined from first principles:
 * band-limited interpolation on an exact rational grid.  Rates are integers; g = gcd(in_rate, out_rate), p = out_rate / g,
 * q = in_rate / g.  Output frame m sits at input time m q / p = n0 + phase / p with n0 = (m q) div p and phase = (m q) mod p
 * in 64-bit integers: exactly p phases, no table interpolation, no accumulated time error.
 *   rho = min(1, p / q) cutoff,  W = zero_crossings / rho,  Wc = ceil(W),  K = 2 Wc taps per phase
 *   tap j of a phase meets input frame n0 - Wc + 1 + j; with u = phase / p + Wc - 1 - j it is
 *   gain rho sinc(pi rho u) I0(kaiser_beta sqrt(1 - (u / W)^2)) / I0(kaiser_beta) for |u| < W, else 0
 *   y_c[m] = sum over j = 0 .. K - 1 of T[phase(m)][j] x_c[n0(m) - Wc + 1 + j], x_c = 0 outside [0, n_in)
 *   n_out = ceil(n_in p / q)
 * The window is applied once (firwindow_kaiser's twice-applied weight belongs to the delay filters only).  Taps are
 * evaluated on the host in long double and rounded once to realsize precision; the sum runs in that precision with j
 * ascending and one fused multiply-add per tap, samples rounded once on store (the convention of the sub-sample delay
 * stage).  Equal rates copy the bytes, NaNs included, whatever the other parameters.
 * zero_crossings 1 .. 128, kaiser_beta >= 0, cutoff in [0.5, 1], gain finite, rates >= 1, realsize 4 or 8: anything else is
 * BFIR_ERR_ARG.  K > 4096 or p K > 2^22 table entries: BFIR_ERR_UNSUPPORTED (44100 -> 96000 has p = 320; the standard audio
 * rates stay far below both). */

/* buffer.cpp:225-330 (the filter src_simple would apply): the K taps of phase 0 .. p - 1 in realsize precision (float or
 * double at `taps`), and K in *n_taps.  Pure host arithmetic, no device.  taps == NULL returns only K (then n_taps must
 * not be NULL).  A phase outside 0 .. p - 1: BFIR_ERR_ARG. */
int bfir_resample_filter(int in_rate, int out_rate, int zero_crossings, double kaiser_beta, double cutoff, double gain,
                         int realsize, int phase, void *taps, int *n_taps);

typedef struct bfir_resampler bfir_resampler;
/* buffer.cpp:225-330 (src_simple's converter state): the phase table, [K][p] in realsize precision, resident on `device`,
 * for interleaved frames of `channels` (1 .. BFIR_MAXCHANNELS) float (realsize 4) or double (realsize 8) samples.
 * Arguments are checked before the device: BFIR_ERR_NO_DEVICE only for valid ones, and never a CPU stand-in. */
bfir_resampler *bfir_resampler_create(int in_rate, int out_rate, int zero_crossings, double kaiser_beta, double cutoff, double gain,
                                      int realsize, int channels, int device, int *err);
/* buffer.cpp:292-298: the frames n_in input frames give, ceil(n_in p / q) -- all of them, where the reference caps the
 * output at the source's frame count.  Negative: BFIR_ERR_ARG. */
int64_t bfir_resampler_out_frames(const bfir_resampler *r, int64_t n_in);
/* buffer.cpp:295-302 (src_simple): n_in interleaved frames at `in` to min(max_out, n_out) frames at `out`, both host
 * buffers; returns the count written or a BFIR_ERR_* code.  Waits for the result. */
int64_t bfir_resampler_run(bfir_resampler *r, const void *in, int64_t n_in, void *out, int64_t max_out);
/* buffer.cpp:295-302: the same on device pointers (aligned to the sample; 16-byte alignment lets whole 16-byte stores
 * through).  Queued on the device's null stream, not waited for. */
int64_t bfir_resampler_run_device(bfir_resampler *r, const void *d_in, int64_t n_in, void *d_out, int64_t max_out);
/* buffer.cpp:316-318: waits for queued work and releases the table and the staging buffers */
void bfir_resampler_destroy(bfir_resampler *r);

/* Page-locked host memory for frame buffers handed to bfir_engine_run: the copy engines read and write it directly, so the
 * staging memcpy through the engine's own pinned buffers is skipped (the reference's callers allocate their frame buffers
 * with _aligned_realloc, foo_dsp_bfir.cpp:291-293; any hipHostMalloc / hipHostRegister'ed buffer is recognised the same way).
 * NULL without a GPU. */
void *bfir_pinned_malloc(size_t size);
void bfir_pinned_free(void *p);

void *bfir_aligned_malloc(size_t size, size_t alignment);
void bfir_aligned_free(void *p);

#ifdef __cplusplus
}
#endif
#endif
