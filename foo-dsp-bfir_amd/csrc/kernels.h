// kernels.h -- host-callable launchers of the gfx950 kernels (internal API,
// C++; the public C ABI is include/bfir_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <vector>

namespace bfir {

// Per-channel output statistics kept on the device; folded into
// bfoverflow_t (brutefir/global.h:96-102) by the host.
struct DevOverflow {
    unsigned int n_overflows;          // samples with |y| > max
    int intlargest;                    // integer outputs: largest unclipped |sample|
    unsigned long long largest_bits;   // bit pattern of max |y| (float widened, or double)
};
// The engine keeps BFIR_OF_SHARDS copies of its per-channel counters and every workgroup updates the copy
// blockIdx.x mod BFIR_OF_SHARDS (args.of_shard_stride elements apart; 0 = a single copy): when the output clips,
// every workgroup adds to n_overflows, and same-address atomics from a hundred thousand workgroups ran the
// plug-in's own shape at half speed.  bfir_engine_get_overflow sums / maximises over the copies.
constexpr int BFIR_OF_SHARDS = 64;
__device__ __forceinline__ DevOverflow *of_shard(DevOverflow *base, long shard_stride)
{
    return base + (long)(blockIdx.x & (BFIR_OF_SHARDS - 1)) * shard_stride;
}

// XCD-aware, bijective block -> work item remap of a launch of W workgroups: each XCD (blocks b, b+8, ...) gets
// one contiguous range of work items, so neighbouring items -- k_mac: ordered (channel, bin tile) major / time tile
// minor -- meet in one L2: it holds a slice of H for the whole launch while consecutive time tiles re-use each
// other's spectra; in the FFT kernels the channels of a block share the cache lines of their frames.
__device__ __forceinline__ int xcd_work_item(int b, int W)
{
    const int xcd = b & 7, qn = W >> 3, rn = W & 7;
    return (xcd < rn ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn) + (b >> 3);
}

// brutefir.cpp:316-321's verdict: block t of this launch has a non-finite sample 0.  The first such block of a run is kept
// by atomicMin in HBM; the latency path (a handful of blocks per call, run_small) also gets one flag per block in pinned
// host memory -- plain, idempotent stores, visible with the stream's end -- so that no copy has to follow the kernels.
template <typename A> __device__ __forceinline__ void flag_bad(const A &a, int t)
{
    atomicMin(a.bad_block, a.block_base + t);
    if (a.bad_host) a.bad_host[t] = 1;
}

// Sample formats (brutefir/global.h:24-34; table of brutefir.cpp:435-538, little-endian host).
struct FmtInfo { int bytes; bool isfloat; bool big_endian; };
inline FmtInfo fmt_info(int fmt)
{
    static const int b[12] = {0, 1, 2, 2, 3, 3, 4, 4, 4, 4, 8, 8};
    FmtInfo f;
    f.bytes = (fmt >= 1 && fmt <= 11) ? b[fmt] : 0;
    f.isfloat = fmt >= 8 && fmt <= 11;
    f.big_endian = fmt == 3 || fmt == 5 || fmt == 7 || fmt == 9 || fmt == 11;
    return f;
}
// get_full_scale (brutefir.cpp:395-398) in the reference's int arithmetic: negative for 32 bits.
inline double fmt_full_scale(int fmt) { return (double)(int32_t)(1u << (8 * fmt_info(fmt).bytes - 1)); }
inline bool fmt_is_native(int fmt) { return fmt == 8 || fmt == 10; }   // FLOAT_LE, FLOAT64_LE: fast staging kernels

// Twiddle tables of one transform size / precision, resident in HBM.
struct FftPlan {
    int log2m = 0;        // M = L complex points; N = 2M reals
    int realsize = 0;     // 4 or 8
    void *tw = nullptr;   // per-pass twiddles  exp(-2 pi i r k / (p R))
    void *ws = nullptr;   // split twiddles     exp(-2 pi i k / N), k < M
    void *twb = nullptr;  // twiddle bases of the persistent kernels (fft_lds.h)
};

int  fft_plan_create(FftPlan *plan, int filter_length, int realsize);   // 0 or negative error
void fft_plan_destroy(FftPlan *plan);
int  fft_threads(int log2m);

// a5: interleaved raw frames -> planar working-precision time buffers.
// Engine e reads frames frame_off .. frame_off+n_frames-1 of the interleaved
// buffer at raw + e*eng_stride_bytes.  dst[gc][dst_off + f], gc = e*C + c.
struct StageInArgs {
    const void *raw; long eng_stride_bytes; long frame_off;
    int n_eng, C, raw_bytes;       // raw_bytes: bytes per raw sample
    int spacing;                   // samples between frames (buffer_format_t.sample_spacing)
    long n_frames;
    void *dst; long dst_ch_stride; long dst_off;   // in reals
    int realsize;
    int fmt = 0;                   // BF_SAMPLE_FORMAT_* code; 0 = FLOAT_LE / FLOAT64_LE by raw_bytes
};
void launch_stage_in(const StageInArgs &a, hipStream_t s);

// a13: planar time -> interleaved raw frames + overflow statistics + NaN guard.
struct StageOutArgs {
    void *raw; long eng_stride_bytes; long frame_off;
    int n_eng, C, raw_bytes;
    int spacing;
    long n_frames;
    const void *src; long src_ch_stride;           // in reals
    int realsize;
    int L;                         // block length: sample 0 of every block is NaN-checked
    double max;                    // bfoverflow_t.max
    DevOverflow *overflow;         // [n_eng*C]
    long of_shard_stride = 0;
    int *bad_block;                // atomicMin of the first block with a non-finite sample 0
    int *bad_host = nullptr;       // latency path: one flag per block of the launch in pinned host memory (flag_bad)
    int block_base;                // index of the chunk's first block within the run
    int fmt = 0;                   // BF_SAMPLE_FORMAT_* code; 0 = FLOAT_LE / FLOAT64_LE by raw_bytes
    // HP-TPDF dither (integer formats only, dither.hip): the shared random table and one state per global channel
    const void *dither_tab = nullptr; int dither_size = 0; void *dither_state = nullptr;
};
void launch_stage_out(const StageOutArgs &a, hipStream_t s);

// dither_state_t (brutefir/global.h:63-69) as the engine keeps it in HBM, one per global channel
struct DevDitherState { int randtab_ptr; int pad; float sf[2]; double sd[2]; };
// class dither's table (brutefir/dither.cpp:21-110): spacing between channels in samples (-1: budget too small)
int dither_spacing(int n_channels, int sample_rate, int max_size, int max_samples_per_loop);
void dither_fill_table(std::vector<int8_t> &tab, int n_channels, int spacing);
void launch_stage_out_dither(const StageOutArgs &a, hipStream_t s);

// a6 + a7 (and a16 with zero_first_half): real FFT of the N-sample window
// [block t-1 | block t] of channel gc, written in the grouped layout to
// dst + gc*dst_ch_stride + ((base_slot + t) % ring) * N.  Block t (t >= 0) is
// at src + gc*src_ch_stride + t*L; the block before block 0 is at
// prev + gc*prev_ch_stride.
struct FwdArgs {
    const void *src; long src_ch_stride;
    const void *prev; long prev_ch_stride;
    void *dst; long dst_ch_stride;
    int ring, base_slot;
    int n_t, n_ch;
    double load_scale, out_scale;
    int zero_first_half;
    int interleaved = 0;           // spectrum layout: 0 = the reference's groups (4 re | 4 im), 1 = (re, im) pairs
    // Direct mode (raw_bytes = 4 / 8, FLOAT_LE / FLOAT64_LE frames): the samples come straight from the
    // interleaved raw frames instead of a planar buffer -- no staging kernel, no planar time buffers.
    // Channel gc = g C + c reads frame f of engine g at raw + g raw_eng_stride + (frame_off + f) C + c (in
    // samples); the block before block 0 is the raw-frame block prev_raw [n_eng][L][C]; the raw frames of the
    // chunk's last two blocks are kept in save_last / save_prev as the pair path keeps them (pair.hip).
    int raw_bytes = 0;
    const void *raw = nullptr; long raw_eng_stride = 0, frame_off = 0; int C = 0;
    const void *prev_raw = nullptr, *carry = nullptr; void *save_last = nullptr, *save_prev = nullptr;
    long hist_eng_stride = 0;
};
void launch_fwd(const FftPlan &plan, const FwdArgs &a, hipStream_t s);

// a8/a9/a10: Y[gc][t] = sum_{i < nblk[gc]} X[gc][slot(t - i)] * H[gc][i].
struct MacArgs {
    const void *x; long x_ch_stride; int ring, base_slot;
    const void *h; long h_ch_stride;               // [gc][B][N]
    const int *nblk;                               // device [n_ch]
    void *y; long y_ch_stride;                     // [gc][n_t][N]
    int n_t, n_ch, N, realsize;
    int B = 0;                                     // partitions allocated per channel (max of nblk)
    int interleaved = 0;                           // layout of x, h and y, as in FwdArgs (fp32 streaming kernel only)
};
// Cache policy of the two big streams, the delay line X and the product spectra Y (each written once and read
// once, a gigabyte apart): the persistent pair kernels and the streaming MAC load and store both nontemporal.
// That is +4 % on the headline pipeline against cached stores and loads (112.1 vs 107.5 Gsamples/s, same box;
// any three of the four nontemporal +1.5..3 %, profiles/r02_nt_policy.txt) -- the lines of the interleaved
// input / output frames, of which every workgroup uses a quarter, then survive in L2 until the other three
// channel pairs have come by.  No effect on small launches.
void launch_mac(const MacArgs &a, hipStream_t s);
// mac_sys.hip: the forward-walking two-lanes-per-bin form of the fp32 pair-layout MAC (B <= 32)
constexpr int BFIR_MAC_SYS_MAX_B = 256;   // partitions the systolic MAC takes (sixteen stages of sixteen)
bool mac_sys_supported(const MacArgs &a);
void launch_mac_sys(const MacArgs &a, hipStream_t s);

// matrix.hip: the partition sums of a matrix engine (n_in inputs -> n_out outputs, one filter per pair),
//   Y[o][t] = sum_{i < n_in} sum_{p < nblk[o][i]} X[i][slot(t - p)] * H[o][i][p],
// inputs in order, partitions in order within an input: the fma chain of every other MAC here.  nblk = 0: no path (skipped).
constexpr int BFIR_MAT_MAX = 8;            // inputs / outputs of a matrix engine (BFIR_MAXCHANNELS)
constexpr int BFIR_MAT_SMALL_MAX = 4;      // output blocks per launch up to which the one-block-per-lane form runs
struct MatArgs {
    const void *x; long x_ch_stride; int ring, base_slot;     // delay line [n_in][ring][N]
    const void *h; long h_pair_stride;                       // [n_out][n_in][B][N]: pair (o, i) at (o n_in + i) h_pair_stride
    int nblk[BFIR_MAT_MAX * BFIR_MAT_MAX];                   // [o n_in + i]: partitions of h_{o,i}, by value (kernel argument)
    void *y; long y_ch_stride;                               // [n_out][n_t][N]
    int n_t, n_in, n_out, N, realsize;
    int interleaved;                                         // layout of x, h and y, as in FwdArgs
};
bool mac_matrix_supported(const MatArgs &a);               // the grid of the launch fits
int launch_mac_matrix(const MatArgs &a, hipStream_t s);    // 0, or -1 if !mac_matrix_supported(a) (nothing launched)

// mimo.hip: k_mac_mimo, the same sums for a mimo engine (bfir_engine_create_mimo: up to BFIR_MIMO_MAX inputs and outputs),
// one fma chain per (output, bin, block) as above: the bits of launch_mac_matrix wherever both can run.  MimoArgs is MatArgs
// with the partition counts in HBM, [o n_in + i] (the engine rewrites the table when the filters are set), and the kernel
// differs from k_mac_matrix in its grid alone: workgroups of one wave over 64 bins, every (bin tile, output tile, time
// tile) in grid x with the time tiles fastest, so that what an XCD runs at one time shares one slice of H in its L2.
constexpr int BFIR_MIMO_MAX = 64;          // inputs / outputs of a mimo engine (BFIR_MIMO_MAXCHANNELS)
struct MimoArgs {
    const void *x; long x_ch_stride; int ring, base_slot;     // delay line [n_in][ring][N]
    const void *h; long h_pair_stride;                       // [n_out][n_in][B][N]: pair (o, i) at (o n_in + i) h_pair_stride
    const int *nblk;                                         // device [n_out n_in]: partitions of h_{o,i}; wave-uniform reads
    void *y; long y_ch_stride;                               // [n_out][n_t][N]
    int n_t, n_in, n_out, N, realsize;
    int interleaved;                                         // layout of x, h and y, as in FwdArgs
};
bool mac_mimo_supported(const MimoArgs &a);                // the grid of the launch fits
int launch_mac_mimo(const MimoArgs &a, hipStream_t s);     // 0, or -1 if !mac_mimo_supported(a) (nothing launched)

// mfade.hip: k_mac_duo, the matrix MAC of a chunk that needs BOTH filter sets of a crossfaded coefficient change on a
// multi-level matrix engine (bfir_engine_set_coeff_matrix_levels_fade): one pass over the delay line computes
//   Y [o][t] = sum_i sum_{p < a.nblk[o][i]} X[i][slot(t - p)] * H [o][i][p]     (a: the old set, exactly launch_mac_matrix(a))
//   Y2[o][t] = sum_i sum_{p < nblk2[o][i]}  X[i][slot(t - p)] * H2[o][i][p]     (the new set: h2, nblk2, y2, y2_ch_stride)
// with k_mac_matrix's fma chain per (set, output, bin, block): the bits of two launch_mac_matrix calls.
struct MatDuoArgs {
    MatArgs a;                                               // the old set and everything both sets share
    const void *h2;                                          // [n_out][n_in][B][N], pairs a.h_pair_stride apart as in a.h
    int nblk2[BFIR_MAT_MAX * BFIR_MAT_MAX];                  // [o n_in + i], by value
    void *y2; long y2_ch_stride;                             // [n_out][..][N]
};
bool mac_duo_supported(const MatDuoArgs &d);               // the grid of the launch fits
int launch_mac_duo(const MatDuoArgs &d, hipStream_t s);    // 0, or -1 if !mac_duo_supported(d) (nothing launched)

// wduo.hip: k_wduo, the same one pass over the delay line for a level of a multi-level mimo engine
// (bfir_engine_create_mimo_levels) -- to k_mac_duo what k_mac_mimo is to k_mac_matrix: the sums of k_mac_duo lane for lane
// (duo_lane, mat_ops.h), both count tables in HBM, k_mac_mimo's grid.  Y and Y2 are bit for bit what launch_mac_mimo(a) and
// launch_mac_mimo of the new set (h2, nblk2, y2, y2_ch_stride) write.
struct WduoArgs {
    MimoArgs a;                                              // the old set and everything both sets share
    const void *h2;                                          // [n_out][n_in][B][N], pairs a.h_pair_stride apart as in a.h
    const int *nblk2;                                        // device [n_out n_in], as a.nblk
    void *y2; long y2_ch_stride;                             // [n_out][..][N]
};
bool wduo_supported(const WduoArgs &d);                    // the grid of the launch fits
int launch_wduo(const WduoArgs &d, hipStream_t s);         // 0, or -1 if !wduo_supported(d) (nothing launched)

// patch.hip: k_patch_pairs, the new set's products of a fade that replaces a list of pairs of a matrix or mimo engine
// (bfir_engine_set_coeff_matrix_pairs_fade), from the old set's products y, which launch_mac_matrix / launch_mac_mimo has
// just written:  Y2[o][t] = Y[o][t] + sum over the listed pairs (o, i) of row o, in input order, of
//   sum_{p < nb_new} X[i][slot(t - p)] * H2[o][i][p]  -  sum_{p < nb_old} X[i][slot(t - p)] * H[o][i][p]
// continuing ONE fma chain per (output, bin, block): the new filter's terms first, then the old filter's with H negated.  A
// row without listed pairs is copied; a pair without partitions in a set causes no loads for that set.
struct PatchArgs {
    const void *x; long x_ch_stride; int ring, base_slot;     // delay line [n_in][ring][N]
    const void *h, *h2; long h_pair_stride;                   // old and new set, [n_out][n_in][B][N] each
    const int *row;                                           // device [n_out + 1]: the entries of row o are row[o] .. row[o + 1] - 1
    const int *ent;                                           // device [entries][3]: input, nb_new, nb_old; wave-uniform reads
    const void *y; long y_ch_stride;                          // [n_out][..][N], read
    void *y2; long y2_ch_stride;                              // [n_out][..][N], written
    int n_t, n_in, n_out, N, realsize;
    int interleaved;                                          // layout of x, h, h2, y and y2, as in FwdArgs
};
bool patch_supported(const PatchArgs &a);                   // the grid of the launch fits
int launch_patch(const PatchArgs &a, hipStream_t s);        // 0, or -1 if !patch_supported(a) (nothing launched)

// wpatch.hip: k_wpatch, the old set's products of a level whose MAC is k_mac_mimo AND the patch behind them in one launch:
// a.y and y2 are bit for bit what launch_mac_mimo(a) followed by launch_patch(wpatch_patch_args(d)) write.
struct WpatchArgs {
    MimoArgs a;                                               // the old set's MAC
    const void *h2;                                           // the new set, as a.h
    const int *row, *ent;                                     // the table of the listed pairs, as PatchArgs has it
    void *y2; long y2_ch_stride;                              // [n_out][..][N], written
};
// the patch of that launch as k_patch_pairs takes it: everything else is a's
inline __host__ __device__ PatchArgs wpatch_patch_args(const WpatchArgs &d)
{
    PatchArgs p;
    p.x = d.a.x; p.x_ch_stride = d.a.x_ch_stride; p.ring = d.a.ring; p.base_slot = d.a.base_slot;
    p.h = d.a.h; p.h2 = d.h2; p.h_pair_stride = d.a.h_pair_stride;
    p.row = d.row; p.ent = d.ent;
    p.y = d.a.y; p.y_ch_stride = d.a.y_ch_stride;
    p.y2 = d.y2; p.y2_ch_stride = d.y2_ch_stride;
    p.n_t = d.a.n_t; p.n_in = d.a.n_in; p.n_out = d.a.n_out; p.N = d.a.N; p.realsize = d.a.realsize;
    p.interleaved = d.a.interleaved;
    return p;
}
bool wpatch_supported(const WpatchArgs &d);                 // the grid of the launch fits
int launch_wpatch(const WpatchArgs &d, hipStream_t s);      // 0, or -1 if !wpatch_supported(d) (nothing launched)

// bank.hip: k_bank_gather, the listed rows of a filter store (H, or a fade's H2) from a coefficient bank, a store of the
// same row form ([entries][B][N], bfir_engine_bank_create), in one launch.  Row tab[3 j] of dst gets the first tab[3 j + 2]
// partitions of bank entry tab[3 j + 1] and zeros behind them; an entry of -1 gives a row of zeros.  A row is bytes: both
// precisions and both layouts are one kernel.
struct BankArgs {
    const void *bank; void *dst;                              // 16-byte aligned
    const int *tab;                                           // device [n_rows][3]: destination row, entry or -1, partitions (<= B)
    int n_rows;
    unsigned long long row_bytes, part_bytes;                 // B N realsize and N realsize, multiples of 16
};
constexpr int BFIR_BANK_SPAN = 4096;                        // the bytes one workgroup moves per step: 256 lanes of 16
constexpr int BFIR_BANK_STEPS = 4;                          // steps per workgroup
bool bank_gather_supported(const BankArgs &a);              // alignment, and the grid of the launch fits
int launch_bank_gather(const BankArgs &a, hipStream_t s);   // 0, or -1 if !bank_gather_supported(a) (nothing launched)

// bankmix.hip: k_bank_mix<R>, the gather that multiplies and adds while it copies (bfir_engine_set_coeff_matrix_bank_mix,
// _bank_mix_fade, _pairs_bank_mix, _pairs_bank_mix_fade).  Row rec[0] of dst gets, in its first rec[1] partitions, the sum of
// rec[2] <= BFIR_BANK_MIX_TERMS bank entries, each times a weight in R, every product and every add rounded on its own and
// the first product starting the sum; a term takes part in the partitions below its own count alone; zeros behind rec[1].
// The host lists live terms only (entry >= 0, weight != 0, count >= 1), in the caller's order; rec[1] is their largest count.
#ifndef BFIR_BANK_MIX_TERMS
#define BFIR_BANK_MIX_TERMS 4                               // the terms of a mix; the public header's constant of this name
#endif
static_assert(BFIR_BANK_MIX_TERMS == 4, "k_bank_mix's records and its register budget are laid out for four terms");
constexpr int BFIR_BANK_MIX_REC = 3 + 4 * BFIR_BANK_MIX_TERMS;   // words of a record: row, count, live terms, then per term
                                                            // entry, count, the weight's bits in R (low word, high word; float: high 0)
struct BankMixArgs {
    const void *bank; void *dst;                              // 16-byte aligned
    const int *tab;                                           // device [n_rows][BFIR_BANK_MIX_REC]
    int n_rows;
    unsigned long long row_bytes, part_bytes;                 // B N realsize and N realsize, multiples of 16
};
constexpr int BFIR_BANK_MIX_STEPS = 2;                      // steps of BFIR_BANK_SPAN bytes per workgroup
bool bank_mix_supported(const BankMixArgs &a);              // alignment, and the grid of the launch fits
int launch_bank_mix(const BankMixArgs &a, int realsize, hipStream_t s);   // 0, or -1 if unsupported (nothing launched)

// lbank.hip: k_lbank_gather, the same for ALL levels of a multi-level matrix or mimo engine in one launch
// (bfir_engine_levels_bank_create: one store per level).  Row tab[W j] of every participating level's dst gets the first
// tab[W j + 2 + k] partitions of that level's bank entry tab[W j + 1] and zeros behind them, W = 2 + BFIR_LBANK_LEVELS.
constexpr int BFIR_LBANK_LEVELS = 4;                        // BFIR_MAX_LEVELS of the public header (engine.hip asserts it)
struct LBankLevel {
    const void *bank; void *dst;                              // 16-byte aligned; dst null: the level is not part of the launch
    unsigned long long row_bytes, part_bytes;                 // blocks[k] N_k realsize and N_k realsize, multiples of 16
};
struct LBankArgs {
    LBankLevel lv[BFIR_LBANK_LEVELS];
    unsigned end[BFIR_LBANK_LEVELS];                          // workgroups of a row up to and with level k (launch_lbank_gather sets them)
    const int *tab;                                           // device [n_rows][2 + BFIR_LBANK_LEVELS]: row, entry or -1, partitions per level
    int n_rows;
};
bool lbank_gather_supported(const LBankArgs &a);            // alignment, and the grid of the launch fits
int launch_lbank_gather(LBankArgs a, hipStream_t s);        // 0, or -1 if !lbank_gather_supported(a) (nothing launched)

// lbankmix.hip: k_lbank_mix<R>, k_lbank_gather's grid with k_bank_mix's body (bfir_engine_set_coeff_matrix_levels_bank_mix,
// _bank_mix_fade, _pairs_bank_mix, _pairs_bank_mix_fade).  On every participating level k, row rec[0] of dst_k gets the sum of
// the record's rec[1] <= BFIR_BANK_MIX_TERMS terms, each that level's bank entry times a weight in R, every product and every
// add rounded on its own and the first product starting the sum; term t takes part in the partitions below its own count on
// the level, rec[2 + 7 t + 3 + k], alone; where no term covers an offset the row gets zeros.  The host lists live terms only
// (entry >= 0, weight != 0), in the caller's order.
constexpr int BFIR_LBANK_MIX_TERM = 3 + BFIR_LBANK_LEVELS;  // words of a term: entry, the weight's bits in R (low, high), the count per level
constexpr int BFIR_LBANK_MIX_REC = 32;                      // words of a record: row, live terms, the terms; the rest unused
static_assert(2 + BFIR_BANK_MIX_TERMS * BFIR_LBANK_MIX_TERM <= BFIR_LBANK_MIX_REC, "a record holds its terms");
struct LBankMixArgs {
    LBankLevel lv[BFIR_LBANK_LEVELS];
    unsigned end[BFIR_LBANK_LEVELS];                          // workgroups of a row up to and with level k (launch_lbank_mix sets them)
    const int *tab;                                           // device [n_rows][BFIR_LBANK_MIX_REC]
    int n_rows;
};
bool lbank_mix_supported(const LBankMixArgs &a);            // alignment, and the grid of the launch fits
int launch_lbank_mix(LBankMixArgs a, int realsize, hipStream_t s);   // 0, or -1 if unsupported (nothing launched)

// a11 + a12: inverse real FFT of Y[gc][t] (grouped layout, times in_scale),
// first L samples to dst + gc*dst_ch_stride + t*L.
struct InvArgs {
    const void *src; long src_ch_stride;           // [gc][n_t][N]
    void *dst; long dst_ch_stride;
    int n_t, n_ch;
    double in_scale;
    int full_output;                               // 1: write all N samples at stride N (stage API)
    int interleaved = 0;                           // layout of src, as in FwdArgs
    // Direct mode (raw_bytes = 4 / 8): the valid half goes straight into the interleaved raw output frames
    // (same addressing as FwdArgs) with the overflow statistics and the NaN guard of real2raw
    // (brutefir/real2raw.cpp:321-336, brutefir.cpp:316-321): no planar output buffer, no staging kernel.
    int raw_bytes = 0;
    void *raw = nullptr; long raw_eng_stride = 0, frame_off = 0; int C = 0;
    double max = 1.0; DevOverflow *overflow = nullptr; int *bad_block = nullptr; int block_base = 0;
    int *bad_host = nullptr;                       // as in StageOutArgs
    long of_shard_stride = 0;
};
void launch_inv(const FftPlan &plan, const InvArgs &a, hipStream_t s);

// Long partitions (bigconv.hip): the real FFT of N = 2L reals, L = M1 M2 = 2^15 .. 2^20 (fp64: from 2^14), in two passes
// per direction over the workgroup FFTs of M1 and M2 points.  Spectra are in TRANSPOSED bin order -- bin k1 + M1 k2 at
// position k1 M2 + k2, bin 0 (DC | Nyquist) at position 0 -- in either layout of FwdArgs.interleaved.
struct BigPlan {
    int log2m = 0, log2m1 = 0, log2m2 = 0;   // M = M1 M2 complex points: columns of M1, rows of M2
    int realsize = 0;
    FftPlan p1, p2;                          // the column and the row transform
    void *t_hi = nullptr, *t_lo = nullptr;   // exp(-2 pi i j / M) = t_hi[j >> 10] t_lo[j & 1023]
    void *s_hi = nullptr, *s_lo = nullptr;   // exp(-2 pi i k / N) likewise: the split twiddles
};
bool big_split(int filter_length, int realsize, int *log2m1, int *log2m2);   // false: not a length the big kernels take
int  big_plan_create(BigPlan *plan, int filter_length, int realsize);         // 0, -1 (unsupported) or -2 (HIP)
void big_plan_destroy(BigPlan *plan);
bool big_launch_fits(const BigPlan &plan, int n_t, int n_ch);                 // the grids of such a launch fit
// The planar forms only (raw_bytes == 0, full_output == 0).  launch_fwd_big works in place on the delay-line slots;
// launch_inv_big CONSUMES a.src (its row pass leaves the half-transformed data there for the column pass).
void launch_fwd_big(const BigPlan &plan, const FwdArgs &a, hipStream_t s);
void launch_inv_big(const BigPlan &plan, const InvArgs &a, hipStream_t s);

// Pair path (pair.hip): two adjacent channels per complex transform, straight from / to interleaved
// FLOAT_LE frames; fp32, even channel count, 512 <= L <= 8192.  `plan` is the plan of 2L points.
bool pair_supported(int filter_length);
// k_fwd / k_inv can take both channels of a stereo float-frame block in one workgroup (direct mode, whole frames)
bool direct_stereo_supported(int filter_length, int realsize);
// fp64 engines of 1024 ... 8192 points in direct mode: k_fwd_run / k_inv_run, runs of blocks per workgroup with the next block's
// frames / spectrum fetched under the current transform (BFIR_RUN64=0: off; =n: blocks per run)
bool run64_supported(int filter_length, int realsize);
// ... and such engines may keep their spectra as (re, im) pairs (engine.hip; 1024 ... 4096 points)
bool pairs64_supported(int filter_length, int realsize);
struct FwdPairArgs {
    const float *raw; long eng_stride; long frame_off;   // input frames; engine stride in floats
    int C, n_eng, n_t;
    const float *prev;                                   // the block before block 0: [n_eng][L][C] raw frames
    float *save_last, *save_prev;                        // where blocks n_t-1 / n_t-2 are kept for the next chunk
    const float *carry;                                  // n_t == 1: the history block that becomes save_prev
    long hist_eng_stride;                                // floats between engines in prev / save_* / carry
    float *dst; long dst_ch_stride; int ring, base_slot; // delay line, (re, im) pairs
    float scale;
    int tp = 0;                                          // pairs in TIME: blocks t, t+1 of one channel per transform (any C)
    int wide = -1;                                       // k_fwd_wide_ps where it applies: 0 never, 1 always, -1 for launches that fill the GPU
};
void launch_fwd_pair(const FftPlan &plan, const FwdPairArgs &a, hipStream_t s);
// wide.hip: channel pairs, C % 4 == 0, frames and history blocks 16-byte aligned -- two pairs in turn per workgroup and
// 16-byte frame loads, the same bits as the pair kernel.  false: not taken (launch_fwd_pair goes on with the pair kernel).
bool launch_fwd_wide(const FftPlan &plan, const FwdPairArgs &a, hipStream_t s);
struct InvPairArgs {
    const float *y; long y_ch_stride;                    // [gc][n_t][N] product spectra, (re, im) pairs
    float *raw; long eng_stride; long frame_off;         // output frames
    int C, n_eng, n_t;
    float scale, max;
    DevOverflow *overflow; int *bad_block; int block_base;
    int *bad_host = nullptr;                             // as in StageOutArgs
    long of_shard_stride = 0;
    int tp = 0;                                          // pairs in time, as in FwdPairArgs
    int frame_stride = 0;                                // channel pairs only: floats between output frames; 0 = C (wider: an odd matrix output beside the pairs)
    int quad = -1;                                       // k_inv_quad_ps where it applies: 0 never, 1 always, -1 for launches that fill the GPU
};
void launch_inv_pair(const FftPlan &plan, const InvPairArgs &a, hipStream_t s);
// quad.hip: channel pairs, C % 4 == 0, frames C floats apart and 16-byte aligned -- two pairs in turn per workgroup and
// 16-byte frame stores, the same bits as the pair kernel.  false: not taken (launch_inv_pair goes on with the pair kernel).
bool launch_inv_quad(const FftPlan &plan, const InvPairArgs &a, hipStream_t s);

// What every one-transform fused back end below (inv_back.h) needs for its overflow statistics and NaN guard.
struct InvStats {
    float max;                                           // bfoverflow_t.max
    DevOverflow *overflow; long of_shard_stride;
    int *bad_block; int block_base; int *bad_host;       // as in StageOutArgs
};
// The launch of a planar middle step k<real, VEC>(args) -- blocks of 256 lanes over args.n samples of args.n_ch channels --
// given its four instances (BFIR_PLANAR_KERNELS) and the verdict on alignment: lane-consecutive, 16 bytes per lane where
// every channel's samples are 16-byte aligned, else one sample per lane.
#define BFIR_PLANAR_KERNELS(k) k<float, 4>, k<float, 1>, k<double, 2>, k<double, 1>
template <typename A>
inline void launch_planar(void (*f4)(A), void (*f1)(A), void (*d2)(A), void (*d1)(A), const A &a, bool aligned, hipStream_t s)
{
    const long lanes = aligned ? a.n / (16 / a.realsize) : a.n;
    const dim3 grid((unsigned)((lanes + 255) / 256), (unsigned)a.n_ch), block(256);
    hipLaunchKernelGGL(a.realsize == 4 ? (aligned ? f4 : f1) : (aligned ? d2 : d1), grid, block, 0, s, a);
}

// fade.hip: the back end of a crossfaded coefficient change (bfir_engine_set_coeff_fade; the reference's blend is
// fftw_convolver::convolver_crossfade_inplace, brutefir/fftw_convolver.cpp:275-321).  The MAC has run twice over the same
// delay line: y_old holds the products with the old filters, y_new those with the new ones.  Sample n of block t blends as
//   out = y_old * (1.0 - f * (real)m) + y_new * f * (real)m,   m = m0 + t L + n,   f = 1 / (real)(K L - 1)
// with C's promotions (fp32: the first product and the sum are double, :301-303).
// k_inv_fade, the fused form: fp32, (re, im) pairs, FLOAT_LE frames, 512 <= L <= 8192 (pair_supported).  One workgroup per
// (output channel, block): Z = Y_old + i Y_new, ONE inverse of 2L points (`plan` is the plan of 2L points), blend, overflow
// statistics, NaN guard, frame store.
struct FadeInvArgs {
    const float *y_old; long y_old_ch_stride;            // [n_ch][..][N] product spectra, (re, im) pairs
    const float *y_new; long y_new_ch_stride;
    float *raw; long frame_off;                          // output frames of ONE engine, n_ch channels wide
    int n_ch, n_t;
    float scale;
    float f; int m0;                                     // the ramp: 1 / (K L - 1), and m of sample 0 of block 0
    InvStats st;
};
void launch_inv_fade(const FftPlan &plan, const FadeInvArgs &a, hipStream_t s);
// k_fade_blend, the general form's middle step: y_old[c][i] <- blend(y_old[c][i], y_new[c][i]) on planar time buffers
// [n_ch][..] (i < n: the chunk's n_t L samples of a channel), m = m0 + i; launch_inv fills them, launch_stage_out follows.
struct FadeBlendArgs {
    void *y_old; const void *y_new; long ch_stride;      // in reals
    int n_ch; long n;
    double f; int m0;                                    // fp32: f is the float the reference computes (:298), widened
    int realsize;
};
void launch_fade_blend(const FadeBlendArgs &a, hipStream_t s);

// nup.hip, levels.hip: the back ends of a two-level engine (bfir_engine_create_nup) and of a multi-level engine
// (bfir_engine_create_levels).  The head level's products are in y; every contributing tail level has left its time output
// in a planar ring [n_ch][zlen] of working precision of its own, sample m at m mod zlen.  Sample n of block t of the chunk is
//   ((y_head[n] + z_0[m_0]) + z_1[m_1]) + z_2[m_2],   m_r = ring[r].m0 + t L + n
// the additions head first, rings in level order, nothing added from a ring where m_r < ring[r].m_min.  Each m0, m_min and
// zlen is a multiple of L, so a block's L samples of a ring are contiguous: the rings wrap between blocks only.
constexpr int BFIR_LEVEL_RINGS = 3;
struct LevelRing {
    const void *z; long z_ch_stride; long zlen;          // planar [n_ch][zlen] reals of working precision
    long long m0, m_min; long m0r;                       // m0r = m0 mod zlen
};
// k_inv_nup (one ring, nup.hip) and k_inv_levels (two or three, levels.hip), the fused form: fp32, (re, im) pairs, FLOAT_LE
// frames, even n_ch, 512 <= L <= 8192 (pair_supported).  One workgroup per (channel pair, block): Z = Y_a + i Y_b, ONE
// inverse of 2L points (`plan` is the plan of 2L points), the sums, overflow statistics, NaN guard, frame store.
struct LevelsInvArgs {
    const float *y; long y_ch_stride;                    // [n_ch][..][N] product spectra, (re, im) pairs
    LevelRing ring[BFIR_LEVEL_RINGS]; int n_rings;       // 1 .. 3
    float *raw; long frame_off;                          // output frames of ONE engine, n_ch channels wide
    int n_ch, n_t;
    float scale;
    InvStats st;
    int frame_stride = 0;                                // floats between output frames; 0 = n_ch (wider: an odd matrix output beside the pairs)
};
void launch_inv_nup(const FftPlan &plan, const LevelsInvArgs &a, hipStream_t s);      // n_rings == 1
void launch_inv_levels(const FftPlan &plan, const LevelsInvArgs &a, hipStream_t s);   // any n_rings: one goes to launch_inv_nup
// k_nup_combine (one ring) and k_levels_combine, the general form's middle step: y[c][i] <- y[c][i] + z_0 (+ z_1 (+ z_2)),
// z_r at (ring[r].m0 + i) mod zlen, on a planar time buffer [n_ch][..] (i < n: the chunk's n_t L samples of a channel) in one
// pass; launch_inv fills it, launch_stage_out follows.
struct LevelsCombineArgs {
    void *y; long y_ch_stride;                           // in reals
    LevelRing ring[BFIR_LEVEL_RINGS]; int n_rings;
    int n_ch; long n;
    int realsize;
};
void launch_nup_combine(const LevelsCombineArgs &a, hipStream_t s);      // n_rings == 1
void launch_levels_combine(const LevelsCombineArgs &a, hipStream_t s);   // any n_rings: one goes to launch_nup_combine
// the alignment verdict (launch_planar) on n_rings rings, and on their second set where a fade keeps one
inline bool rings_aligned16(const LevelRing *ring, const void *const *z_new, int n_rings, int vec)
{
    bool ok = true;
    for (int r = 0; r < n_rings; r++)
        ok = ok && ring[r].z_ch_stride % vec == 0 && ring[r].zlen % vec == 0 && ring[r].m0r % vec == 0 &&
             ((uintptr_t)ring[r].z | (uintptr_t)(z_new ? z_new[r] : nullptr)) % 16 == 0;
    return ok;
}

// mlevels.hip: the fused back end of a multi-level matrix engine (bfir_engine_create_matrix_levels) with an odd output
// count.  Outputs (0, 1), (2, 3), ... go through k_inv_nup / k_inv_levels with n_ch = 2 floor(n_out / 2) and frame_stride =
// n_out; the last output, channel `ch`, through k_inv_lone: fp32, (re, im) pairs, FLOAT_LE frames, 512 <= L <= 8192 (`plan`
// is the plan of 2L points), one workgroup per block, n_rings = 1, 2 or 3 additions per sample as in LevelsInvArgs; n_rings =
// 0 for a chunk to which no level contributes (the pairs then go through k_inv_pair_ps with the same frame_stride).
struct LoneInvArgs {
    const float *y;                                      // [..][N] product spectra of channel ch, (re, im) pairs
    LevelRing ring[BFIR_LEVEL_RINGS]; int n_rings;       // planar rings of ALL channels: channel ch is read
    float *raw; long frame_off;                          // output frames of ONE engine, frame_stride floats apart
    int frame_stride, ch, n_t;
    float scale;
    InvStats st;                                         // overflow: [n_out] per shard, channel ch is updated
};
void launch_inv_lone(const FftPlan &plan, const LoneInvArgs &a, hipStream_t s);

// lfade.hip: the back end of a crossfaded coefficient change on a two-level or multi-level engine
// (bfir_engine_set_coeff_nup_fade / _levels_fade) for a chunk to which one to three tail levels contribute.  The head's MAC
// has run twice (y_old, y_new as in FadeInvArgs) and every contributing level keeps two time rings of ONE geometry: ring[r]
// describes it and points at the level's output under the old set, z_new[r] at its output under the new set.  Sample n of
// block t is  fade_blend(S_old, S_new),  S_x = ((y_x[n] + z_0,x[m_0]) + z_1,x[m_1]) + z_2,x[m_2]  as in LevelsInvArgs, the
// blend as in FadeInvArgs with m = m0 + t L + n.
// k_inv_lfade, the fused form: k_inv_fade's rule (fp32, (re, im) pairs, FLOAT_LE frames, 512 <= L <= 8192, any n_ch; `plan`
// is the plan of 2L points) with n_rings = 1, 2 or 3 additions per set and sample.
struct LfadeInvArgs {
    const float *y_old; long y_old_ch_stride;            // [n_ch][..][N] product spectra, (re, im) pairs
    const float *y_new; long y_new_ch_stride;
    LevelRing ring[BFIR_LEVEL_RINGS]; const void *z_new[BFIR_LEVEL_RINGS]; int n_rings;
    float *raw; long frame_off;                          // output frames of ONE engine, n_ch channels wide
    int n_ch, n_t;
    float scale;
    float f; int m0;                                     // the ramp: 1 / (K L - 1), and m of sample 0 of block 0
    InvStats st;
};
void launch_inv_lfade(const FftPlan &plan, const LfadeInvArgs &a, hipStream_t s);
// k_lfade_sum, the general form's middle step: y_old[c][i] <- blend(y_old[c][i] + old rings, y_new[c][i] + new rings) on
// planar time buffers [n_ch][..] (i < n: the chunk's n_t L samples of a channel) in one pass; launch_inv fills them,
// launch_stage_out follows.
struct LfadeSumArgs {
    void *y_old; const void *y_new; long ch_stride;      // in reals
    LevelRing ring[BFIR_LEVEL_RINGS]; const void *z_new[BFIR_LEVEL_RINGS]; int n_rings;
    int n_ch; long n;
    double f; int m0;                                    // as in FadeBlendArgs
    int realsize;
};
void launch_lfade_sum(const LfadeSumArgs &a, hipStream_t s);

// mixnscale with one buffer (a7 / a11) on half-complex data, for the stage API.
void launch_reorder(const void *in, void *out, int n_fft, double scale, int to_grouped, int realsize,
                    hipStream_t s);

// SURVEY 8f row 3 (stage API only): N-input mixnscale, dirac_convolve, the blend of
// crossfade_inplace, finite check.
constexpr int BFIR_MAX_MIX = 32;
struct MixArgs {
    const void *in[BFIR_MAX_MIX];
    double scale[BFIR_MAX_MIX];
    int n;
};
void launch_reorder_n(const MixArgs &m, void *out, int n_fft, int to_grouped, int realsize, hipStream_t s);
void launch_dirac(const void *in, void *out, int n_fft, int realsize, hipStream_t s);
void launch_crossfade_blend(const void *crossfade_time, void *buffer_time, const void *buffer_tail, int n_fft2,
                            int realsize, hipStream_t s);
void launch_check_finite(const void *buf, int n, int realsize, int *bad, hipStream_t s);

// One convolve / convolve_add / convolve_inplace call of the stage API with the
// reference's exact operation order (separate multiplies and adds).
// mode 0: d = b*c, mode 1: d += b*c.  d may alias b (in-place form).
void launch_cmul_stage(const void *b, const void *c, void *d, int n_fft, int mode, int realsize,
                       hipStream_t s);

// Per-channel delays on an engine's frame streams (delay.hip; bfir_engine_delay_init / _set_delay).  The source of a
// launch is `hist || piece`: sample m of the piece when m >= 0, else frame H + m of the history (H frames, raw and
// interleaved like the piece).  The table lives in HBM and is rewritten by bfir_engine_set_delay: the delay of every
// channel in frames, whether it has a sub-sample filter, and behind it the filters, [BFIR_DELAY_CH][2 h + 1] reals in
// working precision.
constexpr int BFIR_DELAY_CH = 8;
struct DelayTab { int delay[BFIR_DELAY_CH]; int sub[BFIR_DELAY_CH]; };
// Whole samples, any sample size: frame f of dst (f < n_frames) takes channel c from source frame m0 + f - delay[c].
// tab == nullptr: no delays -- with m0 = n - H and n_frames = H this writes the next history, the last H frames of
// `hist || piece`, also where the piece is shorter than H.
struct DelayCopyArgs {
    void *dst; const void *piece; const void *hist;
    long n_frames, m0, H;
    int C, sample_bytes;
    const DelayTab *tab;
};
// One launch for `a` and, behind its workgroups, for `b` where given (a side's delayed piece and its history update: they
// read the same two buffers and write different ones).
void launch_delay_copy(const DelayCopyArgs &a, const DelayCopyArgs *b, hipStream_t s);
// The sub-sample stage, FLOAT_LE / FLOAT64_LE frames: w_c[n] = sum_k f_c[k] u_c[n - d_c - k], k = 0 .. 2 h ascending, in
// working precision from an LDS copy of the source span; a channel without a filter is the raw shift u_c[n - d_c - h].
struct DelaySubArgs {
    void *dst; const void *piece; const void *hist;
    long n_frames, H;
    int C, sample_bytes, realsize, h;
    const DelayTab *tab; const void *taps;
};
void launch_delay_sub(const DelaySubArgs &a, hipStream_t s);

}  // namespace bfir
