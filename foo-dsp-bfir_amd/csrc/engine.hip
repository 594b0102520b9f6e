// engine.hip -- host side of the fused engine: bfir_engine_* of include/bfir_hip.h.
//
// One bfir_engine reproduces n_eng independent `brutefir` instances
// (brutefir/brutefir.hpp:15-128).  State the reference keeps in host memory
// (brutefir.cpp:738-810) lives in HBM for the life of the engine:
//   H     [GC][B][N]        partition spectra        (bfcoeff_t.data, coeff.cpp:292-354)
//   X     [GC][R][N]        delay line of spectra    (cbuf[n][B]; R = 2*chunk+B slots)
//   Y     [GC][chunk][N]    accumulated spectra      (ocbuf[n])
//   tin   2 x [GC][chunk*L] planar time input, double buffered (input_timecbuf)
//   tout  [GC][chunk*L]     planar time output
//   saved 2 x [GC][L]      history blocks kept across reset / reallocation
// GC = n_eng * C global channels.  A matrix engine (bfir_engine_create_matrix: one engine, C = n_in inputs, Co = n_out
// outputs, one filter per (output, input) pair) keeps the input side -- X, tails, saved -- for its C inputs and the output
// side -- Y, the overflow statistics, the output frames -- for its Co outputs; H is [Co][C][B][N], the MAC k_mac_matrix.
// A mimo engine (bfir_engine_create_mimo) is a matrix engine with up to 64 of each and k_mac_mimo as its MAC; a multi-level
// mimo engine (bfir_engine_create_mimo_levels) a multi-level matrix engine whose levels are mimo engines.
// A run of n blocks is cut into chunks of at most `chunk` blocks.  A chunk is front (fwd; stage_in before it on the
// staging path), MAC and back (inv; stage_out after it on the staging path), software-pipelined over three streams.
// What is written once here, because every path shares it: the path an engine takes (choose_path), the coefficient
// side (FilterRows: check_rows, load_filters; split engines, diagonal or matrix: set_coeff_split, set_coeff_split_fade)
// and the chunk schedule (run_chunk: streams, events, the MAC; queue_fwd / queue_inv and the
// two staging launches are what differs per path).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/bfir_hip.h"
#include "kernels.h"
#include "coeff_tables.h"

using namespace bfir;

// ---------------------------------------------------------------------------
// logging (pinfo.c:17-39 shape) and errors
// ---------------------------------------------------------------------------
static bfir_log_fn g_log = nullptr;

extern "C" void bfir_set_log_callback(bfir_log_fn fn) { g_log = fn; }

void bfir_logf(const char *fmt, ...)
{
    if (!g_log) return;
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_log(buf);
}

extern "C" const char *bfir_strerror(int err)
{
    switch (err) {
    case BFIR_OK: return "ok";
    case BFIR_ERR_NONFINITE: return "NaN or Inf values in the system";
    case BFIR_ERR_COEFF: return "NaN or Inf value among coefficients";
    case BFIR_ERR_ARG: return "invalid argument";
    case BFIR_ERR_NO_DEVICE: return "no HIP device";
    case BFIR_ERR_HIP: return "HIP runtime error";
    case BFIR_ERR_STATE: return "engine not initialised";
    case BFIR_ERR_UNSUPPORTED: return "unsupported format or size";
    case BFIR_ERR_IO: return "file could not be opened";
    }
    return "unknown error";
}

extern "C" int bfir_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" const char *bfir_version(void) { return "bfir-hip 0.1 (gfx950)"; }

#define HIP_TRY(expr)                                                              \
    do {                                                                           \
        hipError_t _e = (expr);                                                    \
        if (_e != hipSuccess) {                                                    \
            bfir_logf("HIP error %s at %s:%d", hipGetErrorString(_e), __FILE__, __LINE__); \
            return BFIR_ERR_HIP;                                                   \
        }                                                                          \
    } while (0)

// brutefir::setup_sample_format (brutefir/brutefir.cpp:435-538): all eleven formats
static int fmt_bytes(int fmt) { return fmt_info(fmt).bytes; }

// A block of planar time samples somewhere in HBM: [GC][L] with a channel stride.
struct BlockRef {
    const void *ptr = nullptr;
    long ch_stride = 0;   // in reals
};

struct bfir_engine {
    int device = 0;
    int L = 0, N = 0, B = 0, s = 0, C = 0, n_eng = 1, GC = 0;
    bool matrix = false;            // n_in -> n_out with one filter per pair (matrix.hip); diagonal: output c = input c * h_c
    int Co = 0, GCo = 0;            // output channels per engine / in all: C and GC, or a matrix engine's n_out
    // a matrix engine created by bfir_engine_create_mimo: up to BFIR_MIMO_MAXCHANNELS inputs and outputs, no delays.  Its
    // partition counts are also kept in HBM (d_nblk, d_nblk2: [o C + i]) for k_mac_mimo (mimo.hip), which runs its MAC when
    // mimo_mac is set: always past 8 channels on either side, where k_mac_matrix cannot run; with both counts within 8 --
    // the same bits either way -- only on BFIR_MIMO_MAC=1, read at creation (choose_path)
    bool mimo = false, mimo_mac = false;
    int in_bytes = 0, out_bytes = 0, in_fmt = 0, out_fmt = 0;
    double in_scale = 1.0, out_scale = 1.0, of_max = 1.0;
    FftPlan plan;
    // a big engine (bfir_engine_create_big, bigconv.hip): partitions past one workgroup's transform.  `plan` stays empty and
    // every transform goes through bplan's two passes (queue_transform_*); the spectra X, H, Y are in its transposed bin
    // order, which the MAC never notices and read_spectrum undoes.  Always the staging path.
    bool big = false;
    BigPlan bplan;
    int chunk = 0, ring = 0;        // allocated geometry
    int want_chunk = 0;                    // blocks per launch (bfir_engine_set_chunk); 0 = automatic; buffers are sized lazily
    void *H = nullptr, *X = nullptr, *Y = nullptr, *tout = nullptr;
    void *tin[2] = {nullptr, nullptr};
    void *Yb[2] = {nullptr, nullptr};      // product spectra, one buffer per chunk parity
    void *saved[2] = {nullptr, nullptr};   // [GC][L] each: materialised history blocks
    // first halves of the reference's input_timecbuf[n][0/1] (brutefir.cpp:255-260):
    // where the block each of them holds currently lives
    BlockRef hist[2];
    int *d_nblk = nullptr;
    DevOverflow *d_of = nullptr;
    int *d_bad = nullptr;
    std::vector<int> nblk;          // host copy
    std::vector<char> eng_init;     // per engine: coefficients set
    unsigned long long blockcounter = 0;
    unsigned long long chunk_seq = 0;       // chunks queued since creation
    int curbuf = 0;
    // front (stage_in, fwd) runs on s_front, the MAC on s_mac, the back (inv, stage_out) on the
    // caller's stream, so fwd(k+1), mac(k) and inv/stage_out(k-1) are on the GPU together
    hipStream_t stream = nullptr, s_front = nullptr, s_mac = nullptr, s_in = nullptr, s_out = nullptr;
    hipEvent_t ev_entry = nullptr, ev_fwd[2] = {nullptr, nullptr}, ev_mac[2] = {nullptr, nullptr};
    hipEvent_t ev_inv[2] = {nullptr, nullptr};
    bool pipe3 = true;                     // BFIR_PIPE=2: MAC on the caller's stream (two-stage schedule)
    // spectra (X, H, Y) as (re, im) pairs instead of the reference's 4 re | 4 im groups: the layout
    // of the fp32 fast MAC kernels; chosen once per engine (N >= 512, fp32)
    bool ilv = false;
    // pair path (pair.hip): FLOAT_LE in and out, even channel count, 512 <= L <= 8192 on top of ilv.
    // No planar time buffers; the engine's time history is the raw frames of the last two blocks,
    // tails[set][i] = [n_eng][L][C] floats, set alternating per chunk so a launch never reads and
    // writes the same copy; hist_raw[i] is where input_timecbuf[n][i]'s first half currently lives.
    bool pair = false;
    // ... with an odd channel count (or one channel) the pairs are blocks t, t + 1 of ONE channel (k_fwd_tp_ps / k_inv_tp_ps)
    bool pair_tp = false;
    // matrix engine that may take the pair path (both counts even); it does while every input feeds some output
    // (bfir_engine_set_coeff_matrix): a channel pair is ONE transform, so a NaN in an input no filter reads would reach
    // the spectra of its partner
    bool pair_cap = false;
    // direct path: any other engine whose frames are FLOAT_LE / FLOAT64_LE in and out (fp64 arithmetic, odd
    // channel counts, partitions outside the pair kernels' range): k_fwd reads the raw frames itself and
    // k_inv writes them, one channel per transform; same history bookkeeping as the pair path (tails of raw
    // input frames), no staging kernels, no planar time buffers.  BFIR_DIRECT=0 / BFIR_PAIR=0 (tuning aids,
    // tests) keep the staging kernels.
    bool direct = false;
    FftPlan plan2;                         // transform of 2L complex points
    // Crossfaded coefficient change (bfir_engine_set_coeff_fade; fftw_convolver.cpp:275-321 over fade_len blocks): the
    // second filter set H2 (as H) with its partition counts, loaded by the call; the fade is blocks fade_pos .. fade_len-1
    // of the next fade_len blocks the engine processes (fade_len = 0: none).  run_blocks cuts the chunks at its end, so a
    // chunk is all fade or all plain; a fade chunk runs the MAC twice -- (H, counts) into Y, (H2, counts2) into Yf -- and
    // the fade back end (queue_inv_fade) instead of queue_inv.  With the last fade block queued the sets swap.
    void *H2 = nullptr;
    int *d_nblk2 = nullptr;
    std::vector<int> nblk2;
    int fade_len = 0, fade_pos = 0;
    float fade_f = 0.f; double fade_d = 0.0;   // 1 / (real)(fade_len L - 1) as the reference computes it (:298, :308)
    bool fade_fused = false;               // k_inv_fade serves this engine (fp32 pairs, FLOAT_LE out, a plan of 2L points)
    bool pair_new = false;                 // matrix engines: the path the NEW set alone asks for (after the fade)
    // the fade is a patch (bfir_engine_set_coeff_matrix_pairs_fade): H2 is H with a list of pairs replaced, and a fade chunk
    // runs k_patch_pairs (patch.hip) over d_patch, the table of the listed pairs, behind the old set's MAC instead of the MAC
    // with H2.  Every way a fade ends clears it (fade_swap_sets, a plain set call), and so does fade_begin for every fade:
    // the pairs call sets it behind fade_begin
    bool fade_patch = false;
    int *d_patch = nullptr; size_t patch_ints = 0;   // [Co + 1] row starts, then [entries][3]: input, nb_new, nb_old (PatchArgs)
    // A multi-level matrix or mimo engine (bfir_engine_set_coeff_matrix_levels_pairs_fade): fade_patch is set on the head and
    // on every active tail, each level with a table of its own in its d_patch (the counts are per level), and a launch that
    // needs both sets -- the head while it fades, a tail in lf_mode 1 -- runs the patch behind the old set's MAC instead of
    // k_mac_duo / k_wduo.  lfade_finish clears it on the tails.  patch_fused: on a level whose MAC is k_mac_mimo the two
    // launches are one, k_wpatch (wpatch.hip), the same bits; BFIR_PATCH_FUSED=0|1, read at creation (choose_path)
    bool patch_fused = false;
    // A coefficient bank (bfir_engine_bank_create; uniform matrix and mimo engines): n rows in the form of H's,
    // [entries][B][N], each transformed once by bfir_engine_bank_load, with the partition count it was loaded with on the host
    // (0: empty).  The set calls that name entries copy rows from it into H or H2 with k_bank_gather (bank.hip) over d_gather,
    // the table of the listed rows; the engine's sets are copies and never point into the bank.
    void *bank = nullptr;
    std::vector<int> bank_nb;
    int *d_gather = nullptr; size_t gather_ints = 0;   // [rows][3]: destination row, entry or -1, partitions (BankArgs);
                                                       // a mix call: [rows][BFIR_BANK_MIX_REC], k_bank_mix's records (BankMixArgs)
    // The bank of a multi-level matrix or mimo engine (bfir_engine_levels_bank_create): one such store per level, in `bank` of
    // the head and of every tail, [entries][blocks[k]][2 L_k], loaded through the level split (bfir_engine_levels_bank_load).
    // The head keeps every entry's tap count (0: empty) and its partitions on every level, [entry][BFIR_MAX_LEVELS]; its
    // d_gather is k_lbank_gather's table (lbank.hip), [rows][2 + BFIR_MAX_LEVELS], for all levels of a call in one launch
    // (a mix call: k_lbank_mix's records, [rows][BFIR_LBANK_MIX_REC], lbankmix.hip).
    std::vector<int> lbank_len, lbank_nb;
    void *Yf[2] = {nullptr, nullptr};      // products with H2: [GCo][yf_blocks][N], one per chunk parity like Yb
    int yf_blocks = 0;
    void *ft[2] = {nullptr, nullptr};      // general back end: planar y_old / y_new, [GCo][ft_blocks][L] each
    int ft_blocks = 0;
    float *tails[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    const float *hist_raw[2] = {nullptr, nullptr};
    // HP-TPDF dither (integer output + apply_dither; dither.hip): the reference instance's random table
    // (every engine of a batch would build the same one) and dither_state_t per global channel
    int8_t *d_dither_tab = nullptr; int dither_size = 0;
    DevDitherState *d_dither_state = nullptr;
    // latency path (bfir_engine_run with a handful of blocks, the plug-in's one run() per block): everything
    // on one stream, no events, kernels read and write the pinned staging buffers across the host link
    bool inline_launch = false;            // set around run_chunk by run_small()
    bool async_pending = false;            // run_device queued work that nobody has waited for yet
    int *h_bad = nullptr;                  // pinned: one flag per block of a latency-path call (flag_bad, kernels.h)
    int *bad_host_cur = nullptr;           // ... what the kernels of the chunk being launched are given (null outside run_small)
    bool serial = false;                   // BFIR_PIPE=1: everything on the caller's stream (kernel timing runs)
    // host-pointer path: pinned + device staging, double buffered
    void *pin_in[2] = {nullptr, nullptr}, *pin_out[2] = {nullptr, nullptr};
    void *dev_in[2] = {nullptr, nullptr}, *dev_out[2] = {nullptr, nullptr};
    hipEvent_t ev_h2d[2] = {nullptr, nullptr}, ev_comp[2] = {nullptr, nullptr}, ev_d2h[2] = {nullptr, nullptr};
    size_t stage_bytes_in = 0, stage_bytes_out = 0;
    // Two-level ("nup") engine (bfir_engine_create_nup): THIS engine is the head level -- partitions of L over taps
    // [0, D), D = B L -- and owns the tail level, a diagonal engine of partitions Lt = r L over the taps from D on, whose
    // back end is a planar inverse into a time ring (nup_tail; queue_inv_tail).  Output = y_head + z[n - D], z the tail's
    // overlap-save output in blocks of Lt from sample 0.  Tail block j covers head blocks [j r, (j + 1) r); it is run as
    // soon as its last head block has arrived and first read by head block j r + B (causal: B >= r).  Neither level pairs
    // blocks in time and neither takes the staging path, so the bits do not depend on how the blocks arrive.
    // A multi-level engine (bfir_engine_create_levels) is the same with up to BFIR_MAX_LEVELS - 1 tails, every one a
    // diagonal engine with a ring of its own: tail[i] is level k = i + 1, partitions of L_k = lv_r[i] L over the taps from
    // D_k = lv_D[i] L on; output = ((y_head + z_1[n - D_1]) + z_2[n - D_2]) + z_3[n - D_3].  Two levels are n_tail = 1.
    bool nup = false, nup_tail = false;
    bool levels = false;                   // created by bfir_engine_create_levels: a kind of its own at the C ABI
    // created by bfir_engine_create_matrix_levels, a kind of its own too: the head and every tail are matrix engines -- the
    // delay lines, raw tails and pbuf count by the C inputs; the products, the time rings, tout, the overflow shards and the
    // output frames by the Co outputs -- and every level's MAC is k_mac_matrix.  bfir_engine_create_mimo_levels makes the same
    // with `mimo` set on every level: up to BFIR_MIMO_MAXCHANNELS of each, every level's counts in its d_nblk / d_nblk2 too,
    // and k_mac_mimo as the MAC of every level where mimo_mac is set
    bool mlevels = false;
    // the head of a split engine: its contributing chunks take the fused back end (nup.hip, levels.hip, mlevels.hip).  A
    // diagonal engine's is its pair path; a matrix engine's is chosen by the output side alone (choose_path), whatever the
    // front end does
    bool back_fused = false;
    int n_tail = 0;
    bfir_engine *tail[BFIR_MAX_LEVELS - 1] = {nullptr, nullptr, nullptr};
    int lv_r[BFIR_MAX_LEVELS - 1] = {0, 0, 0}, lv_D[BFIR_MAX_LEVELS - 1] = {0, 0, 0};   // L_k / L and D_k / L (head blocks)
    bool lv_active[BFIR_MAX_LEVELS - 1] = {false, false, false};   // the filters reach past D_k: without, level k does no work at all
    int nup_mask = 0;                      // bit i: tail[i] contributes to the chunk being queued (run_blocks cuts chunks so: every block the same set)
    // raw input frames [L_last][C] from the start of the largest level's block that is still arriving (kept across calls):
    // head block a at (a mod lv_r[n_tail - 1]) L.  The blocks of all levels start at sample 0 and their lengths are nested
    // powers of two, so the one buffer holds every level's partial block; frames of head blocks below pbuf_upto are there.
    void *pbuf = nullptr;
    long long pbuf_upto = 0;
    hipEvent_t ev_nup = nullptr;           // pbuf is filled on the caller's stream; a tail's front waits for this
    // on the tail: its output, planar [GC][zblocks Lt] reals, tail block j in slot j % zblocks; blocks [z_from, z_next) are
    // (or will, in stream order, be) there.  zblocks >= ceil((chunk + B) / r) + 2: what one head chunk can still need
    // plus what is written ahead of it.
    void *zring = nullptr; int zblocks = 0;
    long long z_from = 0, z_next = 0;
    // Crossfaded coefficient change on a two- or multi-level engine (bfir_engine_set_coeff_nup_fade / _levels_fade).  The
    // head fades as a uniform engine does (H2, fade_len, fade_pos, Yf above), over head blocks [a_f, a_f + K), a_f its block
    // counter at the call.  Tail i (r = lv_r[i], Dk = lv_D[i]; head block a reads its block (a - Dk) / r) must have its
    // output under the new set from block j0 = (a_f - Dk) / r on and under the old set up to block j1 = (a_f + K - 1 - Dk) / r,
    // so it keeps a second time ring, zring2, with the geometry of the first, for the new set's output:
    //   at the call   blocks [j0, z_next) have run with the old set: their MAC runs again with H2 on the delay line the tail
    //                 still holds (its ring is ring_extra = ceil(Dk / r) + 1 slots deeper for this) into zring2;
    //   lf_mode 1     blocks up to j1: MAC and inverse twice, (H, zring) and (H2, zring2); launches are cut at j1;
    //   lf_mode 2     blocks past j1: the sets have swapped on the tail, the one inverse goes into zring2;
    //   fade end      with the head's last fade block queued (block j1 is complete by then, because Dk >= r) zring2
    //                 becomes zring (lf_mode 0).
    // The head's fading chunks blend the sums over the old rings and over the new rings (queue_inv_lfade).
    int ring_extra = 0;                    // on a tail: delay-line slots on top of 2 chunk + B
    void *zring2 = nullptr;                // on a tail: allocated, like H2 and Yf, at the first fade
    int lf_mode = 0; long long lf_j1 = -1;
    bool lf_stop = false;                  // on a tail: the new set does not reach this level, it stops when the fade ends
    // Every level of a multi-level matrix engine: a launch that needs both sets of a fade runs k_mac_duo (mfade.hip) instead
    // of k_mac_matrix twice.  BFIR_MFADE_DUO=0|1, read at creation (choose_path).  A level with mimo_mac set: k_wduo (wduo.hip)
    // instead of k_mac_mimo twice
    bool mfade_duo = true;
    // The channel-pair inverse with 16-byte frame stores (k_inv_quad_ps, quad.hip; InvPairArgs.quad): by default for launches
    // that fill the GPU.  BFIR_INV_QUAD=0|1 forbids it / takes it wherever it applies, read at creation (choose_path)
    int inv_quad = -1;
    // The channel-pair forward transform with 16-byte frame loads (k_fwd_wide_ps, wide.hip; FwdPairArgs.wide): the same rule.
    // BFIR_FWD_WIDE=0|1, read at creation (choose_path)
    int fwd_wide = -1;
    // profiling
    bool profiling = false;
    struct Span { int k; hipEvent_t a, b; };
    std::vector<Span> spans;
    std::vector<hipEvent_t> ev_pool;
    double prof_ms[BFIR_K_COUNT] = {0, 0, 0, 0, 0};
    long prof_n[BFIR_K_COUNT] = {0, 0, 0, 0, 0};
    // Per-channel delays on the input frames (side 0: the engine proper reads the delayed stream) and on the output frames
    // (side 1: the caller receives it); bfir_engine_delay_init, delay.hip.  A side keeps the last H = max_delay + 2 h raw
    // frames of its stream in hist[cur] -- every launch writes the next history into the other buffer -- one piece
    // (e->chunk blocks) of scratch frames between its kernels and the engine proper, and the table its kernels read.
    struct DelaySide {
        bool on = false;
        int max_delay = 0, steps = 0, h = 0;
        double beta = 0.0;
        long H = 0;
        void *hist[2] = {nullptr, nullptr}; int cur = 0;
        void *scratch = nullptr; size_t scratch_bytes = 0;
        void *d_tab = nullptr;             // DelayTab, then the taps
        std::vector<int> delay, sub;       // host copy: what bfir_engine_get_delay returns
    };
    DelaySide dly[2];
    hipEvent_t ev_dly = nullptr;           // the delayed input piece is in scratch: the front waits for this
    hipEvent_t ev_dly_done = nullptr; hipStream_t dly_stream = nullptr;   // the last call's launches, and the stream they went to
};

static size_t cbuf_bytes(const bfir_engine *e) { return (size_t)e->N * (size_t)e->s; }

// level k = 0 .. n_tail of a split engine: the head, then its tails (any other engine is its own level 0)
static bfir_engine *level(const bfir_engine *e, int k) { return k == 0 ? const_cast<bfir_engine *>(e) : e->tail[k - 1]; }

// everything a delayed side owns (the device is idle)
static void delay_free(bfir_engine *e, int side)
{
    bfir_engine::DelaySide &d = e->dly[side];
    void *bufs[] = {d.hist[0], d.hist[1], d.scratch, d.d_tab};
    for (void *b : bufs) if (b) (void)hipFree(b);
    d = bfir_engine::DelaySide();
}

// Copy the two history blocks into the engine-owned `saved` buffers so they
// survive the work buffers they may point into.  A reference only ever points
// at its own saved[i] or into a time buffer, never at the other saved buffer.
static int materialise_history(bfir_engine *e)
{
    HIP_TRY(hipDeviceSynchronize());
    const size_t Ls = (size_t)e->L * e->s;
    for (int i = 0; i < 2; i++) {
        if (e->hist[i].ptr != e->saved[i])
            HIP_TRY(hipMemcpy2D(e->saved[i], Ls, e->hist[i].ptr, (size_t)e->hist[i].ch_stride * e->s, Ls, e->GC,
                                hipMemcpyDeviceToDevice));
        e->hist[i].ptr = e->saved[i];
        e->hist[i].ch_stride = e->L;
    }
    HIP_TRY(hipDeviceSynchronize());
    return BFIR_OK;
}

// the pinned + device staging buffers of the host-pointer path (ensure_staging)
static void free_staging(bfir_engine *e)
{
    for (int i = 0; i < 2; i++) {
        if (e->pin_in[i]) (void)hipHostFree(e->pin_in[i]);
        if (e->pin_out[i]) (void)hipHostFree(e->pin_out[i]);
        if (e->dev_in[i]) (void)hipFree(e->dev_in[i]);
        if (e->dev_out[i]) (void)hipFree(e->dev_out[i]);
        e->pin_in[i] = e->pin_out[i] = e->dev_in[i] = e->dev_out[i] = nullptr;
    }
    e->stage_bytes_in = e->stage_bytes_out = 0;
}

static void free_work(bfir_engine *e)
{
    void **bufs[] = {&e->X, &e->Yb[0], &e->Yb[1], &e->tin[0], &e->tin[1], &e->tout};
    for (void **b : bufs) { if (*b) (void)hipFree(*b); *b = nullptr; }
    free_staging(e);
    e->chunk = e->ring = 0;
    if (e->h_bad) { (void)hipHostFree(e->h_bad); e->h_bad = nullptr; }
}

// (Re)allocate the chunk-sized work buffers.  The delay line is carried over
// slot by slot when the ring size changes; the time history is moved into
// `saved` first because it may live in the buffers being freed.
static int alloc_work(bfir_engine *e, int chunk)
{
    const size_t cb = cbuf_bytes(e);
    // fwd of chunk k+1 may run while mac of chunk k still reads its B-1 older slots; a tail level of a two- or multi-level
    // engine keeps ring_extra blocks more, whose MAC a fade runs again (bfir_engine_set_coeff_levels_fade)
    const int ring = 2 * chunk + e->B + e->ring_extra;
    if (e->X) { int rc = materialise_history(e); if (rc != BFIR_OK) return rc; }
    void *X = nullptr, *Y0 = nullptr, *Y1 = nullptr, *tin0 = nullptr, *tin1 = nullptr, *tout = nullptr;
    HIP_TRY(hipMalloc(&X, (size_t)e->GC * ring * cb));
    HIP_TRY(hipMalloc(&Y0, (size_t)e->GCo * chunk * cb));
    HIP_TRY(hipMalloc(&Y1, (size_t)e->GCo * chunk * cb));
    if (e->nup && !e->back_fused) HIP_TRY(hipMalloc(&tout, (size_t)e->GCo * chunk * e->L * e->s));   // the general nup back end's planar sum
    if (!e->pair && !e->direct) {   // the pair and direct paths have no planar time buffers
        HIP_TRY(hipMalloc(&tin0, (size_t)e->GC * chunk * e->L * e->s));
        HIP_TRY(hipMalloc(&tin1, (size_t)e->GC * chunk * e->L * e->s));
        HIP_TRY(hipMalloc(&tout, (size_t)e->GCo * chunk * e->L * e->s));
    }
    HIP_TRY(hipMemset(X, 0, (size_t)e->GC * ring * cb));
    if (e->X) {
        // keep the last B-1 spectra (a tail level: ring_extra more): absolute block j lives in slot j % ring
        const int keep = (int)std::min<unsigned long long>(e->blockcounter, (unsigned long long)(e->B - 1 + e->ring_extra));
        for (int d = 1; d <= keep; d++) {
            const unsigned long long j = e->blockcounter - d;
            const size_t so = (size_t)(j % e->ring) * cb, dn = (size_t)(j % ring) * cb;
            HIP_TRY(hipMemcpy2D((char *)X + dn, (size_t)ring * cb, (char *)e->X + so, (size_t)e->ring * cb, cb,
                                e->GC, hipMemcpyDeviceToDevice));
        }
    }
    HIP_TRY(hipDeviceSynchronize());
    free_work(e);
    e->X = X; e->Yb[0] = Y0; e->Yb[1] = Y1; e->tin[0] = tin0; e->tin[1] = tin1; e->tout = tout;
    e->chunk = chunk; e->ring = ring;
    return BFIR_OK;
}

// Which kernels the engine runs on and how a chunk is scheduled: ilv (spectrum layout), pair / pair_tp / pair_cap,
// direct, pipe3, serial.  Every switch is read HERE, once per engine, at creation.
static void choose_path(bfir_engine *e)
{
    e->ilv = e->s == 4 && e->N >= 512;   // fp32: (re, im) pairs from N = 512 (whole 256-bin columns)
    // BFIR_PAIR=0 (tuning aid) keeps the planar staging kernels
    const char *pv = getenv("BFIR_PAIR");
    // odd channel counts pair blocks in time (BFIR_PAIR_TIME=0 keeps them on the general path)
    const char *tv = getenv("BFIR_PAIR_TIME");
    const bool tp_ok = !(tv && atoi(tv) == 0);
    e->pair_tp = (e->C % 2) == 1 && tp_ok;
    e->pair = e->ilv && e->in_fmt == 8 && e->out_fmt == 8 && ((e->C % 2) == 0 || e->pair_tp) &&
              pair_supported(e->L) && !(pv && atoi(pv) == 0);
    e->pair_tp = e->pair_tp && e->pair;
    if (e->matrix) {
        // channel pairs on both sides or direct mode: time pairs transform blocks t, t + 1 together, so where a launch
        // starts would change the bits of its blocks (a matrix engine's outputs do not depend on the chunking)
        // A level of a multi-level matrix engine pairs by its INPUT side alone: its forward kernel touches nothing else, a
        // tail's back end is a planar inverse, and the head's back ends take an odd output count (queue_inv, queue_inv_nup)
        const bool split = e->nup || e->nup_tail;
        e->pair = e->pair && e->C % 2 == 0 && (split || e->Co % 2 == 0);
        e->pair_tp = false;
        e->pair_cap = e->pair;
    }
    const char *dv = getenv("BFIR_DIRECT");
    // worth it where a channel's samples are 8 bytes apart or wider units: FLOAT64 frames (any C), or one
    // channel (contiguous samples), or float frames with an even channel count (the reference plug-in's own shape:
    // fp64 arithmetic, float32 frames), which k_fwd / k_inv move a channel PAIR at a time with both channels in one
    // workgroup (stereo: two whole frames per lane; wider frames since round 3: 33.5 -> ~40 Gsamples/s at 4-8 channels).  Other 4-byte samples at a stride
    // (float frames, C > 2) are faster through the staging kernels (profiles/r02_other_configs.txt: one
    // channel per workgroup ran the plug-in's shape at 11.4 instead of 20.6 Gsamples/s).  BFIR_DIRECT=1
    // forces it (tests).
    const bool stereo = e->in_bytes == 4 && e->out_bytes == 4 && (e->C % 2) == 0 && !e->ilv &&
                        direct_stereo_supported(e->L, e->s);
    // ... and, since round 3, any float / double frames of an fp64 engine whose transform the run kernels take (k_fwd_run /
    // k_inv_run hide the strided loads under the transform: 3 / 5 channels of float32 frames 33 -> 41-42 Gsamples/s)
    const bool wide = (e->in_bytes == 8 && e->out_bytes == 8) || e->C == 1 || stereo || run64_supported(e->L, e->s);
    e->direct = !e->pair && fmt_is_native(e->in_fmt) && fmt_is_native(e->out_fmt) && !(pv && atoi(pv) == 0) &&
                (dv ? atoi(dv) != 0 : wide);
    if (e->matrix) e->direct = !e->pair;   // a matrix engine has no staging path: float frames only, direct where not paired
    if (e->big) e->pair = e->pair_tp = e->direct = false;   // the two-pass transforms take the planar form only
    if (e->nup || e->nup_tail) {           // both levels of a two-level engine likewise, and no pairs in time: an odd count is direct
        e->pair = e->pair && !e->pair_tp;
        e->pair_tp = false;
        e->direct = !e->pair;
        // the fused back ends read Y as (re, im) pairs and write FLOAT_LE frames: nothing in them depends on the front end,
        // so a matrix head takes them by its output side alone (an odd count: the last output through k_inv_lone)
        e->back_fused = e->nup && (e->matrix ? e->s == 4 && e->ilv && e->out_fmt == BFIR_SAMPLE_FORMAT_FLOAT_LE && pair_supported(e->L)
                                             : e->pair);
    }
    // fp64 engines whose transforms the run kernels take keep their spectra -- delay line, filter partitions, products --
    // as (re, im) PAIRS like the fp32 engines, not in the reference's groups of four: one 16-byte access per bin in the
    // MAC instead of two of 8, the forward kernel's spectrum straight from registers (no LDS staging), conflict-free reads
    // in the inverse.  Only where every kernel on the engine's way reads pairs: direct mode, the systolic MAC (up to 256
    // partitions) -- so the switches that pick other kernels keep the groups (all read HERE, at creation, for such engines).
    // BFIR_F64_PAIRS=0: off (A/B).  Same arithmetic either way: the same bits.
    {
        const char *fp = getenv("BFIR_F64_PAIRS"), *ms = getenv("BFIR_MAC_SYS");
        const bool other_mac = (ms && atoi(ms) == 0) || getenv("BFIR_MAC_BATCHED");
        if (e->s == 8 && e->direct && pairs64_supported(e->L, e->s) && e->B <= BFIR_MAC_SYS_MAX_B && !other_mac &&
            !(fp && atoi(fp) == 0))
            e->ilv = true;
    }
    // both sets of a fading multi-level matrix engine in one MAC launch (k_mac_duo), the default: lower than two launches of
    // k_mac_matrix in every paired run ("Crossfades on multi-level matrix engines"); BFIR_MFADE_DUO=0 keeps the two.
    // The same switch and default on a level whose MAC is k_mac_mimo: k_wduo against two launches of it ("k_wduo")
    if (const char *mv = getenv("BFIR_MFADE_DUO")) e->mfade_duo = atoi(mv) != 0;
    // MAC and patch of a fading pair list in one launch (k_wpatch) on the levels of a multi-level engine whose MAC is
    // k_mac_mimo, only on BFIR_PATCH_FUSED=1: the two launches measured faster ("Pair lists on multi-level engines")
    if (const char *pf = getenv("BFIR_PATCH_FUSED")) e->patch_fused = atoi(pf) != 0;
    // k_mac_matrix stays the default where it can run: k_mac_mimo was not faster there ("k_mac_mimo")
    if (e->mimo) {
        const char *mm = getenv("BFIR_MIMO_MAC");
        e->mimo_mac = e->C > BFIR_MAT_MAX || e->Co > BFIR_MAT_MAX || (mm && atoi(mm) != 0);
    }
    if (const char *qv = getenv("BFIR_INV_QUAD")) e->inv_quad = atoi(qv) != 0;
    if (const char *wv = getenv("BFIR_FWD_WIDE")) e->fwd_wide = atoi(wv) != 0;
    if (const char *pm = getenv("BFIR_PIPE")) { e->pipe3 = atoi(pm) >= 3; e->serial = atoi(pm) == 1; }
    // fp64 engines: one stream.  Their kernels are bound by issue and latency, not by memory, each fills the GPU by itself, and
    // three of them side by side only get into each other's way: the plug-in's shape 42.8 -> 45.9 Gsamples/s, 8 channels 42.5 ->
    // 44.6, cfg5 43.1 either way (profiles/r03_fp64.txt).  The fp32 headline gains 10 % from the three-stream schedule.
    else if (e->s == 8) { e->pipe3 = false; e->serial = true; }
}

// which family the engine runs on (tests read it; per-launch variants such as CPW = 2 depend on alignment and are not here)
static void log_creation(const bfir_engine *e)
{
    char shape[64];
    if (e->big) {
        bfir_logf("bfir engine: big, %d x %d channels, partition %d = %d x %d, %d blocks, realsize %d on device %d. layout=%s",
                  e->n_eng, e->C, e->L, 1 << e->bplan.log2m1, 1 << e->bplan.log2m2, e->B, e->s, e->device, e->ilv ? "pairs" : "grouped");
        return;
    }
    // a matrix engine's path=pair can give way to direct mode while an input feeds no output (bfir_engine_set_coeff_matrix logs it)
    if (e->matrix) snprintf(shape, sizeof(shape), "%s %d -> %d", e->mimo ? "mimo" : "matrix", e->C, e->Co);
    else snprintf(shape, sizeof(shape), "%d x %d channels", e->n_eng, e->C);
    bfir_logf("bfir engine: %s, partition %d, %d blocks, realsize %d on device %d. path=%s layout=%s run=%s",
              shape, e->L, e->B, e->s, e->device,
              e->pair_tp ? "time-pair" : e->pair ? "pair" : e->direct ? "direct" : "staging", e->ilv ? "pairs" : "grouped",
              e->s == 8 && e->direct && run64_supported(e->L, e->s) ? "on" : "off");
}

// matrix: `channels` inputs, `channels_out` outputs, one engine (bfir_engine_create_matrix); else channels_out == channels
// nup_level: 0, or 1 / 2 for the head / tail level of a two-level engine (bfir_engine_create_nup)
// max_channels: the channel cap of the calling kind -- BFIR_MIMO_MAXCHANNELS for a mimo engine (a matrix engine with that cap)
static bfir_engine *engine_create(int n_engines, int filter_length, int filter_blocks, int realsize, int channels,
                                  int channels_out, bool matrix, int in_format, int out_format, int sampling_rate,
                                  int apply_dither, int device, int *err, int nup_level = 0, int ring_extra = 0, bool big = false,
                                  int max_channels = BFIR_MAXCHANNELS)
{
    const bool mimo = matrix && max_channels > BFIR_MAXCHANNELS;
    int dummy;
    if (!err) err = &dummy;
    *err = BFIR_OK;
    // brutefir.cpp:652 (channel limit), fftw_convolver.cpp:64-74 (realsize, length)
    if (channels < 1 || channels > max_channels || channels_out < 1 || channels_out > max_channels) {
        bfir_logf("Number of channels (%d) exceeds limit (%d).", std::max(channels, channels_out), max_channels);
        *err = BFIR_ERR_ARG; return nullptr;
    }
    if (realsize != 4 && realsize != 8) { bfir_logf("Invalid real size %d.", realsize); *err = BFIR_ERR_ARG; return nullptr; }
    if (filter_length < 1 || (filter_length & (filter_length - 1))) {
        bfir_logf("Invalid length %d.", filter_length); *err = BFIR_ERR_ARG; return nullptr;
    }
    if (filter_blocks < 1 || n_engines < 1) { *err = BFIR_ERR_ARG; return nullptr; }
    if (!fmt_bytes(in_format) || !fmt_bytes(out_format)) { *err = BFIR_ERR_UNSUPPORTED; return nullptr; }
    int ndev = bfir_device_count();
    if (ndev <= 0) { *err = BFIR_ERR_NO_DEVICE; return nullptr; }
    if (device < 0 || device >= ndev) { *err = BFIR_ERR_ARG; return nullptr; }
    if (hipSetDevice(device) != hipSuccess) { *err = BFIR_ERR_HIP; return nullptr; }

    bfir_engine *e = new bfir_engine();
    e->device = device;
    e->L = filter_length; e->N = 2 * filter_length; e->B = filter_blocks; e->s = realsize;
    e->C = channels; e->n_eng = n_engines; e->GC = n_engines * channels;
    e->matrix = matrix; e->Co = channels_out; e->GCo = n_engines * channels_out;
    e->mimo = mimo;
    e->in_bytes = fmt_bytes(in_format); e->out_bytes = fmt_bytes(out_format);
    e->in_fmt = in_format; e->out_fmt = out_format;
    // setup_input: normalised scale 1/2^(bits-1); setup_output: full scale; overflow max
    // 2^(bits-1)-1 for integers, 1.0 for floats (brutefir.cpp:395-420, 546-582, 672-684)
    e->in_scale = fmt_info(in_format).isfloat ? 1.0 : 1.0 / fmt_full_scale(in_format);
    e->out_scale = fmt_info(out_format).isfloat ? 1.0 : fmt_full_scale(out_format);
    e->of_max = fmt_info(out_format).isfloat ? 1.0 : fmt_full_scale(out_format) - 1.0;
    e->nup = nup_level == 1; e->nup_tail = nup_level == 2;
    e->ring_extra = ring_extra;
    e->big = big;
    choose_path(e);
    e->nblk.assign(matrix ? (size_t)e->Co * e->C : (size_t)e->GC, 0);   // matrix: [o C + i]
    e->eng_init.assign(n_engines, 0);
    int rc = big ? big_plan_create(&e->bplan, filter_length, realsize) : fft_plan_create(&e->plan, filter_length, realsize);
    if (rc != 0) { *err = (rc == -1) ? BFIR_ERR_UNSUPPORTED : BFIR_ERR_HIP; delete e; return nullptr; }
    auto fail = [&](int code) { *err = code; bfir_engine_destroy(e); return (bfir_engine *)nullptr; };
    if (e->pair || e->direct) {
        if ((e->pair || e->back_fused) && fft_plan_create(&e->plan2, 2 * filter_length, 4) != 0) return fail(BFIR_ERR_HIP);
        const size_t tb = (size_t)e->n_eng * e->L * e->C * e->in_bytes;     // raw input frames of one block
        for (int st = 0; st < 2; st++)
            for (int i = 0; i < 2; i++) {
                if (hipMalloc((void **)&e->tails[st][i], tb) != hipSuccess) return fail(BFIR_ERR_HIP);
                (void)hipMemset(e->tails[st][i], 0, tb);   // input_timecbuf starts zeroed (brutefir.cpp:769)
            }
        // chunk 0 writes set 0, so the (zero) history it reads lives in set 1
        e->hist_raw[0] = e->tails[1][0]; e->hist_raw[1] = e->tails[1][1];
    }
    hipStream_t *streams[] = {&e->stream, &e->s_front, &e->s_mac, &e->s_in, &e->s_out};
    for (hipStream_t *st : streams)
        if (hipStreamCreateWithFlags(st, hipStreamNonBlocking) != hipSuccess) return fail(BFIR_ERR_HIP);
    hipEvent_t *events[] = {&e->ev_entry, &e->ev_fwd[0], &e->ev_fwd[1], &e->ev_mac[0], &e->ev_mac[1],
                            &e->ev_inv[0], &e->ev_inv[1],
                            &e->ev_h2d[0], &e->ev_h2d[1], &e->ev_comp[0], &e->ev_comp[1], &e->ev_d2h[0], &e->ev_d2h[1]};
    for (hipEvent_t *ev : events)
        if (hipEventCreateWithFlags(ev, hipEventDisableTiming) != hipSuccess) return fail(BFIR_ERR_HIP);
    const size_t cb = cbuf_bytes(e), Ls = (size_t)e->L * e->s;
    const size_t n_filters = matrix ? (size_t)e->Co * e->C : (size_t)e->GC;
    const size_t nblk_bytes = sizeof(int) * (mimo ? n_filters : (size_t)e->GC);   // a mimo engine: the table of k_mac_mimo
    if (hipMalloc(&e->H, n_filters * e->B * cb) != hipSuccess ||
        hipMalloc(&e->saved[0], (size_t)e->GC * Ls) != hipSuccess ||
        hipMalloc(&e->saved[1], (size_t)e->GC * Ls) != hipSuccess ||
        hipMalloc((void **)&e->d_nblk, nblk_bytes) != hipSuccess ||
        hipMalloc((void **)&e->d_of, sizeof(DevOverflow) * e->GCo * BFIR_OF_SHARDS) != hipSuccess ||
        hipMalloc((void **)&e->d_bad, sizeof(int)) != hipSuccess)
        return fail(BFIR_ERR_HIP);
    (void)hipMemset(e->H, 0, n_filters * e->B * cb);
    for (int i = 0; i < 2; i++) {   // input_timecbuf starts zeroed (brutefir.cpp:769)
        (void)hipMemset(e->saved[i], 0, (size_t)e->GC * Ls);
        e->hist[i].ptr = e->saved[i]; e->hist[i].ch_stride = e->L;
    }
    (void)hipMemset(e->d_nblk, 0, nblk_bytes);
    (void)hipMemset(e->d_of, 0, sizeof(DevOverflow) * e->GCo * BFIR_OF_SHARDS);
    (void)hipMemset(e->d_bad, 0x7f, sizeof(int));
    if (apply_dither && !fmt_info(out_format).isfloat) {
        // dither::dither(n_channels, sampling_rate, realsize, max_dither_table_size = 0, filter_length, state)
        // as brutefir::init_convolver builds it (brutefir.cpp:709-714)
        const int spacing = dither_spacing(channels, sampling_rate, 0, filter_length);
        if (spacing < 0) return fail(BFIR_ERR_ARG);
        std::vector<int8_t> tab;
        dither_fill_table(tab, channels, spacing);
        std::vector<DevDitherState> st((size_t)e->GC);
        for (int gc = 0; gc < e->GC; gc++) { memset(&st[gc], 0, sizeof(DevDitherState)); st[gc].randtab_ptr = (gc % channels) * spacing + 1; }
        if (hipMalloc((void **)&e->d_dither_tab, tab.size()) != hipSuccess ||
            hipMalloc((void **)&e->d_dither_state, st.size() * sizeof(DevDitherState)) != hipSuccess ||
            hipMemcpy(e->d_dither_tab, tab.data(), tab.size(), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(e->d_dither_state, st.data(), st.size() * sizeof(DevDitherState), hipMemcpyHostToDevice) != hipSuccess)
            return fail(BFIR_ERR_HIP);
        e->dither_size = (int)tab.size();
        bfir_logf("Dither table size is %d bytes.", e->dither_size);
    }
    if (alloc_work(e, 1) != BFIR_OK) return fail(BFIR_ERR_HIP);
    if (hipDeviceSynchronize() != hipSuccess) return fail(BFIR_ERR_HIP);
    log_creation(e);
    return e;
}

extern "C" bfir_engine *bfir_engine_create_batch(int n_engines, int filter_length, int filter_blocks,
                                                 int realsize, int channels, int in_format,
                                                 int out_format, int sampling_rate, int apply_dither,
                                                 int device, int *err)
{
    return engine_create(n_engines, filter_length, filter_blocks, realsize, channels, channels, false, in_format, out_format,
                         sampling_rate, apply_dither, device, err);
}

extern "C" bfir_engine *bfir_engine_create_matrix(int filter_length, int filter_blocks, int realsize, int n_inputs,
                                                  int n_outputs, int in_format, int out_format, int device, int *err)
{
    int dummy;
    if (!err) err = &dummy;
    if (n_inputs < 1 || n_inputs > BFIR_MAXCHANNELS || n_outputs < 1 || n_outputs > BFIR_MAXCHANNELS) {
        bfir_logf("Number of channels (%d -> %d) exceeds limit (%d).", n_inputs, n_outputs, BFIR_MAXCHANNELS);
        *err = BFIR_ERR_ARG; return nullptr;
    }
    // float frames only (no staging kernels, no dither)
    if (!fmt_is_native(in_format) || !fmt_is_native(out_format)) { *err = BFIR_ERR_UNSUPPORTED; return nullptr; }
    return engine_create(1, filter_length, filter_blocks, realsize, n_inputs, n_outputs, true, in_format, out_format, 44100, 0,
                         device, err);
}

extern "C" bfir_engine *bfir_engine_create(int filter_length, int filter_blocks, int realsize,
                                           int channels, int in_format, int out_format,
                                           int sampling_rate, int apply_dither, int device, int *err)
{
    return bfir_engine_create_batch(1, filter_length, filter_blocks, realsize, channels, in_format,
                                    out_format, sampling_rate, apply_dither, device, err);
}

// the partition lengths bfir_engine_create takes (fft_plan_create: 2^4 .. 2^14, one transform's LDS buffer within 160 KB)
static bool length_supported(int filter_length, int realsize)
{
    return filter_length >= 16 && filter_length <= 16384 &&
           ((size_t)filter_length + (size_t)filter_length / 32) * 2 * (size_t)realsize <= 160 * 1024;
}

// A matrix engine of up to BFIR_MIMO_MAXCHANNELS inputs and outputs: everything bfir_engine_create_matrix makes, with the
// wider cap, the partition counts in HBM and k_mac_mimo (mimo.hip) as its MAC.  Every refusal but BFIR_ERR_NO_DEVICE comes
// before the device is touched.
extern "C" bfir_engine *bfir_engine_create_mimo(int filter_length, int filter_blocks, int realsize, int n_inputs, int n_outputs,
                                                int in_format, int out_format, int device, int *err)
{
    int dummy;
    if (!err) err = &dummy;
    if (n_inputs < 1 || n_inputs > BFIR_MIMO_MAXCHANNELS || n_outputs < 1 || n_outputs > BFIR_MIMO_MAXCHANNELS) {
        bfir_logf("Number of channels (%d -> %d) exceeds limit (%d).", n_inputs, n_outputs, BFIR_MIMO_MAXCHANNELS);
        *err = BFIR_ERR_ARG; return nullptr;
    }
    // float frames only (no staging kernels, no dither)
    if (!fmt_is_native(in_format) || !fmt_is_native(out_format)) { *err = BFIR_ERR_UNSUPPORTED; return nullptr; }
    // a power of two outside the lengths bfir_engine_create takes; everything else is engine_create's to judge
    const bool pow2 = filter_length >= 1 && !(filter_length & (filter_length - 1));
    if (pow2 && (realsize == 4 || realsize == 8) && !length_supported(filter_length, realsize)) {
        bfir_logf("bfir engine: partition %d with realsize %d is outside a mimo engine's range.", filter_length, realsize);
        *err = BFIR_ERR_UNSUPPORTED; return nullptr;
    }
    return engine_create(1, filter_length, filter_blocks, realsize, n_inputs, n_outputs, true, in_format, out_format, 44100, 0,
                         device, err, 0, 0, false, BFIR_MIMO_MAXCHANNELS);
}

// Partitions past one workgroup's transform: 2^15 (fp64: 2^14) .. 2^20 samples, the lengths big_split takes.
extern "C" bfir_engine *bfir_engine_create_big(int filter_length, int filter_blocks, int realsize, int channels,
                                               int in_format, int out_format, int sampling_rate, int apply_dither,
                                               int device, int *err)
{
    int dummy, l1, l2;
    if (!err) err = &dummy;
    const bool pow2 = filter_length >= 1 && !(filter_length & (filter_length - 1));
    // everything else about the arguments is engine_create's to judge, in its order
    if (pow2 && (realsize == 4 || realsize == 8) && channels >= 1 && channels <= BFIR_MAXCHANNELS && filter_blocks >= 1) {
        if (!big_split(filter_length, realsize, &l1, &l2)) {
            if (length_supported(filter_length, realsize))
                bfir_logf("bfir engine: partition %d with realsize %d is one workgroup's transform: use bfir_engine_create.",
                          filter_length, realsize);
            else
                bfir_logf("bfir engine: partition %d is past the big engine's range (up to 1048576).", filter_length);
            *err = BFIR_ERR_UNSUPPORTED; return nullptr;
        }
        // one channel's filters and its smallest delay line (a chunk of one block) within the kernels' 32-bit element counts
        if ((2ull + (unsigned long long)filter_blocks) * 2ull * (unsigned long long)filter_length >= (1ull << 31)) {
            bfir_logf("bfir engine: %d partitions of %d are past the kernels' 32-bit indexing.", filter_blocks, filter_length);
            *err = BFIR_ERR_UNSUPPORTED; return nullptr;
        }
    }
    return engine_create(1, filter_length, filter_blocks, realsize, channels, channels, false, in_format, out_format,
                         sampling_rate, apply_dither, device, err, 0, 0, true);
}

// The time ring of tail[i] for head chunks of up to `chunk` blocks; the blocks still to be read are carried over.
static int alloc_zring(bfir_engine *e, int i, int chunk)
{
    bfir_engine *t = e->tail[i];
    const int zb = (chunk + e->lv_D[i] + e->lv_r[i] - 1) / e->lv_r[i] + 2;
    if (zb <= t->zblocks) return BFIR_OK;
    const size_t blk = (size_t)t->L * t->s;
    HIP_TRY(hipDeviceSynchronize());
    void **rings[2] = {&t->zring, &t->zring2};   // the second ring (a fade's new set) exists from the first fade on
    for (void **zr : rings) {
        if (zr == &t->zring2 && !t->zring2) continue;
        void *z = nullptr;
        HIP_TRY(hipMalloc(&z, (size_t)t->GCo * zb * blk));
        HIP_TRY(hipMemset(z, 0, (size_t)t->GCo * zb * blk));
        if (*zr) {
            const long long lo = std::max(t->z_from, t->z_next - t->zblocks);
            for (long long j = lo; j < t->z_next; j++)
                HIP_TRY(hipMemcpy2D((char *)z + (size_t)(j % zb) * blk, (size_t)zb * blk, (char *)*zr + (size_t)(j % t->zblocks) * blk,
                                    (size_t)t->zblocks * blk, blk, t->GCo, hipMemcpyDeviceToDevice));
            HIP_TRY(hipDeviceSynchronize());
            (void)hipFree(*zr);
        }
        *zr = z;
    }
    t->zblocks = zb;
    return BFIR_OK;
}

// The head (level 0) and its tails, for arguments that have passed the checks of the two entry points below.
// matrix: `channels` inputs and `channels_out` outputs at every level (bfir_engine_create_matrix_levels); else the two are equal
// max_channels: the channel cap of every level, as in engine_create (bfir_engine_create_mimo_levels: every level a mimo engine)
static bfir_engine *create_split(int filter_length, int n_levels, const int *blocks, const int *ratios, int realsize, int channels,
                                 int channels_out, bool matrix, int in_format, int out_format, int device, int *err,
                                 int max_channels = BFIR_MAXCHANNELS)
{
    bfir_engine *e = engine_create(1, filter_length, blocks[0], realsize, channels, channels_out, matrix, in_format, out_format,
                                   44100, 0, device, err, 1, 0, false, max_channels);
    if (!e) return nullptr;
    auto fail = [&](int code) { *err = code; bfir_engine_destroy(e); return (bfir_engine *)nullptr; };
    int r = 1, D = blocks[0];
    for (int k = 1; k < n_levels; k++) {
        r *= ratios[k];
        // ceil(D_k / r) + 1 slots on top: the blocks a fade's catch-up runs again (at most that many) and their history
        bfir_engine *t = engine_create(1, r * filter_length, blocks[k], realsize, channels, channels_out, matrix, in_format,
                                       out_format, 44100, 0, device, err, 2, (D + r - 1) / r + 1, false, max_channels);
        if (!t) return fail(*err);
        e->tail[k - 1] = t; e->lv_r[k - 1] = r; e->lv_D[k - 1] = D; e->n_tail = k;
        D += blocks[k] * r;
    }
    if (hipMalloc(&e->pbuf, (size_t)e->tail[e->n_tail - 1]->L * e->C * e->in_bytes) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_nup, hipEventDisableTiming) != hipSuccess)
        return fail(BFIR_ERR_HIP);
    for (int i = 0; i < e->n_tail; i++) if (alloc_zring(e, i, e->chunk) != BFIR_OK) return fail(BFIR_ERR_HIP);
    return e;
}

extern "C" bfir_engine *bfir_engine_create_nup(int filter_length, int head_blocks, int tail_ratio, int tail_blocks, int realsize,
                                               int channels, int in_format, int out_format, int device, int *err)
{
    int dummy;
    if (!err) err = &dummy;
    *err = BFIR_ERR_ARG;
    if (channels < 1 || channels > BFIR_MAXCHANNELS) {
        bfir_logf("Number of channels (%d) exceeds limit (%d).", channels, BFIR_MAXCHANNELS);
        return nullptr;
    }
    if (realsize != 4 && realsize != 8) { bfir_logf("Invalid real size %d.", realsize); return nullptr; }
    if (filter_length < 1 || (filter_length & (filter_length - 1))) { bfir_logf("Invalid length %d.", filter_length); return nullptr; }
    // the tail block a head block reads must be complete: head_blocks >= tail_ratio
    if (tail_ratio < 2 || (tail_ratio & (tail_ratio - 1)) || head_blocks < tail_ratio || tail_blocks < 1) return nullptr;
    *err = BFIR_ERR_UNSUPPORTED;
    if (!length_supported(filter_length, realsize) || (long long)tail_ratio * filter_length > 16384 ||
        !length_supported(tail_ratio * filter_length, realsize))
        return nullptr;
    // float frames only (no staging kernels, no dither)
    if (!fmt_is_native(in_format) || !fmt_is_native(out_format)) return nullptr;
    const int blocks[2] = {head_blocks, tail_blocks}, ratios[2] = {1, tail_ratio};
    bfir_engine *e = create_split(filter_length, 2, blocks, ratios, realsize, channels, channels, false, in_format, out_format, device, err);
    if (!e) return nullptr;
    bfir_logf("bfir engine: two levels, head %d x %d, tail %d x %d; back end %s.", e->L, e->B, e->tail[0]->L, e->tail[0]->B,
              e->pair ? "fused" : "general");
    return e;
}

// what bfir_engine_create_levels and _create_matrix_levels ask of their arguments, the channel counts apart; no device is touched
static int check_levels_args(int filter_length, int n_levels, const int *blocks, const int *ratios, int realsize, int in_format,
                             int out_format)
{
    if (realsize != 4 && realsize != 8) { bfir_logf("Invalid real size %d.", realsize); return BFIR_ERR_ARG; }
    if (filter_length < 1 || (filter_length & (filter_length - 1))) { bfir_logf("Invalid length %d.", filter_length); return BFIR_ERR_ARG; }
    if (n_levels < 2 || n_levels > BFIR_MAX_LEVELS || !blocks || !ratios || ratios[0] != 1) return BFIR_ERR_ARG;
    // L_k and D_k in samples, as doubles: exact at every size a transform could have, and no overflow at any other
    double Lk[BFIR_MAX_LEVELS], Dk = 0.0;
    for (int k = 0; k < n_levels; k++) {
        if (blocks[k] < 1) return BFIR_ERR_ARG;
        if (k > 0 && (ratios[k] < 2 || (ratios[k] & (ratios[k] - 1)))) return BFIR_ERR_ARG;
        Lk[k] = k == 0 ? (double)filter_length : Lk[k - 1] * ratios[k];
        // a block of level k is first read D_k samples after it began: it must be complete by then
        if (k > 0 && Dk < Lk[k]) return BFIR_ERR_ARG;
        Dk += blocks[k] * Lk[k];
    }
    for (int k = 0; k < n_levels; k++)
        if (Lk[k] > 16384.0 || !length_supported((int)Lk[k], realsize)) return BFIR_ERR_UNSUPPORTED;
    // float frames only (no staging kernels, no dither)
    if (!fmt_is_native(in_format) || !fmt_is_native(out_format)) return BFIR_ERR_UNSUPPORTED;
    return BFIR_OK;
}

extern "C" bfir_engine *bfir_engine_create_levels(int filter_length, int n_levels, const int *blocks, const int *ratios,
                                                  int realsize, int channels, int in_format, int out_format, int device, int *err)
{
    int dummy;
    if (!err) err = &dummy;
    *err = BFIR_ERR_ARG;
    if (channels < 1 || channels > BFIR_MAXCHANNELS) {
        bfir_logf("Number of channels (%d) exceeds limit (%d).", channels, BFIR_MAXCHANNELS);
        return nullptr;
    }
    *err = check_levels_args(filter_length, n_levels, blocks, ratios, realsize, in_format, out_format);
    if (*err != BFIR_OK) return nullptr;
    bfir_engine *e = create_split(filter_length, n_levels, blocks, ratios, realsize, channels, channels, false, in_format, out_format, device,
                                   err);
    if (!e) return nullptr;
    e->levels = true;
    char desc[160];
    int n = snprintf(desc, sizeof(desc), "%d x %d", e->L, e->B);
    for (int i = 0; i < e->n_tail; i++) n += snprintf(desc + n, sizeof(desc) - n, ", %d x %d", e->tail[i]->L, e->tail[i]->B);
    bfir_logf("bfir engine: %d levels, %s; back end %s.", n_levels, desc, e->pair ? "fused" : "general");
    return e;
}

extern "C" bfir_engine *bfir_engine_create_matrix_levels(int filter_length, int n_levels, const int *blocks, const int *ratios,
                                                         int realsize, int n_inputs, int n_outputs, int in_format, int out_format,
                                                         int device, int *err)
{
    int dummy;
    if (!err) err = &dummy;
    *err = BFIR_ERR_ARG;
    if (n_inputs < 1 || n_inputs > BFIR_MAXCHANNELS || n_outputs < 1 || n_outputs > BFIR_MAXCHANNELS) {
        bfir_logf("Number of channels (%d -> %d) exceeds limit (%d).", n_inputs, n_outputs, BFIR_MAXCHANNELS);
        return nullptr;
    }
    *err = check_levels_args(filter_length, n_levels, blocks, ratios, realsize, in_format, out_format);
    if (*err != BFIR_OK) return nullptr;
    bfir_engine *e = create_split(filter_length, n_levels, blocks, ratios, realsize, n_inputs, n_outputs, true, in_format, out_format,
                                  device, err);
    if (!e) return nullptr;
    e->mlevels = true;
    char desc[160];
    int n = snprintf(desc, sizeof(desc), "%d x %d", e->L, e->B);
    for (int i = 0; i < e->n_tail; i++) n += snprintf(desc + n, sizeof(desc) - n, ", %d x %d", e->tail[i]->L, e->tail[i]->B);
    bfir_logf("bfir engine: matrix %d -> %d, %d levels, %s; back end %s.", e->C, e->Co, n_levels, desc,
              e->back_fused ? "fused" : "general");
    return e;
}

// bfir_engine_create_matrix_levels with the channel cap of a mimo engine: the head and every tail are mimo engines, so a
// level's MAC is k_mac_mimo (two sets: k_wduo) where either count passes 8 and its partition counts are tables in HBM.
// Every refusal but BFIR_ERR_NO_DEVICE comes before the device is touched.
extern "C" bfir_engine *bfir_engine_create_mimo_levels(int filter_length, int n_levels, const int *blocks, const int *ratios,
                                                       int realsize, int n_inputs, int n_outputs, int in_format, int out_format,
                                                       int device, int *err)
{
    int dummy;
    if (!err) err = &dummy;
    *err = BFIR_ERR_ARG;
    if (n_inputs < 1 || n_inputs > BFIR_MIMO_MAXCHANNELS || n_outputs < 1 || n_outputs > BFIR_MIMO_MAXCHANNELS) {
        bfir_logf("Number of channels (%d -> %d) exceeds limit (%d).", n_inputs, n_outputs, BFIR_MIMO_MAXCHANNELS);
        return nullptr;
    }
    *err = check_levels_args(filter_length, n_levels, blocks, ratios, realsize, in_format, out_format);
    if (*err != BFIR_OK) return nullptr;
    bfir_engine *e = create_split(filter_length, n_levels, blocks, ratios, realsize, n_inputs, n_outputs, true, in_format, out_format,
                                  device, err, BFIR_MIMO_MAXCHANNELS);
    if (!e) return nullptr;
    e->mlevels = true;
    char desc[160];
    int n = snprintf(desc, sizeof(desc), "%d x %d", e->L, e->B);
    for (int i = 0; i < e->n_tail; i++) n += snprintf(desc + n, sizeof(desc) - n, ", %d x %d", e->tail[i]->L, e->tail[i]->B);
    bfir_logf("bfir engine: mimo %d -> %d, %d levels, %s; back end %s; MAC %s.", e->C, e->Co, n_levels, desc,
              e->back_fused ? "fused" : "general", e->mimo_mac ? "k_mac_mimo" : "k_mac_matrix");
    return e;
}

extern "C" void bfir_engine_destroy(bfir_engine *e)
{
    if (!e) return;
    (void)hipSetDevice(e->device);
    (void)hipDeviceSynchronize();
    for (bfir_engine *t : e->tail) if (t) bfir_engine_destroy(t);
    if (e->pbuf) (void)hipFree(e->pbuf);
    if (e->zring) (void)hipFree(e->zring);
    if (e->zring2) (void)hipFree(e->zring2);
    if (e->ev_nup) (void)hipEventDestroy(e->ev_nup);
    for (int side = 0; side < 2; side++) delay_free(e, side);
    if (e->ev_dly) (void)hipEventDestroy(e->ev_dly);
    if (e->ev_dly_done) (void)hipEventDestroy(e->ev_dly_done);
    free_work(e);
    fft_plan_destroy(&e->plan);
    fft_plan_destroy(&e->plan2);
    big_plan_destroy(&e->bplan);
    for (int st = 0; st < 2; st++) for (int i = 0; i < 2; i++) if (e->tails[st][i]) (void)hipFree(e->tails[st][i]);
    void *bufs[] = {e->H, e->saved[0], e->saved[1], e->d_nblk, e->d_of, e->d_bad, e->d_dither_tab, e->d_dither_state,
                    e->H2, e->d_nblk2, e->Yf[0], e->Yf[1], e->ft[0], e->ft[1], e->d_patch, e->bank, e->d_gather};
    for (void *b : bufs) if (b) (void)hipFree(b);
    for (auto &sp : e->spans) { (void)hipEventDestroy(sp.a); (void)hipEventDestroy(sp.b); }
    for (auto ev : e->ev_pool) (void)hipEventDestroy(ev);
    hipEvent_t events[] = {e->ev_entry, e->ev_fwd[0], e->ev_fwd[1], e->ev_mac[0], e->ev_mac[1], e->ev_inv[0], e->ev_inv[1],
                           e->ev_h2d[0], e->ev_h2d[1], e->ev_comp[0], e->ev_comp[1], e->ev_d2h[0], e->ev_d2h[1]};
    for (hipEvent_t ev : events) if (ev) (void)hipEventDestroy(ev);
    hipStream_t streams[] = {e->stream, e->s_front, e->s_mac, e->s_in, e->s_out};
    for (hipStream_t st : streams) if (st) (void)hipStreamDestroy(st);
    delete e;
}

extern "C" int bfir_engine_is_initialized(const bfir_engine *e)
{
    if (!e) return 0;
    for (char c : e->eng_init) if (!c) return 0;
    return 1;
}

extern "C" int bfir_engine_set_chunk(bfir_engine *e, int blocks_per_launch)
{
    if (!e || blocks_per_launch < 0) return BFIR_ERR_ARG;   // 0: automatic (the default)
    e->want_chunk = blocks_per_launch;
    return BFIR_OK;
}

// The planar transforms of an engine: one workgroup per transform, or a big engine's two passes.
static void queue_transform_fwd(const bfir_engine *e, const FwdArgs &a, hipStream_t s)
{
    if (e->big) launch_fwd_big(e->bplan, a, s); else launch_fwd(e->plan, a, s);
}
static void queue_transform_inv(const bfir_engine *e, const InvArgs &a, hipStream_t s)
{
    if (e->big) launch_inv_big(e->bplan, a, s); else launch_inv(e->plan, a, s);
}

// The filters of one set call as the rows of H they go to: the C channels of a diagonal engine, or the Co x C pairs of a
// matrix engine ([o C + i]).  A row without taps is an all-zero filter (a matrix engine: no path from input i to output o).
namespace {
struct FilterRows {
    std::vector<const void *> taps;
    std::vector<int> len;        // the tap count of every row
    int n_required = 0;          // a NULL among the first so many rows is BFIR_ERR_ARG: the n_coeffs of a diagonal engine
    explicit FilterRows(size_t n_rows = 0) : taps(n_rows), len(n_rows) {}
};
}

// coeffs[n] (n < n_coeffs) for channel n, all of `length` taps; the channels past n_coeffs get zeros
static FilterRows diagonal_rows(const bfir_engine *e, const void *const *coeffs, int n_coeffs, int length)
{
    FilterRows r((size_t)e->C);
    r.n_required = std::min(n_coeffs, e->C);                    // brutefir.cpp:190-193
    for (int n = 0; n < r.n_required; n++) r.taps[n] = coeffs[n];
    for (int &len : r.len) len = length;
    return r;
}

// coeffs[o n_in + i], NULL = no path; every filter of its own length (a NULL has none), or all of `length` taps
static FilterRows matrix_rows(const bfir_engine *e, const void *const *coeffs, const int *lengths, int length)
{
    const int P = e->Co * e->C;                                 // filters, [o][i]
    FilterRows r((size_t)P);
    for (int n = 0; n < P; n++) {
        r.taps[n] = coeffs[n];
        r.len[n] = !lengths ? length : coeffs[n] ? lengths[n] : 0;
    }
    return r;
}

// coeff::preprocess_coeff's finite check over the first max_taps taps of every row (what the call loads), scaled in
// working precision (fftw_convolver.cpp:491,507).  Every entry point calls it once, before its first upload: a NaN / Inf
// tap anywhere is refused before anything is uploaded at any level.
static int check_rows(const bfir_engine *e, const FilterRows &r, size_t max_taps, double scale)
{
    for (int n = 0; n < (int)r.taps.size(); n++) {
        if (!r.taps[n]) { if (n < r.n_required) return BFIR_ERR_ARG; continue; }
        const size_t cnt = std::min((size_t)r.len[n], max_taps);
        bool finite = true;
        if (e->s == 4) {
            const float *src = (const float *)r.taps[n];
            const float sc = (float)scale;
            for (size_t i = 0; i < cnt; i++) finite &= std::isfinite((double)(src[i] * sc));
        } else {
            const double *src = (const double *)r.taps[n];
            for (size_t i = 0; i < cnt; i++) finite &= std::isfinite(src[i] * scale);
        }
        if (!finite) {
            bfir_logf("NaN or Inf value among coefficients.");
            if (e->matrix) bfir_logf("Error preprocessing coefficient %d (output %d, input %d)", n, n / e->C, n % e->C);
            else bfir_logf("Error preprocessing coefficient %d", n);
            return BFIR_ERR_COEFF;
        }
    }
    return BFIR_OK;
}

// convolver_coeffs2cbuf for the rows of a call that has passed check_rows: row n goes to row row0 + n of Hdst, nb
// partitions each.  Hdst: the filter buffer that takes them, H or (a fade's second set) H2.
static int load_filters(bfir_engine *e, void *Hdst, int row0, const FilterRows &r, int nb, double scale)
{
    const int n_rows = (int)r.taps.size();
    const size_t taps_pad = (size_t)nb * e->L;
    const size_t cb = cbuf_bytes(e);
    // zero padded impulse per filter; a block past the end is all zero (coeff.cpp:315-339)
    std::vector<char> host((size_t)n_rows * taps_pad * e->s, 0);
    for (int n = 0; n < n_rows; n++)
        if (r.taps[n] && r.len[n] > 0)
            memcpy(host.data() + (size_t)n * taps_pad * e->s, r.taps[n], std::min((size_t)r.len[n], taps_pad) * e->s);
    void *d_taps = nullptr;
    void *rows = (char *)Hdst + (size_t)row0 * e->B * cb;
    HIP_TRY(hipMalloc(&d_taps, host.size()));
    HIP_TRY(hipMemcpyAsync(d_taps, host.data(), host.size(), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemsetAsync(rows, 0, (size_t)n_rows * e->B * cb, e->stream));
    FwdArgs fa;                                                 // one "channel" per filter
    // window of block b = [L zeros | taps b*L .. b*L+L)
    fa.src = d_taps; fa.src_ch_stride = (long)taps_pad;
    fa.prev = nullptr; fa.prev_ch_stride = 0;
    fa.dst = rows; fa.dst_ch_stride = (long)e->B * e->N;
    fa.ring = e->B; fa.base_slot = 0;
    fa.n_t = nb; fa.n_ch = n_rows;
    fa.load_scale = scale;
    fa.out_scale = 1.0 / (double)e->N;                          // fftw_convolver.cpp:520
    fa.zero_first_half = 1;
    fa.interleaved = e->ilv;
    queue_transform_fwd(e, fa, e->stream);
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipFree(d_taps));
    HIP_TRY(hipGetLastError());
    return BFIR_OK;
}

// A host table into the device table a kernel reads it from (d_gather, d_patch of any level), which grows where it is too
// small.  The device is idle.
static int upload_table(int *&d, size_t &cap, const std::vector<int> &tab)
{
    if (tab.size() > cap) {
        if (d) (void)hipFree(d);
        d = nullptr; cap = 0;
        HIP_TRY(hipMalloc((void **)&d, sizeof(int) * tab.size()));
        cap = tab.size();
    }
    HIP_TRY(hipMemcpy(d, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice));
    return BFIR_OK;
}

// The partition counts of a level (a uniform engine: itself), new on the host in nblk or (second: a fade's new set) nblk2, to
// where a kernel reads them: the C channels from row0 on of a diagonal engine, the whole table of a mimo engine (k_mac_mimo,
// k_wduo); the MAC of any other matrix engine takes them by value (MatArgs.nblk).  The device is idle.
static int upload_counts(bfir_engine *l, bool second, int row0 = 0)
{
    const std::vector<int> &nb = second ? l->nblk2 : l->nblk;
    int *d = second ? l->d_nblk2 : l->d_nblk;
    if (!l->matrix) HIP_TRY(hipMemcpy(d + row0, nb.data() + row0, sizeof(int) * l->C, hipMemcpyHostToDevice));
    else if (l->mimo) HIP_TRY(hipMemcpy(d, nb.data(), sizeof(int) * nb.size(), hipMemcpyHostToDevice));
    return BFIR_OK;
}

// the C channels of one engine
extern "C" int bfir_engine_set_coeff_at(bfir_engine *e, int engine_index, const void *const *coeffs,
                                        int n_coeffs, int length, int coeff_blocks, double scale)
{
    if (!e || engine_index < 0 || engine_index >= e->n_eng || !coeffs || length < 0 || coeff_blocks < 1)
        return BFIR_ERR_ARG;
    if (e->matrix) return BFIR_ERR_UNSUPPORTED;                 // bfir_engine_set_coeff_matrix
    if (e->nup) return BFIR_ERR_UNSUPPORTED;                    // bfir_engine_set_coeff_nup
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    e->fade_len = e->fade_pos = 0;                              // a plain change during a fade cancels it: a hard cut, as ever
    e->eng_init[engine_index] = 0;                              // free_coeff(), brutefir.cpp:188
    const int nb = std::min(coeff_blocks, e->B);                // run() never looks past B blocks
    const int gc0 = engine_index * e->C;
    const FilterRows rows = diagonal_rows(e, coeffs, n_coeffs, length);
    int rc = check_rows(e, rows, (size_t)nb * e->L, scale);
    if (rc == BFIR_OK) rc = load_filters(e, e->H, gc0, rows, nb, scale);
    if (rc != BFIR_OK) return rc;
    for (int n = 0; n < e->C; n++) e->nblk[gc0 + n] = nb;
    rc = upload_counts(e, false, gc0);
    if (rc != BFIR_OK) return rc;
    e->eng_init[engine_index] = 1;
    return BFIR_OK;
}

extern "C" int bfir_engine_set_coeff(bfir_engine *e, const void *const *coeffs, int n_coeffs,
                                     int length, int coeff_blocks, double scale)
{
    return bfir_engine_set_coeff_at(e, 0, coeffs, n_coeffs, length, coeff_blocks, scale);
}

static void lfade_finish(bfir_engine *e, bool take_new);

// Level i + 1 of a split engine gets taps it did not have: it starts (again) with its next block that begins.  Its signal
// state is cleared, the blocks it did not compute read as zero, and its first blocks lack the input from before (a
// transient like the one of a new engine).  Output queued before it stopped is still in the ring.
static int level_start(bfir_engine *e, int i)
{
    bfir_engine *t = e->tail[i];
    const int r = e->lv_r[i];
    const size_t blk = (size_t)t->L * t->s;
    const long long j0 = (long long)((e->blockcounter + r - 1) / r);
    HIP_TRY(hipMemset(t->X, 0, (size_t)t->GC * t->ring * cbuf_bytes(t)));
    for (int st = 0; st < 2; st++) for (int h = 0; h < 2; h++) HIP_TRY(hipMemset(t->tails[st][h], 0, (size_t)t->L * t->C * t->in_bytes));
    const long long oldest = std::max(0ll, ((long long)e->blockcounter - e->lv_D[i]) / r);   // the oldest block of the level still to be read
    if (t->z_next <= oldest || t->z_next == t->z_from) t->z_from = j0;
    else for (long long j = t->z_next; j < j0; j++)   // fewer than D_k / L_k + 2 <= zblocks of them
        HIP_TRY(hipMemset2D((char *)t->zring + (size_t)(j % t->zblocks) * blk, (size_t)t->zblocks * blk, 0, blk, t->GCo));
    t->z_next = j0;
    t->blockcounter = 0; t->curbuf = 0;
    return BFIR_OK;
}

// Does every input of a matrix engine feed some output?  It does if any filter of its column has taps on any level:
// count(k, n) is the partition count of filter n = o C + i on level k (a uniform engine has the one level).
template <class Count> static bool every_input_read(const bfir_engine *e, Count count)
{
    for (int i = 0; i < e->C; i++) {
        bool read = false;
        for (int o = 0; o < e->Co; o++)
            for (int k = 0; k <= e->n_tail; k++) read = read || count(k, o * e->C + i) > 0;
        if (!read) return false;
    }
    return true;
}

// a pair-capable matrix engine between its two paths: same delay-line layout and history bookkeeping on both, the next
// chunk just takes the other
static void matrix_take_path(bfir_engine *e, bool pair)
{
    if (e->pair != pair)
        bfir_logf("bfir matrix engine: %s: path=%s from the next block on.",
                  pair ? "every input feeds an output" : "an input feeds no output", pair ? "pair" : "direct");
    e->pair = pair; e->direct = !pair;
}

// The partition counts of a uniform matrix engine's active set are new in e->nblk and where its MAC reads them (the device is
// idle): the path, and the engine has its coefficients.
static int matrix_counts_set(bfir_engine *e)
{
    if (e->pair_cap) matrix_take_path(e, every_input_read(e, [&](int, int n) { return e->nblk[n]; }));
    e->eng_init[0] = 1;
    return BFIR_OK;
}

// Where the rows of a set call on a uniform engine come from (the SplitSource of the uniform kinds): host taps, all loaded with
// nb partitions; entries of the engine's bank (ent[j]: the entry of row j of the call, -1: none); or weighted sums of entries
// (k_bank_mix's records, coeff_tables::mix_records).  set_coeff_uniform asks the source for its finite check, the partition
// count of every row and to write its rows, and is otherwise the same for all three.
namespace {
struct UniformSource {
    const FilterRows *rows = nullptr; double scale = 1.0; int nb = 0;
    const std::vector<int> *ent = nullptr;
    const std::vector<int> *mix = nullptr;
};
}

static UniformSource uniform_taps(const bfir_engine *e, const FilterRows &rows, double scale, int coeff_blocks)
{
    UniformSource s;
    s.rows = &rows; s.scale = scale; s.nb = std::min(coeff_blocks, e->B);   // run() never looks past B blocks
    return s;
}

static int set_coeff_uniform(bfir_engine *e, const UniformSource &src, const std::vector<int> *list, int fade_blocks,
                             bool check_first = true);

// the n_out x n_in filters of a matrix engine: coeffs[o n_in + i], NULL = no path from input i to output o
extern "C" int bfir_engine_set_coeff_matrix(bfir_engine *e, const void *const *coeffs, int length, int coeff_blocks,
                                            double scale)
{
    if (!e) return BFIR_ERR_ARG;
    if (!e->matrix || e->mlevels) return BFIR_ERR_UNSUPPORTED;   // bfir_engine_set_coeff_matrix_levels
    if (!coeffs || length < 0 || coeff_blocks < 1) return BFIR_ERR_ARG;
    const FilterRows rows = matrix_rows(e, coeffs, nullptr, length);
    // as bfir_engine_set_coeff_at: a NaN / Inf tap is refused on the idle device, behind free_coeff()
    return set_coeff_uniform(e, uniform_taps(e, rows, scale, coeff_blocks), nullptr, -1, false);
}

// The rows of a set call on a split engine, cut at every D_k: level k (0: the head) gets taps [D_k, D_(k+1)) of every row
// that reaches past D_k.  Host arithmetic alone: neither the device nor the engine's state is touched.
namespace {
struct LevelSplit {
    struct Level {
        FilterRows rows;         // the part of every row that falls into the level (a row without taps there: none)
        std::vector<int> nb;     // the row's partitions there
        int nb_max = 0;          // 0: the set does not reach the level
    } lv[BFIR_MAX_LEVELS];
};
}

// A filter of a matrix engine has ceil(len / L_k) partitions on level k, its own count (0: skipped on that level, never
// multiplied by zero).  The channels of a diagonal engine all get the level's count, the zero rows past n_coeffs too, and
// on the head at least one partition.
static LevelSplit split_rows(const bfir_engine *e, const FilterRows &r)
{
    LevelSplit sp;
    const size_t n_rows = r.taps.size();
    for (int k = 0; k <= e->n_tail; k++) {
        const bfir_engine *l = level(e, k);
        LevelSplit::Level &s = sp.lv[k];
        const long long D = k == 0 ? 0 : (long long)e->lv_D[k - 1] * e->L;
        s.rows = FilterRows(n_rows); s.nb.assign(n_rows, 0);
        for (size_t n = 0; n < n_rows; n++) {
            const int len = (int)std::max(0ll, std::min((long long)r.len[n] - D, (long long)l->B * l->L));
            s.rows.len[n] = len;
            if (len > 0 && r.taps[n]) s.rows.taps[n] = (const char *)r.taps[n] + (size_t)D * e->s;
            s.nb[n] = (len + l->L - 1) / l->L;
            s.nb_max = std::max(s.nb_max, s.nb[n]);
        }
        if (!e->matrix) { s.nb_max = std::max(s.nb_max, k == 0 ? 1 : 0); s.nb.assign(n_rows, s.nb_max); }
    }
    return sp;
}

// what the set calls of a split engine ask of the lengths: none negative, none past the taps its levels hold
static int check_split_lengths(const bfir_engine *e, const FilterRows &r)
{
    long long cap = 0;
    for (int k = 0; k <= e->n_tail; k++) cap += (long long)level(e, k)->B * level(e, k)->L;
    for (int len : r.len) if (len < 0 || (long long)len > cap) return BFIR_ERR_ARG;
    return BFIR_OK;
}

// The partition counts of a split engine's active set are new on every level (sp: nb and nb_max; the device is idle): a
// level the set newly reaches starts, one it no longer reaches stops, a matrix engine takes its path, and the engine has
// its coefficients.
static int split_counts_set(bfir_engine *e, const LevelSplit &sp)
{
    for (int i = 0; i < e->n_tail; i++) {
        const bool active = sp.lv[i + 1].nb_max > 0;
        if (active && !e->lv_active[i]) { const int rc = level_start(e, i); if (rc != BFIR_OK) return rc; }
        e->lv_active[i] = active;
        e->tail[i]->eng_init[0] = 1;
    }
    if (e->matrix) {
        // An input is read if any filter of its column has taps on any level; while one is not, no level pairs channels (a
        // pair is ONE transform: a NaN on the unread input would reach the spectra of its partner)
        const bool all_read = every_input_read(e, [&](int k, int n) { return sp.lv[k].nb[n]; });
        for (int i = 0; i < e->n_tail; i++) if (e->tail[i]->pair_cap) matrix_take_path(e->tail[i], all_read);
        // While no level beyond the head has taps the engine IS bfir_engine_create_matrix(L, blocks[0], ...) and takes its path,
        // which pairs channels only with an even count on both sides: so it gives that engine's bytes
        bool any_tail = false;
        for (int i = 0; i < e->n_tail; i++) any_tail = any_tail || e->lv_active[i];
        if (e->pair_cap) {
            if (all_read && !any_tail && (e->Co & 1)) {
                if (e->pair) bfir_logf("bfir matrix engine: no level beyond the head has taps: path=direct from the next block on.");
                e->pair = false; e->direct = true;
            } else matrix_take_path(e, all_read);
        }
    }
    e->eng_init[0] = 1;
    return BFIR_OK;
}

// Where the rows of a set call on a split engine come from: host taps (rows, scale), which every level uploads and
// transforms; entries of the engine's bank (bfir_engine_levels_bank_create; ent[j]: the entry of row j, -1: none), which
// every level holds transformed already; or weighted sums of entries (mix: k_lbank_mix's records, mix_nb: the rows' counts,
// [row][BFIR_MAX_LEVELS], both of coeff_tables::level_mix_records).  set_coeff_split, set_coeff_split_fade and set_pairs_split
// ask the source for its checks and its split and are otherwise the same for all three: where taps are loaded level by
// level, entries and mixes are marked for ONE launch behind the loop (lbank_gather, lbank_mix_gather).
namespace {
struct SplitSource {
    const FilterRows *rows = nullptr; double scale = 1.0;
    const std::vector<int> *ent = nullptr;
    const std::vector<int> *mix = nullptr, *mix_nb = nullptr;
};
}

static SplitSource taps_source(const FilterRows &rows, double scale) { SplitSource s; s.rows = &rows; s.scale = scale; return s; }
static int source_check_lengths(const bfir_engine *e, const SplitSource &src) { return src.rows ? check_split_lengths(e, *src.rows) : BFIR_OK; }
static int source_check_rows(const bfir_engine *e, const SplitSource &src) { return src.rows ? check_rows(e, *src.rows, SIZE_MAX, src.scale) : BFIR_OK; }

// the rows of the call
static size_t source_size(const SplitSource &src)
{
    return src.rows ? src.rows->taps.size() : src.ent ? src.ent->size() : src.mix_nb->size() / BFIR_MAX_LEVELS;
}

// The split of a source.  Bank entries: counts only, what the host table holds since the entry was loaded; no FilterRows.
// Mixes: the counts level_mix_records found, the largest of every row's live terms per level.
static LevelSplit source_split(const bfir_engine *e, const SplitSource &src)
{
    if (src.rows) return split_rows(e, *src.rows);
    LevelSplit sp;
    const size_t n = source_size(src);
    for (int k = 0; k <= e->n_tail; k++) {
        LevelSplit::Level &s = sp.lv[k];
        s.nb.assign(n, 0);
        for (size_t j = 0; j < n; j++) {
            const int en = src.ent ? (*src.ent)[j] : -1;
            s.nb[j] = src.mix_nb ? (*src.mix_nb)[j * BFIR_MAX_LEVELS + k] : en < 0 ? 0 : e->lbank_nb[(size_t)en * BFIR_MAX_LEVELS + k];
            s.nb_max = std::max(s.nb_max, s.nb[j]);
        }
    }
    return sp;
}

static_assert(BFIR_LBANK_LEVELS == BFIR_MAX_LEVELS, "k_lbank_gather takes one descriptor per level");

// k_lbank_gather's level descriptors: level k of the bank into dst[k] (H or H2 of the level; null: not part of the launch)
static LBankArgs lbank_args(const bfir_engine *e, void *const (&dst)[BFIR_MAX_LEVELS])
{
    LBankArgs a = {};
    for (int k = 0; k <= e->n_tail; k++) {
        const bfir_engine *l = level(e, k);
        a.lv[k].bank = l->bank; a.lv[k].dst = dst[k];
        a.lv[k].part_bytes = cbuf_bytes(l); a.lv[k].row_bytes = (unsigned long long)l->B * a.lv[k].part_bytes;
    }
    return a;
}

// Row j of the call (destination row (*list)[j], or j: the whole matrix) from bank entry ent[j], on every level with a
// destination: the table goes up, ONE gather for all levels is queued on e->stream behind whatever the call has queued
// there, and the host waits for it.  The device is idle; the counts are the caller's (the source's split).
static int lbank_gather(bfir_engine *e, void *const (&dst)[BFIR_MAX_LEVELS], const std::vector<int> &ent, const std::vector<int> *list)
{
    const int rc = upload_table(e->d_gather, e->gather_ints, coeff_tables::level_gather_table(list, ent, e->lbank_nb, e->n_tail + 1));
    if (rc != BFIR_OK) return rc;
    LBankArgs a = lbank_args(e, dst);
    a.tab = e->d_gather; a.n_rows = (int)ent.size();
    if (launch_lbank_gather(a, e->stream) != 0) return BFIR_ERR_UNSUPPORTED;   // checked by the entry point: not reached
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipGetLastError());
    return BFIR_OK;
}

static_assert(coeff_tables::kLevelMixRec == BFIR_LBANK_MIX_REC && coeff_tables::kLevelMixTerm == BFIR_LBANK_MIX_TERM,
              "coeff_tables::level_mix_records writes k_lbank_mix's records");

// k_lbank_mix's arguments: lbank_args' descriptors
static LBankMixArgs lbank_mix_args(const bfir_engine *e, void *const (&dst)[BFIR_MAX_LEVELS])
{
    const LBankArgs g = lbank_args(e, dst);
    LBankMixArgs a = {};
    for (int k = 0; k < BFIR_LBANK_LEVELS; k++) a.lv[k] = g.lv[k];
    return a;
}

// The same for a mix call: the records (their destination rows are in them) go up, ONE k_lbank_mix launch for all levels is
// queued on e->stream, and the host waits for it.
static int lbank_mix_gather(bfir_engine *e, void *const (&dst)[BFIR_MAX_LEVELS], const std::vector<int> &rec)
{
    const int rc = upload_table(e->d_gather, e->gather_ints, rec);
    if (rc != BFIR_OK) return rc;
    LBankMixArgs a = lbank_mix_args(e, dst);
    a.tab = e->d_gather; a.n_rows = (int)(rec.size() / BFIR_LBANK_MIX_REC);
    if (launch_lbank_mix(a, e->s, e->stream) != 0) return BFIR_ERR_UNSUPPORTED;   // checked by the entry point: not reached
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipGetLastError());
    return BFIR_OK;
}

// the one launch of a source without taps
static int source_gather(bfir_engine *e, void *const (&dst)[BFIR_MAX_LEVELS], const SplitSource &src, const std::vector<int> *list)
{
    return src.mix ? lbank_mix_gather(e, dst, *src.mix) : lbank_gather(e, dst, *src.ent, list);
}

// The filters of a two-level, multi-level or multi-level matrix engine, split at every D_k: taps [0, D_1) to the head,
// [D_k, D_(k+1)) to level k.  Mid-stream every delay line is kept: the head takes the new filters from the next block,
// level k from its next block that completes; what a level has already put into its time ring still plays.
static int set_coeff_split(bfir_engine *e, const SplitSource &src)
{
    int rc = source_check_lengths(e, src);
    if (rc != BFIR_OK) return rc;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    if (e->fade_len > 0) { e->fade_len = e->fade_pos = 0; e->fade_patch = false; lfade_finish(e, false); }   // a plain change during a fade cancels it: a hard cut
    e->eng_init[0] = 0;
    rc = source_check_rows(e, src);
    if (rc != BFIR_OK) return rc;
    const LevelSplit sp = source_split(e, src);
    void *gather[BFIR_MAX_LEVELS] = {};
    // the head, then level after level: the part of every filter that falls into the level and its partitions there
    for (int k = 0; k <= e->n_tail; k++) {
        bfir_engine *l = level(e, k);
        const LevelSplit::Level &s = sp.lv[k];
        if (s.nb_max > 0) {   // a level on which no filter has taps does no work at all (a matrix head: its MAC stores zeros)
            if (!src.rows) gather[k] = l->H;
            else rc = load_filters(l, l->H, 0, s.rows, s.nb_max, src.scale);
            if (rc != BFIR_OK) return rc;
        }
        l->nblk = s.nb;
        rc = upload_counts(l, false);
        if (rc != BFIR_OK) return rc;
    }
    if (!src.rows) { rc = source_gather(e, gather, src, nullptr); if (rc != BFIR_OK) return rc; }
    return split_counts_set(e, sp);
}

extern "C" int bfir_engine_set_coeff_nup(bfir_engine *e, const void *const *coeffs, int n_coeffs, int length, double scale)
{
    if (!e) return BFIR_ERR_ARG;
    if (!e->nup || e->levels || e->mlevels) return BFIR_ERR_UNSUPPORTED;
    if (!coeffs || n_coeffs < 0) return BFIR_ERR_ARG;
    const FilterRows rows = diagonal_rows(e, coeffs, n_coeffs, length);
    return set_coeff_split(e, taps_source(rows, scale));
}

extern "C" int bfir_engine_set_coeff_levels(bfir_engine *e, const void *const *coeffs, int n_coeffs, int length, double scale)
{
    if (!e) return BFIR_ERR_ARG;
    if (!e->levels) return BFIR_ERR_UNSUPPORTED;
    if (!coeffs || n_coeffs < 0) return BFIR_ERR_ARG;
    const FilterRows rows = diagonal_rows(e, coeffs, n_coeffs, length);
    return set_coeff_split(e, taps_source(rows, scale));
}

// The n_out x n_in filters of a multi-level matrix engine, each of its own length: coeffs[o n_in + i], NULL = no path
extern "C" int bfir_engine_set_coeff_matrix_levels(bfir_engine *e, const void *const *coeffs, const int *lengths, double scale)
{
    if (!e) return BFIR_ERR_ARG;
    if (!e->mlevels) return BFIR_ERR_UNSUPPORTED;
    if (!coeffs || !lengths) return BFIR_ERR_ARG;
    const FilterRows rows = matrix_rows(e, coeffs, lengths, 0);
    return set_coeff_split(e, taps_source(rows, scale));
}

// ---------------------------------------------------------------------------
// crossfaded coefficient change: the engine-level form of fftw_convolver::convolver_crossfade_inplace
// (brutefir/fftw_convolver.cpp:275-321), stretched over fade_blocks blocks
// ---------------------------------------------------------------------------
// a tail level of a fading two- or multi-level engine takes the new set (its H2 becomes H) ...
static void tail_swap_sets(bfir_engine *t)
{
    std::swap(t->H, t->H2);
    std::swap(t->d_nblk, t->d_nblk2);
    std::swap(t->nblk, t->nblk2);
}

// ... and the fade of such an engine ends, for its tails.  take_new (the head has queued its last fade block, or
// bfir_engine_reset): every level is on the new set, the second ring of every level becomes its ring, and a level the new
// set does not reach stops as bfir_engine_set_coeff_levels would stop it.  Without (a plain set_coeff ends the fade, a hard
// cut): a level keeps the ring that holds its output up to z_next -- the second one if it has passed its last old block.
static void lfade_finish(bfir_engine *e, bool take_new)
{
    for (int i = 0; i < e->n_tail; i++) {
        bfir_engine *t = e->tail[i];
        if (take_new && e->mlevels && t->pair_cap) matrix_take_path(t, t->pair_new);   // after the fade the new set decides
        t->fade_patch = false;
        if (!t->lf_mode) continue;
        if (take_new && t->lf_mode == 1) tail_swap_sets(t);
        if (take_new || t->lf_mode == 2) std::swap(t->zring, t->zring2);
        if (take_new && t->lf_stop) e->lv_active[i] = false;
        t->lf_mode = 0; t->lf_stop = false;
    }
}

// the old set gives way to the new one: H2 becomes H (the buffer that was H is the next fade's H2)
static void fade_swap_sets(bfir_engine *e)
{
    std::swap(e->H, e->H2);
    std::swap(e->d_nblk, e->d_nblk2);
    std::swap(e->nblk, e->nblk2);
    e->fade_len = e->fade_pos = 0;
    e->fade_patch = false;
    if (e->matrix && e->pair_cap) matrix_take_path(e, e->pair_new);
    if (e->nup) lfade_finish(e, true);
}

// what every fade call asks of fade_blocks and of the engine's state
static int check_fade_args(const bfir_engine *e, int fade_blocks)
{
    // m = 0 .. K L - 1 must be exact as a float (fftw_convolver.cpp:302 multiplies by (float)n)
    if (fade_blocks < 1 || (long long)fade_blocks * e->L > (1ll << 24)) return BFIR_ERR_ARG;
    if (!bfir_engine_is_initialized(e) || e->fade_len > 0) return BFIR_ERR_STATE;
    return BFIR_OK;
}

// What a fade needs beside the active set, allocated at the first fade: on every level (a uniform engine: itself) H2 for
// n_rows filters with its counts, on a tail the second ring; and which back end the fade takes.  The device is idle.
static int fade_prepare(bfir_engine *e, int n_rows)
{
    for (int k = 0; k <= e->n_tail; k++) {
        bfir_engine *l = level(e, k);
        if (l->H2) continue;
        HIP_TRY(hipMalloc(&l->H2, (size_t)n_rows * l->B * cbuf_bytes(l)));
        // not read by k_mac_matrix; swapped with d_nblk.  A mimo engine: the second table of k_mac_mimo
        HIP_TRY(hipMalloc((void **)&l->d_nblk2, sizeof(int) * (l->mimo ? (size_t)n_rows : (size_t)l->GC)));
    }
    for (int i = 0; i < e->n_tail; i++) {
        bfir_engine *t = e->tail[i];
        if (!t->zring2) HIP_TRY(hipMalloc(&t->zring2, (size_t)t->GCo * t->zblocks * t->L * t->s));
    }
    e->fade_fused = e->s == 4 && e->ilv && e->out_fmt == BFIR_SAMPLE_FORMAT_FLOAT_LE && pair_supported(e->L);
    // direct / staging engines (a split engine: an odd channel count) have none yet
    if (e->fade_fused && !e->plan2.tw && fft_plan_create(&e->plan2, 2 * e->L, 4) != 0) return BFIR_ERR_HIP;
    return BFIR_OK;
}

// the fade is the next fade_blocks blocks the engine processes
static void fade_begin(bfir_engine *e, int fade_blocks)
{
    e->fade_f = (float)(1.0 / (double)(float)(fade_blocks * e->L - 1));
    e->fade_d = 1.0 / (double)(fade_blocks * e->L - 1);
    e->fade_len = fade_blocks; e->fade_pos = 0;
    e->fade_patch = false;                                      // a pairs fade sets it behind this call
}

// a uniform engine, diagonal (coeffs[n] for channel n < n_coeffs) or matrix (coeffs[o n_in + i], NULL = no path)
static int set_coeff_fade(bfir_engine *e, const void *const *coeffs, int n_coeffs, int length, int coeff_blocks, double scale,
                          int fade_blocks)
{
    if (e->n_eng > 1 || e->d_dither_tab) return BFIR_ERR_UNSUPPORTED;   // batches; HP-TPDF dither (a recursion over the output samples)
    if (e->nup) return BFIR_ERR_UNSUPPORTED;                            // two-level engines do not fade
    if (!coeffs || length < 0 || coeff_blocks < 1) return BFIR_ERR_ARG;
    const int rc = check_fade_args(e, fade_blocks);
    if (rc != BFIR_OK) return rc;
    const FilterRows rows = e->matrix ? matrix_rows(e, coeffs, nullptr, length) : diagonal_rows(e, coeffs, n_coeffs, length);
    return set_coeff_uniform(e, uniform_taps(e, rows, scale, coeff_blocks), nullptr, fade_blocks);
}

extern "C" int bfir_engine_set_coeff_fade(bfir_engine *e, const void *const *coeffs, int n_coeffs, int length,
                                          int coeff_blocks, double scale, int fade_blocks)
{
    if (!e) return BFIR_ERR_ARG;
    if (e->matrix) return BFIR_ERR_UNSUPPORTED;                 // bfir_engine_set_coeff_matrix_fade
    if (n_coeffs < 0) return BFIR_ERR_ARG;
    return set_coeff_fade(e, coeffs, n_coeffs, length, coeff_blocks, scale, fade_blocks);
}

extern "C" int bfir_engine_set_coeff_matrix_fade(bfir_engine *e, const void *const *coeffs, int length, int coeff_blocks,
                                                 double scale, int fade_blocks)
{
    if (!e) return BFIR_ERR_ARG;
    if (!e->matrix || e->mlevels) return BFIR_ERR_UNSUPPORTED;
    return set_coeff_fade(e, coeffs, 0, length, coeff_blocks, scale, fade_blocks);
}

// ---------------------------------------------------------------------------
// a list of (output, input) pairs of a uniform matrix or mimo engine replaced: bfir_engine_set_coeff_matrix_pairs, _fade
// ---------------------------------------------------------------------------
namespace {
struct PairList {
    FilterRows rows;             // the listed filters in list order, all of `length` taps (NULL: the path is removed)
    std::vector<int> row;        // where each goes: filter o C + i
};
}

// What every pairs call with taps asks of its list; host arithmetic alone.  Every listed filter has its own lengths[k] taps,
// or (lengths == nullptr) all have `length`; a NULL has none.
static int pairs_list(const bfir_engine *e, int n_pairs, const int *outputs, const int *inputs, const void *const *coeffs,
                      const int *lengths, int length, PairList &pl)
{
    if (!outputs || !inputs || !coeffs || n_pairs < 1) return BFIR_ERR_ARG;
    const int rc = coeff_tables::list_rows(e->Co, e->C, n_pairs, outputs, inputs, pl.row);
    if (rc != BFIR_OK) return rc;
    pl.rows = FilterRows((size_t)n_pairs);
    for (int k = 0; k < n_pairs; k++) {
        pl.rows.taps[k] = coeffs[k];
        pl.rows.len[k] = !coeffs[k] ? 0 : lengths ? lengths[k] : length;
    }
    return BFIR_OK;
}

// The listed rows of a level (a uniform engine: itself) into Hdst (H, or H2 holding a copy of H): row j of `rows` with nb[j]
// partitions, as load_filters gives them, to row list[j], on the stream that owns every write to the level's store.  A row
// without partitions (a removed path; a filter that does not reach the level) is cleared, as a whole-matrix call leaves the
// row of a NULL.  The spectrum of a row does not depend on the rows transformed with it (one workgroup per row and
// partition, k_fwd's planar form), so row by row gives the bytes of the whole matrix in one call.
static int load_listed_rows(bfir_engine *l, void *Hdst, const FilterRows &rows, const std::vector<int> &nb,
                            const std::vector<int> &list, double scale)
{
    const size_t row_bytes = (size_t)l->B * cbuf_bytes(l);
    for (size_t j = 0; j < list.size(); j++) {
        if (nb[j] == 0) {
            HIP_TRY(hipMemsetAsync((char *)Hdst + (size_t)list[j] * row_bytes, 0, row_bytes, l->stream));
            continue;
        }
        FilterRows one(1);
        one.taps[0] = rows.taps[j]; one.len[0] = rows.len[j];
        const int rc = load_filters(l, Hdst, list[j], one, nb[j], scale);
        if (rc != BFIR_OK) return rc;
    }
    HIP_TRY(hipStreamSynchronize(l->stream));
    return BFIR_OK;
}

extern "C" int bfir_engine_set_coeff_matrix_pairs(bfir_engine *e, int n_pairs, const int *outputs, const int *inputs,
                                                  const void *const *coeffs, int length, int coeff_blocks, double scale)
{
    if (!e) return BFIR_ERR_ARG;
    if (!e->matrix || e->mlevels) return BFIR_ERR_UNSUPPORTED;
    if (length < 0 || coeff_blocks < 1) return BFIR_ERR_ARG;
    PairList pl;
    const int rc = pairs_list(e, n_pairs, outputs, inputs, coeffs, nullptr, length, pl);
    if (rc != BFIR_OK) return rc;
    if (!bfir_engine_is_initialized(e)) return BFIR_ERR_STATE;   // nothing to patch
    return set_coeff_uniform(e, uniform_taps(e, pl.rows, scale, coeff_blocks), &pl.row, -1);
}

extern "C" int bfir_engine_set_coeff_matrix_pairs_fade(bfir_engine *e, int n_pairs, const int *outputs, const int *inputs,
                                                       const void *const *coeffs, int length, int coeff_blocks, double scale,
                                                       int fade_blocks)
{
    if (!e) return BFIR_ERR_ARG;
    if (!e->matrix || e->mlevels) return BFIR_ERR_UNSUPPORTED;
    if (e->n_eng > 1 || e->d_dither_tab) return BFIR_ERR_UNSUPPORTED;   // as every fade: HP-TPDF dither is a recursion over the output
    if (length < 0 || coeff_blocks < 1) return BFIR_ERR_ARG;
    PairList pl;
    int rc = pairs_list(e, n_pairs, outputs, inputs, coeffs, nullptr, length, pl);
    if (rc == BFIR_OK) rc = check_fade_args(e, fade_blocks);
    if (rc != BFIR_OK) return rc;
    return set_coeff_uniform(e, uniform_taps(e, pl.rows, scale, coeff_blocks), &pl.row, fade_blocks);
}


// ---------------------------------------------------------------------------
// coefficient banks of a uniform matrix or mimo engine: filters transformed once into a store of the engine's own row form
// (bfir_engine_bank_create, _bank_load), and the four set calls with bank entries in place of host taps
// (bfir_engine_set_coeff_matrix_bank, _bank_fade, _pairs_bank, _pairs_bank_fade): one k_bank_gather launch (bank.hip) where
// the calls with taps upload and transform; and the same four with a weighted sum of up to BFIR_BANK_MIX_TERMS entries in
// place of one (bfir_engine_set_coeff_matrix_bank_mix, ...): one k_bank_mix launch (bankmix.hip)
// ---------------------------------------------------------------------------
static bool bank_kind(const bfir_engine *e) { return e->matrix && !e->mlevels; }
static int read_store_spectrum(bfir_engine *e, const void *store, int f, int block, void *dst);

extern "C" int bfir_engine_bank_create(bfir_engine *e, int n_entries)
{
    if (!e) return BFIR_ERR_ARG;
    if (!bank_kind(e)) return BFIR_ERR_UNSUPPORTED;
    if (n_entries < 1) return BFIR_ERR_ARG;
    if (e->bank) return BFIR_ERR_STATE;
    HIP_TRY(hipSetDevice(e->device));
    if (hipMalloc(&e->bank, (size_t)n_entries * e->B * cbuf_bytes(e)) != hipSuccess) {
        (void)hipGetLastError();
        e->bank = nullptr;
        return BFIR_ERR_HIP;
    }
    e->bank_nb.assign((size_t)n_entries, 0);                   // every entry empty; the store itself is not cleared
    return BFIR_OK;
}

extern "C" int bfir_engine_bank_destroy(bfir_engine *e)
{
    if (!e) return BFIR_ERR_ARG;
    if (!bank_kind(e)) return BFIR_ERR_UNSUPPORTED;
    if (!e->bank) return BFIR_OK;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    (void)hipFree(e->bank);
    e->bank = nullptr;
    e->bank_nb.clear();
    return BFIR_OK;
}

extern "C" int bfir_engine_bank_entries(const bfir_engine *e)
{
    if (!e) return BFIR_ERR_ARG;
    if (!bank_kind(e)) return BFIR_ERR_UNSUPPORTED;
    return (int)e->bank_nb.size();
}

extern "C" int bfir_engine_bank_blocks(const bfir_engine *e, int entry)
{
    if (!e) return BFIR_ERR_ARG;
    if (!bank_kind(e)) return BFIR_ERR_UNSUPPORTED;
    if (entry < 0 || (size_t)entry >= e->bank_nb.size()) return BFIR_ERR_ARG;
    return e->bank_nb[entry];
}

extern "C" int bfir_engine_bank_load(bfir_engine *e, int first, int n, const void *const *coeffs, int length, int coeff_blocks,
                                     double scale)
{
    if (!e) return BFIR_ERR_ARG;
    if (!bank_kind(e)) return BFIR_ERR_UNSUPPORTED;
    if (!coeffs || n < 1 || first < 0 || length < 0 || coeff_blocks < 1) return BFIR_ERR_ARG;
    if (!e->bank) return BFIR_ERR_STATE;
    if ((size_t)first + (size_t)n > e->bank_nb.size()) return BFIR_ERR_ARG;
    const int nb = std::min(coeff_blocks, e->B);
    FilterRows rows((size_t)n);
    for (int k = 0; k < n; k++) { rows.taps[k] = coeffs[k]; rows.len[k] = coeffs[k] ? length : 0; }
    // a NaN / Inf tap anywhere is refused before anything is uploaded: the bank is unchanged
    int rc = check_rows(e, rows, (size_t)nb * e->L, scale);
    if (rc != BFIR_OK) return rc;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());                            // the store is written on an idle device
    for (int k = 0; k < n; k++) e->bank_nb[first + k] = 0;     // a failed load leaves them empty
    rc = load_filters(e, e->bank, first, rows, nb, scale);      // one upload, one transform launch; the rows' other partitions cleared
    if (rc != BFIR_OK) return rc;
    for (int k = 0; k < n; k++) e->bank_nb[first + k] = coeffs[k] ? nb : 0;
    return BFIR_OK;
}

extern "C" int bfir_engine_bank_read(bfir_engine *e, int entry, int block, void *dst)
{
    if (!e) return BFIR_ERR_ARG;
    if (!bank_kind(e)) return BFIR_ERR_UNSUPPORTED;
    if (!dst || block < 0 || block >= e->B) return BFIR_ERR_ARG;
    if (!e->bank) return BFIR_ERR_STATE;
    if (entry < 0 || (size_t)entry >= e->bank_nb.size()) return BFIR_ERR_ARG;
    if (block >= e->bank_nb[entry]) {   // what a gather writes there: an empty entry has no spectra, a short one zeros behind its count
        memset(dst, 0, cbuf_bytes(e));
        return BFIR_OK;
    }
    return read_store_spectrum(e, e->bank, entry, block, dst);
}

namespace {
struct BankList {
    std::vector<int> row;        // a pairs call: the rows of the store that are written, filter o C + i (else the whole store)
    std::vector<int> ent;        // the bank entry of each, or -1: no path
    std::vector<int> mix;        // a mix call: k_bank_mix's records, [rows][BFIR_BANK_MIX_REC] (ent is not used)
};
}

static_assert(coeff_tables::kMixRec == BFIR_BANK_MIX_REC, "coeff_tables::mix_records writes k_bank_mix's records");

// The source's rows of Hdst (H, or H2) from the bank: the table goes up, ONE gather (k_bank_gather, or a mix call's
// k_bank_mix) is queued on the stream that owns every write to the store, and the host waits for it.  The device is idle.
static int bank_gather(bfir_engine *e, void *Hdst, const UniformSource &src, const std::vector<int> *list)
{
    const std::vector<int> tab = src.mix ? *src.mix : coeff_tables::gather_table(list, *src.ent, e->bank_nb);
    const int rc = upload_table(e->d_gather, e->gather_ints, tab);
    if (rc != BFIR_OK) return rc;
    if (src.mix) {
        BankMixArgs a;
        a.bank = e->bank; a.dst = Hdst; a.tab = e->d_gather; a.n_rows = (int)(tab.size() / BFIR_BANK_MIX_REC);
        a.part_bytes = cbuf_bytes(e); a.row_bytes = (unsigned long long)e->B * a.part_bytes;
        if (launch_bank_mix(a, e->s, e->stream) != 0) return BFIR_ERR_UNSUPPORTED;
    } else {
        BankArgs a;
        a.bank = e->bank; a.dst = Hdst; a.tab = e->d_gather; a.n_rows = (int)src.ent->size();
        a.part_bytes = cbuf_bytes(e); a.row_bytes = (unsigned long long)e->B * a.part_bytes;
        if (launch_bank_gather(a, e->stream) != 0) return BFIR_ERR_UNSUPPORTED;
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipGetLastError());
    return BFIR_OK;
}

// k_patch_pairs' table of one level (a uniform engine: itself) in its d_patch, for the listed rows and the counts of its two sets
static int patch_table_set(bfir_engine *l, const std::vector<int> &list)
{
    return upload_table(l->d_patch, l->patch_ints, coeff_tables::patch_table(l->Co, l->C, list, l->nblk2, l->nblk));
}

// The front end of a uniform matrix engine's fade, its two sets' counts in nblk and nblk2: no channel pairs around an unread
// input, per set.  The fade's forward transforms take the pair path only if every input is read under BOTH sets; after the
// fade the new set decides (pair_new, fade_swap_sets).
static void fade_front_end(bfir_engine *e)
{
    if (!e->matrix || !e->pair_cap) return;
    e->pair_new = every_input_read(e, [&](int, int n) { return e->nblk2[n]; });
    matrix_take_path(e, e->pair_new && every_input_read(e, [&](int, int n) { return e->nblk[n]; }));
}

// the three operations of a UniformSource: the finite check (taps alone), ...
static int source_check(const bfir_engine *e, const UniformSource &src)
{
    return src.rows ? check_rows(e, *src.rows, (size_t)src.nb * e->L, src.scale) : BFIR_OK;
}

// ... the partition count of every row of the call (a diagonal engine: its zero rows past n_coeffs too, which are still
// multiplied; a matrix NULL and a -1 entry: 0, no path; a mix: the largest live term's), ...
static std::vector<int> source_counts(const bfir_engine *e, const UniformSource &src)
{
    std::vector<int> nb(src.rows ? src.rows->taps.size() : src.ent ? src.ent->size() : src.mix->size() / BFIR_BANK_MIX_REC);
    for (size_t j = 0; j < nb.size(); j++)
        nb[j] = src.rows ? (e->matrix && !src.rows->taps[j] ? 0 : src.nb)
              : src.ent  ? coeff_tables::entry_count(e->bank_nb, (*src.ent)[j]) : (*src.mix)[j * BFIR_BANK_MIX_REC + 1];
    return nb;
}

// ... and its rows (nb: their counts) written to Hdst, row j of the call to row list[j], or all of them (list == nullptr) to
// the whole store: taps in one load_filters or row by row, entries and mixes in one gather.  Every write is queued on
// e->stream, and the host has waited for the last of them.
static int source_write(bfir_engine *e, const UniformSource &src, const std::vector<int> &nb, void *Hdst, const std::vector<int> *list)
{
    if (!src.rows) return bank_gather(e, Hdst, src, list);
    if (!list) return load_filters(e, Hdst, 0, *src.rows, src.nb, src.scale);
    return load_listed_rows(e, Hdst, *src.rows, nb, *list, src.scale);
}

// Every coefficient change of a uniform engine but the batch form (bfir_engine_set_coeff_at), its arguments checked by the
// entry point: the rows of `src` replace the rows `list` of the filter store (nullptr: the whole store), at once
// (fade_blocks < 0; the active set H is written) or over the next fade_blocks blocks (the second set H2 is).  A NaN / Inf tap
// is refused before anything changes -- or (check_first = false: bfir_engine_set_coeff_matrix) on the idle device behind
// free_coeff(), which leaves the engine without coefficients.
static int set_coeff_uniform(bfir_engine *e, const UniformSource &src, const std::vector<int> *list, int fade_blocks, bool check_first)
{
    const bool fade = fade_blocks >= 0;
    int rc = check_first ? source_check(e, src) : BFIR_OK;
    if (rc != BFIR_OK) return rc;
    HIP_TRY(hipSetDevice(e->device));
    // queued work may still read the bank, what was H before the last fade's swap, or a table: all written on an idle device
    HIP_TRY(hipDeviceSynchronize());
    if (!fade) {
        e->fade_len = e->fade_pos = 0;                          // a plain change during a fade cancels it: a hard cut, the old set
        e->fade_patch = false;                                  // stays and (a list) is patched
        if (!list) e->eng_init[0] = 0;                          // free_coeff(), brutefir.cpp:188
        if (!check_first) rc = source_check(e, src);
    } else {
        rc = fade_prepare(e, (int)e->nblk.size());
        // a list: the merged set is the whole store copied, then the listed rows, both on e->stream and so in order
        if (rc == BFIR_OK && list)
            HIP_TRY(hipMemcpyAsync(e->H2, e->H, e->nblk.size() * e->B * cbuf_bytes(e), hipMemcpyDeviceToDevice, e->stream));
    }
    if (rc != BFIR_OK) return rc;
    const std::vector<int> nb = source_counts(e, src);
    rc = source_write(e, src, nb, fade ? e->H2 : e->H, list);
    if (rc != BFIR_OK) return rc;
    std::vector<int> &cnt = fade ? e->nblk2 : e->nblk;
    if (fade) { if (list) e->nblk2 = e->nblk; else e->nblk2.assign(e->nblk.size(), 0); }
    for (size_t j = 0; j < nb.size(); j++) cnt[coeff_tables::dest_row(list, j)] = nb[j];
    rc = upload_counts(e, fade);
    if (rc != BFIR_OK) return rc;
    if (!fade) return matrix_counts_set(e);
    if (list) { rc = patch_table_set(e, *list); if (rc != BFIR_OK) return rc; }
    fade_front_end(e);
    fade_begin(e, fade_blocks);
    e->fade_patch = list != nullptr;                            // behind fade_begin, which clears it
    return BFIR_OK;
}

// The eight calls with bank entries.  pairs: a list (outputs, inputs, entries of n), else the whole matrix (entries[o C + i]);
// fade_blocks < 0: the plain call; n_terms > 0: a mix call, n_terms (entry, weight) terms per row in place of one entry.  The
// order of the refusals is that of the calls with taps, with the bank's own behind the arguments.
static int set_coeff_bank(bfir_engine *e, bool pairs, int n, const int *outputs, const int *inputs, const int *entries,
                          bool fade, int fade_blocks, bool mix = false, int n_terms = 0, const double *weights = nullptr)
{
    if (!e) return BFIR_ERR_ARG;
    if (!bank_kind(e)) return BFIR_ERR_UNSUPPORTED;
    if (fade && (e->n_eng > 1 || e->d_dither_tab)) return BFIR_ERR_UNSUPPORTED;   // as every fade
    if (!entries || (pairs && (!outputs || !inputs || n < 1))) return BFIR_ERR_ARG;
    if (mix && (!weights || n_terms < 1 || n_terms > BFIR_BANK_MIX_TERMS)) return BFIR_ERR_ARG;
    if (!e->bank) return BFIR_ERR_STATE;
    BankList bl;
    const std::vector<int> *list = pairs ? &bl.row : nullptr;
    const int n_rows = pairs ? n : e->Co * e->C;
    int rc = pairs ? coeff_tables::list_rows(e->Co, e->C, n, outputs, inputs, bl.row) : BFIR_OK;
    if (rc == BFIR_OK) rc = mix ? coeff_tables::mix_records(e->bank_nb, e->s, list, n_rows, n_terms, entries, weights, bl.mix)
                                : coeff_tables::check_entries(e->bank_nb, n_rows, entries, bl.ent);
    if (rc == BFIR_OK && fade) rc = check_fade_args(e, fade_blocks);
    if (rc != BFIR_OK) return rc;
    if (pairs && !bfir_engine_is_initialized(e)) return BFIR_ERR_STATE;   // nothing to patch
    if (n_rows > 65535) return BFIR_ERR_UNSUPPORTED;            // the gather's grid; a matrix has 64 x 64 rows at most
    UniformSource src;
    if (mix) src.mix = &bl.mix; else src.ent = &bl.ent;
    return set_coeff_uniform(e, src, list, fade ? fade_blocks : -1);
}

extern "C" int bfir_engine_set_coeff_matrix_bank(bfir_engine *e, const int *entries)
{
    return set_coeff_bank(e, false, 0, nullptr, nullptr, entries, false, 0);
}

extern "C" int bfir_engine_set_coeff_matrix_bank_fade(bfir_engine *e, const int *entries, int fade_blocks)
{
    return set_coeff_bank(e, false, 0, nullptr, nullptr, entries, true, fade_blocks);
}

extern "C" int bfir_engine_set_coeff_matrix_pairs_bank(bfir_engine *e, int n_pairs, const int *outputs, const int *inputs,
                                                       const int *entries)
{
    return set_coeff_bank(e, true, n_pairs, outputs, inputs, entries, false, 0);
}

extern "C" int bfir_engine_set_coeff_matrix_pairs_bank_fade(bfir_engine *e, int n_pairs, const int *outputs, const int *inputs,
                                                            const int *entries, int fade_blocks)
{
    return set_coeff_bank(e, true, n_pairs, outputs, inputs, entries, true, fade_blocks);
}

extern "C" int bfir_engine_set_coeff_matrix_bank_mix(bfir_engine *e, int n_terms, const int *entries, const double *weights)
{
    return set_coeff_bank(e, false, 0, nullptr, nullptr, entries, false, 0, true, n_terms, weights);
}

extern "C" int bfir_engine_set_coeff_matrix_bank_mix_fade(bfir_engine *e, int n_terms, const int *entries, const double *weights,
                                                          int fade_blocks)
{
    return set_coeff_bank(e, false, 0, nullptr, nullptr, entries, true, fade_blocks, true, n_terms, weights);
}

extern "C" int bfir_engine_set_coeff_matrix_pairs_bank_mix(bfir_engine *e, int n_pairs, const int *outputs, const int *inputs,
                                                           int n_terms, const int *entries, const double *weights)
{
    return set_coeff_bank(e, true, n_pairs, outputs, inputs, entries, false, 0, true, n_terms, weights);
}

extern "C" int bfir_engine_set_coeff_matrix_pairs_bank_mix_fade(bfir_engine *e, int n_pairs, const int *outputs, const int *inputs,
                                                                int n_terms, const int *entries, const double *weights,
                                                                int fade_blocks)
{
    return set_coeff_bank(e, true, n_pairs, outputs, inputs, entries, true, fade_blocks, true, n_terms, weights);
}

extern "C" int bfir_engine_fade_remaining(const bfir_engine *e)
{
    if (!e) return BFIR_ERR_ARG;
    if (e->nup) return BFIR_ERR_UNSUPPORTED;
    return e->fade_len > 0 ? e->fade_len - e->fade_pos : 0;
}

// partition spectrum `block` of row `f` of a filter store (H, or the bank) to host, in the reference's grouped layout
static int read_store_spectrum(bfir_engine *e, const void *store, int f, int block, void *dst)
{
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t cb = cbuf_bytes(e);
    HIP_TRY(hipMemcpy(dst, (const char *)store + ((size_t)f * e->B + block) * cb, cb, hipMemcpyDeviceToHost));
    if (e->big) {   // ... and natural bin order: bin k1 + M1 k2 is kept at position k1 M2 + k2 (bigconv.hip), in either layout
        const int l1 = e->bplan.log2m1, M2 = 1 << e->bplan.log2m2;
        const bool ilv = e->ilv;
        auto natural = [&](auto *o) {
            using R = typename std::remove_pointer<decltype(o)>::type;
            std::vector<R> tmp(o, o + e->N);
            for (int k = 0; k < e->N / 2; k++) {
                const int p = (k & ((1 << l1) - 1)) * M2 + (k >> l1);
                o[8 * (k >> 2) + (k & 3)] = ilv ? tmp[2 * p] : tmp[8 * (p >> 2) + (p & 3)];
                o[8 * (k >> 2) + 4 + (k & 3)] = ilv ? tmp[2 * p + 1] : tmp[8 * (p >> 2) + 4 + (p & 3)];
            }
        };
        if (e->s == 4) natural((float *)dst); else natural((double *)dst);
    } else if (e->ilv) {   // hand out the reference's grouped layout (fftw_convolver.cpp:883-907)
        auto regroup = [&](auto *o) {
            using R = typename std::remove_pointer<decltype(o)>::type;
            std::vector<R> tmp(o, o + e->N);
            for (int k = 0; k < e->N / 2; k++) {
                o[8 * (k >> 2) + (k & 3)] = tmp[2 * k];
                o[8 * (k >> 2) + 4 + (k & 3)] = tmp[2 * k + 1];
            }
        };
        if (e->s == 4) regroup((float *)dst); else regroup((double *)dst);
    }
    return BFIR_OK;
}

// ... of filter `f` of the active set
static int read_spectrum(bfir_engine *e, int f, int block, void *dst) { return read_store_spectrum(e, e->H, f, block, dst); }

extern "C" int bfir_engine_read_coeff(bfir_engine *e, int channel, int block, void *dst)
{
    if (!e || channel < 0 || channel >= e->GC || block < 0 || block >= e->B || !dst) return BFIR_ERR_ARG;
    if (e->matrix) return BFIR_ERR_UNSUPPORTED;                 // bfir_engine_read_coeff_matrix
    if (e->nup) return BFIR_ERR_UNSUPPORTED;                    // bfir_engine_read_coeff_nup
    return read_spectrum(e, channel, block, dst);
}

extern "C" int bfir_engine_read_coeff_nup(bfir_engine *e, int level, int channel, int block, void *dst)
{
    if (!e) return BFIR_ERR_ARG;
    if (!e->nup || e->levels || e->mlevels) return BFIR_ERR_UNSUPPORTED;
    if (level < 0 || level > 1 || !dst) return BFIR_ERR_ARG;
    bfir_engine *lv = level ? e->tail[0] : e;
    if (channel < 0 || channel >= lv->GC || block < 0 || block >= lv->B) return BFIR_ERR_ARG;
    return read_spectrum(lv, channel, block, dst);
}

extern "C" int bfir_engine_read_coeff_levels(bfir_engine *e, int level, int channel, int block, void *dst)
{
    if (!e) return BFIR_ERR_ARG;
    if (!e->levels) return BFIR_ERR_UNSUPPORTED;
    if (level < 0 || level > e->n_tail || !dst) return BFIR_ERR_ARG;
    bfir_engine *lv = level ? e->tail[level - 1] : e;
    if (channel < 0 || channel >= lv->GC || block < 0 || block >= lv->B) return BFIR_ERR_ARG;
    return read_spectrum(lv, channel, block, dst);
}

extern "C" int bfir_engine_read_coeff_matrix(bfir_engine *e, int output, int input, int block, void *dst)
{
    if (!e) return BFIR_ERR_ARG;
    if (!e->matrix || e->mlevels) return BFIR_ERR_UNSUPPORTED;   // bfir_engine_read_coeff_matrix_levels
    if (output < 0 || output >= e->Co || input < 0 || input >= e->C || block < 0 || block >= e->B || !dst) return BFIR_ERR_ARG;
    return read_spectrum(e, output * e->C + input, block, dst);
}

extern "C" int bfir_engine_read_coeff_matrix_levels(bfir_engine *e, int level, int output, int input, int block, void *dst)
{
    if (!e) return BFIR_ERR_ARG;
    if (!e->mlevels) return BFIR_ERR_UNSUPPORTED;
    if (level < 0 || level > e->n_tail || !dst) return BFIR_ERR_ARG;
    bfir_engine *lv = level ? e->tail[level - 1] : e;
    if (output < 0 || output >= lv->Co || input < 0 || input >= lv->C || block < 0 || block >= lv->B) return BFIR_ERR_ARG;
    return read_spectrum(lv, output * lv->C + input, block, dst);
}

// ---------------------------------------------------------------------------
// profiling helpers
// ---------------------------------------------------------------------------
static hipEvent_t take_event(bfir_engine *e)
{
    if (!e->ev_pool.empty()) { hipEvent_t ev = e->ev_pool.back(); e->ev_pool.pop_back(); return ev; }
    hipEvent_t ev = nullptr;
    (void)hipEventCreate(&ev);
    return ev;
}

struct ProfScope {
    bfir_engine *e; int k; hipStream_t st; hipEvent_t a = nullptr;
    ProfScope(bfir_engine *e_, int k_, hipStream_t st_) : e(e_), k(k_), st(st_)
    {
        if (e->profiling) { a = take_event(e); (void)hipEventRecord(a, st); }
    }
    ~ProfScope()
    {
        if (e->profiling) {
            hipEvent_t b = take_event(e);
            (void)hipEventRecord(b, st);
            e->spans.push_back({k, a, b});
        }
    }
};

static void drain_spans(bfir_engine *e)
{
    for (auto &sp : e->spans) {
        float ms = 0.f;
        if (hipEventSynchronize(sp.b) == hipSuccess && hipEventElapsedTime(&ms, sp.a, sp.b) == hipSuccess) {
            e->prof_ms[sp.k] += ms;
            e->prof_n[sp.k] += 1;
        }
        e->ev_pool.push_back(sp.a);
        e->ev_pool.push_back(sp.b);
    }
    e->spans.clear();
}

extern "C" int bfir_engine_set_profiling(bfir_engine *e, int enable)
{
    if (!e) return BFIR_ERR_ARG;
    for (bfir_engine *t : e->tail) if (t) (void)bfir_engine_set_profiling(t, enable);   // a two- or multi-level engine reports the sum of its levels
    drain_spans(e);
    e->profiling = enable != 0;
    if (e->profiling && e->ev_pool.size() < 4096) {   // keep event creation out of timed regions
        for (int i = 0; i < 4096; i++) { hipEvent_t ev = nullptr; if (hipEventCreate(&ev) == hipSuccess) e->ev_pool.push_back(ev); }
    }
    for (int k = 0; k < BFIR_K_COUNT; k++) { e->prof_ms[k] = 0; e->prof_n[k] = 0; }
    return BFIR_OK;
}

extern "C" int bfir_engine_get_profile(bfir_engine *e, int kernel, double *total_ms, int64_t *launches)
{
    if (!e || kernel < 0 || kernel >= BFIR_K_COUNT) return BFIR_ERR_ARG;
    drain_spans(e);
    double ms = e->prof_ms[kernel];
    int64_t n = e->prof_n[kernel];
    for (bfir_engine *t : e->tail)
        if (t) { drain_spans(t); ms += t->prof_ms[kernel]; n += t->prof_n[kernel]; }
    if (total_ms) *total_ms = ms;
    if (launches) *launches = n;
    return BFIR_OK;
}

// ---------------------------------------------------------------------------
// brutefir::run, chunked and software-pipelined over three streams
// ---------------------------------------------------------------------------
// Queue one chunk of tc blocks (frames frame_off .. of every engine's raw
// buffer).  `st` is the caller's stream: the input must be ready on it when
// this is called, and the output is complete on it when its work is.
//   s_front : front(k)                (k = chunk sequence number)
//   s_mac   : mac(k)                  waits fwd(k) and inv(k-2) (owner of Yb[k&1])
//   st      : back(k)                 waits mac(k)
// fwd(k) writes delay-line slots that mac(k-2) may still read (ring = 2*chunk+B),
// and stage_in(k) rewrites the time buffer fwd(k-2) read; both are ordered by
// events / stream order.  So fwd(k+1), mac(k) and inv/stage_out(k-1) share the
// GPU: none of the kernels saturates VALU or HBM alone (load-latency phases,
// profiles/r01_phase_trace.txt), together they fill each other's gaps.
// Front and back are what the engine's path makes them:
//   staging : stage_in -> fwd         inv -> stage_out     planar time buffers tin / tout between them
//   pair    : fwd_pair                inv_pair             raw frames <-> spectra of two channels per transform (pair.hip)
//   direct  : fwd                     inv                  k_fwd / k_inv in direct mode (kernels.h), one channel per transform
// Pair and direct have no planar time buffers; their inverse writes the raw frames and the overflow statistics itself.
enum class Path { Staging, Pair, Direct };
// a matrix engine may change between pair and direct when its filters are set (bfir_engine_set_coeff_matrix)
static Path chunk_path(const bfir_engine *e) { return e->pair ? Path::Pair : e->direct ? Path::Direct : Path::Staging; }

// One chunk as its launches see it
struct Chunk {
    const void *d_in; long in_stride; void *d_out; long out_stride;   // the caller's frames; engine strides in bytes
    long frame_off; int tc, block_base;
    int par;         // chunk parity: which tin / tails set / Yb / events are this chunk's
    int base_slot;   // delay-line slot of its first block
    // input_timecbuf bookkeeping: block j of the chunk lands in buffer !(curbuf ^ (j & 1)); this is the last block's
    int idx_last;
    void *Y;         // product spectra
    // a fade chunk (all of its blocks fade): the products with the new set, Yf's own channel stride, m of its first sample
    bool fade = false; void *Y2 = nullptr; long y2_ch_stride = 0; int m0 = 0;
};

// The MAC of a diagonal engine's chunk (second = the fade's new set: H2 and its counts) ...
static MacArgs mac_args(const bfir_engine *e, int base_slot, void *Y, int tc, bool second = false)
{
    MacArgs a;
    a.x = e->X; a.x_ch_stride = (long)e->ring * e->N; a.ring = e->ring; a.base_slot = base_slot;
    a.h = second ? e->H2 : e->H; a.h_ch_stride = (long)e->B * e->N;
    a.nblk = second ? e->d_nblk2 : e->d_nblk;
    a.y = Y; a.y_ch_stride = (long)e->chunk * e->N;
    a.n_t = tc; a.n_ch = e->GC; a.N = e->N; a.realsize = e->s; a.B = e->B;
    a.interleaved = e->ilv;   // the pair path implies it
    return a;
}

// ... and of a matrix engine's: k_mac_matrix over the engine's delay line and filters.
static MatArgs matrix_mac_args(const bfir_engine *e, int base_slot, void *Y, int tc, bool second = false)
{
    const std::vector<int> &nblk = second ? e->nblk2 : e->nblk;
    MatArgs a;
    a.x = e->X; a.x_ch_stride = (long)e->ring * e->N; a.ring = e->ring; a.base_slot = base_slot;
    a.h = second ? e->H2 : e->H; a.h_pair_stride = (long)e->B * e->N;
    for (int j = 0; j < BFIR_MAT_MAX * BFIR_MAT_MAX; j++) a.nblk[j] = j < (int)nblk.size() ? nblk[j] : 0;
    a.y = Y; a.y_ch_stride = (long)e->chunk * e->N;
    a.n_t = tc; a.n_in = e->C; a.n_out = e->Co; a.N = e->N; a.realsize = e->s;
    a.interleaved = e->ilv;
    return a;
}

// ... and of a mimo engine's where k_mac_mimo runs it: the same, with the counts in the engine's table in HBM
static MimoArgs mimo_mac_args(const bfir_engine *e, int base_slot, void *Y, int tc, bool second = false)
{
    MimoArgs a;
    a.x = e->X; a.x_ch_stride = (long)e->ring * e->N; a.ring = e->ring; a.base_slot = base_slot;
    a.h = second ? e->H2 : e->H; a.h_pair_stride = (long)e->B * e->N;
    a.nblk = second ? e->d_nblk2 : e->d_nblk;
    a.y = Y; a.y_ch_stride = (long)e->chunk * e->N;
    a.n_t = tc; a.n_in = e->C; a.n_out = e->Co; a.N = e->N; a.realsize = e->s;
    a.interleaved = e->ilv;
    return a;
}

// The MAC of tc blocks of an engine, a level included, from delay-line slot base_slot on into Y (y_ch_stride reals per
// channel) with the active or the second set: k_mac on a diagonal engine, k_mac_matrix on a matrix engine, k_mac_mimo
// on a mimo engine (mimo_mac).
static int queue_mac(const bfir_engine *e, int base_slot, void *Y, long y_ch_stride, int tc, bool second, hipStream_t s)
{
    if (!e->matrix) {
        MacArgs a = mac_args(e, base_slot, Y, tc, second);
        a.y_ch_stride = y_ch_stride;
        launch_mac(a, s);
        return BFIR_OK;
    }
    if (e->mimo_mac) {
        MimoArgs a = mimo_mac_args(e, base_slot, Y, tc, second);
        a.y_ch_stride = y_ch_stride;
        return launch_mac_mimo(a, s) != 0 ? BFIR_ERR_UNSUPPORTED : BFIR_OK;
    }
    MatArgs a = matrix_mac_args(e, base_slot, Y, tc, second);
    a.y_ch_stride = y_ch_stride;
    return launch_mac_matrix(a, s) != 0 ? BFIR_ERR_UNSUPPORTED : BFIR_OK;
}

// a chunk the matrix MAC cannot take is refused before anything is queued (never skipped)
static int matrix_chunk_ok(const bfir_engine *e, int tc)
{
    if (e->matrix && !(e->mimo_mac ? mac_mimo_supported(mimo_mac_args(e, 0, nullptr, tc))
                                   : mac_matrix_supported(matrix_mac_args(e, 0, nullptr, tc)))) {
        bfir_logf("bfir engine: %d blocks per launch are past the matrix MAC's grid.", tc);
        return BFIR_ERR_UNSUPPORTED;
    }
    return BFIR_OK;
}

// Both sets of a fading level of a multi-level matrix engine in one launch (k_mac_duo, mfade.hip): the old set as
// matrix_mac_args gives it, the new set into Y2.
static bool chunk_takes_duo(const bfir_engine *e) { return e->matrix && e->mfade_duo && (e->mlevels || e->nup_tail); }

static MatDuoArgs matrix_duo_args(const bfir_engine *e, int base_slot, void *Y, void *Y2, long y2_ch_stride, int tc)
{
    MatDuoArgs d;
    d.a = matrix_mac_args(e, base_slot, Y, tc);
    d.h2 = e->H2;
    for (int j = 0; j < BFIR_MAT_MAX * BFIR_MAT_MAX; j++) d.nblk2[j] = j < (int)e->nblk2.size() ? e->nblk2[j] : 0;
    d.y2 = Y2; d.y2_ch_stride = y2_ch_stride;
    return d;
}

// ... and where the level's MAC is k_mac_mimo: k_wduo (wduo.hip), both tables in HBM
static WduoArgs wduo_args(const bfir_engine *e, int base_slot, void *Y, void *Y2, long y2_ch_stride, int tc)
{
    WduoArgs d;
    d.a = mimo_mac_args(e, base_slot, Y, tc);
    d.h2 = e->H2; d.nblk2 = e->d_nblk2;
    d.y2 = Y2; d.y2_ch_stride = y2_ch_stride;
    return d;
}

// the one launch for both sets of tc blocks from base_slot on: Y as queue_mac gives it (e->chunk blocks per channel), Y2
static int queue_duo(const bfir_engine *e, int base_slot, void *Y, void *Y2, long y2_ch_stride, int tc, hipStream_t s)
{
    const int rc = e->mimo_mac ? launch_wduo(wduo_args(e, base_slot, Y, Y2, y2_ch_stride, tc), s)
                               : launch_mac_duo(matrix_duo_args(e, base_slot, Y, Y2, y2_ch_stride, tc), s);
    return rc != 0 ? BFIR_ERR_UNSUPPORTED : BFIR_OK;
}

// ... whose grid differs from the one-set MAC's (other tiles): refused before anything is queued, as matrix_chunk_ok
static int matrix_fade_chunk_ok(const bfir_engine *e, int tc)
{
    if (chunk_takes_duo(e) && !(e->mimo_mac ? wduo_supported(wduo_args(e, 0, nullptr, nullptr, 0, tc))
                                            : mac_duo_supported(matrix_duo_args(e, 0, nullptr, nullptr, 0, tc)))) {
        bfir_logf("bfir engine: %d fading blocks per launch are past the matrix MAC's grid.", tc);
        return BFIR_ERR_UNSUPPORTED;
    }
    return BFIR_OK;
}

// The new set's products of a patch fade's chunk from the old set's (k_patch_pairs, patch.hip), behind the old set's MAC
static PatchArgs patch_args(const bfir_engine *e, int base_slot, void *Y, void *Y2, long y2_ch_stride, int tc)
{
    PatchArgs a;
    a.x = e->X; a.x_ch_stride = (long)e->ring * e->N; a.ring = e->ring; a.base_slot = base_slot;
    a.h = e->H; a.h2 = e->H2; a.h_pair_stride = (long)e->B * e->N;
    a.row = e->d_patch; a.ent = e->d_patch + e->Co + 1;
    a.y = Y; a.y_ch_stride = (long)e->chunk * e->N;
    a.y2 = Y2; a.y2_ch_stride = y2_ch_stride;
    a.n_t = tc; a.n_in = e->C; a.n_out = e->Co; a.N = e->N; a.realsize = e->s;
    a.interleaved = e->ilv;
    return a;
}

// MAC and patch in one launch (k_wpatch, wpatch.hip): a level of a multi-level engine whose MAC is k_mac_mimo, where the
// switch asks for it.  A uniform engine keeps its two launches, and so does a level on k_mac_matrix.
static bool chunk_takes_wpatch(const bfir_engine *e) { return e->patch_fused && e->mimo_mac && (e->mlevels || e->nup_tail); }

static WpatchArgs wpatch_args(const bfir_engine *e, int base_slot, void *Y, long y_ch_stride, void *Y2, long y2_ch_stride, int tc)
{
    WpatchArgs d;
    d.a = mimo_mac_args(e, base_slot, Y, tc);
    d.a.y_ch_stride = y_ch_stride;
    d.h2 = e->H2;
    d.row = e->d_patch; d.ent = e->d_patch + e->Co + 1;
    d.y2 = Y2; d.y2_ch_stride = y2_ch_stride;
    return d;
}

// ... whose grid is its own (k_wpatch: k_mac_mimo's, but for one instance): refused before anything is queued, as
// matrix_fade_chunk_ok
static int patch_chunk_ok(const bfir_engine *e, int tc)
{
    const long ys = (long)e->chunk * e->N;
    if (!patch_supported(patch_args(e, 0, nullptr, nullptr, 0, tc)) ||
        (chunk_takes_wpatch(e) && !wpatch_supported(wpatch_args(e, 0, nullptr, ys, nullptr, 0, tc)))) {
        bfir_logf("bfir engine: %d fading blocks per launch are past the pair-list kernel's grid.", tc);
        return BFIR_ERR_UNSUPPORTED;
    }
    return BFIR_OK;
}

// The old set's products of tc blocks from base_slot on into Y and, behind them, the patch into Y2: the MAC queue_mac
// launches and k_patch_pairs, or k_wpatch for both (the same bits).  spans (a chunk of a multi-level engine): every launch
// is a BFIR_K_MAC span of its own, so the profile's launch count tells the one launch from the two.
static int queue_mac_patch(bfir_engine *e, int base_slot, void *Y, long y_ch_stride, void *Y2, long y2_ch_stride, int tc,
                           hipStream_t s, bool spans)
{
    const bool prof = e->profiling;
    if (!spans) e->profiling = false;
    int rc;
    if (chunk_takes_wpatch(e)) {
        ProfScope ps(e, BFIR_K_MAC, s);
        rc = launch_wpatch(wpatch_args(e, base_slot, Y, y_ch_stride, Y2, y2_ch_stride, tc), s) != 0 ? BFIR_ERR_UNSUPPORTED : BFIR_OK;
    } else {
        {
            ProfScope ps(e, BFIR_K_MAC, s);
            rc = queue_mac(e, base_slot, Y, y_ch_stride, tc, false, s);
        }
        if (rc == BFIR_OK) {
            ProfScope ps(e, BFIR_K_MAC, s);
            PatchArgs a = patch_args(e, base_slot, Y, Y2, y2_ch_stride, tc);
            a.y_ch_stride = y_ch_stride;
            rc = launch_patch(a, s) != 0 ? BFIR_ERR_UNSUPPORTED : BFIR_OK;
        }
    }
    e->profiling = prof;
    return rc;
}

// what the path's kernels ask of the caller's frame buffers (the staging kernels: nothing)
static int chunk_aligned(const bfir_engine *e, Path p, const Chunk &c)
{
    // a multi-level matrix engine with an odd output count stores its frame pairs at 4-byte alignment
    const uintptr_t out_mask = (e->pair_tp || (e->matrix && (e->Co & 1))) ? 3 : 7;
    if (p == Path::Pair &&
        ((((uintptr_t)c.d_in | (uintptr_t)c.in_stride) & (e->pair_tp ? 3 : 7)) || (((uintptr_t)c.d_out | (uintptr_t)c.out_stride) & out_mask))) {
        bfir_logf("bfir engine: frame buffers of the float fast path must be 8-byte aligned (4 with an odd channel count).");
        return BFIR_ERR_ARG;
    }
    if (p == Path::Direct && (((uintptr_t)c.d_in | (uintptr_t)c.in_stride) % e->in_bytes ||
                              ((uintptr_t)c.d_out | (uintptr_t)c.out_stride) % e->out_bytes)) {
        bfir_logf("bfir engine: frame buffers must be aligned to their sample size.");
        return BFIR_ERR_ARG;
    }
    return BFIR_OK;
}

// staging path, ahead of the forward transform: raw frames -> planar time buffer tin[par]
static void queue_stage_in(bfir_engine *e, const Chunk &c, hipStream_t sf)
{
    ProfScope ps(e, BFIR_K_STAGE_IN, sf);
    StageInArgs a;
    a.raw = c.d_in; a.eng_stride_bytes = c.in_stride; a.frame_off = c.frame_off;
    a.n_eng = e->n_eng; a.C = e->C; a.raw_bytes = e->in_bytes; a.spacing = e->C; a.fmt = e->in_fmt;
    a.n_frames = (long)c.tc * e->L;
    a.dst = e->tin[c.par]; a.dst_ch_stride = (long)e->chunk * e->L; a.dst_off = 0;
    a.realsize = e->s;
    launch_stage_in(a, sf);
}

// The chunk's blocks -> delay-line spectra.  Pair and direct keep the raw frames of the chunk's last two blocks in
// tails[par] as the time history of the next chunk (the staging path: queue_stage_out).
static void queue_fwd(bfir_engine *e, Path p, const Chunk &c, hipStream_t sf)
{
    ProfScope ps(e, BFIR_K_FWD, sf);
    if (p == Path::Pair) {
        FwdPairArgs a;
        a.raw = (const float *)c.d_in; a.eng_stride = c.in_stride / 4; a.frame_off = c.frame_off;
        a.C = e->C; a.n_eng = e->n_eng; a.n_t = c.tc;
        a.prev = e->hist_raw[e->curbuf];
        a.save_last = e->tails[c.par][c.idx_last]; a.save_prev = e->tails[c.par][1 ^ c.idx_last];
        a.carry = e->hist_raw[1 ^ c.idx_last];
        a.hist_eng_stride = (long)e->L * e->C;
        a.dst = (float *)e->X; a.dst_ch_stride = (long)e->ring * e->N; a.ring = e->ring; a.base_slot = c.base_slot;
        a.scale = (float)e->in_scale;
        a.tp = e->pair_tp; a.wide = e->fwd_wide;
        launch_fwd_pair(e->plan2, a, sf);
    } else {
        FwdArgs a;
        a.dst = e->X; a.dst_ch_stride = (long)e->ring * e->N; a.ring = e->ring; a.base_slot = c.base_slot;
        a.n_t = c.tc; a.n_ch = e->GC;
        a.load_scale = 1.0; a.out_scale = e->in_scale; a.zero_first_half = 0; a.interleaved = e->ilv;
        if (p == Path::Direct) {
            a.src = nullptr; a.src_ch_stride = 0; a.prev = nullptr; a.prev_ch_stride = 0;
            a.raw_bytes = e->in_bytes; a.raw = c.d_in; a.raw_eng_stride = c.in_stride / e->in_bytes; a.frame_off = c.frame_off; a.C = e->C;
            a.prev_raw = e->hist_raw[e->curbuf];
            a.save_last = e->tails[c.par][c.idx_last]; a.save_prev = e->tails[c.par][1 ^ c.idx_last];
            a.carry = e->hist_raw[1 ^ c.idx_last];
            a.hist_eng_stride = (long)e->L * e->C;
        } else {
            a.src = e->tin[c.par]; a.src_ch_stride = (long)e->chunk * e->L;
            // the block before this chunk, as the reference sees it: first half of
            // input_timecbuf[n][curbuf] (fftw_convolver.cpp:184 left it there one call earlier)
            a.prev = e->hist[e->curbuf].ptr; a.prev_ch_stride = e->hist[e->curbuf].ch_stride;
        }
        queue_transform_fwd(e, a, sf);
    }
    if (p != Path::Staging) { e->hist_raw[0] = e->tails[c.par][0]; e->hist_raw[1] = e->tails[c.par][1]; }
}

// What the one-transform fused back ends of chunk c take for their overflow statistics and NaN guard.
static InvStats inv_stats(const bfir_engine *e, const Chunk &c)
{
    return InvStats{(float)e->of_max, e->d_of, e->GCo, e->d_bad, c.block_base, e->bad_host_cur};
}

// The rings of the tails in nup_mask for the head chunk that starts at blockcounter, in level order; z_new: beside each its
// second ring during a fade.  Returns their number; the entries past it repeat the first (kernel arguments nothing reads).
static int chunk_rings(const bfir_engine *e, LevelRing (&ring)[BFIR_LEVEL_RINGS], const void **z_new = nullptr)
{
    int nr = 0;
    for (int i = 0; i < e->n_tail; i++) {
        if (!(e->nup_mask >> i & 1)) continue;
        const bfir_engine *t = e->tail[i];
        // a level outside the fade (neither set reaches it, but output queued before it stopped still plays) adds the same to both sums
        if (z_new) z_new[nr] = t->lf_mode ? t->zring2 : t->zring;
        LevelRing &g = ring[nr++];
        g.z = t->zring; g.zlen = g.z_ch_stride = (long)t->zblocks * t->L;
        g.m0 = ((long long)e->blockcounter - e->lv_D[i]) * e->L; g.m_min = t->z_from * (long long)t->L;
        g.m0r = (long)(((g.m0 % g.zlen) + g.zlen) % g.zlen);
    }
    if (!nr) ring[0] = LevelRing{nullptr, 0, 0, 0, 0, 0};
    for (int k = std::max(nr, 1); k < BFIR_LEVEL_RINGS; k++) { ring[k] = ring[0]; if (z_new) z_new[k] = z_new[0]; }
    return nr;
}

// The last output of a matrix engine with an odd output count, beside the pairs below it whose frames are Co floats apart:
// alone through k_inv_lone, with the nr rings (none: a chunk to which no level contributes).
static void queue_inv_lone(bfir_engine *e, const Chunk &c, const LevelRing (&ring)[BFIR_LEVEL_RINGS], int nr, hipStream_t st)
{
    LoneInvArgs a;
    a.ch = e->Co & ~1;
    a.y = (const float *)c.Y + (long)a.ch * e->chunk * e->N;
    for (int k = 0; k < BFIR_LEVEL_RINGS; k++) a.ring[k] = ring[k];
    a.n_rings = nr;
    a.raw = (float *)c.d_out; a.frame_off = c.frame_off;
    a.frame_stride = e->Co; a.n_t = c.tc;
    a.scale = (float)e->out_scale; a.st = inv_stats(e, c);
    launch_inv_lone(e->plan2, a, st);
}

// Product spectra -> the chunk's output blocks: raw frames + overflow statistics (pair, direct) or planar tout (staging).
// The output side counts by Co / GCo where a matrix engine can get (never the staging path).
static void queue_inv(bfir_engine *e, Path p, const Chunk &c, hipStream_t st)
{
    ProfScope ps(e, BFIR_K_INV, st);
    if (p == Path::Pair) {
        InvPairArgs a;
        a.y = (const float *)c.Y; a.y_ch_stride = (long)e->chunk * e->N;
        a.raw = (float *)c.d_out; a.eng_stride = c.out_stride / 4; a.frame_off = c.frame_off;
        a.C = e->Co; a.n_eng = e->n_eng; a.n_t = c.tc;
        a.scale = (float)e->out_scale; a.max = (float)e->of_max;
        a.overflow = e->d_of; a.of_shard_stride = e->GCo; a.bad_block = e->d_bad; a.block_base = c.block_base; a.bad_host = e->bad_host_cur;
        a.tp = e->pair_tp; a.quad = e->inv_quad;
        if (e->matrix && (e->Co & 1)) {
            // the head of a multi-level matrix engine with an odd output count, in a chunk to which no level contributes: the
            // pairs below it through the pair kernel, frames Co floats apart, then the last output alone (k_inv_lone, no ring)
            a.C = e->Co & ~1; a.frame_stride = e->Co;
            LevelRing none[BFIR_LEVEL_RINGS] = {};
            queue_inv_lone(e, c, none, 0, st);
        }
        launch_inv_pair(e->plan2, a, st);
        return;
    }
    InvArgs a;
    a.src = c.Y; a.src_ch_stride = (long)e->chunk * e->N;
    a.n_t = c.tc;
    a.in_scale = e->out_scale; a.full_output = 0; a.interleaved = e->ilv;
    if (p == Path::Direct) {
        a.dst = nullptr; a.dst_ch_stride = 0; a.n_ch = e->GCo;
        a.raw_bytes = e->out_bytes; a.raw = c.d_out; a.raw_eng_stride = c.out_stride / e->out_bytes; a.frame_off = c.frame_off; a.C = e->Co;
        a.max = e->of_max; a.overflow = e->d_of; a.of_shard_stride = e->GCo; a.bad_block = e->d_bad; a.block_base = c.block_base; a.bad_host = e->bad_host_cur;
    } else {
        a.dst = e->tout; a.dst_ch_stride = (long)e->chunk * e->L; a.n_ch = e->GC;
    }
    queue_transform_inv(e, a, st);
}

// staging path, after the inverse transform: planar tout -> raw frames + overflow statistics (+ dither)
// `src`: planar [GCo][..] with src_ch_stride reals per channel -- tout, or a fade's blended scratch (any path: Co channels)
static void queue_stage_out(bfir_engine *e, const Chunk &c, const void *src, long src_ch_stride, hipStream_t st)
{
    ProfScope ps(e, BFIR_K_STAGE_OUT, st);
    StageOutArgs a;
    a.raw = c.d_out; a.eng_stride_bytes = c.out_stride; a.frame_off = c.frame_off;
    a.n_eng = e->n_eng; a.C = e->Co; a.raw_bytes = e->out_bytes; a.spacing = e->Co; a.fmt = e->out_fmt;
    a.n_frames = (long)c.tc * e->L;
    a.src = src; a.src_ch_stride = src_ch_stride;
    a.realsize = e->s; a.L = e->L; a.max = e->of_max;
    a.overflow = e->d_of; a.of_shard_stride = e->GCo; a.bad_block = e->d_bad; a.block_base = c.block_base; a.bad_host = e->bad_host_cur;
    a.dither_tab = e->d_dither_tab; a.dither_size = e->dither_size; a.dither_state = e->d_dither_state;
    // the kernel takes up to BFIR_MAXCHANNELS channels of a frame: the outputs of a wider engine (mimo, one engine, float
    // frames) go in groups of that many, each a channel subset of the Co-wide frame with its own overflow records
    for (int c0 = BFIR_MAXCHANNELS; c0 < e->Co; c0 += BFIR_MAXCHANNELS) {
        StageOutArgs g = a;
        g.C = std::min(BFIR_MAXCHANNELS, e->Co - c0);
        g.raw = (char *)c.d_out + (size_t)c0 * e->out_bytes;
        g.src = (const char *)src + (size_t)c0 * src_ch_stride * e->s;
        g.overflow = e->d_of + c0;
        launch_stage_out(g, st);
    }
    a.C = std::min(BFIR_MAXCHANNELS, e->Co);
    launch_stage_out(a, st);
}

// The fade back end of a chunk whose blocks all fade: Y (old set) and Y2 (new set) -> blended output frames.
static void queue_inv_fade(bfir_engine *e, const Chunk &c, hipStream_t st)
{
    if (e->fade_fused) {   // one inverse per output channel and block, blend, statistics and frame store in one kernel
        ProfScope ps(e, BFIR_K_INV, st);
        FadeInvArgs a;
        a.y_old = (const float *)c.Y; a.y_old_ch_stride = (long)e->chunk * e->N;
        a.y_new = (const float *)c.Y2; a.y_new_ch_stride = c.y2_ch_stride;
        a.raw = (float *)c.d_out; a.frame_off = c.frame_off;
        a.n_ch = e->Co; a.n_t = c.tc;
        a.scale = (float)e->out_scale; a.st = inv_stats(e, c);
        a.f = e->fade_f; a.m0 = c.m0;
        launch_inv_fade(e->plan2, a, st);
        return;
    }
    // the general form: two planar inverses into the fade's own scratch, the blend, then the staging path's output kernel
    const long t_stride = (long)e->ft_blocks * e->L;
    {
        ProfScope ps(e, BFIR_K_INV, st);
        InvArgs a;
        a.n_t = c.tc; a.n_ch = e->GCo;
        a.in_scale = e->out_scale; a.full_output = 0; a.interleaved = e->ilv;
        a.dst_ch_stride = t_stride;
        a.src = c.Y; a.src_ch_stride = (long)e->chunk * e->N; a.dst = e->ft[0];
        queue_transform_inv(e, a, st);
        a.src = c.Y2; a.src_ch_stride = c.y2_ch_stride; a.dst = e->ft[1];
        queue_transform_inv(e, a, st);
        FadeBlendArgs b;
        b.y_old = e->ft[0]; b.y_new = e->ft[1]; b.ch_stride = t_stride;
        b.n_ch = e->GCo; b.n = (long)c.tc * e->L;
        b.f = e->s == 4 ? (double)e->fade_f : e->fade_d; b.m0 = c.m0; b.realsize = e->s;
        launch_fade_blend(b, st);
    }
    queue_stage_out(e, c, e->ft[0], t_stride, st);
}

// The back end of a tail level's chunk (tc tail blocks from block z_next on): planar inverses into the time ring, one per
// stretch between wraps.
// n blocks of product spectra (channel stride y_ch_stride reals) -> tail blocks j .. of a time ring of the level
static void inv_to_ring(bfir_engine *e, const void *Y, long y_ch_stride, void *zring, long long j, int n_blocks, hipStream_t st)
{
    for (int t0 = 0; t0 < n_blocks;) {
        const int slot = (int)((j + t0) % e->zblocks), n = std::min(n_blocks - t0, e->zblocks - slot);
        InvArgs a;
        a.src = (const char *)Y + (size_t)t0 * cbuf_bytes(e); a.src_ch_stride = y_ch_stride;
        a.dst = (char *)zring + (size_t)slot * e->L * e->s; a.dst_ch_stride = (long)e->zblocks * e->L;
        a.n_t = n; a.n_ch = e->GCo;
        a.in_scale = e->out_scale; a.full_output = 0; a.interleaved = e->ilv;
        launch_inv(e->plan, a, st);
        t0 += n;
    }
}

// During a fade (lf_mode, above): up to its last old block the level has run its MAC twice and inverts both products, the
// old set's into its ring and the new set's into the second ring; past it the one product is the new set's.
static void queue_inv_tail(bfir_engine *e, const Chunk &c, hipStream_t st)
{
    ProfScope ps(e, BFIR_K_INV, st);
    inv_to_ring(e, c.Y, (long)e->chunk * e->N, e->lf_mode == 2 ? e->zring2 : e->zring, e->z_next, c.tc, st);
    if (e->lf_mode == 1) inv_to_ring(e, c.Y2, c.y2_ch_stride, e->zring2, e->z_next, c.tc, st);
    e->z_next += c.tc;
    if (e->lf_mode == 1 && e->z_next > e->lf_j1) { tail_swap_sets(e); e->lf_mode = 2; }   // launches take H by value
}

// The back end of a head chunk whose blocks all have the contributions of the tails in nup_mask: Y and their time rings
// -> output frames.  One ring takes the two-level kernels (nup.hip), two or three take those of levels.hip.
static void queue_inv_nup(bfir_engine *e, const Chunk &c, hipStream_t st)
{
    LevelRing ring[BFIR_LEVEL_RINGS];
    const int nr = chunk_rings(e, ring);
    if (e->back_fused) {   // one inverse per channel pair and block, the sum, statistics and frame store in one kernel
        ProfScope ps(e, BFIR_K_INV, st);
        // a matrix engine with an odd output count: the pairs below it, frames Co floats apart, then the last output alone
        const int n_pair = e->Co & ~1;
        if (n_pair < e->Co) queue_inv_lone(e, c, ring, nr, st);
        LevelsInvArgs a;
        a.y = (const float *)c.Y; a.y_ch_stride = (long)e->chunk * e->N;
        for (int k = 0; k < BFIR_LEVEL_RINGS; k++) a.ring[k] = ring[k];
        a.n_rings = nr;
        a.raw = (float *)c.d_out; a.frame_off = c.frame_off;
        a.n_ch = n_pair; a.n_t = c.tc; a.frame_stride = n_pair == e->Co ? 0 : e->Co;
        a.scale = (float)e->out_scale; a.st = inv_stats(e, c);
        launch_inv_levels(e->plan2, a, st);
        return;
    }
    // the general form: a planar inverse into tout, the sum, then the staging path's output kernel
    const long t_stride = (long)e->chunk * e->L;
    {
        ProfScope ps(e, BFIR_K_INV, st);
        InvArgs a;
        a.src = c.Y; a.src_ch_stride = (long)e->chunk * e->N; a.dst = e->tout; a.dst_ch_stride = t_stride;
        a.n_t = c.tc; a.n_ch = e->GCo;
        a.in_scale = e->out_scale; a.full_output = 0; a.interleaved = e->ilv;
        launch_inv(e->plan, a, st);
        LevelsCombineArgs b;
        b.y = e->tout; b.y_ch_stride = t_stride;
        for (int k = 0; k < BFIR_LEVEL_RINGS; k++) b.ring[k] = ring[k];
        b.n_rings = nr;
        b.n_ch = e->GCo; b.n = (long)c.tc * e->L; b.realsize = e->s;
        launch_levels_combine(b, st);
    }
    queue_stage_out(e, c, e->tout, t_stride, st);
}

// The back end of a FADING head chunk of a two- or multi-level engine whose blocks all have the contributions of the tails
// in nup_mask (not empty): Y, Y2 and the two rings of every contributing level -> blended output frames (lfade.hip).
static void queue_inv_lfade(bfir_engine *e, const Chunk &c, hipStream_t st)
{
    LevelRing ring[BFIR_LEVEL_RINGS];
    const void *z_new[BFIR_LEVEL_RINGS];
    const int nr = chunk_rings(e, ring, z_new);
    if (e->fade_fused) {   // one inverse per channel and block, both sums, blend, statistics and frame store in one kernel
        ProfScope ps(e, BFIR_K_INV, st);
        LfadeInvArgs a;
        a.y_old = (const float *)c.Y; a.y_old_ch_stride = (long)e->chunk * e->N;
        a.y_new = (const float *)c.Y2; a.y_new_ch_stride = c.y2_ch_stride;
        for (int k = 0; k < BFIR_LEVEL_RINGS; k++) { a.ring[k] = ring[k]; a.z_new[k] = z_new[k]; }
        a.n_rings = nr;
        a.raw = (float *)c.d_out; a.frame_off = c.frame_off;
        a.n_ch = e->Co; a.n_t = c.tc;                      // a matrix engine: its outputs, an odd count included
        a.scale = (float)e->out_scale; a.st = inv_stats(e, c);
        a.f = e->fade_f; a.m0 = c.m0;
        launch_inv_lfade(e->plan2, a, st);
        return;
    }
    // the general form: two planar inverses into the fade's own scratch, sums and blend, then the staging path's output kernel
    const long t_stride = (long)e->ft_blocks * e->L;
    {
        ProfScope ps(e, BFIR_K_INV, st);
        InvArgs a;
        a.n_t = c.tc; a.n_ch = e->GCo;
        a.in_scale = e->out_scale; a.full_output = 0; a.interleaved = e->ilv;
        a.dst_ch_stride = t_stride;
        a.src = c.Y; a.src_ch_stride = (long)e->chunk * e->N; a.dst = e->ft[0];
        launch_inv(e->plan, a, st);
        a.src = c.Y2; a.src_ch_stride = c.y2_ch_stride; a.dst = e->ft[1];
        launch_inv(e->plan, a, st);
        LfadeSumArgs b;
        b.y_old = e->ft[0]; b.y_new = e->ft[1]; b.ch_stride = t_stride;
        for (int k = 0; k < BFIR_LEVEL_RINGS; k++) { b.ring[k] = ring[k]; b.z_new[k] = z_new[k]; }
        b.n_rings = nr;
        b.n_ch = e->GCo; b.n = (long)c.tc * e->L;
        b.f = e->s == 4 ? (double)e->fade_f : e->fade_d; b.m0 = c.m0; b.realsize = e->s;
        launch_lfade_sum(b, st);
    }
    queue_stage_out(e, c, e->ft[0], t_stride, st);
}

// The staging path's time history, once the chunk is queued (plain or fading: its front is the same): only the
// references move; the samples stay where stage_in put them (this time buffer is not rewritten before chunk k+2, by
// which time both references have moved on).
static void move_staging_history(bfir_engine *e, const Chunk &c)
{
    const long t_stride = (long)e->chunk * e->L;
    const size_t Ls = (size_t)e->L * e->s;
    char *tin = (char *)e->tin[c.par];
    if (c.tc >= 2) { e->hist[1 ^ c.idx_last].ptr = tin + (size_t)(c.tc - 2) * Ls; e->hist[1 ^ c.idx_last].ch_stride = t_stride; }
    e->hist[c.idx_last].ptr = tin + (size_t)(c.tc - 1) * Ls; e->hist[c.idx_last].ch_stride = t_stride;
}

// The schedule, the same on every path.  On the latency path (inline_launch) everything is on st and stream order is
// the only order: no event at all.
static int run_chunk(bfir_engine *e, const void *d_in, long in_stride, void *d_out, long out_stride,
                     long frame_off, int tc, int block_base, hipStream_t st, hipEvent_t input_ready)
{
    int rc = matrix_chunk_ok(e, tc);
    if (rc != BFIR_OK) return rc;
    const Path p = chunk_path(e);
    const int par = (int)(e->chunk_seq & 1);
    Chunk c;
    c.d_in = d_in; c.in_stride = in_stride; c.d_out = d_out; c.out_stride = out_stride;
    c.frame_off = frame_off; c.tc = tc; c.block_base = block_base;
    c.par = par;
    c.base_slot = (int)(e->blockcounter % (unsigned long long)e->ring);
    c.idx_last = 1 ^ e->curbuf ^ ((tc - 1) & 1);
    c.Y = e->Yb[e->pipe3 ? par : 0];
    // run_blocks cut the chunk so that it is all fade or all plain
    c.fade = e->fade_len > 0;
    const bool both = c.fade || e->lf_mode == 1;   // ... or, a tail level of a fading engine, all up to its last old block: both sets
    if (both) { c.Y2 = e->Yf[e->pipe3 ? par : 0]; c.y2_ch_stride = (long)e->yf_blocks * e->N; c.m0 = e->fade_pos * e->L; }
    // a pair list fades: the new set's products from the old set's, wherever both are needed (a uniform engine or the head
    // of a split one while it fades, a tail level up to its last old block)
    const bool patch = both && e->fade_patch;
    const bool duo = both && !patch && chunk_takes_duo(e);
    if (duo) { rc = matrix_fade_chunk_ok(e, tc); if (rc != BFIR_OK) return rc; }
    if (patch) { rc = patch_chunk_ok(e, tc); if (rc != BFIR_OK) return rc; }
    rc = chunk_aligned(e, p, c);
    if (rc != BFIR_OK) return rc;
    if (c.fade && e->fade_fused && (((uintptr_t)d_out | (uintptr_t)out_stride) & 3)) {
        bfir_logf("bfir engine: frame buffers must be aligned to their sample size.");
        return BFIR_ERR_ARG;
    }
    const bool il = e->inline_launch;
    hipStream_t sf = (e->serial || il) ? st : e->s_front;
    hipStream_t sm = (e->pipe3 && !il) ? e->s_mac : st;

    // the front only waits for the input, never for the back of the chunk before
    if (input_ready) HIP_TRY(hipStreamWaitEvent(sf, input_ready, 0));
    if (p == Path::Staging) queue_stage_in(e, c, sf);   // does not touch the ring: ahead of the wait, it may overlap mac(k-2)
    if (!il && e->chunk_seq >= 2) HIP_TRY(hipStreamWaitEvent(sf, e->ev_mac[par], 0));   // mac(k-2) is done with the ring
    queue_fwd(e, p, c, sf);
    if (!il) {
        HIP_TRY(hipEventRecord(e->ev_fwd[par], sf));
        HIP_TRY(hipStreamWaitEvent(sm, e->ev_fwd[par], 0));
        if (e->pipe3 && e->chunk_seq >= 2) HIP_TRY(hipStreamWaitEvent(sm, e->ev_inv[par], 0));   // inv(k-2) has read Yb[par]
    }
    if (patch && (e->mlevels || e->nup_tail)) {   // the old set's MAC and the patch behind it, or k_wpatch: a span per launch
        if ((rc = queue_mac_patch(e, c.base_slot, c.Y, (long)e->chunk * e->N, c.Y2, c.y2_ch_stride, tc, sm, true)) != BFIR_OK) return rc;
    } else {
        ProfScope ps(e, BFIR_K_MAC, sm);
        if (duo) {   // a multi-level matrix engine: both sets in one pass over the delay line
            if ((rc = queue_duo(e, c.base_slot, c.Y, c.Y2, c.y2_ch_stride, tc, sm)) != BFIR_OK) return rc;
        }
        else if (patch) {   // a uniform engine: the old set's MAC and the patch behind it, one span
            if ((rc = queue_mac_patch(e, c.base_slot, c.Y, (long)e->chunk * e->N, c.Y2, c.y2_ch_stride, tc, sm, false)) != BFIR_OK) return rc;
        }
        else if ((rc = queue_mac(e, c.base_slot, c.Y, (long)e->chunk * e->N, tc, false, sm)) != BFIR_OK) return rc;
        // the same delay line through the same kernels with the new set, behind the first
        if (both && !duo && !patch && (rc = queue_mac(e, c.base_slot, c.Y2, c.y2_ch_stride, tc, true, sm)) != BFIR_OK) return rc;
    }
    if (!il) {
        HIP_TRY(hipEventRecord(e->ev_mac[par], sm));
        if (e->pipe3) HIP_TRY(hipStreamWaitEvent(st, e->ev_mac[par], 0));
    }
    if (c.fade && e->nup_mask) queue_inv_lfade(e, c, st);
    else if (c.fade) queue_inv_fade(e, c, st);
    else if (e->nup_tail) queue_inv_tail(e, c, st);
    else if (e->nup_mask) queue_inv_nup(e, c, st);
    else queue_inv(e, p, c, st);
    if (e->pipe3 && !il) HIP_TRY(hipEventRecord(e->ev_inv[par], st));
    if (p == Path::Staging) {
        if (!c.fade) queue_stage_out(e, c, e->tout, (long)e->chunk * e->L, st);
        move_staging_history(e, c);
    }
    e->curbuf ^= (tc & 1);
    e->blockcounter += (unsigned long long)tc;
    e->chunk_seq += 1;
    if (c.fade) {
        e->fade_pos += tc;
        if (e->fade_pos >= e->fade_len) fade_swap_sets(e);   // the last fade block is queued: launches take H by value
    }
    return BFIR_OK;
}

// The fade's work buffers, sized for the chunks it can be cut into: min(chunk, fade_len) blocks (the head, a uniform or a
// matrix engine), or for the launches of a tail level of a fading engine: its chunk, and no planar scratch.
static int ensure_fade_buffers(bfir_engine *e)
{
    const int want = e->nup_tail ? e->chunk : std::min(e->chunk, e->fade_len);
    const bool need_ft = !e->fade_fused && !e->nup_tail;
    if (e->yf_blocks >= want && (!need_ft || e->ft_blocks >= want)) return BFIR_OK;
    HIP_TRY(hipDeviceSynchronize());   // queued fade chunks may still use the old ones
    for (int i = 0; i < 2; i++) {
        if (e->Yf[i]) (void)hipFree(e->Yf[i]);
        if (e->ft[i]) (void)hipFree(e->ft[i]);
        e->Yf[i] = e->ft[i] = nullptr;
    }
    e->yf_blocks = e->ft_blocks = 0;
    for (int i = 0; i < (e->pipe3 ? 2 : 1); i++) HIP_TRY(hipMalloc(&e->Yf[i], (size_t)e->GCo * want * cbuf_bytes(e)));
    e->yf_blocks = want;
    if (need_ft) {
        for (int i = 0; i < 2; i++) HIP_TRY(hipMalloc(&e->ft[i], (size_t)e->GCo * want * e->L * e->s));
        e->ft_blocks = want;
    }
    return BFIR_OK;
}

// ---------------------------------------------------------------------------
// crossfaded coefficient change on a two-level or multi-level engine (the schedule: bfir_engine, "lf_mode")
// ---------------------------------------------------------------------------
// floor(a / b), b > 0
static long long floor_div(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// Catch-up: the blocks a level has run with the old set that the fade's first head block, or a later one, reads under
// the new set -- their MAC again, with the new set alone, on the delay line the level still holds, into the second ring.
// A level that restarted mid-stream less than that many blocks ago (bfir_engine_set_coeff_levels) has only those since,
// the ones before read as zero under the new set.  Then the level's place in the lf_mode schedule.
// A pair list (patch): the new set's products are the old set's plus the listed pairs' difference here too, as in every
// launch of the fade that takes both sets -- the old set's MAC of those blocks again into the level's product buffer (the
// chain that produced them: the same bits) and the patch behind it.
static int lfade_catch_up(bfir_engine *e, int fade_blocks, const LevelSplit &sp, bool patch)
{
    const long long a_f = (long long)e->blockcounter;
    for (int i = 0; i < e->n_tail; i++) {
        bfir_engine *t = e->tail[i];
        if (!e->lv_active[i]) continue;
        const int r = e->lv_r[i];
        int rc = ensure_fade_buffers(t);
        if (rc != BFIR_OK) return rc;
        HIP_TRY(hipMemsetAsync(t->zring2, 0, (size_t)t->GCo * t->zblocks * t->L * t->s, e->stream));
        long long j0 = std::max(t->z_from, floor_div(a_f - e->lv_D[i], r));
        j0 = std::max(j0, t->z_next - std::min<long long>((long long)t->blockcounter, t->ring_extra));
        const long yf_stride = (long)t->yf_blocks * t->N;
        for (long long j = j0; j < t->z_next;) {
            const int n = (int)std::min<long long>(t->z_next - j, t->yf_blocks);
            const long long bc = (long long)t->blockcounter - (t->z_next - j);   // the level's own count of block j
            if (patch) rc = queue_mac_patch(t, (int)(bc % t->ring), t->Yb[0], (long)t->chunk * t->N, t->Yf[0], yf_stride, n, e->stream, false);
            else rc = queue_mac(t, (int)(bc % t->ring), t->Yf[0], yf_stride, n, true, e->stream);
            if (rc != BFIR_OK) return rc;   // a matrix level: checked before anything changed, not reached
            inv_to_ring(t, t->Yf[0], yf_stride, t->zring2, j, n, e->stream);
            j += n;
        }
        t->lf_j1 = floor_div(a_f + fade_blocks - 1 - e->lv_D[i], r);
        t->lf_stop = sp.lv[i + 1].nb_max == 0;
        t->lf_mode = 1;
        if (t->z_next > t->lf_j1) { tail_swap_sets(t); t->lf_mode = 2; }   // every old block the fade reads has run
    }
    return BFIR_OK;
}

// The listed filters of a pairs call on a multi-level matrix engine, split at every D_k (spl: row j of it is filter
// list[j] = o C + i), merged into the active set's counts: nb and nb_max of every level of the merged set.  No rows.
static LevelSplit merged_counts(const bfir_engine *e, const LevelSplit &spl, const std::vector<int> &list)
{
    LevelSplit sp;
    for (int k = 0; k <= e->n_tail; k++) {
        LevelSplit::Level &s = sp.lv[k];
        s.nb = level(e, k)->nblk;
        for (size_t j = 0; j < list.size(); j++) s.nb[list[j]] = spl.lv[k].nb[j];
        for (int nb : s.nb) s.nb_max = std::max(s.nb_max, nb);
    }
    return sp;
}

// The crossfade of a two-level, multi-level or multi-level matrix engine: the split of set_coeff_split into H2 of every
// level, the catch-up, and the head's fade as a uniform engine's.
// list (bfir_engine_set_coeff_matrix_levels_pairs_fade): `rows` are the listed filters alone, row j the new filter list[j] =
// o C + i, and the new set is the active one with those replaced.  Every level's H2 is its H copied and the listed rows'
// part loaded, its table goes to its d_patch, and the launches that take both sets patch (fade_patch).
static int set_coeff_split_fade(bfir_engine *e, const SplitSource &src, int fade_blocks, const std::vector<int> *list = nullptr)
{
    int rc = source_check_lengths(e, src);
    if (rc == BFIR_OK) rc = check_fade_args(e, fade_blocks);
    if (rc != BFIR_OK) return rc;
    for (int n = 0; src.rows && n < src.rows->n_required; n++) if (!src.rows->taps[n]) return BFIR_ERR_ARG;
    const LevelSplit spl = source_split(e, src);
    const LevelSplit sp = list ? merged_counts(e, spl, *list) : spl;
    for (int i = 0; i < e->n_tail; i++) {
        // a level the old set does not reach runs no forward transforms: it has no delay line to fade on (per level, not
        // per filter: a filter of a matrix engine that is new on a running level fades in)
        if (sp.lv[i + 1].nb_max > 0 && !e->lv_active[i]) {
            bfir_logf("bfir engine: the new filters reach level %d, the active ones do not: load the first set zero-padded to the "
                      "longest length that will be faded to.", i + 1);
            return BFIR_ERR_UNSUPPORTED;
        }
    }
    // a NaN / Inf tap at any level is refused before anything is uploaded at any level: the engine keeps running the old set
    rc = source_check_rows(e, src);
    if (rc != BFIR_OK) return rc;
    // the catch-up's launches (up to a tail's chunk) must fit the matrix MAC's grid: refused before anything changes
    for (int i = 0; i < e->n_tail; i++)
        if (e->lv_active[i]) {
            rc = matrix_chunk_ok(e->tail[i], e->tail[i]->chunk);
            if (rc == BFIR_OK && list) rc = patch_chunk_ok(e->tail[i], e->tail[i]->chunk);
            if (rc != BFIR_OK) return rc;
        }
    HIP_TRY(hipSetDevice(e->device));
    // queued work may still read what was H before the last fade's swap, and the catch-up below reads the delay lines: the
    // device is idle from here to the end of the call
    HIP_TRY(hipDeviceSynchronize());
    const size_t n_rows = list ? (size_t)e->Co * e->C : source_size(src);
    rc = fade_prepare(e, (int)n_rows);
    if (rc != BFIR_OK) return rc;
    void *gather[BFIR_MAX_LEVELS] = {};   // bank entries: the levels of the one gather behind the loop; a skipped level is not among them
    for (int k = 0; k <= e->n_tail; k++) {
        bfir_engine *l = level(e, k);
        const LevelSplit::Level &s = sp.lv[k];
        if (k > 0 && !e->lv_active[k - 1]) continue;
        l->nblk2 = s.nb;
        if (list) {
            // the level's store copied on the stream that writes the listed rows and so ordered before them: the level's own
            // where they are loaded, the head's where the one gather behind the loop copies them
            HIP_TRY(hipMemcpyAsync(l->H2, l->H, n_rows * l->B * cbuf_bytes(l), hipMemcpyDeviceToDevice, src.rows ? l->stream : e->stream));
            if (!src.rows) gather[k] = l->H2;
            else rc = load_listed_rows(l, l->H2, spl.lv[k].rows, spl.lv[k].nb, *list, src.scale);
            if (rc == BFIR_OK) rc = patch_table_set(l, *list);
            if (rc != BFIR_OK) return rc;
        } else if (s.nb_max > 0) {
            if (!src.rows) gather[k] = l->H2;
            else rc = load_filters(l, l->H2, 0, s.rows, s.nb_max, src.scale);
            if (rc != BFIR_OK) return rc;
        } else {
            // The new set does not reach the level.  A matrix engine: every count 0, its products with the new set are stored
            // as zeros.  A diagonal engine: one all-zero partition, so its products with the new set are zero.
            HIP_TRY(hipMemset(l->H2, 0, n_rows * l->B * cbuf_bytes(l)));
            if (!e->matrix) l->nblk2.assign(n_rows, 1);
        }
        rc = upload_counts(l, true);
        if (rc != BFIR_OK) return rc;
    }
    if (!src.rows) { rc = source_gather(e, gather, src, list); if (rc != BFIR_OK) return rc; }
    if (e->matrix) {
        // Front end: a level pairs channels only while every input is read under BOTH sets (an input is read if any filter of
        // its column has taps on any level); after the fade the new set decides (fade_swap_sets, lfade_finish).  The head of an
        // engine without taps beyond D_1 and an odd output count is direct, as bfir_engine_set_coeff_matrix_levels has it.
        const bool read_old = every_input_read(e, [&](int k, int n) { return level(e, k)->nblk[n]; });
        const bool read_new = every_input_read(e, [&](int k, int n) { return sp.lv[k].nb[n]; });
        bool tail_old = false, tail_new = false;
        for (int i = 0; i < e->n_tail; i++) { tail_old = tail_old || e->lv_active[i]; tail_new = tail_new || sp.lv[i + 1].nb_max > 0; }
        for (int i = 0; i < e->n_tail; i++) {
            bfir_engine *t = e->tail[i];
            t->pair_new = read_new;
            if (t->pair_cap) matrix_take_path(t, read_old && read_new);
        }
        if (e->pair_cap) {
            const bool odd = (e->Co & 1) != 0;
            e->pair_new = read_new && !(odd && !tail_new);
            matrix_take_path(e, e->pair_new && read_old && !(odd && !tail_old));
        }
    }
    rc = lfade_catch_up(e, fade_blocks, sp, list != nullptr);
    if (rc != BFIR_OK) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipGetLastError());
    fade_begin(e, fade_blocks);
    if (list) {   // behind fade_begin, which clears it; every way the fade ends clears it again (fade_swap_sets, lfade_finish)
        e->fade_patch = true;
        for (int i = 0; i < e->n_tail; i++) e->tail[i]->fade_patch = e->lv_active[i];
        bfir_logf("bfir matrix engine: crossfade of %d pairs over %d blocks on %d levels; a launch that needs both sets runs %s.",
                  (int)list->size(), fade_blocks, e->n_tail + 1,
                  chunk_takes_wpatch(e) ? "k_wpatch" : (e->mimo_mac ? "k_mac_mimo and k_patch_pairs" : "k_mac_matrix and k_patch_pairs"));
    } else if (e->matrix)
        bfir_logf("bfir matrix engine: crossfade over %d blocks on %d levels; a launch that needs both sets runs %s.", fade_blocks,
                  e->n_tail + 1, chunk_takes_duo(e) ? (e->mimo_mac ? "k_wduo" : "k_mac_duo") : (e->mimo_mac ? "k_mac_mimo twice" : "k_mac_matrix twice"));
    return BFIR_OK;
}

extern "C" int bfir_engine_set_coeff_nup_fade(bfir_engine *e, const void *const *coeffs, int n_coeffs, int length, double scale,
                                              int fade_blocks)
{
    if (!e) return BFIR_ERR_ARG;
    if (!e->nup || e->levels || e->mlevels) return BFIR_ERR_UNSUPPORTED;
    if (!coeffs || n_coeffs < 0) return BFIR_ERR_ARG;
    const FilterRows rows = diagonal_rows(e, coeffs, n_coeffs, length);
    return set_coeff_split_fade(e, taps_source(rows, scale), fade_blocks);
}

extern "C" int bfir_engine_set_coeff_levels_fade(bfir_engine *e, const void *const *coeffs, int n_coeffs, int length, double scale,
                                                 int fade_blocks)
{
    if (!e) return BFIR_ERR_ARG;
    if (!e->levels) return BFIR_ERR_UNSUPPORTED;
    if (!coeffs || n_coeffs < 0) return BFIR_ERR_ARG;
    const FilterRows rows = diagonal_rows(e, coeffs, n_coeffs, length);
    return set_coeff_split_fade(e, taps_source(rows, scale), fade_blocks);
}

// every filter of its own length, partition counts per filter and level, and the front-end rule of
// bfir_engine_set_coeff_matrix_fade
extern "C" int bfir_engine_set_coeff_matrix_levels_fade(bfir_engine *e, const void *const *coeffs, const int *lengths, double scale,
                                                        int fade_blocks)
{
    if (!e) return BFIR_ERR_ARG;
    if (!e->mlevels) return BFIR_ERR_UNSUPPORTED;
    if (!coeffs || !lengths) return BFIR_ERR_ARG;
    const FilterRows rows = matrix_rows(e, coeffs, lengths, 0);
    return set_coeff_split_fade(e, taps_source(rows, scale), fade_blocks);
}

// ---------------------------------------------------------------------------
// a list of (output, input) pairs of a multi-level matrix or mimo engine replaced:
// bfir_engine_set_coeff_matrix_levels_pairs, _pairs_fade
// ---------------------------------------------------------------------------
// What both calls ask of their list, every filter of its own length; host arithmetic alone.
static int pairs_list_levels(const bfir_engine *e, int n_pairs, const int *outputs, const int *inputs, const void *const *coeffs,
                             const int *lengths, PairList &pl)
{
    if (!lengths) return BFIR_ERR_ARG;
    const int rc = pairs_list(e, n_pairs, outputs, inputs, coeffs, lengths, 0, pl);
    return rc != BFIR_OK ? rc : check_split_lengths(e, pl.rows);   // no length negative, none past the taps the levels hold
}

// The listed rows (row j of the source is filter list[j] = o C + i, the list checked) of the active set replaced on every level
static int set_pairs_split(bfir_engine *e, const SplitSource &src, const std::vector<int> &list)
{
    // nothing to patch; or a fade: a tail past its last old block already runs the new set, there is no ONE active set
    if (!bfir_engine_is_initialized(e) || e->fade_len > 0) return BFIR_ERR_STATE;
    int rc = source_check_rows(e, src);                         // a NaN / Inf tap: the engine keeps its filters and stays initialised
    if (rc != BFIR_OK) return rc;
    const LevelSplit spl = source_split(e, src);
    const LevelSplit sp = merged_counts(e, spl, list);
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    void *gather[BFIR_MAX_LEVELS] = {};
    for (int k = 0; k <= e->n_tail; k++) {
        bfir_engine *l = level(e, k);
        int nb_old = 0;
        for (int nb : l->nblk) nb_old = std::max(nb_old, nb);
        // a level the active set does not reach was not loaded by the set call (set_coeff_split): its store reads as zeros
        // before the first listed row goes in, as load_filters leaves the rows of the whole matrix
        if (nb_old == 0 && sp.lv[k].nb_max > 0) HIP_TRY(hipMemset(l->H, 0, l->nblk.size() * l->B * cbuf_bytes(l)));
        if (!src.rows) gather[k] = l->H;                        // a listed entry that does not reach the level: its row cleared, as below
        else rc = load_listed_rows(l, l->H, spl.lv[k].rows, spl.lv[k].nb, list, src.scale);
        if (rc != BFIR_OK) return rc;
        l->nblk = sp.lv[k].nb;
        rc = upload_counts(l, false);
        if (rc != BFIR_OK) return rc;
    }
    if (!src.rows) { rc = source_gather(e, gather, src, &list); if (rc != BFIR_OK) return rc; }
    return split_counts_set(e, sp);
}

extern "C" int bfir_engine_set_coeff_matrix_levels_pairs(bfir_engine *e, int n_pairs, const int *outputs, const int *inputs,
                                                         const void *const *coeffs, const int *lengths, double scale)
{
    if (!e) return BFIR_ERR_ARG;
    if (!e->mlevels) return BFIR_ERR_UNSUPPORTED;
    PairList pl;
    const int rc = pairs_list_levels(e, n_pairs, outputs, inputs, coeffs, lengths, pl);
    if (rc != BFIR_OK) return rc;
    return set_pairs_split(e, taps_source(pl.rows, scale), pl.row);
}

extern "C" int bfir_engine_set_coeff_matrix_levels_pairs_fade(bfir_engine *e, int n_pairs, const int *outputs, const int *inputs,
                                                              const void *const *coeffs, const int *lengths, double scale,
                                                              int fade_blocks)
{
    if (!e) return BFIR_ERR_ARG;
    if (!e->mlevels) return BFIR_ERR_UNSUPPORTED;
    PairList pl;
    const int rc = pairs_list_levels(e, n_pairs, outputs, inputs, coeffs, lengths, pl);
    if (rc != BFIR_OK) return rc;
    return set_coeff_split_fade(e, taps_source(pl.rows, scale), fade_blocks, &pl.row);
}

// ---------------------------------------------------------------------------
// coefficient banks of a multi-level matrix or mimo engine: one store per level in the form of that level's H, loaded through
// the level split (bfir_engine_levels_bank_create, _load), and the four set calls with bank entries in place of host taps
// (bfir_engine_set_coeff_matrix_levels_bank, _bank_fade, _pairs_bank, _pairs_bank_fade): set_coeff_split, set_coeff_split_fade
// and set_pairs_split with a SplitSource of entries, ONE k_lbank_gather launch (lbank.hip) for all levels where the calls
// with taps upload and transform level by level
// ---------------------------------------------------------------------------
extern "C" int bfir_engine_levels_bank_create(bfir_engine *e, int n_entries)
{
    if (!e) return BFIR_ERR_ARG;
    if (!e->mlevels) return BFIR_ERR_UNSUPPORTED;
    if (n_entries < 1) return BFIR_ERR_ARG;
    if (e->bank) return BFIR_ERR_STATE;
    HIP_TRY(hipSetDevice(e->device));
    for (int k = 0; k <= e->n_tail; k++) {
        bfir_engine *l = level(e, k);
        if (hipMalloc(&l->bank, (size_t)n_entries * l->B * cbuf_bytes(l)) == hipSuccess) continue;
        (void)hipGetLastError();
        l->bank = nullptr;
        for (int j = 0; j < k; j++) { (void)hipFree(level(e, j)->bank); level(e, j)->bank = nullptr; }   // no bank is left
        return BFIR_ERR_HIP;
    }
    e->lbank_len.assign((size_t)n_entries, 0);                 // every entry empty; the stores themselves are not cleared
    e->lbank_nb.assign((size_t)n_entries * BFIR_MAX_LEVELS, 0);
    return BFIR_OK;
}

extern "C" int bfir_engine_levels_bank_destroy(bfir_engine *e)
{
    if (!e) return BFIR_ERR_ARG;
    if (!e->mlevels) return BFIR_ERR_UNSUPPORTED;
    if (!e->bank) return BFIR_OK;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    for (int k = 0; k <= e->n_tail; k++) { (void)hipFree(level(e, k)->bank); level(e, k)->bank = nullptr; }
    e->lbank_len.clear(); e->lbank_nb.clear();
    return BFIR_OK;
}

extern "C" int bfir_engine_levels_bank_entries(const bfir_engine *e)
{
    if (!e) return BFIR_ERR_ARG;
    if (!e->mlevels) return BFIR_ERR_UNSUPPORTED;
    return (int)e->lbank_len.size();
}

extern "C" int bfir_engine_levels_bank_length(const bfir_engine *e, int entry)
{
    if (!e) return BFIR_ERR_ARG;
    if (!e->mlevels) return BFIR_ERR_UNSUPPORTED;
    if (entry < 0 || (size_t)entry >= e->lbank_len.size()) return BFIR_ERR_ARG;
    return e->lbank_len[entry];
}

extern "C" int bfir_engine_levels_bank_blocks(const bfir_engine *e, int entry, int level)
{
    if (!e) return BFIR_ERR_ARG;
    if (!e->mlevels) return BFIR_ERR_UNSUPPORTED;
    if (entry < 0 || (size_t)entry >= e->lbank_len.size() || level < 0 || level > e->n_tail) return BFIR_ERR_ARG;
    return e->lbank_nb[(size_t)entry * BFIR_MAX_LEVELS + level];
}

extern "C" int bfir_engine_levels_bank_load(bfir_engine *e, int first, int n, const void *const *coeffs, const int *lengths,
                                            double scale)
{
    if (!e) return BFIR_ERR_ARG;
    if (!e->mlevels) return BFIR_ERR_UNSUPPORTED;
    if (!coeffs || !lengths || n < 1 || first < 0) return BFIR_ERR_ARG;
    FilterRows rows((size_t)n);
    for (int k = 0; k < n; k++) { rows.taps[k] = coeffs[k]; rows.len[k] = coeffs[k] ? lengths[k] : 0; }
    int rc = check_split_lengths(e, rows);
    if (rc != BFIR_OK) return rc;
    if (!e->bank) return BFIR_ERR_STATE;
    if ((size_t)first + (size_t)n > e->lbank_len.size()) return BFIR_ERR_ARG;
    // a NaN / Inf tap anywhere is refused before anything is uploaded: the bank is unchanged
    rc = check_rows(e, rows, SIZE_MAX, scale);
    if (rc != BFIR_OK) return rc;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());                            // the stores are written on an idle device
    for (int k = 0; k < n; k++) {                               // a failed load leaves them empty
        e->lbank_len[first + k] = 0;
        for (int lv = 0; lv < BFIR_MAX_LEVELS; lv++) e->lbank_nb[(size_t)(first + k) * BFIR_MAX_LEVELS + lv] = 0;
    }
    // the split of set_coeff_split, and per level its one load: an entry is on every level the row that
    // bfir_engine_set_coeff_matrix_levels writes for the same taps, length and scale
    const LevelSplit sp = split_rows(e, rows);
    for (int lv = 0; lv <= e->n_tail; lv++) {
        bfir_engine *l = level(e, lv);
        if (sp.lv[lv].nb_max == 0) continue;                    // none of the n filters reaches the level: nothing transformed, counts 0
        rc = load_filters(l, l->bank, first, sp.lv[lv].rows, sp.lv[lv].nb_max, scale);
        if (rc != BFIR_OK) return rc;
    }
    for (int k = 0; k < n; k++) {
        e->lbank_len[first + k] = rows.len[k];
        for (int lv = 0; lv <= e->n_tail; lv++) e->lbank_nb[(size_t)(first + k) * BFIR_MAX_LEVELS + lv] = sp.lv[lv].nb[k];
    }
    return BFIR_OK;
}

extern "C" int bfir_engine_levels_bank_read(bfir_engine *e, int entry, int level, int block, void *dst)
{
    if (!e) return BFIR_ERR_ARG;
    if (!e->mlevels) return BFIR_ERR_UNSUPPORTED;
    if (!dst || level < 0 || level > e->n_tail) return BFIR_ERR_ARG;
    bfir_engine *l = level ? e->tail[level - 1] : e;
    if (block < 0 || block >= l->B) return BFIR_ERR_ARG;
    if (!e->bank) return BFIR_ERR_STATE;
    if (entry < 0 || (size_t)entry >= e->lbank_len.size()) return BFIR_ERR_ARG;
    if (block >= e->lbank_nb[(size_t)entry * BFIR_MAX_LEVELS + level]) {   // what a gather writes there: zeros at and past the count
        memset(dst, 0, cbuf_bytes(l));
        return BFIR_OK;
    }
    return read_store_spectrum(l, l->bank, entry, block, dst);
}

// The four calls.  pairs: a list (outputs, inputs, entries of n), else the whole matrix (entries[o C + i]); fade_blocks of a
// fade.  The refusals of the list and of the bank come first, then those of the call with taps in its own order.
static int set_coeff_lbank(bfir_engine *e, bool pairs, int n, const int *outputs, const int *inputs, const int *entries, bool fade,
                           int fade_blocks)
{
    if (!e) return BFIR_ERR_ARG;
    if (!e->mlevels) return BFIR_ERR_UNSUPPORTED;
    if (!entries || (pairs && (!outputs || !inputs || n < 1))) return BFIR_ERR_ARG;
    if (!e->bank) return BFIR_ERR_STATE;
    BankList bl;
    int rc = pairs ? coeff_tables::list_rows(e->Co, e->C, n, outputs, inputs, bl.row) : BFIR_OK;
    if (rc == BFIR_OK) rc = coeff_tables::check_entries(e->lbank_len, pairs ? n : e->Co * e->C, entries, bl.ent);   // 0 = empty
    if (rc != BFIR_OK) return rc;
    // the gather's own limits (alignment, a partition of whole 16 bytes, rows, grid), before anything is touched or launched
    void *stores[BFIR_MAX_LEVELS] = {};
    for (int k = 0; k <= e->n_tail; k++) stores[k] = level(e, k)->H;
    LBankArgs ga = lbank_args(e, stores);
    ga.n_rows = (int)bl.ent.size();
    if (!lbank_gather_supported(ga)) return BFIR_ERR_UNSUPPORTED;
    SplitSource src;
    src.ent = &bl.ent;
    if (fade) return set_coeff_split_fade(e, src, fade_blocks, pairs ? &bl.row : nullptr);
    return pairs ? set_pairs_split(e, src, bl.row) : set_coeff_split(e, src);
}

extern "C" int bfir_engine_set_coeff_matrix_levels_bank(bfir_engine *e, const int *entries)
{
    return set_coeff_lbank(e, false, 0, nullptr, nullptr, entries, false, 0);
}

extern "C" int bfir_engine_set_coeff_matrix_levels_bank_fade(bfir_engine *e, const int *entries, int fade_blocks)
{
    return set_coeff_lbank(e, false, 0, nullptr, nullptr, entries, true, fade_blocks);
}

extern "C" int bfir_engine_set_coeff_matrix_levels_pairs_bank(bfir_engine *e, int n_pairs, const int *outputs, const int *inputs,
                                                              const int *entries)
{
    return set_coeff_lbank(e, true, n_pairs, outputs, inputs, entries, false, 0);
}

extern "C" int bfir_engine_set_coeff_matrix_levels_pairs_bank_fade(bfir_engine *e, int n_pairs, const int *outputs,
                                                                   const int *inputs, const int *entries, int fade_blocks)
{
    return set_coeff_lbank(e, true, n_pairs, outputs, inputs, entries, true, fade_blocks);
}

// The four mix calls (bfir_engine_set_coeff_matrix_levels_bank_mix, _bank_mix_fade, _pairs_bank_mix, _pairs_bank_mix_fade):
// set_coeff_lbank with n_terms (entry, weight) terms per row in place of one entry, a SplitSource of mix records and ONE
// k_lbank_mix launch (lbankmix.hip) for all levels.  The refusals of the list, the terms and the bank come first, then the
// launch's own, then those of the call with taps in its own order.
static int set_coeff_lbank_mix(bfir_engine *e, bool pairs, int n, const int *outputs, const int *inputs, int n_terms,
                               const int *entries, const double *weights, bool fade, int fade_blocks)
{
    if (!e) return BFIR_ERR_ARG;
    if (!e->mlevels) return BFIR_ERR_UNSUPPORTED;
    if (!entries || !weights || (pairs && (!outputs || !inputs || n < 1))) return BFIR_ERR_ARG;
    if (n_terms < 1 || n_terms > BFIR_BANK_MIX_TERMS) return BFIR_ERR_ARG;
    if (!e->bank) return BFIR_ERR_STATE;
    BankList bl;
    std::vector<int> nb;
    const std::vector<int> *list = pairs ? &bl.row : nullptr;
    int rc = pairs ? coeff_tables::list_rows(e->Co, e->C, n, outputs, inputs, bl.row) : BFIR_OK;
    if (rc == BFIR_OK) rc = coeff_tables::level_mix_records(e->lbank_len, e->lbank_nb, e->n_tail + 1, e->s, list,
                                                            pairs ? n : e->Co * e->C, n_terms, entries, weights, bl.mix, nb);
    if (rc != BFIR_OK) return rc;
    // the launch's own limits (alignment, a partition of whole 16 bytes, rows, grid), before anything is touched or launched
    void *stores[BFIR_MAX_LEVELS] = {};
    for (int k = 0; k <= e->n_tail; k++) stores[k] = level(e, k)->H;
    LBankMixArgs ma = lbank_mix_args(e, stores);
    ma.n_rows = (int)(bl.mix.size() / BFIR_LBANK_MIX_REC);
    if (!lbank_mix_supported(ma)) return BFIR_ERR_UNSUPPORTED;
    for (int k = 0; k <= e->n_tail; k++) if (level(e, k)->s != e->s) return BFIR_ERR_UNSUPPORTED;   // one weight, one precision
    SplitSource src;
    src.mix = &bl.mix; src.mix_nb = &nb;
    if (fade) return set_coeff_split_fade(e, src, fade_blocks, list);
    return pairs ? set_pairs_split(e, src, bl.row) : set_coeff_split(e, src);
}

extern "C" int bfir_engine_set_coeff_matrix_levels_bank_mix(bfir_engine *e, int n_terms, const int *entries, const double *weights)
{
    return set_coeff_lbank_mix(e, false, 0, nullptr, nullptr, n_terms, entries, weights, false, 0);
}

extern "C" int bfir_engine_set_coeff_matrix_levels_bank_mix_fade(bfir_engine *e, int n_terms, const int *entries,
                                                                 const double *weights, int fade_blocks)
{
    return set_coeff_lbank_mix(e, false, 0, nullptr, nullptr, n_terms, entries, weights, true, fade_blocks);
}

extern "C" int bfir_engine_set_coeff_matrix_levels_pairs_bank_mix(bfir_engine *e, int n_pairs, const int *outputs, const int *inputs,
                                                                  int n_terms, const int *entries, const double *weights)
{
    return set_coeff_lbank_mix(e, true, n_pairs, outputs, inputs, n_terms, entries, weights, false, 0);
}

extern "C" int bfir_engine_set_coeff_matrix_levels_pairs_bank_mix_fade(bfir_engine *e, int n_pairs, const int *outputs,
                                                                       const int *inputs, int n_terms, const int *entries,
                                                                       const double *weights, int fade_blocks)
{
    return set_coeff_lbank_mix(e, true, n_pairs, outputs, inputs, n_terms, entries, weights, true, fade_blocks);
}

extern "C" int bfir_engine_fade_remaining_levels(const bfir_engine *e)
{
    if (!e) return BFIR_ERR_ARG;
    if (!e->nup) return BFIR_ERR_UNSUPPORTED;
    return e->fade_len > 0 ? e->fade_len - e->fade_pos : 0;
}

// The frames of head blocks [lo, hi) of this call (the head block at frame_off is call0) -> pbuf, but for those that
// this call has put there already.  [lo, hi) lies in one block of the largest level.
static int nup_keep(bfir_engine *e, const void *d_in, long frame_off, long long call0, long long lo, long long hi, hipStream_t st,
                    hipEvent_t input_ready)
{
    lo = std::max(lo, std::max(call0, e->pbuf_upto));
    if (lo >= hi) return BFIR_OK;
    const size_t fb = (size_t)e->C * e->in_bytes;   // bytes per input frame
    if (!e->inline_launch && input_ready) HIP_TRY(hipStreamWaitEvent(st, input_ready, 0));
    HIP_TRY(hipMemcpyAsync((char *)e->pbuf + (size_t)(lo % e->lv_r[e->n_tail - 1]) * e->L * fb,
                           (const char *)d_in + ((size_t)frame_off + (size_t)(lo - call0) * e->L) * fb, (size_t)(hi - lo) * e->L * fb,
                           hipMemcpyDefault, st));
    e->pbuf_upto = hi;
    return BFIR_OK;
}

// Two- and multi-level engines, ahead of head chunk [a0, a0 + *tc) (a0 = blockcounter): run, level after level, every
// block of the level that is complete with head block a0 + *tc - 1 and not yet run, then cut the chunk so that its blocks
// all have the same set of contributing levels (nup_mask).  A block that lies wholly in this call's buffer is transformed
// straight from the caller's frames -- neighbours in one launch -- and the one that began in an earlier call from pbuf,
// where nup_keep_partial put its first frames; all of a call's input is there when the call is made, so chunks need not
// be cut at multiples of any r.  A tail's front and MAC run on the tail's own streams, its inverse on st: stream order keeps
// every ring's writes ahead of this chunk's back end and behind the reads of the chunks before.
static int nup_tail_ahead(bfir_engine *e, const void *d_in, long frame_off, long long call0, int *tc, hipStream_t st,
                          hipEvent_t input_ready)
{
    const long long a0 = (long long)e->blockcounter, a1 = a0 + *tc;
    const size_t fb = (size_t)e->C * e->in_bytes;   // bytes per input frame
    const int r_last = e->lv_r[e->n_tail - 1];
    for (int i = 0; i < e->n_tail; i++) {
        bfir_engine *t = e->tail[i];
        const int r = e->lv_r[i];
        t->inline_launch = e->inline_launch;
        if (!e->lv_active[i]) continue;
        for (const long long j_end = a1 / r; t->z_next < j_end;) {
            const long long j = t->z_next;
            if (t->lf_mode == 1) { const int rc = ensure_fade_buffers(t); if (rc != BFIR_OK) return rc; }
            if (j * r < call0) {   // began before this call: the rest of its frames join the ones kept in pbuf
                int rc = nup_keep(e, d_in, frame_off, call0, j * r, (j + 1) * r, st, input_ready);
                if (rc != BFIR_OK) return rc;
                if (!e->inline_launch) HIP_TRY(hipEventRecord(e->ev_nup, st));
                rc = run_chunk(t, (const char *)e->pbuf + (size_t)((j * r) % r_last) * e->L * fb, 0, nullptr, 0, 0, 1, 0, st,
                               e->inline_launch ? nullptr : e->ev_nup);
                if (rc != BFIR_OK) return rc;
            } else {
                int nt = (int)std::min<long long>(j_end - j, t->chunk);
                if (t->lf_mode == 1) nt = (int)std::min<long long>(nt, t->lf_j1 - j + 1);   // a launch's blocks are all of one kind
                const int rc = run_chunk(t, d_in, 0, nullptr, 0, frame_off + (long)(j * r - call0) * e->L, nt, 0, st, input_ready);
                if (rc != BFIR_OK) return rc;
            }
        }
    }
    // head block a reads block (a - D_k / L) / r of level k: there from z_from on, and (a stopped level) up to z_next
    auto mask = [&](long long a) {
        int m = 0;
        for (int i = 0; i < e->n_tail; i++) {
            const bfir_engine *t = e->tail[i];
            const long long d = a - e->lv_D[i];
            if (d >= 0 && d / e->lv_r[i] >= t->z_from && d / e->lv_r[i] < t->z_next) m |= 1 << i;
        }
        return m;
    };
    e->nup_mask = mask(a0);
    int same = 1;
    while (same < *tc && mask(a0 + same) == e->nup_mask) same++;
    *tc = same;
    return BFIR_OK;
}

// ... and at the end of a call: the frames of the blocks that are still arriving go to pbuf, because the caller's
// buffer is gone when the rest of them comes.
static int nup_keep_partial(bfir_engine *e, const void *d_in, long frame_off, long long call0, int n, hipStream_t st,
                            hipEvent_t input_ready)
{
    const long long hi = call0 + n;
    long long lo = hi;
    for (int i = 0; i < e->n_tail; i++)
        if (e->lv_active[i]) lo = std::min(lo, e->tail[i]->z_next * e->lv_r[i]);
    return nup_keep(e, d_in, frame_off, call0, lo, hi, st, input_ready);
}

// n blocks of the caller's buffers (from frame frame_off, block block_base of the call), cut into chunks of at most
// e->chunk blocks and at the end of a fade, so that a chunk is all fade or all plain.
static int run_blocks(bfir_engine *e, const void *d_in, long in_stride, void *d_out, long out_stride, long frame_off, int n,
                      int block_base, hipStream_t st, hipEvent_t input_ready)
{
    const long long call0 = (long long)e->blockcounter;   // the head block at frame_off (two-level engines)
    if (e->mlevels) {   // every level's MAC must take its longest launch of this call: refused before anything is queued
        int rc = matrix_chunk_ok(e, std::min(e->chunk, n));
        for (int i = 0; i < e->n_tail && rc == BFIR_OK; i++) rc = matrix_chunk_ok(e->tail[i], std::min(e->tail[i]->chunk, n));
        if (rc == BFIR_OK && e->fade_len > 0) {   // ... and, fading, the launches that take both sets (a pair list: the patch)
            auto both_ok = [&](const bfir_engine *l) {
                const int tc = std::min(l->chunk, n);
                return l->fade_patch ? patch_chunk_ok(l, tc) : matrix_fade_chunk_ok(l, tc);
            };
            rc = both_ok(e);
            for (int i = 0; i < e->n_tail && rc == BFIR_OK; i++)
                if (e->tail[i]->lf_mode == 1) rc = both_ok(e->tail[i]);
        }
        if (rc != BFIR_OK) return rc;
    }
    for (int c0 = 0; c0 < n;) {
        int tc = std::min(e->chunk, n - c0);
        if (e->nup) {
            const int rc = nup_tail_ahead(e, d_in, frame_off, call0, &tc, st, input_ready);
            if (rc != BFIR_OK) return rc;
        }
        if (e->fade_len > 0) {
            const int rc = ensure_fade_buffers(e);
            if (rc != BFIR_OK) return rc;
            tc = std::min(tc, std::min(e->fade_len - e->fade_pos, e->yf_blocks));
        }
        if (e->inline_launch) e->bad_host_cur = e->h_bad + block_base + c0;   // the NaN verdict of block t lands in h_bad[t]
        const int rc = run_chunk(e, d_in, in_stride, d_out, out_stride, frame_off + (long)c0 * e->L, tc, block_base + c0, st,
                                 c0 == 0 ? input_ready : nullptr);
        if (rc != BFIR_OK) return rc;
        c0 += tc;
    }
    if (e->nup) return nup_keep_partial(e, d_in, frame_off, call0, n, st, input_ready);
    return BFIR_OK;
}

// ---------------------------------------------------------------------------
// Per-channel input and output delays (delay.cpp:27-140, 148-265, 552-600; kernels in delay.hip)
// ---------------------------------------------------------------------------
static int delay_channels(const bfir_engine *e, int side) { return side == BFIR_DELAY_INPUT ? e->C : e->Co; }
static int delay_sample_bytes(const bfir_engine *e, int side) { return side == BFIR_DELAY_INPUT ? e->in_bytes : e->out_bytes; }
static bool delay_side_ok(int side) { return side == BFIR_DELAY_INPUT || side == BFIR_DELAY_OUTPUT; }

// The side's table as its kernels read it: the delays, which channels have a filter, the filters.  The device is idle.
static int delay_upload(bfir_engine *e, int side, const int *delay, const int *sub)
{
    bfir_engine::DelaySide &d = e->dly[side];
    const int n_taps = 2 * d.h + 1, C = delay_channels(e, side);
    std::vector<unsigned char> host(sizeof(DelayTab) + (size_t)BFIR_DELAY_CH * n_taps * e->s, 0);
    DelayTab *tab = (DelayTab *)host.data();
    for (int c = 0; c < C; c++) {
        tab->delay[c] = delay[c];
        tab->sub[c] = sub[c] != 0;
        if (sub[c] != 0) {
            const int rc = bfir_subdelay_filter(d.h, sub[c], d.steps, d.beta, e->s, host.data() + sizeof(DelayTab) + (size_t)c * n_taps * e->s);
            if (rc != BFIR_OK) return rc;
        }
    }
    HIP_TRY(hipMemcpy(d.d_tab, host.data(), host.size(), hipMemcpyHostToDevice));
    d.delay.assign(delay, delay + C);
    d.sub.assign(sub, sub + C);
    return BFIR_OK;
}

extern "C" int bfir_engine_delay_init(bfir_engine *e, int side, int max_delay, int step_count, int half_filter_length,
                                      double kaiser_beta)
{
    if (!e || !delay_side_ok(side) || max_delay < 0 || max_delay > (1 << 24) || step_count < 0 || step_count == 1) return BFIR_ERR_ARG;
    if (step_count >= 2 && (half_filter_length < 1 || half_filter_length > 128)) return BFIR_ERR_ARG;
    if (e->n_eng > 1 || e->mimo) return BFIR_ERR_UNSUPPORTED;   // batches; a mimo engine (DelayTab holds BFIR_DELAY_CH channels)
    if (step_count >= 2 && !fmt_is_native(side == BFIR_DELAY_INPUT ? e->in_fmt : e->out_fmt)) return BFIR_ERR_UNSUPPORTED;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    e->async_pending = false;
    delay_free(e, side);
    bfir_engine::DelaySide &d = e->dly[side];
    d.max_delay = max_delay; d.steps = step_count; d.h = step_count >= 2 ? half_filter_length : 0; d.beta = kaiser_beta;
    d.H = (long)max_delay + 2 * d.h;
    const size_t hist_bytes = (size_t)std::max(1L, d.H) * delay_channels(e, side) * delay_sample_bytes(e, side);
    const size_t tab_bytes = sizeof(DelayTab) + (size_t)BFIR_DELAY_CH * (2 * d.h + 1) * e->s;
    bool ok = hipMalloc(&d.hist[0], hist_bytes) == hipSuccess && hipMalloc(&d.hist[1], hist_bytes) == hipSuccess &&
              hipMalloc(&d.d_tab, tab_bytes) == hipSuccess;
    ok = ok && hipMemset(d.hist[0], 0, hist_bytes) == hipSuccess && hipMemset(d.hist[1], 0, hist_bytes) == hipSuccess;
    ok = ok && (e->ev_dly || hipEventCreateWithFlags(&e->ev_dly, hipEventDisableTiming) == hipSuccess);
    ok = ok && (e->ev_dly_done || hipEventCreateWithFlags(&e->ev_dly_done, hipEventDisableTiming) == hipSuccess);
    const std::vector<int> zero(BFIR_DELAY_CH, 0);
    int rc = ok ? delay_upload(e, side, zero.data(), zero.data()) : BFIR_ERR_HIP;
    if (rc == BFIR_OK && hipDeviceSynchronize() != hipSuccess) rc = BFIR_ERR_HIP;
    if (rc != BFIR_OK) { (void)hipGetLastError(); delay_free(e, side); return rc; }
    d.on = true;
    bfir_logf("bfir engine: %s delays up to %d frames%s.", side == BFIR_DELAY_INPUT ? "input" : "output", max_delay,
              d.steps ? " and a sub-sample stage" : "");
    return BFIR_OK;
}

extern "C" int bfir_engine_set_delay(bfir_engine *e, int side, const int *delay, const int *subdelay, int n_channels)
{
    if (!e || !delay || !delay_side_ok(side)) return BFIR_ERR_ARG;
    if (e->mimo) return BFIR_ERR_UNSUPPORTED;
    bfir_engine::DelaySide &d = e->dly[side];
    if (!d.on) return BFIR_ERR_STATE;
    if (n_channels != delay_channels(e, side)) return BFIR_ERR_ARG;
    std::vector<int> sub(BFIR_DELAY_CH, 0);
    for (int c = 0; c < n_channels; c++) {
        if (delay[c] < 0 || delay[c] > d.max_delay) return BFIR_ERR_ARG;
        sub[c] = subdelay ? subdelay[c] : 0;   // no array: whole samples
        if (sub[c] != 0 && (d.steps < 2 || sub[c] <= -d.steps || sub[c] >= d.steps)) return BFIR_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());   // launches already queued read the table as it is
    e->async_pending = false;
    return delay_upload(e, side, delay, sub.data());
}

extern "C" int bfir_engine_get_delay(const bfir_engine *e, int side, int *delay, int *subdelay, int n_channels)
{
    if (!e || !delay || !subdelay || !delay_side_ok(side)) return BFIR_ERR_ARG;
    if (e->mimo) return BFIR_ERR_UNSUPPORTED;
    const bfir_engine::DelaySide &d = e->dly[side];
    if (!d.on) return BFIR_ERR_STATE;
    if (n_channels != delay_channels(e, side)) return BFIR_ERR_ARG;
    for (int c = 0; c < n_channels; c++) { delay[c] = d.delay[c]; subdelay[c] = d.sub[c]; }
    return BFIR_OK;
}

extern "C" int bfir_engine_delay_latency(const bfir_engine *e, int side)
{
    if (!e || !delay_side_ok(side)) return BFIR_ERR_ARG;
    if (e->mimo) return BFIR_ERR_UNSUPPORTED;
    return e->dly[side].on ? e->dly[side].h : 0;
}

// bfir_engine_reset: both histories read as silence again, the settings stay (the device is idle)
static void delay_reset(bfir_engine *e)
{
    for (int side = 0; side < 2; side++) {
        bfir_engine::DelaySide &d = e->dly[side];
        if (!d.on) continue;
        const size_t bytes = (size_t)std::max(1L, d.H) * delay_channels(e, side) * delay_sample_bytes(e, side);
        for (void *h : d.hist) (void)hipMemset(h, 0, bytes);
    }
}

// One piece of a side: src (n frames, raw) -> the delayed frames in dst, and the next history.
static void queue_delay(bfir_engine *e, int side, const void *src, void *dst, long n, hipStream_t st)
{
    bfir_engine::DelaySide &d = e->dly[side];
    const int C = delay_channels(e, side), sb = delay_sample_bytes(e, side);
    const DelayTab *tab = (const DelayTab *)d.d_tab;
    // the next history: the last H frames of hist || src, into the other buffer
    DelayCopyArgs up;
    up.dst = d.hist[1 ^ d.cur]; up.piece = src; up.hist = d.hist[d.cur]; up.n_frames = d.H; up.m0 = n - d.H; up.H = d.H;
    up.C = C; up.sample_bytes = sb; up.tab = nullptr;
    if (d.steps >= 2) {
        DelaySubArgs a;
        a.dst = dst; a.piece = src; a.hist = d.hist[d.cur]; a.n_frames = n; a.H = d.H;
        a.C = C; a.sample_bytes = sb; a.realsize = e->s; a.h = d.h;
        a.tab = tab; a.taps = (const char *)d.d_tab + sizeof(DelayTab);
        launch_delay_sub(a, st);
        launch_delay_copy(up, nullptr, st);
    } else {   // whole samples: the piece and the history update in one launch
        DelayCopyArgs a;
        a.dst = dst; a.piece = src; a.hist = d.hist[d.cur]; a.n_frames = n; a.m0 = 0; a.H = d.H;
        a.C = C; a.sample_bytes = sb; a.tab = tab;
        launch_delay_copy(a, d.H > 0 ? &up : nullptr, st);
    }
    if (d.H > 0) d.cur ^= 1;
}

// run_blocks with a delayed side: the call in pieces of at most e->chunk blocks; per piece the input kernels on st, ahead
// of the event the front waits for, the engine proper between the two scratch buffers, and the output kernels on st behind
// the back end (every chunk's inverse and frame store run on st, after st has waited for that chunk's MAC and so for its
// front: a piece's launches have all read the input scratch before the next piece's input kernels overwrite it).
static int run_blocks_delayed(bfir_engine *e, const void *d_in, long in_stride, void *d_out, long out_stride, int n, int block_base,
                              hipStream_t st, hipEvent_t input_ready)
{
    bfir_engine::DelaySide &di = e->dly[BFIR_DELAY_INPUT], &dout = e->dly[BFIR_DELAY_OUTPUT];
    const size_t fin = (size_t)e->C * e->in_bytes, fout = (size_t)e->Co * e->out_bytes;
    const size_t want[2] = {(size_t)e->chunk * e->L * fin, (size_t)e->chunk * e->L * fout};
    for (int side = 0; side < 2; side++) {   // the work buffers grew (ensure_chunk): so does the scratch
        bfir_engine::DelaySide &d = e->dly[side];
        if (!d.on || d.scratch_bytes >= want[side]) continue;
        HIP_TRY(hipDeviceSynchronize());
        if (d.scratch) (void)hipFree(d.scratch);
        d.scratch = nullptr; d.scratch_bytes = 0;
        HIP_TRY(hipMalloc(&d.scratch, want[side]));
        d.scratch_bytes = want[side];
    }
    // a caller that changes streams between calls: the histories and the scratch are the last call's until its launches end
    if (e->dly_stream && e->dly_stream != st && !e->inline_launch) HIP_TRY(hipStreamWaitEvent(st, e->ev_dly_done, 0));
    for (int c0 = 0; c0 < n;) {
        const int tc = std::min(e->chunk, n - c0);
        const void *src = (const char *)d_in + (size_t)c0 * e->L * fin;
        void *dst = (char *)d_out + (size_t)c0 * e->L * fout;
        // Every piece is a run_blocks call of its own, and a tail level's first front of a call runs on that level's own
        // stream, which has waited for nothing yet: with the input side off every piece gets the caller's event (a wait on
        // an event that has passed costs nothing), with it on the event recorded behind this piece's input kernels.
        hipEvent_t ready = input_ready;
        if (di.on) {
            if (ready) HIP_TRY(hipStreamWaitEvent(st, ready, 0));
            queue_delay(e, BFIR_DELAY_INPUT, src, di.scratch, (long)tc * e->L, st);
            src = di.scratch;
            ready = nullptr;
            if (!e->inline_launch) { HIP_TRY(hipEventRecord(e->ev_dly, st)); ready = e->ev_dly; }
        }
        const int rc = run_blocks(e, src, in_stride, dout.on ? dout.scratch : dst, out_stride, 0, tc, block_base + c0, st, ready);
        if (rc != BFIR_OK) return rc;
        if (dout.on) queue_delay(e, BFIR_DELAY_OUTPUT, dout.scratch, dst, (long)tc * e->L, st);
        c0 += tc;
    }
    e->dly_stream = nullptr;   // the latency path ends with its stream idle: nothing is left to wait for
    if (!e->inline_launch) { HIP_TRY(hipEventRecord(e->ev_dly_done, st)); e->dly_stream = st; }
    return BFIR_OK;
}

// the engine proper, behind its delays where a side has them
static int run_call(bfir_engine *e, const void *d_in, long in_stride, void *d_out, long out_stride, int n, int block_base,
                    hipStream_t st, hipEvent_t input_ready)
{
    if (e->dly[0].on || e->dly[1].on) return run_blocks_delayed(e, d_in, in_stride, d_out, out_stride, n, block_base, st, input_ready);
    return run_blocks(e, d_in, in_stride, d_out, out_stride, 0, n, block_base, st, input_ready);
}

// What the work buffers of a big engine's default chunk may take: the delay line, both Yb and the three time buffers.
// Its blocks are long, so launches of a few hundred of them already fill the GPU; bfir_engine_set_chunk can ask for more.
static constexpr size_t kBigWorkBytes = 8ull << 30;

static int ensure_chunk(bfir_engine *e, int n_blocks)
{
    // automatic: as many blocks per launch as give a launch the work of 4096 blocks of the 8-channel, 4096-sample
    // headline shape (measured best for long jobs, profiles/r01_bench_chunk_sweep.jsonl) -- small engines need longer
    // launches to keep the three kernels of the pipeline overlapped (the stereo plug-in shape: +12 % fp64 / +19 % fp32
    // at 32768 blocks per launch against 4096, profiles/r03_chunk.txt) -- between 4096 and 32768, less when the
    // delay line of that many blocks would pass 4 GiB (many channels or engines)
    int limit = e->want_chunk;
    if (limit <= 0) {
        const long slots = (long)((4ull << 30) / ((size_t)e->GC * cbuf_bytes(e)));
        long want = (8L * 4096 * 4096) / ((long)e->GC * e->L);
        want = std::max(4096L, std::min(32768L, want));
        limit = (int)std::max(16L, std::min(want, (slots - e->B) / 2));
        if (e->matrix) {
            // the input ring and the output products separately: each Yb of n_out spectra per block within 4 GiB too,
            // and the work per launch counted by the wider side
            const int wide = std::max(e->C, e->Co);
            const long yslots = (long)((4ull << 30) / ((size_t)e->Co * cbuf_bytes(e)));
            want = std::max(4096L, std::min(32768L, (8L * 4096 * 4096) / ((long)wide * e->L)));
            limit = (int)std::max(16L, std::min(std::min(want, (slots - e->B) / 2), yslots));
        }
    }
    // HP-TPDF dither is a recursion over a channel's samples (dither.hip: one lane walks them in order), so a
    // launch's length is its run time: bound it (64 blocks: the serial walk stays in the milliseconds and the
    // other kernels of the pipeline get the GPU in between; integer outputs are off the measured path)
    if (e->d_dither_tab) limit = std::min(limit, 64);
    if (e->big && e->want_chunk <= 0) {
        // a chunk of c blocks holds 2 c + B delay-line slots, two Yb of c spectra (4 c + B spectra of N reals) and three time
        // buffers of c blocks of L reals (1.5 c spectra): the most blocks that keep all of them within kBigWorkBytes
        const long spectra = (long)(kBigWorkBytes / ((size_t)e->GC * cbuf_bytes(e)));
        limit = (int)std::max(1L, std::min((long)limit, (2 * (spectra - e->B)) / 11));
    }
    const int want = std::max(1, std::min(limit, n_blocks));
    if (e->big && want > e->chunk) {
        // the MAC kernels and the transforms index one channel's delay line and products with 32-bit element counts here
        // and there, and launch_mac / launch_*_big would skip a launch whose grid does not fit: refused before anything
        // is allocated or queued
        const unsigned long long ring = 2ull * want + e->B;
        if (ring * (unsigned long long)e->N >= (1ull << 31) || !big_launch_fits(e->bplan, want, e->GC)) {
            bfir_logf("bfir engine: %d blocks of %d per launch are past the kernels' 32-bit indexing.", want, e->L);
            return BFIR_ERR_UNSUPPORTED;
        }
    }
    // a mimo engine: a launch past k_mac_mimo's grid is refused here, before anything is allocated or queued
    if (e->mimo_mac && want > e->chunk) { const int rc = matrix_chunk_ok(e, want); if (rc != BFIR_OK) return rc; }
    // ... and on a multi-level mimo engine one past the grid of any level's MAC, the fading form included
    if (e->mimo && e->mlevels && want > e->chunk) {
        for (int k = 0; k <= e->n_tail; k++) {
            const bfir_engine *l = level(e, k);
            const int lw = k == 0 ? want : (want + e->lv_r[k - 1] - 1) / e->lv_r[k - 1];
            int rc = matrix_chunk_ok(l, lw);
            if (rc == BFIR_OK && (k == 0 ? e->fade_len > 0 : l->lf_mode == 1)) rc = matrix_fade_chunk_ok(l, lw);
            if (rc != BFIR_OK) return rc;
        }
    }
    if (want > e->chunk) {
        const int rc = alloc_work(e, want);
        if (rc != BFIR_OK || !e->nup) return rc;
        // a tail's launches take its blocks of one head chunk; its ring what that chunk can still need
        for (int i = 0; i < e->n_tail; i++) {
            const int tw = (want + e->lv_r[i] - 1) / e->lv_r[i];
            if (tw > e->tail[i]->chunk) { const int rc2 = alloc_work(e->tail[i], tw); if (rc2 != BFIR_OK) return rc2; }
            const int rc3 = alloc_zring(e, i, want);
            if (rc3 != BFIR_OK) return rc3;
        }
        return BFIR_OK;
    }
    return BFIR_OK;
}

extern "C" int bfir_engine_run_device(bfir_engine *e, const void *d_in, int64_t in_stride_bytes,
                                      void *d_out, int64_t out_stride_bytes, int n_blocks, void *hip_stream)
{
    if (!e || !d_in || !d_out || n_blocks < 0) return BFIR_ERR_ARG;
    if (!bfir_engine_is_initialized(e)) return BFIR_ERR_STATE;
    if (n_blocks == 0) return BFIR_OK;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : e->stream;
    int rc = ensure_chunk(e, n_blocks);
    if (rc != BFIR_OK) return rc;
    // whatever produced d_in on the caller's stream must be done before the front reads it
    HIP_TRY(hipEventRecord(e->ev_entry, st));
    rc = run_call(e, d_in, in_stride_bytes, d_out, out_stride_bytes, n_blocks, 0, st, e->ev_entry);
    if (rc != BFIR_OK) return rc;
    HIP_TRY(hipGetLastError());
    e->async_pending = true;
    return BFIR_OK;
}

extern "C" int bfir_engine_sync(bfir_engine *e)
{
    if (!e) return BFIR_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    e->async_pending = false;
    drain_spans(e);
    int bad = INT_MAX;
    HIP_TRY(hipMemcpy(&bad, e->d_bad, sizeof(int), hipMemcpyDeviceToHost));
    if (bad != 0x7f7f7f7f) {
        HIP_TRY(hipMemset(e->d_bad, 0x7f, sizeof(int)));
        bfir_logf("NaN or Inf values in the system! Invalid input? Aborting.\n");
        return BFIR_ERR_NONFINITE;
    }
    return BFIR_OK;
}

// memcpy between the caller's (pageable) buffers and the pinned staging buffers, split over a few
// threads when it is large: one core moves ~9 GB/s, the host link 63 GB/s.
static void copy_host(void *dst, const void *src, size_t n)
{
    constexpr size_t kMinPerThread = 4u << 20;
    unsigned hw = std::thread::hardware_concurrency();
    size_t nt = std::min<size_t>(std::min<size_t>(hw ? hw : 1, 8), n / kMinPerThread);
    if (nt <= 1) { memcpy(dst, src, n); return; }
    const size_t per = ((n / nt) + 4095) & ~(size_t)4095;
    std::vector<std::thread> th;
    for (size_t i = 1; i < nt; i++) {
        const size_t o = i * per;
        if (o >= n) break;
        th.emplace_back([=]() { memcpy((char *)dst + o, (const char *)src + o, std::min(per, n - o)); });
    }
    memcpy(dst, src, std::min(per, n));
    for (auto &t : th) t.join();
}

// Is [p, p + n) page-locked host memory the copy engines can reach directly (bfir_pinned_malloc, or the caller's own
// hipHostMalloc / hipHostRegister)?  Then the staging memcpy -- one pass of a few host cores over every byte, the slowest leg
// of the host-pointer path -- is skipped for that buffer.
static bool is_pinned_host(const void *p, size_t n)
{
    hipPointerAttribute_t a0, a1;
    if (hipPointerGetAttributes(&a0, p) != hipSuccess) { (void)hipGetLastError(); return false; }   // pageable: not known to the runtime
    if (a0.type != hipMemoryTypeHost) return false;
    if (n <= 1) return true;
    if (hipPointerGetAttributes(&a1, (const char *)p + n - 1) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a1.type == hipMemoryTypeHost;
}

extern "C" void *bfir_pinned_malloc(size_t size)
{
    void *p = nullptr;
    if (bfir_device_count() <= 0) return nullptr;
    if (hipHostMalloc(&p, size ? size : 1, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}

extern "C" void bfir_pinned_free(void *p)
{
    if (p) (void)hipHostFree(p);
}

// Host-path chunk: the link, not the GPU, bounds this path, so the pinned staging buffers stay small.
static int host_chunk(const bfir_engine *e) { return std::min(e->chunk, 512); }

static int ensure_staging(bfir_engine *e, int min_blocks = 0)
{
    const int hc = std::max(host_chunk(e), min_blocks);
    const size_t bin = (size_t)e->n_eng * hc * e->L * e->C * e->in_bytes;
    const size_t bout = (size_t)e->n_eng * hc * e->L * e->Co * e->out_bytes;
    if (e->stage_bytes_in >= bin && e->stage_bytes_out >= bout) return BFIR_OK;
    free_staging(e);
    for (int i = 0; i < 2; i++) {
        HIP_TRY(hipHostMalloc(&e->pin_in[i], bin, hipHostMallocDefault));
        HIP_TRY(hipHostMalloc(&e->pin_out[i], bout, hipHostMallocDefault));
        HIP_TRY(hipMalloc(&e->dev_in[i], bin));
        HIP_TRY(hipMalloc(&e->dev_out[i], bout));
    }
    e->stage_bytes_in = bin; e->stage_bytes_out = bout;
    return BFIR_OK;
}

// A handful of blocks per call -- the plug-in's pattern is ONE (foo_dsp_bfir.cpp:311-349): what
// counts is the latency of the call, not throughput.  No copy engine, no second stream, no event: the
// caller's frames go into the pinned staging buffer, the kernels read them from there and write the output
// frames into the other one straight across the host link (a block is a few KiB), launched back to back on
// one stream; one 4-byte copy brings the NaN verdict; one stream synchronise ends the call.
static constexpr int kSmallRun = 4;

// 16 bytes per lane between pinned host memory and HBM (whole cache lines across the host link)
__global__ __launch_bounds__(256) void k_copy16(uint4 *__restrict__ dst, const uint4 *__restrict__ src, long n16)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n16) dst[i] = src[i];
}

static void copy16(void *dst, const void *src, size_t bytes, hipStream_t st)
{
    const long n16 = (long)(bytes / 16);
    hipLaunchKernelGGL(k_copy16, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, st, (uint4 *)dst, (const uint4 *)src, n16);
}

static int run_small(bfir_engine *e, const void *inbuf, void *outbuf, int n_blocks)
{
    int rc = ensure_chunk(e, n_blocks);
    if (rc != BFIR_OK) return rc;
    rc = ensure_staging(e, kSmallRun);
    if (rc != BFIR_OK) return rc;
    if (e->async_pending) { HIP_TRY(hipDeviceSynchronize()); e->async_pending = false; }
    if (!e->h_bad) { HIP_TRY(hipHostMalloc((void **)&e->h_bad, sizeof(int) * kSmallRun, hipHostMallocDefault)); }
    for (int t = 0; t < kSmallRun; t++) e->h_bad[t] = 0;
    const size_t per_in = (size_t)n_blocks * e->L * e->C * e->in_bytes, per_out = (size_t)n_blocks * e->L * e->Co * e->out_bytes;
    memcpy(e->pin_in[0], inbuf, per_in * e->n_eng);       // engine after engine, n_blocks * L frames each: same layout
    // Frames wider than what one workgroup of the fused FFT kernels consumes (a channel pair or one channel of
    // many): every workgroup would pull its 8 bytes of each frame across the host link on its own (measured:
    // 26 us per FFT kernel for one block of the 8-channel headline shape, against 8 us for stereo frames).
    // Those engines get the block into HBM and out of it by a copy kernel moving whole lines: two more
    // launches, ~35 us less per call.
    const bool bounce = (e->pair || e->direct) && ((size_t)e->C * e->in_bytes > 8 || (e->matrix && (size_t)e->Co * e->out_bytes > 8)) &&
                        !getenv("BFIR_NO_BOUNCE");
    const void *src = e->pin_in[0];
    void *dst = e->pin_out[0];
    if (bounce) {
        copy16(e->dev_in[0], e->pin_in[0], per_in * e->n_eng, e->stream);
        src = e->dev_in[0]; dst = e->dev_out[0];
    }
    e->inline_launch = true;
    rc = run_call(e, src, (long)per_in, dst, (long)per_out, n_blocks, 0, e->stream, nullptr);   // the work buffers hold e->chunk blocks
    e->bad_host_cur = nullptr;
    e->inline_launch = false;
    if (rc != BFIR_OK) return rc;
    if (bounce) copy16(e->pin_out[0], e->dev_out[0], per_out * e->n_eng, e->stream);
    // no copy of the verdict: the kernels flagged bad blocks in pinned host memory themselves (one 4-byte copy was a blit
    // kernel of 3.5 us plus its launch, a tenth of the call)
    HIP_TRY(hipStreamSynchronize(e->stream));
    drain_spans(e);
    memcpy(outbuf, e->pin_out[0], per_out * e->n_eng);
    bool bad = false;
    for (int t = 0; t < n_blocks; t++) bad = bad || e->h_bad[t] != 0;
    if (bad) {
        HIP_TRY(hipMemset(e->d_bad, 0x7f, sizeof(int)));
        bfir_logf("NaN or Inf values in the system! Invalid input? Aborting.\n");
        return BFIR_ERR_NONFINITE;
    }
    return BFIR_OK;
}

// Host-pointer run: pinned double buffers, H2D on s_in, kernels on the engine's
// streams, D2H on s_out, so the copies of neighbouring chunks overlap the compute
// (the reference's raw2real / real2raw staging, fftw_convolver.cpp:156-185, 405-466,
// turned into pinned-host staging).
extern "C" int bfir_engine_run(bfir_engine *e, const void *inbuf, void *outbuf, int n_blocks)
{
    if (!e || !inbuf || !outbuf || n_blocks < 0) return BFIR_ERR_ARG;
    if (!bfir_engine_is_initialized(e)) return BFIR_ERR_STATE;
    if (n_blocks == 0) return BFIR_OK;
    HIP_TRY(hipSetDevice(e->device));
    if (n_blocks <= kSmallRun && !getenv("BFIR_NO_SMALL_RUN")) return run_small(e, inbuf, outbuf, n_blocks);
    int rc = ensure_chunk(e, std::min(n_blocks, 512));   // see host_chunk()
    if (rc != BFIR_OK) return rc;
    rc = ensure_staging(e);
    if (rc != BFIR_OK) return rc;
    const size_t fin = (size_t)e->C * e->in_bytes, fout = (size_t)e->Co * e->out_bytes;  // bytes per frame
    const size_t eng_in = (size_t)n_blocks * e->L * fin, eng_out = (size_t)n_blocks * e->L * fout;
    const int hc = host_chunk(e);
    const int nchunks = (n_blocks + hc - 1) / hc;
    // page-locked caller buffers go straight to / from the copy engines (no staging memcpy); BFIR_NO_PINNED_DIRECT=1: A/B, tests
    const bool direct_ok = !getenv("BFIR_NO_PINNED_DIRECT");
    const bool in_direct = direct_ok && is_pinned_host(inbuf, eng_in * e->n_eng);
    const bool out_direct = direct_ok && is_pinned_host(outbuf, eng_out * e->n_eng);
    auto copy_out = [&](int k) -> int {
        const int b = k & 1, c0 = k * hc, tc = std::min(hc, n_blocks - c0);
        HIP_TRY(hipEventSynchronize(e->ev_d2h[b]));
        if (out_direct) return BFIR_OK;
        const size_t per = (size_t)tc * e->L * fout;
        for (int g = 0; g < e->n_eng; g++)
            copy_host((char *)outbuf + g * eng_out + (size_t)c0 * e->L * fout, (char *)e->pin_out[b] + g * per, per);
        return BFIR_OK;
    };
    for (int k = 0; k < nchunks; k++) {
        const int b = k & 1, c0 = k * hc, tc = std::min(hc, n_blocks - c0);
        if (k >= 2) { rc = copy_out(k - 2); if (rc != BFIR_OK) return rc; }
        const size_t per_in = (size_t)tc * e->L * fin, per_out = (size_t)tc * e->L * fout;
        if (in_direct) {
            for (int g = 0; g < e->n_eng; g++)
                HIP_TRY(hipMemcpyAsync((char *)e->dev_in[b] + g * per_in, (const char *)inbuf + g * eng_in + (size_t)c0 * e->L * fin,
                                       per_in, hipMemcpyHostToDevice, e->s_in));
        } else {
            for (int g = 0; g < e->n_eng; g++)
                copy_host((char *)e->pin_in[b] + g * per_in, (const char *)inbuf + g * eng_in + (size_t)c0 * e->L * fin, per_in);
            HIP_TRY(hipMemcpyAsync(e->dev_in[b], e->pin_in[b], per_in * e->n_eng, hipMemcpyHostToDevice, e->s_in));
        }
        HIP_TRY(hipEventRecord(e->ev_h2d[b], e->s_in));
        rc = run_call(e, e->dev_in[b], (long)per_in, e->dev_out[b], (long)per_out, tc, c0, e->stream, e->ev_h2d[b]);
        if (rc != BFIR_OK) return rc;
        HIP_TRY(hipEventRecord(e->ev_comp[b], e->stream));
        HIP_TRY(hipStreamWaitEvent(e->s_out, e->ev_comp[b], 0));
        if (out_direct) {
            for (int g = 0; g < e->n_eng; g++)
                HIP_TRY(hipMemcpyAsync((char *)outbuf + g * eng_out + (size_t)c0 * e->L * fout, (char *)e->dev_out[b] + g * per_out,
                                       per_out, hipMemcpyDeviceToHost, e->s_out));
        } else
            HIP_TRY(hipMemcpyAsync(e->pin_out[b], e->dev_out[b], per_out * e->n_eng, hipMemcpyDeviceToHost, e->s_out));
        HIP_TRY(hipEventRecord(e->ev_d2h[b], e->s_out));
        // the next H2D into dev_in[b] must not overtake this chunk's kernels
        HIP_TRY(hipStreamWaitEvent(e->s_in, e->ev_comp[b], 0));
    }
    for (int k = std::max(0, nchunks - 2); k < nchunks; k++) { rc = copy_out(k); if (rc != BFIR_OK) return rc; }
    return bfir_engine_sync(e);
}

// A two- or multi-level engine forgets all signal state -- every delay line, every time history, the partial input blocks
// and every level's queued output -- and zeroes the counters: it then behaves as newly created with the same coefficients.
// (The plain engine keeps input_timecbuf, a quirk of the reference that has no meaning here.)
static void nup_reset(bfir_engine *e)
{
    (void)hipDeviceSynchronize();
    if (e->fade_len > 0) fade_swap_sets(e);   // a fade ends at once, with the new set active at every level
    for (int k = 0; k <= e->n_tail; k++) {
        bfir_engine *l = level(e, k);
        (void)hipMemset(l->X, 0, (size_t)l->GC * l->ring * cbuf_bytes(l));
        for (int st = 0; st < 2; st++)
            for (int i = 0; i < 2; i++) (void)hipMemset(l->tails[st][i], 0, (size_t)l->L * l->C * l->in_bytes);
        l->blockcounter = 0; l->curbuf = 0;
        l->z_from = l->z_next = 0;
    }
    e->pbuf_upto = 0;
    (void)hipMemset(e->d_of, 0, sizeof(DevOverflow) * e->GCo * BFIR_OF_SHARDS);
    (void)hipDeviceSynchronize();
}

extern "C" void bfir_engine_reset(bfir_engine *e)
{
    if (!e) return;
    (void)hipSetDevice(e->device);
    if (e->dly[0].on || e->dly[1].on) { (void)hipDeviceSynchronize(); delay_reset(e); }
    if (e->nup) { nup_reset(e); return; }
    // brutefir.cpp:346-367: counters only.  procblocks = 0 hides every
    // delay-line slot written before the reset (brutefir.cpp:292), which the
    // zeroed ring reproduces; the time-domain history is NOT cleared, so both
    // input_timecbuf halves are kept (copied out of the work buffers).
    (void)materialise_history(e);
    if (e->fade_len > 0) fade_swap_sets(e);   // a fade ends at once, with the new set active (the device is idle here)
    (void)hipMemset(e->d_of, 0, sizeof(DevOverflow) * e->GCo * BFIR_OF_SHARDS);
    // block t < B-1 of the new run still reads slots (t - i) mod ring, i > t: the B-1 slots at the top of
    // every channel's ring.  Only those need to read as zero; the rest is rewritten before it is read.
    if (e->B > 1) {
        const size_t cb = cbuf_bytes(e);
        (void)hipMemset2D((char *)e->X + (size_t)(e->ring - (e->B - 1)) * cb, (size_t)e->ring * cb, 0,
                          (size_t)(e->B - 1) * cb, (size_t)e->GC);
    }
    (void)hipDeviceSynchronize();
    e->blockcounter = 0;
    e->curbuf = 0;
}

extern "C" int bfir_engine_get_overflow(bfir_engine *e, int channel, bfir_overflow *of)
{
    if (!e || !of || channel < 0 || channel >= e->GCo) return BFIR_ERR_ARG;   // an output of a matrix engine
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    // the copies of the counters (kernels.h, BFIR_OF_SHARDS): counts add up, peaks are maxima (the bit patterns of
    // non-negative floats order like integers); the dither kernel keeps its running state in copy 0
    std::vector<DevOverflow> all((size_t)e->GCo * BFIR_OF_SHARDS);
    HIP_TRY(hipMemcpy(all.data(), e->d_of, all.size() * sizeof(DevOverflow), hipMemcpyDeviceToHost));
    DevOverflow d = all[channel];
    for (int sh = 1; sh < BFIR_OF_SHARDS; sh++) {
        const DevOverflow &o = all[(size_t)sh * e->GCo + channel];
        d.n_overflows += o.n_overflows;
        d.intlargest = std::max(d.intlargest, o.intlargest);
        d.largest_bits = std::max(d.largest_bits, o.largest_bits);
    }
    of->n_overflows = d.n_overflows;
    of->intlargest = d.intlargest;
    if (e->s == 4) {
        unsigned int u = (unsigned int)d.largest_bits;
        float f;
        memcpy(&f, &u, sizeof(f));
        of->largest = (double)f;
    } else {
        double f;
        memcpy(&f, &d.largest_bits, sizeof(f));
        of->largest = f;
    }
    of->max = e->of_max;
    return BFIR_OK;
}
