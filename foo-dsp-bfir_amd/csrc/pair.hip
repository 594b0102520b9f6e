// pair.hip -- two channels per transform, straight from / to interleaved float frames.
//
// The engine's fast path for FLOAT_LE in and out, an even channel count and fp32 arithmetic
// (the plug-in's and the offline drivers' configuration: foo_dsp_bfir.cpp:283-284,
// preprocessor.cpp:292-293).  Channels 2c and 2c+1 of a frame are adjacent floats, so
//
//     z[n] = x_2c[n] + i x_2c+1[n],    n = 0 .. N-1   (N = 2L: previous block | this block)
//
// is ONE 8-byte load per point from the raw frames, and one complex FFT of N points yields both
// half-complex spectra (the classic two-for-one split, no twiddle):
//
//     X_a[k] = (Z[k] + conj Z[N-k]) / 2,      X_b[k] = (Z[k] - conj Z[N-k]) / (2i).
//
// The inverse runs the same identity backwards (Z = Y_a + i Y_b, Hermitian-extended), and
// Re z / Im z of the complex inverse are the two channels' samples, stored as 8-byte pairs
// into the raw output frames together with the overflow statistics and the NaN guard of
// real2raw (brutefir/real2raw.cpp:321-336, brutefir.cpp:316-321).
// This replaces raw2real + R2HC + mixnscale (fftw_convolver.cpp:156-209, a5-a7) and
// mixnscale + HC2R + real2raw (:360-466, a11-a13) for such engines and removes the planar time
// buffers with their 2 x 2 trips through HBM; the MAC between them is k_mac_stream.
// Spectra are (re, im) pairs (MacArgs.interleaved); bin 0 carries DC | Nyquist.
#include "kernels.h"

#include <algorithm>
#include <cstdlib>

#include "fft_lds.h"
#include "pair_io.h"

namespace bfir {

namespace {

// ---- persistent forward kernel -------------------------------------------------------------------
// A forward kernel that transforms one block per workgroup waits for memory, not arithmetic
// (profiles/r02_alias_and_bottleneck_experiments.txt: 0.235 ms of VALU + LDS under 0.33 ms of exposed
// load / store / twiddle time per 4096 blocks).  Here ONE workgroup transforms a run of consecutive blocks
// of one channel pair:
//   * every block is loaded once: the half-window "current block" of transform t is the "previous
//     block" of transform t+1 and stays in registers (same thread: n -> n - L keeps the lane);
//   * the next block is fetched right after the first butterflies of the current transform and is
//     only waited for when that transform has stored its spectra, which in turn drain while the
//     next transform computes (a workgroup that ends with its stores keeps its CU slot until they land);
//   * twiddles never touch memory in steady state: the bases of the last pass live in registers, those
//     of the passes before it in 9 KB of LDS, for the workgroup's life (LdsFft::butterflies_tb), so
//     nothing queues behind the prefetch in vmcnt order.
// Same arithmetic as one LdsFft::run per block except that a derived twiddle carries one more rounding.
template <int LOG2N>
__global__ __launch_bounds__(FftCfg<LOG2N>::NT, 4) void k_fwd_pair_ps(FwdPairArgs a, const float2 *__restrict__ twb, int run_len)
{
    using F = LdsFft<float, LOG2N, -1>;
    constexpr int N = F::M, NT = F::NT, P = F::P, L = N / 2, H = P / 2;   // H points per thread and block
    static_assert(F::radix(0) == 16 && P == 16, "in_index(tid, e) = tid + e * (N / 16)");
    static_assert(F::phys(32) == 33 && F::phys(N - 1) == N - 1 + N / 32 - 1, "the split step's addresses assume i + (i >> 5)");
    __shared__ __attribute__((aligned(16))) float2 lds[F::LDS_ELEMS + 1];   // + 1: see the split step
    __shared__ __attribute__((aligned(16))) float2 ldsb[F::LDSB_ELEMS];

    const int tid = threadIdx.x;
    const int w = xcd_work_item(blockIdx.x, gridDim.x);
    const int half_c = a.C / 2, pairs = a.n_eng * half_c;
    const int rr = w / pairs, pp = w - rr * pairs;                       // run, pair: the pairs of a run share an XCD
    // The two-for-one split halves every sum (Xa = (Z[k] + conj Z[N-k]) / 2 ...): the half goes into the input
    // scale instead, which is exact (a power of two commutes with every rounding of the transform), and
    // the two purely real bins, which the split takes unhalved, are doubled back (exact again).
    const float sc = 0.5f * a.scale;
    const int g = pp / half_c, cp = pp - g * half_c;
    const int C = a.C;
    const int t0 = rr * run_len, t1 = min(a.n_t, t0 + run_len);
    if (t0 >= t1) return;

    float2 B[F::NBREG];
    F::load_bases(B, ldsb, twb, tid);                                    // the first exchange's barrier publishes ldsb

    // frame n = tid + e NT of a block of frames sits at byte  blk + 4 (e NT C + tid C)  (+ 8 cp for the pair)
    const float *__restrict__ raw = a.raw + (long)g * a.eng_stride + a.frame_off * C + 2 * cp;
    const long hist = (long)g * a.hist_eng_stride + 2 * cp;
    const unsigned blk_bytes = (unsigned)L * C * 4u;
    const unsigned fo = (unsigned)tid * (unsigned)C * 4u;                // lane offset into a block of frames
    const unsigned estep = (unsigned)NT * C * 4u;                        // bytes between a thread's consecutive points
    static_assert(H == 8, "the prefetch statement moves eight points per thread");
    float2 cur[H];
    u32x2 nxt[H];                                                        // raw frames of the next block, as loaded
    {
        const __amdgpu_buffer_rsrc_t ro = make_rsrc((t0 == 0) ? a.prev + hist : raw + (long)(t0 - 1) * L * C, blk_bytes);
#pragma unroll
        for (int e = 0; e < H; e++) {
            const float2 v = buf_load2(ro, fo, e * estep);
            cur[e].x = v.x * sc; cur[e].y = v.y * sc;
        }
        if (a.n_t == 1) {                                                // one-block chunk: the other history block moves on unchanged
            const __amdgpu_buffer_rsrc_t rc = make_rsrc(a.carry + hist, blk_bytes), rp = make_rsrc(a.save_prev + hist, blk_bytes);
#pragma unroll
            for (int e = 0; e < H; e++) buf_store2(rp, fo, e * estep, buf_load2(rc, fo, e * estep));
        }
        const __amdgpu_buffer_rsrc_t rb = make_rsrc(raw + (long)t0 * L * C, blk_bytes);
#pragma unroll
        for (int e = 0; e < H; e++) nxt[e] = __builtin_amdgcn_raw_buffer_load_b64(rb, fo, e * estep, 0);
        // these (compiler-counted) loads are consumed before the loop, so inside it the compiler has no
        // pending load of its own to wait for
#pragma unroll
        for (int e = 0; e < H; e++) asm volatile("" : "+v"(nxt[e]));
    }
    float *__restrict__ da0 = a.dst + (long)(g * C + 2 * cp) * a.dst_ch_stride;
    for (int t = t0; t < t1; t++) {
        float re[P], im[P];
        // block t has landed when all but the 2 (P/4) spectrum stores issued after its prefetch are done
        asm_wait_vmcnt<2 * (P / 4)>(nxt);
        if (t >= a.n_t - 2) {                                            // uniform: the chunk's last two blocks
            // the engine's history: raw frames of the last two blocks of the chunk (stores only: nothing in
            // this branch for the compiler to wait for, and it lies outside the window the counted wait spans)
            const __amdgpu_buffer_rsrc_t rk = make_rsrc((t == a.n_t - 1 ? a.save_last : a.save_prev) + hist, blk_bytes);
#pragma unroll
            for (int e = 0; e < H; e++) __builtin_amdgcn_raw_buffer_store_b64(nxt[e], rk, fo, e * estep, 0);
        }
#pragma unroll
        for (int e = 0; e < H; e++) {
            float2 v; v.x = __uint_as_float(nxt[e].x); v.y = __uint_as_float(nxt[e].y);   // raw frames of block t
            re[e] = cur[e].x; im[e] = cur[e].y;                          // window = [block t-1 | block t]
            cur[e].x = v.x * sc; cur[e].y = v.y * sc;
            re[H + e] = cur[e].x; im[H + e] = cur[e].y;
        }
        {
            float2 w0[1];
            F::template butterflies<0>(re, im, w0);
        }
        static_for<1, F::NP>([&](auto S_) {
            constexpr int S = decltype(S_)::value;
            // LDS addresses are formed afresh per phase from an opaque copy of the lane index: otherwise
            // the compiler hoists a dozen of them out of the transform loop and spills them around it
            int tl = tid; asm volatile("" : "+v"(tl));
            F::template exchange<S - 1>(re, im, lds, tl);
            F::template butterflies_tb<S>(re, im, B, ldsb, tl);
            if constexpr (S == 1) {
                // fetch block t+1 under the remaining passes (after the widest butterfly); past the end of
                // the run the descriptor has zero bytes and the loads return zeros (no branch, see above)
                asm_prefetch8x2(nxt, fo, make_rsrc_words(raw + (long)(t + 1) * L * C, t + 1 < t1 ? blk_bytes : 0u), estep);
            }
        });

        // Z in natural order to LDS, then two-for-one split.  Every LDS address below is one per-thread base
        // plus a compile-time offset (i + (i >> 5) is additive for offsets that are multiples of 32).
        int tz = tid; asm volatile("" : "+v"(tz));
        __syncthreads();
        {
            float2 *zw = lds + F::phys(tz);
            static_for<0, P>([&](auto E_) {
                constexpr int e = decltype(E_)::value;
                static_assert(F::out_index(0, e) % 32 == 0, "additive padding");
                float2 v; v.x = re[e]; v.y = im[e];
                zw[F::phys(F::out_index(0, e))] = v;
            });
        }
        __syncthreads();
        const long slot = (long)((a.base_slot + t) % a.ring) * N;
        const __amdgpu_buffer_rsrc_t rxa = make_rsrc(da0 + slot, (unsigned)N * 4u), rxb = make_rsrc(da0 + a.dst_ch_stride + slot, (unsigned)N * 4u);
        // A thread splits two ADJACENT bins (k = 2 m, 2 m + 1; m = tid + j NT) so that each spectrum store is
        // 16 bytes per lane: vector stores are issue-bound per instruction on this chip (8-byte stores run at
        // about 7 B/clk/CU, MI355X_MICROARCH.md cycle table), and this kernel stores twice what it loads.
        // Z[k], Z[k+1] sit at zk[phys(2 NT j)], + 1.  Z[N-k-1] sits at zn1[-phys(2 NT j)]: N-1-2 tid has
        // its low five bits free of borrows; Z[N-k] one element further, two where N-k is a multiple of 32 (a pad
        // element lies between).  Lane 0 at j = 0 reads Z[N] = lds[LDS_ELEMS], the spare element: its
        // bin 0 is replaced below.
        const float2 *zk = lds + F::phys(2 * tz);
        constexpr int OMAX = F::phys(2 * NT * (P / 4 - 1));              // bases lowered so that every offset is >= 0
        const float2 *zn1 = lds + (F::phys(N - 1 - 2 * tz) - OMAX);
        const float2 *zn0 = zn1 + ((tz & 15) == 0 ? 2 : 1);
#pragma unroll
        for (int j = 0; j < P / 4; j++) {
            // one pair at a time: left alone the scheduler fetches all sixteen Z values first (32 registers
            // on top of the prefetch and the carried block)
            if (j > 0) __builtin_amdgcn_sched_barrier(0);
            const int o = F::phys(2 * NT * j);
            const float2 zk0 = zk[o], zk1 = zk[o + 1];
            const float2 zn0v = zn0[OMAX - o], zn1v = zn1[OMAX - o];
            float4 xa, xb;
            xa.x = zk0.x + zn0v.x; xa.y = zk0.y - zn0v.y;
            xb.x = zk0.y + zn0v.y; xb.y = zn0v.x - zk0.x;
            xa.z = zk1.x + zn1v.x; xa.w = zk1.y - zn1v.y;
            xb.z = zk1.y + zn1v.y; xb.w = zn1v.x - zk1.x;
            if (j == 0) {                                                // m = tid: bin 0 is DC | Nyquist, both real
                const float2 zh = lds[F::phys(L)];
                const bool k0 = tz == 0;
                xa.x = k0 ? 2.f * zk0.x : xa.x; xa.y = k0 ? 2.f * zh.x : xa.y;
                xb.x = k0 ? 2.f * zk0.y : xb.x; xb.y = k0 ? 2.f * zh.y : xb.y;
            }
            buf_store4<2>(rxa, (unsigned)tz * 16u, (unsigned)(j * NT) * 16u, xa);
            buf_store4<2>(rxb, (unsigned)tz * 16u, (unsigned)(j * NT) * 16u, xb);
        }
        // the next transform's first exchange starts with a barrier, which also protects these LDS reads
    }
    // The last prefetch (zero-byte descriptor: it returns zeros) is still in flight and will write nxt[]:
    // those registers must not be handed to anything else before it has landed.
    asm_wait_vmcnt<0>(nxt);
}

// ---- persistent forward kernel, pairs in TIME ------------------------------------------------------------
// The same two-for-one transform for engines whose channels cannot be paired (an odd channel count, one channel --
// the 8-GPU point of a channel-sharded stream): blocks t and t + 1 of ONE channel are the real and the imaginary part,
//
//     z[n] = w_t[n] + i w_{t+1}[n],     w_t = [block t-1 | block t]   (the window brutefir.cpp:255-263 transforms),
//
// so that X_a is block t's delay-line spectrum and X_b block t + 1's -- channels never mix (brutefir.cpp:252-334), and
// the split, the scaling and every rounding are those of the channel-pair kernel: the spectra are the SAME numbers
// whichever way the blocks are paired up.  One workgroup walks a run of an even number of blocks of one channel; a
// thread keeps its 8 samples of block t + 1 (the next window's "previous block") in registers, fetches blocks
// t + 2 and t + 3 (4-byte samples at the frame stride) under the passes, same hand-counted wait as above.  When the
// chunk ends on an odd block the imaginary part is zero (zero-byte descriptor) and its spectrum is not stored (ditto).
template <int LOG2N>
__global__ __launch_bounds__(FftCfg<LOG2N>::NT, 4) void k_fwd_tp_ps(FwdPairArgs a, const float2 *__restrict__ twb, int run_len)
{
    using F = LdsFft<float, LOG2N, -1>;
    constexpr int N = F::M, NT = F::NT, P = F::P, L = N / 2, H = P / 2;
    static_assert(F::radix(0) == 16 && P == 16, "in_index(tid, e) = tid + e * (N / 16)");
    static_assert(F::phys(32) == 33 && F::phys(N - 1) == N - 1 + N / 32 - 1, "the split step's addresses assume i + (i >> 5)");
    __shared__ __attribute__((aligned(16))) float2 lds[F::LDS_ELEMS + 1];
    __shared__ __attribute__((aligned(16))) float2 ldsb[F::LDSB_ELEMS];

    const int tid = threadIdx.x;
    const int w = xcd_work_item(blockIdx.x, gridDim.x);
    const int C = a.C, units = a.n_eng * C;
    const int rr = w / units, pp = w - rr * units;                       // run, channel: the channels of a run share an XCD
    const int g = pp / C, c = pp - g * C;
    const float sc = 0.5f * a.scale;                                     // the split's 1/2, see k_fwd_pair_ps
    const int t0 = rr * run_len, t1 = min(a.n_t, t0 + run_len);          // run_len is even
    if (t0 >= t1) return;

    float2 B[F::NBREG];
    F::load_bases(B, ldsb, twb, tid);

    const float *__restrict__ raw = a.raw + (long)g * a.eng_stride + a.frame_off * C + c;
    const long hist = (long)g * a.hist_eng_stride + c;
    const unsigned blk_bytes = (unsigned)L * C * 4u;
    const unsigned fo = (unsigned)tid * (unsigned)C * 4u;                // lane offset into a block of frames
    const unsigned estep = (unsigned)NT * C * 4u;                        // bytes between a thread's consecutive samples
    static_assert(H == 8, "the prefetch statement moves eight samples per thread and block");
    float prv[H];                                                        // block t - 1, scaled
    unsigned nb[H], nc[H];                                               // raw samples of blocks t and t + 1, as loaded
    {
        const __amdgpu_buffer_rsrc_t ro = make_rsrc((t0 == 0) ? a.prev + hist : raw + (long)(t0 - 1) * L * C, blk_bytes);
#pragma unroll
        for (int e = 0; e < H; e++) prv[e] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ro, fo, e * estep, 0)) * sc;
        if (a.n_t == 1) {                                                // one-block chunk: the other history block moves on unchanged
            const __amdgpu_buffer_rsrc_t rc = make_rsrc(a.carry + hist, blk_bytes), rp = make_rsrc(a.save_prev + hist, blk_bytes);
#pragma unroll
            for (int e = 0; e < H; e++)
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_amdgcn_raw_buffer_load_b32(rc, fo, e * estep, 0), rp, fo, e * estep, 0);
        }
        const __amdgpu_buffer_rsrc_t rb = make_rsrc(raw + (long)t0 * L * C, blk_bytes);
        const __amdgpu_buffer_rsrc_t rn = make_rsrc(raw + (long)(t0 + 1) * L * C, t0 + 1 < t1 ? blk_bytes : 0u);
#pragma unroll
        for (int e = 0; e < H; e++) {
            nb[e] = __builtin_amdgcn_raw_buffer_load_b32(rb, fo, e * estep, 0);
            nc[e] = __builtin_amdgcn_raw_buffer_load_b32(rn, fo, e * estep, 0);
        }
        // consumed before the loop, so inside it the compiler has no pending load of its own to wait for
#pragma unroll
        for (int e = 0; e < H; e++) asm volatile("" : "+v"(nb[e]), "+v"(nc[e]));
    }
    float *__restrict__ da0 = a.dst + (long)(g * C + c) * a.dst_ch_stride;
    for (int t = t0; t < t1; t += 2) {
        float re[P], im[P];
        // blocks t, t + 1 have landed when all but the 2 (P/4) spectrum stores issued after their prefetch are done
        asm_wait_vmcnt<2 * (P / 4)>(nb, nc);
        if (t + 1 >= a.n_t - 2) {                                        // uniform: one of the chunk's last two blocks is here
            // the engine's history: the raw samples of the last two blocks of the chunk (stores only, outside the
            // window the counted wait spans)
            if (t >= a.n_t - 2) {
                const __amdgpu_buffer_rsrc_t rk = make_rsrc((t == a.n_t - 1 ? a.save_last : a.save_prev) + hist, blk_bytes);
#pragma unroll
                for (int e = 0; e < H; e++) __builtin_amdgcn_raw_buffer_store_b32(nb[e], rk, fo, e * estep, 0);
            }
            if (t + 1 < a.n_t) {
                const __amdgpu_buffer_rsrc_t rk = make_rsrc((t + 1 == a.n_t - 1 ? a.save_last : a.save_prev) + hist, blk_bytes);
#pragma unroll
                for (int e = 0; e < H; e++) __builtin_amdgcn_raw_buffer_store_b32(nc[e], rk, fo, e * estep, 0);
            }
        }
#pragma unroll
        for (int e = 0; e < H; e++) {
            const float vb = __uint_as_float(nb[e]) * sc, vc = __uint_as_float(nc[e]) * sc;
            re[e] = prv[e]; im[e] = vb;                                  // windows [t-1 | t] and [t | t+1]
            re[H + e] = vb; im[H + e] = vc;
            prv[e] = vc;
        }
        {
            float2 w0[1];
            F::template butterflies<0>(re, im, w0);
        }
        static_for<1, F::NP>([&](auto S_) {
            constexpr int S = decltype(S_)::value;
            int tl = tid; asm volatile("" : "+v"(tl));
            F::template exchange<S - 1>(re, im, lds, tl);
            F::template butterflies_tb<S>(re, im, B, ldsb, tl);
            if constexpr (S == 1) {
                // blocks t + 2 and t + 3 under the remaining passes; past the end of the run the descriptors have
                // zero bytes and the loads return zeros (no branch)
                asm_prefetch2x8x1(nb, nc, fo, make_rsrc_words(raw + (long)(t + 2) * L * C, t + 2 < t1 ? blk_bytes : 0u),
                                  make_rsrc_words(raw + (long)(t + 3) * L * C, t + 3 < t1 ? blk_bytes : 0u), estep);
            }
        });

        // Z in natural order to LDS, then two-for-one split (k_fwd_pair_ps)
        int tz = tid; asm volatile("" : "+v"(tz));
        __syncthreads();
        {
            float2 *zw = lds + F::phys(tz);
            static_for<0, P>([&](auto E_) {
                constexpr int e = decltype(E_)::value;
                static_assert(F::out_index(0, e) % 32 == 0, "additive padding");
                float2 v; v.x = re[e]; v.y = im[e];
                zw[F::phys(F::out_index(0, e))] = v;
            });
        }
        __syncthreads();
        const long slot_a = (long)((a.base_slot + t) % a.ring) * N, slot_b = (long)((a.base_slot + t + 1) % a.ring) * N;
        const __amdgpu_buffer_rsrc_t rxa = make_rsrc(da0 + slot_a, (unsigned)N * 4u);
        const __amdgpu_buffer_rsrc_t rxb = make_rsrc(da0 + slot_b, t + 1 < a.n_t ? (unsigned)N * 4u : 0u);   // odd end: dropped
        const float2 *zk = lds + F::phys(2 * tz);
        constexpr int OMAX = F::phys(2 * NT * (P / 4 - 1));
        const float2 *zn1 = lds + (F::phys(N - 1 - 2 * tz) - OMAX);
        const float2 *zn0 = zn1 + ((tz & 15) == 0 ? 2 : 1);
#pragma unroll
        for (int j = 0; j < P / 4; j++) {
            if (j > 0) __builtin_amdgcn_sched_barrier(0);
            const int o = F::phys(2 * NT * j);
            const float2 zk0 = zk[o], zk1 = zk[o + 1];
            const float2 zn0v = zn0[OMAX - o], zn1v = zn1[OMAX - o];
            float4 xa, xb;
            xa.x = zk0.x + zn0v.x; xa.y = zk0.y - zn0v.y;
            xb.x = zk0.y + zn0v.y; xb.y = zn0v.x - zk0.x;
            xa.z = zk1.x + zn1v.x; xa.w = zk1.y - zn1v.y;
            xb.z = zk1.y + zn1v.y; xb.w = zn1v.x - zk1.x;
            if (j == 0) {                                                // bin 0 is DC | Nyquist, both real
                const float2 zh = lds[F::phys(L)];
                const bool k0 = tz == 0;
                xa.x = k0 ? 2.f * zk0.x : xa.x; xa.y = k0 ? 2.f * zh.x : xa.y;
                xb.x = k0 ? 2.f * zk0.y : xb.x; xb.y = k0 ? 2.f * zh.y : xb.y;
            }
            buf_store4<2>(rxa, (unsigned)tz * 16u, (unsigned)(j * NT) * 16u, xa);
            buf_store4<2>(rxb, (unsigned)tz * 16u, (unsigned)(j * NT) * 16u, xb);
        }
    }
    // the last prefetch (zero-byte descriptors) is still in flight and will write nb / nc: see k_fwd_pair_ps
    asm_wait_vmcnt<0>(nb, nc);
}

// ---- persistent inverse kernel ---------------------------------------------------------------------
// The same treatment for the way back: one workgroup turns a run of consecutive product spectra of one
// channel pair into output frames.  The next block's two spectra (64 KiB per workgroup) are fetched into
// registers (8 x 16 bytes per thread) under the passes of the current transform and only staged into LDS
// when the passes are done with it; the 8-byte strided output stores drain under the next transform;
// twiddles from bases (LdsFft::butterflies_tb); overflow statistics reduced once per run, not per block.
template <int LOG2N>
__global__ __launch_bounds__(FftCfg<LOG2N>::NT, inv_ps_min_waves<LOG2N>()) void k_inv_pair_ps(InvPairArgs a, const float2 *__restrict__ twb, int run_len)
{
    using F = LdsFft<float, LOG2N, +1>;
    constexpr int N = F::M, NT = F::NT, P = F::P, L = N / 2, Q = P / 4;   // Q 16-byte pieces per thread and spectrum
    __shared__ __attribute__((aligned(16))) float2 lds[F::LDS_ELEMS];
    __shared__ __attribute__((aligned(16))) float2 ldsb[F::LDSB_ELEMS];
    __shared__ unsigned int red_max[NT / 64 > 0 ? NT / 64 : 1][2], red_cnt[NT / 64 > 0 ? NT / 64 : 1][2];

    const int tid = threadIdx.x;
    const int w = xcd_work_item(blockIdx.x, gridDim.x);
    const int half_c = a.C / 2, pairs = a.n_eng * half_c;
    const int rr = w / pairs, pp = w - rr * pairs;
    const int g = pp / half_c, cp = pp - g * half_c;
    const int C = a.C;
    const int FS = a.frame_stride ? a.frame_stride : C;                  // floats between output frames
    const int gc = g * C + 2 * cp;
    const int t0 = rr * run_len, t1 = min(a.n_t, t0 + run_len);
    if (t0 >= t1) return;

    float2 B[F::NBREG];
    F::load_bases(B, ldsb, twb, tid);

    const float *__restrict__ ya0 = a.y + (long)gc * a.y_ch_stride;
    float *__restrict__ out0 = a.raw + (long)g * a.eng_stride + a.frame_off * FS + 2 * cp;
    const unsigned blk_bytes = (unsigned)L * FS * 4u;
    const unsigned cio = (unsigned)FS;                                   // floats between a pair's consecutive frames
    static_assert(Q == 4, "the prefetch statement moves four 16-byte pieces per thread and spectrum");
    u32x4 qa[Q], qb[Q];
    {
        const __amdgpu_buffer_rsrc_t ra = make_rsrc(ya0 + (long)t0 * N, (unsigned)N * 4u);
        const __amdgpu_buffer_rsrc_t rb = make_rsrc(ya0 + a.y_ch_stride + (long)t0 * N, (unsigned)N * 4u);
#pragma unroll
        for (int j = 0; j < Q; j++) {
            qa[j] = __builtin_amdgcn_raw_buffer_load_b128(ra, (unsigned)tid * 16u, (unsigned)(j * NT) * 16u, 2);
            qb[j] = __builtin_amdgcn_raw_buffer_load_b128(rb, (unsigned)tid * 16u, (unsigned)(j * NT) * 16u, 2);
        }
        // consumed before the loop: inside it the compiler has no pending load of its own (see k_fwd_pair_ps)
#pragma unroll
        for (int j = 0; j < Q; j++) asm volatile("" : "+v"(qa[j]), "+v"(qb[j]));
    }
    // brutefir/real2raw.cpp:321-336 counts v < 0 ? v < -max : v > max (strict, NaN never counts) and tracks the
    // largest magnitude: with symmetric limits that is |v| > max, and a float maximum that skips NaNs
    // (fmaxf) -- three instructions per sample instead of twelve.
    const float rmax = a.max;
    float pk0 = 0.f, pk1 = 0.f;
    unsigned int c0 = 0u, c1 = 0u;
    int bad = 0x7fffffff;
    for (int t = t0; t < t1; t++) {
        // both spectra into LDS: Ya at [0, L), Yb at [L, 2L)  (float2 units)
        int ts = tid; asm volatile("" : "+v"(ts));
        // block t's spectra have landed when all but the P/2 output stores issued after their prefetch are done
        asm_wait_vmcnt<P / 2>(qa, qb);
        __syncthreads();                                                 // the previous transform's readers are done
        {
            u32x4 *l4 = (u32x4 *)lds;
#pragma unroll
            for (int j = 0; j < Q; j++) { l4[ts + j * NT] = qa[j]; l4[L / 2 + ts + j * NT] = qb[j]; }
        }
        __syncthreads();
        // Z[k] = Ya[k] + i Yb[k], Hermitian-extended to the full circle
        float re[P], im[P];
        static_for<0, P>([&](auto E_) {
            constexpr int e = decltype(E_)::value;
            // k = base + tid with a compile-time base: which side of L a point lies on is known per e,
            // and only e with base 0 / base L can hit the two real bins (tid 0) -- selects, no branches
            constexpr int base = F::in_index(0, e);
            static_assert(base + NT <= L || base >= L, "a thread's points do not straddle L");
            const int k = base + ts;
            const int kk = (base < L) ? k : N - k;                       // kk == L only for base == L, tid == 0
            const bool edge = (base == 0 || base == L) && ts == 0;
            const float2 pa = lds[edge ? 0 : kk], pb = lds[L + (edge ? 0 : kk)];
            float zr, zi;
            if (base < L) { zr = pa.x - pb.y; zi = pa.y + pb.x; }
            else          { zr = pa.x + pb.y; zi = pb.x - pa.y; }         // conj Ya + i conj Yb
            if (base == 0) { zr = edge ? pa.x : zr; zi = edge ? pb.x : zi; }   // DC of both channels
            if (base == L) { zr = edge ? pa.y : zr; zi = edge ? pb.y : zi; }   // Nyquist of both channels
            re[e] = zr * a.scale; im[e] = zi * a.scale;
        });
        pin_registers(re, im);   // every read of the staged spectra happens before the first exchange's barrier
        {
            float2 w0[1];
            F::template butterflies<0>(re, im, w0);
        }
        static_for<1, F::NP>([&](auto S_) {
            constexpr int S = decltype(S_)::value;
            int tl = tid; asm volatile("" : "+v"(tl));
            F::template exchange<S - 1>(re, im, lds, tl);
            F::template butterflies_tb<S>(re, im, B, ldsb, tl);
            if constexpr (S == 1) {
                // the next block's spectra, under the remaining passes; past the end of the run the descriptors
                // have zero bytes and the loads return zeros (no branch in the loop, see k_fwd_pair_ps)
                const unsigned nbytes = t + 1 < t1 ? (unsigned)N * 4u : 0u;
                asm_prefetch2x4x4(qa, qb, (unsigned)tl * 16u, make_rsrc_words(ya0 + (long)(t + 1) * N, nbytes),
                                  make_rsrc_words(ya0 + a.y_ch_stride + (long)(t + 1) * N, nbytes), (unsigned)NT * 16u);
            }
        });

        // first L samples are the valid half (the taps sit in the upper half of their blocks)
        const __amdgpu_buffer_rsrc_t ro = make_rsrc(out0 + (long)t * L * FS, blk_bytes);
        int to = tid; asm volatile("" : "+v"(to));
#pragma unroll
        for (int e = 0; e < P; e++) {
            const int n = F::out_index(to, e);
            if (F::out_index(0, e) < L) {                                // compile time: out_index(tid, e) = tid + const, tid < NT <= L
                float2 v; v.x = re[e]; v.y = im[e];
                buf_store2(ro, (unsigned)to * cio * 4u, (unsigned)F::out_index(0, e) * cio * 4u, v);
                c0 += (fabsf(v.x) > rmax) ? 1u : 0u;
                c1 += (fabsf(v.y) > rmax) ? 1u : 0u;
                pk0 = fmaxf(pk0, fabsf(v.x)); pk1 = fmaxf(pk1, fabsf(v.y));
                // brutefir/brutefir.cpp:316-321: only sample 0 of each block is checked; the first bad block
                // of the run is reported once, after the loop (no atomic inside it)
                if (F::out_index(0, e) == 0) {
                    const bool nf = n == 0 && !(isfinite(v.x) && isfinite(v.y));
                    bad = (nf && t < bad) ? t : bad;
                }
            }
        }
    }
    // The last prefetch (zero-byte descriptors: it returns zeros) is still in flight and will write qa / qb.
    // Without this wait the compiler reuses those registers below -- for the ADDRESSES of the atomics, which the
    // late zeros then turn into a null pointer (seen as a sporadic "memory access fault on address (nil)").
    asm_wait_vmcnt<0>(qa, qb);
    if (bad != 0x7fffffff) flag_bad(a, bad);
    unsigned int mx0 = __float_as_uint(pk0), mx1 = __float_as_uint(pk1);   // non-negative floats order like their bits
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned int m0 = __shfl_xor(mx0, o), m1 = __shfl_xor(mx1, o);
        mx0 = m0 > mx0 ? m0 : mx0; mx1 = m1 > mx1 ? m1 : mx1;
        c0 += __shfl_xor(c0, o); c1 += __shfl_xor(c1, o);
    }
    if ((tid & 63) == 0) { red_max[tid >> 6][0] = mx0; red_max[tid >> 6][1] = mx1; red_cnt[tid >> 6][0] = c0; red_cnt[tid >> 6][1] = c1; }
    __syncthreads();
    if (tid < 2) {
        unsigned int m = 0u, n = 0u;
        for (int wv = 0; wv < (NT + 63) / 64; wv++) { m = red_max[wv][tid] > m ? red_max[wv][tid] : m; n += red_cnt[wv][tid]; }
        DevOverflow *of = of_shard(a.overflow, a.of_shard_stride) + (gc + tid);
        if (n) atomicAdd(&of->n_overflows, n);
        // filtered: the peak only ever grows, a stale read costs an extra atomic, never a wrong result
        if ((unsigned long long)m > *(volatile unsigned long long *)&of->largest_bits)
            atomicMax(&of->largest_bits, (unsigned long long)m);
    }
}

// ---- persistent inverse kernel, pairs in TIME --------------------------------------------------------------
// Z = Y_t + i Y_{t+1} of ONE channel: Re z is block t's output, Im z block t + 1's (k_fwd_tp_ps).  4-byte samples at
// the frame stride, 16 stores per transform (hence the wait for all but 16), both blocks' overflow statistics go to
// the one channel; at an odd chunk end Y_{t+1} reads as zero and its samples are not stored (zero-byte descriptors).
__device__ __forceinline__ void buf_store1(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff, float f)
{
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(f), r, voff, soff, 0);
}

template <int LOG2N>
__global__ __launch_bounds__(FftCfg<LOG2N>::NT, inv_ps_min_waves<LOG2N>()) void k_inv_tp_ps(InvPairArgs a, const float2 *__restrict__ twb, int run_len)
{
    using F = LdsFft<float, LOG2N, +1>;
    constexpr int N = F::M, NT = F::NT, P = F::P, L = N / 2, Q = P / 4;
    __shared__ __attribute__((aligned(16))) float2 lds[F::LDS_ELEMS];
    __shared__ __attribute__((aligned(16))) float2 ldsb[F::LDSB_ELEMS];
    __shared__ unsigned int red_max[NT / 64 > 0 ? NT / 64 : 1][2], red_cnt[NT / 64 > 0 ? NT / 64 : 1][2];

    const int tid = threadIdx.x;
    const int w = xcd_work_item(blockIdx.x, gridDim.x);
    const int C = a.C, units = a.n_eng * C;
    const int rr = w / units, pp = w - rr * units;
    const int g = pp / C, c = pp - g * C;
    const int gc = g * C + c;
    const int t0 = rr * run_len, t1 = min(a.n_t, t0 + run_len);          // run_len is even
    if (t0 >= t1) return;

    float2 B[F::NBREG];
    F::load_bases(B, ldsb, twb, tid);

    const float *__restrict__ ya0 = a.y + (long)gc * a.y_ch_stride;
    float *__restrict__ out0 = a.raw + (long)g * a.eng_stride + a.frame_off * C + c;
    const unsigned blk_bytes = (unsigned)L * C * 4u;
    const unsigned cio = (unsigned)C;                                    // floats between a channel's consecutive samples
    static_assert(Q == 4, "the prefetch statement moves four 16-byte pieces per thread and spectrum");
    u32x4 qa[Q], qb[Q];
    {
        const __amdgpu_buffer_rsrc_t ra = make_rsrc(ya0 + (long)t0 * N, (unsigned)N * 4u);
        const __amdgpu_buffer_rsrc_t rb = make_rsrc(ya0 + (long)(t0 + 1) * N, t0 + 1 < t1 ? (unsigned)N * 4u : 0u);
#pragma unroll
        for (int j = 0; j < Q; j++) {
            qa[j] = __builtin_amdgcn_raw_buffer_load_b128(ra, (unsigned)tid * 16u, (unsigned)(j * NT) * 16u, 2);
            qb[j] = __builtin_amdgcn_raw_buffer_load_b128(rb, (unsigned)tid * 16u, (unsigned)(j * NT) * 16u, 2);
        }
#pragma unroll
        for (int j = 0; j < Q; j++) asm volatile("" : "+v"(qa[j]), "+v"(qb[j]));
    }
    const float rmax = a.max;
    float pk0 = 0.f, pk1 = 0.f;
    unsigned int c0 = 0u, c1 = 0u;
    int bad = 0x7fffffff;
    for (int t = t0; t < t1; t += 2) {
        int ts = tid; asm volatile("" : "+v"(ts));
        // the two spectra have landed when all but the P output stores issued after their prefetch are done
        asm_wait_vmcnt<P>(qa, qb);
        __syncthreads();                                                 // the previous transform's readers are done
        {
            u32x4 *l4 = (u32x4 *)lds;
#pragma unroll
            for (int j = 0; j < Q; j++) { l4[ts + j * NT] = qa[j]; l4[L / 2 + ts + j * NT] = qb[j]; }
        }
        __syncthreads();
        // Z[k] = Ya[k] + i Yb[k], Hermitian-extended to the full circle (k_inv_pair_ps)
        float re[P], im[P];
        static_for<0, P>([&](auto E_) {
            constexpr int e = decltype(E_)::value;
            constexpr int base = F::in_index(0, e);
            static_assert(base + NT <= L || base >= L, "a thread's points do not straddle L");
            const int k = base + ts;
            const int kk = (base < L) ? k : N - k;
            const bool edge = (base == 0 || base == L) && ts == 0;
            const float2 pa = lds[edge ? 0 : kk], pb = lds[L + (edge ? 0 : kk)];
            float zr, zi;
            if (base < L) { zr = pa.x - pb.y; zi = pa.y + pb.x; }
            else          { zr = pa.x + pb.y; zi = pb.x - pa.y; }
            if (base == 0) { zr = edge ? pa.x : zr; zi = edge ? pb.x : zi; }
            if (base == L) { zr = edge ? pa.y : zr; zi = edge ? pb.y : zi; }
            re[e] = zr * a.scale; im[e] = zi * a.scale;
        });
        pin_registers(re, im);
        {
            float2 w0[1];
            F::template butterflies<0>(re, im, w0);
        }
        static_for<1, F::NP>([&](auto S_) {
            constexpr int S = decltype(S_)::value;
            int tl = tid; asm volatile("" : "+v"(tl));
            F::template exchange<S - 1>(re, im, lds, tl);
            F::template butterflies_tb<S>(re, im, B, ldsb, tl);
            if constexpr (S == 1) {
                asm_prefetch2x4x4(qa, qb, (unsigned)tl * 16u,
                                  make_rsrc_words(ya0 + (long)(t + 2) * N, t + 2 < t1 ? (unsigned)N * 4u : 0u),
                                  make_rsrc_words(ya0 + (long)(t + 3) * N, t + 3 < t1 ? (unsigned)N * 4u : 0u), (unsigned)NT * 16u);
            }
        });

        // first L samples are the valid half: Re -> block t, Im -> block t + 1
        const bool has_b = t + 1 < a.n_t;
        const __amdgpu_buffer_rsrc_t roa = make_rsrc(out0 + (long)t * L * C, blk_bytes);
        const __amdgpu_buffer_rsrc_t rob = make_rsrc(out0 + (long)(t + 1) * L * C, has_b ? blk_bytes : 0u);
        int to = tid; asm volatile("" : "+v"(to));
#pragma unroll
        for (int e = 0; e < P; e++) {
            const int n = F::out_index(to, e);
            if (F::out_index(0, e) < L) {
                const float va = re[e], vb = has_b ? im[e] : 0.f;
                buf_store1(roa, (unsigned)to * cio * 4u, (unsigned)F::out_index(0, e) * cio * 4u, va);
                buf_store1(rob, (unsigned)to * cio * 4u, (unsigned)F::out_index(0, e) * cio * 4u, vb);
                c0 += (fabsf(va) > rmax) ? 1u : 0u;
                c1 += (fabsf(vb) > rmax) ? 1u : 0u;
                pk0 = fmaxf(pk0, fabsf(va)); pk1 = fmaxf(pk1, fabsf(vb));
                // brutefir/brutefir.cpp:316-321: only sample 0 of each block is checked
                if (F::out_index(0, e) == 0) {
                    const bool na = n == 0 && !isfinite(va), nbb = n == 0 && has_b && !isfinite(vb);
                    bad = (na && t < bad) ? t : bad;
                    bad = (nbb && t + 1 < bad) ? t + 1 : bad;
                }
            }
        }
    }
    asm_wait_vmcnt<0>(qa, qb);                                           // see k_inv_pair_ps
    if (bad != 0x7fffffff) flag_bad(a, bad);
    unsigned int mx0 = __float_as_uint(fmaxf(pk0, pk1)), mx1 = 0u;       // one channel: its peak over both blocks
    c0 += c1; c1 = 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned int m0 = __shfl_xor(mx0, o);
        mx0 = m0 > mx0 ? m0 : mx0;
        c0 += __shfl_xor(c0, o);
    }
    if ((tid & 63) == 0) { red_max[tid >> 6][0] = mx0; red_cnt[tid >> 6][0] = c0; }
    __syncthreads();
    if (tid == 0) {
        unsigned int m = 0u, n = 0u;
        for (int wv = 0; wv < (NT + 63) / 64; wv++) { m = red_max[wv][0] > m ? red_max[wv][0] : m; n += red_cnt[wv][0]; }
        DevOverflow *of = of_shard(a.overflow, a.of_shard_stride) + gc;
        if (n) atomicAdd(&of->n_overflows, n);
        if ((unsigned long long)m > *(volatile unsigned long long *)&of->largest_bits)
            atomicMax(&of->largest_bits, (unsigned long long)m);
    }
    (void)mx1;
}

}  // namespace

#define BFIR_FOR_PAIR_LOG2N(F) F(10) F(11) F(12) F(13) F(14)

bool pair_supported(int filter_length)
{
    return filter_length >= 512 && filter_length <= 8192;             // N = 2L complex points, 2^10 .. 2^14 (whole waves)
}

// Blocks per workgroup of the persistent kernels.  Long runs are best for a kernel on its own (forward:
// 16 blocks) but the engine runs forward, MAC and inverse of neighbouring chunks concurrently, and a
// kernel made of a few hundred long-lived workgroups holds every CU slot until it ends, so the other
// two cannot slip in: the pipeline is fastest with SHORT runs (profiles/r02_pair_run_sweep.txt:
// 108 Gsamples/s at 4 blocks per workgroup against 95 at 32).  BFIR_PAIR_RUN_FWD / _INV override (tuning aid).
static int pair_run_len(int n_t, int pairs, bool inverse)
{
    if (const char *e = getenv(inverse ? "BFIR_PAIR_RUN_INV" : "BFIR_PAIR_RUN_FWD")) return std::max(1, atoi(e));
    const int slots = 512;                                 // 256 CUs x 2 workgroups
    const int runs = std::max(1, slots / std::max(1, pairs));
    const int fill = std::max(1, (n_t + runs - 1) / runs); // what one round of workgroups would need
    return std::min(fill, 4);
}

void launch_fwd_pair(const FftPlan &plan, const FwdPairArgs &a, hipStream_t s)
{
    if (a.tp) {                                            // pairs in time: one unit per channel, runs of an even number of blocks
        const int units = a.n_eng * a.C;
        if (a.n_t <= 0 || units <= 0 || !plan.twb) return;
        // as many TRANSFORMS per workgroup as the channel-pair kernels take (a transform is two blocks here): 105.5 against
        // 103.4 Gsamples/s at 7 channels, 104.2 against 101.7 at one (profiles/r03_channels.txt)
        const int len = 2 * pair_run_len((a.n_t + 1) / 2, units, false), runs = (a.n_t + len - 1) / len;
        switch (plan.log2m) {
#define F(lg) case lg: hipLaunchKernelGGL((k_fwd_tp_ps<lg>), dim3(runs * units), dim3(FftCfg<lg>::NT), 0, s, a, (const float2 *)plan.twb, len); break;
            BFIR_FOR_PAIR_LOG2N(F)
#undef F
        }
        return;
    }
    if (launch_fwd_wide(plan, a, s)) return;               // two channel pairs per workgroup, 16-byte frame loads (wide.hip)
    const int pairs = a.n_eng * (a.C / 2);
    if (a.n_t <= 0 || pairs <= 0 || !plan.twb) return;
    const int len = pair_run_len(a.n_t, pairs, false), runs = (a.n_t + len - 1) / len;
    switch (plan.log2m) {
#define F(lg) case lg: hipLaunchKernelGGL((k_fwd_pair_ps<lg>), dim3(runs * pairs), dim3(FftCfg<lg>::NT), 0, s, a, (const float2 *)plan.twb, len); break;
        BFIR_FOR_PAIR_LOG2N(F)
#undef F
    }
}

void launch_inv_pair(const FftPlan &plan, const InvPairArgs &a, hipStream_t s)
{
    if (a.tp) {                                            // pairs in time (k_inv_tp_ps)
        const int units = a.n_eng * a.C;
        if (a.n_t <= 0 || units <= 0 || !plan.twb) return;
        const int len = 2 * pair_run_len((a.n_t + 1) / 2, units, true), runs = (a.n_t + len - 1) / len;
        switch (plan.log2m) {
#define F(lg) case lg: hipLaunchKernelGGL((k_inv_tp_ps<lg>), dim3(runs * units), dim3(FftCfg<lg>::NT), 0, s, a, (const float2 *)plan.twb, len); break;
            BFIR_FOR_PAIR_LOG2N(F)
#undef F
        }
        return;
    }
    if (launch_inv_quad(plan, a, s)) return;               // two channel pairs per workgroup, 16-byte frame stores (quad.hip)
    const int pairs = a.n_eng * (a.C / 2);
    if (a.n_t <= 0 || pairs <= 0 || !plan.twb) return;
    const int len = pair_run_len(a.n_t, pairs, true), runs = (a.n_t + len - 1) / len;
    switch (plan.log2m) {
#define F(lg) case lg: hipLaunchKernelGGL((k_inv_pair_ps<lg>), dim3(runs * pairs), dim3(FftCfg<lg>::NT), 0, s, a, (const float2 *)plan.twb, len); break;
        BFIR_FOR_PAIR_LOG2N(F)
#undef F
    }
}

}  // namespace bfir
