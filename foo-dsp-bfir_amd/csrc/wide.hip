// wide.hip -- the forward transform of the float fast path with whole 16-byte pieces of the input frames.
//
// k_fwd_pair_ps (pair.hip) turns the frames of ONE channel pair into delay-line spectra: a lane loads 8 bytes of every
// 32-byte frame (C = 8), a wave instruction touches 16 cache lines and uses a quarter of each, and half of its
// vector-memory instructions do nothing a 16-byte load would not do.  (The L2 merges those quarters, HBM sees each line
// about once either way: what this kernel saves is load instructions and L2 requests, profiles/wide_io.txt.)
//
// Here one workgroup owns channels 4q .. 4q + 3 of one engine for a run of consecutive blocks and transforms, per block,
// pair A (4q, 4q + 1), then pair B (4q + 2, 4q + 3), each exactly as k_fwd_pair_ps does it -- the same window
// [block t-1 | block t], the same 0.5 * scale folded into the input, the same passes, split, DC | Nyquist fix-up and
// nontemporal 16-byte spectrum stores, hence the same bits.  A block is loaded once, in eight 16-byte pieces per thread.
//
// Registers (the reason k_inv_quad_ps had no forward sibling at first: both pairs' carried half-window, 32, plus both
// pairs' prefetch, 32, on top of the 32 of the butterflies and their temporaries do not fit four waves per SIMD if all of
// it is live through both transforms).  The schedule that fits:
//   * the ONE prefetch statement of a block (eight buffer_load_dwordx4: block t + 1, both pairs) is issued only under
//     pair B's passes, when B's raw half of block t has been consumed;
//   * its destinations are OUTPUTS of the statement ("=&v", as asm_prefetch2x4x4_out in quad.hip), so between the top of
//     the block and the prefetch those 32 registers are the compiler's;
//   * under A's passes: 32 working + 32 carried + 16 (B's raw half of block t); under B's: 32 + 32 + 32 prefetch.
// Exactly pair B's eight spectrum stores follow the prefetch, so block t + 1 has landed at "all but 8".
#include "kernels.h"

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>

#include "fft_lds.h"
#include "pair_io.h"

namespace bfir {

namespace {

// The pass of pair B's transform under which the next block is fetched: 1, behind the widest butterflies, as in
// k_fwd_pair_ps.  One pass later (2) needs four registers fewer at N = 8192 and was slower in the pipeline
// (profiles/wide_io.txt).
constexpr int WIDE_PF_PASS = 1;

// 8 x 16 bytes per lane: d[e] <- buffer[voff + e * step], destinations as outputs (see above).  No `nt`: the other quad
// of the frame line reads the same lines from the same L2.
__device__ __forceinline__ void asm_prefetch8x4_out(u32x4 (&d)[8], unsigned voff, i32x4 r, unsigned step)
{
    const unsigned s1 = __builtin_amdgcn_readfirstlane(step), s2 = 2 * s1, s3 = 3 * s1, s4 = 4 * s1, s5 = 5 * s1, s6 = 6 * s1, s7 = 7 * s1;
    asm volatile("s_nop 4\n\t"
                 "buffer_load_dwordx4 %0, %8, %9, 0 offen\n\t"
                 "buffer_load_dwordx4 %1, %8, %9, %10 offen\n\t"
                 "buffer_load_dwordx4 %2, %8, %9, %11 offen\n\t"
                 "buffer_load_dwordx4 %3, %8, %9, %12 offen\n\t"
                 "buffer_load_dwordx4 %4, %8, %9, %13 offen\n\t"
                 "buffer_load_dwordx4 %5, %8, %9, %14 offen\n\t"
                 "buffer_load_dwordx4 %6, %8, %9, %15 offen\n\t"
                 "buffer_load_dwordx4 %7, %8, %9, %16 offen"
                 : "=&v"(d[0]), "=&v"(d[1]), "=&v"(d[2]), "=&v"(d[3]), "=&v"(d[4]), "=&v"(d[5]), "=&v"(d[6]), "=&v"(d[7])
                 : "v"(voff), "s"(r), "s"(s1), "s"(s2), "s"(s3), "s"(s4), "s"(s5), "s"(s6), "s"(s7)
                 : "memory");
}

template <int LOG2N>
__global__ __launch_bounds__(FftCfg<LOG2N>::NT, 4) void k_fwd_wide_ps(FwdPairArgs a, const float2 *__restrict__ twb, int run_len)
{
    using F = LdsFft<float, LOG2N, -1>;
    constexpr int N = F::M, NT = F::NT, P = F::P, L = N / 2, H = P / 2;   // H points per thread and block
    static_assert(F::radix(0) == 16 && P == 16, "in_index(tid, e) = tid + e * (N / 16)");
    static_assert(F::phys(32) == 33 && F::phys(N - 1) == N - 1 + N / 32 - 1, "the split step's addresses assume i + (i >> 5)");
    static_assert(WIDE_PF_PASS >= 1 && WIDE_PF_PASS < F::NP, "the prefetch goes under one of the passes behind the first");
    __shared__ __attribute__((aligned(16))) float2 lds[F::LDS_ELEMS + 1];   // + 1: see the split step of k_fwd_pair_ps
    __shared__ __attribute__((aligned(16))) float2 ldsb[F::LDSB_ELEMS];

    const int tid = threadIdx.x;
    const int w = xcd_work_item(blockIdx.x, gridDim.x);
    const int quarter_c = a.C / 4, units = a.n_eng * quarter_c;
    const int rr = w / units, pp = w - rr * units;                       // run, quad: the quads of a run share an XCD
    const float sc = 0.5f * a.scale;                                     // the split's 1/2, see k_fwd_pair_ps
    const int g = pp / quarter_c, cq = pp - g * quarter_c;
    const int C = a.C;
    const int t0 = rr * run_len, t1 = min(a.n_t, t0 + run_len);
    if (t0 >= t1) return;

    float2 B[F::NBREG];
    F::load_bases(B, ldsb, twb, tid);                                    // the first exchange's barrier publishes ldsb

    // frame n = tid + e NT of a block of frames sits at byte  blk + 4 (e NT C + tid C)  (+ 16 cq for the quad)
    const float *__restrict__ raw = a.raw + (long)g * a.eng_stride + a.frame_off * C + 4 * cq;
    const long hist = (long)g * a.hist_eng_stride + 4 * cq;
    const unsigned blk_bytes = (unsigned)L * C * 4u;
    const unsigned fo = (unsigned)tid * (unsigned)C * 4u;                // lane offset into a block of frames
    const unsigned estep = (unsigned)NT * C * 4u;                        // bytes between a thread's consecutive points
    static_assert(H == 8, "the prefetch statement moves eight 16-byte pieces per thread");
    float4 cur[H];                                                       // block t - 1, scaled: pair A in .xy, pair B in .zw
    u32x4 nxt[H];                                                        // raw frames of the next block, as loaded
    {
        const __amdgpu_buffer_rsrc_t ro = make_rsrc((t0 == 0) ? a.prev + hist : raw + (long)(t0 - 1) * L * C, blk_bytes);
#pragma unroll
        for (int e = 0; e < H; e++) {
            const float4 v = buf_load4(ro, fo, e * estep);
            cur[e].x = v.x * sc; cur[e].y = v.y * sc; cur[e].z = v.z * sc; cur[e].w = v.w * sc;
        }
        if (a.n_t == 1) {
            // one-block chunk: the other history block moves on unchanged (carry -> save_prev), done here as the pair
            // kernel does it, so that such launches need not be declined
            const __amdgpu_buffer_rsrc_t rc = make_rsrc(a.carry + hist, blk_bytes);
            u32x4 mv[H];
#pragma unroll
            for (int e = 0; e < H; e++) mv[e] = __builtin_amdgcn_raw_buffer_load_b128(rc, fo, e * estep, 0);
            asm_store8x4(mv, fo, make_rsrc_words(a.save_prev + hist, blk_bytes), estep);
        }
        const __amdgpu_buffer_rsrc_t rb = make_rsrc(raw + (long)t0 * L * C, blk_bytes);
#pragma unroll
        for (int e = 0; e < H; e++) nxt[e] = __builtin_amdgcn_raw_buffer_load_b128(rb, fo, e * estep, 0);
        // these (compiler-counted) loads are consumed before the loop, so inside it the compiler has no
        // pending load of its own to wait for
#pragma unroll
        for (int e = 0; e < H; e++) asm volatile("" : "+v"(nxt[e]));
    }
    float *__restrict__ da0 = a.dst + (long)(g * C + 4 * cq) * a.dst_ch_stride;
    for (int t = t0; t < t1; t++) {
        // block t has landed when all but pair B's 2 (P/4) spectrum stores issued after its prefetch are done
        asm_wait_vmcnt<2 * (P / 4)>(nxt);
        if (t >= a.n_t - 2) {                                            // uniform: the chunk's last two blocks
            // the engine's history: raw frames of the last two blocks of the chunk, the layout of k_fwd_pair_ps (one asm
            // statement, see asm_store8x4; after the counted wait, i.e. outside the window it spans)
            asm_store8x4(nxt, fo, make_rsrc_words((t == a.n_t - 1 ? a.save_last : a.save_prev) + hist, blk_bytes), estep);
        }
        unsigned bx[H], by[H];                                           // pair B's raw half of block t waits through A's transform
#pragma unroll
        for (int e = 0; e < H; e++) { bx[e] = nxt[e].z; by[e] = nxt[e].w; }
        static_for<0, 2>([&](auto PR_) {
            constexpr int PR = decltype(PR_)::value;                     // 0: pair A, 1: pair B
            float re[P], im[P];
#pragma unroll
            for (int e = 0; e < H; e++) {                                // window = [block t-1 | block t]
                if constexpr (PR == 0) {
                    re[e] = cur[e].x; im[e] = cur[e].y;
                    cur[e].x = __uint_as_float(nxt[e].x) * sc; cur[e].y = __uint_as_float(nxt[e].y) * sc;
                    re[H + e] = cur[e].x; im[H + e] = cur[e].y;
                } else {
                    re[e] = cur[e].z; im[e] = cur[e].w;
                    cur[e].z = __uint_as_float(bx[e]) * sc; cur[e].w = __uint_as_float(by[e]) * sc;
                    re[H + e] = cur[e].z; im[H + e] = cur[e].w;
                }
            }
            {
                float2 w0[1];
                F::template butterflies<0>(re, im, w0);
            }
            static_for<1, F::NP>([&](auto S_) {
                constexpr int S = decltype(S_)::value;
                // LDS addresses afresh per phase from an opaque copy of the lane index (k_fwd_pair_ps).  The first
                // exchange opens with a barrier: B's protects A's split reads, A's those of the block before.
                int tl = tid; asm volatile("" : "+v"(tl));
                F::template exchange<S - 1>(re, im, lds, tl);
                F::template butterflies_tb<S>(re, im, B, ldsb, tl);
                if constexpr (PR == 1 && S == WIDE_PF_PASS) {
                    // block t+1, both pairs, under B's remaining passes; past the end of the run the descriptor has
                    // zero bytes and the loads return zeros (no branch in the loop)
                    asm_prefetch8x4_out(nxt, fo, make_rsrc_words(raw + (long)(t + 1) * L * C, t + 1 < t1 ? blk_bytes : 0u), estep);
                }
            });

            // Z in natural order to LDS, then two-for-one split: k_fwd_pair_ps, statement for statement
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
            float *da = da0 + (long)(2 * PR) * a.dst_ch_stride + slot;   // pair B: two channel strides further on
            const __amdgpu_buffer_rsrc_t rxa = make_rsrc(da, (unsigned)N * 4u), rxb = make_rsrc(da + a.dst_ch_stride, (unsigned)N * 4u);
            const float2 *zk = lds + F::phys(2 * tz);
            constexpr int OMAX = F::phys(2 * NT * (P / 4 - 1));          // bases lowered so that every offset is >= 0
            const float2 *zn1 = lds + (F::phys(N - 1 - 2 * tz) - OMAX);
            const float2 *zn0 = zn1 + ((tz & 15) == 0 ? 2 : 1);
#pragma unroll
            for (int j = 0; j < P / 4; j++) {
                if (j > 0) __builtin_amdgcn_sched_barrier(0);            // one pair of bins at a time (k_fwd_pair_ps)
                const int o = F::phys(2 * NT * j);
                const float2 zk0 = zk[o], zk1 = zk[o + 1];
                const float2 zn0v = zn0[OMAX - o], zn1v = zn1[OMAX - o];
                float4 xa, xb;
                xa.x = zk0.x + zn0v.x; xa.y = zk0.y - zn0v.y;
                xb.x = zk0.y + zn0v.y; xb.y = zn0v.x - zk0.x;
                xa.z = zk1.x + zn1v.x; xa.w = zk1.y - zn1v.y;
                xb.z = zk1.y + zn1v.y; xb.w = zn1v.x - zk1.x;
                if (j == 0) {                                            // m = tid: bin 0 is DC | Nyquist, both real
                    const float2 zh = lds[F::phys(L)];
                    const bool k0 = tz == 0;
                    xa.x = k0 ? 2.f * zk0.x : xa.x; xa.y = k0 ? 2.f * zh.x : xa.y;
                    xb.x = k0 ? 2.f * zk0.y : xb.x; xb.y = k0 ? 2.f * zh.y : xb.y;
                }
                buf_store4<2>(rxa, (unsigned)tz * 16u, (unsigned)(j * NT) * 16u, xa);
                buf_store4<2>(rxb, (unsigned)tz * 16u, (unsigned)(j * NT) * 16u, xb);
            }
        });
    }
    // The last prefetch (zero-byte descriptor: it returns zeros) is still in flight and will write nxt[]:
    // those registers must not be handed to anything else before it has landed.
    asm_wait_vmcnt<0>(nxt);
}

}  // namespace

// N = 8192 and 16384: 118 registers, no scratch, four waves per SIMD as k_fwd_pair_ps (87 / 88), the LDS of that kernel.
// N = 4096 is not instantiated: its last pass is a radix-16 one with six base twiddles in registers, and at four waves
// per SIMD (128 registers) the compiler's report shows 172 bytes of scratch per lane (42 registers spilled; 20 bytes / 4
// registers with the prefetch under pass 2) -- a spill is a vector-memory operation inside the counted window
// (tests/test_wide_isa.py holds the others to none).  N = 1024 and 2048 stay on the pair kernel too: no scratch at four
// waves (118 / 126 registers; 110 / 118 under pass 2), but their pair kernels reach five (87 / 94 registers), which this
// kernel's live set (96 registers under pair B's passes before any temporary) cannot.
#define BFIR_FOR_WIDE_LOG2N(F) F(13) F(14)

static std::atomic<int64_t> g_wide_launches{0};            // bfir_fwd_wide_launches, below

// Blocks per workgroup (two transforms each): 4.  Unlike the inverse (quad_run_len: 2, the four transforms of a pair
// kernel's workgroup) this kernel carries its half-window from block to block, so a run of n blocks loads n + 1: in the
// pipeline 2 / 3 / 4 blocks gave 119.0-119.6 / 120.0-121.0 / 120.3-121.0 Gsamples/s against the parent's 117.6-118.7, 6 the
// same as 4 and 8 less (profiles/wide_io.txt).  BFIR_WIDE_RUN_FWD overrides (tuning aid).
static int wide_run_len(int n_t, int units)
{
    if (const char *e = getenv("BFIR_WIDE_RUN_FWD")) return std::max(1, atoi(e));
    const int slots = 512;                                 // 256 CUs x 2 workgroups
    const int runs = std::max(1, slots / std::max(1, units));
    const int fill = std::max(1, (n_t + runs - 1) / runs); // what one round of workgroups would need
    return std::min(fill, 4);
}

// Sizes at which the kernel was measured to pay in the pipeline (profiles/wide_io.txt): what FwdPairArgs.wide = -1 takes.
// N = 16384 (one workgroup per CU: 148 KB of LDS) is not among them: 8 channels at L = 8192 ran at 114.7-118.1 Gsamples/s
// (117.8-121.3 with 2 blocks per workgroup) against the parent's 117.3-120.8; BFIR_FWD_WIDE=1 takes it there too.
static bool wide_pays(int log2m) { return log2m == 13; }

// Takes the launch where the frames can be read in 16-byte pieces; false: the caller's pair kernel does it.
bool launch_fwd_wide(const FftPlan &plan, const FwdPairArgs &a, hipStream_t s)
{
    if (a.tp || a.wide == 0 || a.C <= 0 || a.C % 4 != 0) return false;
    // every piece 16-byte aligned: the frames and the four history blocks (a one-block chunk is taken too: the kernel
    // moves carry -> save_prev itself)
    const uintptr_t ptrs = (uintptr_t)a.raw | (uintptr_t)a.prev | (uintptr_t)a.save_last | (uintptr_t)a.save_prev | (uintptr_t)a.carry;
    if ((ptrs & 15u) != 0 || (a.eng_stride & 3) != 0 || (a.hist_eng_stride & 3) != 0) return false;
    const int units = a.n_eng * (a.C / 4);
    if (a.n_t <= 0 || units <= 0 || !plan.twb) return false;
    // Two transforms in turn per workgroup: by default only where the launch fills the GPU anyway, so that a call of
    // a few blocks (the latency path) keeps one transform per workgroup.  BFIR_FWD_WIDE=1 lifts that.
    if (a.wide < 0 && ((long)a.n_t * units < 512 || !wide_pays(plan.log2m))) return false;
    const int len = wide_run_len(a.n_t, units), runs = (a.n_t + len - 1) / len;
    switch (plan.log2m) {
#define F(lg) case lg: hipLaunchKernelGGL((k_fwd_wide_ps<lg>), dim3(runs * units), dim3(FftCfg<lg>::NT), 0, s, a, (const float2 *)plan.twb, len); break;
        BFIR_FOR_WIDE_LOG2N(F)
#undef F
        default: return false;
    }
    g_wide_launches.fetch_add(1, std::memory_order_relaxed);
    return true;
}

}  // namespace bfir

// Launches of k_fwd_wide_ps in this process.  For tests/test_wide_path_gpu.py, not part of the public interface: which
// kernel took a launch cannot be seen from the output, whose bits are those of the pair kernel.
extern "C" int64_t bfir_fwd_wide_launches(void) { return bfir::g_wide_launches.load(std::memory_order_relaxed); }
