// quad.hip -- the inverse of the float fast path with whole 16-byte pieces of the output frames.
//
// k_inv_pair_ps (pair.hip) turns the product spectra of ONE channel pair into output frames: each of its workgroups
// stores 8 bytes into every frame of its blocks, so the C/2 pair-workgroups of a block write every 32-byte sector of
// the frames in quarters (C = 8), which the L2 merges only part of the time (0.75 - 0.94 GB written for 0.537 GB of
// frames at the headline), and a thread issues sixteen 8-byte stores per transform -- vector stores are bound by
// instruction issue, not by bytes (MI355X_MICROARCH.md cycle table).
//
// The inverse kernel carries nothing from block to block, so one workgroup can do TWO channel pairs of a block in turn:
// pair A (channels 4q, 4q + 1), then pair B (4q + 2, 4q + 3), each exactly as k_inv_pair_ps does it -- the same staging,
// Hermitian extension, passes and scale, hence the same bits.  A's valid half (8 points x 2 channels = 16 registers)
// waits in registers through B's transform, and the two halves leave together: eight 16-byte stores per thread and
// block (channels 4q .. 4q + 3 of a frame) instead of 2 x 8 eight-byte ones.
#include "kernels.h"

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>

#include "fft_lds.h"
#include "pair_io.h"

namespace bfir {

namespace {

// The prefetch alternates: under A's passes the two spectra of pair B of the same block, under B's passes those of pair
// A of the next block (zero-byte descriptors past the end of the run, as in k_inv_pair_ps).  The eight stores of a block
// are issued after B's passes, i.e. after the prefetch of the next block's A: A waits for "all but 8", B -- nothing
// follows its prefetch -- for "all but 0".  The alternation is unrolled (static_for over the pair) so that each wait is
// a compile-time constant; scripts/audit_ps_isa.py (audit_quad) counts both windows in the emitted code.
//
// Registers: A's half costs 16 on top of what k_inv_pair_ps holds through the passes, more than the widest butterflies
// leave at four waves per SIMD.  So the prefetch destinations are OUTPUTS of the prefetch statement here ("=&v", not the
// "+v" of asm_prefetch2x4x4): between the staging of a transform and its prefetch -- the Hermitian extension and the two
// radix-16 passes -- those 32 registers are free for the butterflies (cdna_hip_programming.md 5.7 form (ii)).
__device__ __forceinline__ void asm_prefetch2x4x4_out(u32x4 (&a)[4], u32x4 (&b)[4], unsigned voff, i32x4 ra, i32x4 rb, unsigned step)
{
    const unsigned s1 = __builtin_amdgcn_readfirstlane(step), s2 = 2 * s1, s3 = 3 * s1;
    asm volatile("s_nop 4\n\t"
                 "buffer_load_dwordx4 %0, %8, %9, 0 offen nt\n\t"
                 "buffer_load_dwordx4 %4, %8, %10, 0 offen nt\n\t"
                 "buffer_load_dwordx4 %1, %8, %9, %11 offen nt\n\t"
                 "buffer_load_dwordx4 %5, %8, %10, %11 offen nt\n\t"
                 "buffer_load_dwordx4 %2, %8, %9, %12 offen nt\n\t"
                 "buffer_load_dwordx4 %6, %8, %10, %12 offen nt\n\t"
                 "buffer_load_dwordx4 %3, %8, %9, %13 offen nt\n\t"
                 "buffer_load_dwordx4 %7, %8, %10, %13 offen nt"
                 : "=&v"(a[0]), "=&v"(a[1]), "=&v"(a[2]), "=&v"(a[3]), "=&v"(b[0]), "=&v"(b[1]), "=&v"(b[2]), "=&v"(b[3])
                 : "v"(voff), "s"(ra), "s"(rb), "s"(s1), "s"(s2), "s"(s3)
                 : "memory");
}

template <int LOG2N>
__global__ __launch_bounds__(FftCfg<LOG2N>::NT, inv_ps_min_waves<LOG2N>()) void k_inv_quad_ps(InvPairArgs a, const float2 *__restrict__ twb, int run_len)
{
    using F = LdsFft<float, LOG2N, +1>;
    constexpr int N = F::M, NT = F::NT, P = F::P, L = N / 2, Q = P / 4;   // Q 16-byte pieces per thread and spectrum
    constexpr int NW = NT / 64 > 0 ? NT / 64 : 1;
    __shared__ __attribute__((aligned(16))) float2 lds[F::LDS_ELEMS];
    __shared__ __attribute__((aligned(16))) float2 ldsb[F::LDSB_ELEMS];
    __shared__ unsigned int red_max[NW][4], red_cnt[NW][4];

    const int tid = threadIdx.x;
    const int w = xcd_work_item(blockIdx.x, gridDim.x);
    const int quarter_c = a.C / 4, units = a.n_eng * quarter_c;
    const int rr = w / units, pp = w - rr * units;                       // run, quad: the quads of a run share an XCD
    const int g = pp / quarter_c, cq = pp - g * quarter_c;
    const int C = a.C;
    const int gc = g * C + 4 * cq;
    const int t0 = rr * run_len, t1 = min(a.n_t, t0 + run_len);
    if (t0 >= t1) return;

    float2 B[F::NBREG];
    F::load_bases(B, ldsb, twb, tid);

    const float *__restrict__ ya0 = a.y + (long)gc * a.y_ch_stride;
    float *__restrict__ out0 = a.raw + (long)g * a.eng_stride + a.frame_off * C + 4 * cq;
    const unsigned blk_bytes = (unsigned)L * C * 4u;
    const unsigned cio = (unsigned)C;                                    // floats between consecutive frames
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
    // overflow statistics and the NaN verdict per channel, as in k_inv_pair_ps
    const float rmax = a.max;
    float pk[4] = {0.f, 0.f, 0.f, 0.f};
    unsigned int cn[4] = {0u, 0u, 0u, 0u};
    int bad = 0x7fffffff;
    for (int t = t0; t < t1; t++) {
        float hr[P], hi[P];                                              // pair A's valid half (the entries with out_index < L)
        static_for<0, 2>([&](auto PR_) {
            constexpr int PR = decltype(PR_)::value;                     // 0: pair A, 1: pair B
            // both spectra into LDS: Ya at [0, L), Yb at [L, 2L)  (float2 units)
            int ts = tid; asm volatile("" : "+v"(ts));
            if constexpr (PR == 0) asm_wait_vmcnt<P / 2>(qa, qb);        // all but the block's P/2 stores, issued after A's prefetch
            else asm_wait_vmcnt<0>(qa, qb);                              // nothing was issued after B's prefetch
            __syncthreads();                                             // the previous transform's readers are done
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
                const int kk = (base < L) ? k : N - k;                   // kk == L only for base == L, tid == 0
                const bool edge = (base == 0 || base == L) && ts == 0;
                const float2 pa = lds[edge ? 0 : kk], pb = lds[L + (edge ? 0 : kk)];
                float zr, zi;
                if (base < L) { zr = pa.x - pb.y; zi = pa.y + pb.x; }
                else          { zr = pa.x + pb.y; zi = pb.x - pa.y; }     // conj Ya + i conj Yb
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
                    // under A's passes pair B of this block, under B's passes pair A of the next one; past the end of
                    // the run the descriptors have zero bytes and the loads return zeros (no branch in the loop)
                    const int tn = t + PR;
                    const unsigned nbytes = tn < t1 ? (unsigned)N * 4u : 0u;
                    const float *yn = ya0 + (long)(2 - 2 * PR) * a.y_ch_stride + (long)tn * N;
                    asm_prefetch2x4x4_out(qa, qb, (unsigned)tl * 16u, make_rsrc_words(yn, nbytes),
                                          make_rsrc_words(yn + a.y_ch_stride, nbytes), (unsigned)NT * 16u);
                }
            });

            // first L samples are the valid half (the taps sit in the upper half of their blocks)
            int to = tid; asm volatile("" : "+v"(to));
            u32x4 fo[P / 2];                                             // pair B: the block's eight 16-byte pieces, by frame
#pragma unroll
            for (int e = 0; e < P; e++) {
                const int n = F::out_index(to, e);
                if (F::out_index(0, e) < L) {                            // compile time: out_index(tid, e) = tid + const, tid < NT <= L
                    float2 v; v.x = re[e]; v.y = im[e];
                    if constexpr (PR == 0) { hr[e] = v.x; hi[e] = v.y; }
                    else {
                        u32x4 &f = fo[F::out_index(0, e) / NT];          // a thread's valid points are NT frames apart
                        f.x = __float_as_uint(hr[e]); f.y = __float_as_uint(hi[e]); f.z = __float_as_uint(v.x); f.w = __float_as_uint(v.y);
                    }
                    cn[2 * PR] += (fabsf(v.x) > rmax) ? 1u : 0u;
                    cn[2 * PR + 1] += (fabsf(v.y) > rmax) ? 1u : 0u;
                    pk[2 * PR] = fmaxf(pk[2 * PR], fabsf(v.x)); pk[2 * PR + 1] = fmaxf(pk[2 * PR + 1], fabsf(v.y));
                    // brutefir/brutefir.cpp:316-321: only sample 0 of each block is checked; the first bad block
                    // of the run, of either pair, is reported once, after the loop (no atomic inside it)
                    if (F::out_index(0, e) == 0) {
                        const bool nf = n == 0 && !(isfinite(v.x) && isfinite(v.y));
                        bad = (nf && t < bad) ? t : bad;
                    }
                }
            }
            if constexpr (PR == 1)
                asm_store8x4(fo, (unsigned)to * cio * 4u, make_rsrc_words(out0 + (long)t * L * C, blk_bytes), (unsigned)NT * cio * 4u);
        });
    }
    // The last prefetch (zero-byte descriptors: it returns zeros) is still in flight and will write qa / qb: those
    // registers must not be handed to anything else before it has landed (see k_inv_pair_ps).
    asm_wait_vmcnt<0>(qa, qb);
    if (bad != 0x7fffffff) flag_bad(a, bad);
    unsigned int mx[4];                                                  // non-negative floats order like their bits
#pragma unroll
    for (int c = 0; c < 4; c++) mx[c] = __float_as_uint(pk[c]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const unsigned int m = __shfl_xor(mx[c], o);
            mx[c] = m > mx[c] ? m : mx[c];
            cn[c] += __shfl_xor(cn[c], o);
        }
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 4; c++) { red_max[tid >> 6][c] = mx[c]; red_cnt[tid >> 6][c] = cn[c]; }
    }
    __syncthreads();
    if (tid < 4) {
        unsigned int m = 0u, n = 0u;
        for (int wv = 0; wv < (NT + 63) / 64; wv++) { m = red_max[wv][tid] > m ? red_max[wv][tid] : m; n += red_cnt[wv][tid]; }
        DevOverflow *of = of_shard(a.overflow, a.of_shard_stride) + (gc + tid);
        if (n) atomicAdd(&of->n_overflows, n);
        // filtered: the peak only ever grows, a stale read costs an extra atomic, never a wrong result
        if ((unsigned long long)m > *(volatile unsigned long long *)&of->largest_bits)
            atomicMax(&of->largest_bits, (unsigned long long)m);
    }
}

}  // namespace

// N = 2048 and 4096 stay on the pair kernel: their last pass is a radix-8 / radix-16 one (more base twiddles in registers,
// wider butterflies under the prefetch) and the compiler's report shows scratch at the pair kernel's waves per SIMD (96
// and 104 bytes per lane) -- a spill is a vector-memory operation inside the counted windows (tests/test_quad_isa.py
// holds the others to none).  N = 1024 stays there too: no scratch at four waves (123 registers), but its pair kernel reaches
// five (89), and compiled for five this kernel spills 77 registers (80 with the prefetch behind the last pass; with A's
// half in LDS the LDS bounds it to three).
#define BFIR_FOR_QUAD_LOG2N(F) F(13) F(14)

static std::atomic<int64_t> g_quad_launches{0};            // bfir_inv_quad_launches, below

// Blocks per workgroup (two transforms each): 2, the pair kernel's four transforms.  With 4 the kernel alone is faster
// (0.371 against 0.378 ms per 4096 blocks) and the pipeline slower (profiles/quad_io.txt), as pair_run_len found for the
// pair kernels.  BFIR_QUAD_RUN_INV overrides (tuning aid).
static int quad_run_len(int n_t, int units)
{
    if (const char *e = getenv("BFIR_QUAD_RUN_INV")) return std::max(1, atoi(e));
    const int slots = 512;                                 // 256 CUs x 2 workgroups
    const int runs = std::max(1, slots / std::max(1, units));
    const int fill = std::max(1, (n_t + runs - 1) / runs); // what one round of workgroups would need
    return std::min(fill, 2);
}

// Takes the launch where the frames can be written in 16-byte pieces; false: the caller's pair kernel does it.
bool launch_inv_quad(const FftPlan &plan, const InvPairArgs &a, hipStream_t s)
{
    if (a.tp || a.quad == 0 || a.C <= 0 || a.C % 4 != 0 || (a.frame_stride != 0 && a.frame_stride != a.C)) return false;
    if ((((uintptr_t)a.raw) & 15u) != 0 || (a.eng_stride & 3) != 0) return false;   // every piece 16-byte aligned
    const int units = a.n_eng * (a.C / 4);
    if (a.n_t <= 0 || units <= 0 || !plan.twb) return false;
    // Two transforms in turn per workgroup: by default only where the launch fills the GPU anyway, so that a
    // call of a few blocks (the latency path) keeps one transform per workgroup.  BFIR_INV_QUAD=1 lifts that.
    if (a.quad < 0 && (long)a.n_t * units < 512) return false;
    const int len = quad_run_len(a.n_t, units), runs = (a.n_t + len - 1) / len;
    switch (plan.log2m) {
#define F(lg) case lg: hipLaunchKernelGGL((k_inv_quad_ps<lg>), dim3(runs * units), dim3(FftCfg<lg>::NT), 0, s, a, (const float2 *)plan.twb, len); break;
        BFIR_FOR_QUAD_LOG2N(F)
#undef F
        default: return false;
    }
    g_quad_launches.fetch_add(1, std::memory_order_relaxed);
    return true;
}

}  // namespace bfir

// Launches of k_inv_quad_ps in this process.  For tests/test_quad_path_gpu.py, not part of the public interface: which
// kernel took a launch cannot be seen from the output, whose bits are those of the pair kernel.
extern "C" int64_t bfir_inv_quad_launches(void) { return bfir::g_quad_launches.load(std::memory_order_relaxed); }
