// mlevels.hip -- the last output of a multi-level MATRIX engine (bfir_engine_create_matrix_levels, engine.hip) whose output
// count is odd, on the fused back end.
//
// Such an engine sends its output pairs (0, 1), (2, 3), ... through k_inv_nup / k_inv_levels (nup.hip, levels.hip) with
// n_ch = 2 floor(n_out / 2) and the frame stride n_out; the one output left over has no partner for their two-for-one
// transform and comes here.  The head level has left its product spectrum in y; every contributing tail level its time
// output in a planar ring (LevelRing, kernels.h).  Sample n of head block t of the chunk is
//   ((y_head[n] + z_0[m_0]) + z_1[m_1]) + z_2[m_2],   m_r = ring[r].m0 + t L + n   (nothing from ring r where m_r < m_min)
// as in levels.hip: the additions in fp32, head first, rings in level order; overflow statistics and the NaN guard of
// real2raw (brutefir/real2raw.cpp:321-336, brutefir.cpp:316-321) act on the sum.
//
//   k_inv_lone<LOG2N, NR>   fp32, (re, im) pairs, FLOAT_LE frames, 512 <= L <= 8192, NR = 0 .. 3 rings.  One workgroup is
//                           one block of the one channel: Z = Y + i 0, Hermitian-extended, through the complex plan of
//                           N = 2L points the pair kernels use (the partner is zero, the imaginary half of the result is
//                           dropped), NR ring additions, statistics, NaN guard, one 4-byte store per frame.
#include "kernels.h"

#include "fft_lds.h"

namespace bfir {

namespace {

template <int LOG2N, int NR>
__global__ __launch_bounds__(FftCfg<LOG2N>::NT) void k_inv_lone(LoneInvArgs a, const float2 *__restrict__ tw)
{
    using F = LdsFft<float, LOG2N, +1>;
    constexpr int N = F::M, NT = F::NT, P = F::P, L = N / 2, Q = P / 4;   // Q 16-byte pieces per thread
    constexpr int NW = NT / 64 > 0 ? NT / 64 : 1;
    static_assert(L <= F::LDS_ELEMS, "the spectrum (L pairs) is staged in the transform's buffer");
    static_assert(NR >= 0 && NR <= BFIR_LEVEL_RINGS, "no ring (a chunk to which no level contributes) to three");
    constexpr int NRA = NR > 0 ? NR : 1;
    __shared__ __attribute__((aligned(16))) float2 lds[F::LDS_ELEMS];
    __shared__ unsigned int red_max[NW], red_cnt[NW];

    const int tid = threadIdx.x;
    const int t = xcd_work_item(blockIdx.x, gridDim.x);
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const f32x4 *__restrict__ ya = (const f32x4 *)(a.y + (long)t * N);

    // the spectrum into LDS at [0, L) (float2 units); it is read once: nontemporal
    {
        f32x4 *l4 = (f32x4 *)lds;
#pragma unroll
        for (int j = 0; j < Q; j++) l4[tid + j * NT] = __builtin_nontemporal_load(ya + tid + j * NT);
    }
    __syncthreads();
    // Z[k] = Y[k], Hermitian-extended to the full circle; bin 0 carries DC | Nyquist
    float re[P], im[P];
    static_for<0, P>([&](auto E_) {
        constexpr int e = decltype(E_)::value;
        constexpr int base = F::in_index(0, e);
        static_assert(base + NT <= L || base >= L, "a thread's points do not straddle L");
        const int k = base + tid;
        const int kk = (base < L) ? k : N - k;                           // kk == L only for base == L, tid == 0
        const bool edge = (base == 0 || base == L) && tid == 0;
        const float2 pa = lds[edge ? 0 : kk];
        float zr = pa.x, zi = (base < L) ? pa.y : -pa.y;                  // the upper half: conj Y
        if (base == 0) zi = edge ? 0.f : zi;                              // DC
        if (base == L) { zr = edge ? pa.y : zr; zi = edge ? 0.f : zi; }   // Nyquist
        re[e] = zr * a.scale; im[e] = zi * a.scale;
    });
    pin_registers(re, im);   // every read of the staged spectrum happens before run()'s first barrier

    F::run(re, im, lds, tw, tid);

    // first L samples are the valid half, Re z the channel.  The block's L samples of a ring are contiguous (zlen, m0 and
    // m_min are multiples of L): a ring wraps between blocks only, and a block has all of a ring's samples or none.  A ring
    // without samples for this block is read at its start and its samples dropped.
    float *__restrict__ out = a.raw + (a.frame_off + (long)t * L) * a.frame_stride + a.ch;
    const float *__restrict__ za[NRA];
    bool has_z[NRA];
#pragma unroll
    for (int r = 0; r < NR; r++) {
        const LevelRing &g = a.ring[r];
        has_z[r] = g.m0 + (long long)t * L >= g.m_min;
        long zi0 = g.m0r + (long)t * L;
        zi0 = zi0 >= g.zlen ? zi0 - g.zlen : zi0;
        za[r] = (const float *)g.z + (long)a.ch * g.z_ch_stride + (has_z[r] ? zi0 : 0);
    }
    const float rmax = a.max;
    float pk = 0.f;
    unsigned int cnt = 0u;
#pragma unroll
    for (int e = 0; e < P; e++) {
        if (F::out_index(0, e) < L) {                                    // compile time: out_index(tid, e) = tid + const, tid < NT <= L
            const int n = F::out_index(tid, e);
            float v = re[e];
#pragma unroll
            for (int r = 0; r < NR; r++) {                               // level order: ((y + z_0) + z_1) + z_2
                const float z = za[r][n];
                v = has_z[r] ? v + z : v;
            }
            out[(long)n * a.frame_stride] = v;
            // real2raw.cpp:321-336 with symmetric limits: |v| > max, NaN never counts (k_inv_pair_ps)
            cnt += (fabsf(v) > rmax) ? 1u : 0u;
            pk = fmaxf(pk, fabsf(v));
            // brutefir.cpp:316-321: only sample 0 of each block is checked
            if (F::out_index(0, e) == 0) {
                if (n == 0 && !isfinite(v)) flag_bad(a, t);
            }
        }
    }
    unsigned int mx = __float_as_uint(pk);                               // non-negative floats order like their bits
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned int m2 = __shfl_xor(mx, o);
        mx = m2 > mx ? m2 : mx;
        cnt += __shfl_xor(cnt, o);
    }
    if ((tid & 63) == 0) { red_max[tid >> 6] = mx; red_cnt[tid >> 6] = cnt; }
    __syncthreads();
    if (tid == 0) {
        unsigned int m2 = 0u, n2 = 0u;
        for (int wv = 0; wv < NW; wv++) { m2 = red_max[wv] > m2 ? red_max[wv] : m2; n2 += red_cnt[wv]; }
        DevOverflow *of = of_shard(a.overflow, a.of_shard_stride) + a.ch;
        if (n2) atomicAdd(&of->n_overflows, n2);
        // filtered: the peak only ever grows, a stale read costs an extra atomic, never a wrong result
        if ((unsigned long long)m2 > *(volatile unsigned long long *)&of->largest_bits)
            atomicMax(&of->largest_bits, (unsigned long long)m2);
    }
}

}  // namespace

#define BFIR_FOR_LONE_LOG2N(F) F(10) F(11) F(12) F(13) F(14)

void launch_inv_lone(const FftPlan &plan, const LoneInvArgs &a, hipStream_t s)
{
    if (a.n_t <= 0 || !plan.tw || a.n_rings < 0 || a.n_rings > BFIR_LEVEL_RINGS) return;
    const dim3 grid(a.n_t);
    switch (plan.log2m) {
#define F(lg)                                                                                                                   \
    case lg:                                                                                                                    \
        if (a.n_rings == 0) hipLaunchKernelGGL((k_inv_lone<lg, 0>), grid, dim3(FftCfg<lg>::NT), 0, s, a, (const float2 *)plan.tw);      \
        else if (a.n_rings == 1) hipLaunchKernelGGL((k_inv_lone<lg, 1>), grid, dim3(FftCfg<lg>::NT), 0, s, a, (const float2 *)plan.tw);      \
        else if (a.n_rings == 2) hipLaunchKernelGGL((k_inv_lone<lg, 2>), grid, dim3(FftCfg<lg>::NT), 0, s, a, (const float2 *)plan.tw); \
        else hipLaunchKernelGGL((k_inv_lone<lg, 3>), grid, dim3(FftCfg<lg>::NT), 0, s, a, (const float2 *)plan.tw);             \
        break;
        BFIR_FOR_LONE_LOG2N(F)
#undef F
    }
}

}  // namespace bfir
