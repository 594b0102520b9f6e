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
//                           one block of the one channel: the one-spectrum form of the shared fused back end (inv_back.h),
//                           Z = Y + i 0 through the complex plan of N = 2L points the pair kernels use (the partner is
//                           zero, the imaginary half of the result is dropped), one 4-byte store per frame.
#include "kernels.h"

#include "inv_back.h"

namespace bfir {

namespace {

template <int LOG2N, int NR>
__global__ __launch_bounds__(FftCfg<LOG2N>::NT) void k_inv_lone(LoneInvArgs a, const float2 *__restrict__ tw)
{
    constexpr int N = 1 << LOG2N, L = N / 2, NRA = NR > 0 ? NR : 1;
    const int t = xcd_work_item(blockIdx.x, gridDim.x);
    const int C = a.frame_stride;
    float *__restrict__ out = a.raw + (a.frame_off + (long)t * L) * C + a.ch;
    const BlockRings<NR> br = block_rings<NR, L>(a.ring, t, a.ch);
    const float *__restrict__ za[NRA] = {};
#pragma unroll
    for (int r = 0; r < NR; r++) za[r] = (const float *)a.ring[r].z + br.at[r];
    // Re z the channel; the partner is zero
    inv_back_block<LOG2N, false, 1>(a.y + (long)t * N, nullptr, a.scale, tw, a.st, t, a.ch, [&] {
        return [=](int n, float re, float, float (&v)[1]) {
            v[0] = re;
#pragma unroll
            for (int r = 0; r < NR; r++) v[0] = ring_add(v[0], za[r][n], br.keep[r]);   // level order: ((y + z_0) + z_1) + z_2
            out[(long)n * C] = v[0];
        };
    });
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
