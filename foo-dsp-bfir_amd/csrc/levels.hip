// levels.hip -- the back end of a multi-level engine (bfir_engine_create_levels, engine.hip) for a chunk to which two or
// three tail levels contribute; with one contributing level the engine takes the two-level kernels of nup.hip.
//
// The head level (partitions of L) has left its product spectra in Y; every contributing tail level its time output in a
// planar ring [n_ch][zlen] of working precision, sample m at m mod zlen (LevelRing, kernels.h).  Sample n of head block t
// of the chunk is
//   ((y_head[n] + z_0[m_0]) + z_1[m_1]) + z_2[m_2],   m_r = ring[r].m0 + t L + n   (nothing from ring r where m_r < m_min)
// the additions in working precision, head first, rings in level order; format conversion, overflow statistics and the
// NaN guard act on the sum.
//
//   k_inv_levels      fp32, (re, im) pairs, FLOAT_LE frames, even channel count, 512 <= L <= 8192: k_inv_nup with NR = 2 or
//                     3 rings, the channel-pair form of the shared fused back end (inv_back.h).
//   k_levels_combine  everything else: launch_inv has written y_head as a planar time buffer; this adds the rings to it in
//                     place, in one pass, and launch_stage_out converts, counts and guards as for a plain chunk.
#include "kernels.h"

#include "inv_back.h"

namespace bfir {

namespace {

template <int LOG2N, int NR>
__global__ __launch_bounds__(FftCfg<LOG2N>::NT) void k_inv_levels(LevelsInvArgs a, const float2 *__restrict__ tw)
{
    static_assert(NR >= 2 && NR <= BFIR_LEVEL_RINGS, "one ring is k_inv_nup's");
    inv_back_pair_rings<LOG2N, NR>(a, tw);
}

// lane-consecutive, VEC samples (16 bytes) per lane; VEC = 1 where a channel's samples are not 16-byte aligned.  Every m0,
// m_min and zlen is a multiple of L >= 16, so a lane's VEC samples are all inside or all outside a ring and never
// straddle its wrap.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void k_levels_combine(LevelsCombineArgs a)
{
    struct __attribute__((aligned(sizeof(T) * VEC))) V { T v[VEC]; };
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (i >= a.n) return;
    V *__restrict__ py = (V *)((T *)a.y + (long)blockIdx.y * a.y_ch_stride + i);
    V y = *py;
#pragma unroll
    for (int r = 0; r < BFIR_LEVEL_RINGS; r++) {
        const LevelRing &g = a.ring[r];
        if (r < a.n_rings && g.m0 + i >= g.m_min) {
            long zi = g.m0r + i;
            zi = zi >= g.zlen ? zi - g.zlen : zi;
            const V z = *(const V *)((const T *)g.z + (long)blockIdx.y * g.z_ch_stride + zi);
#pragma unroll
            for (int j = 0; j < VEC; j++) y.v[j] = y.v[j] + z.v[j];
        }
    }
    *py = y;
}

}  // namespace

#define BFIR_FOR_LEVELS_LOG2N(F) F(10) F(11) F(12) F(13) F(14)

void launch_inv_levels(const FftPlan &plan, const LevelsInvArgs &a, hipStream_t s)
{
    const int items = a.n_t * (a.n_ch / 2);
    if (a.n_rings == 1) return launch_inv_nup(plan, a, s);
    if (items <= 0 || !plan.tw || a.n_rings < 2 || a.n_rings > BFIR_LEVEL_RINGS) return;
    switch (plan.log2m) {
#define F(lg)                                                                                                                   \
    case lg:                                                                                                                    \
        if (a.n_rings == 2) hipLaunchKernelGGL((k_inv_levels<lg, 2>), dim3(items), dim3(FftCfg<lg>::NT), 0, s, a, (const float2 *)plan.tw); \
        else hipLaunchKernelGGL((k_inv_levels<lg, 3>), dim3(items), dim3(FftCfg<lg>::NT), 0, s, a, (const float2 *)plan.tw);   \
        break;
        BFIR_FOR_LEVELS_LOG2N(F)
#undef F
    }
}

void launch_levels_combine(const LevelsCombineArgs &a, hipStream_t s)
{
    if (a.n_rings == 1) return launch_nup_combine(a, s);   // no runtime ring loop
    if (a.n <= 0 || a.n_ch <= 0 || a.n_rings < 2 || a.n_rings > BFIR_LEVEL_RINGS) return;
    const int vec = 16 / a.realsize;
    const bool aligned = a.n % vec == 0 && a.y_ch_stride % vec == 0 && (uintptr_t)a.y % 16 == 0 && rings_aligned16(a.ring, nullptr, a.n_rings, vec);
    launch_planar(BFIR_PLANAR_KERNELS(k_levels_combine), a, aligned, s);
}

}  // namespace bfir
