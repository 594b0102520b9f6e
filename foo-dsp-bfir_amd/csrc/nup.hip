// nup.hip -- the back end of a two-level ("non-uniformly partitioned") engine (bfir_engine_create_nup, engine.hip).
//
// The head level (partitions of L) has left its product spectra in Y; the tail level (partitions of Lt = r L) has left its
// time output z in a planar ring [n_ch][zlen] of working precision, sample m of z at m mod zlen.  Sample n of head block t
// of the chunk is
//   y_head[n] + z[m],   m = m0 + t L + n   (m0 = first sample of the chunk - D; nothing is added where m < m_min)
// one addition in working precision, head first; format conversion, overflow statistics and the NaN guard act on the sum.
//
//   k_inv_nup      fp32, (re, im) pairs, FLOAT_LE frames, even channel count, 512 <= L <= 8192: the channel-pair form of
//                  the shared fused back end (inv_back.h) with one ring, 8-byte stores (both channels of a frame).
//   k_nup_combine  everything else: launch_inv has written y_head as a planar time buffer; this adds z to it in place and
//                  launch_stage_out converts, counts and guards as for a plain chunk of the staging path.
#include "kernels.h"

#include "inv_back.h"

namespace bfir {

namespace {

template <int LOG2N>
__global__ __launch_bounds__(FftCfg<LOG2N>::NT) void k_inv_nup(LevelsInvArgs a, const float2 *__restrict__ tw)
{
    inv_back_pair_rings<LOG2N, 1>(a, tw);
}

// lane-consecutive, VEC samples (16 bytes) per lane; VEC = 1 where a channel's samples are not 16-byte aligned.  m0, m_min
// and zlen are multiples of L >= 16, so a lane's VEC samples are all inside or all outside z and never straddle the wrap.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void k_nup_combine(LevelsCombineArgs a)
{
    struct __attribute__((aligned(sizeof(T) * VEC))) V { T v[VEC]; };
    const LevelRing &g = a.ring[0];
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (i >= a.n || g.m0 + i < g.m_min) return;
    long zi = g.m0r + i;
    zi = zi >= g.zlen ? zi - g.zlen : zi;
    V *__restrict__ py = (V *)((T *)a.y + (long)blockIdx.y * a.y_ch_stride + i);
    const V *__restrict__ pz = (const V *)((const T *)g.z + (long)blockIdx.y * g.z_ch_stride + zi);
    V y = *py;
    const V z = *pz;
#pragma unroll
    for (int j = 0; j < VEC; j++) y.v[j] = y.v[j] + z.v[j];
    *py = y;
}

}  // namespace

#define BFIR_FOR_NUP_LOG2N(F) F(10) F(11) F(12) F(13) F(14)

void launch_inv_nup(const FftPlan &plan, const LevelsInvArgs &a, hipStream_t s)
{
    const int items = a.n_t * (a.n_ch / 2);
    if (items <= 0 || !plan.tw || a.n_rings != 1) return;
    switch (plan.log2m) {
#define F(lg) case lg: hipLaunchKernelGGL((k_inv_nup<lg>), dim3(items), dim3(FftCfg<lg>::NT), 0, s, a, (const float2 *)plan.tw); break;
        BFIR_FOR_NUP_LOG2N(F)
#undef F
    }
}

void launch_nup_combine(const LevelsCombineArgs &a, hipStream_t s)
{
    if (a.n <= 0 || a.n_ch <= 0 || a.n_rings != 1) return;
    const int vec = 16 / a.realsize;
    const bool aligned = a.n % vec == 0 && a.y_ch_stride % vec == 0 && (uintptr_t)a.y % 16 == 0 && rings_aligned16(a.ring, nullptr, 1, vec);
    launch_planar(BFIR_PLANAR_KERNELS(k_nup_combine), a, aligned, s);
}

}  // namespace bfir
