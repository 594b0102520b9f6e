// lfade.hip -- the back end of a crossfaded coefficient change on a two-level or multi-level engine
// (bfir_engine_set_coeff_nup_fade / _levels_fade, engine.hip) for a head chunk to which one, two or three tail levels
// contribute; a fading chunk without a contributing level takes the kernels of fade.hip.
//
// The head's MAC has run twice on its delay line (old filters -> Y_old, new filters -> Y_new), and every contributing tail
// level keeps TWO time rings of one geometry (LevelRing, kernels.h): its output under the old set and under the new one.
// Sample n of head block t of the chunk is
//   fade_blend(S_old, S_new, f, m),   S_x = ((y_head,x[n] + z_0,x[m_0]) + z_1,x[m_1]) + z_2,x[m_2],   m = m0 + t L + n
// the sums in working precision, head first, rings in level order, as levels.hip defines them; the blend is the one of
// fftw_convolver::convolver_crossfade_inplace (brutefir/fftw_convolver.cpp:275-321; fade_blend.h); format conversion,
// overflow statistics and the NaN guard act on the blended sample.
//
//   k_inv_lfade  fp32, (re, im) pairs, FLOAT_LE frames, 512 <= L <= 8192, any channel count.  k_inv_fade with NR = 1, 2 or
//                3 rings per set: one workgroup is one (channel, block) of the shared fused back end (inv_back.h),
//                Z = Y_old + i Y_new, the old rings added to the real part and the new rings to the imaginary part, the
//                blend, 4-byte stores at the frame stride.
//   k_lfade_sum  everything else: launch_inv has written y_old and y_new as planar time buffers; this adds each set's
//                rings and blends into y_old in place, in one pass, and launch_stage_out converts, counts and guards as
//                for a plain chunk of the staging path.
#include "kernels.h"

#include "fade_blend.h"
#include "inv_back.h"

namespace bfir {

namespace {

template <int LOG2N, int NR>
__global__ __launch_bounds__(FftCfg<LOG2N>::NT) void k_inv_lfade(LfadeInvArgs a, const float2 *__restrict__ tw)
{
    constexpr int N = 1 << LOG2N, L = N / 2;
    static_assert(NR >= 1 && NR <= BFIR_LEVEL_RINGS, "no ring is k_inv_fade's");
    // the channels of a block store into the same cache lines of the output frames: one XCD
    const int w = xcd_work_item(blockIdx.x, gridDim.x);
    const int t = w / a.n_ch, gc = w - t * a.n_ch;
    const int C = a.n_ch;
    float *__restrict__ out = a.raw + (a.frame_off + (long)t * L) * C + gc;
    // the two rings of a level share their geometry
    const BlockRings<NR> br = block_rings<NR, L>(a.ring, t, gc);
    const float *__restrict__ zo[NR], *__restrict__ zn[NR];
#pragma unroll
    for (int r = 0; r < NR; r++) { zo[r] = (const float *)a.ring[r].z + br.at[r]; zn[r] = (const float *)a.z_new[r] + br.at[r]; }
    const int m_blk = a.m0 + t * L;
    const float f = a.f;
    // Re z = y_old, Im z = y_new
    inv_back_block<LOG2N, true, 1>(a.y_old + (long)gc * a.y_old_ch_stride + (long)t * N, a.y_new + (long)gc * a.y_new_ch_stride + (long)t * N,
                                   a.scale, tw, a.st, t, gc, [&] {
        return [=](int n, float re, float im, float (&v)[1]) {
            float so = re, sn = im;
#pragma unroll
            for (int r = 0; r < NR; r++) {                           // level order: ((y + z_0) + z_1) + z_2, per set
                so = ring_add(so, zo[r][n], br.keep[r]);
                sn = ring_add(sn, zn[r][n], br.keep[r]);
            }
            v[0] = fade_blend(so, sn, f, m_blk + n);
            out[(long)n * C] = v[0];
        };
    });
}

// lane-consecutive, VEC samples (16 bytes) per lane; VEC = 1 where a channel's samples are not 16-byte aligned.  Every m0,
// m_min and zlen is a multiple of L >= 16, so a lane's VEC samples are all inside or all outside a ring and never
// straddle its wrap (k_levels_combine).
template <typename T, int VEC>
__global__ __launch_bounds__(256) void k_lfade_sum(LfadeSumArgs a)
{
    struct __attribute__((aligned(sizeof(T) * VEC))) V { T v[VEC]; };
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (i >= a.n) return;
    const long at = (long)blockIdx.y * a.ch_stride + i;
    V *__restrict__ po = (V *)((T *)a.y_old + at);
    V o = *po;
    V nw = *(const V *)((const T *)a.y_new + at);
#pragma unroll
    for (int r = 0; r < BFIR_LEVEL_RINGS; r++) {
        const LevelRing &g = a.ring[r];
        if (r < a.n_rings && g.m0 + i >= g.m_min) {
            long zi = g.m0r + i;
            zi = zi >= g.zlen ? zi - g.zlen : zi;
            const long zat = (long)blockIdx.y * g.z_ch_stride + zi;
            const V z0 = *(const V *)((const T *)g.z + zat), z1 = *(const V *)((const T *)a.z_new[r] + zat);
#pragma unroll
            for (int j = 0; j < VEC; j++) { o.v[j] = o.v[j] + z0.v[j]; nw.v[j] = nw.v[j] + z1.v[j]; }
        }
    }
    const T f = (T)a.f;
#pragma unroll
    for (int j = 0; j < VEC; j++) o.v[j] = fade_blend(o.v[j], nw.v[j], f, a.m0 + (int)i + j);
    *po = o;
}

}  // namespace

#define BFIR_FOR_LFADE_LOG2N(F) F(10) F(11) F(12) F(13) F(14)

void launch_inv_lfade(const FftPlan &plan, const LfadeInvArgs &a, hipStream_t s)
{
    const int items = a.n_t * a.n_ch;
    if (items <= 0 || !plan.tw || a.n_rings < 1 || a.n_rings > BFIR_LEVEL_RINGS) return;
    const dim3 grid(items);
    switch (plan.log2m) {
#define F(lg)                                                                                                                   \
    case lg:                                                                                                                    \
        if (a.n_rings == 1) hipLaunchKernelGGL((k_inv_lfade<lg, 1>), grid, dim3(FftCfg<lg>::NT), 0, s, a, (const float2 *)plan.tw);      \
        else if (a.n_rings == 2) hipLaunchKernelGGL((k_inv_lfade<lg, 2>), grid, dim3(FftCfg<lg>::NT), 0, s, a, (const float2 *)plan.tw); \
        else hipLaunchKernelGGL((k_inv_lfade<lg, 3>), grid, dim3(FftCfg<lg>::NT), 0, s, a, (const float2 *)plan.tw);                     \
        break;
        BFIR_FOR_LFADE_LOG2N(F)
#undef F
    }
}

void launch_lfade_sum(const LfadeSumArgs &a, hipStream_t s)
{
    if (a.n <= 0 || a.n_ch <= 0 || a.n_rings < 1 || a.n_rings > BFIR_LEVEL_RINGS) return;
    const int vec = 16 / a.realsize;
    // the rule of launch_levels_combine, over both sets of rings
    const bool aligned = a.n % vec == 0 && a.ch_stride % vec == 0 && ((uintptr_t)a.y_old | (uintptr_t)a.y_new) % 16 == 0 &&
                         rings_aligned16(a.ring, a.z_new, a.n_rings, vec);
    launch_planar(BFIR_PLANAR_KERNELS(k_lfade_sum), a, aligned, s);
}

}  // namespace bfir
