// fade.hip -- the back end of a crossfaded coefficient change (bfir_engine_set_coeff_fade, engine.hip).
//
// fftw_convolver::convolver_crossfade_inplace (brutefir/fftw_convolver.cpp:275-321) convolves one block with two filter
// sets and blends the two time signals with a linear ramp (:296-315).  The engine does the same over K blocks: the MAC
// runs twice on the one delay line (old filters -> Y_old, new filters -> Y_new), and what follows is here.
//
//   k_inv_fade    fp32, (re, im) pairs, FLOAT_LE frames, 512 <= L <= 8192.  The two-for-one identity pair.hip uses for two
//                 CHANNELS serves the two filter SETS of one channel: Z = Y_old + i Y_new, Hermitian-extended, is the
//                 spectrum of y_old + i y_new, so ONE complex inverse of N = 2L points yields both time signals.  One
//                 workgroup is one (output channel, block) of the shared fused back end (inv_back.h); its samples are
//                 the blend, 4-byte stores at the frame stride.
//   k_fade_blend  everything else: launch_inv has written y_old and y_new as planar time buffers; this blends them in place
//                 and launch_stage_out converts, counts and guards as for a plain chunk of the staging path.
#include "kernels.h"

#include "fade_blend.h"
#include "inv_back.h"

namespace bfir {

namespace {

template <int LOG2N>
__global__ __launch_bounds__(FftCfg<LOG2N>::NT) void k_inv_fade(FadeInvArgs a, const float2 *__restrict__ tw)
{
    constexpr int N = 1 << LOG2N, L = N / 2;
    // the channels of a block store into the same cache lines of the output frames: one XCD
    const int w = xcd_work_item(blockIdx.x, gridDim.x);
    const int t = w / a.n_ch, gc = w - t * a.n_ch;
    // Re z = y_old, Im z = y_new
    inv_back_block<LOG2N, true, 1>(a.y_old + (long)gc * a.y_old_ch_stride + (long)t * N, a.y_new + (long)gc * a.y_new_ch_stride + (long)t * N,
                                   a.scale, tw, a.st, t, gc, [&] {
        const int C = a.n_ch;
        float *__restrict__ out = a.raw + (a.frame_off + (long)t * L) * C + gc;
        const int m_blk = a.m0 + t * L;
        const float f = a.f;
        return [=](int n, float re, float im, float (&v)[1]) {
            v[0] = fade_blend(re, im, f, m_blk + n);
            out[(long)n * C] = v[0];
        };
    });
}

// lane-consecutive, VEC samples (16 bytes) per lane; VEC = 1 where a channel's samples are not 16-byte aligned
template <typename T, int VEC>
__global__ __launch_bounds__(256) void k_fade_blend(FadeBlendArgs a)
{
    struct __attribute__((aligned(sizeof(T) * VEC))) V { T v[VEC]; };
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (i >= a.n) return;
    const long at = (long)blockIdx.y * a.ch_stride + i;
    V *__restrict__ po = (V *)((T *)a.y_old + at);
    const V *__restrict__ pn = (const V *)((const T *)a.y_new + at);
    V o = *po;
    const V nw = *pn;
    const T f = (T)a.f;
#pragma unroll
    for (int j = 0; j < VEC; j++) o.v[j] = fade_blend(o.v[j], nw.v[j], f, a.m0 + (int)i + j);
    *po = o;
}

}  // namespace

#define BFIR_FOR_FADE_LOG2N(F) F(10) F(11) F(12) F(13) F(14)

void launch_inv_fade(const FftPlan &plan, const FadeInvArgs &a, hipStream_t s)
{
    const int items = a.n_t * a.n_ch;
    if (items <= 0 || !plan.tw) return;
    switch (plan.log2m) {
#define F(lg) case lg: hipLaunchKernelGGL((k_inv_fade<lg>), dim3(items), dim3(FftCfg<lg>::NT), 0, s, a, (const float2 *)plan.tw); break;
        BFIR_FOR_FADE_LOG2N(F)
#undef F
    }
}

void launch_fade_blend(const FadeBlendArgs &a, hipStream_t s)
{
    if (a.n <= 0 || a.n_ch <= 0) return;
    const int vec = 16 / a.realsize;
    const bool aligned = a.n % vec == 0 && a.ch_stride % vec == 0 && ((uintptr_t)a.y_old | (uintptr_t)a.y_new) % 16 == 0;
    launch_planar(BFIR_PLANAR_KERNELS(k_fade_blend), a, aligned, s);
}

}  // namespace bfir
