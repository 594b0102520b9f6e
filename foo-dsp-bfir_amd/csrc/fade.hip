// fade.hip -- the back end of a crossfaded coefficient change (bfir_engine_set_coeff_fade, engine.hip).
//
// fftw_convolver::convolver_crossfade_inplace (brutefir/fftw_convolver.cpp:275-321) convolves one block with two filter
// sets and blends the two time signals with a linear ramp (:296-315).  The engine does the same over K blocks: the MAC
// runs twice on the one delay line (old filters -> Y_old, new filters -> Y_new), and what follows is here.
//
//   k_inv_fade    fp32, (re, im) pairs, FLOAT_LE frames, 512 <= L <= 8192.  The two-for-one identity pair.hip uses for two
//                 CHANNELS serves the two filter SETS of one channel: Z = Y_old + i Y_new, Hermitian-extended, is the
//                 spectrum of y_old + i y_new, so ONE complex inverse of N = 2L points yields both time signals.  One
//                 workgroup is one (output channel, block): load, transform, blend, overflow statistics and NaN guard of
//                 real2raw (brutefir/real2raw.cpp:321-336, brutefir.cpp:316-321), 4-byte stores at the frame stride.
//   k_fade_blend  everything else: launch_inv has written y_old and y_new as planar time buffers; this blends them in place
//                 and launch_stage_out converts, counts and guards as for a plain chunk of the staging path.
#include "kernels.h"

#include "fade_blend.h"
#include "fft_lds.h"

namespace bfir {

namespace {

template <int LOG2N>
__global__ __launch_bounds__(FftCfg<LOG2N>::NT) void k_inv_fade(FadeInvArgs a, const float2 *__restrict__ tw)
{
    using F = LdsFft<float, LOG2N, +1>;
    constexpr int N = F::M, NT = F::NT, P = F::P, L = N / 2, Q = P / 4;   // Q 16-byte pieces per thread and spectrum
    constexpr int NW = NT / 64 > 0 ? NT / 64 : 1;
    static_assert(N <= F::LDS_ELEMS, "both spectra (2 x L pairs) are staged in the transform's buffer");
    __shared__ __attribute__((aligned(16))) float2 lds[F::LDS_ELEMS];
    __shared__ unsigned int red_max[NW], red_cnt[NW];

    const int tid = threadIdx.x;
    // the channels of a block store into the same cache lines of the output frames: one XCD
    const int w = xcd_work_item(blockIdx.x, gridDim.x);
    const int t = w / a.n_ch, gc = w - t * a.n_ch;
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const f32x4 *__restrict__ ya = (const f32x4 *)(a.y_old + (long)gc * a.y_old_ch_stride + (long)t * N);
    const f32x4 *__restrict__ yb = (const f32x4 *)(a.y_new + (long)gc * a.y_new_ch_stride + (long)t * N);

    // both spectra into LDS: Y_old at [0, L), Y_new at [L, 2L)  (float2 units); each is read once: nontemporal
    {
        f32x4 *l4 = (f32x4 *)lds;
#pragma unroll
        for (int j = 0; j < Q; j++) {
            l4[tid + j * NT] = __builtin_nontemporal_load(ya + tid + j * NT);
            l4[L / 2 + tid + j * NT] = __builtin_nontemporal_load(yb + tid + j * NT);
        }
    }
    __syncthreads();
    // Z[k] = Y_old[k] + i Y_new[k], Hermitian-extended to the full circle (k_inv_pair_ps); bin 0 carries DC | Nyquist
    float re[P], im[P];
    static_for<0, P>([&](auto E_) {
        constexpr int e = decltype(E_)::value;
        constexpr int base = F::in_index(0, e);
        static_assert(base + NT <= L || base >= L, "a thread's points do not straddle L");
        const int k = base + tid;
        const int kk = (base < L) ? k : N - k;                           // kk == L only for base == L, tid == 0
        const bool edge = (base == 0 || base == L) && tid == 0;
        const float2 pa = lds[edge ? 0 : kk], pb = lds[L + (edge ? 0 : kk)];
        float zr, zi;
        if (base < L) { zr = pa.x - pb.y; zi = pa.y + pb.x; }
        else          { zr = pa.x + pb.y; zi = pb.x - pa.y; }             // conj Y_old + i conj Y_new
        if (base == 0) { zr = edge ? pa.x : zr; zi = edge ? pb.x : zi; }   // DC of both
        if (base == L) { zr = edge ? pa.y : zr; zi = edge ? pb.y : zi; }   // Nyquist of both
        re[e] = zr * a.scale; im[e] = zi * a.scale;
    });
    pin_registers(re, im);   // every read of the staged spectra happens before run()'s first barrier

    F::run(re, im, lds, tw, tid);

    // first L samples are the valid half: Re z = y_old, Im z = y_new
    const int C = a.n_ch;
    float *__restrict__ out = a.raw + (a.frame_off + (long)t * L) * C + gc;
    const int m_blk = a.m0 + t * L;
    const float rmax = a.max;
    float pk = 0.f;
    unsigned int cnt = 0u;
#pragma unroll
    for (int e = 0; e < P; e++) {
        if (F::out_index(0, e) < L) {                                    // compile time: out_index(tid, e) = tid + const, tid < NT <= L
            const int n = F::out_index(tid, e);
            const float v = fade_blend(re[e], im[e], a.f, m_blk + n);
            out[(long)n * C] = v;
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
        DevOverflow *of = of_shard(a.overflow, a.of_shard_stride) + gc;
        if (n2) atomicAdd(&of->n_overflows, n2);
        // filtered: the peak only ever grows, a stale read costs an extra atomic, never a wrong result
        if ((unsigned long long)m2 > *(volatile unsigned long long *)&of->largest_bits)
            atomicMax(&of->largest_bits, (unsigned long long)m2);
    }
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
    constexpr int V4 = 16 / (int)sizeof(float), V8 = 16 / (int)sizeof(double);
    const int vec = a.realsize == 4 ? V4 : V8;
    const bool aligned = a.n % vec == 0 && a.ch_stride % vec == 0 && ((uintptr_t)a.y_old | (uintptr_t)a.y_new) % 16 == 0;
    const long lanes = aligned ? a.n / vec : a.n;
    const dim3 grid((unsigned)((lanes + 255) / 256), (unsigned)a.n_ch), block(256);
    if (a.realsize == 4) {
        if (aligned) hipLaunchKernelGGL((k_fade_blend<float, V4>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((k_fade_blend<float, 1>), grid, block, 0, s, a);
    } else {
        if (aligned) hipLaunchKernelGGL((k_fade_blend<double, V8>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((k_fade_blend<double, 1>), grid, block, 0, s, a);
    }
}

}  // namespace bfir
