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
//                3 rings per set: one workgroup is one (channel, block), Z = Y_old + i Y_new, ONE complex inverse of
//                N = 2L points, the old rings added to the real part and the new rings to the imaginary part, blend,
//                overflow statistics and NaN guard of real2raw (brutefir/real2raw.cpp:321-336, brutefir.cpp:316-321),
//                4-byte stores at the frame stride.
//   k_lfade_sum  everything else: launch_inv has written y_old and y_new as planar time buffers; this adds each set's
//                rings and blends into y_old in place, in one pass, and launch_stage_out converts, counts and guards as
//                for a plain chunk of the staging path.
#include "kernels.h"

#include "fade_blend.h"
#include "fft_lds.h"

namespace bfir {

namespace {

template <int LOG2N, int NR>
__global__ __launch_bounds__(FftCfg<LOG2N>::NT) void k_inv_lfade(LfadeInvArgs a, const float2 *__restrict__ tw)
{
    using F = LdsFft<float, LOG2N, +1>;
    constexpr int N = F::M, NT = F::NT, P = F::P, L = N / 2, Q = P / 4;   // Q 16-byte pieces per thread and spectrum
    constexpr int NW = NT / 64 > 0 ? NT / 64 : 1;
    static_assert(N <= F::LDS_ELEMS, "both spectra (2 x L pairs) are staged in the transform's buffer");
    static_assert(NR >= 1 && NR <= BFIR_LEVEL_RINGS, "no ring is k_inv_fade's");
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
    // Z[k] = Y_old[k] + i Y_new[k], Hermitian-extended to the full circle (k_inv_fade); bin 0 carries DC | Nyquist
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

    // first L samples are the valid half: Re z = y_old, Im z = y_new.  The block's L samples of a ring are contiguous
    // (zlen, m0 and m_min are multiples of L): a ring wraps between blocks only, and a block has all of a ring's samples
    // or none (k_inv_levels).  A ring without samples for this block is read at its start and its samples dropped.  The
    // two rings of a level share their geometry.
    const int C = a.n_ch;
    float *__restrict__ out = a.raw + (a.frame_off + (long)t * L) * C + gc;
    const float *__restrict__ zo[NR], *__restrict__ zn[NR];
    bool has_z[NR];
#pragma unroll
    for (int r = 0; r < NR; r++) {
        const LevelRing &g = a.ring[r];
        has_z[r] = g.m0 + (long long)t * L >= g.m_min;
        long zi0 = g.m0r + (long)t * L;
        zi0 = zi0 >= g.zlen ? zi0 - g.zlen : zi0;
        const long at = (long)gc * g.z_ch_stride + (has_z[r] ? zi0 : 0);
        zo[r] = (const float *)g.z + at;
        zn[r] = (const float *)a.z_new[r] + at;
    }
    const int m_blk = a.m0 + t * L;
    const float rmax = a.max;
    float pk = 0.f;
    unsigned int cnt = 0u;
#pragma unroll
    for (int e = 0; e < P; e++) {
        if (F::out_index(0, e) < L) {                                    // compile time: out_index(tid, e) = tid + const, tid < NT <= L
            const int n = F::out_index(tid, e);
            float so = re[e], sn = im[e];
#pragma unroll
            for (int r = 0; r < NR; r++) {                               // level order: ((y + z_0) + z_1) + z_2, per set
                const float z0 = zo[r][n], z1 = zn[r][n];
                so = has_z[r] ? so + z0 : so;
                sn = has_z[r] ? sn + z1 : sn;
            }
            const float v = fade_blend(so, sn, a.f, m_blk + n);
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
    constexpr int V4 = 16 / (int)sizeof(float), V8 = 16 / (int)sizeof(double);
    const int vec = a.realsize == 4 ? V4 : V8;
    // the rule of launch_levels_combine, over both sets of rings
    bool aligned = a.n % vec == 0 && a.ch_stride % vec == 0 && ((uintptr_t)a.y_old | (uintptr_t)a.y_new) % 16 == 0;
    for (int r = 0; r < a.n_rings; r++)
        aligned = aligned && a.ring[r].z_ch_stride % vec == 0 && a.ring[r].zlen % vec == 0 && a.ring[r].m0r % vec == 0 &&
                  ((uintptr_t)a.ring[r].z | (uintptr_t)a.z_new[r]) % 16 == 0;
    const long lanes = aligned ? a.n / vec : a.n;
    const dim3 grid((unsigned)((lanes + 255) / 256), (unsigned)a.n_ch), block(256);
    if (a.realsize == 4) {
        if (aligned) hipLaunchKernelGGL((k_lfade_sum<float, V4>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((k_lfade_sum<float, 1>), grid, block, 0, s, a);
    } else {
        if (aligned) hipLaunchKernelGGL((k_lfade_sum<double, V8>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((k_lfade_sum<double, 1>), grid, block, 0, s, a);
    }
}

}  // namespace bfir
