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
//   k_inv_levels      fp32, (re, im) pairs, FLOAT_LE frames, even channel count, 512 <= L <= 8192.  k_inv_nup with NR = 2 or
//                     3 rings: one workgroup is one (channel pair, block), Z = Y_a + i Y_b, ONE complex inverse of N = 2L
//                     points, both channels' ring samples added, overflow statistics and NaN guard of real2raw
//                     (brutefir/real2raw.cpp:321-336, brutefir.cpp:316-321), 8-byte stores (both channels of a frame).
//   k_levels_combine  everything else: launch_inv has written y_head as a planar time buffer; this adds the rings to it in
//                     place, in one pass, and launch_stage_out converts, counts and guards as for a plain chunk.
#include "kernels.h"

#include "fft_lds.h"

namespace bfir {

namespace {

template <int LOG2N, int NR>
__global__ __launch_bounds__(FftCfg<LOG2N>::NT) void k_inv_levels(LevelsInvArgs a, const float2 *__restrict__ tw)
{
    using F = LdsFft<float, LOG2N, +1>;
    constexpr int N = F::M, NT = F::NT, P = F::P, L = N / 2, Q = P / 4;   // Q 16-byte pieces per thread and spectrum
    constexpr int NW = NT / 64 > 0 ? NT / 64 : 1;
    static_assert(N <= F::LDS_ELEMS, "both spectra (2 x L pairs) are staged in the transform's buffer");
    static_assert(NR >= 2 && NR <= BFIR_LEVEL_RINGS, "one ring is k_inv_nup's");
    __shared__ __attribute__((aligned(16))) float2 lds[F::LDS_ELEMS];
    __shared__ unsigned int red_max[NW][2], red_cnt[NW][2];

    const int tid = threadIdx.x;
    // the channel pairs of a block store into the same cache lines of the output frames: one XCD
    const int w = xcd_work_item(blockIdx.x, gridDim.x);
    const int pairs = a.n_ch >> 1;
    const int t = w / pairs, gc = 2 * (w - t * pairs);
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    struct __attribute__((packed, aligned(4))) frame2 { float x, y; };   // both channels of a frame, one store
    const f32x4 *__restrict__ ya = (const f32x4 *)(a.y + (long)gc * a.y_ch_stride + (long)t * N);
    const f32x4 *__restrict__ yb = (const f32x4 *)(a.y + (long)(gc + 1) * a.y_ch_stride + (long)t * N);

    // both spectra into LDS: Y_a at [0, L), Y_b at [L, 2L)  (float2 units); each is read once: nontemporal
    {
        f32x4 *l4 = (f32x4 *)lds;
#pragma unroll
        for (int j = 0; j < Q; j++) {
            l4[tid + j * NT] = __builtin_nontemporal_load(ya + tid + j * NT);
            l4[L / 2 + tid + j * NT] = __builtin_nontemporal_load(yb + tid + j * NT);
        }
    }
    __syncthreads();
    // Z[k] = Y_a[k] + i Y_b[k], Hermitian-extended to the full circle (k_inv_pair_ps); bin 0 carries DC | Nyquist
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
        else          { zr = pa.x + pb.y; zi = pb.x - pa.y; }             // conj Y_a + i conj Y_b
        if (base == 0) { zr = edge ? pa.x : zr; zi = edge ? pb.x : zi; }   // DC of both
        if (base == L) { zr = edge ? pa.y : zr; zi = edge ? pb.y : zi; }   // Nyquist of both
        re[e] = zr * a.scale; im[e] = zi * a.scale;
    });
    pin_registers(re, im);   // every read of the staged spectra happens before run()'s first barrier

    F::run(re, im, lds, tw, tid);

    // first L samples are the valid half: Re z = channel gc, Im z = channel gc + 1.  The block's L samples of a ring are
    // contiguous (zlen, m0 and m_min are multiples of L): a ring wraps between blocks only, and a block has all of a
    // ring's samples or none.  A ring without samples for this block is read at its start and its samples dropped.
    const int C = a.frame_stride ? a.frame_stride : a.n_ch;   // floats between frames
    float *__restrict__ out = a.raw + (a.frame_off + (long)t * L) * C + gc;
    const float *__restrict__ za[NR];
    bool has_z[NR];
#pragma unroll
    for (int r = 0; r < NR; r++) {
        const LevelRing &g = a.ring[r];
        has_z[r] = g.m0 + (long long)t * L >= g.m_min;
        long zi0 = g.m0r + (long)t * L;
        zi0 = zi0 >= g.zlen ? zi0 - g.zlen : zi0;
        za[r] = (const float *)g.z + (long)gc * g.z_ch_stride + (has_z[r] ? zi0 : 0);
    }
    const float rmax = a.max;
    float pk0 = 0.f, pk1 = 0.f;
    unsigned int c0 = 0u, c1 = 0u;
#pragma unroll
    for (int e = 0; e < P; e++) {
        if (F::out_index(0, e) < L) {                                    // compile time: out_index(tid, e) = tid + const, tid < NT <= L
            const int n = F::out_index(tid, e);
            float2 v;
            v.x = re[e]; v.y = im[e];
#pragma unroll
            for (int r = 0; r < NR; r++) {                               // level order: ((y + z_0) + z_1) + z_2
                const float z0 = za[r][n], z1 = za[r][a.ring[r].z_ch_stride + n];
                v.x = has_z[r] ? v.x + z0 : v.x;
                v.y = has_z[r] ? v.y + z1 : v.y;
            }
            *(frame2 *)(out + (long)n * C) = frame2{v.x, v.y};                         // gc even; C even: 8-byte aligned, odd (a matrix engine's lone output beside the pairs): 4
            // real2raw.cpp:321-336 with symmetric limits: |v| > max, NaN never counts (k_inv_pair_ps)
            c0 += (fabsf(v.x) > rmax) ? 1u : 0u;
            c1 += (fabsf(v.y) > rmax) ? 1u : 0u;
            pk0 = fmaxf(pk0, fabsf(v.x)); pk1 = fmaxf(pk1, fabsf(v.y));
            // brutefir.cpp:316-321: only sample 0 of each block is checked
            if (F::out_index(0, e) == 0) {
                if (n == 0 && !(isfinite(v.x) && isfinite(v.y))) flag_bad(a, t);
            }
        }
    }
    unsigned int mx0 = __float_as_uint(pk0), mx1 = __float_as_uint(pk1);   // non-negative floats order like their bits
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned int m0 = __shfl_xor(mx0, o), m1 = __shfl_xor(mx1, o);
        mx0 = m0 > mx0 ? m0 : mx0; mx1 = m1 > mx1 ? m1 : mx1;
        c0 += __shfl_xor(c0, o); c1 += __shfl_xor(c1, o);
    }
    if ((tid & 63) == 0) { red_max[tid >> 6][0] = mx0; red_max[tid >> 6][1] = mx1; red_cnt[tid >> 6][0] = c0; red_cnt[tid >> 6][1] = c1; }
    __syncthreads();
    if (tid < 2) {
        unsigned int m2 = 0u, n2 = 0u;
        for (int wv = 0; wv < NW; wv++) { m2 = red_max[wv][tid] > m2 ? red_max[wv][tid] : m2; n2 += red_cnt[wv][tid]; }
        DevOverflow *of = of_shard(a.overflow, a.of_shard_stride) + gc + tid;
        if (n2) atomicAdd(&of->n_overflows, n2);
        // filtered: the peak only ever grows, a stale read costs an extra atomic, never a wrong result
        if ((unsigned long long)m2 > *(volatile unsigned long long *)&of->largest_bits)
            atomicMax(&of->largest_bits, (unsigned long long)m2);
    }
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
    if (a.n <= 0 || a.n_ch <= 0 || a.n_rings < 1 || a.n_rings > BFIR_LEVEL_RINGS) return;
    constexpr int V4 = 16 / (int)sizeof(float), V8 = 16 / (int)sizeof(double);
    const int vec = a.realsize == 4 ? V4 : V8;
    bool aligned = a.n % vec == 0 && a.y_ch_stride % vec == 0 && (uintptr_t)a.y % 16 == 0;
    for (int r = 0; r < a.n_rings; r++)
        aligned = aligned && a.ring[r].z_ch_stride % vec == 0 && a.ring[r].zlen % vec == 0 && a.ring[r].m0r % vec == 0 &&
                  (uintptr_t)a.ring[r].z % 16 == 0;
    const long lanes = aligned ? a.n / vec : a.n;
    const dim3 grid((unsigned)((lanes + 255) / 256), (unsigned)a.n_ch), block(256);
    if (a.realsize == 4) {
        if (aligned) hipLaunchKernelGGL((k_levels_combine<float, V4>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((k_levels_combine<float, 1>), grid, block, 0, s, a);
    } else {
        if (aligned) hipLaunchKernelGGL((k_levels_combine<double, V8>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((k_levels_combine<double, 1>), grid, block, 0, s, a);
    }
}

}  // namespace bfir
