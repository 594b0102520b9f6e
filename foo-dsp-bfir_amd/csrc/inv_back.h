// inv_back.h -- the one body of the one-transform fused back ends (k_inv_fade, k_inv_nup, k_inv_levels, k_inv_lfade,
// k_inv_lone): stage, Hermitian extension, ONE complex inverse of N = 2L points, then per sample of the valid half what
// the kernel's emit step makes of (Re z, Im z), with the overflow statistics and the NaN guard of real2raw
// (brutefir/real2raw.cpp:321-336, brutefir.cpp:316-321) on what it stored.
#pragma once
#include "kernels.h"

#include "fft_lds.h"

namespace bfir {

namespace {

// Where block t of a chunk finds channel ch's samples of its NR contributing rings (NR = 0: none).  The block's L samples
// of a ring are contiguous (zlen, m0 and m_min are multiples of L): a ring wraps between blocks only, and a block has all
// of a ring's samples or none.  A ring without samples for this block is read at its start and its samples dropped.
template <int NR> struct BlockRings {
    long at[NR > 0 ? NR : 1];        // offset of sample 0 of the block within ring r, in reals from ring[r].z
    unsigned keep[NR > 0 ? NR : 1];  // all ones where the block has the ring's samples, else 0 (ring_add)
};
// has ? v + z : v, bit for bit, as a bit select under the ring's mask.  Written with a condition, some instances get a
// branch around the addition per sample, with the ring load sunk into it and waited for there, and those ran 2 .. 6 %
// slower than the ones that got a select (profiles/inv_back.txt); the mask comes out of an asm statement so that it stays
// a mask.
__device__ __forceinline__ float ring_add(float v, float z, unsigned keep)
{
    const float s = v + z;
    return __uint_as_float((__float_as_uint(s) & keep) | (__float_as_uint(v) & ~keep));
}
template <int NR, int L>
__device__ __forceinline__ BlockRings<NR> block_rings(const LevelRing (&ring)[BFIR_LEVEL_RINGS], int t, int ch)
{
    static_assert(NR >= 0 && NR <= BFIR_LEVEL_RINGS, "no ring (a chunk to which no level contributes) to three");
    BlockRings<NR> b;
#pragma unroll
    for (int r = 0; r < NR; r++) {
        const LevelRing &g = ring[r];
        const bool has = g.m0 + (long long)t * L >= g.m_min;
        long zi0 = g.m0r + (long)t * L;
        zi0 = zi0 >= g.zlen ? zi0 - g.zlen : zi0;
        b.at[r] = (long)ch * g.z_ch_stride + (has ? zi0 : 0);
        b.keep[r] = __builtin_amdgcn_readfirstlane(has ? ~0u : 0u);   // t is the workgroup's: a scalar
        asm volatile("" : "+s"(b.keep[r]));
    }
    return b;
}

// One workgroup (FftCfg<LOG2N>::NT threads), one transform.  ya / yb: the block's product spectra, (re, im) pairs, L of
// them each; TWO: Z = Y_a + i Y_b (two channels, or the two filter sets of one), else Z = Y_a + i 0 and the imaginary half
// of the result means nothing.  make_emit() is called once the transform is done and returns the emit step: emit(n, re,
// im, v) turns sample n < L of the result into the K samples it stores, v[0 .. K) -- those of channels ch .. ch + K - 1,
// whose DevOverflow entries are updated; block t of the launch is flagged where sample 0 of one of them is not finite.
// What a kernel works out inside make_emit does not stand in front of the staging loads (k_inv_fade<13>: 1.4 % of its
// time); the ring kernels work out their pointers before the call, where registers are free (inside: 8 more VGPRs and
// k_inv_levels<10,2> 0.7 % slower).  profiles/inv_back.txt has both.
template <int LOG2N, bool TWO, int K, typename MakeEmit>
__device__ __forceinline__ void inv_back_block(const float *__restrict__ ya, const float *__restrict__ yb, float scale,
                                               const float2 *__restrict__ tw, const InvStats &st, int t, int ch, MakeEmit make_emit)
{
    using F = LdsFft<float, LOG2N, +1>;
    constexpr int N = F::M, NT = F::NT, P = F::P, L = N / 2, Q = P / 4;   // Q 16-byte pieces per thread and spectrum
    constexpr int NW = NT / 64 > 0 ? NT / 64 : 1;
    static_assert((TWO ? N : L) <= F::LDS_ELEMS, "the spectra (L pairs each) are staged in the transform's buffer");
    static_assert(K == 1 || K == 2, "samples per frame");
    __shared__ __attribute__((aligned(16))) float2 lds[F::LDS_ELEMS];
    __shared__ unsigned int red_max[NW][K], red_cnt[NW][K];

    const int tid = threadIdx.x;
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    // the spectra into LDS: Y_a at [0, L), Y_b at [L, 2L)  (float2 units); each is read once: nontemporal
    {
        const f32x4 *__restrict__ a4 = (const f32x4 *)ya, *__restrict__ b4 = (const f32x4 *)yb;
        f32x4 *l4 = (f32x4 *)lds;
#pragma unroll
        for (int j = 0; j < Q; j++) {
            l4[tid + j * NT] = __builtin_nontemporal_load(a4 + tid + j * NT);
            if constexpr (TWO) l4[L / 2 + tid + j * NT] = __builtin_nontemporal_load(b4 + tid + j * NT);
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
        const float2 pa = lds[edge ? 0 : kk];
        float zr, zi;
        if constexpr (TWO) {
            const float2 pb = lds[L + (edge ? 0 : kk)];
            if (base < L) { zr = pa.x - pb.y; zi = pa.y + pb.x; }
            else          { zr = pa.x + pb.y; zi = pb.x - pa.y; }             // conj Y_a + i conj Y_b
            if (base == 0) { zr = edge ? pa.x : zr; zi = edge ? pb.x : zi; }   // DC of both
            if (base == L) { zr = edge ? pa.y : zr; zi = edge ? pb.y : zi; }   // Nyquist of both
        } else {
            zr = pa.x; zi = (base < L) ? pa.y : -pa.y;                        // the upper half: conj Y
            if (base == 0) zi = edge ? 0.f : zi;                              // DC
            if (base == L) { zr = edge ? pa.y : zr; zi = edge ? 0.f : zi; }   // Nyquist
        }
        re[e] = zr * scale; im[e] = zi * scale;
    });
    pin_registers(re, im);   // every read of the staged spectra happens before run()'s first barrier

    F::run(re, im, lds, tw, tid);

    // first L samples are the valid half
    const auto emit = make_emit();
    const float rmax = st.max;
    float pk[K];
    unsigned int cnt[K];
#pragma unroll
    for (int c = 0; c < K; c++) { pk[c] = 0.f; cnt[c] = 0u; }
#pragma unroll
    for (int e = 0; e < P; e++) {
        if (F::out_index(0, e) < L) {                                    // compile time: out_index(tid, e) = tid + const, tid < NT <= L
            const int n = F::out_index(tid, e);
            float v[K];
            emit(n, re[e], im[e], v);
            bool finite = true;
#pragma unroll
            for (int c = 0; c < K; c++) {
                // real2raw.cpp:321-336 with symmetric limits: |v| > max, NaN never counts (k_inv_pair_ps)
                cnt[c] += (fabsf(v[c]) > rmax) ? 1u : 0u;
                pk[c] = fmaxf(pk[c], fabsf(v[c]));
                finite = finite && isfinite(v[c]);
            }
            // brutefir.cpp:316-321: only sample 0 of each block is checked
            if (F::out_index(0, e) == 0) {
                if (n == 0 && !finite) flag_bad(st, t);
            }
        }
    }
    unsigned int mx[K];
#pragma unroll
    for (int c = 0; c < K; c++) mx[c] = __float_as_uint(pk[c]);          // non-negative floats order like their bits
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int c = 0; c < K; c++) {
            const unsigned int m2 = __shfl_xor(mx[c], o);
            mx[c] = m2 > mx[c] ? m2 : mx[c];
            cnt[c] += __shfl_xor(cnt[c], o);
        }
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int c = 0; c < K; c++) { red_max[tid >> 6][c] = mx[c]; red_cnt[tid >> 6][c] = cnt[c]; }
    }
    __syncthreads();
    if (tid < K) {
        unsigned int m2 = 0u, n2 = 0u;
        for (int wv = 0; wv < NW; wv++) { m2 = red_max[wv][tid] > m2 ? red_max[wv][tid] : m2; n2 += red_cnt[wv][tid]; }
        DevOverflow *of = of_shard(st.overflow, st.of_shard_stride) + ch + tid;
        if (n2) atomicAdd(&of->n_overflows, n2);
        // filtered: the peak only ever grows, a stale read costs an extra atomic, never a wrong result
        if ((unsigned long long)m2 > *(volatile unsigned long long *)&of->largest_bits)
            atomicMax(&of->largest_bits, (unsigned long long)m2);
    }
}

// The channel-pair form with NR = 1 .. 3 rings, the whole of k_inv_nup<LOG2N> (NR = 1) and k_inv_levels<LOG2N, NR>: one
// workgroup is one (channel pair, block), Re z = channel gc, Im z = channel gc + 1, the rings added in level order,
// ((y + z_0) + z_1) + z_2, one 8-byte store per frame.
template <int LOG2N, int NR>
__device__ __forceinline__ void inv_back_pair_rings(const LevelsInvArgs &a, const float2 *__restrict__ tw)
{
    constexpr int N = 1 << LOG2N, L = N / 2;
    static_assert(NR >= 1, "no ring is k_inv_pair_ps'");
    // the channel pairs of a block store into the same cache lines of the output frames: one XCD
    const int w = xcd_work_item(blockIdx.x, gridDim.x);
    const int pairs = a.n_ch >> 1;
    const int t = w / pairs, gc = 2 * (w - t * pairs);
    struct __attribute__((packed, aligned(4))) frame2 { float x, y; };   // both channels of a frame, one store
    const int C = a.frame_stride ? a.frame_stride : a.n_ch;   // floats between frames
    float *__restrict__ out = a.raw + (a.frame_off + (long)t * L) * C + gc;
    const BlockRings<NR> br = block_rings<NR, L>(a.ring, t, gc);
    const float *__restrict__ za[NR], *__restrict__ zb[NR];
#pragma unroll
    for (int r = 0; r < NR; r++) { za[r] = (const float *)a.ring[r].z + br.at[r]; zb[r] = za[r] + a.ring[r].z_ch_stride; }
    inv_back_block<LOG2N, true, 2>(a.y + (long)gc * a.y_ch_stride + (long)t * N, a.y + (long)(gc + 1) * a.y_ch_stride + (long)t * N,
                                   a.scale, tw, a.st, t, gc, [&] {
        return [=](int n, float re, float im, float (&v)[2]) {
            v[0] = re; v[1] = im;
#pragma unroll
            for (int r = 0; r < NR; r++) {
                v[0] = ring_add(v[0], za[r][n], br.keep[r]);
                v[1] = ring_add(v[1], zb[r][n], br.keep[r]);
            }
            *(frame2 *)(out + (long)n * C) = frame2{v[0], v[1]};   // gc even; C even: 8-byte aligned, odd (a matrix engine's lone output beside the pairs): 4
        };
    });
}

}  // namespace

}  // namespace bfir
