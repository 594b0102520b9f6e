// bigconv.hip -- batched real FFTs of partitions that do not fit one workgroup's LDS (2^15 .. 2^20 samples in fp32,
// 2^14 .. 2^20 in fp64): the transforms of a "big" engine (bfir_engine_create_big).
//
// N = 2L reals are M = L complex points z[m] = (x[2m], x[2m+1]), M = M1 M2, transformed in two passes per direction over
// the workgroup FFT of fft_lds.h (input m = n1 M2 + n2, bin k = k1 + M1 k2):
//   forward A  k_big_fwd_cols  a tile of W adjacent columns n2 (128 contiguous bytes per row n1) straight from the planar
//                              time buffers, W FFTs of M1 points side by side, times exp(-2 pi i n2 k1 / M), stored as
//                              [k1][n2] (128-byte pieces) into the block's slot of the delay line;
//   forward B  k_big_fwd_rows  rows k1 and M1 - k1 of that slot (rows 0 and M1/2 share a workgroup), FFTs of M2 points on
//                              contiguous data, the real split X_k = E_k + W^k O_k between the two rows, stored back in
//                              place in the engine's layout, (re, im) pairs or groups of 4 re | 4 im.
//   inverse A' k_big_inv_rows  the same row pairs of a product spectrum, Z_k = (Y_k + conj Y_{M-k}) + i conj(W^k) (Y_k -
//                              conj Y_{M-k}), inverse FFTs of M2 points, times exp(+2 pi i n2 k1 / M), in place as pairs;
//   inverse B' k_big_inv_cols  tiles of W columns, inverse FFTs of M1 points, the rows n1 < M1/2 (the valid half) to the
//                              planar output in 128-byte pieces.
// The spectra stay in TRANSPOSED bin order: bin k = k1 + M1 k2 lives at position k1 M2 + k2.  X, H and Y of a big engine
// share the order and the MAC kernels, elementwise per position, never notice; bin 0 is position 0 (DC | Nyquist).  The
// partner bin M - k of (k1, k2) is (M1 - k1, M2 - 1 - k2), and (0, M2 - k2) in row 0.  So a transform makes two round trips
// through HBM, every access is lane-consecutive, and nothing is transposed.
// Twiddles between the passes and of the split come from host tables (long double, like every table here) of at most 1024
// entries: exp(-2 pi i j / M) = T_hi[j >> 10] T_lo[j & 1023], one complex multiply, no transcendental call.
#include "kernels.h"

#include <cmath>
#include <cstdio>
#include <vector>

#include "fft_lds.h"

namespace bfir {

namespace {

constexpr int BIG_LO_BITS = 10;

template <typename T> static void *big_upload(const std::vector<long double> &v)
{
    std::vector<T> h(v.size());
    for (size_t i = 0; i < v.size(); i++) h[i] = (T)v[i];
    void *d = nullptr;
    if (hipMalloc(&d, h.size() * sizeof(T)) != hipSuccess) return nullptr;
    if (hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return nullptr; }
    return d;
}

// exp(-2 pi i (j << shift) / period), j < n
static void big_fill(std::vector<long double> &t, int n, int shift, long period)
{
    const long double two_pi = 6.283185307179586476925286766559L;
    t.resize(2 * (size_t)n);
    for (int j = 0; j < n; j++) {
        const long double ang = -two_pi * (long double)((long)j << shift) / (long double)period;
        t[2 * (size_t)j] = cosl(ang);
        t[2 * (size_t)j + 1] = sinl(ang);
    }
}

// exp(-2 pi i j / period) from the two tables of a period
template <typename V2> __device__ __forceinline__ V2 big_tw(const V2 *__restrict__ hi, const V2 *__restrict__ lo, unsigned j)
{
    const V2 a = hi[j >> BIG_LO_BITS], c = lo[j & ((1u << BIG_LO_BITS) - 1u)];
    V2 w; w.x = a.x * c.x - a.y * c.y; w.y = a.x * c.y + a.y * c.x;
    return w;
}

// work item -> (block t, channel gc, part): blocks major, the parts of one transform adjacent (one XCD's L2)
__device__ __forceinline__ void big_item(int n_part, int n_ch, int &t, int &gc, int &part)
{
    const int wi = xcd_work_item(blockIdx.x, gridDim.x);
    const int tr = wi / n_part;
    part = wi - tr * n_part;
    t = tr / n_ch; gc = tr - t * n_ch;
}

// the two rows of work item rp < M1/2: (0, M1/2), each its own mirror image, or (rp, M1 - rp), mirror images of each other
__device__ __forceinline__ int big_row(int rp, int half, int M1) { return rp == 0 ? (half ? M1 / 2 : 0) : (half ? M1 - rp : rp); }
// position within its row of the partner bin M - k of (row, k2)
__device__ __forceinline__ int big_partner(int rp, int half, int k2, int M2) { return (rp == 0 && half == 0) ? ((M2 - k2) & (M2 - 1)) : M2 - 1 - k2; }

// ---- forward A: columns --------------------------------------------------------------------------------------------
template <typename T, int LG1, int W>
__global__ __launch_bounds__(FftCfg<LG1>::NT * W) void k_big_fwd_cols(FwdArgs a, int log2m2,
                                                                      const typename Vec2<T>::type *__restrict__ tw,
                                                                      const typename Vec2<T>::type *__restrict__ thi,
                                                                      const typename Vec2<T>::type *__restrict__ tlo)
{
    using F = LdsFft<T, LG1, -1>;
    using V2 = typename Vec2<T>::type;
    constexpr int M1 = F::M, P = F::P, LS = F::LDS_ELEMS | 1;   // odd stride: the W transforms on different banks
    __shared__ __attribute__((aligned(16))) V2 lds_all[W * LS];
    const int col = (int)threadIdx.x % W, tid = (int)threadIdx.x / W;
    const int M2 = 1 << log2m2;
    const long M = (long)M1 << log2m2;
    int t, gc, tile;
    big_item(M2 / W, a.n_ch, t, gc, tile);
    const int n2 = tile * W + col;
    const T *__restrict__ cur = (const T *)a.src + (long)gc * a.src_ch_stride + (long)t * M;
    const T *__restrict__ old = (t == 0) ? (const T *)a.prev + (long)gc * a.prev_ch_stride : cur - M;
    V2 *__restrict__ dst = (V2 *)((T *)a.dst + (long)gc * a.dst_ch_stride + (long)((a.base_slot + t) % a.ring) * (2 * M));

    // z[m] = x[2m] + i x[2m+1] over the window [previous block | this block], m = n1 M2 + n2
    T re[P], im[P];
    const T ls = (T)a.load_scale;
#pragma unroll
    for (int e = 0; e < P; e++) {
        const int n1 = F::in_index(tid, e);
        const long m = (long)n1 * M2 + n2;
        if (n1 < M1 / 2) {
            if (a.zero_first_half) {
                re[e] = (T)0; im[e] = (T)0;
            } else {
                const V2 v = *(const V2 *)(old + 2 * m);
                re[e] = v.x * ls; im[e] = v.y * ls;
            }
        } else {
            const V2 v = *(const V2 *)(cur + (2 * m - M));
            re[e] = v.x * ls; im[e] = v.y * ls;
        }
    }

    F::run(re, im, lds_all + col * LS, tw, tid);

#pragma unroll
    for (int e = 0; e < P; e++) {
        const int k1 = F::out_index(tid, e);
        const V2 w = big_tw(thi, tlo, (unsigned)k1 * (unsigned)n2);
        cmul(re[e], im[e], w.x, w.y);
        V2 v; v.x = re[e]; v.y = im[e];
        dst[(long)k1 * M2 + n2] = v;
    }
}

// ---- forward B: rows, in place ---------------------------------------------------------------------------------------
template <typename T, int LG2, bool ILV>
__global__ __launch_bounds__(FftCfg<LG2>::NT * 2) void k_big_fwd_rows(FwdArgs a, int log2m1,
                                                                      const typename Vec2<T>::type *__restrict__ tw,
                                                                      const typename Vec2<T>::type *__restrict__ shi,
                                                                      const typename Vec2<T>::type *__restrict__ slo)
{
    using F = LdsFft<T, LG2, -1>;
    using V2 = typename Vec2<T>::type;
    using V4 = typename Vec4<T>::type;
    constexpr int M2 = F::M, NT = F::NT, P = F::P;
    static_assert(NT >= 64, "the two rows of a workgroup are whole waves");
    __shared__ __attribute__((aligned(16))) V2 lds_all[2][F::LDS_ELEMS];
    const int half = (int)threadIdx.x / NT, tid = (int)threadIdx.x - half * NT;
    const int M1 = 1 << log2m1;
    const long M = (long)M2 << log2m1;
    int t, gc, rp;
    big_item(M1 / 2, a.n_ch, t, gc, rp);
    const int row = big_row(rp, half, M1);
    V2 *__restrict__ rowp = (V2 *)((T *)a.dst + (long)gc * a.dst_ch_stride + (long)((a.base_slot + t) % a.ring) * (2 * M)) + (long)row * M2;
    V2 *lds = lds_all[half];

    T re[P], im[P];
#pragma unroll
    for (int e = 0; e < P; e++) {
        const V2 v = rowp[F::in_index(tid, e)];
        re[e] = v.x; im[e] = v.y;
    }

    F::run(re, im, lds, tw, tid);

    // Z in natural order to LDS so every thread can fetch Z[M-k] from the partner row
    __syncthreads();
#pragma unroll
    for (int e = 0; e < P; e++) {
        V2 v; v.x = re[e]; v.y = im[e];
        lds[F::phys(F::out_index(tid, e))] = v;
    }
    __syncthreads();
    // X_k = E_k + W^k O_k,  E = (Z_k + conj Z_{M-k})/2,  O = -i (Z_k - conj Z_{M-k})/2
    const V2 *plds = rp == 0 ? lds_all[half] : lds_all[half ^ 1];
    const T os = (T)a.out_scale;
#pragma unroll
    for (int e = 0; e < P; e++) {
        const int k2 = F::out_index(tid, e);
        const unsigned k = (unsigned)row + ((unsigned)k2 << log2m1);
        const V2 pz = plds[F::phys(big_partner(rp, half, k2, M2))];
        const V2 w = big_tw(shi, slo, k);
        T er = (T)0.5 * (re[e] + pz.x), ei = (T)0.5 * (im[e] - pz.y);
        T orr = (T)0.5 * (im[e] + pz.y), oi = (T)-0.5 * (re[e] - pz.x);
        T tr = orr * w.x - oi * w.y, ti = orr * w.y + oi * w.x;
        T xr = er + tr, xi = ei + ti;
        if (k == 0) xi = re[e] - im[e];  // the imaginary slot of bin 0 carries Re X_{N/2}
        re[e] = xr * os; im[e] = xi * os;
    }
    pin_registers(re, im);   // every Z[M-k] read happens before the barrier
    __syncthreads();
    T *ldsr = (T *)lds;
#pragma unroll
    for (int e = 0; e < P; e++) {
        const int k2 = F::out_index(tid, e);   // the row starts on a group boundary: the layout is that of its positions
        if constexpr (ILV) {
            V2 v; v.x = re[e]; v.y = im[e];
            ((V2 *)ldsr)[k2] = v;
        } else {
            ldsr[8 * (k2 >> 2) + (k2 & 3)] = re[e];
            ldsr[8 * (k2 >> 2) + 4 + (k2 & 3)] = im[e];
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < P / 2; j++) {
        const int idx = tid + j * NT;
        ((V4 *)rowp)[idx] = ((const V4 *)ldsr)[idx];
    }
}

// ---- inverse A': rows, in place --------------------------------------------------------------------------------------
template <typename T, int LG2, bool ILV>
__global__ __launch_bounds__(FftCfg<LG2>::NT * 2) void k_big_inv_rows(InvArgs a, int log2m1,
                                                                      const typename Vec2<T>::type *__restrict__ tw,
                                                                      const typename Vec2<T>::type *__restrict__ shi,
                                                                      const typename Vec2<T>::type *__restrict__ slo,
                                                                      const typename Vec2<T>::type *__restrict__ thi,
                                                                      const typename Vec2<T>::type *__restrict__ tlo)
{
    using F = LdsFft<T, LG2, +1>;
    using V2 = typename Vec2<T>::type;
    using V4 = typename Vec4<T>::type;
    constexpr int M2 = F::M, NT = F::NT, P = F::P;
    static_assert(NT >= 64, "the two rows of a workgroup are whole waves");
    __shared__ __attribute__((aligned(16))) V2 lds_all[2][F::LDS_ELEMS];
    const int half = (int)threadIdx.x / NT, tid = (int)threadIdx.x - half * NT;
    const int M1 = 1 << log2m1;
    const long M = (long)M2 << log2m1;
    int t, gc, rp;
    big_item(M1 / 2, a.n_ch, t, gc, rp);
    const int row = big_row(rp, half, M1);
    // the product spectrum is consumed here: the columns pass reads what this one leaves in its place
    V2 *__restrict__ rowp = (V2 *)((T *)const_cast<void *>(a.src) + (long)gc * a.src_ch_stride + (long)t * (2 * M)) + (long)row * M2;
    V2 *lds = lds_all[half];

    T *ldsr = (T *)lds;
#pragma unroll
    for (int j = 0; j < P / 2; j++) {
        const int idx = tid + j * NT;
        ((V4 *)ldsr)[idx] = ((const V4 *)rowp)[idx];
    }
    __syncthreads();

    // Z_k = (Y_k + conj Y_{M-k}) + i conj(W^k) (Y_k - conj Y_{M-k})
    const T *pldsr = (const T *)(rp == 0 ? lds_all[half] : lds_all[half ^ 1]);
    T re[P], im[P];
    const T sc = (T)a.in_scale;
#pragma unroll
    for (int e = 0; e < P; e++) {
        const int k2 = F::in_index(tid, e);
        const int q = big_partner(rp, half, k2, M2);
        const unsigned k = (unsigned)row + ((unsigned)k2 << log2m1);
        T xr, xi, yr, yi;
        if constexpr (ILV) {
            const V2 vx = ((const V2 *)ldsr)[k2], vy = ((const V2 *)pldsr)[q];
            xr = vx.x * sc; xi = vx.y * sc; yr = vy.x * sc; yi = vy.y * sc;
        } else {
            xr = ldsr[8 * (k2 >> 2) + (k2 & 3)] * sc; xi = ldsr[8 * (k2 >> 2) + 4 + (k2 & 3)] * sc;
            yr = pldsr[8 * (q >> 2) + (q & 3)] * sc; yi = pldsr[8 * (q >> 2) + 4 + (q & 3)] * sc;
        }
        if (k == 0) { yr = xi; xi = (T)0; yi = (T)0; }  // Y_0 = (DC, 0), Y_M = (Nyquist, 0)
        const V2 w = big_tw(shi, slo, k);
        T ar = xr + yr, ai = xi - yi, br = xr - yr, bi = xi + yi;
        T tr = br * w.x + bi * w.y, ti = bi * w.x - br * w.y;
        re[e] = ar - ti; im[e] = ai + tr;
    }
    pin_registers(re, im);   // every read of the staged rows happens before run()'s first barrier

    F::run(re, im, lds, tw, tid);

    // lane-consecutive 8- or 16-byte stores straight from the registers: staging the row in LDS for 16-byte stores, as forward
    // B does, changed nothing in an alternated run ("Long partitions")
#pragma unroll
    for (int e = 0; e < P; e++) {
        const int n2 = F::out_index(tid, e);
        const V2 w = big_tw(thi, tlo, (unsigned)row * (unsigned)n2);
        cmul(re[e], im[e], w.x, -w.y);
        V2 v; v.x = re[e]; v.y = im[e];
        rowp[n2] = v;
    }
}

// ---- inverse B': columns ---------------------------------------------------------------------------------------------
template <typename T, int LG1, int W>
__global__ __launch_bounds__(FftCfg<LG1>::NT * W) void k_big_inv_cols(InvArgs a, int log2m2,
                                                                      const typename Vec2<T>::type *__restrict__ tw)
{
    using F = LdsFft<T, LG1, +1>;
    using V2 = typename Vec2<T>::type;
    constexpr int M1 = F::M, P = F::P, LS = F::LDS_ELEMS | 1;
    __shared__ __attribute__((aligned(16))) V2 lds_all[W * LS];
    const int col = (int)threadIdx.x % W, tid = (int)threadIdx.x / W;
    const int M2 = 1 << log2m2;
    const long M = (long)M1 << log2m2;
    int t, gc, tile;
    big_item(M2 / W, a.n_ch, t, gc, tile);
    const int n2 = tile * W + col;
    const V2 *__restrict__ src = (const V2 *)((const T *)a.src + (long)gc * a.src_ch_stride + (long)t * (2 * M));
    T *__restrict__ dst = (T *)a.dst + (long)gc * a.dst_ch_stride + (long)t * M;

    T re[P], im[P];
#pragma unroll
    for (int e = 0; e < P; e++) {
        const V2 v = src[(long)F::in_index(tid, e) * M2 + n2];
        re[e] = v.x; im[e] = v.y;
    }

    F::run(re, im, lds_all + col * LS, tw, tid);

    // z[m] = (y[2m], y[2m+1]), m = n1 M2 + n2: the first L samples are the rows n1 < M1/2
#pragma unroll
    for (int e = 0; e < P; e++) {
        const int n1 = F::out_index(tid, e);
        if (n1 < M1 / 2) {
            V2 v; v.x = re[e]; v.y = im[e];
            *(V2 *)(dst + 2 * ((long)n1 * M2 + n2)) = v;
        }
    }
}

// 128 contiguous bytes per row of a column tile
template <typename T> constexpr int big_w() { return 128 / (2 * (int)sizeof(T)); }

template <typename T, int LG1> void fwd_cols_t(const BigPlan &p, const FwdArgs &a, hipStream_t s)
{
    using V2 = typename Vec2<T>::type;
    constexpr int W = big_w<T>();
    const unsigned grid = (unsigned)((long)a.n_t * a.n_ch * ((1 << p.log2m2) / W));
    hipLaunchKernelGGL((k_big_fwd_cols<T, LG1, W>), dim3(grid), dim3(FftCfg<LG1>::NT * W), 0, s, a, p.log2m2, (const V2 *)p.p1.tw,
                       (const V2 *)p.t_hi, (const V2 *)p.t_lo);
}
template <typename T, int LG2> void fwd_rows_t(const BigPlan &p, const FwdArgs &a, hipStream_t s)
{
    using V2 = typename Vec2<T>::type;
    const unsigned grid = (unsigned)((long)a.n_t * a.n_ch * ((1 << p.log2m1) / 2));
    if (a.interleaved)
        hipLaunchKernelGGL((k_big_fwd_rows<T, LG2, true>), dim3(grid), dim3(FftCfg<LG2>::NT * 2), 0, s, a, p.log2m1, (const V2 *)p.p2.tw,
                           (const V2 *)p.s_hi, (const V2 *)p.s_lo);
    else
        hipLaunchKernelGGL((k_big_fwd_rows<T, LG2, false>), dim3(grid), dim3(FftCfg<LG2>::NT * 2), 0, s, a, p.log2m1, (const V2 *)p.p2.tw,
                           (const V2 *)p.s_hi, (const V2 *)p.s_lo);
}
template <typename T, int LG2> void inv_rows_t(const BigPlan &p, const InvArgs &a, hipStream_t s)
{
    using V2 = typename Vec2<T>::type;
    const unsigned grid = (unsigned)((long)a.n_t * a.n_ch * ((1 << p.log2m1) / 2));
    if (a.interleaved)
        hipLaunchKernelGGL((k_big_inv_rows<T, LG2, true>), dim3(grid), dim3(FftCfg<LG2>::NT * 2), 0, s, a, p.log2m1, (const V2 *)p.p2.tw,
                           (const V2 *)p.s_hi, (const V2 *)p.s_lo, (const V2 *)p.t_hi, (const V2 *)p.t_lo);
    else
        hipLaunchKernelGGL((k_big_inv_rows<T, LG2, false>), dim3(grid), dim3(FftCfg<LG2>::NT * 2), 0, s, a, p.log2m1, (const V2 *)p.p2.tw,
                           (const V2 *)p.s_hi, (const V2 *)p.s_lo, (const V2 *)p.t_hi, (const V2 *)p.t_lo);
}
template <typename T, int LG1> void inv_cols_t(const BigPlan &p, const InvArgs &a, hipStream_t s)
{
    using V2 = typename Vec2<T>::type;
    constexpr int W = big_w<T>();
    const unsigned grid = (unsigned)((long)a.n_t * a.n_ch * ((1 << p.log2m2) / W));
    hipLaunchKernelGGL((k_big_inv_cols<T, LG1, W>), dim3(grid), dim3(FftCfg<LG1>::NT * W), 0, s, a, p.log2m2, (const V2 *)p.p1.tw);
}

}  // namespace

// The split per size ("Long partitions"): M1 one of 16, 64, 256 -- the column sizes whose passes are all radix 4
// / 8 / 16 with nothing left over -- and M2 = M / M1 the largest of 1024, 2048, 4096 that gives.
#define BIG_FOR_LOG2M1(F) F(4) F(6) F(8)
#define BIG_FOR_LOG2M2(F) F(10) F(11) F(12)
bool big_split(int filter_length, int realsize, int *log2m1, int *log2m2)
{
    int lg = 0;
    while ((1L << lg) < filter_length) lg++;
    if ((1L << lg) != filter_length || lg > 20 || lg < (realsize == 8 ? 14 : 15)) return false;
    const int l1 = lg <= 16 ? 4 : lg <= 18 ? 6 : 8;
    *log2m1 = l1; *log2m2 = lg - l1;
    return true;
}

int big_plan_create(BigPlan *plan, int filter_length, int realsize)
{
    int l1, l2;
    if ((realsize != 4 && realsize != 8) || !big_split(filter_length, realsize, &l1, &l2)) return -1;
    *plan = BigPlan();
    plan->log2m = l1 + l2; plan->log2m1 = l1; plan->log2m2 = l2; plan->realsize = realsize;
    if (fft_plan_create(&plan->p1, 1 << l1, realsize) != 0 || fft_plan_create(&plan->p2, 1 << l2, realsize) != 0) {
        big_plan_destroy(plan);
        return -2;
    }
    const long M = 1L << plan->log2m, N = 2 * M;
    const int n_lo = 1 << BIG_LO_BITS, n_hi = (int)(M >> BIG_LO_BITS);
    std::vector<long double> thi, tlo, shi, slo;
    big_fill(thi, n_hi, BIG_LO_BITS, M); big_fill(tlo, n_lo, 0, M);
    big_fill(shi, n_hi, BIG_LO_BITS, N); big_fill(slo, n_lo, 0, N);
    if (realsize == 4) {
        plan->t_hi = big_upload<float>(thi); plan->t_lo = big_upload<float>(tlo);
        plan->s_hi = big_upload<float>(shi); plan->s_lo = big_upload<float>(slo);
    } else {
        plan->t_hi = big_upload<double>(thi); plan->t_lo = big_upload<double>(tlo);
        plan->s_hi = big_upload<double>(shi); plan->s_lo = big_upload<double>(slo);
    }
    if (!plan->t_hi || !plan->t_lo || !plan->s_hi || !plan->s_lo) { big_plan_destroy(plan); return -2; }
    return 0;
}

void big_plan_destroy(BigPlan *plan)
{
    fft_plan_destroy(&plan->p1);
    fft_plan_destroy(&plan->p2);
    void **tabs[] = {&plan->t_hi, &plan->t_lo, &plan->s_hi, &plan->s_lo};
    for (void **t : tabs) { if (*t) (void)hipFree(*t); *t = nullptr; }
}

// Every grid of a launch of n_t blocks x n_ch channels is a 32-bit count (the column passes have the most workgroups)
bool big_launch_fits(const BigPlan &plan, int n_t, int n_ch)
{
    const long tiles = (1L << plan.log2m2) / (128 / (2 * plan.realsize));
    return n_t > 0 && n_ch > 0 && (long)n_t * n_ch * tiles < (1L << 31);
}

void launch_fwd_big(const BigPlan &plan, const FwdArgs &a, hipStream_t s)
{
    if (a.n_t <= 0 || a.n_ch <= 0) return;
    if (a.raw_bytes != 0 || !big_launch_fits(plan, a.n_t, a.n_ch)) {
        fprintf(stderr, "bfir: launch_fwd_big takes the planar form and 32-bit grids only: launch skipped\n");
        return;
    }
    switch (plan.log2m1) {
#define F(lg) case lg: if (plan.realsize == 4) fwd_cols_t<float, lg>(plan, a, s); else fwd_cols_t<double, lg>(plan, a, s); break;
        BIG_FOR_LOG2M1(F)
#undef F
    }
    switch (plan.log2m2) {
#define F(lg) case lg: if (plan.realsize == 4) fwd_rows_t<float, lg>(plan, a, s); else fwd_rows_t<double, lg>(plan, a, s); break;
        BIG_FOR_LOG2M2(F)
#undef F
    }
}

void launch_inv_big(const BigPlan &plan, const InvArgs &a, hipStream_t s)
{
    if (a.n_t <= 0 || a.n_ch <= 0) return;
    if (a.raw_bytes != 0 || a.full_output != 0 || !big_launch_fits(plan, a.n_t, a.n_ch)) {
        fprintf(stderr, "bfir: launch_inv_big takes the planar form and 32-bit grids only: launch skipped\n");
        return;
    }
    switch (plan.log2m2) {
#define F(lg) case lg: if (plan.realsize == 4) inv_rows_t<float, lg>(plan, a, s); else inv_rows_t<double, lg>(plan, a, s); break;
        BIG_FOR_LOG2M2(F)
#undef F
    }
    switch (plan.log2m1) {
#define F(lg) case lg: if (plan.realsize == 4) inv_cols_t<float, lg>(plan, a, s); else inv_cols_t<double, lg>(plan, a, s); break;
        BIG_FOR_LOG2M1(F)
#undef F
    }
}

}  // namespace bfir
