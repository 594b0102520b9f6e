// delay.hip -- per-channel delays on an engine's input and output frames: the reference's delay class
// (brutefir/delay.cpp, firwindow.c) as two kernels and one host routine.
//   bfir_subdelay_filter   delay::sample_sinc + firwindow_kaiser (delay.cpp:278-306, firwindow.c:89-210), host arithmetic
//   k_delay_copy           whole-sample delays on raw frames of any sample size (delay.cpp:552-600 shifts bytes the same
//                          way), and the history update: the last H frames of `hist || piece`
//   k_delay_sub            the sub-sample stage: a 2 h + 1 tap FIR per channel in working precision, the source span
//                          staged in LDS (the reference runs it as a one-block FFT convolution, delay.cpp:148-180)
// The engine wiring (history buffers, the device table, where the launches go) is in engine.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/bfir_hip.h"
#include "kernels.h"

namespace bfir {

// 16 bytes of units of type T, stored by one lane
template <typename T> struct alignas(16) Pack16 { T v[16 / sizeof(T)]; };

// One lane writes V consecutive units (T: the sample type, or bytes for 3-byte samples and unaligned buffers) of dst.
// Unit u lies in frame u / (C ups), channel (u / ups) % C; its source is the same unit of source frame m0 + frame - d_ch.
// Workgroup `block` of the job's n_blocks takes the work item xcd_work_item gives it: an XCD walks one contiguous range of
// frames in order, so the frames its channels read at their different delays meet in that XCD's L2.
template <typename T, bool VEC>
__device__ __forceinline__ void delay_copy_job(const DelayCopyArgs &a, int block, int n_blocks, int ups)
{
    constexpr int V = VEC ? (int)(16 / sizeof(T)) : 1;
    const int upf = a.C * ups;   // units per frame
    const long n_units = a.n_frames * upf;
    const long u0 = ((long)xcd_work_item(block, n_blocks) * 256 + threadIdx.x) * V;
    if (u0 >= n_units) return;
    long frame = u0 / upf;
    const int r = (int)(u0 - frame * upf);
    int ch = r / ups, q = r - ch * ups;
    const T *piece = (const T *)a.piece, *hist = (const T *)a.hist;
    Pack16<T> p;
#pragma unroll
    for (int i = 0; i < V; i++) {
        T v = 0;
        if (u0 + i < n_units) {
            const long m = a.m0 + frame - (a.tab ? (long)a.tab->delay[ch] : 0L);
            v = m >= 0 ? piece[m * upf + ch * ups + q] : hist[(a.H + m) * upf + ch * ups + q];
        }
        p.v[i] = v;
        if (++q == ups) { q = 0; if (++ch == a.C) { ch = 0; frame++; } }
    }
    T *dst = (T *)a.dst + u0;
    if (VEC && u0 + V <= n_units) *(Pack16<T> *)dst = p;
    else {
#pragma unroll
        for (int i = 0; i < V; i++) if (u0 + i < n_units) dst[i] = p.v[i];
    }
}

// workgroups [0, ga) run job a, the rest job b
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_delay_copy(DelayCopyArgs a, DelayCopyArgs b, int ga, int ups)
{
    if ((int)blockIdx.x < ga) delay_copy_job<T, VEC>(a, (int)blockIdx.x, ga, ups);
    else delay_copy_job<T, VEC>(b, (int)blockIdx.x - ga, (int)gridDim.x - ga, ups);
}

template <typename T> static void delay_copy_t(const DelayCopyArgs &a, const DelayCopyArgs &b, int ups, bool vec, hipStream_t s)
{
    const long per = (vec ? (long)(16 / sizeof(T)) : 1) * 256;   // units per workgroup
    const int ga = (int)((a.n_frames * a.C * ups + per - 1) / per), gb = (int)((b.n_frames * b.C * ups + per - 1) / per);
    if (ga + gb <= 0) return;
    const dim3 grid((unsigned)(ga + gb)), block(256);
    if (vec) hipLaunchKernelGGL((k_delay_copy<T, true>), grid, block, 0, s, a, b, ga, ups);
    else hipLaunchKernelGGL((k_delay_copy<T, false>), grid, block, 0, s, a, b, ga, ups);
}

void launch_delay_copy(const DelayCopyArgs &a, const DelayCopyArgs *b, hipStream_t s)
{
    DelayCopyArgs none = a;
    none.n_frames = 0;   // no second job: no workgroups for it
    const DelayCopyArgs &b2 = b ? *b : none;
    const uintptr_t all = (uintptr_t)a.dst | (uintptr_t)a.piece | (uintptr_t)a.hist | (uintptr_t)b2.dst | (uintptr_t)b2.piece | (uintptr_t)b2.hist;
    const int sb = a.sample_bytes;
    const bool vec = (((uintptr_t)a.dst | (uintptr_t)b2.dst) & 15) == 0;   // whole 16-byte stores; a buffer's tail is stored unit by unit
    // the unit is the sample where every buffer is aligned to it, else the byte (3-byte samples always)
    if (sb == 8 && (all & 7) == 0) delay_copy_t<uint64_t>(a, b2, 1, vec, s);
    else if (sb == 4 && (all & 3) == 0) delay_copy_t<uint32_t>(a, b2, 1, vec, s);
    else if (sb == 2 && (all & 1) == 0) delay_copy_t<uint16_t>(a, b2, 1, vec, s);
    else delay_copy_t<uint8_t>(a, b2, sb, vec, s);
}

// Frames per workgroup of the sub-sample kernel: one lane per frame.
constexpr int kSubTile = 256;

template <typename F> __device__ __forceinline__ F delay_src(const DelaySubArgs &a, long m, int c)
{
    return m >= 0 ? ((const F *)a.piece)[m * a.C + c] : ((const F *)a.hist)[(a.H + m) * a.C + c];
}

// R: working precision, F: frame sample type.  LDS: the tile's output frames (F, interleaved), then per channel the
// kSubTile + 2 h source samples the tile's taps reach, widened to R on load.
template <typename R, typename F>
__global__ __launch_bounds__(kSubTile) void k_delay_sub(DelaySubArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    F *out = (F *)smem;
    R *span = (R *)(smem + (size_t)kSubTile * BFIR_DELAY_CH * sizeof(F));
    const int tid = threadIdx.x, h2 = 2 * a.h, width = kSubTile + h2;
    const long t0 = (long)xcd_work_item((int)blockIdx.x, (int)gridDim.x) * kSubTile;   // an XCD walks one range of frames (k_delay_copy)
    for (int c = 0; c < a.C; c++) {
        if (!a.tab->sub[c]) continue;
        const long d = a.tab->delay[c];
        for (int i = tid; i < width; i += kSubTile) {
            const long m = t0 + i - h2 - d;
            span[c * width + i] = m < a.n_frames ? (R)delay_src<F>(a, m, c) : (R)0;
        }
    }
    __syncthreads();
    const long t = t0 + tid;
    if (t < a.n_frames) {
        const int n_taps = h2 + 1;
        for (int c = 0; c < a.C; c++) {
            if (!a.tab->sub[c]) {   // no arithmetic: the sample's bytes, shifted by d + h
                out[tid * a.C + c] = delay_src<F>(a, t - a.tab->delay[c] - a.h, c);
                continue;
            }
            const R *f = (const R *)a.taps + (size_t)c * n_taps;
            const R *u = span + c * width + tid + h2;
            R acc = (R)0;
            for (int k = 0; k < n_taps; k++) acc = fma(f[k], u[-k], acc);
            out[tid * a.C + c] = (F)acc;
        }
    }
    __syncthreads();
    // the tile's frames as whole 16-byte stores where the destination allows them
    const long left = a.n_frames - t0;
    const size_t bytes = (size_t)(left < kSubTile ? left : kSubTile) * a.C * sizeof(F);
    unsigned char *dst = (unsigned char *)a.dst + (size_t)t0 * a.C * sizeof(F);
    if ((((uintptr_t)dst | bytes) & 15) == 0) {
        for (size_t i = (size_t)tid * 16; i < bytes; i += (size_t)kSubTile * 16) *(uint4 *)(dst + i) = *(const uint4 *)(smem + i);
    } else {
        for (size_t i = tid; i < bytes / sizeof(F); i += kSubTile) ((F *)dst)[i] = out[i];
    }
}

void launch_delay_sub(const DelaySubArgs &a, hipStream_t s)
{
    if (a.n_frames <= 0) return;
    const dim3 grid((unsigned)((a.n_frames + kSubTile - 1) / kSubTile)), block(kSubTile);
    const size_t lds = (size_t)kSubTile * BFIR_DELAY_CH * a.sample_bytes + (size_t)a.C * (kSubTile + 2 * a.h) * a.realsize;
    if (a.realsize == 4 && a.sample_bytes == 4) hipLaunchKernelGGL((k_delay_sub<float, float>), grid, block, lds, s, a);
    else if (a.realsize == 4) hipLaunchKernelGGL((k_delay_sub<float, double>), grid, block, lds, s, a);
    else if (a.sample_bytes == 4) hipLaunchKernelGGL((k_delay_sub<double, float>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((k_delay_sub<double, double>), grid, block, lds, s, a);
}

}  // namespace bfir

// ---------------------------------------------------------------------------
// The filters of the sub-sample stage: host arithmetic in double, the operations of delay::sample_sinc and
// firwindow_kaiser in their order, so that the taps are the reference's.
// ---------------------------------------------------------------------------
// I_0, the series of firwindow.c:15-52: term_n = term_(n-1) * (x / 2) / n, summed as squares until the term underflows
static double kaiser_i0(double x)
{
    const double half = x / 2.0;
    double sum = 1.0, term = 1.0, n = 1.0;
    do {
        term *= half;
        term /= n;
        sum += term * term;
        n += 1.0;
    } while (term != 0.0 && std::isfinite(sum));
    return sum;
}

// the window at x in [-1, 1] (firwindow.c:54-87; a rounding error past the ends is clamped)
static double kaiser_at(double x, double beta, double inv_i0_beta)
{
    if (x < -1.0) x = -1.0;
    if (x > 1.0) x = 1.0;
    return kaiser_i0(beta * std::sqrt(1.0 - x * x)) * inv_i0_beta;
}

template <typename R> static void subdelay_taps(int h, double offset, double beta, R *taps)
{
    const int len = 2 * h + 1;
    for (int n = 0; n < len; n++) {   // delay.cpp:290-302
        const double x = M_PI * ((double)(n - h) - offset);
        taps[n] = (R)(x == 0.0 ? 1.0 : std::sin(x) / x);
    }
    // firwindow_kaiser with a non-zero offset (firwindow.c:102-161).  |offset| < 1 and it is not 0, so its fraction is not
    // 0 either and the window's peak lies between taps `rise` and `rise + 1`: a rising and a falling half, each with its
    // own step.  Every tap is multiplied by its weight twice, as the reference does (:129-130, :153-158).
    const double fl = std::floor(offset);
    const int rise = h + (int)fl;
    const double frac = offset - fl;
    const double inv = 1.0 / kaiser_i0(beta);
    double step = 1.0 / ((double)rise + frac);
    int n = 0;
    for (; n <= rise; n++) {
        const double y = kaiser_at(-1.0 + (double)n * step, beta, inv);
        taps[n] *= y;
        taps[n] *= y;
    }
    step = 1.0 / ((double)(len - rise - 1) - frac);
    for (; n < len; n++) {
        const double y = kaiser_at(((double)(n - rise) - frac) * step, beta, inv);
        taps[n] *= y;
        taps[n] *= y;
    }
}

extern "C" int bfir_subdelay_filter(int half_filter_length, int subdelay, int step_count, double kaiser_beta, int realsize,
                                    void *taps)
{
    const int h = half_filter_length;
    if (!taps || step_count < 2 || h < 1 || h > 128 || (realsize != 4 && realsize != 8)) return BFIR_ERR_ARG;
    if (subdelay <= -step_count || subdelay >= step_count) return BFIR_ERR_ARG;
    if (subdelay == 0) {   // delay.cpp:229-240: a unit tap, no window
        for (int n = 0; n <= 2 * h; n++) {
            if (realsize == 4) ((float *)taps)[n] = n == h ? 1.f : 0.f;
            else ((double *)taps)[n] = n == h ? 1.0 : 0.0;
        }
        return BFIR_OK;
    }
    const double offset = (double)subdelay / step_count;   // delay.cpp:246, :255
    if (realsize == 4) subdelay_taps(h, offset, kaiser_beta, (float *)taps);
    else subdelay_taps(h, offset, kaiser_beta, (double *)taps);
    return BFIR_OK;
}
