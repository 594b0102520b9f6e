// resample.hip -- sampling-rate conversion of a whole impulse response: what buffer::resample_snd_file (brutefir/
// buffer.cpp:225-330) hands to libsamplerate, here band-limited interpolation on an exact rational grid.
//   bfir_resample_filter   the K taps of one of the p phases: a Kaiser-windowed sinc, host arithmetic in long double
//   k_resample             the polyphase FIR over interleaved frames: a tile of output frames per workgroup, the source span
//                          of one channel at a time staged in LDS in working precision (the structure of k_delay_sub)
//   bfir_resampler_*       the phase table resident on the device, runs from host or device buffers
// With g = gcd(in_rate, out_rate), p = out_rate / g and q = in_rate / g, output frame m sits at input time m q / p =
// n0 + phase / p, n0 = (m q) div p, phase = (m q) mod p in 64-bit integers: exactly p phases, no table interpolation and no
// accumulated time error.  rho = min(1, p / q) cutoff, W = Z / rho, Wc = ceil(W), K = 2 Wc; tap j of a phase meets input
// frame n0 - Wc + 1 + j and, with u = phase / p + Wc - 1 - j, is gain rho sinc(pi rho u) I0(beta sqrt(1 - (u / W)^2)) /
// I0(beta) for |u| < W, else 0 -- the window once, not twice as firwindow_kaiser applies it to the delay filters.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/bfir_hip.h"
#include "kernels.h"

namespace bfir {

// Output frames per workgroup, one lane per frame: the largest of kResTile, kResTile / 2, ... 1 whose LDS request -- the
// tile's output frames, then the source span of one channel, ceil(tile q / p) + K samples -- fits kResLds, the 64 KiB a
// launch may ask for without setting an attribute.  At the largest K (4096) and q / p (2048) a tile of 1 asks for 48 KiB.
constexpr int kResTile = 256;
constexpr int kResLds = 65536;
constexpr int kResMaxTaps = 4096;        // K
constexpr long kResMaxTable = 1L << 22;  // p K

struct ResampleArgs {
    void *dst; const void *src; const void *tab;   // tab: [K][p] in working precision, tap-major
    long n_in, n_out;                              // frames of src; frames of dst to write
    long p, q;
    int C, K, Wc, tile, width;
};

__host__ __device__ __forceinline__ size_t resample_out_bytes(int tile, int C, int sample_bytes)
{
    return ((size_t)tile * C * sample_bytes + 15) & ~(size_t)15;
}

// R: working precision, F: frame sample type.
template <typename R, typename F>
__global__ __launch_bounds__(kResTile) void k_resample(ResampleArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    F *out = (F *)smem;
    R *span = (R *)(smem + resample_out_bytes(a.tile, a.C, (int)sizeof(F)));
    const int tid = threadIdx.x;
    const long m0 = (long)xcd_work_item((int)blockIdx.x, (int)gridDim.x) * a.tile;   // an XCD walks one range of frames
    const long first = m0 * a.q / a.p;            // n0 of the tile's first frame
    const long base = first - a.Wc + 1;           // the source frame span[0] holds
    const long m = m0 + tid;
    const bool live = tid < a.tile && m < a.n_out;
    const long mq = m * a.q, n0 = mq / a.p;
    const R *t = (const R *)a.tab + (mq - n0 * a.p);   // this frame's phase: tap j at t[j p]
    const R *u = span + (live ? (int)(n0 - first) : 0);
    const F *src = (const F *)a.src;
    for (int c = 0; c < a.C; c++) {
        if (c) __syncthreads();
        for (int i = tid; i < a.width; i += kResTile) {
            const long n = base + i;
            span[i] = n >= 0 && n < a.n_in ? (R)src[n * a.C + c] : (R)0;
        }
        __syncthreads();
        if (live) {
            R acc = (R)0;
            for (int j = 0; j < a.K; j++) acc = fma(t[(size_t)j * a.p], u[j], acc);
            out[tid * a.C + c] = (F)acc;
        }
    }
    __syncthreads();
    // the tile's frames as whole 16-byte stores where the destination allows them
    const long left = a.n_out - m0;
    const size_t bytes = (size_t)(left < a.tile ? left : a.tile) * a.C * sizeof(F);
    unsigned char *dst = (unsigned char *)a.dst + (size_t)m0 * a.C * sizeof(F);
    if ((((uintptr_t)dst | bytes) & 15) == 0) {
        for (size_t i = (size_t)tid * 16; i < bytes; i += (size_t)kResTile * 16) *(uint4 *)(dst + i) = *(const uint4 *)(smem + i);
    } else {
        for (size_t i = tid; i < bytes / sizeof(F); i += kResTile) ((F *)dst)[i] = out[i];
    }
}

static long resample_width(int tile, long p, long q, int K) { return ((long)tile * q + p - 1) / p + K; }

static int resample_tile(long p, long q, int K, int C, int realsize)
{
    int tile = kResTile;
    while (tile > 1 && resample_out_bytes(tile, C, realsize) + (size_t)resample_width(tile, p, q, K) * realsize > (size_t)kResLds)
        tile >>= 1;
    return tile;
}

// 0, or BFIR_ERR_UNSUPPORTED where the grid does not fit (nothing launched)
static int launch_resample(ResampleArgs a, int realsize, hipStream_t s)
{
    if (a.n_out <= 0) return BFIR_OK;
    a.tile = resample_tile(a.p, a.q, a.K, a.C, realsize);
    a.width = (int)resample_width(a.tile, a.p, a.q, a.K);
    const long groups = (a.n_out + a.tile - 1) / a.tile;
    if (groups > 0x7fffffffL) return BFIR_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)groups), block(kResTile);
    const size_t lds = resample_out_bytes(a.tile, a.C, realsize) + (size_t)a.width * realsize;
    if (realsize == 4) hipLaunchKernelGGL((k_resample<float, float>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((k_resample<double, double>), grid, block, lds, s, a);
    return hipGetLastError() == hipSuccess ? BFIR_OK : BFIR_ERR_HIP;
}

}  // namespace bfir

// ---------------------------------------------------------------------------
// The phase table: host arithmetic in long double, each tap rounded once to the working precision.
// ---------------------------------------------------------------------------
namespace {

struct ResampleGeom {
    long p, q;
    int K, Wc;
    long double rho, W, beta, gain, inv_i0_beta;
};

// I_0(x) = sum over n of ((x / 2)^n / n!)^2, summed until a term no longer changes the sum.  (The delay filters' kaiser_i0
// in delay.hip runs the reference's own loop in double, to underflow; in long double that loop is some 1500 terms long.)
long double resample_i0(long double x)
{
    const long double half = x / 2.0L;
    long double sum = 1.0L, term = 1.0L, n = 1.0L;
    for (;;) {
        term *= half;
        term /= n;
        const long double next = sum + term * term;
        if (next == sum || !std::isfinite(next)) return next;
        sum = next;
        n += 1.0L;
    }
}

long gcd_l(long a, long b) { while (b) { const long t = a % b; a = b; b = t; } return a; }

// BFIR_OK, BFIR_ERR_ARG for anything out of range, BFIR_ERR_UNSUPPORTED for a table past the limits
int resample_geom(int in_rate, int out_rate, int zero_crossings, double kaiser_beta, double cutoff, double gain, int realsize,
                  ResampleGeom *g)
{
    if (in_rate < 1 || out_rate < 1 || zero_crossings < 1 || zero_crossings > 128 || (realsize != 4 && realsize != 8))
        return BFIR_ERR_ARG;
    if (!(kaiser_beta >= 0.0) || !std::isfinite(kaiser_beta) || !(cutoff >= 0.5 && cutoff <= 1.0) || !std::isfinite(gain))
        return BFIR_ERR_ARG;
    const long d = gcd_l(in_rate, out_rate);
    g->p = out_rate / d;
    g->q = in_rate / d;
    g->rho = (g->p < g->q ? (long double)g->p / (long double)g->q : 1.0L) * (long double)cutoff;
    g->W = (long double)zero_crossings / g->rho;
    // Wc = ceil(W) in exact integers, so that K does not hang on a rounding where W is whole (1 -> 3 at cutoff 1: W = 3 Z):
    // cutoff = M 2^(ex - 53) with M a 53-bit integer, W = Z q' 2^(53 - ex) / (p' M), (p', q') = (p, q) when p < q, else (1, 1)
    int ex = 0;
    const unsigned __int128 M = (unsigned __int128)std::ldexp(std::frexp(cutoff, &ex), 53);
    const unsigned __int128 num = ((unsigned __int128)zero_crossings * (unsigned __int128)(g->p < g->q ? g->q : 1)) << (53 - ex);
    const unsigned __int128 den = (unsigned __int128)(g->p < g->q ? g->p : 1) * M;
    const unsigned __int128 wc = (num + den - 1) / den;
    if (wc > (unsigned __int128)(bfir::kResMaxTaps / 2)) return BFIR_ERR_UNSUPPORTED;
    g->Wc = (int)wc;
    g->K = 2 * g->Wc;
    if (g->p * g->K > bfir::kResMaxTable) return BFIR_ERR_UNSUPPORTED;
    g->beta = (long double)kaiser_beta;
    g->gain = (long double)gain;
    g->inv_i0_beta = 1.0L / resample_i0(g->beta);
    return BFIR_OK;
}

long double resample_tap(const ResampleGeom &g, long phase, int j)
{
    // u = phase / p + Wc - 1 - j from one exact integer numerator
    const long double u = (long double)((long)(g.Wc - 1 - j) * g.p + phase) / (long double)g.p;
    if (!(std::fabs(u) < g.W)) return 0.0L;
    const long double x = 3.141592653589793238462643383279502884L * g.rho * u;
    const long double sinc = x == 0.0L ? 1.0L : std::sin(x) / x;
    const long double r = u / g.W;
    return g.gain * g.rho * sinc * resample_i0(g.beta * std::sqrt(1.0L - r * r)) * g.inv_i0_beta;
}

template <typename R> void resample_phase(const ResampleGeom &g, long phase, R *taps, long stride)
{
    for (int j = 0; j < g.K; j++) taps[(size_t)j * stride] = (R)resample_tap(g, phase, j);
}

}  // namespace

extern "C" int bfir_resample_filter(int in_rate, int out_rate, int zero_crossings, double kaiser_beta, double cutoff, double gain,
                                    int realsize, int phase, void *taps, int *n_taps)
{
    ResampleGeom g;
    const int rc = resample_geom(in_rate, out_rate, zero_crossings, kaiser_beta, cutoff, gain, realsize, &g);
    if (rc != BFIR_OK) return rc;
    if (phase < 0 || phase >= g.p || (!taps && !n_taps)) return BFIR_ERR_ARG;
    if (n_taps) *n_taps = g.K;
    if (!taps) return BFIR_OK;
    if (realsize == 4) resample_phase(g, phase, (float *)taps, 1);
    else resample_phase(g, phase, (double *)taps, 1);
    return BFIR_OK;
}

struct bfir_resampler {
    int device = 0, realsize = 4, C = 1;
    ResampleGeom g;
    void *d_tab = nullptr;
    void *d_in = nullptr, *d_out = nullptr;   // staging for bfir_resampler_run, grown on demand
    size_t cap_in = 0, cap_out = 0;
};

extern "C" bfir_resampler *bfir_resampler_create(int in_rate, int out_rate, int zero_crossings, double kaiser_beta, double cutoff,
                                                 double gain, int realsize, int channels, int device, int *err)
{
    int dummy;
    if (!err) err = &dummy;
    ResampleGeom g;
    *err = resample_geom(in_rate, out_rate, zero_crossings, kaiser_beta, cutoff, gain, realsize, &g);
    if (*err == BFIR_OK && (channels < 1 || channels > BFIR_MAXCHANNELS)) *err = BFIR_ERR_ARG;
    if (*err != BFIR_OK) return nullptr;
    const int ndev = bfir_device_count();
    if (ndev <= 0) { *err = BFIR_ERR_NO_DEVICE; return nullptr; }
    if (device < 0 || device >= ndev) { *err = BFIR_ERR_ARG; return nullptr; }
    if (hipSetDevice(device) != hipSuccess) { *err = BFIR_ERR_HIP; return nullptr; }
    bfir_resampler *r = new bfir_resampler();
    r->device = device; r->realsize = realsize; r->C = channels; r->g = g;
    if (g.p != g.q) {   // equal rates copy bytes: no table
        const size_t n = (size_t)g.p * g.K;
        std::vector<unsigned char> tab(n * realsize);
        for (long ph = 0; ph < g.p; ph++) {
            if (realsize == 4) resample_phase(g, ph, (float *)tab.data() + ph, g.p);
            else resample_phase(g, ph, (double *)tab.data() + ph, g.p);
        }
        if (hipMalloc(&r->d_tab, tab.size()) != hipSuccess ||
            hipMemcpy(r->d_tab, tab.data(), tab.size(), hipMemcpyHostToDevice) != hipSuccess) {
            if (r->d_tab) (void)hipFree(r->d_tab);
            delete r;
            *err = BFIR_ERR_HIP;
            return nullptr;
        }
    }
    return r;
}

extern "C" void bfir_resampler_destroy(bfir_resampler *r)
{
    if (!r) return;
    (void)hipSetDevice(r->device);
    (void)hipDeviceSynchronize();
    if (r->d_tab) (void)hipFree(r->d_tab);
    if (r->d_in) (void)hipFree(r->d_in);
    if (r->d_out) (void)hipFree(r->d_out);
    delete r;
}

extern "C" int64_t bfir_resampler_out_frames(const bfir_resampler *r, int64_t n_in)
{
    if (!r || n_in < 0) return BFIR_ERR_ARG;
    const unsigned __int128 n = ((unsigned __int128)n_in * (unsigned __int128)r->g.p + (unsigned __int128)(r->g.q - 1)) / (unsigned __int128)r->g.q;
    return n > (unsigned __int128)INT64_MAX ? (int64_t)BFIR_ERR_ARG : (int64_t)n;
}

extern "C" int64_t bfir_resampler_run_device(bfir_resampler *r, const void *d_in, int64_t n_in, void *d_out, int64_t max_out)
{
    if (!r || n_in < 0 || max_out < 0 || (n_in > 0 && !d_in)) return BFIR_ERR_ARG;
    int64_t n = bfir_resampler_out_frames(r, n_in);
    if (n < 0) return n;
    if (n > max_out) n = max_out;
    if (n == 0) return 0;
    if (!d_out) return BFIR_ERR_ARG;
    if (hipSetDevice(r->device) != hipSuccess) return BFIR_ERR_HIP;
    if (r->g.p == r->g.q) {   // the bytes, NaNs included
        if (hipMemcpyAsync(d_out, d_in, (size_t)n * r->C * r->realsize, hipMemcpyDeviceToDevice, nullptr) != hipSuccess)
            return BFIR_ERR_HIP;
        return n;
    }
    bfir::ResampleArgs a;
    a.dst = d_out; a.src = d_in; a.tab = r->d_tab;
    a.n_in = n_in; a.n_out = n;
    a.p = r->g.p; a.q = r->g.q;
    a.C = r->C; a.K = r->g.K; a.Wc = r->g.Wc; a.tile = 0; a.width = 0;
    const int rc = bfir::launch_resample(a, r->realsize, nullptr);
    return rc == BFIR_OK ? n : (int64_t)rc;
}

static bool resample_grow(void **buf, size_t *cap, size_t bytes)
{
    if (bytes <= *cap) return true;
    if (*buf) (void)hipFree(*buf);
    *buf = nullptr; *cap = 0;
    if (hipMalloc(buf, bytes) != hipSuccess) { *buf = nullptr; return false; }
    *cap = bytes;
    return true;
}

extern "C" int64_t bfir_resampler_run(bfir_resampler *r, const void *in, int64_t n_in, void *out, int64_t max_out)
{
    if (!r || n_in < 0 || max_out < 0 || (n_in > 0 && !in)) return BFIR_ERR_ARG;
    int64_t n = bfir_resampler_out_frames(r, n_in);
    if (n < 0) return n;
    if (n > max_out) n = max_out;
    if (n == 0) return 0;
    if (!out) return BFIR_ERR_ARG;
    if (hipSetDevice(r->device) != hipSuccess) return BFIR_ERR_HIP;
    const size_t frame = (size_t)r->C * r->realsize;
    if (!resample_grow(&r->d_in, &r->cap_in, (size_t)n_in * frame) || !resample_grow(&r->d_out, &r->cap_out, (size_t)n * frame))
        return BFIR_ERR_HIP;
    if (hipMemcpy(r->d_in, in, (size_t)n_in * frame, hipMemcpyHostToDevice) != hipSuccess) return BFIR_ERR_HIP;
    const int64_t got = bfir_resampler_run_device(r, r->d_in, n_in, r->d_out, n);
    if (got < 0) return got;
    if (hipMemcpy(out, r->d_out, (size_t)got * frame, hipMemcpyDeviceToHost) != hipSuccess) return BFIR_ERR_HIP;
    return got;
}
