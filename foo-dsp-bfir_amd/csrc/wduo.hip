// wduo.hip -- k_wduo: the partition sums of a level of a multi-level mimo engine (bfir_engine_create_mimo_levels: up to 64
// inputs -> 64 outputs) under the TWO filter sets of a crossfaded coefficient change, in one pass over the delay line, for
// the launches that need both sets (bfir_engine_set_coeff_matrix_levels_fade: the head while it fades, a tail level up to
// its last old block).
//
//     Y [o][t](k) = sum_{i < n_in} sum_{p < nblk [o][i]} X[i][slot(t - p)](k) H [o][i][p](k)        (the old set)
//     Y2[o][t](k) = sum_{i < n_in} sum_{p < nblk2[o][i]} X[i][slot(t - p)](k) H2[o][i][p](k)        (the new set)
//
// It is to k_mac_duo (mfade.hip) what k_mac_mimo (mimo.hip) is to k_mac_matrix.  The sums are k_mac_duo's, lane for lane
// (duo_lane, mat_ops.h): one fma chain per (set, output, bin, block) -- inputs in index order, partitions in order, the four
// fmas of mat_cmac per term, a (set, output, input) with count 0 skipped, the DC | Nyquist select in the wave that holds bin
// 0 -- and every (set, output, bin, block) stored exactly once, an output without any filter as zeros.  That chain is
// k_mac_mimo's as well, so Y and Y2 are bit for bit what two launch_mac_mimo calls write (old set, new set): that is this
// kernel's specification.  What differs from k_mac_duo:
//   counts   both tables live in HBM, [o n_in + i], and are read with wave-uniform (scalar) loads;
//   grid     k_mac_mimo's: a workgroup is ONE wave over 64 bins, grid x holds every (bin tile, output tile, time tile), bin
//            tile major and time tile fastest, through xcd_work_item.  The workgroups an XCD runs at one time are consecutive
//            time tiles of one (bin tile, output tile) and share the slice of H AND H2 that tile reads,
//                2 sets x NO outputs x n_in x B x 64 bins x 2 reals    (fp32, NO = 2: 2 MiB at 64 inputs and B = 16)
//            which is k_mac_mimo's slice at its NO = 4 and one set, out of the XCD's 4 MiB L2.
// Offsets into X, H, H2, Y and Y2 are 64-bit; the grid is the only limit (wduo_supported).
#include "kernels.h"

#include <climits>

#include "fft_lds.h"
#include "mat_ops.h"

namespace bfir {

constexpr int kWduoBins = 64;   // bins per workgroup: one wave

template <typename T, bool ILV, int NO, int TT>
__global__ __launch_bounds__(kWduoBins, 4) void k_wduo(WduoArgs d, int n_ot, int nTT)
{
    const int w = xcd_work_item(blockIdx.x, gridDim.x);
    const int g = w / nTT, tt = w - g * nTT;                     // (bin tile, output tile), time tile
    const int bt = g / n_ot, ot = g - bt * n_ot;
    const int k = bt * kWduoBins + threadIdx.x;                  // bin
    if (k >= d.a.N / 2) return;
    duo_lane<T, ILV, NO, TT>(d, k, bt == 0, ot * NO, tt * TT);
}

// The register tile is k_mac_duo's: both sets' accumulators are 4 NO TT registers, 64 at the widest (fp32 2 x 8), inside the
// 128 registers of four waves per SIMD.  NO = 2 from two outputs on (fp32), 1 (fp64); TT = 1 on the latency path (launches
// of up to BFIR_MAT_SMALL_MAX blocks), else 8 (fp32) or 4 (fp64).  NO = 2 with two sets is also what keeps the slice of
// filters an XCD's resident workgroups share at k_mac_mimo's size (above).
static int wduo_no(const MimoArgs &a) { return a.realsize == 4 && a.n_out >= 2 ? 2 : 1; }
static int wduo_tt(const MimoArgs &a) { return a.n_t <= BFIR_MAT_SMALL_MAX ? 1 : (a.realsize == 4 ? 8 : 4); }

// workgroups of the launch: (bin tiles, output tiles, time tiles)
static void wduo_grid(const MimoArgs &a, int no, int tt, long &nbt, long &n_ot, long &nTT)
{
    nbt = (a.N / 2 + kWduoBins - 1) / kWduoBins; n_ot = (a.n_out + no - 1) / no; nTT = ((long)a.n_t + tt - 1) / tt;
}

bool wduo_supported(const WduoArgs &d)
{
    const MimoArgs &a = d.a;
    if (a.n_in < 1 || a.n_in > BFIR_MIMO_MAX || a.n_out < 1 || a.n_out > BFIR_MIMO_MAX || a.n_t < 0) return false;
    if (a.N < 2 || (a.realsize != 4 && a.realsize != 8)) return false;
    long nbt, n_ot, nTT;
    wduo_grid(a, wduo_no(a), wduo_tt(a), nbt, n_ot, nTT);
    return nbt * n_ot * nTT <= INT_MAX / kWduoBins;             // workgroup ids in int, threads per dimension in 32 bits
}

template <typename T, bool ILV, int NO> static void launch_wduo_t(const WduoArgs &d, int tt, hipStream_t s)
{
    long nbt, n_ot, nTT;
    wduo_grid(d.a, NO, tt, nbt, n_ot, nTT);
    const dim3 grid((unsigned)(nbt * n_ot * nTT)), block(kWduoBins);
    if (tt == 1) {
        hipLaunchKernelGGL((k_wduo<T, ILV, NO, 1>), grid, block, 0, s, d, (int)n_ot, (int)nTT);
    } else {
        constexpr int TTB = sizeof(T) == 4 ? 8 : 4;
        hipLaunchKernelGGL((k_wduo<T, ILV, NO, TTB>), grid, block, 0, s, d, (int)n_ot, (int)nTT);
    }
}

int launch_wduo(const WduoArgs &d, hipStream_t s)
{
    if (!wduo_supported(d)) return -1;
    const MimoArgs &a = d.a;
    if (a.n_t == 0) return 0;
    const int no = wduo_no(a), tt = wduo_tt(a);
    if (a.realsize == 4) {
        if (a.interleaved) { if (no == 2) launch_wduo_t<float, true, 2>(d, tt, s); else launch_wduo_t<float, true, 1>(d, tt, s); }
        else { if (no == 2) launch_wduo_t<float, false, 2>(d, tt, s); else launch_wduo_t<float, false, 1>(d, tt, s); }
    } else {
        if (a.interleaved) launch_wduo_t<double, true, 1>(d, tt, s);
        else launch_wduo_t<double, false, 1>(d, tt, s);
    }
    return 0;
}

}  // namespace bfir
