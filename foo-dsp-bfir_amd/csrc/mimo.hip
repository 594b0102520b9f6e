// mimo.hip -- k_mac_mimo: the partition sums of a mimo engine (bfir_engine_create_mimo: up to 64 inputs -> 64 outputs).
//
//     Y[o][t](k) = sum_{i < n_in} sum_{p < nblk[o][i]} X[i][slot(t - p)](k) H[o][i][p](k)
//
// The sums are k_mac_matrix's, lane for lane (mat_lane, mat_ops.h): one lane owns one bin, a tile of TT consecutive output
// blocks and the accumulators of NO outputs; inputs in index order, partitions in order, the four fmas of mat_cmac per term,
// a pair with nblk = 0 skipped.  So wherever both kernels can run the bits are the same, and a block of filters on the
// diagonal gives the bits of a matrix engine on that block's channels.  What a wide matrix changes is the traffic: H is
// [n_out][n_in][B][N], 128 MiB at 32 -> 32, B = 16, L = 1024, and a lane's arithmetic per byte of H is TT complex MACs, no
// more.  Two things differ from k_mac_matrix:
//   counts   nblk is a table in HBM, [o n_in + i], read with wave-uniform (scalar) loads: 4096 ints do not travel by value;
//   grid     a workgroup is ONE wave over 64 bins, and grid x holds every (bin tile, output tile, time tile), bin tile major
//            and time tile fastest, XCD-aware (xcd_work_item: each XCD one contiguous range).  The workgroups an XCD runs at
//            one time are then consecutive time tiles of one (bin tile, output tile) -- or of a few, when the launch has
//            fewer time tiles than the XCD has wave slots -- and read the same slice of H,
//                NO outputs x n_in x B x 64 bins x 2 reals    (fp32, NO = 4: 2 MiB at 64 inputs and B = 16, 1 MiB at 32)
//            out of that XCD's 4 MiB L2; the output tiles of a bin tile follow each other on the same XCD, so the delay
//            line of those bins is fetched by one XCD only.  Where the slices in flight pass the L2 (many partitions, few
//            blocks per launch) the launch is as correct and H comes from the Infinity Cache or HBM once per workgroup.
// Offsets into X, H and Y are 64-bit; the grid is the only limit (mac_mimo_supported).
#include "kernels.h"

#include <climits>

#include "fft_lds.h"
#include "mat_ops.h"

namespace bfir {

template <typename T, bool ILV, int NO, int TT>
__global__ __launch_bounds__(kMimoBins, 4) void k_mac_mimo(MimoArgs a, int n_ot, int nTT)
{
    const int w = xcd_work_item(blockIdx.x, gridDim.x);
    const int g = w / nTT, tt = w - g * nTT;                     // (bin tile, output tile), time tile
    const int bt = g / n_ot, ot = g - bt * n_ot;
    const int k = bt * kMimoBins + threadIdx.x;                  // bin
    if (k >= a.N / 2) return;
    mat_lane<T, ILV, NO, TT>(a, k, bt == 0, ot * NO, tt * TT);
}

// the register tile and the grid: mimo_no, mimo_tt, mimo_grid (mat_ops.h; k_wpatch, wpatch.hip, runs on them too)
bool mac_mimo_supported(const MimoArgs &a)
{
    if (a.n_in < 1 || a.n_in > BFIR_MIMO_MAX || a.n_out < 1 || a.n_out > BFIR_MIMO_MAX || a.n_t < 0) return false;
    if (a.N < 2 || (a.realsize != 4 && a.realsize != 8)) return false;
    const int no = mimo_no(a);
    long nbt, n_ot, nTT;
    mimo_grid(a, no, mimo_tt(a, no), nbt, n_ot, nTT);
    return nbt * n_ot * nTT <= INT_MAX / kMimoBins;             // workgroup ids in int, threads per dimension in 32 bits
}

template <typename T, bool ILV, int NO> static void launch_mac_mimo_t(const MimoArgs &a, int tt, hipStream_t s)
{
    long nbt, n_ot, nTT;
    mimo_grid(a, NO, tt, nbt, n_ot, nTT);
    const dim3 grid((unsigned)(nbt * n_ot * nTT)), block(kMimoBins);
    if (tt == 1) {
        hipLaunchKernelGGL((k_mac_mimo<T, ILV, NO, 1>), grid, block, 0, s, a, (int)n_ot, (int)nTT);
    } else {
        constexpr int TTB = sizeof(T) == 4 ? 8 : (NO == 1 ? 8 : 4);
        hipLaunchKernelGGL((k_mac_mimo<T, ILV, NO, TTB>), grid, block, 0, s, a, (int)n_ot, (int)nTT);
    }
}

template <typename T, bool ILV> static void launch_mac_mimo_l(const MimoArgs &a, int no, int tt, hipStream_t s)
{
    switch (no) {
    case 1: launch_mac_mimo_t<T, ILV, 1>(a, tt, s); break;
    case 2: launch_mac_mimo_t<T, ILV, 2>(a, tt, s); break;
    default:
        if constexpr (sizeof(T) == 4) launch_mac_mimo_t<T, ILV, 4>(a, tt, s);
        break;
    }
}

int launch_mac_mimo(const MimoArgs &a, hipStream_t s)
{
    if (!mac_mimo_supported(a)) return -1;
    if (a.n_t == 0) return 0;
    const int no = mimo_no(a), tt = mimo_tt(a, no);
    if (a.realsize == 4) {
        if (a.interleaved) launch_mac_mimo_l<float, true>(a, no, tt, s);
        else launch_mac_mimo_l<float, false>(a, no, tt, s);
    } else {
        if (a.interleaved) launch_mac_mimo_l<double, true>(a, no, tt, s);
        else launch_mac_mimo_l<double, false>(a, no, tt, s);
    }
    return 0;
}

}  // namespace bfir
