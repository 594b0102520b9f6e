// mfade.hip -- k_mac_duo: the partition sums of a matrix engine under TWO filter sets in one pass over the delay line, for
// the chunks of a crossfaded coefficient change on a multi-level matrix engine that need both sets
// (bfir_engine_set_coeff_matrix_levels_fade: the head while it fades, a tail level up to its last old block).
//
//     Y [o][t](k) = sum_{i < n_in} sum_{p < nblk [o][i]} X[i][slot(t - p)](k) H [o][i][p](k)        (the old set)
//     Y2[o][t](k) = sum_{i < n_in} sum_{p < nblk2[o][i]} X[i][slot(t - p)](k) H2[o][i][p](k)        (the new set)
//
// Every (set, output, bin, block) has exactly k_mac_matrix's chain (matrix.hip): inputs in index order, partitions in order
// within an input, the four fmas of mat_cmac per term, the DC | Nyquist select in the wave that holds bin 0.  So Y and Y2
// are bit for bit what two launches of k_mac_matrix write; that is this kernel's specification.  A (set, output, input)
// with partition count 0 -- a NULL filter, or one that does not reach this level in that set -- is skipped, never
// multiplied by zero.
//
// It is mat_tile's loop with two H pointer sets and two count tables (duo_tile, duo_lane in mat_ops.h, shared with k_wduo): one lane owns one bin, a tile of TT consecutive blocks
// and the accumulators of NO outputs under both sets (4 NO TT registers).  Per input the window of TT delay-line spectra is
// set up ONCE and step p loads ONE new spectrum for both sets (two launches of k_mac_matrix do each twice); the step loop
// runs to the larger of the two sets' maxima and every (set, output) is guarded by its own wave-uniform p < nb.  Each
// (set, output, bin, block) is stored exactly once, outputs without any filter as zeros.  Offsets are 64-bit.
#include "kernels.h"

#include <algorithm>
#include <climits>

#include "fft_lds.h"
#include "mat_ops.h"

namespace bfir {

// grid: as k_mac_matrix -- x = (bin tile, time tile) through the XCD remap, y = output tile of NO outputs
template <typename T, bool ILV, int NO, int TT>
__global__ __launch_bounds__(256, 4) void k_mac_duo(MatDuoArgs d, int nbt, int nTT)
{
    const MatArgs &a = d.a;
    const int w = xcd_work_item(blockIdx.x, gridDim.x);
    const int bt = w / nTT, tt = w - bt * nTT;
    const int k = bt * blockDim.x + threadIdx.x;                 // bin
    const int N2 = a.N / 2;
    if (k >= N2) return;
    const int t0 = tt * TT, o0 = blockIdx.y * NO;
    const bool wave0 = __builtin_amdgcn_readfirstlane((int)(bt == 0 && threadIdx.x < 64)) != 0;
    duo_lane<T, ILV, NO, TT>(d, k, wave0, o0, t0);
}

// Output tile NO: 2 from two outputs on (fp32), 1 (fp64), more outputs in grid y; time tile TT: 1 for the latency path (up to
// BFIR_MAT_SMALL_MAX blocks), else 8 (fp32) or 4 (fp64).  Both sets' accumulators are 4 NO TT registers: 64 at the widest
// (fp32 2 x 8), the count of k_mac_matrix's widest tiles, inside the 128 registers of four waves per SIMD.
static int duo_no(const MatArgs &a) { return a.realsize == 4 && a.n_out >= 2 ? 2 : 1; }
static int duo_tt(const MatArgs &a) { return a.n_t <= BFIR_MAT_SMALL_MAX ? 1 : (a.realsize == 4 ? 8 : 4); }

bool mac_duo_supported(const MatDuoArgs &d)
{
    const MatArgs &a = d.a;
    if (a.n_in < 1 || a.n_in > BFIR_MAT_MAX || a.n_out < 1 || a.n_out > BFIR_MAT_MAX || a.n_t < 0) return false;
    if (a.N < 2 || (a.realsize != 4 && a.realsize != 8)) return false;
    const int tt = duo_tt(a);
    const long threads = std::min(256, std::max(64, a.N / 2));   // as launch_mac_duo_t
    const long nbt = (a.N / 2 + threads - 1) / threads, nTT = ((long)a.n_t + tt - 1) / tt;
    return nbt * nTT <= INT_MAX && nbt * nTT * threads <= (long)UINT32_MAX;   // workgroup ids in int, threads per dimension
}

template <typename T, bool ILV, int NO> static void launch_mac_duo_t(const MatDuoArgs &d, int tt, hipStream_t s)
{
    const MatArgs &a = d.a;
    const int threads = std::min(256, std::max(64, a.N / 2));
    const int nbt = (a.N / 2 + threads - 1) / threads;
    const int n_ot = (a.n_out + NO - 1) / NO;
    if (tt == 1) {
        hipLaunchKernelGGL((k_mac_duo<T, ILV, NO, 1>), dim3(nbt * a.n_t, n_ot), dim3(threads), 0, s, d, nbt, a.n_t);
    } else {
        constexpr int TTB = sizeof(T) == 4 ? 8 : 4;
        const int nTT = (a.n_t + TTB - 1) / TTB;
        hipLaunchKernelGGL((k_mac_duo<T, ILV, NO, TTB>), dim3(nbt * nTT, n_ot), dim3(threads), 0, s, d, nbt, nTT);
    }
}

int launch_mac_duo(const MatDuoArgs &d, hipStream_t s)
{
    if (!mac_duo_supported(d)) return -1;
    const MatArgs &a = d.a;
    if (a.n_t == 0) return 0;
    const int no = duo_no(a), tt = duo_tt(a);
    if (a.realsize == 4) {
        if (a.interleaved) { if (no == 2) launch_mac_duo_t<float, true, 2>(d, tt, s); else launch_mac_duo_t<float, true, 1>(d, tt, s); }
        else { if (no == 2) launch_mac_duo_t<float, false, 2>(d, tt, s); else launch_mac_duo_t<float, false, 1>(d, tt, s); }
    } else {
        if (a.interleaved) launch_mac_duo_t<double, true, 1>(d, tt, s);
        else launch_mac_duo_t<double, false, 1>(d, tt, s);
    }
    return 0;
}

}  // namespace bfir
