// matrix.hip -- k_mac_matrix: the partition sums of a matrix engine (n_in inputs -> n_out outputs, one filter per pair).
//
//     Y[o][t](k) = sum_{i < n_in} sum_{p < nblk[o][i]} X[i][slot(t - p)](k) H[o][i][p](k)
//
// per bin k, inputs in index order, partitions p = 0 .. nb - 1 within an input: ONE fma chain per (output, bin, block) with
// the four fmas of k_mac_small / cmac4 per term.  With a single filter in an output's row the chain is the diagonal MAC's,
// bit for bit.  A pair with nblk = 0 (a NULL filter) is skipped, never multiplied by zero: a NaN in an input no filter reads
// reaches no output.
//
// One lane owns one bin, a tile of TT consecutive output blocks and the accumulators of NO outputs (2 NO TT registers): the
// lane's body is mat_tile / mat_lane in mat_ops.h, which k_mac_mimo (mimo.hip) instantiates too.  Per input it walks the
// partitions in order with a window of TT delay-line spectra in registers, X[t0 + j - p] for j < TT: step p loads ONE new spectrum (X[t0 - p], in place of the one nobody needs any more) and the NO filter spectra H[o][i][p], then
// does NO x TT complex MACs -- every X load feeds NO TT of them, every H load TT.  Operands are fetched one step ahead.
// Bin 0 (DC | Nyquist: two independent real sums) is carried by the wave that holds it (DCNY), with a select per term.
// Every (output, bin, block) of the launch is stored exactly once, outputs without any filter as zeros: Y needs no clearing.
// Offsets into X, H and Y are 64-bit; the grid is the only limit (mac_matrix_supported).
#include "kernels.h"

#include <algorithm>
#include <climits>

#include "fft_lds.h"
#include "mat_ops.h"

namespace bfir {

// grid: x = (bin tile, time tile), XCD-aware as k_mac (each XCD a contiguous range, bin tile major, so its L2 holds the
// slice of H and X of its bins); y = output tile of NO outputs
template <typename T, bool ILV, int NO, int TT>
__global__ __launch_bounds__(256, 4) void k_mac_matrix(MatArgs a, int nbt, int nTT)
{
    const int w = xcd_work_item(blockIdx.x, gridDim.x);
    const int bt = w / nTT, tt = w - bt * nTT;
    const int k = bt * blockDim.x + threadIdx.x;                 // bin
    const int N2 = a.N / 2;
    if (k >= N2) return;
    const bool wave0 = __builtin_amdgcn_readfirstlane((int)(bt == 0 && threadIdx.x < 64)) != 0;
    mat_lane<T, ILV, NO, TT>(a, k, wave0, blockIdx.y * NO, tt * TT);
}

// Output tile NO: the output count rounded up to a power of two, at most 4 (fp32) / 2 (fp64), more outputs in several tiles
// (grid y); time tile TT: 1 for the latency path (a handful of blocks), else 8 (fp32; fp64 one output) or 4 (fp64): 64
// accumulator registers.  Larger tiles (fp32 8 x 4, fp64 4 x 4) pass the 128 registers of four waves per SIMD and spill.
static int mat_no(const MatArgs &a) { const int cap = a.realsize == 4 ? 4 : 2; int no = 1; while (no < a.n_out && no < cap) no *= 2; return no; }
static int mat_tt(const MatArgs &a, int no)
{
    if (a.n_t <= BFIR_MAT_SMALL_MAX) return 1;
    return a.realsize == 4 ? 8 : (no == 1 ? 8 : 4);
}

bool mac_matrix_supported(const MatArgs &a)
{
    if (a.n_in < 1 || a.n_in > BFIR_MAT_MAX || a.n_out < 1 || a.n_out > BFIR_MAT_MAX || a.n_t < 0) return false;
    if (a.N < 2 || (a.realsize != 4 && a.realsize != 8)) return false;
    const int no = mat_no(a), tt = mat_tt(a, no);
    const long threads = std::min(256, std::max(64, a.N / 2));   // as launch_mac_matrix_t
    const long nbt = (a.N / 2 + threads - 1) / threads, nTT = ((long)a.n_t + tt - 1) / tt;
    return nbt * nTT <= INT_MAX && nbt * nTT * threads <= (long)UINT32_MAX;   // workgroup ids in int, threads per dimension
}

template <typename T, bool ILV, int NO> static void launch_mac_matrix_t(const MatArgs &a, int tt, hipStream_t s)
{
    const int threads = std::min(256, std::max(64, a.N / 2));
    const int nbt = (a.N / 2 + threads - 1) / threads;
    const int n_ot = (a.n_out + NO - 1) / NO;
    if (tt == 1) {
        hipLaunchKernelGGL((k_mac_matrix<T, ILV, NO, 1>), dim3(nbt * a.n_t, n_ot), dim3(threads), 0, s, a, nbt, a.n_t);
    } else {
        constexpr int TTB = sizeof(T) == 4 ? 8 : (NO == 1 ? 8 : 4);
        const int nTT = (a.n_t + TTB - 1) / TTB;
        hipLaunchKernelGGL((k_mac_matrix<T, ILV, NO, TTB>), dim3(nbt * nTT, n_ot), dim3(threads), 0, s, a, nbt, nTT);
    }
}

template <typename T, bool ILV> static void launch_mac_matrix_l(const MatArgs &a, int no, int tt, hipStream_t s)
{
    switch (no) {
    case 1: launch_mac_matrix_t<T, ILV, 1>(a, tt, s); break;
    case 2: launch_mac_matrix_t<T, ILV, 2>(a, tt, s); break;
    default:
        if constexpr (sizeof(T) == 4) launch_mac_matrix_t<T, ILV, 4>(a, tt, s);
        break;
    }
}

int launch_mac_matrix(const MatArgs &a, hipStream_t s)
{
    if (!mac_matrix_supported(a)) return -1;
    if (a.n_t == 0) return 0;
    const int no = mat_no(a), tt = mat_tt(a, no);
    if (a.realsize == 4) {
        if (a.interleaved) launch_mac_matrix_l<float, true>(a, no, tt, s);
        else launch_mac_matrix_l<float, false>(a, no, tt, s);
    } else {
        if (a.interleaved) launch_mac_matrix_l<double, true>(a, no, tt, s);
        else launch_mac_matrix_l<double, false>(a, no, tt, s);
    }
    return 0;
}

}  // namespace bfir
