// patch.hip -- k_patch_pairs: the new set's product spectra of a crossfaded coefficient change that replaces a LIST of
// (output, input) pairs of a matrix or mimo engine (bfir_engine_set_coeff_matrix_pairs_fade), from the old set's:
//
//     Y2[o][t](k) = Y[o][t](k) + sum_{listed (o, i)} ( sum_{p < nb_new} X[i][slot(t - p)](k) H2[o][i][p](k)
//                                                    - sum_{p < nb_old} X[i][slot(t - p)](k) H [o][i][p](k) )
//
// It runs behind the old set's MAC of a fading chunk (k_mac_matrix or k_mac_mimo, unchanged) on the same stream, in place of
// that MAC's second run over the whole matrix: one moving source is one column, 64 filters out of 4096.
//
// One lane owns one bin, ONE output row and a tile of TT consecutive blocks (mat_lane's shape with NO = 1, mat_ops.h).  It
// loads Y[o][t] of its tile into its accumulators, walks the row's listed pairs in input order, and per pair continues the
// ONE fma chain per (output, bin, block) with the four fmas of mat_cmac per term:
//     first  the new filter's partitions p = 0 .. nb_new - 1 in order, with H2[o][i][p],
//     then   the old filter's partitions p = 0 .. nb_old - 1 in order, with -H[o][i][p] (the loaded value negated: exact).
// Then it stores the tile into Y2[o][t].  A row without listed pairs is copied: the fade's back end reads Y2 for every
// output.  A pass with no partitions (an added path's old filter, a removed path's new one) loads nothing, and a listed pair
// without a filter in either set loads nothing at all: nothing is ever multiplied by zero, so a NaN in an input no filter
// reads reaches no output.  Bin 0 (DC | Nyquist, two real sums) is carried by the wave that holds it, as mat_cmac<DCNY>.
// The chain of an (output, bin, block) does not depend on TT: the one-block form (launches of up to BFIR_MAT_SMALL_MAX
// blocks) and the tiled form give the same bits.
//
// The listed pairs come as a table in HBM (PatchArgs.row, .ent), written by the call while the device is idle and read with
// wave-uniform loads.  The grid is k_mac_mimo's: workgroups of one wave over 64 bins, every (bin tile, output, time tile) in
// grid x, time tiles fastest, XCD-aware.  Offsets into X, H, Y are 64-bit; the grid is the only limit (patch_supported).
#include "kernels.h"

#include <climits>

#include "fft_lds.h"
#include "mat_ops.h"

namespace bfir {

constexpr int kPatchBins = 64;   // bins per workgroup: one wave; the lane's walk: patch_pass, patch_row (mat_ops.h)

template <typename T, bool ILV, int TT>
__global__ __launch_bounds__(kPatchBins, 4) void k_patch_pairs(PatchArgs a, int nTT)
{
    const int w = xcd_work_item(blockIdx.x, gridDim.x);
    const int g = w / nTT, tt = w - g * nTT;                     // (bin tile, output), time tile
    const int bt = g / a.n_out, o = g - bt * a.n_out;
    const int k = bt * kPatchBins + threadIdx.x;                 // bin
    if (k >= a.N / 2) return;
    const int t0 = tt * TT;
    const int ore = ILV ? 2 * k : 8 * (k >> 2) + (k & 3), oim = ILV ? ore + 1 : ore + 4;
    const T *__restrict__ Y = (const T *)a.y + (long)o * a.y_ch_stride;
    T *__restrict__ Y2 = (T *)a.y2 + (long)o * a.y2_ch_stride;
    T ar[TT], ai[TT];
#pragma unroll
    for (int j = 0; j < TT; j++) {
        ar[j] = (T)0; ai[j] = (T)0;
        if (t0 + j < a.n_t) mat_ld<T, ILV>(Y + (long)(t0 + j) * a.N, ore, oim, ar[j], ai[j]);
    }
    if (bt == 0) patch_row<T, ILV, TT, true>(a, o, t0, ore, oim, k == 0, ar, ai);
    else patch_row<T, ILV, TT, false>(a, o, t0, ore, oim, false, ar, ai);
#pragma unroll
    for (int j = 0; j < TT; j++) {
        if (t0 + j < a.n_t) {
            T *yo = Y2 + (long)(t0 + j) * a.N;
            if constexpr (ILV) {
                using V2 = typename Vec2<T>::type;
                V2 v; v.x = ar[j]; v.y = ai[j];
                *(V2 *)(yo + ore) = v;
            } else {
                yo[ore] = ar[j]; yo[oim] = ai[j];
            }
        }
    }
}

// time tile: 1 on the latency path (launches of up to BFIR_MAT_SMALL_MAX blocks), else 8 (fp32) / 4 (fp64) -- 16 accumulator
// registers and as many for the window; fp64 with 8 passes the 128 registers of four waves per SIMD and spills
static int patch_tt(int realsize) { return realsize == 4 ? 8 : 4; }
static long patch_groups(const PatchArgs &a)
{
    const long tt = a.n_t <= BFIR_MAT_SMALL_MAX ? 1 : patch_tt(a.realsize);
    const long nbt = (a.N / 2 + kPatchBins - 1) / kPatchBins, nTT = ((long)a.n_t + tt - 1) / tt;
    return nbt * a.n_out * nTT;
}

bool patch_supported(const PatchArgs &a)
{
    if (a.n_in < 1 || a.n_in > BFIR_MIMO_MAX || a.n_out < 1 || a.n_out > BFIR_MIMO_MAX || a.n_t < 0) return false;
    if (a.N < 2 || (a.realsize != 4 && a.realsize != 8)) return false;
    return patch_groups(a) <= INT_MAX / kPatchBins;             // workgroup ids in int, threads per dimension in 32 bits
}

template <typename T, bool ILV> static void launch_patch_t(const PatchArgs &a, hipStream_t s)
{
    const dim3 grid((unsigned)patch_groups(a)), block(kPatchBins);
    if (a.n_t <= BFIR_MAT_SMALL_MAX) hipLaunchKernelGGL((k_patch_pairs<T, ILV, 1>), grid, block, 0, s, a, a.n_t);
    else {
        constexpr int TTB = sizeof(T) == 4 ? 8 : 4;             // patch_tt
        hipLaunchKernelGGL((k_patch_pairs<T, ILV, TTB>), grid, block, 0, s, a, (a.n_t + TTB - 1) / TTB);
    }
}

int launch_patch(const PatchArgs &a, hipStream_t s)
{
    if (!patch_supported(a)) return -1;
    if (a.n_t == 0) return 0;
    if (a.realsize == 4) {
        if (a.interleaved) launch_patch_t<float, true>(a, s);
        else launch_patch_t<float, false>(a, s);
    } else {
        if (a.interleaved) launch_patch_t<double, true>(a, s);
        else launch_patch_t<double, false>(a, s);
    }
    return 0;
}

}  // namespace bfir
