// wpatch.hip -- k_wpatch: the old set's partition sums of a level of a multi-level mimo engine AND the new set's, as the old
// ones plus the listed pairs' difference, in one launch -- for the launches that need both sets while a pair list fades
// (bfir_engine_set_coeff_matrix_levels_pairs_fade: the head while it fades, a tail level up to its last old block).
//
//     Y [o][t](k) = sum_{i < n_in} sum_{p < nblk[o][i]} X[i][slot(t - p)](k) H[o][i][p](k)                  (k_mac_mimo)
//     Y2[o][t](k) = Y[o][t](k) + sum_{listed (o, i)} ( sum_{p < nb_new} X[i][slot(t - p)](k) H2[o][i][p](k)
//                                                    - sum_{p < nb_old} X[i][slot(t - p)](k) H [o][i][p](k) )  (k_patch_pairs)
//
// It is to launch_mac_mimo followed by launch_patch what k_wduo (wduo.hip) is to two launches of k_mac_mimo.  A lane owns
// one bin, a tile of TT blocks and NO outputs, on k_mac_mimo's grid (mimo_no, mimo_tt, mimo_grid: mat_ops.h).  It runs
// mat_tile into its accumulators -- k_mac_mimo's chain -- and stores Y.  Then, for each of its NO outputs in turn, it
// continues that output's accumulators through the row's listed pairs (patch_row, the body k_patch_pairs runs after
// loading the same values back from Y), and stores Y2: Y never makes the round trip through memory, and the second launch
// is saved.  The chain of an (output, bin, block) depends neither on NO nor on TT, so Y and Y2 are bit for bit what the two
// launches write (launch_mac_mimo(d.a), launch_patch(wpatch_patch_args(d))): that is this kernel's specification, and
// tests/test_lpairs_gpu.py holds it to that (BFIR_PATCH_FUSED=0|1).
// A row without listed pairs stores its Y twice.
// Behind BFIR_PATCH_FUSED=1, default 0: at 64 -> 64 the two launches measured faster in every run ("Pair lists on
// multi-level engines") -- the lane walks the listed pairs of its NO outputs one after the other, where k_patch_pairs gives
// every output a lane of its own.
// Offsets into X, H, H2, Y and Y2 are 64-bit; the grid is the only limit (wpatch_supported).
#include "kernels.h"

#include <climits>

#include "fft_lds.h"
#include "mat_ops.h"

namespace bfir {

// every (output, block) of the lane's tile, exactly once
template <typename T, bool ILV, int NO, int TT>
__device__ __forceinline__ void wpatch_store(void *y, long ch_stride, int n_out, int n_t, int N, int o0, int t0, int ore, int oim,
                                             const T (&ar)[NO][TT], const T (&ai)[NO][TT])
{
#pragma unroll
    for (int o = 0; o < NO; o++) {
        if (o0 + o >= n_out) break;
        T *__restrict__ Y = (T *)y + (long)(o0 + o) * ch_stride;
#pragma unroll
        for (int j = 0; j < TT; j++) {
            if (t0 + j < n_t) {
                T *yo = Y + (long)(t0 + j) * N;
                if constexpr (ILV) {
                    using V2 = typename Vec2<T>::type;
                    V2 v; v.x = ar[o][j]; v.y = ai[o][j];
                    *(V2 *)(yo + ore) = v;
                } else {
                    yo[ore] = ar[o][j]; yo[oim] = ai[o][j];
                }
            }
        }
    }
}

template <typename T, bool ILV, int NO, int TT, bool DCNY>
__device__ __forceinline__ void wpatch_lane(const WpatchArgs &d, int o0, int t0, int ore, int oim, bool k0)
{
    const MimoArgs &a = d.a;
    const PatchArgs p = wpatch_patch_args(d);
    T ar[NO][TT], ai[NO][TT];
#pragma unroll
    for (int o = 0; o < NO; o++)
#pragma unroll
        for (int j = 0; j < TT; j++) { ar[o][j] = (T)0; ai[o][j] = (T)0; }
    mat_tile<T, ILV, NO, TT, DCNY>(a, o0, t0, ore, oim, k0, ar, ai);
    wpatch_store<T, ILV, NO, TT>(a.y, a.y_ch_stride, a.n_out, a.n_t, a.N, o0, t0, ore, oim, ar, ai);
#pragma unroll
    for (int o = 0; o < NO; o++)
        if (o0 + o < a.n_out) patch_row<T, ILV, TT, DCNY>(p, o0 + o, t0, ore, oim, k0, ar[o], ai[o]);
    wpatch_store<T, ILV, NO, TT>(p.y2, p.y2_ch_stride, a.n_out, a.n_t, a.N, o0, t0, ore, oim, ar, ai);
}

template <typename T, bool ILV, int NO, int TT>
__global__ __launch_bounds__(kMimoBins, 4) void k_wpatch(WpatchArgs d, int n_ot, int nTT)
{
    const int w = xcd_work_item(blockIdx.x, gridDim.x);
    const int g = w / nTT, tt = w - g * nTT;                     // (bin tile, output tile), time tile
    const int bt = g / n_ot, ot = g - bt * n_ot;
    const int k = bt * kMimoBins + threadIdx.x;                  // bin
    if (k >= d.a.N / 2) return;
    const int ore = ILV ? 2 * k : 8 * (k >> 2) + (k & 3), oim = ILV ? ore + 1 : ore + 4;
    if (bt == 0) wpatch_lane<T, ILV, NO, TT, true>(d, ot * NO, tt * TT, ore, oim, k == 0);
    else wpatch_lane<T, ILV, NO, TT, false>(d, ot * NO, tt * TT, ore, oim, false);
}

// k_mac_mimo's tile but for ONE instance: fp32 in the grouped layout (N < 512) with four outputs takes TT = 4 where
// k_mac_mimo takes 8.  With 8 it is the one instance that spills: 7 SGPRs at 118 VGPRs (behind the 64 accumulator registers
// the patch keeps a window of its own, and the grouped layout two addresses per bin).  fp64 with one output fits at TT = 8
// (123 / 128 VGPRs).  The bits do not depend on TT.  DESIGN.md, "Pair lists on multi-level engines", has the table.
static int wpatch_tt(const MimoArgs &a, int no)
{
    const int tt = mimo_tt(a, no);
    return tt > 4 && a.realsize == 4 && !a.interleaved && no == 4 ? 4 : tt;
}

bool wpatch_supported(const WpatchArgs &d)
{
    const MimoArgs &a = d.a;
    if (!mac_mimo_supported(a)) return false;
    const int no = mimo_no(a);
    long nbt, n_ot, nTT;
    mimo_grid(a, no, wpatch_tt(a, no), nbt, n_ot, nTT);
    return nbt * n_ot * nTT <= INT_MAX / kMimoBins;             // workgroup ids in int, threads per dimension in 32 bits
}

template <typename T, bool ILV, int NO> static void launch_wpatch_t(const WpatchArgs &d, int tt, hipStream_t s)
{
    long nbt, n_ot, nTT;
    mimo_grid(d.a, NO, tt, nbt, n_ot, nTT);
    const dim3 grid((unsigned)(nbt * n_ot * nTT)), block(kMimoBins);
    if (tt == 1) {
        hipLaunchKernelGGL((k_wpatch<T, ILV, NO, 1>), grid, block, 0, s, d, (int)n_ot, (int)nTT);
    } else {
        constexpr int TTB = sizeof(T) == 4 ? (!ILV && NO == 4 ? 4 : 8) : (NO == 1 ? 8 : 4);   // wpatch_tt
        hipLaunchKernelGGL((k_wpatch<T, ILV, NO, TTB>), grid, block, 0, s, d, (int)n_ot, (int)nTT);
    }
}

template <typename T, bool ILV> static void launch_wpatch_l(const WpatchArgs &d, int no, int tt, hipStream_t s)
{
    switch (no) {
    case 1: launch_wpatch_t<T, ILV, 1>(d, tt, s); break;
    case 2: launch_wpatch_t<T, ILV, 2>(d, tt, s); break;
    default:
        if constexpr (sizeof(T) == 4) launch_wpatch_t<T, ILV, 4>(d, tt, s);
        break;
    }
}

int launch_wpatch(const WpatchArgs &d, hipStream_t s)
{
    if (!wpatch_supported(d)) return -1;
    const MimoArgs &a = d.a;
    if (a.n_t == 0) return 0;
    const int no = mimo_no(a), tt = wpatch_tt(a, no);
    if (a.realsize == 4) {
        if (a.interleaved) launch_wpatch_l<float, true>(d, no, tt, s);
        else launch_wpatch_l<float, false>(d, no, tt, s);
    } else {
        if (a.interleaved) launch_wpatch_l<double, true>(d, no, tt, s);
        else launch_wpatch_l<double, false>(d, no, tt, s);
    }
    return 0;
}

}  // namespace bfir
