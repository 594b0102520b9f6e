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
// It is mat_tile's loop with two H pointer sets and two count tables: one lane owns one bin, a tile of TT consecutive blocks
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

namespace {

template <typename T, bool ILV, int NO, int TT, bool DCNY>
__device__ __forceinline__ void duo_tile(const MatDuoArgs &d, int o0, int t0, int ore, int oim, bool k0,
                                         T (&ar)[2][NO][TT], T (&ai)[2][NO][TT])
{
    const MatArgs &a = d.a;
    const long N = a.N;
    const int ring = a.ring;
    const int sl = (a.base_slot + t0) % ring;                    // delay-line slot of block t0
    for (int i = 0; i < a.n_in; i++) {
        int nb[2][NO], nbm = 0, sm = 0, om = 0;
#pragma unroll
        for (int s = 0; s < 2; s++)
#pragma unroll
            for (int o = 0; o < NO; o++) {
                nb[s][o] = o0 + o < a.n_out ? (s ? d.nblk2 : a.nblk)[(o0 + o) * a.n_in + i] : 0;
                if (nb[s][o] > nbm) { nbm = nb[s][o]; sm = s; om = o; }
            }
        if (nbm == 0) continue;                                  // no filter of this tile reads input i under either set
        const T *__restrict__ Xi = (const T *)a.x + (long)i * a.x_ch_stride;
        // filter spectra of (set, o, i); one without a filter is pointed at the one with nbm partitions (loaded, never used)
        const T *__restrict__ Hp[2][NO];
#pragma unroll
        for (int s = 0; s < 2; s++)
#pragma unroll
            for (int o = 0; o < NO; o++) {
                const bool own = nb[s][o] > 0;
                const T *base = (const T *)((own ? s : sm) ? d.h2 : a.h);
                Hp[s][o] = base + ((long)(o0 + (own ? o : om)) * a.n_in + i) * a.h_pair_stride;
            }
        // the window of mat_tile: slot (j - p) mod TT holds X[t0 + j - p]; blocks t0 + j >= n_t only reach accumulators that
        // are never stored
        T wr[TT], wi[TT];
#pragma unroll
        for (int j = 0; j < TT; j++) {
            int sj = sl + j; if (sj >= ring) sj -= ring;
            mat_ld<T, ILV>(Xi + (long)sj * N, ore, oim, wr[j], wi[j]);
        }
        T qxr = (T)0, qxi = (T)0, qhr[2][NO], qhi[2][NO];        // operands of the next step (step 0 takes no new X)
#pragma unroll
        for (int s = 0; s < 2; s++)
#pragma unroll
            for (int o = 0; o < NO; o++) mat_ld<T, ILV>(Hp[s][o], ore, oim, qhr[s][o], qhi[s][o]);
        for (int p0 = 0; p0 < nbm; p0 += TT) {
#pragma unroll
            for (int ii = 0; ii < TT; ii++) {
                const int p = p0 + ii;
                if (p < nbm) {                                   // wave-uniform
                    if (p > 0) { wr[(TT - ii) % TT] = qxr; wi[(TT - ii) % TT] = qxi; }
                    // prefetch step p + 1 (clamped to the last step: in range, not used)
                    const int pn = p + 1 < nbm ? p + 1 : p;
                    int sn = sl - pn; if (sn < 0) sn += ring;       // X[t0 - pn] enters the window at step pn
                    mat_ld<T, ILV>(Xi + (long)sn * N, ore, oim, qxr, qxi);
#pragma unroll
                    for (int s = 0; s < 2; s++)
#pragma unroll
                        for (int o = 0; o < NO; o++) {
                            if (p < nb[s][o]) {                  // wave-uniform: a (set, pair) without this partition is skipped
#pragma unroll
                                for (int j = 0; j < TT; j++) {
                                    const int idx = (j - ii + TT) % TT;
                                    mat_cmac<DCNY>(ar[s][o][j], ai[s][o][j], wr[idx], wi[idx], qhr[s][o], qhi[s][o], k0);
                                }
                            }
                            const int po = pn < nb[s][o] ? pn : (nb[s][o] > 0 ? nb[s][o] - 1 : pn);
                            mat_ld<T, ILV>(Hp[s][o] + (long)po * N, ore, oim, qhr[s][o], qhi[s][o]);
                        }
                }
            }
        }
    }
}

}  // namespace

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
    const int ore = ILV ? 2 * k : 8 * (k >> 2) + (k & 3), oim = ILV ? ore + 1 : ore + 4;
    T ar[2][NO][TT], ai[2][NO][TT];
#pragma unroll
    for (int s = 0; s < 2; s++)
#pragma unroll
        for (int o = 0; o < NO; o++)
#pragma unroll
            for (int j = 0; j < TT; j++) { ar[s][o][j] = (T)0; ai[s][o][j] = (T)0; }
    const bool wave0 = __builtin_amdgcn_readfirstlane((int)(bt == 0 && threadIdx.x < 64)) != 0;
    if (wave0) duo_tile<T, ILV, NO, TT, true>(d, o0, t0, ore, oim, k == 0, ar, ai);
    else duo_tile<T, ILV, NO, TT, false>(d, o0, t0, ore, oim, false, ar, ai);
#pragma unroll
    for (int s = 0; s < 2; s++) {
        T *__restrict__ Ys = (T *)(s ? d.y2 : a.y);
        const long ch_stride = s ? d.y2_ch_stride : a.y_ch_stride;
#pragma unroll
        for (int o = 0; o < NO; o++) {
            if (o0 + o >= a.n_out) break;
            T *__restrict__ Y = Ys + (long)(o0 + o) * ch_stride;
#pragma unroll
            for (int j = 0; j < TT; j++) {
                if (t0 + j < a.n_t) {
                    T *yo = Y + (long)(t0 + j) * a.N;
                    if constexpr (ILV) {
                        using V2 = typename Vec2<T>::type;
                        V2 v; v.x = ar[s][o][j]; v.y = ai[s][o][j];
                        *(V2 *)(yo + ore) = v;
                    } else {
                        yo[ore] = ar[s][o][j]; yo[oim] = ai[s][o][j];
                    }
                }
            }
        }
    }
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
