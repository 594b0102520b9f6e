// mat_ops.h -- what the matrix MAC kernels share (matrix.hip: k_mac_matrix; mfade.hip: k_mac_duo; mimo.hip: k_mac_mimo):
// one complex multiply-add in the order of every MAC here, the load of one bin of a spectrum in either layout, and the
// sums of one lane of k_mac_matrix and k_mac_mimo (mat_tile, mat_lane), which differ in their grids alone, and likewise of
// k_mac_duo and k_wduo (wduo.hip), the two-set forms (duo_tile, duo_lane); the walk of a row's listed pairs that
// k_patch_pairs (patch.hip) and k_wpatch (wpatch.hip) share (patch_pass, patch_row); and k_mac_mimo's choice of its register
// tile and grid (mimo_no, mimo_tt, mimo_grid), which k_wpatch takes over.
#pragma once
#include "kernels.h"

#include "fft_lds.h"

namespace bfir {

// one complex multiply-add of k_mac_small's order; DCNY: lane k == 0 keeps two real sums instead
template <bool DCNY, typename T>
__device__ __forceinline__ void mat_cmac(T &ar, T &ai, T xr, T xi, T hr, T hi, bool k0)
{
    const T r1 = fma(xr, hr, ar);
    const T r2 = fma(-xi, hi, r1);
    const T i2 = fma(xi, hr, fma(xr, hi, ai));
    if constexpr (DCNY) {
        const T ny = fma(xi, hi, ai);
        ar = k0 ? r1 : r2; ai = k0 ? ny : i2;
    } else {
        ar = r2; ai = i2;
    }
}

template <typename T, bool ILV>
__device__ __forceinline__ void mat_ld(const T *__restrict__ s, int ore, int oim, T &re, T &im)
{
    if constexpr (ILV) {
        using V2 = typename Vec2<T>::type;
        const V2 v = *(const V2 *)(s + ore);
        re = v.x; im = v.y;
    } else {
        re = s[ore]; im = s[oim];
    }
}

// The sums of one lane -- one bin, the tile of TT output blocks from t0, the NO outputs from o0 -- into its accumulators.  A is
// MatArgs (k_mac_matrix: the partition counts by value) or MimoArgs (k_mac_mimo: a table in HBM): a.nblk[o n_in + i] either
// way, wave-uniform.  Per input the lane walks the partitions in order with a window of TT delay-line spectra in registers,
// X[t0 + j - p] for j < TT: step p loads ONE new spectrum and the NO filter spectra H[o][i][p], then does NO x TT complex
// MACs.  Operands are fetched one step ahead.
template <typename T, bool ILV, int NO, int TT, bool DCNY, typename A>
__device__ __forceinline__ void mat_tile(const A &a, int o0, int t0, int ore, int oim, bool k0,
                                         T (&ar)[NO][TT], T (&ai)[NO][TT])
{
    const long N = a.N;
    const int ring = a.ring;
    const int sl = (a.base_slot + t0) % ring;                    // delay-line slot of block t0
    for (int i = 0; i < a.n_in; i++) {
        int nb[NO], nbm = 0, om = 0;
#pragma unroll
        for (int o = 0; o < NO; o++) {
            nb[o] = o0 + o < a.n_out ? a.nblk[(o0 + o) * a.n_in + i] : 0;
            if (nb[o] > nbm) { nbm = nb[o]; om = o; }
        }
        if (nbm == 0) continue;                                  // no filter of this tile reads input i
        const T *__restrict__ Xi = (const T *)a.x + (long)i * a.x_ch_stride;
        // filter spectra of (o, i); a pair without a filter is pointed at one with nbm partitions (loaded, never used)
        const T *__restrict__ Hp[NO];
#pragma unroll
        for (int o = 0; o < NO; o++)
            Hp[o] = (const T *)a.h + ((long)(o0 + (nb[o] > 0 ? o : om)) * a.n_in + i) * a.h_pair_stride;
        // window: slot (j - p) mod TT holds X[t0 + j - p].  In the last tile of a launch the blocks t0 + j >= n_t are slots
        // the NEXT chunk's forward transform may be writing at this moment (ring = 2 chunk + B keeps the read in bounds):
        // their values only reach accumulators that are never stored, so that race is harmless and needs no wait
        T wr[TT], wi[TT];
#pragma unroll
        for (int j = 0; j < TT; j++) {
            int sj = sl + j; if (sj >= ring) sj -= ring;
            mat_ld<T, ILV>(Xi + (long)sj * N, ore, oim, wr[j], wi[j]);
        }
        T qxr = (T)0, qxi = (T)0, qhr[NO], qhi[NO];              // operands of the next step (step 0 takes no new X)
#pragma unroll
        for (int o = 0; o < NO; o++) mat_ld<T, ILV>(Hp[o], ore, oim, qhr[o], qhi[o]);
        for (int p0 = 0; p0 < nbm; p0 += TT) {
#pragma unroll
            for (int ii = 0; ii < TT; ii++) {
                const int p = p0 + ii;
                if (p < nbm) {                                   // wave-uniform
                    if (p > 0) { wr[(TT - ii) % TT] = qxr; wi[(TT - ii) % TT] = qxi; }
                    // prefetch step p + 1 (clamped to the last step: in range, not used); each H register pair is
                    // reloaded as soon as its output's MACs have read it, so H costs 2 NO registers, not 4 NO
                    const int pn = p + 1 < nbm ? p + 1 : p;
                    int sn = sl - pn; if (sn < 0) sn += ring;       // X[t0 - pn] enters the window at step pn
                    mat_ld<T, ILV>(Xi + (long)sn * N, ore, oim, qxr, qxi);
#pragma unroll
                    for (int o = 0; o < NO; o++) {
                        if (p < nb[o]) {                         // wave-uniform: pairs without this partition are skipped
#pragma unroll
                            for (int j = 0; j < TT; j++) {
                                const int idx = (j - ii + TT) % TT;
                                mat_cmac<DCNY>(ar[o][j], ai[o][j], wr[idx], wi[idx], qhr[o], qhi[o], k0);
                            }
                        }
                        const int po = pn < nb[o] ? pn : (nb[o] > 0 ? nb[o] - 1 : pn);
                        mat_ld<T, ILV>(Hp[o] + (long)po * N, ore, oim, qhr[o], qhi[o]);
                    }
                }
            }
        }
    }
}


// ... and the whole of that lane: accumulate (the wave that holds bin 0 carries DC | Nyquist as two real sums), then store
// every (output, block) of the tile exactly once, outputs without any filter as zeros.
template <typename T, bool ILV, int NO, int TT, typename A>
__device__ __forceinline__ void mat_lane(const A &a, int k, bool wave0, int o0, int t0)
{
    const int ore = ILV ? 2 * k : 8 * (k >> 2) + (k & 3), oim = ILV ? ore + 1 : ore + 4;
    T ar[NO][TT], ai[NO][TT];
#pragma unroll
    for (int o = 0; o < NO; o++)
#pragma unroll
        for (int j = 0; j < TT; j++) { ar[o][j] = (T)0; ai[o][j] = (T)0; }
    if (wave0) mat_tile<T, ILV, NO, TT, true>(a, o0, t0, ore, oim, k == 0, ar, ai);
    else mat_tile<T, ILV, NO, TT, false>(a, o0, t0, ore, oim, false, ar, ai);
#pragma unroll
    for (int o = 0; o < NO; o++) {
        if (o0 + o >= a.n_out) break;
        T *__restrict__ Y = (T *)a.y + (long)(o0 + o) * a.y_ch_stride;
#pragma unroll
        for (int j = 0; j < TT; j++) {
            if (t0 + j < a.n_t) {
                T *yo = Y + (long)(t0 + j) * a.N;
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

// The sums of one lane under the TWO filter sets of a crossfaded coefficient change (k_mac_duo, mfade.hip; k_wduo, wduo.hip):
// mat_tile's loop with two H pointer sets and two count tables.  D is MatDuoArgs (the counts by value) or WduoArgs (two
// tables in HBM): d.a.nblk / d.nblk2 [o n_in + i] either way, wave-uniform.  Per input the window of TT delay-line spectra is
// set up ONCE and step p loads ONE new spectrum for both sets; the step loop runs to the larger of the two sets' maxima and
// every (set, output) is guarded by its own wave-uniform p < nb.
template <typename T, bool ILV, int NO, int TT, bool DCNY, typename D>
__device__ __forceinline__ void duo_tile(const D &d, int o0, int t0, int ore, int oim, bool k0,
                                         T (&ar)[2][NO][TT], T (&ai)[2][NO][TT])
{
    const auto &a = d.a;
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

// ... and the whole of that lane, as mat_lane: accumulate under both sets, then store every (set, output, block) of the tile
// exactly once, outputs without any filter as zeros.
template <typename T, bool ILV, int NO, int TT, typename D>
__device__ __forceinline__ void duo_lane(const D &d, int k, bool wave0, int o0, int t0)
{
    const auto &a = d.a;
    const int ore = ILV ? 2 * k : 8 * (k >> 2) + (k & 3), oim = ILV ? ore + 1 : ore + 4;
    T ar[2][NO][TT], ai[2][NO][TT];
#pragma unroll
    for (int s = 0; s < 2; s++)
#pragma unroll
        for (int o = 0; o < NO; o++)
#pragma unroll
            for (int j = 0; j < TT; j++) { ar[s][o][j] = (T)0; ai[s][o][j] = (T)0; }
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

// The continuation of one output's fma chains through the listed pairs of its row: the one body of k_patch_pairs
// (patch.hip, which documents the sum) and k_wpatch (wpatch.hip).
//
// One filter of a listed pair, nb > 0 partitions at Hp, into the accumulators of the lane's tile: mat_tile's walk for one
// output -- the window of TT delay-line spectra X[t0 + j - p] in registers, step p loads ONE new spectrum and H[p], operands
// fetched one step ahead.  NEG: the old filter, subtracted.
template <typename T, bool ILV, int TT, bool DCNY, bool NEG>
__device__ __forceinline__ void patch_pass(const PatchArgs &a, const T *__restrict__ Xi, const T *__restrict__ Hp, int nb,
                                           int sl, int ore, int oim, bool k0, T (&ar)[TT], T (&ai)[TT])
{
    const long N = a.N;
    const int ring = a.ring;
    // blocks t0 + j >= n_t of the last tile: slots the next chunk's forward transform may be writing (in bounds: ring = 2
    // chunk + B); their values only reach accumulators that are never stored
    T wr[TT], wi[TT];
#pragma unroll
    for (int j = 0; j < TT; j++) {
        int sj = sl + j; if (sj >= ring) sj -= ring;
        mat_ld<T, ILV>(Xi + (long)sj * N, ore, oim, wr[j], wi[j]);
    }
    T qxr = (T)0, qxi = (T)0, qhr, qhi;                          // operands of the next step (step 0 takes no new X)
    mat_ld<T, ILV>(Hp, ore, oim, qhr, qhi);
    for (int p0 = 0; p0 < nb; p0 += TT) {
#pragma unroll
        for (int ii = 0; ii < TT; ii++) {
            const int p = p0 + ii;
            if (p < nb) {                                        // wave-uniform
                if (p > 0) { wr[(TT - ii) % TT] = qxr; wi[(TT - ii) % TT] = qxi; }
                const T hr = NEG ? -qhr : qhr, hi = NEG ? -qhi : qhi;
                const int pn = p + 1 < nb ? p + 1 : p;           // prefetch step p + 1 (clamped: in range, not used)
                int sn = sl - pn; if (sn < 0) sn += ring;        // X[t0 - pn] enters the window at step pn
                mat_ld<T, ILV>(Xi + (long)sn * N, ore, oim, qxr, qxi);
                mat_ld<T, ILV>(Hp + (long)pn * N, ore, oim, qhr, qhi);
#pragma unroll
                for (int j = 0; j < TT; j++) {
                    const int idx = (j - ii + TT) % TT;
                    mat_cmac<DCNY>(ar[j], ai[j], wr[idx], wi[idx], hr, hi, k0);
                }
            }
        }
    }
}

template <typename T, bool ILV, int TT, bool DCNY>
__device__ __forceinline__ void patch_row(const PatchArgs &a, int o, int t0, int ore, int oim, bool k0, T (&ar)[TT], T (&ai)[TT])
{
    const int sl = (a.base_slot + t0) % a.ring;                  // delay-line slot of block t0
    const int e1 = a.row[o + 1];
    for (int e = a.row[o]; e < e1; e++) {                        // the row's listed pairs, in input order
        const int i = a.ent[3 * e], nb_new = a.ent[3 * e + 1], nb_old = a.ent[3 * e + 2];
        const T *__restrict__ Xi = (const T *)a.x + (long)i * a.x_ch_stride;
        const long hoff = ((long)o * a.n_in + i) * a.h_pair_stride;
        if (nb_new > 0) patch_pass<T, ILV, TT, DCNY, false>(a, Xi, (const T *)a.h2 + hoff, nb_new, sl, ore, oim, k0, ar, ai);
        if (nb_old > 0) patch_pass<T, ILV, TT, DCNY, true>(a, Xi, (const T *)a.h + hoff, nb_old, sl, ore, oim, k0, ar, ai);
    }
}

// k_mac_mimo's register tile and grid (mimo.hip), which k_wpatch (wpatch.hip) runs on as well.  The tile is k_mac_matrix's,
// for its reason (64 accumulator registers, four waves per SIMD): NO = the output count rounded up to a power of two, at
// most 4 (fp32) / 2 (fp64); TT = 1 on the latency path (launches of up to BFIR_MAT_SMALL_MAX blocks), else 8 (fp32; fp64
// with one output) or 4 (fp64).
constexpr int kMimoBins = 64;   // bins per workgroup: one wave
inline int mimo_no(const MimoArgs &a) { const int cap = a.realsize == 4 ? 4 : 2; int no = 1; while (no < a.n_out && no < cap) no *= 2; return no; }
inline int mimo_tt(const MimoArgs &a, int no)
{
    if (a.n_t <= BFIR_MAT_SMALL_MAX) return 1;
    return a.realsize == 4 ? 8 : (no == 1 ? 8 : 4);
}

// workgroups of the launch: (bin tiles, output tiles, time tiles)
inline void mimo_grid(const MimoArgs &a, int no, int tt, long &nbt, long &n_ot, long &nTT)
{
    nbt = (a.N / 2 + kMimoBins - 1) / kMimoBins; n_ot = (a.n_out + no - 1) / no; nTT = ((long)a.n_t + tt - 1) / tt;
}

}  // namespace bfir
