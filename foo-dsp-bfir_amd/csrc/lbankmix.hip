// lbankmix.hip -- k_lbank_mix<R>: rows of the filter stores of ALL levels of a multi-level matrix or mimo engine written as
// weighted sums of up to BFIR_BANK_MIX_TERMS entries of its coefficient bank, the device side of
// bfir_engine_set_coeff_matrix_levels_bank_mix, _bank_mix_fade, _pairs_bank_mix and _pairs_bank_mix_fade.
//
// It has k_lbank_gather's grid (lbank.hip) with k_bank_mix's body (bankmix.hip).  The transform of every level is linear, so
// the weighted sum of an entry's spectra on a level is that level's spectrum of the weighted sum of the taps, and a filter
// between measured entries needs no transform on any level:
//
//     on every level k that takes part, every stored real of partition p < c_k of row rec.row of dst_k
//                                =  fl(w_1 h_1), then fl(. + fl(w_m h_m)) for m = 2, 3, ... over the record's terms with
//                                   count on level k > p, in the record's order
//     partitions c_k .. blocks[k] - 1  =  zeros                    (c_k: the largest count of the record's terms on level k)
//
// Each multiply and each add is rounded on its own in R (no fma), and the first product starts the sum (no 0 + ..., a product
// of -0 stays -0), so one term of weight 1 writes the bytes k_lbank_gather writes.  A term is read in the partitions below
// its OWN count on the level alone: what an entry's store holds past its count is never read, and a term that does not reach
// the level takes no part there.
//
// The level descriptors come by value (a null destination: the level is skipped), the listed rows as ONE table in HBM,
// [n_rows][BFIR_LBANK_MIX_REC]: destination row, live terms, then per term its entry, the weight's bits in R (low word, high
// word) and its count on every level.  The host (level_mix_records, coeff_tables.h) compacts the live terms (entry >= 0,
// converted weight != 0) to the front in listed order, so there is no liveness test here, and no per-level row count either:
// where no term covers an offset the lane stores zeros.  The grid is (pieces of a row over the participating levels, laid end
// to end) x (listed rows): a workgroup finds its level by comparing blockIdx.x with the prefix sums a.end[], with selects over
// the by-value descriptors and never an indexed read of them, and its record depends on blockIdx.y alone, so the words of
// the record are wave-uniform (scalar) loads.  A piece is BFIR_BANK_MIX_STEPS spans of BFIR_BANK_SPAN bytes, 256 lanes, 16
// bytes per lane and step: a lane issues the loads of every term that covers its offset, up to 2 x 4 x 16 bytes = 32
// registers, before it forms its sums and makes one 16-byte store per step.  Offsets are 64-bit per level.  No LDS, no scratch.
#include "kernels.h"
#include "mix_ops.h"

#include <climits>

namespace bfir {

constexpr int kLMixLanes = BFIR_BANK_SPAN / 16;
constexpr int kLMixT = BFIR_BANK_MIX_TERMS;

template <typename R>
__global__ __launch_bounds__(kLMixLanes) void k_lbank_mix(LBankMixArgs a)
{
    using V = MixVec<R>;
    constexpr int kN = 16 / sizeof(R);
    // the level of this workgroup: selects over the by-value descriptors, never an indexed read of them
    LBankLevel lv = a.lv[0];
    unsigned first = 0;
    int k = 0;
#pragma unroll
    for (int j = 1; j < BFIR_LBANK_LEVELS; j++)
        if (blockIdx.x >= a.end[j - 1]) { lv = a.lv[j]; first = a.end[j - 1]; k = j; }
    const int *__restrict__ rec = a.tab + BFIR_LBANK_MIX_REC * (size_t)blockIdx.y;   // wave-uniform
    const int row = rec[0], nt = rec[1];
    const char *src[kLMixT];
    unsigned long long lim[kLMixT];                           // the bytes of term j that take part on this level; 0 behind the record's terms
    R w[kLMixT];
#pragma unroll
    for (int j = 0; j < kLMixT; j++) {
        const int *__restrict__ t = rec + 2 + BFIR_LBANK_MIX_TERM * j;
        const bool on = j < nt;
        src[j] = (const char *)lv.bank + (unsigned long long)(on ? t[0] : 0) * lv.row_bytes;
        lim[j] = on ? (unsigned long long)t[3 + k] * lv.part_bytes : 0ull;   // the table is memory: k indexes a scalar load
        w[j] = mix_weight(on ? t[1] : 0, on ? t[2] : 0, R(0));
    }
    char *__restrict__ dst = (char *)lv.dst + (unsigned long long)row * lv.row_bytes;
    const unsigned long long off0 =
        (unsigned long long)(blockIdx.x - first) * (BFIR_BANK_MIX_STEPS * BFIR_BANK_SPAN) + threadIdx.x * 16u;
    V v[BFIR_BANK_MIX_STEPS][kLMixT];
#pragma unroll
    for (int u = 0; u < BFIR_BANK_MIX_STEPS; u++) {
        const unsigned long long off = off0 + (unsigned long long)u * BFIR_BANK_SPAN;
#pragma unroll
        for (int j = 0; j < kLMixT; j++) {
            v[u][j] = V{};
            if (off < lim[j]) v[u][j] = *(const V *)(src[j] + off);   // lim[j] <= row_bytes: inside the entry
        }
    }
#pragma unroll
    for (int u = 0; u < BFIR_BANK_MIX_STEPS; u++) {
        const unsigned long long off = off0 + (unsigned long long)u * BFIR_BANK_SPAN;
        V r = V{};                                            // no term covers the offset: zeros
        bool any = false;
#pragma unroll
        for (int j = 0; j < kLMixT; j++) {
            const bool on = off < lim[j];
#pragma unroll
            for (int n = 0; n < kN; n++) {
                const R p = mix_mul(w[j], v[u][j].x[n]);
                const R q = mix_add(r.x[n], p);
                r.x[n] = !on ? r.x[n] : any ? q : p;          // the first product starts the sum
            }
            any = any || on;
        }
        if (off < lv.row_bytes) *(V *)(dst + off) = r;
    }
}

// the workgroups a row of level k takes: none if the level is not part of the launch
static unsigned long long lmix_groups(const LBankLevel &lv)
{
    const unsigned long long per = (unsigned long long)BFIR_BANK_MIX_STEPS * BFIR_BANK_SPAN;
    return lv.dst ? (lv.row_bytes + per - 1) / per : 0;
}

bool lbank_mix_supported(const LBankMixArgs &a)
{
    if (a.n_rows < 0 || a.n_rows > 65535) return false;      // the table is the launch's: launch_lbank_mix asks for it
    unsigned long long groups = 0;
    for (const LBankLevel &lv : a.lv) {
        if (!lv.dst) continue;
        if (!lv.bank || lv.part_bytes == 0 || lv.part_bytes % 16 || lv.row_bytes % lv.part_bytes) return false;
        if (((uintptr_t)lv.bank | (uintptr_t)lv.dst) % 16) return false;
        groups += lmix_groups(lv);
        if (groups > (unsigned long long)(INT_MAX / kLMixLanes)) return false;   // threads per dimension in 32 bits
    }
    return true;
}

int launch_lbank_mix(LBankMixArgs a, int realsize, hipStream_t s)
{
    if (!a.tab || !lbank_mix_supported(a) || (realsize != 4 && realsize != 8)) return -1;
    unsigned long long groups = 0;
    for (int k = 0; k < BFIR_LBANK_LEVELS; k++) { groups += lmix_groups(a.lv[k]); a.end[k] = (unsigned)groups; }
    if (a.n_rows == 0 || groups == 0) return 0;
    const dim3 grid((unsigned)groups, (unsigned)a.n_rows), block(kLMixLanes);
    if (realsize == 4) hipLaunchKernelGGL(k_lbank_mix<float>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k_lbank_mix<double>, grid, block, 0, s, a);
    return 0;
}

}  // namespace bfir
