// lbank.hip -- k_lbank_gather: rows of the filter stores of ALL levels of a multi-level matrix or mimo engine written from its
// coefficient bank (bfir_engine_levels_bank_create), the device side of bfir_engine_set_coeff_matrix_levels_bank, _bank_fade,
// _pairs_bank and _pairs_bank_fade.
//
// The bank of such an engine is one store per level, [entries][blocks[k]][N_k] spectra in the level's precision and layout,
// and a coefficient change that names entries is a copy of rows on every level.  k_bank_gather (bank.hip) makes the copies of
// one store in one launch; its cost at the renderer's shape is the launch, the table upload and the wait, not the bytes.  So
// the levels of a call do not get a launch, a table and a wait each: this kernel makes the copies of every level at once,
//
//     on every level k that takes part:   row tab[j].row of dst_k  =  the first tab[j].count[k] partitions of entry tab[j].entry
//                                          of bank_k, then zeros up to blocks[k] partitions   (entry -1: zeros throughout)
//
// The level descriptors come by value (bank, destination, bytes of a partition and of a row; a null destination: the level is
// skipped), the listed rows as ONE table in HBM ([n_rows][2 + BFIR_LBANK_LEVELS]: destination row, entry, the count on every
// level).  The grid is (pieces of a row over the participating levels, laid end to end) x (listed rows): a workgroup finds
// its level by comparing blockIdx.x with the prefix sums a.end[] -- wave-uniform, and no workgroup is idle -- and its record
// depends on blockIdx.y alone, so the words of the record are scalar loads.  The body is k_bank_gather's: 256 lanes move
// BFIR_BANK_STEPS spans of BFIR_BANK_SPAN bytes, 16 bytes per lane and step, all loads of a lane issued before its first
// store; lanes past the copied part load nothing and store zeros, lanes past the row store nothing.  Offsets are 64-bit per
// level.  No LDS, no scratch.
#include "kernels.h"

#include <climits>

namespace bfir {

constexpr int kLBankLanes = BFIR_BANK_SPAN / 16;
constexpr int kLBankRec = 2 + BFIR_LBANK_LEVELS;

__global__ __launch_bounds__(kLBankLanes) void k_lbank_gather(LBankArgs a)
{
    // the level of this workgroup: selects over the by-value descriptors, never an indexed read of them
    LBankLevel lv = a.lv[0];
    unsigned first = 0;
    int k = 0;
#pragma unroll
    for (int j = 1; j < BFIR_LBANK_LEVELS; j++)
        if (blockIdx.x >= a.end[j - 1]) { lv = a.lv[j]; first = a.end[j - 1]; k = j; }
    const int *__restrict__ rec = a.tab + kLBankRec * (size_t)blockIdx.y;   // wave-uniform
    const int row = rec[0], ent = rec[1], cnt = rec[2 + k];
    const unsigned long long live = ent < 0 ? 0ull : (unsigned long long)cnt * lv.part_bytes;   // the copied bytes of the row
    const char *__restrict__ src = (const char *)lv.bank + (unsigned long long)(ent < 0 ? 0 : ent) * lv.row_bytes;
    char *__restrict__ dst = (char *)lv.dst + (unsigned long long)row * lv.row_bytes;
    const unsigned long long off0 = (unsigned long long)(blockIdx.x - first) * (BFIR_BANK_STEPS * BFIR_BANK_SPAN) + threadIdx.x * 16u;
    uint4 v[BFIR_BANK_STEPS];
#pragma unroll
    for (int u = 0; u < BFIR_BANK_STEPS; u++) {
        const unsigned long long off = off0 + (unsigned long long)u * BFIR_BANK_SPAN;
        v[u] = make_uint4(0u, 0u, 0u, 0u);
        if (off < live) v[u] = *(const uint4 *)(src + off);     // live <= row_bytes: inside the entry
    }
#pragma unroll
    for (int u = 0; u < BFIR_BANK_STEPS; u++) {
        const unsigned long long off = off0 + (unsigned long long)u * BFIR_BANK_SPAN;
        if (off < lv.row_bytes) *(uint4 *)(dst + off) = v[u];
    }
}

// the workgroups a row of level k takes: none if the level is not part of the launch
static unsigned long long lbank_groups(const LBankLevel &lv)
{
    const unsigned long long per = (unsigned long long)BFIR_BANK_STEPS * BFIR_BANK_SPAN;
    return lv.dst ? (lv.row_bytes + per - 1) / per : 0;
}

bool lbank_gather_supported(const LBankArgs &a)
{
    if (a.n_rows < 0 || a.n_rows > 65535) return false;      // the table is the launch's: launch_lbank_gather asks for it
    unsigned long long groups = 0;
    for (const LBankLevel &lv : a.lv) {
        if (!lv.dst) continue;
        if (!lv.bank || lv.part_bytes == 0 || lv.part_bytes % 16 || lv.row_bytes % lv.part_bytes) return false;
        if (((uintptr_t)lv.bank | (uintptr_t)lv.dst) % 16) return false;
        groups += lbank_groups(lv);
        if (groups > (unsigned long long)(INT_MAX / kLBankLanes)) return false;   // threads per dimension in 32 bits
    }
    return true;
}

int launch_lbank_gather(LBankArgs a, hipStream_t s)
{
    if (!a.tab || !lbank_gather_supported(a)) return -1;
    unsigned long long groups = 0;
    for (int k = 0; k < BFIR_LBANK_LEVELS; k++) { groups += lbank_groups(a.lv[k]); a.end[k] = (unsigned)groups; }
    if (a.n_rows == 0 || groups == 0) return 0;
    hipLaunchKernelGGL(k_lbank_gather, dim3((unsigned)groups, (unsigned)a.n_rows), dim3(kLBankLanes), 0, s, a);
    return 0;
}

}  // namespace bfir
