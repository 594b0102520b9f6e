// bank.hip -- k_bank_gather: rows of a filter store written from a coefficient bank (bfir_engine_bank_create), the device
// side of bfir_engine_set_coeff_matrix_bank, _bank_fade, _pairs_bank and _pairs_bank_fade.
//
// A bank is a store of filter rows in the form of the engine's own store H: [entries][B][N] spectra in the engine's precision
// and layout, transformed once by bfir_engine_bank_load.  A coefficient change that names bank entries is then a copy of
// rows, and this kernel makes all of them in one launch:
//
//     row tab[j].row of dst  =  the first tab[j].count partitions of bank entry tab[j].entry, then zeros up to B partitions
//                               (entry -1: zeros throughout)
//
// which is, over all B partitions, the row load_filters (engine.hip) writes for the same taps: it clears the row and
// transforms `count` partitions into it.  The partitions behind the count are WRITTEN as zeros, not copied, so whatever an
// entry holds there is never read.
//
// A row is bytes: one body serves both precisions and both layouts.  The listed rows come as a table in HBM ([n_rows][3]:
// destination row, entry, count), written by the call while the device is idle; a workgroup's record depends on blockIdx.y
// alone, so the three words are wave-uniform (scalar) loads.  The grid is (spans of a row) x (listed rows): a workgroup of
// 256 lanes moves BFIR_BANK_STEPS spans of BFIR_BANK_SPAN = 256 x 16 bytes, every lane one 16-byte load and one 16-byte store
// per step, all loads of a lane issued before its first store.  A partition is a multiple of 16 bytes, so every 16 bytes are
// wholly copied or wholly zero; the lanes past the copied part load nothing.  Offsets are 64-bit (a bank of a few thousand
// long filters passes 4 GiB).  No LDS, no scratch.
#include "kernels.h"

#include <climits>

namespace bfir {

constexpr int kBankLanes = BFIR_BANK_SPAN / 16;

__global__ __launch_bounds__(kBankLanes) void k_bank_gather(BankArgs a)
{
    const int *__restrict__ rec = a.tab + 3 * (size_t)blockIdx.y;   // wave-uniform
    const int row = rec[0], ent = rec[1], cnt = rec[2];
    const unsigned long long live = ent < 0 ? 0ull : (unsigned long long)cnt * a.part_bytes;   // the copied bytes of the row
    const char *__restrict__ src = (const char *)a.bank + (unsigned long long)(ent < 0 ? 0 : ent) * a.row_bytes;
    char *__restrict__ dst = (char *)a.dst + (unsigned long long)row * a.row_bytes;
    const unsigned long long off0 = (unsigned long long)blockIdx.x * (BFIR_BANK_STEPS * BFIR_BANK_SPAN) + threadIdx.x * 16u;
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
        if (off < a.row_bytes) *(uint4 *)(dst + off) = v[u];
    }
}

static unsigned long long bank_groups_x(const BankArgs &a)
{
    const unsigned long long per = (unsigned long long)BFIR_BANK_STEPS * BFIR_BANK_SPAN;
    return (a.row_bytes + per - 1) / per;
}

bool bank_gather_supported(const BankArgs &a)
{
    if (!a.bank || !a.dst || !a.tab || a.n_rows < 0 || a.n_rows > 65535) return false;
    if (a.part_bytes == 0 || a.part_bytes % 16 || a.row_bytes % a.part_bytes) return false;
    if (((uintptr_t)a.bank | (uintptr_t)a.dst) % 16) return false;
    return bank_groups_x(a) <= (unsigned long long)(INT_MAX / kBankLanes);   // threads per dimension in 32 bits
}

int launch_bank_gather(const BankArgs &a, hipStream_t s)
{
    if (!bank_gather_supported(a)) return -1;
    if (a.n_rows == 0) return 0;
    hipLaunchKernelGGL(k_bank_gather, dim3((unsigned)bank_groups_x(a), (unsigned)a.n_rows), dim3(kBankLanes), 0, s, a);
    return 0;
}

}  // namespace bfir
