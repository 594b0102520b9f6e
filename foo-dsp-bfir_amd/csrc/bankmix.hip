// bankmix.hip -- k_bank_mix<R>: rows of a filter store written as weighted sums of up to BFIR_BANK_MIX_TERMS entries of a
// coefficient bank, the device side of bfir_engine_set_coeff_matrix_bank_mix, _bank_mix_fade, _pairs_bank_mix and
// _pairs_bank_mix_fade.
//
// The transform is linear: a weighted sum of entry SPECTRA is the spectrum of the same weighted sum of the taps, so a filter
// between measured entries (two on an arc, three on a triangle, four on a grid), or one entry at another level, needs no
// transform.  It is k_bank_gather (bank.hip) with arithmetic in the copy:
//
//     every stored real of partition p < c of row rec.row  =  fl(w_1 h_1), then fl(. + fl(w_m h_m)) for m = 2, 3, ...
//                                                             over the record's terms with count > p, in the record's order
//     partitions c .. B - 1                                =  zeros
//
// Each multiply and each add is rounded on its own in R (no fma: __fmul_rn and its kin are not contracted), and the first
// product starts the sum (no 0 + ..., a product of -0 stays -0), so a NumPy restatement from bfir_engine_bank_read is exact
// to the bit, and one term of weight 1 writes the bytes k_bank_gather writes.  A term is read in the partitions below its
// OWN count alone: what an entry's store holds past its count is never read.  Real and imaginary parts, DC and Nyquist and
// both spectrum layouts are all "stored reals": the operation is elementwise and the layout does not matter to it.
//
// The host (bank_mix_gather, engine.hip) compacts the live terms (entry >= 0, converted weight != 0) to the front in listed
// order, so there is no liveness test here; c is their largest count, and a row without a live term has c = 0 and is zeros.
// A record depends on blockIdx.y alone, so its words are wave-uniform (scalar) loads.  The grid is k_bank_gather's, (pieces
// of a row) x (listed rows), 256 lanes, 16 bytes per lane and step, BFIR_BANK_MIX_STEPS steps per workgroup: a lane issues the
// loads of every term that covers its offset, up to 2 x 4 x 16 bytes = 32 registers, before it forms its sums and makes one
// 16-byte store per step.  Offsets are 64-bit.  No LDS, no scratch.
#include "kernels.h"
#include "mix_ops.h"

#include <climits>

namespace bfir {

constexpr int kMixLanes = BFIR_BANK_SPAN / 16;
constexpr int kMixT = BFIR_BANK_MIX_TERMS;

template <typename R>
__global__ __launch_bounds__(kMixLanes) void k_bank_mix(BankMixArgs a)
{
    using V = MixVec<R>;
    constexpr int kN = 16 / sizeof(R);
    const int *__restrict__ rec = a.tab + BFIR_BANK_MIX_REC * (size_t)blockIdx.y;   // wave-uniform
    const int row = rec[0], nt = rec[2];
    const char *src[kMixT];
    unsigned long long lim[kMixT];                            // the bytes of term j that take part; 0 behind the record's terms
    R w[kMixT];
#pragma unroll
    for (int j = 0; j < kMixT; j++) {
        const bool on = j < nt;
        src[j] = (const char *)a.bank + (unsigned long long)(on ? rec[3 + 4 * j] : 0) * a.row_bytes;
        lim[j] = on ? (unsigned long long)rec[4 + 4 * j] * a.part_bytes : 0ull;
        w[j] = mix_weight(on ? rec[5 + 4 * j] : 0, on ? rec[6 + 4 * j] : 0, R(0));
    }
    char *__restrict__ dst = (char *)a.dst + (unsigned long long)row * a.row_bytes;
    const unsigned long long off0 = (unsigned long long)blockIdx.x * (BFIR_BANK_MIX_STEPS * BFIR_BANK_SPAN) + threadIdx.x * 16u;
    V v[BFIR_BANK_MIX_STEPS][kMixT];
#pragma unroll
    for (int u = 0; u < BFIR_BANK_MIX_STEPS; u++) {
        const unsigned long long off = off0 + (unsigned long long)u * BFIR_BANK_SPAN;
#pragma unroll
        for (int j = 0; j < kMixT; j++) {
            v[u][j] = V{};
            if (off < lim[j]) v[u][j] = *(const V *)(src[j] + off);   // lim[j] <= row_bytes: inside the entry
        }
    }
#pragma unroll
    for (int u = 0; u < BFIR_BANK_MIX_STEPS; u++) {
        const unsigned long long off = off0 + (unsigned long long)u * BFIR_BANK_SPAN;
        V r = V{};                                            // at and past rec[1] partitions no term covers the offset: zeros
        bool any = false;
#pragma unroll
        for (int j = 0; j < kMixT; j++) {
            const bool on = off < lim[j];
#pragma unroll
            for (int n = 0; n < kN; n++) {
                const R p = mix_mul(w[j], v[u][j].x[n]);
                const R q = mix_add(r.x[n], p);
                r.x[n] = !on ? r.x[n] : any ? q : p;          // the first product starts the sum
            }
            any = any || on;
        }
        if (off < a.row_bytes) *(V *)(dst + off) = r;
    }
}

static unsigned long long mix_groups_x(const BankMixArgs &a)
{
    const unsigned long long per = (unsigned long long)BFIR_BANK_MIX_STEPS * BFIR_BANK_SPAN;
    return (a.row_bytes + per - 1) / per;
}

bool bank_mix_supported(const BankMixArgs &a)
{
    if (!a.bank || !a.dst || !a.tab || a.n_rows < 0 || a.n_rows > 65535) return false;
    if (a.part_bytes == 0 || a.part_bytes % 16 || a.row_bytes % a.part_bytes) return false;
    if (((uintptr_t)a.bank | (uintptr_t)a.dst) % 16) return false;
    return mix_groups_x(a) <= (unsigned long long)(INT_MAX / kMixLanes);   // threads per dimension in 32 bits
}

int launch_bank_mix(const BankMixArgs &a, int realsize, hipStream_t s)
{
    if (!bank_mix_supported(a) || (realsize != 4 && realsize != 8)) return -1;
    if (a.n_rows == 0) return 0;
    const dim3 grid((unsigned)mix_groups_x(a), (unsigned)a.n_rows), block(kMixLanes);
    if (realsize == 4) hipLaunchKernelGGL(k_bank_mix<float>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k_bank_mix<double>, grid, block, 0, s, a);
    return 0;
}

}  // namespace bfir
