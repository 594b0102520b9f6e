// mat_ops.h -- the two per-term operations the matrix MAC kernels share (matrix.hip: k_mac_matrix; mfade.hip: k_mac_duo):
// one complex multiply-add in the order of every MAC here, and the load of one bin of a spectrum in either layout.
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

}  // namespace bfir
