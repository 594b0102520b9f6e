// mix_ops.h -- the arithmetic of a bank mix, shared by k_bank_mix (bankmix.hip) and k_lbank_mix (lbankmix.hip): 16 bytes of
// reals, a weight from the two words of a record, and a multiply and an add that are each rounded on their own in R
// (__fmul_rn and its kin are not contracted into an fma).
#pragma once

#include <hip/hip_runtime.h>

namespace bfir {

template <typename R> struct alignas(16) MixVec { R x[16 / sizeof(R)]; };

__device__ inline float mix_weight(int lo, int, float) { return __int_as_float(lo); }
__device__ inline double mix_weight(int lo, int hi, double) { return __hiloint2double(hi, lo); }
__device__ inline float mix_mul(float a, float b) { return __fmul_rn(a, b); }
__device__ inline double mix_mul(double a, double b) { return __dmul_rn(a, b); }
__device__ inline float mix_add(float a, float b) { return __fadd_rn(a, b); }
__device__ inline double mix_add(double a, double b) { return __dadd_rn(a, b); }

}  // namespace bfir
