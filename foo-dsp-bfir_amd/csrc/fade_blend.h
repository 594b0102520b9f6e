// fade_blend.h -- the blend of fftw_convolver::convolver_crossfade_inplace (brutefir/fftw_convolver.cpp:296-315), shared by
// the fade back ends of fade.hip (uniform and matrix engines) and lfade.hip (two-level and multi-level engines).
#pragma once
#include <hip/hip_runtime.h>

namespace bfir {

// crossfade[n] * (1.0 - f * (float)n) + buffer[n] * f * (float)n with C's promotions (:301-303): `1.0` is a double, so
// the first product and the sum are double; the second product is float.  Every operation rounded on its own.
__device__ __forceinline__ float fade_blend(float y_old, float y_new, float f, int m)
{
#pragma clang fp contract(off)
    const float fm = f * (float)m;
    const double a = (double)y_old * (1.0 - (double)fm);
    const float b = y_new * f * (float)m;
    return (float)(a + (double)b);
}
// fp64, same roles (old faded out, new faded in): buf1[n] * (1.0 - d * (double)n) + buf2[n] * d * (double)n  (:311-313)
__device__ __forceinline__ double fade_blend(double y_old, double y_new, double d, int m)
{
#pragma clang fp contract(off)
    return y_old * (1.0 - d * (double)m) + y_new * d * (double)m;
}

}  // namespace bfir
