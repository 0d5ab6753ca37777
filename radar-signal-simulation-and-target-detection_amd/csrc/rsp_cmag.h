// rsp_cmag.h -- |x| of a complex value, the one magnitude routine of the device code: k2_pc's
// magnitude maps (rsp_k2.hip) and the stage-3 CFAR's amplitudes (rsp_stage3.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));
typedef double d2 __attribute__((ext_vector_type(2)));

// |x| (fsf:184-185 abs): hardware square root for float (v_sqrt_f32, 1 ulp); for double the
// compiler's own refinement of v_rsq_f64 (Goldschmidt step + two Newton corrections) without
// its ldexp scaling and class checks, which guard only denormal / infinite inputs -- not the
// magnitudes of a radar map; 0 stays 0.
__device__ __forceinline__ float cmag(f2 x) { return __builtin_amdgcn_sqrtf(x.x * x.x + x.y * x.y); }
__device__ __forceinline__ double cmag(d2 x) {
    const double q = x.x * x.x + x.y * x.y;
    const double r = __builtin_amdgcn_rsq(q);           // v_rsq_f64
    double g = q * r, h = 0.5 * r;
    const double r0 = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r0, g);
    h = __builtin_fma(h, r0, h);
    g = __builtin_fma(__builtin_fma(-g, g, q), h, g);
    g = __builtin_fma(__builtin_fma(-g, g, q), h, g);
    return q > 0.0 ? g : 0.0;
}

}  // namespace
