// rsp_k3_arith.h -- the arithmetic of the cross GOCA-CFAR test (fsf:197-209), shared by k3_cfar and
// k3_finish (rsp_k3.hip) and by the map detector k_xcfar (rsp_xcfar.hip), so that the two give the
// same bits on the same map.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// mean() = sum / n over the slices of fsf:197-203 (max(a/n, b/n) = max(a, b)/n).  double: the
// correctly rounded quotient, as MATLAB, without a division: q0 = x * RN(1/n), r = x - q0 n
// (exact, one FMA), q = RN(q0 + r RN(1/n)) is RN(x/n) (Markstein's theorem: RN(1/n) within half
// an ulp, q0 within one ulp of x/n; no underflow for these sums).  float: a multiply by 1/n
// (<= 1 ulp from the quotient).
template <class T>
__device__ __forceinline__ T k3_quot(T x, T fn, T in) {
    if constexpr (sizeof(T) == 8) {
        const T q0 = x * in;
        return __builtin_fma(__builtin_fma(-q0, fn, x), in, q0);
    } else {
        return x * in;
    }
}
// The noise level of the four slice sums.  ONE (n_R = n_V, the reference's 5/5): max(nR, nV) is one
// quotient of the largest slice sum.
template <bool ONE, class T>
__device__ __forceinline__ T k3_noise2(T lr, T tr, T lv, T tv, T fR, T iR, T fV, T iV) {
    if (ONE) return k3_quot(fmax(fmax(lr, tr), fmax(lv, tv)), fR, iR);
    const T nR = k3_quot(fmax(lr, tr), fR, iR), nV = k3_quot(fmax(lv, tv), fV, iV);
    return nR > nV ? nR : nV;
}

}  // namespace
