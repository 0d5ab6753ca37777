// rsp_k3_arith.h -- the arithmetic of the cross GOCA-CFAR test (fsf:197-209), shared by k3_cfar and
// k3_finish (rsp_k3.hip) and by the map detector k_xcfar (rsp_xcfar.hip), so that the two give the
// same bits on the same map.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// mean() = sum / n over the slices of fsf:197-203 (max(a/n, b/n) = max(a, b)/n).  double: the
// correctly rounded quotient, as MATLAB, without a division: q0 = x * RN(1/n), r = x - q0 n
// (exact, one FMA), q = RN(q0 + r RN(1/n)) is RN(x/n) (Markstein's theorem: RN(1/n) within half
// an ulp, q0 within one ulp of x/n).  The residual r is a multiple of ulp(q0), so it is exact even
// where it is subnormal, and the form equals RN(x/n) wherever the quotient is a normal number
// (x >= n 2^-1022; include/rsp.h, "Value domain").  Below that, x/n can lie exactly half way between
// two subnormals (n even and no power of two); the division then rounds to even and this form to
// the side r RN(1/n) falls on.  x = +Inf: q0 = +Inf and the residual is NaN, where the division gives
// +Inf.  The map detector, whose thresholds are an output, asks for SAT: one select returns q0 when
// the refined quotient is NaN.  K3's hot path keeps the bare form, and differs from the map detector
// only on a slice sum that overflowed: with nR NaN, `nR > nV ? nR : nV` below returns nV, which may be
// finite (with nV NaN, or ONE, the threshold is NaN and no cell exceeds it), where SAT gives a
// threshold of +Inf.  K3's slice sums are sums of magnitudes inside the magnitude domain of
// include/rsp.h ("Value domain": below 2^512), which cannot overflow.  float: a multiply by 1/n
// (<= 1 ulp from the quotient).
template <bool SAT = false, class T>
__device__ __forceinline__ T k3_quot(T x, T fn, T in) {
    if constexpr (sizeof(T) == 8) {
        const T q0 = x * in;
        const T q = __builtin_fma(__builtin_fma(-q0, fn, x), in, q0);
        if constexpr (SAT) return q == q ? q : q0;   // NaN only from a q0 that is not finite
        return q;
    } else {
        return x * in;
    }
}
// The noise level of the four slice sums.  ONE (n_R = n_V, the reference's 5/5): max(nR, nV) is one
// quotient of the largest slice sum.
template <bool ONE, bool SAT = false, class T>
__device__ __forceinline__ T k3_noise2(T lr, T tr, T lv, T tv, T fR, T iR, T fV, T iV) {
    if (ONE) return k3_quot<SAT>(fmax(fmax(lr, tr), fmax(lv, tv)), fR, iR);
    const T nR = k3_quot<SAT>(fmax(lr, tr), fR, iR), nV = k3_quot<SAT>(fmax(lv, tv), fV, iV);
    return nR > nV ? nR : nV;
}

}  // namespace
