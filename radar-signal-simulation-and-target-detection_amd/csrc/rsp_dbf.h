// rsp_dbf.h -- the matrix-core DBF that K1 (rsp_k1.hip) and the stand-alone k_dbf (rsp_dbf.hip)
// share: one trait, so that both run the same sequence of fused operations per output element.
// No kernel.  In the anonymous namespace like rsp_device.h: each unit gets its own copy.
#pragma once
#include "rsp_device.h"

namespace {

// DBF (fsf:93-97) on the matrix cores as a real GEMM: D[16 rows x 16 pulses] += A[16 x 4
// channels] * B[4 channels x 16 pulses], rows = (Re, Im) x 8 beams of conj(W), one MFMA per
// (channel group, Re/Im part of x).  A lane's 16-B load is its B operand:
//  - float: v_mfma_f32_16x16x4f32; the load holds pulses (p, p+1) of one channel (re, im, re,
//    im), the B operand of two column blocks (even / odd pulses); D row 4*(lane>>4) + i.
//  - double: v_mfma_f64_16x16x4f64; the load holds one pulse (re, im); D row (lane>>4) + 4*i
//    (the f64 C/D layout, cdna_hip_programming.md section 3).
// Which (beam, part) a D row is, is the A table's business (rsp_dbf_atab, rsp_geometry.h).
template <class T> struct Dbf;
template <> struct Dbf<float> {
    static constexpr int PPL = 2, NACC = 2;
    typedef f32x4 Ld;
    typedef f32x4 Acc;
    static __device__ __forceinline__ Ld bits(u32x4 t) { return __builtin_bit_cast(f32x4, t); }
    static __device__ __forceinline__ void mma(Acc (&acc)[NACC], float are, float aim, Ld x) {
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(are, x.x, acc[0], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(aim, x.y, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(are, x.z, acc[1], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(aim, x.w, acc[1], 0, 0, 0);
    }
    static __device__ __forceinline__ int row(int grp, int i) { return 4 * grp + i; }
};
template <> struct Dbf<double> {
    static constexpr int PPL = 1, NACC = 1;
    typedef d2 Ld;
    typedef f64x4 Acc;
    static __device__ __forceinline__ Ld bits(u32x4 t) { return __builtin_bit_cast(d2, t); }
    static __device__ __forceinline__ void mma(Acc (&acc)[NACC], double are, double aim, Ld x) {
        acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(are, x.x, acc[0], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(aim, x.y, acc[0], 0, 0, 0);
    }
    static __device__ __forceinline__ int row(int grp, int i) { return grp + 4 * i; }
};

}  // namespace
