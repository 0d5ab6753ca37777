// rsp_device.h -- what every device translation unit of the frame chain shares (rsp_k1.hip,
// rsp_k2.hip, rsp_k3.hip, rsp_frame_aux.hip, rsp_stage3.hip, rsp_vcfar.hip, rsp_xcfar.hip, rsp_dbf.hip, rsp_mtd.hip, rsp_detect.hip, rsp_pc.hip, rsp_ddc.hip): the complex types and
// arithmetic, the raw buffer-resource loads and stores, the dynamic LDS block, the z addressing and
// the host-side launch helper.  No kernel.  Everything is in the anonymous namespace or static, so
// each unit gets its own copy and no unit exports a helper.
//
// Every kernel is a template over the real type T of the plan: double (complex128, the
// reference's MATLAB arithmetic; the default) or float (complex64).  Complex values are
// 2-wide ext_vector pairs (re, im) of T in registers, LDS and HBM alike.
#pragma once
#include "rsp_internal.h"
#include "rsp_cmag.h"   // f2, d2
#include <math.h>
#include <algorithm>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

template <class T> struct CxT;
template <> struct CxT<float> { typedef f2 V; };
template <> struct CxT<double> { typedef d2 V; };
template <class T> using cx = typename CxT<T>::V;   // complex of T
template <class V> struct ScalT;
template <> struct ScalT<f2> { typedef float S; };
template <> struct ScalT<d2> { typedef double S; };
template <class V> using scal = typename ScalT<V>::S;

// ---- complex arithmetic ------------------------------------------------------------------
// float: complex adds are single v_pk_add_f32 and products two packed ops; double: plain
// v_fma_f64 (gfx950 has no packed f64 arithmetic).
__device__ __forceinline__ f2 vmul(f2 a, f2 b) { return a.xx * b + a.yy * f2{-b.y, b.x}; }
__device__ __forceinline__ d2 vmul(d2 a, d2 b) { return d2{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
template <bool INV>
__device__ __forceinline__ f2 vrot(f2 a) {   // * (-i) forward, * (+i) inverse
    return INV ? a.yx * f2{-1.f, 1.f} : a.yx * f2{1.f, -1.f};
}
template <bool INV>
__device__ __forceinline__ d2 vrot(d2 a) {
    return INV ? d2{-a.y, a.x} : d2{a.y, -a.x};
}
template <bool INV, class V>
__device__ __forceinline__ V vtw(double c, double s) {   // exp(-+ i theta)
    typedef scal<V> S;
    return V{(S)c, (S)(INV ? s : -s)};
}
// |x| (fsf:184-185 abs): cmag, rsp_cmag.h (shared with the stage-3 CFAR)

// Raw buffer resources (SRSRC): 32-bit byte offsets and hardware range checking.  An offset at
// or past num_records reads 0 / drops the store, so masked lanes need no branch or select.
#define RSP_OOB 0x80000000u   // > any buffer this library makes (plans are validated < 2 GB/frame)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, 0x00020000);
}
// AUX: cache-policy bits of the load (2 = non-temporal)
template <class V, int AUX = 0> __device__ __forceinline__ V buf_ld(__amdgpu_buffer_rsrc_t r, unsigned off) {
    static_assert(sizeof(V) == 8 || sizeof(V) == 16, "one complex sample");
    if constexpr (sizeof(V) == 8)
        return __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b64(r, (int)off, 0, AUX));
    else
        return __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, AUX));
}
// A twiddle table in global memory read through a buffer resource: tw + e advances the per-lane
// byte offset, tw[i] (i a constant after unrolling) goes to the instruction's scalar offset, so
// the lgR loads of a butterfly share one offset VGPR instead of a 64-bit address each.
template <class V>
struct TwG {
    __amdgpu_buffer_rsrc_t r;
    unsigned off;
    __device__ __forceinline__ TwG operator+(int e) const { return TwG{r, off + (unsigned)e * (unsigned)sizeof(V)}; }
    __device__ __forceinline__ V operator[](int i) const {
        if constexpr (sizeof(V) == 8)
            return __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b64(r, (int)off, i * (int)sizeof(V), 0));
        else
            return __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, i * (int)sizeof(V), 0));
    }
};
// AUX: cache-policy bits of the store (2 = non-temporal)
template <int AUX = 0>
__device__ __forceinline__ void buf_st(__amdgpu_buffer_rsrc_t r, unsigned off, f2 x) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, x), r, (int)off, 0, AUX);
}
template <int AUX = 0>
__device__ __forceinline__ void buf_st(__amdgpu_buffer_rsrc_t r, unsigned off, d2 x) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, x), r, (int)off, 0, AUX);
}
template <int AUX = 0>
__device__ __forceinline__ void buf_st1(__amdgpu_buffer_rsrc_t r, unsigned off, float x) {
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(x), r, (int)off, 0, AUX);
}
template <int AUX = 0>
__device__ __forceinline__ void buf_st1(__amdgpu_buffer_rsrc_t r, unsigned off, double x) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, x), r, (int)off, 0, AUX);
}
// Non-temporal z and RDM stores: z (50 MB per frame, read back by K2 after the whole launch) and
// the RDM (never re-read on the device) only evict lines from L2 and the Infinity Cache
// (interleaved A/B: K1 -5.5 %, k2_pc -1.2 %).
#define RSP_Z_AUX 2     // K1's z stores
#define RSP_RDM_AUX 2   // K2's RDM stores

__device__ __forceinline__ int ilog2(int x) { return 31 - __clz(x); }

// One dynamic LDS allocation shared by every kernel of the including unit (each casts it to its types).
extern __shared__ __attribute__((aligned(16))) unsigned char rsp_lds[];

// Compacted used-sample index n' -> fast-time sample (Geometry::ivl_*).  Constant indices
// only: a per-lane index into the kernel-argument arrays would become a vector load, and its
// s_waitcnt vmcnt(0) would wait for every earlier vector memory op (e.g. pending z stores).
__device__ __forceinline__ int used_sample(const Geometry& g, int np) {
    int lo_q = g.ivl_lo[0], st_q = g.ivl_start[0];
#pragma unroll
    for (int i = 1; i < RSP_MAX_IVL; ++i)
        if (i < g.nivl && np >= g.ivl_start[i]) {
            lo_q = g.ivl_lo[i];
            st_q = g.ivl_start[i];
        }
    return lo_q + np - st_q;
}

// z (compacted Doppler-domain rows) addressing: row (b, v), compacted sample n'.
__device__ __forceinline__ size_t zaddr(const Geometry& g, int b, int v, int np) {
    const int lgNZ = ilog2(g.NZ);
    return (((size_t)b * g.nzc + (np >> lgNZ)) * g.P + v) * g.NZ + (np & (g.NZ - 1));
}

// A table from global memory into LDS, all NTHR threads of the workgroup.
template <int NTHR, class V>
__device__ __forceinline__ void stage_lds(V* lds, const V* glob, int n) {
    for (int i = threadIdx.x; i < n; i += NTHR) lds[i] = glob[i];
}

}  // namespace

// ---------------------------------------------------------------------------------------
// Dynamic LDS above 64 KiB must be opted in per kernel (gfx950 has 160 KiB per CU).
template <class K>
static hipError_t allow_lds(K kernel, size_t bytes) {
    if (bytes <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)bytes);
}
// One kernel launch: the LDS opt-in, the launch, the launch's error.
template <class K, class... A>
static hipError_t launch(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t s, A... args) {
    const hipError_t e = allow_lds(kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
    return hipGetLastError();
}
