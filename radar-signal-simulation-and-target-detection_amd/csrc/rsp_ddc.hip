// rsp_ddc.hip -- the digital down-converter (gfx950): NCO mixer, FIR and decimator of a real cube x [P x N x C]
// in MATLAB's layout (pulse index fastest) into the complex baseband cube y [P x No x C] (include/rsp.h has
// the definition; simulation_learn.m:79-102).
//
// k_ddc<T, NV, IQ>: a workgroup takes TP pulses x TK outputs of one channel (DdcDesc, rsp_geometry.h).  Thread t
// has pulse t mod TP and k lane t / TP: with P >= 64 a wave is 64 consecutive pulses of one sample row, with
// P = 1 it is 64 consecutive outputs, and in between both -- loads and stores are contiguous per wave in either
// regime.  The workgroup stages the (TK - 1) D + LC input rows of LC taps in LDS:
//   ms [rows]       the NCO value of the row, complex of T: the row's sample index is uniform over pulses, so
//                   one lane per row runs the 64-bit phase accumulator and the double sincos, never a lane per
//                   sample;
//   xs [rows][TP]   x as it is read, reals of T.  The product v = x m is formed in registers at each use:
//                   holding v would double the tile (16 bytes a sample against 8 in double) and with it the
//                   share of halo rows, L - D of them per tile, that neighbouring tiles read twice;
//   hs [L]          the taps.
// Loads take NV consecutive pulses per lane, 16 bytes (two doubles, four floats), where P is a multiple of NV
// and the base is aligned (else NV = 1); a store is one complex per lane, 16 bytes in double and 8 in single.
// The output's channel planes lie d.opitch elements apart (P No, or k_dbf's plane pitch when the result feeds it).
// Rows outside [0, N) and pulses past P read zeros through the buffer resource's range check (offset
// RSP_OOB), and stores past the tile's share of the cube are dropped the same way: nothing outside the
// P No C output elements is written.
// Each output is the chain acc = fma(h[j], x m, acc), j ascending from acc = 0, per part: the same values in
// the same order whatever the tiling, so results do not depend on TP, TK, LC or NV.  A filter whose rows do not
// fit the LDS budget is staged LC taps at a time, the accumulators kept in registers across the passes.
#include "rsp_device.h"
#include "rsp_noise_math.h"

namespace {

template <class E, int N>
struct alignas(sizeof(E) * N) Pack {   // N consecutive reals: one load
    E e[N];
};

template <class U>
__device__ __forceinline__ U ld_raw(__amdgpu_buffer_rsrc_t r, unsigned off) {
    static_assert(sizeof(U) == 4 || sizeof(U) == 8 || sizeof(U) == 16, "one load");
    if constexpr (sizeof(U) == 4)
        return __builtin_bit_cast(U, __builtin_amdgcn_raw_buffer_load_b32(r, (int)off, 0, 0));
    else if constexpr (sizeof(U) == 8)
        return __builtin_bit_cast(U, __builtin_amdgcn_raw_buffer_load_b64(r, (int)off, 0, 0));
    else
        return __builtin_bit_cast(U, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0));
}

__device__ __forceinline__ float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }

template <class T, int NV, bool IQ>
__global__ __launch_bounds__(RSP_DDC_THREADS) void k_ddc(DdcDesc d, const T* __restrict__ x, const T* __restrict__ h,
                                                         cx<T>* __restrict__ y) {
    typedef cx<T> V;
    typedef Pack<T, NV> U;
    V* ms = reinterpret_cast<V*>(rsp_lds);                  // [rows]
    T* xs = reinterpret_cast<T*>(rsp_lds + d.ms_bytes);     // [rows][TP], 16-byte aligned
    T* hs = xs + d.rows * d.TP;                             // [L]
    const int tid = threadIdx.x, nthr = d.threads;
    int b = blockIdx.x;
    const int pt = b % d.p_tiles;
    b /= d.p_tiles;
    const int kt = b % d.k_tiles, c = b / d.k_tiles;
    const int p0 = pt * d.TP, k0 = kt * d.TK;
    const int pl = tid & (d.TP - 1), kl = tid >> d.lgTP;
    const __amdgpu_buffer_rsrc_t rx = buf_rsrc(x, d.in_bytes), ry = buf_rsrc(y, d.out_bytes);

    for (int i = tid; i < d.L; i += nthr) hs[i] = h[i];

    T are[RSP_DDC_MAX_KPT], aim[RSP_DDC_MAX_KPT];
#pragma unroll
    for (int i = 0; i < RSP_DDC_MAX_KPT; ++i) are[i] = aim[i] = (T)0;

    const int lgU = d.lgTP - ilog2(NV);   // NV <= TP: load units of a row = TP / NV
    for (int j0 = 0; j0 < d.L; j0 += d.LC) {
        const int lc = min(d.LC, d.L - j0);
        const int rows = (d.TK - 1) * d.D + lc;
        const int nbase = d.off + k0 * d.D - (j0 + lc - 1);   // the sample of row 0
        if (j0) __syncthreads();   // the rows of the last pass are read
        for (int r = tid; r < rows; r += nthr) {
            const int n = nbase + r;
            V m = V{(T)0, (T)0};
            if (n >= 0 && n < d.N) {
                const uint64_t phase = d.w0 + (uint64_t)n * d.w;
                double sn, cs;
                rsp_nm_sincos2pi((double)(phase >> 11) * 0x1p-53, &sn, &cs);
                m = IQ ? V{(T)cs, (T)-sn} : V{(T)sn, (T)0};
            }
            ms[r] = m;
        }
        // unit u of the tile is row u >> lgU, pulses NV (u mod 2^lgU) ..: LDS element u NV.  RSP_DDC_LOADS loads
        // per thread are in flight before the first of them is stored.
        const int units = rows << lgU;
        for (int u0 = tid; u0 < units; u0 += RSP_DDC_LOADS * nthr) {
            U xin[RSP_DDC_LOADS];
#pragma unroll
            for (int i = 0; i < RSP_DDC_LOADS; ++i) {
                const int u = u0 + i * nthr;
                const int n = nbase + (u >> lgU), p = p0 + NV * (u & ((1 << lgU) - 1));
                const bool in = u < units && n >= 0 && n < d.N && p < d.P;   // P is a multiple of NV: a unit is inside or outside as a whole
                const unsigned o = in ? ((unsigned)(c * d.N + n) * (unsigned)d.P + (unsigned)p) * (unsigned)sizeof(T) : RSP_OOB;
                xin[i] = ld_raw<U>(rx, o);
            }
#pragma unroll
            for (int i = 0; i < RSP_DDC_LOADS; ++i) {
                const int u = u0 + i * nthr;
                if (u < units) reinterpret_cast<U*>(xs)[u] = xin[i];
            }
        }
        __syncthreads();
        if (kl < d.KL) {
            const int r0 = kl * d.D + lc - 1, rstep = d.KL * d.D;
            for (int jj = 0; jj < lc; ++jj) {
                const T hj = hs[j0 + jj];
#pragma unroll
                for (int i = 0; i < RSP_DDC_MAX_KPT; ++i)
                    if (i < d.KPT) {
                        const int r = r0 + i * rstep - jj;
                        const T xv = xs[r * d.TP + pl];
                        const V m = ms[r];
                        are[i] = fma_t(hj, xv * m.x, are[i]);
                        if constexpr (IQ) aim[i] = fma_t(hj, xv * m.y, aim[i]);
                    }
            }
        }
    }
    if (kl < d.KL) {
        const int p = p0 + pl;
#pragma unroll
        for (int i = 0; i < RSP_DDC_MAX_KPT; ++i)
            if (i < d.KPT) {
                const int k = k0 + kl + i * d.KL;
                const bool in = k < d.No && p < d.P;
                const unsigned o = in ? ((unsigned)c * d.opitch + (unsigned)k * (unsigned)d.P + (unsigned)p) * (unsigned)sizeof(V) : RSP_OOB;
                buf_st(ry, o, V{are[i], IQ ? aim[i] : (T)0});
            }
    }
}

template <class T, int NV>
hipError_t launch_ddc_m(const DdcDesc& d, const void* x, const void* h, void* y, hipStream_t s) {
    const dim3 grid((unsigned)(d.k_tiles * d.p_tiles * d.C)), block((unsigned)d.threads);
    const T* xp = static_cast<const T*>(x);
    const T* hp = static_cast<const T*>(h);
    cx<T>* yp = static_cast<cx<T>*>(y);
    if (d.mode == RSP_DDC_NCO_IQ) return launch(k_ddc<T, NV, true>, grid, block, d.lds_bytes, s, d, xp, hp, yp);
    return launch(k_ddc<T, NV, false>, grid, block, d.lds_bytes, s, d, xp, hp, yp);
}

template <class T>
hipError_t launch_ddc_t(const DdcDesc& d, const void* x, const void* h, void* y, hipStream_t s) {
    constexpr int NV = 16 / (int)sizeof(T);
    if (d.P % NV == 0 && d.TP >= NV && (uintptr_t)x % 16 == 0) return launch_ddc_m<T, NV>(d, x, h, y, s);
    return launch_ddc_m<T, 1>(d, x, h, y, s);
}

}  // namespace

hipError_t launch_ddc(const DdcDesc& d, int prec, const void* x, const void* h, void* y, hipStream_t s) {
    if (d.No < 1) return hipSuccess;   // N <= off: no output
    return prec == RSP_PREC_F64 ? launch_ddc_t<double>(d, x, h, y, s) : launch_ddc_t<float>(d, x, h, y, s);
}
