// rsp_xcfar.hip -- the cross GOCA-CFAR of fun_run_goca_cfar_8 (fsf:192-213) as a map detector for
// gfx950: any real amplitude map (or the magnitudes of a complex one) in, a dense flag map, the
// threshold of every cell and the hit list out (the semantics are restated in include/rsp.h).
//
// k_xcfar<T, CPLX>: grid (range column strips, Doppler row blocks, maps), 256 threads.  A workgroup
// takes RSP_XC_ROWS Doppler rows of RSP_XC_COLS consecutive range columns and
//   1. stages the cross its cells read into LDS as amplitudes (CPLX: the magnitudes of the stage-2
//      result, by k2_pc's cmag): its own rows over COLS + 2 hR' columns (the range windows; hR' = hR
//      rounded up to 4) and the hV rows above and below over its own columns (the Doppler windows).
//      The corners of the (ROWS + 2 hV) x (COLS + 2 hR') rectangle are never read, so they are
//      neither loaded nor held.  A row per wave and step, lanes across the row in 16-byte units (a
//      map whose rows do not start on 16 bytes: one element per lane), NLD rows of loads in flight
//      per wave;
//   2. resolves a row per wave and step, lanes across the columns (LDS reads of consecutive words:
//      conflict-free): the four slice sums in the order rsp.h fixes (k3_map_sums' order), K3's
//      noise level (rsp_k3_arith.h), one multiply by T, A > threshold.  A cell that is not under
//      test gets flag 0 and threshold +Inf;
//   3. amplitudes (on request), thresholds and flags leave as whole row segments of the strip; hits
//      go to an LDS queue (one LDS atomic per wave and row, slots by ballot) that the workgroup
//      empties at the end with one global atomic; hits beyond QCAP in a workgroup (a dense map) are
//      reserved per wave and row on the global counter.  Hits are counted past hits_cap.
// No product feeds an add outside k3_quot's explicit FMAs, so no fused multiply-add can form.
#include "rsp_device.h"
#include "rsp_cmag.h"
#include "rsp_k3_arith.h"
#include <type_traits>

namespace {

constexpr int COLS = RSP_XC_COLS, ROWS = RSP_XC_ROWS;
constexpr int WAVES = RSP_THREADS / 64;
constexpr int QCAP = 512;   // hit records of the LDS queue
#ifndef XC_NLD
#define XC_NLD 4   // measured: 8 and 16 cost more in registers (workgroups per CU) than they hide in latency
#endif
constexpr int NLD = XC_NLD;   // rows of loads a wave has in flight while staging
constexpr int WMAX = xc_tile_width(RSP_XC_HMAX_R);
static_assert(COLS == 64 && ROWS % WAVES == 0 && ROWS <= 256, "a lane per column, a wave per row and step");
static_assert(sizeof(rsp_stage3_hit) == 32, "hit record layout");
// the envelope's corner with the queue fits a CU; the reference's 15 / 15 leaves room for three workgroups
static_assert(xc_lds_bytes(RSP_XC_HMAX_R, RSP_XC_HMAX_V, sizeof(double)) + QCAP * 20 + 8 <= RSP_LDS_BYTES, "envelope");
static_assert(3 * (xc_lds_bytes(15, 15, sizeof(double)) + QCAP * 20 + 8) <= RSP_LDS_BYTES, "3 workgroups per CU at 5/10/5/10");

extern __shared__ __align__(16) unsigned char xc_tile[];

template <class E, int N>
struct alignas(sizeof(E) * N) Pack {   // N consecutive map elements: one load
    E e[N];
};

// Map row t of the workgroup whose own rows start at b0, at the strip's first column: its own rows
// [b0, b0 + ROWS) lie in S[ROWS][W] with the strip at column hRa, the hV rows above and the hV rows
// below in H[2 hV][COLS] behind it.  t is wave-uniform wherever this is called.
template <class T>
__device__ __forceinline__ T* xc_row(T* S, int t, int b0, int W, int hRa, int hV) {
    if (t >= b0 && t < b0 + ROWS) return S + (t - b0) * W + hRa;
    return S + ROWS * W + (t < b0 ? t - (b0 - hV) : hV + t - (b0 + ROWS)) * COLS;
}

template <class T, bool CPLX, int N>
__device__ __forceinline__ void xc_stage(T* __restrict__ S, const void* __restrict__ in, size_t mapoff, int G, int W, int hRa,
                                         int hV, int cb, int tb, int te, int b0, int lane, int wave) {
    typedef typename std::conditional<CPLX, cx<T>, T>::type E;
    typedef Pack<E, N> U;
    constexpr int NJ = (WMAX / N + 63) / 64;   // units of a tile row per lane
    const E* __restrict__ src = static_cast<const E*>(in) + mapoff;   // W and cb are multiples of 4, N divides 4
    for (int t0 = tb + wave; t0 < te; t0 += NLD * WAVES) {
        U x[NLD][NJ];
        bool ok[NLD][NJ];
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int t = t0 + u * WAVES;
            const bool band = t >= b0 && t < b0 + ROWS;   // a row of the workgroup's own: the range windows read all of it
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int tc = (lane + 64 * j) * N, c = cb + tc;   // tile column, map column of the unit
                // a unit lies inside the map or outside it as a whole: c and (N > 1) G are multiples of N
                ok[u][j] = t < te && tc < W && c >= 0 && c < G && (band || (tc >= hRa && tc < hRa + COLS));
                if (ok[u][j]) x[u][j] = *reinterpret_cast<const U*>(src + (size_t)t * G + c);
            }
        }
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int t = t0 + u * WAVES;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                if (!ok[u][j]) continue;
                T* dst = xc_row(S, t, b0, W, hRa, hV) + ((lane + 64 * j) * N - hRa);
#pragma unroll
                for (int e = 0; e < N; ++e) {
                    if constexpr (CPLX) dst[e] = cmag(x[u][j].e[e]);
                    else dst[e] = x[u][j].e[e];
                }
            }
        }
    }
}

template <class T, bool CPLX>
__global__ __launch_bounds__(RSP_THREADS) void k_xcfar(XcDesc d, const void* __restrict__ in, double* __restrict__ amp,
                                                       double* __restrict__ thr, uint8_t* __restrict__ flags,
                                                       rsp_stage3_hit* __restrict__ hits, int* __restrict__ count,
                                                       int hits_cap) {
    T* S = reinterpret_cast<T*>(xc_tile);   // the cross, by xc_row
    __shared__ T q_amp[QCAP], q_thr[QCAP];
    __shared__ int q_cell[QCAP];   // (row in the workgroup) << 8 | column in the strip
    __shared__ int qn[2];
    typedef typename std::conditional<CPLX, cx<T>, T>::type E;
    constexpr int EPU = 16 / sizeof(E);   // elements per 16-byte unit
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g0 = blockIdx.x * COLS, v0 = blockIdx.y * ROWS, map = blockIdx.z;
    const int P = d.P, G = d.G, hR = d.hR, hV = d.hV;
    const int hRa = (hR + 3) & ~3, W = COLS + 2 * hRa, cb = g0 - hRa;
    const int tb = max(v0 - hV, 0), te = min(v0 + ROWS + hV, P);   // staged rows [tb, te)
    const size_t mapoff = (size_t)map * P * G;
    if (threadIdx.x == 0) qn[0] = 0;
    if (EPU > 1 && G % EPU == 0) xc_stage<T, CPLX, EPU>(S, in, mapoff, G, W, hRa, hV, cb, tb, te, v0, lane, wave);
    else xc_stage<T, CPLX, 1>(S, in, mapoff, G, W, hRa, hV, cb, tb, te, v0, lane, wave);
    __syncthreads();
    const T Tc = (T)d.T;
    const T fR = (T)d.rR, fV = (T)d.rV;
    const T iR = (T)1 / fR, iV = (T)1 / fV;   // as k3_cfar forms them
    const int c = g0 + lane;
    const bool incol = c < G, rut = c >= d.r0 && c < d.r1;   // the column is in the map / under test
    for (int vl = wave; vl < ROWS; vl += WAVES) {
        const int v = v0 + vl;
        if (v >= P) break;   // wave-uniform
        T a = 0, t = 0;
        bool hit = false;
        if (incol) {
            const T* rowp = S + vl * W + hRa + lane;   // xc_row(v) + lane
            a = *rowp;
            double td = INFINITY;
            if (rut && v >= d.v0 && v < d.v1) {
                T lr = 0, tr = 0, lv = 0, tv = 0;
                const T* lrp = rowp - hR;
                const T* trp = rowp + d.gR + 1;
                for (int q = 0; q < d.rR; ++q) lr += lrp[q];
                for (int q = 0; q < d.rR; ++q) tr += trp[q];
                for (int q = 0; q < d.rV; ++q) lv += xc_row(S, v - hV + q, v0, W, hRa, hV)[lane];
                for (int q = 0; q < d.rV; ++q) tv += xc_row(S, v + d.gV + 1 + q, v0, W, hRa, hV)[lane];
                t = Tc * k3_noise2<false, true>(lr, tr, lv, tv, fR, iR, fV, iV);   // SAT: a sum of +Inf gives +Inf
                hit = a > t;
                td = (double)t;
            }
            const size_t o = mapoff + (size_t)v * G + c;
            if (thr) thr[o] = td;
            if (amp) amp[o] = (double)a;
            if (flags) flags[o] = hit ? 1 : 0;
        }
        // hits go to the LDS queue; what does not fit (a dense map) is reserved on the global counter
        const unsigned long long m = __ballot(hit);
        if (m) {   // wave-uniform
            const int nh = __popcll(m);
            int off = 0;
            if (lane == 0) off = atomicAdd(&qn[0], nh);
            off = __shfl(off, 0);
            const int qfirst = max(off, QCAP), over = max(off + nh - qfirst, 0);   // the wave's hits past the queue
            int gbase = 0;
            if (over) {
                if (lane == 0) gbase = atomicAdd(count, over);
                gbase = __shfl(gbase, 0);
            }
            if (hit) {
                const int k = off + __popcll(m & ((1ull << lane) - 1ull));
                if (k < QCAP) {
                    q_cell[k] = (vl << 8) | lane;
                    q_amp[k] = a;
                    q_thr[k] = t;
                } else {
                    const int gidx = gbase + (k - qfirst);
                    if (hits && gidx >= 0 && gidx < hits_cap)   // counted past the capacity: the host grows the list
                        hits[gidx] = rsp_stage3_hit{v + 1, c + 1, map + 1, 0, (double)a, (double)t};
                }
            }
        }
    }
    __syncthreads();
    const int n = min(qn[0], QCAP);
    if (n == 0) return;   // uniform
    if (threadIdx.x == 0) qn[1] = atomicAdd(count, n);   // one global reservation per workgroup
    __syncthreads();
    if (!hits) return;
    for (int i = threadIdx.x; i < n; i += RSP_THREADS) {
        const int idx = qn[1] + i, e = q_cell[i];
        if (idx >= 0 && idx < hits_cap)   // counted past the capacity; the host grows the list and runs again
            hits[idx] = rsp_stage3_hit{v0 + (e >> 8) + 1, g0 + (e & 255) + 1, map + 1, 0, (double)q_amp[i], (double)q_thr[i]};
    }
}

template <class T, bool CPLX>
hipError_t launch_t(const XcDesc& d, const void* in, int n_maps, double* amp, double* thr, uint8_t* flags,
                    rsp_stage3_hit* hits, int* count, int hits_cap, hipStream_t s) {
    const size_t lds = xc_lds_bytes(d.hR, d.hV, sizeof(T));
    constexpr size_t queue = QCAP * (2 * sizeof(T) + sizeof(int)) + 2 * sizeof(int);   // the static LDS
    if (lds + queue > RSP_LDS_BYTES) return hipErrorInvalidValue;
    const dim3 grid((d.G + COLS - 1) / COLS, (d.P + ROWS - 1) / ROWS, n_maps);
    return launch(k_xcfar<T, CPLX>, grid, dim3(RSP_THREADS), lds, s, d, in, amp, thr, flags, hits, count, hits_cap);
}

}  // namespace

hipError_t launch_xcfar(const XcDesc& d, int prec, bool cplx, const void* in, int n_maps, double* amp, double* thr,
                        uint8_t* flags, rsp_stage3_hit* hits, int* count, int hits_cap, hipStream_t s) {
    // the kernel's envelope, whatever the caller checked: the window inside the tile's halos, the
    // cells under test inside the map and a halo away from its edges, the 32-bit cell index of the
    // hit counter and the grid's y / z limits
    const bool any = d.r1 > d.r0 && d.v1 > d.v0;
    if (d.P < 1 || d.G < 1 || d.rR < 1 || d.rV < 1 || d.gR < 0 || d.gV < 0 || d.hR < 0 || d.hR > RSP_XC_HMAX_R || d.hV < 0 ||
        d.hV > RSP_XC_HMAX_V || n_maps < 1 || n_maps > 65535 || (d.P + ROWS - 1) / ROWS > 65535 ||
        (long long)n_maps * d.P * d.G >= (1ll << 31) || hits_cap < 0 || !in || !count)
        return hipErrorInvalidValue;
    if (any ? ((long long)d.rR + d.gR != d.hR || (long long)d.rV + d.gV != d.hV || d.r0 < d.hR || d.r1 > d.G - d.hR ||
               d.v0 < d.hV || d.v1 > d.P - d.hV)
            : (d.r0 != d.r1 || d.v0 != d.v1 || d.hR != 0 || d.hV != 0))
        return hipErrorInvalidValue;
    if (prec == RSP_PREC_F64)
        return cplx ? launch_t<double, true>(d, in, n_maps, amp, thr, flags, hits, count, hits_cap, s)
                    : launch_t<double, false>(d, in, n_maps, amp, thr, flags, hits, count, hits_cap, s);
    return cplx ? launch_t<float, true>(d, in, n_maps, amp, thr, flags, hits, count, hits_cap, s)
                : launch_t<float, false>(d, in, n_maps, amp, thr, flags, hits, count, hits_cap, s);
}
