// rsp_stage3.hip -- stage-3 range CFAR of the stage-2 path for gfx950: local_execute_cfar /
// executeCFAR_2D / Function_CFAR1D_sub of debug_simulated_data_processing_v2.m:419-511 (the
// semantics are restated in include/rsp.h).
//
// k_s3_cfar<T, CPLX>: grid (range chunks, Doppler row blocks, maps), 256 threads.  The device maps
// are range-contiguous per Doppler row, so the window slides along the coalesced axis.  A
// workgroup takes RSP_S3_ROWS Doppler rows of RSP_S3_CH range cells on the map's own column grid
// (so a group of 4 cells is 4-aligned whenever G is a multiple of 4); each of its 4 waves takes
// one row per pass, in LDS rows of its own:
//   1. stage columns [g0 - H, g0 + CH + H), clipped to the map, into LDS as amplitudes (CPLX: the
//      magnitudes of the stage-2 result, by k2_pc's cmag), H = s + r;
//   2. form the mean of every r-cell window that lies in the staged columns once per start column:
//      the r cells added in ascending order, one division -- the leading window of cell y is the
//      trailing window of cell y - (2 s + r + 1), and both read the same entry;
//   3. each lane resolves 4 consecutive cells: the cell's segment decides which of its two windows
//      exist (a window that leaves the segment is replaced by the opposite one, :486-496), max or
//      min, one multiplication by T, A >= threshold;
//   4. thresholds (and the amplitudes, on request) leave as 32-B stores, the flags as 4 packed bytes;
//      hits go to an LDS queue (one LDS atomic per lane) that the workgroup empties after its last
//      pass with one global atomic.  All workgroups bump one counter: with a reservation per 4 rows
//      (15 106 workgroups at the reference frame) the kernel took 0.16 ms whatever it wrote, with one
//      per 16 rows 0.075 - 0.12 ms depending on what it writes, hence 16 rows per
//      workgroup.  More than QCAP hits in a workgroup (a dense map) reserve the rest per lane.
// A window mean is used only when the window lies inside the cell's segment, so staging and the
// means need not know the segments.  Notched rows are written as zeros, so no output needs a memset.
// Every operation is a single IEEE operation of T (no fused multiply-add can form: no product feeds
// an add), `/` is the correctly rounded division (the Makefile passes no fast-math flag, and hipcc's
// default for float is the correctly rounded one).
#include "rsp_device.h"
#include "rsp_cmag.h"
#include <type_traits>

namespace {

constexpr int CH = RSP_S3_CH, ROWS = RSP_S3_ROWS, HMAX = RSP_S3_HMAX, W = CH + 2 * HMAX;
constexpr int WAVES = RSP_THREADS / 64, PASSES = ROWS / WAVES;   // a wave takes one Doppler row per pass
constexpr int QCAP = 512;                                        // hit records of the LDS queue
static_assert(ROWS % WAVES == 0 && CH == 4 * 64 && ROWS <= 256, "one wave per Doppler row, 4 cells per lane");
static_assert(sizeof(rsp_stage3_hit) == 32, "hit record layout");

template <class T, bool CPLX>
__global__ __launch_bounds__(RSP_THREADS) void k_s3_cfar(S3Desc d, const void* __restrict__ in, double* __restrict__ amp,
                                                         double* __restrict__ thr, uint8_t* __restrict__ flags,
                                                         rsp_stage3_hit* __restrict__ hits, int* __restrict__ count,
                                                         int hits_cap) {
    __shared__ T S[WAVES][W];   // amplitudes of columns base .. base + CH + 2 H - 1 of the wave's row
    __shared__ T M[WAVES][W];   // M[j - base]: mean of columns j .. j + r - 1
    __shared__ T q_amp[QCAP], q_thr[QCAP];
    __shared__ int q_cell[QCAP];   // (row in the workgroup) << 8 | column in the chunk
    __shared__ int qn[2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g0 = blockIdx.x * CH, v0 = blockIdx.y * ROWS, map = blockIdx.z;
    const int H = d.H, r = d.r, G = d.G;
    const int base = g0 - H, lo = max(base, 0), hi = min(g0 + CH + H, G);
    const int c4 = g0 + 4 * lane;
    const T Tc = (T)d.T, rn = (T)r;
    if (threadIdx.x == 0) qn[0] = 0;
    for (int pass = 0; pass < PASSES; ++pass) {
        const int vl = pass * WAVES + wave, v = v0 + vl;
        const bool live = v < d.P;                                   // wave-uniform
        const bool notch = live && v >= d.z0 && v <= d.z1;           // wave-uniform
        const size_t rowoff = ((size_t)map * d.P + (live ? v : 0)) * G;
        if (live && (!notch || amp)) {
            // hi - lo <= W = NL * 64 columns: every load of the lane is issued before the first is used
            typedef typename std::conditional<CPLX, cx<T>, T>::type E;
            constexpr int NL = W / 64;
            const E* __restrict__ src = static_cast<const E*>(in) + rowoff;
            E x[NL];
#pragma unroll
            for (int u = 0; u < NL; ++u) {
                const int c = lo + lane + 64 * u;
                if (c < hi) x[u] = src[c];
            }
#pragma unroll
            for (int u = 0; u < NL; ++u) {
                const int c = lo + lane + 64 * u;
                if (c >= hi) continue;
                if constexpr (CPLX) S[wave][c - base] = cmag(x[u]);
                else S[wave][c - base] = x[u];
            }
        }
        __syncthreads();
        if (live && !notch) {
            for (int j = lo + lane; j + r <= hi; j += 64) {
                const T* w = &S[wave][j - base];
                T sum = w[0];
                for (int q = 1; q < r; ++q) sum += w[q];
                M[wave][j - base] = sum / rn;
            }
        }
        __syncthreads();
        T a4[4] = {0, 0, 0, 0}, t4[4] = {0, 0, 0, 0};
        unsigned fl = 0;
        int nh = 0;
        if (live && !notch) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = c4 + i;
                if (c >= G) break;
                const int k = c < d.seg_a[1] ? 0 : (c < d.seg_a[2] ? 1 : 2);
                const int y = c - d.seg_a[k], n = d.seg_n[k];
                const int jl = c - H - base, jr = c + d.s + 1 - base;   // both >= 0; read only when in the segment
                const bool hasl = y >= H, hasr = y + H < n;             // n >= 2 H: at least one of them
                const T ml = M[wave][hasl ? jl : jr], mr = M[wave][hasr ? jr : jl];
                const T u = d.method == 0 ? (ml > mr ? ml : mr) : (ml < mr ? ml : mr);
                const T t = u * Tc, a = S[wave][c - base];
                a4[i] = a;
                t4[i] = t;
                if (a >= t) {
                    fl |= 1u << (8 * i);
                    ++nh;
                }
            }
        } else if (live && amp) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (c4 + i < G) a4[i] = S[wave][c4 + i - base];
        }
        if (live && c4 < G) {
            const size_t o = rowoff + c4;
            if ((G & 3) == 0) {   // whole groups of 4, 4-aligned in every row
                if (thr) *reinterpret_cast<f64x4*>(thr + o) = f64x4{(double)t4[0], (double)t4[1], (double)t4[2], (double)t4[3]};
                if (amp) *reinterpret_cast<f64x4*>(amp + o) = f64x4{(double)a4[0], (double)a4[1], (double)a4[2], (double)a4[3]};
                if (flags) *reinterpret_cast<unsigned*>(flags + o) = fl;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (c4 + i >= G) break;
                    if (thr) thr[o + i] = (double)t4[i];
                    if (amp) amp[o + i] = (double)a4[i];
                    if (flags) flags[o + i] = (uint8_t)((fl >> (8 * i)) & 1u);
                }
            }
        }
        // hits go to the LDS queue; what does not fit (a dense map) reserves its slots per lane
        if (nh) {
            int off = atomicAdd(&qn[0], nh);
            const int over = max(off + nh - max(off, QCAP), 0);   // this lane's hits past the queue
            int gidx = over ? atomicAdd(count, over) : 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (!((fl >> (8 * i)) & 1u)) continue;
                if (off < QCAP) {
                    q_cell[off] = (vl << 8) | (4 * lane + i);
                    q_amp[off] = a4[i];
                    q_thr[off] = t4[i];
                } else {
                    if (hits && gidx >= 0 && gidx < hits_cap)   // counted past the capacity: the host grows the list
                        hits[gidx] = rsp_stage3_hit{v + 1, c4 + i + 1, map + 1, 0, (double)a4[i], (double)t4[i]};
                    ++gidx;
                }
                ++off;
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
hipError_t launch_t(const S3Desc& d, const void* in, int n_maps, double* amp, double* thr, uint8_t* flags,
                    rsp_stage3_hit* hits, int* count, int hits_cap, hipStream_t s) {
    const dim3 grid((d.G + CH - 1) / CH, (d.P + ROWS - 1) / ROWS, n_maps);
    hipLaunchKernelGGL((k_s3_cfar<T, CPLX>), grid, dim3(RSP_THREADS), 0, s, d, in, amp, thr, flags, hits, count, hits_cap);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_s3(const S3Desc& d, int prec, bool cplx, const void* in, int n_maps, double* amp, double* thr,
                     uint8_t* flags, rsp_stage3_hit* hits, int* count, int hits_cap, hipStream_t s) {
    // the kernel's envelope, whatever the caller checked: the tile halo and the grid's y / z limits
    if (d.H < 1 || d.H > HMAX || d.r < 1 || d.r + d.s != d.H || d.P < 1 || d.G < 1 || n_maps < 1 || n_maps > 65535 ||
        (d.P + ROWS - 1) / ROWS > 65535 || !in || !count)
        return hipErrorInvalidValue;
    if (prec == RSP_PREC_F64)
        return cplx ? launch_t<double, true>(d, in, n_maps, amp, thr, flags, hits, count, hits_cap, s)
                    : launch_t<double, false>(d, in, n_maps, amp, thr, flags, hits, count, hits_cap, s);
    return cplx ? launch_t<float, true>(d, in, n_maps, amp, thr, flags, hits, count, hits_cap, s)
                : launch_t<float, false>(d, in, n_maps, amp, thr, flags, hits, count, hits_cap, s);
}
