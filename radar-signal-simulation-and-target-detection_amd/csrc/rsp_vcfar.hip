// rsp_vcfar.hip -- Doppler cell-averaging CFAR of the stage-2 path for gfx950: local_cfar_detector of
// main_simulate_echoes_with_array_v3.m:278-314 (the semantics are restated in include/rsp.h).
//
// k_vcfar<T, CPLX>: grid (range column strips, Doppler row blocks, maps), 256 threads.  The device
// maps are range-contiguous per Doppler row, so this window slides along the strided axis: a
// workgroup takes RSP_VC_ROWS Doppler rows of a strip of RSP_VC_COLS consecutive range columns,
//   1. stages rows [v0 - halo, v0 + ROWS + halo), clipped to the map, of the strip into LDS as
//      amplitudes (CPLX: the magnitudes of the stage-2 result, by k2_pc's cmag), halo = r + h: a row
//      per wave and step, each a contiguous segment along G, NLD rows of loads in flight per wave.  The
//      tile is dynamic LDS sized by the halo in use;
//   2. resolves a row per wave and step, lanes across the columns (LDS reads of consecutive words:
//      conflict-free): the row decides the two windows for the whole wave, every lane adds the cells
//      of its column in the order rsp.h fixes, divides once (CA) or once per window (GOCA, SOCA),
//      multiplies by T, A > threshold;
//   3. amplitudes (on request), thresholds and flags leave as whole row segments of the strip; hits
//      go to an LDS queue (one LDS atomic per wave and row, slots by ballot) that the workgroup empties
//      at the end with one global atomic; hits beyond QCAP in a workgroup (a dense map) are reserved
//      per wave and row on the global counter.  Hits are counted past hits_cap.
// Every operation is a single IEEE operation of T (no product feeds an add, so no fused multiply-add
// can form), `/` is the correctly rounded division (rsp_stage3.hip says why).
#include "rsp_device.h"
#include "rsp_cmag.h"
#include <type_traits>

namespace {

constexpr int COLS = RSP_VC_COLS, ROWS = RSP_VC_ROWS, HMAX = RSP_VC_HMAX;
constexpr int WAVES = RSP_THREADS / 64;
constexpr int QCAP = 512;   // hit records of the LDS queue
constexpr int NLD = 4;      // rows of loads a wave has in flight while staging
static_assert(COLS == 64 && ROWS % WAVES == 0 && ROWS <= 256, "a lane per column, a wave per row and step");
static_assert(sizeof(rsp_stage3_hit) == 32, "hit record layout");

extern __shared__ __align__(16) unsigned char vc_tile[];

template <class T, bool CPLX>
__global__ __launch_bounds__(RSP_THREADS) void k_vcfar(VcDesc d, const void* __restrict__ in, double* __restrict__ amp,
                                                       double* __restrict__ thr, uint8_t* __restrict__ flags,
                                                       rsp_stage3_hit* __restrict__ hits, int* __restrict__ count,
                                                       int hits_cap) {
    T* S = reinterpret_cast<T*>(vc_tile);   // S[(row - tb) * COLS + column - g0]
    __shared__ T q_amp[QCAP], q_thr[QCAP];
    __shared__ int q_cell[QCAP];   // (row in the workgroup) << 8 | column in the strip
    __shared__ int qn[2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g0 = blockIdx.x * COLS, v0 = blockIdx.y * ROWS, map = blockIdx.z;
    const int P = d.P, G = d.G, r = d.r, h = d.h;
    const int tb = max(v0 - d.halo, 0), te = min(v0 + ROWS + d.halo, P);   // staged rows [tb, te)
    const int c = g0 + lane;
    const bool incol = c < G;
    const size_t mapoff = (size_t)map * P * G;
    const T Tc = (T)d.T;
    if (threadIdx.x == 0) qn[0] = 0;
    {
        typedef typename std::conditional<CPLX, cx<T>, T>::type E;
        const E* __restrict__ src = static_cast<const E*>(in) + mapoff + c;
        for (int t0 = tb + wave; t0 < te; t0 += NLD * WAVES) {
            E x[NLD];
#pragma unroll
            for (int u = 0; u < NLD; ++u) {
                const int t = t0 + u * WAVES;
                if (t < te && incol) x[u] = src[(size_t)t * G];
            }
#pragma unroll
            for (int u = 0; u < NLD; ++u) {
                const int t = t0 + u * WAVES;
                if (t >= te || !incol) continue;
                if constexpr (CPLX) S[(t - tb) * COLS + lane] = cmag(x[u]);
                else S[(t - tb) * COLS + lane] = x[u];
            }
        }
    }
    __syncthreads();
    const auto cell = [&](int row) -> T { return S[(row - tb) * COLS + lane]; };   // the lane's column, by map row
    // acc + rows [b, b + n) of the lane's column in ascending order, one add per row (have false:
    // the sum starts from the first row); n and have are wave-uniform
    const auto add_rows = [&](int b, int n, T& acc, bool& have) {
        for (int q = 0; q < n; ++q) {
            const T x = cell(b + q);
            acc = have ? acc + x : x;
            have = true;
        }
    };
    for (int vl = wave; vl < ROWS; vl += WAVES) {
        const int v = v0 + vl;
        if (v >= P) break;   // wave-uniform, as the windows below
        const int gs = max(v - h, 0), l0 = max(gs - r, 0), nL = gs - l0;      // lead rows [l0, gs)
        const int t0 = min(v + h, P - 1) + 1, nT = min(t0 + r, P) - t0;       // trail rows [t0, t0 + nT)
        T a = 0, t = 0;
        bool hit = false;
        if (incol) {
            a = cell(v);
            T noise = 0;
            if (d.method == 0) {   // one running sum over both windows, one division
                T sum = 0;
                bool have = false;
                add_rows(l0, nL, sum, have);
                add_rows(t0, nT, sum, have);
                if (have) noise = sum / (T)(nL + nT);
            } else {
                T sL = 0, sT = 0;
                bool haveL = false, haveT = false;
                add_rows(l0, nL, sL, haveL);
                add_rows(t0, nT, sT, haveT);
                const T mL = haveL ? sL / (T)nL : (T)0, mT = haveT ? sT / (T)nT : (T)0;
                if (haveL && haveT) noise = d.method == 1 ? (mL > mT ? mL : mT) : (mL < mT ? mL : mT);
                else noise = haveL ? mL : mT;   // one side empty: the other; both: 0
            }
            t = noise * Tc;
            hit = a > t;
            const size_t o = mapoff + (size_t)v * G + c;
            if (thr) thr[o] = (double)t;
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
hipError_t launch_t(const VcDesc& d, const void* in, int n_maps, double* amp, double* thr, uint8_t* flags,
                    rsp_stage3_hit* hits, int* count, int hits_cap, hipStream_t s) {
    const size_t lds = vc_lds_bytes(d.halo, sizeof(T));
    constexpr size_t queue = QCAP * (2 * sizeof(T) + sizeof(int)) + 2 * sizeof(int);   // the static LDS
    if (lds + queue > RSP_LDS_BYTES) return hipErrorInvalidValue;
    // launch() opts the tile in where it exceeds 64 KiB; at halo <= HMAX tile and queue stay below (48 + 10 KiB)
    static_assert(vc_lds_bytes(HMAX, sizeof(double)) + QCAP * 20 + 8 <= 64 * 1024, "no opt-in inside the envelope");
    const dim3 grid((d.G + COLS - 1) / COLS, (d.P + ROWS - 1) / ROWS, n_maps);
    return launch(k_vcfar<T, CPLX>, grid, dim3(RSP_THREADS), lds, s, d, in, amp, thr, flags, hits, count, hits_cap);
}

}  // namespace

hipError_t launch_vcfar(const VcDesc& d, int prec, bool cplx, const void* in, int n_maps, double* amp, double* thr,
                        uint8_t* flags, rsp_stage3_hit* hits, int* count, int hits_cap, hipStream_t s) {
    // the kernel's envelope, whatever the caller checked: the tile halo, the 32-bit cell index of the
    // hit counter and the grid's y / z limits
    if (d.r < 1 || d.h < 0 || d.r + d.h != d.halo || d.halo > HMAX || d.method < 0 || d.method > 2 || d.P < 1 || d.G < 1 ||
        n_maps < 1 || n_maps > 65535 || (d.P + ROWS - 1) / ROWS > 65535 ||
        (long long)n_maps * d.P * d.G >= (1ll << 31) || hits_cap < 0 || !in || !count)
        return hipErrorInvalidValue;
    if (prec == RSP_PREC_F64)
        return cplx ? launch_t<double, true>(d, in, n_maps, amp, thr, flags, hits, count, hits_cap, s)
                    : launch_t<double, false>(d, in, n_maps, amp, thr, flags, hits, count, hits_cap, s);
    return cplx ? launch_t<float, true>(d, in, n_maps, amp, thr, flags, hits, count, hits_cap, s)
                : launch_t<float, false>(d, in, n_maps, amp, thr, flags, hits, count, hits_cap, s);
}
