// rsp_detect.hip -- detection on any complex range-Doppler cube for gfx950: the adjacent-beam sum maps
// (fsf:184-187) and S9 of a device hit list (fsf:237-297) as kernels of their own, around the cross
// GOCA-CFAR k_xcfar (rsp_xcfar.hip).  The semantics are restated in include/rsp.h.
//
// k_pairsum<T, LAYOUT>: S[pair][v][g] = cmag(x(v, g, pair)) + cmag(x(v, g, pair + 1)), one rounded add in T,
// range-contiguous: the layout k_xcfar and S9 read.  K3's bits: the magnitudes are k2_pc's (rsp_cmag.h) and
// the add is k3_cfar's.  Every cube element is read from HBM once: a thread keeps beam b's magnitudes in
// registers for the pair (b, b + 1).
//   DET_LAYOUT_MATLAB, x [V x G x B] with the Doppler index fastest: grid (range tiles, Doppler tiles), 256
//     threads.  A workgroup takes ROWS = 64 Doppler rows of COLS = 64 range cells and walks the beams.  Loads
//     run along v, 16 bytes per lane (one complex double; two complex singles where the columns start on 16
//     bytes, i.e. V even and an aligned base -- else one per lane, xc_stage's rule); stores run along g, a
//     lane per range cell.  Between them the beam's magnitudes turn through an LDS tile m[v][g] of ROWS rows
//     of COLS + 1 elements.  The padding rule: the row stride is odd in elements.  Writes (a lane group
//     holds one column g, rows v ascending) then hit banks stride * v: 32 distinct banks for the 32 lanes of a
//     ds_write_b32 group with one float per lane, 16 distinct even banks (two banks each) for the 16 lanes of
//     a ds_write_b64 group; with two floats per lane the rows of a group are 2 apart and 2 lanes share a bank,
//     which a ds_write_b32 absorbs (MI355X_MICROARCH.md, LDS: 2-way costs a store nothing).  Reads (a wave
//     holds one row, lanes across g) are consecutive words.  The next beam's loads are issued before the
//     stores of the current pair.
//   DET_LAYOUT_DEVICE, x [B][V][G] (the stage-2 result): element-wise, a thread per 16-byte unit of a plane
//     (G % EPU == 0 and an aligned base, else per element), walking the beams.
// Tails along v and g are predicated; nothing is padded.
//
// k_s9<T, LAYOUT>: a lane per hit of k_xcfar's device list, in whatever order it is.  s9_estimate (rsp_s9.h:
// K3's S9) with S read from the maps in global memory and the monopulse inputs taken from the two cube
// elements at the integer cell: their magnitudes (cmag again; no magnitude cube exists) or the complex values.
#include "rsp_device.h"
#include "rsp_cmag.h"
#include "rsp_s9.h"

namespace {

constexpr int TV = RSP_PS_ROWS, TG = RSP_PS_COLS, LW = TG + RSP_PS_PAD;
constexpr int WAVES = RSP_THREADS / 64;
static_assert(TG == 64 && TV % WAVES == 0 && (TG * TV) % (2 * RSP_THREADS) == 0, "a lane per range cell, a wave per row and step");
static_assert(LW % 2 == 1, "the padding rule: an odd row stride");
static_assert(sizeof(rsp_stage3_hit) == 32 && sizeof(DevDet) == 48, "record layouts");

template <class E, int N>
struct alignas(sizeof(E) * N) Pack {   // N consecutive elements: one load or store
    E e[N];
};

template <class T, int N>
__device__ __forceinline__ void ps_matlab(const DetDesc& d, const cx<T>* __restrict__ x, T* __restrict__ S) {
    typedef Pack<cx<T>, N> U;
    constexpr int UV = TV / N;                    // units of a tile column
    constexpr int NU = TG * UV / RSP_THREADS;     // units per thread
    constexpr int NR = TV / WAVES;                // rows per thread on the store side
    T* tile = reinterpret_cast<T*>(rsp_lds);      // m[TV][LW]
    const int V = d.V, G = d.G, B = d.B;
    const int g0 = blockIdx.x * TG, v0 = blockIdx.y * TV;
    const size_t plane = (size_t)V * G;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // load side: unit u = thread + k 256 is rows N (u % UV) .. of column u / UV (N > 1: V is even, so a unit
    // lies inside the map or outside it as a whole)
    U xin[NU];
    auto load = [&](int b) {
        const cx<T>* __restrict__ xb = x + (size_t)b * plane;
#pragma unroll
        for (int k = 0; k < NU; ++k) {
            const int u = threadIdx.x + k * RSP_THREADS, g = g0 + u / UV, v = v0 + N * (u % UV);
            xin[k] = U{};
            if (g < G && v < V) xin[k] = *reinterpret_cast<const U*>(xb + (size_t)g * V + v);
        }
    };
    T prev[NR];
    const bool gok = g0 + lane < G;
    load(0);
    for (int b = 0; b < B; ++b) {
#pragma unroll
        for (int k = 0; k < NU; ++k) {
            const int u = threadIdx.x + k * RSP_THREADS;
            T* dst = tile + N * (u % UV) * LW + u / UV;
#pragma unroll
            for (int e = 0; e < N; ++e) dst[e * LW] = cmag(xin[k].e[e]);
        }
        __syncthreads();
        if (b + 1 < B) load(b + 1);   // in flight across the stores of pair b - 1
        T* __restrict__ out = S + (size_t)(b > 0 ? b - 1 : 0) * plane + (size_t)v0 * G + g0 + lane;
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            const int vl = wave + k * WAVES;
            const T m = tile[vl * LW + lane];
            if (b > 0 && gok && v0 + vl < V) out[(size_t)vl * G] = prev[k] + m;
            prev[k] = m;
        }
        __syncthreads();   // the tile is read before the next beam's magnitudes replace it
    }
}

template <class T, int N>
__device__ __forceinline__ void ps_device(const DetDesc& d, const cx<T>* __restrict__ x, T* __restrict__ S) {
    typedef Pack<cx<T>, N> U;
    typedef Pack<T, N> R;
    const size_t plane = (size_t)d.V * d.G, nu = plane / N;   // N > 1: G % N == 0
    const size_t u = (size_t)blockIdx.x * RSP_THREADS + threadIdx.x;
    if (u >= nu) return;
    const U* __restrict__ xu = reinterpret_cast<const U*>(x) + u;
    R* __restrict__ su = reinterpret_cast<R*>(S) + u;
    U cur = xu[0];
    R prev{};
    for (int b = 0; b < d.B; ++b) {
        U nxt = cur;
        if (b + 1 < d.B) nxt = xu[(size_t)(b + 1) * nu];
        R m, s;
#pragma unroll
        for (int e = 0; e < N; ++e) {
            m.e[e] = cmag(cur.e[e]);
            s.e[e] = prev.e[e] + m.e[e];
        }
        if (b > 0) su[(size_t)(b - 1) * nu] = s;
        prev = m;
        cur = nxt;
    }
}

template <class T, int LAYOUT>
__global__ __launch_bounds__(RSP_THREADS) void k_pairsum(DetDesc d, const void* __restrict__ xin, void* __restrict__ Sout) {
    constexpr int EPU = 16 / sizeof(cx<T>);
    const cx<T>* x = static_cast<const cx<T>*>(xin);
    T* S = static_cast<T*>(Sout);
    if constexpr (LAYOUT == DET_LAYOUT_MATLAB) {
        if (EPU > 1 && d.vec) ps_matlab<T, EPU>(d, x, S);
        else ps_matlab<T, 1>(d, x, S);
    } else {
        if (EPU > 1 && d.vec) ps_device<T, EPU>(d, x, S);
        else ps_device<T, 1>(d, x, S);
    }
}

// s9_estimate reads the monopulse inputs of cell (v, r) as map[v G + r] of four maps: the magnitudes and
// the complex values of beams pair and pair + 1.  Here each of them is one value of the hit's own (no
// magnitude cube exists, and the MATLAB layout is not v G + r): the "map" whose element v G + r is that
// value.  The address is formed in integers; only element v G + r of it is ever read.
template <class E>
__device__ __forceinline__ const E* s9_cell_view(const E* value, size_t cell) {
    return reinterpret_cast<const E*>(reinterpret_cast<uintptr_t>(value) - cell * sizeof(E));
}

template <class T, int LAYOUT>
__global__ __launch_bounds__(RSP_THREADS) void k_s9(DetDesc d, S9Consts k, const void* __restrict__ xin, const void* __restrict__ Sin,
                                                    const rsp_stage3_hit* __restrict__ hits, int n, DevDet* __restrict__ dets) {
    const int i = blockIdx.x * RSP_THREADS + threadIdx.x;
    if (i >= n) return;
    const rsp_stage3_hit h = hits[i];
    const int V = d.V, G = d.G, v = h.v_idx - 1, r = h.r_idx - 1, pair = h.beam_idx - 1;
    if (v < 0 || v >= V || r < 0 || r >= G || pair < 0 || pair >= d.B - 1) return;   // not a record of this cube's detector
    const size_t plane = (size_t)V * G;
    const T* __restrict__ Sp = static_cast<const T*>(Sin) + (size_t)pair * plane;
    auto sval = [&](int vv, int rr) -> T { return Sp[(size_t)vv * G + rr]; };
    const size_t cell = (size_t)v * G + r;
    const cx<T>* __restrict__ xp = static_cast<const cx<T>*>(xin) + (size_t)pair * plane +
                                   (LAYOUT == DET_LAYOUT_MATLAB ? (size_t)r * V + v : cell);
    const cx<T> xa = xp[0], xb = xp[plane];
    const T ma = cmag(xa), mb = cmag(xb);
    s9_estimate<T>(k, sval, V, G, G, v, r, pair, s9_cell_view(&ma, cell), s9_cell_view(&mb, cell),
                   d.cplx ? s9_cell_view(&xa, cell) : nullptr, d.cplx ? s9_cell_view(&xb, cell) : nullptr, &dets[i]);
}

template <class T>
hipError_t pairsum_t(const DetDesc& d, int layout, const void* x, void* S, hipStream_t s) {
    if (layout == DET_LAYOUT_MATLAB) {
        const dim3 grid((d.G + TG - 1) / TG, (d.V + TV - 1) / TV);
        return launch(k_pairsum<T, DET_LAYOUT_MATLAB>, grid, dim3(RSP_THREADS), ps_lds_bytes(sizeof(T)), s, d, x, S);
    }
    const size_t nu = (size_t)d.V * d.G / (d.vec ? 16 / sizeof(cx<T>) : 1);
    return launch(k_pairsum<T, DET_LAYOUT_DEVICE>, dim3((unsigned)((nu + RSP_THREADS - 1) / RSP_THREADS)), dim3(RSP_THREADS), 0, s, d,
                  x, S);
}

template <class T>
hipError_t s9_t(const DetDesc& d, int layout, const S9Consts& k, const void* x, const void* S, const rsp_stage3_hit* hits, int n,
                DevDet* dets, hipStream_t s) {
    const dim3 grid((n + RSP_THREADS - 1) / RSP_THREADS);
    if (layout == DET_LAYOUT_MATLAB)
        return launch(k_s9<T, DET_LAYOUT_MATLAB>, grid, dim3(RSP_THREADS), 0, s, d, k, x, S, hits, n, dets);
    return launch(k_s9<T, DET_LAYOUT_DEVICE>, grid, dim3(RSP_THREADS), 0, s, d, k, x, S, hits, n, dets);
}

// The envelope both launchers check, whatever the caller checked: shapes, the layout, a cube and maps of
// fewer than 2^31 elements (the kernels' plane offsets are size_t; the grids are not)
bool det_ok(const DetDesc& d, int layout, const void* x, const void* S) {
    return d.V >= 1 && d.G >= 1 && d.B >= 2 && (long long)d.V * d.G * d.B < (1ll << 31) && (d.V + TV - 1) / TV <= 65535 &&
           (layout == DET_LAYOUT_MATLAB || layout == DET_LAYOUT_DEVICE) && x && S;
}

}  // namespace

hipError_t launch_pairsum(DetDesc d, int prec, int layout, const void* x, void* S, hipStream_t s) {
    if (!det_ok(d, layout, x, S)) return hipErrorInvalidValue;
    // 16-byte units of two complex singles: where the units of every column (MATLAB layout: V even) or of
    // every plane (device layout: G even, which makes V G even) start on 16 bytes; S then starts on 8
    const int len = layout == DET_LAYOUT_MATLAB ? d.V : d.G;
    d.vec = prec != RSP_PREC_F64 && len % 2 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)S % 8 == 0 ? 1 : 0;
    return prec == RSP_PREC_F64 ? pairsum_t<double>(d, layout, x, S, s) : pairsum_t<float>(d, layout, x, S, s);
}

hipError_t launch_s9(const DetDesc& d, int prec, int layout, const DevConsts& k, const void* x, const void* S,
                     const rsp_stage3_hit* hits, int n, DevDet* dets, hipStream_t s) {
    if (!det_ok(d, layout, x, S) || n < 0 || (n > 0 && (!hits || !dets))) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const S9Consts s9c{k.range_axis, k.velocity_axis, k.beam_angles, k.klut, k.deltaR, k.deltaV};
    return prec == RSP_PREC_F64 ? s9_t<double>(d, layout, s9c, x, S, hits, n, dets, s)
                                : s9_t<float>(d, layout, s9c, x, S, hits, n, dets, s);
}
