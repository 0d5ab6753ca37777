// rsp_k3.hip -- K3 of the per-frame radar chain for CDNA4 (gfx950), and its launchers.
//
//   k3_cfar     : |RDM| adjacent-beam sum (fsf:184-187), cross GOCA-CFAR (fsf:192-213),
//                 atomic compaction (fsf:215-221) and S9 spline/monopulse estimation
//                 (fsf:237-290) of each detection.
//   k3_finish   : the band route's deferred cells, after the on-demand K2 of the edge rows.
//   k3_smap     : the adjacent-beam sum maps alone, where no range cell is under test.
//
// Reads the magnitude maps of K2 (rsp_k2.hip).
#include "rsp_device.h"
#include "rsp_k3_arith.h"
#include "rsp_s9.h"   // spline_peak, S9Consts, s9_estimate

namespace {

// ======================================================================================
// K3: GOCA-CFAR on adjacent-beam sums + compaction + S9 estimation
// ======================================================================================
#define K3_QCAP 1024

#define K3_VEC 8       // 16-B loads per beam per thread in flight (halo-less 98-row tiles: 8 -> 120 rows per sweep)
#define RSP_K3_WGS 3   // k3_cfar workgroups per CU the register budget is sized for

constexpr int floor4(int x) { return x >= 0 ? (x & ~3) : -((-x + 3) & ~3); }

// 4 consecutive cells of an S row from LDS (16-B aligned): one ds_read_b128 (float) or two
// (double)
__device__ __forceinline__ void ld4(const float* p, float (&o)[4]) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
    o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
}
__device__ __forceinline__ void ld4(const double* p, double (&o)[4]) {
    const d2 a = *reinterpret_cast<const d2*>(p), b = *reinterpret_cast<const d2*>(p + 2);
    o[0] = a.x; o[1] = a.y; o[2] = b.x; o[3] = b.y;
}
template <class T> struct U16;   // one 16-B unit of a map row
template <> struct U16<float> { typedef f32x4 U; static constexpr int E = 4; };
template <> struct U16<double> { typedef d2 U; static constexpr int E = 2; };

// ---- the CFAR test's arithmetic, shared by k3_cfar and k3_finish: k3_quot, k3_noise2 (rsp_k3_arith.h)
// S(v, r) = |A| + |B| (fsf:184-187) from the magnitude maps of beams pair, pair + 1: the same two
// values and the same add as k3_cfar's tile load
template <class T>
struct K3Maps {
    const T* __restrict__ MA;
    const T* __restrict__ MB;
    int Gp;
    __device__ __forceinline__ T operator()(int vv, int rr) const {
        const size_t o = (size_t)vv * Gp + rr;
        return MA[o] + MB[o];
    }
};
// The four slice sums of cell (v, r) of the compile-time window from the maps, in sum() order.
// has_lv / has_tv false: that Doppler slice is left at 0 (its rows are not in the maps yet).
template <int RR, int RV, int GR, int GV, class T>
__device__ __forceinline__ void k3_map_sums(const K3Maps<T>& sg, int v, int r, T& lr, T& tr, T& lv, T& tv,
                                            bool has_lv = true, bool has_tv = true) {
    lr = 0; tr = 0; lv = 0; tv = 0;
    for (int qq = 0; qq < RR; ++qq) lr += sg(v, r - (GR + RR) + qq);
    for (int qq = 0; qq < RR; ++qq) tr += sg(v, r + GR + 1 + qq);
    for (int qq = 0; qq < RV; ++qq) {
        if (has_lv) lv += sg(v + qq - GV - RV, r);
        if (has_tv) tv += sg(v + qq + GV + 1, r);
    }
}

// ---- the band route (K2 of the rows under test, the edge rows on demand) ---------------------
// A cell whose test or S9 reads a row outside [hV, P - hV): its Doppler slices reach hV rows up and
// down, S9 two.
__device__ __forceinline__ bool k3_edge_cell(int v, int P) {
    return v < 2 * RSP_K3_FAST_HV || v >= P - 2 * RSP_K3_FAST_HV;
}
// K3_DEFER: an edge cell that passes the test on the slices it has (below) goes on the frame's deferred list (the count keeps
// counting past the capacity; the host grows the list and runs the phases again), and the edge rows
// its slices (v - hV .. v - hV + refV - 1 and the mirror) and S9 (v - 2 .. v + 2) read are flagged
// for both beams of the pair.
__device__ __forceinline__ void k3_defer_cell(const FramePtrs& fp, int f, int P, int pair, int v, int r, int cap) {
    constexpr int hV = RSP_K3_FAST_HV;
    const int i = atomicAdd(fp.count[f] + 1, 1);
    if (i < cap) fp.defer[f][i] = int2{(pair << 16) | v, r};
    unsigned char* need = fp.need[f] + pair * 2 * hV;
#pragma unroll 1
    for (int q = 0; q < 15; ++q) {
        const int vv = q < 5 ? v - hV + q : (q < 10 ? v + hV - 9 + q : v - 12 + q);   // left slice, right slice, S9
        const int e = vv < hV ? vv : vv - (P - 2 * hV);   // edge row index, when vv is one
        if (vv >= 0 && vv < P && (vv < hV || vv >= P - hV)) need[e] = need[2 * hV + e] = 1;
    }
}

// RR/RV/GR/GV = reference/guard cell counts when known at compile time (the reference's
// 5/5/10/10, v8:45-46), 0 = runtime; RTC = the tile width g.cfar_RT when they are (32 or 64),
// so that the LDS row stride and every window offset are compile-time constants.  Tiles: RT
// range cells x all P Doppler cells of one beam pair, tile starts aligned to 4 cells so that
// the magnitude rows load as 16-B units.
// DEFER (the band route's first phase, FAST only; the maps then hold rows [hV, P - hV) alone): a
// prefilter survivor at an edge cell (k3_edge_cell) is not tested here but left to k3_finish
// (k3_defer_cell); every other cell goes through exactly the code of the whole kernel.
template <class T, int RR, int RV, int GR, int GV, int RTC, bool DEFER = false>
__global__ __launch_bounds__(RSP_THREADS, RSP_K3_WGS) void k3_cfar(Geometry g, DevConsts k, FramePtrs fp, int defer_cap) {
    T* S = reinterpret_cast<T*>(rsp_lds);   // [P][W] | queue[K3_QCAP] | qn, base
    typedef typename U16<T>::U U;
    constexpr int EPU = U16<T>::E;
    constexpr bool FAST = RR > 0 && RV > 0 && GR > 0 && GV > 0 && (RTC == 32 || RTC == 64);
    static_assert(!DEFER || (FAST && RV + GV == RSP_K3_FAST_HV && RR == RV), "the band route follows the 5/5/10/10 window");
    // FAST (the compile-time 5/5/10/10 kernel): the tile holds the band's own cells only, no halo;
    // the prefilter takes whichever range slice lies inside the tile, survivors and S9 read the
    // rest from the maps.  The generic kernel's tile holds the halo (g.cfar_W, g.cfar_hR).
    // FAST rows: RTC cells; complex double rows get 2 extra cells (stride 132 dwords = 4 mod 64
    // banks), see the row-group order of the CFAR loop
    constexpr int WC = ((RTC + 3) & ~3) + (sizeof(T) == 8 ? 2 : 0);
    // XCD-aware order (bijective swizzle, cdna_hip_programming.md T1): the workgroups that
    // share an XCD take consecutive (tile, pair) ids with pairs fastest, so beam b's tile --
    // read by pairs b-1 and b -- and the range halos of neighbouring tiles are L2 hits
    const int npair = g.B - 1, ntile = k3_ntiles(g);
    int wg = blockIdx.x;
    {
        const int nwg = gridDim.x, xcd = wg & 7, q = nwg >> 3, rm = nwg & 7;
        wg = (xcd < rm ? xcd * (q + 1) : rm * (q + 1) + (xcd - rm) * q) + (wg >> 3);
    }
    const int pair = wg % npair, col = wg / npair;
    const int tile = col % ntile, col2 = col / ntile;
    const int band = col2 % g.cfar_nband, f = col2 / g.cfar_nband;
    const int P = g.P, G = g.G, W = FAST ? WC : g.cfar_W, hR = FAST ? 0 : g.cfar_hR, RT = FAST ? RTC : g.cfar_RT;
    const int rR = RR ? RR : g.refR, gR = GR ? GR : g.guardR, rV = RV ? RV : g.refV, gV = GV ? GV : g.guardV;
    const int rc0 = rR + gR;                           // first cell under test (0-based)
    const int tstart = (rc0 & ~3) + tile * RT;         // multiple of 4
    const int c0 = tstart - hR;                        // tile column 0 (multiple of 4; may be < 0)
    const int cut_lo = max(tstart, rc0), cut_hi = min(tstart + RT, G - rc0);
    // Doppler band: cells under test in rows [v0, v1), the tile holds rows [vt0, vt1) (the
    // band alone when FAST, else plus the rV + gV window rows on each side; bands of one tile
    // column tile the map)
    const int hV = rV + gV;
    const int v0 = hV + band * g.cfar_VB, v1 = min(hV + (band + 1) * g.cfar_VB, P - hV);
    const int vt0 = FAST ? v0 : max(v0 - hV, 0), vt1 = FAST ? max(v1, v0) : min(v1 + hV, P), nv = vt1 - vt0;
    int* queue = reinterpret_cast<int*>(S + g.cfar_rows * W);
    int* qn = queue + K3_QCAP;
    const T* Sv = S - vt0 * W;                         // row v of the map at Sv + v W
    const int Gp = g.Gp;
    const T* __restrict__ MA = static_cast<const T*>(fp.mag[f]) + (size_t)pair * P * Gp;   // |RDM| of beams pair, pair+1
    const T* __restrict__ MB = MA + (size_t)P * Gp;
    const cx<T>* __restrict__ RA = g.mono_c ? static_cast<const cx<T>*>(fp.rdm[f]) + (size_t)pair * P * G : nullptr;
    const cx<T>* __restrict__ RB = RA ? RA + (size_t)P * G : nullptr;
    // S(v, r) from the maps: the same two values and the same add as the tile load below
    const K3Maps<T> sg{MA, MB, Gp};
    if (threadIdx.x == 0) qn[0] = 0;
    // ---- load S = |A| + |B| (fsf:184-187) from the magnitude maps: 16 B per lane,
    //      K3_VEC units of each beam in flight per thread
    if constexpr (FAST) {
        // a thread keeps one 16-B column unit and walks the rows: one address add per load
        constexpr int WU = WC / EPU, NTR = RSP_THREADS / WU;
        const int u = threadIdx.x % WU, rr = threadIdx.x / WU;
        const int r = c0 + EPU * u;
        const bool colok = rr < NTR && r >= 0 && r < G;   // rows are padded to Gp: r + EPU - 1 < Gp
        const T* pa = MA + (size_t)(vt0 + rr) * Gp + r;
        const T* pb = MB + (size_t)(vt0 + rr) * Gp + r;
        U* sd = reinterpret_cast<U*>(S + rr * WC) + u;
        // complex single: the two maps as buffer resources, a unit outside the tile gets an
        // out-of-range offset (bit 31) and reads 0 -- no branch around a load, so the 2 K3_VEC
        // loads of a sweep are in flight together
        const unsigned mbytes = (unsigned)((size_t)P * Gp * sizeof(T));
        const __amdgpu_buffer_rsrc_t ra = buf_rsrc(MA, mbytes), rbm = buf_rsrc(MB, mbytes);
        const unsigned base = colok ? (unsigned)(((size_t)(vt0 + rr) * Gp + r) * sizeof(T)) : RSP_OOB;
        const unsigned rowb = (unsigned)Gp * (unsigned)sizeof(T);
        for (int vb = 0; vb < nv; vb += K3_VEC * NTR) {
            U xa[K3_VEC], xb[K3_VEC];
#pragma unroll
            for (int q = 0; q < K3_VEC; ++q) {
                if constexpr (sizeof(T) == 4) {   // complex double: plain loads (35.0 vs 36.0 us)
                    const unsigned bad = (unsigned)(nv - 1 - (vb + rr + q * NTR)) & 0x80000000u;
                    const unsigned off = (base + (unsigned)(vb + q * NTR) * rowb) | bad;
                    xa[q] = __builtin_bit_cast(U, __builtin_amdgcn_raw_buffer_load_b128(ra, (int)off, 0, 0));
                    xb[q] = __builtin_bit_cast(U, __builtin_amdgcn_raw_buffer_load_b128(rbm, (int)off, 0, 0));
#pragma unroll
                    for (int e = 1; e < EPU; ++e)   // the row pad past G (Gp > G) is not written by K2
                        if (r + e >= G) { xa[q][e] = 0; xb[q][e] = 0; }
                    continue;
                }
                xa[q] = U{};
                xb[q] = xa[q];
                if (colok && vb + rr + q * NTR < nv) {
                    xa[q] = *reinterpret_cast<const U*>(pa + (size_t)(vb + q * NTR) * Gp);
                    xb[q] = *reinterpret_cast<const U*>(pb + (size_t)(vb + q * NTR) * Gp);
#pragma unroll
                    for (int e = 1; e < EPU; ++e)
                        if (r + e >= G) { xa[q][e] = 0; xb[q][e] = 0; }
                }
            }
#pragma unroll
            for (int q = 0; q < K3_VEC; ++q)
                if (rr < NTR && vb + rr + q * NTR < nv) sd[(vb + q * NTR) * WU] = xa[q] + xb[q];
        }
    } else {
        const int WU = W / EPU, nu = nv * WU;
        for (int e0 = 0; e0 < nu; e0 += K3_VEC * RSP_THREADS) {
            U xa[K3_VEC], xb[K3_VEC];
#pragma unroll
            for (int u = 0; u < K3_VEC; ++u) {
                const int e = e0 + threadIdx.x + u * RSP_THREADS;
                xa[u] = U{};
                xb[u] = xa[u];
                if (e < nu) {
                    const int vl = e / WU, r = c0 + EPU * (e - vl * WU), v = vt0 + vl;
                    if (r >= 0 && r < G) {   // rows are padded to Gp (multiple of 4): r + EPU - 1 < Gp
                        xa[u] = *reinterpret_cast<const U*>(MA + (size_t)v * Gp + r);
                        xb[u] = *reinterpret_cast<const U*>(MB + (size_t)v * Gp + r);
#pragma unroll
                        for (int q = 1; q < EPU; ++q)
                            if (r + q >= G) { xa[u][q] = 0; xb[u][q] = 0; }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < K3_VEC; ++u) {
                const int e = e0 + threadIdx.x + u * RSP_THREADS;
                if (e < nu) reinterpret_cast<U*>(S)[e] = xa[u] + xb[u];
            }
        }
    }
    __syncthreads();
    if (fp.smap[f]) {   // on request: rdm_for_cfar_all as thresholded here, [pair][v][r]
        T* sm = static_cast<T*>(fp.smap[f]) + (size_t)pair * P * G;
        const int wlo = tile == 0 ? 0 : tstart, whi = tile == ntile - 1 ? G : min(tstart + RT, G);
        const int vlo = band == 0 ? 0 : v0, vhi = band == g.cfar_nband - 1 ? P : v1;   // inside [vt0, vt1)
        const int nwc = whi - wlo;
        for (int e = threadIdx.x; e < (vhi - vlo) * nwc; e += RSP_THREADS) {
            const int v = vlo + e / nwc, r = wlo + (e - (v - vlo) * nwc);
            sm[(size_t)v * G + r] = FAST ? sg(v, r) : Sv[v * W + (r - c0)];
        }
    }
    if (v1 <= v0 || cut_hi <= cut_lo) return;
    const double Tc = g.T;
    // mean() = sum / n over the slices of fsf:197-203: k3_quot, k3_noise2
    const T fR = (T)rR, fV = (T)rV;
    const T iR = (T)1 / fR, iV = (T)1 / fV;
    auto quot = [&](T x, T fn, T in) -> T { return k3_quot(x, fn, in); };
    auto noise2 = [&](T lr, T tr, T lv, T tv) -> T { return k3_noise2<FAST && RR == RV>(lr, tr, lv, tv, fR, iR, fV, iV); };
    const S9Consts s9c{k.range_axis, k.velocity_axis, k.beam_angles, k.klut, k.deltaR, k.deltaV};
    // hits past the LDS queue are only counted here (qn keeps counting); the overflow pass below
    // finds them again
#define K3_HIT(V, C, CUT, LR, TR, LV, TV)                                                               \
    do {                                                                                                \
        if ((CUT) > (T)Tc * noise2(LR, TR, LV, TV)) {                                                   \
            const int qi = atomicAdd(qn, 1);                                                            \
            if (qi < K3_QCAP) queue[qi] = ((V) << 16) | (C);                                            \
        }                                                                                               \
    } while (0)
    // ---- cross GOCA-CFAR (fsf:192-213); hits go to an LDS queue so that the S9 work is
    //      spread over the whole workgroup instead of serialising in the lane that owns a range cell
    if constexpr (FAST) {   // RT = 32: long-P / double tiles (LDS cap in the plan)
        // a thread takes 4 adjacent range cells of one Doppler row: every window value comes
        // from 16-B LDS reads; sums run left to right over each slice like mean()
        constexpr int DL = -(GR + RR), DR = GR + 1;              // window starts rel. to the cell
        constexpr int BL = floor4(DL);
        constexpr int NL = (DL + 3 + RR - BL + 3) / 4;
        constexpr int lgT = RTC == 64 ? 4 : 3;                    // log2 threads per row (RT / 4)
        // 16-lane row groups of a wave take rows {0, 2, 1, 3} + 4w: the ds_read_b128 lane groups
        // ({0-3,12-15,20-27}, ... MI355X_MICROARCH.md §LDS) then pair rows 2 apart, 2W = 192
        // floats = 0 mod 64 banks, conflict-free (adjacent rows, W = 96 = 32 mod 64, were 2-way)
        const int rg = threadIdx.x >> lgT;
        // complex double (8 threads per row, 32 B per thread, two ds_read_b128 of 16 lanes from 4
        // row groups; row stride 34 doubles, so a 16-B slot's bank is (row + 2 q + base / 2) mod
        // 16 slots): row groups 4a + {0, 1, 2, 3} take rows {0, 1, 8, 9} + 2 (a mod 4) + 16 (a / 4),
        // and their column groups q are rotated by {0, 4, 4, 0}, so that each ds_read_b128 lane
        // group holds four rows {0, 1, 8, 9} (+ x) of ONE half of the columns (q < 4 or q >= 4).
        // Every lane of a group then reads at the same offset (the halo-less prefilter's right
        // slice is read by q < 4 only, the left one by q >= 4), and rows + 2 q cover the 16 slots
        // once.  (Rows 2a + {0, 16, 1, 17} with unrotated columns put the two slices in one lane
        // group: 2-way on a quarter of the slots, 30 % of K3's LDS cycles.)
        const int q = lgT == 3 ? ((threadIdx.x & 7) ^ (((rg ^ (rg >> 1)) & 1) << 2)) : threadIdx.x & ((1 << lgT) - 1);
        const int c = 4 * q;                                      // first tile column of the group
        const int r = c0 + c;
        const int rgp = lgT == 4 ? (rg & ~3) | ((rg & 1) << 1) | ((rg >> 1) & 1)
                                 : (rg & 1) + ((rg & 2) << 2) + 2 * ((rg >> 2) & 3) + 16 * (rg >> 4);
        // Exact prefilter.  A hit needs CUT > T mean(max of the four slices) >= T mean(left range
        // slice): quot() is the correctly rounded (double) or a monotone (float) quotient and the
        // product with T > 0 rounds monotonically, so a cell with CUT <= T quot(lr) cannot be a
        // hit.  That test needs one range slice alone (4 ld4 per 4 cells, where the full window
        // took 27: the CFAR phase was bound by LDS bandwidth); the rare survivors (T = 8 on
        // amplitude sums: cells near targets) run the full test on the maps with the sums in
        // sum() order, so the detection list is the one the full test gives.  A NaN sum never
        // rejects (the comparison is false).
        {
            const T Tt = (T)Tc;
            const bool pf = Tc > 0.0;   // the bound needs T > 0; otherwise every cell takes the full test
            // The tile has no halo: lanes whose 4 cells start in the first 16 tile columns test the
            // right range slice (cells c + 11 .. c + 15 + 3 <= 30 < RT), the others the left one
            // (c - 15 >= 1): either is a lower bound of the max.  The right slice's loads start at
            // c + OR so that both slices sit at the same register offsets when the alignment allows
            // (ld4 of double: 2 cells; of float: 4 cells, so float selects between offsets 1 and 3)
            static_assert(RR == 5 && GR == 10 && NL == 3 && BL == -16, "slice constants for the 5/10 window");
            constexpr int OR = sizeof(T) == 8 ? 10 : 8, XR = DR - OR;   // XR: register offset of the right slice
            const bool useR = q < 4;
            const int base = useR ? OR : BL;
#pragma unroll 1
            for (int v = v0 + rgp; v < v1; v += RSP_THREADS >> lgT) {
                const T* row = Sv + v * WC + c;
                T xl[4 * NL], cv[4];
#pragma unroll
                for (int j = 0; j < NL; ++j) {
                    T t[4];
                    ld4(row + base + 4 * j, t);
#pragma unroll
                    for (int i = 0; i < 4; ++i) xl[4 * j + i] = t[i];
                }
                ld4(row, cv);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    T lr = 0;   // the left or the right slice sum (a lower bound either way)
#pragma unroll
                    for (int qq = 0; qq < RR; ++qq) {
                        const T xa = xl[i + DL - BL + qq];
                        if constexpr (XR != DL - BL) lr += useR ? xl[i + XR + qq] : xa;
                        else lr += xa;
                    }
                    const int ri = r + i;
                    if (ri >= cut_lo && ri < cut_hi && (!pf || !(cv[i] <= Tt * quot(lr, fR, iR)))) {
                        // DEFER: the Doppler slice below a cell with v < 2 hV, or above one with
                        // v >= P - 2 hV, lies in rows the maps do not hold yet.  The noise level is
                        // a monotone function of the largest slice sum (sums of magnitudes, >= 0), so
                        // a cell that fails the test on the slices it has cannot be a hit (the
                        // prefilter's argument, T > 0); one that passes waits for k3_finish.
                        const bool no_lv = DEFER && v < 2 * RSP_K3_FAST_HV, no_tv = DEFER && v >= P - 2 * RSP_K3_FAST_HV;
                        T tr, lv, tv;   // every slice from the maps, in sum() order
                        k3_map_sums<RR, RV, GR, GV>(sg, v, ri, lr, tr, lv, tv, !no_lv, !no_tv);
                        if (no_lv || no_tv) {
                            if (!pf || !(cv[i] <= Tt * noise2(lr, tr, lv, tv))) k3_defer_cell(fp, f, P, pair, v, ri, defer_cap);
                        } else {
                            K3_HIT(v, c + i, cv[i], lr, tr, lv, tv);
                        }
                    }
                }
            }
        }
    } else {
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;   // 4 waves
        for (int rb = cut_lo; rb < cut_hi; rb += 64) {
            const int r = rb + lane;
            if (r >= cut_hi) continue;
            const int c = r - c0;
            for (int v = v0 + wv; v < v1; v += 4) {
                const T* rowp = Sv + v * W;
                T lr = 0, tr = 0, lv = 0, tv = 0;
                const T* lrp = rowp + c - gR - rR;
                const T* trp = rowp + c + gR + 1;
                const T* lvp = Sv + (v - gV - rV) * W + c;
                const T* tvp = Sv + (v + gV + 1) * W + c;
                for (int qq = 0; qq < rR; ++qq) {
                    lr += lrp[qq];
                    tr += trp[qq];
                }
                for (int qq = 0; qq < rV; ++qq) {
                    lv += lvp[qq * W];
                    tv += tvp[qq * W];
                }
                K3_HIT(v, c, rowp[c], lr, tr, lv, tv);
            }
        }
    }
#undef K3_HIT
    __syncthreads();
    const int nhit = qn[0], n = min(nhit, K3_QCAP);
    if (n == 0) return;
    if (threadIdx.x == 0) qn[1] = atomicAdd(fp.count[f], n);   // one global reservation per workgroup
    __syncthreads();
    const int base = qn[1];
    // S(v, r) as the CFAR test read it: FAST, the maps (survivors and S9 never read the tile);
    // else the tile.  The generic tile's Doppler halo is the window's rV + gV rows; S9 reads rows
    // v - 2 .. v + 2, so with rV + gV = 1 a hit on a band's first or last row reaches one row past
    // the tile (the rows of the neighbouring band, outside this tile's LDS): those come from the
    // maps, the same two values and the same add.  The range halo is never narrower than 2
    // (derive_k3_tiling).
    auto st = [&](int vv, int rr) -> T {
        if constexpr (FAST) return sg(vv, rr);
        else return vv >= vt0 && vv < vt1 ? Sv[vv * W + (rr - c0)] : sg(vv, rr);
    };
    for (int i = threadIdx.x; i < n; i += RSP_THREADS) {
        const int idx = base + i;
        if (idx >= g.max_dets) break;   // counted; the host grows the list and runs K3 again
        const int e = queue[i];
        const int v = e >> 16, c = e & 0xFFFF;
        s9_estimate<T>(s9c, st, P, G, Gp, v, c0 + c, pair, MA, MB, RA, RB, &fp.dets[f][idx]);
    }
    if (nhit <= K3_QCAP) return;   // uniform
    // Overflow pass (more than K3_QCAP hits in this tile: a cluttered frame or a low T_CFAR).  The
    // list holds every hit, like all_raw_detections(end+1, :) (fsf:215-221): the queued cells are
    // marked in a bitmap over the tile's cells under test (in the queue's LDS), and every other
    // cell is tested again, with the same sums in the same order as above, so the same cells hit;
    // each unmarked hit reserves its slot and runs S9.  Outside the CFAR loop, so the common path
    // keeps its registers and schedule (an in-loop spill call cost K3 25 %).
    constexpr int HELD = K3_QCAP / RSP_THREADS;
    int held[HELD];
#pragma unroll
    for (int u = 0; u < HELD; ++u) held[u] = queue[threadIdx.x + u * RSP_THREADS];
    __syncthreads();
    unsigned* bm = reinterpret_cast<unsigned*>(queue);   // ncr x (v1 - v0) bits <= K3_QCAP x 32
    const int ncr = cut_hi - cut_lo, ncell = (v1 - v0) * ncr;
#pragma unroll
    for (int u = 0; u < HELD; ++u) bm[threadIdx.x + u * RSP_THREADS] = 0u;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < HELD; ++u) {
        const int v = held[u] >> 16, r = c0 + (held[u] & 0xFFFF);
        const int bit = (v - v0) * ncr + (r - cut_lo);
        atomicOr(&bm[bit >> 5], 1u << (bit & 31));
    }
    __syncthreads();
    for (int e = threadIdx.x; e < ncell; e += RSP_THREADS) {
        if (bm[e >> 5] >> (e & 31) & 1u) continue;
        const int v = v0 + e / ncr, r = cut_lo + (e - (e / ncr) * ncr);
        if (DEFER && k3_edge_cell(v, P)) continue;   // deferred or ruled out by the loop above
        T lr = 0, tr = 0, lv = 0, tv = 0;
        for (int qq = 0; qq < rR; ++qq) {
            lr += st(v, r - gR - rR + qq);
            tr += st(v, r + gR + 1 + qq);
        }
        for (int qq = 0; qq < rV; ++qq) {
            lv += st(v + qq - gV - rV, r);
            tv += st(v + qq + gV + 1, r);
        }
        if (st(v, r) > (T)Tc * noise2(lr, tr, lv, tv)) {
            const int idx = atomicAdd(fp.count[f], 1);
            if (idx < g.max_dets) s9_estimate<T>(s9c, st, P, G, Gp, v, r, pair, MA, MB, RA, RB, &fp.dets[f][idx]);
        }
    }
}

// The band route's last phase, after the on-demand K2: the full test of each deferred cell through
// the same sums in the same order as k3_cfar's survivors, the same noise level and the same S9; hits
// join the frame's detection list.  Grid (K3_FIN_WGS, frames): a fixed small grid that strides over
// the list, whose length only the device knows.
#define K3_FIN_WGS 4
template <class T, int RR, int RV, int GR, int GV>
__global__ __launch_bounds__(RSP_THREADS) void k3_finish(Geometry g, DevConsts k, FramePtrs fp, int defer_cap) {
    const int f = blockIdx.y, P = g.P, G = g.G, Gp = g.Gp;
    const int n = min(fp.count[f][1], defer_cap);   // past the capacity: counted, the host runs the phases again
    const T fR = (T)RR, fV = (T)RV, iR = (T)1 / fR, iV = (T)1 / fV;
    const S9Consts s9c{k.range_axis, k.velocity_axis, k.beam_angles, k.klut, k.deltaR, k.deltaV};
    for (int i = blockIdx.x * RSP_THREADS + threadIdx.x; i < n; i += K3_FIN_WGS * RSP_THREADS) {
        const int2 e = fp.defer[f][i];
        const int pair = e.x >> 16, v = e.x & 0xFFFF, r = e.y;
        const T* MA = static_cast<const T*>(fp.mag[f]) + (size_t)pair * P * Gp;
        const K3Maps<T> sg{MA, MA + (size_t)P * Gp, Gp};
        T lr, tr, lv, tv;
        k3_map_sums<RR, RV, GR, GV>(sg, v, r, lr, tr, lv, tv);
        if (sg(v, r) > (T)g.T * k3_noise2<RR == RV>(lr, tr, lv, tv, fR, iR, fV, iV)) {
            const int idx = atomicAdd(fp.count[f], 1);
            if (idx < g.max_dets)
                s9_estimate<T>(s9c, sg, P, G, Gp, v, r, pair, sg.MA, sg.MB, (const cx<T>*)nullptr, (const cx<T>*)nullptr,
                               &fp.dets[f][idx]);
        }
    }
}

// rdm_for_cfar_all alone, for a range window that leaves no cell under test (G <= 2 (rR + gR):
// k3_cfar has no tile then): S = |A| + |B| of every cell, the add k3_cfar's tile load makes.
// Grid: (cells / RSP_THREADS, pairs, frames).
template <class T>
__global__ __launch_bounds__(RSP_THREADS) void k3_smap(Geometry g, FramePtrs fp) {
    const int pair = blockIdx.y, f = blockIdx.z, e = blockIdx.x * RSP_THREADS + threadIdx.x;
    if (!fp.smap[f] || e >= g.P * g.G) return;
    const int v = e / g.G, r = e - v * g.G;
    const T* MA = static_cast<const T*>(fp.mag[f]) + (size_t)pair * g.P * g.Gp;
    const T* MB = MA + (size_t)g.P * g.Gp;
    static_cast<T*>(fp.smap[f])[(size_t)pair * g.P * g.G + e] = MA[(size_t)v * g.Gp + r] + MB[(size_t)v * g.Gp + r];
}

}  // namespace

template <class T>
static hipError_t launch_k3_p(const Geometry& g, const DevConsts& k, const FramePtrs& fp, int nf, hipStream_t s, int phase,
                              int defer_cap) {
    const size_t lds = (size_t)g.cfar_rows * g.cfar_W * sizeof(T) + (K3_QCAP + 4) * sizeof(int);
    const dim3 grid(k3_ntiles(g) * g.cfar_nband * (g.B - 1) * nf);   // 1-D; k3_cfar remaps it XCD-aware
    const bool ref = k3_fast_params(g);   // the reference's cfar_params (v8:45-46); the plan sized the tile for it
    if (phase != K3_WHOLE && !ref) return hipErrorInvalidValue;   // the band route is the compile-time kernel's
    if (phase == K3_FINISH)
        return launch(k3_finish<T, 5, 5, 10, 10>, dim3(K3_FIN_WGS, nf), dim3(RSP_THREADS), 0, s, g, k, fp, defer_cap);
    const auto kernel = phase == K3_DEFER ? (g.cfar_RT == 64 ? k3_cfar<T, 5, 5, 10, 10, 64, true>
                                                             : k3_cfar<T, 5, 5, 10, 10, 32, true>)
                        : ref && g.cfar_RT == 64 ? k3_cfar<T, 5, 5, 10, 10, 64>
                        : ref && g.cfar_RT == 32 ? k3_cfar<T, 5, 5, 10, 10, 32>
                                                 : k3_cfar<T, 0, 0, 0, 0, 0>;
    return launch(kernel, grid, dim3(RSP_THREADS), lds, s, g, k, fp, defer_cap);
}

hipError_t launch_k3(const Geometry& g, const DevConsts& k, const FramePtrs& fp, int nf, hipStream_t s, int phase,
                     int defer_cap) {
    if (g.B < 2) return hipSuccess;
    if (g.G - 2 * (g.refR + g.guardR) <= 0) {   // no range cell under test: no detections, the maps on request
        bool want = false;
        for (int f = 0; f < nf; ++f) want = want || fp.smap[f];
        if (!want) return hipSuccess;
        const dim3 grid((g.P * g.G + RSP_THREADS - 1) / RSP_THREADS, g.B - 1, nf);
        if (g.prec == RSP_PREC_F64) hipLaunchKernelGGL(k3_smap<double>, grid, dim3(RSP_THREADS), 0, s, g, fp);
        else hipLaunchKernelGGL(k3_smap<float>, grid, dim3(RSP_THREADS), 0, s, g, fp);
        return hipGetLastError();
    }
    return g.prec == RSP_PREC_F64 ? launch_k3_p<double>(g, k, fp, nf, s, phase, defer_cap)
                                  : launch_k3_p<float>(g, k, fp, nf, s, phase, defer_cap);
}
