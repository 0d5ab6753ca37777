// rsp_geometry.h -- the device-free half of a plan: the descriptors the kernels take as arguments,
// every sizing and routing decision (sample windows, overlap-save blocks, the K1 tile and route,
// the K2 job list and dispatch order, the K3 tiling) and the host tables a plan uploads.  Plain
// C++17: no HIP header, so that rsp_geometry.cpp builds and runs (and is sanitized) without a GPU.
#pragma once
#include "rsp.h"

#include <complex>
#include <stddef.h>
#include <stdint.h>
#include <vector>

// Helpers the kernels call too; empty under a plain C++ compiler.
#ifdef __HIPCC__
#define RSP_HD __host__ __device__
#else
#define RSP_HD
#endif

#define RSP_MAX_F 8          // frames batched per launch
#define RSP_K2_POINTS 4096   // complex points per pulse-compression workgroup (Geometry::k2_pts)
#define RSP_K2_MIXPTS 2560   // Geometry::k2_pts of a complex-double plan with a 2560-point block
#define K1_THREADS 512       // threads per K1 workgroup (8 waves)

// Arithmetic of a plan: every device buffer, table and operation of the chain is in one of
// these.  PREC_F64 is MATLAB's complex double (the reference's arithmetic, fsf:47,92,101,131);
// PREC_F32 is complex single (an explicitly narrower option).
#define RSP_PREC_F32 0
#define RSP_PREC_F64 1

// LDS of a gfx950 compute unit: the most one workgroup can request.
constexpr size_t RSP_LDS_BYTES = 160 * 1024;

// Pulse-compression segment (fsf:105-126).  Output gates [ga, gb) of the stitched
// row come from this segment.  x~(n) = x(n) for lo_eff <= n <= hi, else 0, where
// [lo, hi] is the window of samples that reach a kept gate (plan-time analysis).
struct SegDesc {
    int type;        // 0 = direct FIR (narrow, fsf:111-112), 1 = FFT overlap-save (fsf:115-120)
    int ga, gb;      // stitched gate range
    int seg_lo;      // 0-based first sample of the segment (seg_start - 1)
    int lo, hi;      // needed sample window (0-based, inclusive), lo >= seg_lo
    int off;         // compacted sample index of `lo`
    // direct FIR: y[g] = sum_j h[j] x~(seg_lo + k - j), k = (g + delay) mod Ls
    int ntaps, delay, Ls, taps_off;
    // FFT overlap-save: y[g] = sum_{j<Lh} h[j] x~(seg_lo + g - j), block size M = 2^logM,
    // V = M-Lh+1 valid outputs per block
    int Lh, M, logM, V, nblocks, H_off, tw_off;
    int rows_per_wg;
};

// One group of pulse-compression workgroups: segment `seg`, overlap-save block `blk`.
struct K2Job {
    int seg, blk, wg_begin, wg_count;
};

// One pulse-compression workgroup, in dispatch order: record blockIdx.x of the table a plan uploads
// (DevConsts::k2rec) is everything k2_pc needs to find its work -- one 16-byte scalar load instead of
// the dispatch-order lookup followed by a search of the job list.  wg = the workgroup's index in
// job order (jobs[].wg_begin + its position in the job); row0 = its first row of the B x P row set.
struct K2Rec {
    int seg, blk, row0, wg;
};

// The rows of one k2_pc launch: row i of the set, i < total = B n, is Doppler row
// v = base + j + (j >= split ? gap : 0), j = i mod n, of beam b = i / n.  Three sets: every row
// (n = P); the band of rows K3's compile-time window tests, [hV, P - hV); the edge rows around it,
// [0, hV) and [P - hV, P), which the fast path computes only where a detection reads them.
struct K2Rows {
    int n, base, split, gap, total;
};
// rho = b P + v of row i: the row's index in z, the RD map and the magnitude map.  Everything a
// row's workgroup computes depends on rho alone, whichever set, launch or workgroup holds it.
RSP_HD inline int k2_rho(const K2Rows& s, int P, int i) {
    const int b = i / s.n, j = i - b * s.n;
    return b * P + s.base + j + (j >= s.split ? s.gap : 0);
}
enum { K2SET_ALL = 0, K2SET_BAND = 1, K2SET_EDGE = 2 };
// hV of the compile-time 5/5/10/10 window, the one the band route exists for
#define RSP_K3_FAST_HV 15
// beams whose edge-row flags fit a frame's flag block (2 hV bytes per beam)
#define RSP_NEED_BMAX 16
#define RSP_NEED_BYTES (RSP_NEED_BMAX * 2 * RSP_K3_FAST_HV)

#define RSP_MAX_SEG 3
#define RSP_MAX_JOBS 16
#define RSP_MAX_IVL 4

struct Geometry {
    int prec;        // RSP_PREC_F32 / RSP_PREC_F64
    int C, B, P, N, G;
    int cpitch;      // device cube channel pitch in complex samples (= N*P)
    int Gp;          // row stride of the magnitude maps (G rounded up to 4)
    int NT, nU, ntiles, Ppad;
    int NZ, nzc;     // z layout: NZ compacted samples per (row, chunk) slab, nzc chunks per row
    int twPp_elems;  // per-pass twiddles of the P-point FFT
    int pow2P, logP;
    // non-power-of-two P = rqR * rqQ (rqR = 2 or 4, rqQ odd >= 3): K1's factored slow-time DFT
    // (k1_dft_rq); rqQ = 0: the direct O(P^2) DFT.  twq_elems = complex entries of its
    // frequency-set twiddle table (DevConsts::twQ)
    int rqR, rqQ, twq_elems;
    int nseg, njobs, nwg_k2;
    // complex points of LDS rows per pulse-compression workgroup: RSP_K2_POINTS, or 2560 in a
    // complex-double plan with a 2560-point block (4 workgroups per CU: 40 KB of LDS each, no pads);
    // power-of-two blocks then take 2048 / M rows
    int k2_pts;
    int cfar_RT, cfar_hR, cfar_W;
    int cfar_VB, cfar_nband, cfar_rows;   // K3 Doppler bands: cells under test per band, bands, tile rows
    int refR, guardR, refV, guardV;
    double T;        // T_CFAR
    int max_dets;    // detection-list capacity per frame of the launch (grows on demand, rsp_plan.cpp)
    int ncu;         // compute units of the device (persistent K1 grid)
    int k1_tiled;    // force the one-tile-per-workgroup K1 (RSP_PLAN_K1_TILED, parity tests)
    int mono_c;      // S9 angle from the complex ratio of the RD map (RSP_PLAN_MONOPULSE_COMPLEX)
    // used fast-time samples as <= RSP_MAX_IVL intervals: compacted n' in [ivl_start[q],
    // ivl_start[q+1]) is sample ivl_lo[q] + n' - ivl_start[q] (kernel-argument lookup, no
    // dependent global load before the cube loads)
    int nivl, ivl_lo[RSP_MAX_IVL], ivl_start[RSP_MAX_IVL];
    // pulse-compression segment and job tables travel as kernel arguments too
    SegDesc segs[RSP_MAX_SEG];
    K2Job jobs[RSP_MAX_JOBS];
};
// Geometry is a kernel argument: the host and the device compiler must lay it out alike.
static_assert(sizeof(SegDesc) == 76 && sizeof(K2Job) == 16 && sizeof(Geometry) == 680, "kernel-argument layout");
static_assert(sizeof(K2Rec) == 16, "one 16-byte scalar load per workgroup");

// K3's compile-time path: the reference's cfar_params (v8:45-46) and a 32/64-cell tile
RSP_HD inline bool k3_fast_params(const Geometry& g) {
    return g.refR == 5 && g.refV == 5 && g.guardR == 10 && g.guardV == 10 && (g.cfar_RT == 32 || g.cfar_RT == 64);
}

// K3 tiles: range cells from the first cell under test rounded down to 4, cfar_RT per tile
// (k3_cfar, launch_k3, rsp_profile_stages).
RSP_HD inline int k3_ntiles(const Geometry& g) {
    const int rc0 = g.refR + g.guardR;
    return (g.G - rc0 - (rc0 & ~3) + g.cfar_RT - 1) / g.cfar_RT;
}

// Magnitude-map bytes K3 reads from HBM per frame (the K3 stage's algorithmic bytes): on the
// fast path the halo-less tiles hold only the Doppler rows under test, P - 2 (refV + guardV), over
// the tiled range columns (first cell under test rounded down to 4, k3_ntiles * cfar_RT cells,
// clipped to G); each beam's map is read by two pairs, the second read an L2 hit (XCD-aware
// order).  The general path reads whole maps.  bench.py / tests/test_bench_args.py restate it.
RSP_HD inline long long k3_map_bytes(const Geometry& g, int real_bytes) {
    if (k3_fast_params(g)) {
        const int hV = g.refV + g.guardV, c0 = (g.refR + g.guardR) & ~3;
        const int rows = g.P - 2 * hV > 0 ? g.P - 2 * hV : 0;
        const int c1 = c0 + k3_ntiles(g) * g.cfar_RT < g.G ? c0 + k3_ntiles(g) * g.cfar_RT : g.G;
        return (long long)g.B * rows * (c1 > c0 ? c1 - c0 : 0) * real_bytes;
    }
    return (long long)g.B * g.P * g.G * real_bytes;
}

// Workgroups per CU that K2's instantiation is sized for: k2_pc<T, 4> for the 2560-point
// workgroups, k2_pc<T, 2> for RSP_K2_POINTS (launch_k2_p, rsp_fill_k2_layout).
RSP_HD inline int k2_wg_per_cu(const Geometry& g) { return g.k2_pts != RSP_K2_POINTS ? 4 : 2; }

struct SynthTarget {          // per-target constants of S4 (fsf:51-73), host-computed
    int delay;                // delay_samples
    double amp;
    double fd_prt;            // doppler_freq * prt   (phase per pulse / 2pi)
    double dphi;              // channel phase step (rad)
};
#define RSP_MAX_SYNTH_TARGETS 64
struct SynthTargets {         // by value in the kernel arguments (2 KiB): no upload, no sync
    SynthTarget t[RSP_MAX_SYNTH_TARGETS];
};

// Frequencies per wave-uniform set of the factored slow-time DFT's Q-point stage (k1_dft_rq)
#define RQ_RK 6
// Complex LDS entries of k1_dft_rq's tables, twQ | W_P^i.  Pass 2 prefetches the table rows of
// the step after its last one: up to 2 RQ_RK entries past a frequency set's rows, which for the
// last set lie in W_P^i.  P < 2 RQ_RK (P = 6: Q = 3) would end them past W_P^i, so the request
// is never smaller than the prefetch reaches (P >= 12: exactly twq_elems + P).
inline int rq_table_elems(int twq_elems, int P) { return twq_elems + (P > 2 * RQ_RK ? P : 2 * RQ_RK); }

// LDS pad shift of a pulse-compression workgroup's rows (one pad per 32 points; k2_sh in
// rsp_k2.hip says why) and the complex LDS slots of pts points with their pads.
constexpr int RSP_K2_SH = 5;
RSP_HD constexpr int k2_lds_data(int pts, int sh) { return pts + (pts >> sh); }

// ---- radix plans of the Stockham FFTs (K1's slow-time FFT, K2's overlap-save blocks) ----------
// The one description of a transform's passes: the kernels instantiate their passes from it and the
// host builds the twiddle tables from it.  A plan reaches a template as a type with a static
// constexpr member `p` (C++17 has no class-type template parameters).
struct RadixPlan {
    int np;       // passes
    int rad[4];   // radix of pass q < np
};
RSP_HD constexpr int clog2(int x) { return x <= 1 ? 0 : 1 + clog2(x >> 1); }
// 2^m points: radix-16 passes, the remainder as 8 / 4 (m = 5 -> 8 x 4; never a lone radix-2 pass
// unless m = 1)
RSP_HD constexpr RadixPlan plan_pow2(int m) {
    RadixPlan p{0, {1, 1, 1, 1}};
    while (m > 0) {
        const int b = (m == 5) ? 3 : (m >= 4 ? 4 : m);
        p.rad[p.np++] = 1 << b;
        m -= b;
    }
    return p;
}
// The overlap-save block of 2^m points: a 3-pass plan takes its last two radices in the other order
// (2048 = 16 x 8 x 16, 1024 = 16 x 4 x 16): a palindrome, so the inverse FFT runs the same radices,
// and both Ns = 1 passes -- the forward first pass and the inverse first pass fused into the
// forward last one -- are radix 16, whose stride-16 stores are at most 2-way conflicted
// (tools/ab/lds_conflicts64.py).
RSP_HD constexpr RadixPlan plan_os_pow2(int m) {
    RadixPlan p = plan_pow2(m);
    if (p.np == 3) {
        const int t = p.rad[1];
        p.rad[1] = p.rad[2];
        p.rad[2] = t;
    }
    return p;
}
// The mixed-radix overlap-save block 2560 = 16 x 10 x 16: one block covers x2's long segment
// (Lh = 700, 1860 gates), which takes two 2048-point blocks in powers of two -- 37.5% fewer points.
RSP_HD constexpr RadixPlan plan_os_2560() { return RadixPlan{3, {16, 10, 16, 1}}; }
// The same radices in reverse order: the inverse FFT of an overlap-save block, so that its first
// pass consumes exactly the elements the forward FFT's last pass leaves in each thread's registers.
RSP_HD constexpr RadixPlan plan_rev(RadixPlan p) {
    RadixPlan r{p.np, {1, 1, 1, 1}};
    for (int q = 0; q < p.np; ++q) r.rad[q] = p.rad[p.np - 1 - q];
    return r;
}
// Ns before pass q: the product of the earlier radices (q = np: the transform's length)
RSP_HD constexpr int plan_ns(RadixPlan p, int q) {
    int ns = 1;
    for (int i = 0; i < q; ++i) ns *= p.rad[i];
    return ns;
}
RSP_HD constexpr int plan_len(RadixPlan p) { return plan_ns(p, p.np); }
// Twiddle entries per butterfly index k of a radix-R pass: full rows W^(k r), r = 1 .. R - 1, or
// (cmp) compact tables W^(k 2^i), 2^i < R (load_tw in rsp_fft_passes.h)
RSP_HD constexpr int tw_row(int R, bool cmp) { return cmp ? clog2(R - 1) + 1 : R - 1; }
// Offset of pass q's table inside the plan's concatenated per-pass tables: pass i >= 1 owns Ns_i rows
// of tw_row(R_i) entries (pass 0: Ns = 1, no twiddles); q = np: the tables' total
RSP_HD constexpr int plan_tw_off(RadixPlan p, int q, bool cmp) {
    int off = 0;
    for (int i = 1; i < q; ++i) off += plan_ns(p, i) * tw_row(p.rad[i], cmp);
    return off;
}
RSP_HD constexpr int plan_tw_total(RadixPlan p, bool cmp) { return plan_tw_off(p, p.np, cmp); }
// The reversed plan's tables equal the forward ones (the conjugation happens in load_tw)
RSP_HD constexpr bool plan_is_palindrome(RadixPlan p) {
    for (int q = 0; q < p.np; ++q)
        if (p.rad[q] != p.rad[p.np - 1 - q]) return false;
    return true;
}
template <int LG> struct PlanPow2 { static constexpr RadixPlan p = plan_pow2(LG); };
template <int M> struct PlanOs { static constexpr RadixPlan p = M == 2560 ? plan_os_2560() : plan_os_pow2(clog2(M)); };
template <class P> struct PlanRev { static constexpr RadixPlan p = plan_rev(P::p); };

// K1's launch configuration for C channels and B beams: the template arguments CP (channels padded
// to the MFMA's groups of 4) and BMAX of the K1 kernels, NJ channel groups, MB MFMA row blocks of
// 8 beams and TPW sub-tiles per wave of a load round (16 16-B registers per lane).  The Atab
// layout, the route, the LDS sizes and the launchers' template dispatch all read this.
struct K1Cfg {
    int CP, BMAX, NJ, MB, TPW;
    // the persistent K1 has 2 TPW instantiations only where their loads stay within 16 16-B
    // registers per lane and 4 sub-tiles (x4: 2 x 8 channels); elsewhere they would spill
    bool twice_ok;
};
constexpr K1Cfg k1_cfg(int C, int B) {
    const int cp = C <= 8 ? 8 : (C <= 16 ? 16 : 32), bmax = B <= 4 ? 4 : (B <= 8 ? 8 : 16);
    const int nj = cp / 4, mb = bmax <= 8 ? 1 : 2, tpw = (16 / nj) / mb > 0 ? (16 / nj) / mb : 1;
    return K1Cfg{cp, bmax, nj, mb, tpw, 2 * tpw * nj <= 16 && 2 * tpw <= 4};
}

// The DBF's MFMA A operands per lane, [MB][CP/4][Re, Im][64] reals (MB, CP: k1_cfg(C, B)): lane l of
// block (mb, j) holds A[row l & 15][channel 4 j + (l >> 4)], entry 0 the coefficient of Re x_c and
// entry 1 that of Im x_c in the row's part of y_b = sum_c a[b][c] x_c, a = conj(W) (conj != 0, fsf:95)
// or W; W column-major B x C, interleaved (re, im).  Padded beams and channels: zeros.  Which
// (beam, part) row m of block mb is:
//   DBF_ROWS_SPLIT  beam 8 mb + (m & 7), part m >> 3 (0 Re, 1 Im): K1's, and k_dbf's in complex double
//   DBF_ROWS_PAIR   beam 8 mb + (m >> 1), part m & 1: k_dbf's in complex single
enum { DBF_ROWS_SPLIT = 0, DBF_ROWS_PAIR = 1 };
void rsp_dbf_atab(const double* W, int B, int C, int conj, int layout, std::vector<double>& atab);

// ---- the stand-alone DBF (k_dbf, rsp_dbf.hip) ----
// A workgroup of RSP_DBF_THREADS / 64 waves takes RSP_DBF_ROUNDS rounds of TPW sub-tiles per wave
// (TPW = K1Cfg::TPW) of 16 (complex double) or 32 (complex single) positions each.
#define RSP_DBF_THREADS 256
#define RSP_DBF_ROUNDS 2
struct DbfDesc {          // kernel argument
    int S, C, B;          // positions (P N), channels, beams
    int pitch, opitch;    // complex elements between channel planes / beam planes (even in complex single)
    unsigned in_bytes, out_bytes;   // C pitch and B opitch elements: the buffer resources' range
};
RSP_HD constexpr int dbf_sub_tile(int prec) { return prec == RSP_PREC_F64 ? 16 : 32; }
RSP_HD constexpr int dbf_wg_positions(int C, int B, int prec) {
    return (RSP_DBF_THREADS / 64) * RSP_DBF_ROUNDS * k1_cfg(C, B).TPW * dbf_sub_tile(prec);
}
RSP_HD constexpr int dbf_workgroups(int S, int C, int B, int prec) {
    return (S + dbf_wg_positions(C, B, prec) - 1) / dbf_wg_positions(C, B, prec);
}
// The plane pitch rsp_dbf gives its own device buffers: S, rounded up to even in complex single
// (16-B loads and stores of position pairs)
RSP_HD constexpr int dbf_pitch(int S, int prec) { return prec == RSP_PREC_F64 ? S : (S + 1) & ~1; }
// The checks of rsp_dbf / rsp_profile_dbf / rsp_dbf_describe that need no device: sizes (P, N >= 1,
// 1 <= C <= 32, 1 <= B <= 16, the plan's envelope), precision, and that either side of the kernel
// stays within the 32-bit offsets of a buffer resource.  RSP_OK, or the refusal with its message set.
int rsp_dbf_check_sizes(int64_t P, int64_t N, int64_t C, int64_t B, int precision);
// ... and of the call's pointers and dtype
int rsp_dbf_check_args(const void* plan, const void* cube, int dtype, const void* W, const void* out);
// The kernel argument for planes at `pitch` / `opitch` elements (sizes already checked)
DbfDesc dbf_desc(int S, int C, int B, int pitch, int opitch, int prec);

// ---- the stand-alone MTD of any length (k_mtd_any, rsp_mtd.hip) ----
// A workgroup holds `cols` columns of L points in LDS, L = nfft (a power of two) or the chirp-z
// length M = the least power of two >= 2 nfft - 1, and transforms them with the Stockham passes of
// PlanPow2<log2 L>, 16 points per thread.  Complex double: 1024 points, 16 KB and one wave per
// workgroup, so that a pass's barrier costs nothing and nine workgroups share a CU's LDS; complex
// single: 4096 points, 32 KB and four waves (measured against 2048 points in either precision,
// profiles/mtd_prof.json and DESIGN.md section 3h).  Never more than RSP_MTD_MAX_COLS columns, so that
// short transforms do not turn a narrow map into one workgroup; a row longer than a workgroup's points is
// one column, up to the 4096 complex doubles (64 KB + pads) of nfft = 2047.  Rows carry K2's pad, one
// element per 32 (RSP_K2_SH).
#define RSP_MTD_MAX_COLS 16
#define RSP_MTD_MAX_LG 12   // M of nfft = 2047
RSP_HD constexpr int mtd_wg_points(int prec) { return prec == RSP_PREC_F64 ? 1024 : 4096; }
RSP_HD constexpr int mtd_cols(int L, int prec) {
    return mtd_wg_points(prec) / L < 1 ? 1 : (mtd_wg_points(prec) / L > RSP_MTD_MAX_COLS ? RSP_MTD_MAX_COLS : mtd_wg_points(prec) / L);
}
RSP_HD constexpr int mtd_threads(int L, int prec) {
    return mtd_cols(L, prec) * L / 16 < 64 ? 64 : (mtd_cols(L, prec) * L / 16 > 256 ? 256 : mtd_cols(L, prec) * L / 16);
}
RSP_HD constexpr int mtd_row_stride(int L) { return k2_lds_data(L, RSP_K2_SH); }
RSP_HD constexpr size_t mtd_lds_bytes(int L, int prec) {
    return (size_t)mtd_cols(L, prec) * mtd_row_stride(L) * (prec == RSP_PREC_F64 ? 16 : 8);
}
// The chirp-z length of nfft: the least power of two >= 2 nfft - 1
RSP_HD constexpr int mtd_chirp_len(int nfft) {
    int M = 1;
    while (M < 2 * nfft - 1) M *= 2;
    return M;
}
struct MtdDesc {          // kernel argument
    int P, G, n_maps, nfft;
    int L, lgL, chirp;    // points of the LDS transform, its log2, 1 on the chirp-z route
    int cols, col_tiles;  // columns per workgroup, workgroups per map
    int shift, has_win;
    int vec;              // complex single: bit 0 the loads, bit 1 the stores take element pairs (16 B)
};
// The checks of rsp_mtd / rsp_mtd_device / rsp_profile_mtd / rsp_mtd_describe that need no device:
// precision, sizes (nfft = 0: P), the cap, and input and output under 2 GB.  RSP_OK and *nfft_out =
// the resolved length, or the refusal with its message set.
int rsp_mtd_check_sizes(int64_t P, int64_t G, int64_t n_maps, int64_t nfft, int precision, int* nfft_out);
// The kernel argument of sizes already checked; vec is left 0 (the launcher's caller knows the pointers)
MtdDesc mtd_desc(int P, int G, int n_maps, int nfft, int shift, bool has_win, int prec);
// The chirp-z tables of nfft, w[0 .. nfft) | Bf[0 .. M), evaluated in long double and rounded once to
// the precision (the doubles hold the rounded values); empty for a power of two
void rsp_mtd_tables(int nfft, int prec, std::vector<std::complex<double>>& out);
// The Stockham twiddles k_mtd_any reads for an L-point transform: the compact tables of
// PlanPow2<log2 L> and then those of its reverse (the inverse passes of the chirp-z route)
void rsp_mtd_twiddles(int lgL, std::vector<std::complex<double>>& out);

// Which K1 slow-time FFTs run k1_fft_dif (the persistent and the tiled K1 agree, so their outputs
// are bit-identical): P = 64, 128 always; P = 256 for plans of more than 8 channels (with 8, the
// persistent K1's 8 sub-tiles of loads per wave and the DIF's registers spill: the Stockham passes)
RSP_HD constexpr bool k1_dif(int lgp, int cp) { return lgp >= 6 && (lgp <= 7 || (lgp == 8 && cp >= 16)); }

// The slow-time transform of a plan: which K1 kernel launch_k1 starts in `mode`, the transform it
// runs, the sub-tiles per wave of the persistent kernels (0: tiled) and the k_mtd_cols
// instantiation of the stage-2 path.  The one decision: launch_k1, launch_mtd_cols,
// rsp_query_k1_route and rsp_plan_describe all read it.  kernel / transform use the values of
// rsp.h's RSP_K1_KERNEL_* / RSP_K1_TRANSFORM_*.
enum { K1K_TILED = 0, K1K_PERSISTENT = 1, K1K_PERSISTENT_FACTORED = 2 };
enum { K1X_STOCKHAM = 0, K1X_DIF = 1, K1X_FACTORED = 2, K1X_DIRECT = 3 };
struct K1Route {
    int kernel, transform, tpw, lgp2;
};
// `mode` bits as launch_k1's: 1 = apply DBF, 2 = apply MTD (3: the frame chain; 0: the stage-2
// transpose, always the tiled kernel).
K1Route k1_route(const Geometry& g, int mode);
bool k1_persistent_fits(const Geometry& g);

// Dynamic LDS bytes each launcher requests
size_t k1_tiled_lds(const Geometry& g, bool rq);    // k1_dbf_mtd: tile | twiddles, or (rq) k1_dft_rq's tables
size_t k1p_lds(const Geometry& g);                  // k1p_dbf_mtd
size_t k1q_lds(const Geometry& g);                  // k1q_dbf_mtd
size_t mtd_cols_lds(const Geometry& g);             // k_mtd_cols: 16 columns | twiddles

// Everything rsp_plan_create_ex derives from its arguments before it touches the device: the
// Geometry, the segment and job lists, the buffer sizes and the host tables in upload order
// (complex tables as complex double; the plan narrows them to its precision on upload).
struct PlanHost {
    typedef std::complex<double> cd;
    Geometry g{};
    std::vector<SegDesc> segs;
    std::vector<K2Job> jobs;
    int det_bound = 1;   // cells under test per frame: the most detections a frame can have
    size_t z_elems = 0, rdm_elems = 0, mag_elems = 0;
    std::vector<double> atab;        // DBF MFMA A operands per lane: [MB][CP/4][Re,Im][64]
    std::vector<cd> twP, twPp, twD, twQ;
    std::vector<double> win, taps;
    std::vector<cd> H, twM;
    std::vector<double> range_axis, velocity_axis, beam_angles, klut;
    std::vector<int> k2order;        // pulse-compression workgroup dispatch order
    std::vector<K2Rec> k2rec;        // the same as per-workgroup records: what the plan uploads
    // the band and edge row sets (K2SET_BAND, K2SET_EDGE) and their record tables, built like k2rec
    // (n = 0 and no records: the plan has no such set, see k2_row_set)
    K2Rows k2rows[3] = {};
    std::vector<K2Rec> k2rec_band, k2rec_edge;
};
// The row set `which` of a plan: n = 0 for the band and edge sets of a plan whose K3 is not the
// compile-time 5/5/10/10 kernel (they follow that window's hV) or whose P has no row under test.
K2Rows k2_row_set(const Geometry& g, int which);
// One record table: the jobs (segment x block) over `rows_total` rows, interleaved in proportion and
// laid out over the XCDs (derive_k2_order says how).  jobs / order may be null.
int k2_build_records(const Geometry& g, const std::vector<SegDesc>& segs, int rows_total, std::vector<K2Job>* jobs,
                     std::vector<int>* order, std::vector<K2Rec>* rec);

// Stage-3 range CFAR (k_s3_cfar, rsp_stage3.hip).  A workgroup resolves RSP_S3_ROWS Doppler rows
// (4 waves, a row per wave and pass) of RSP_S3_CH range cells on the map's own column grid, each
// row from a tile that holds the chunk and RSP_S3_HMAX cells on either side: s + r <= RSP_S3_HMAX
// is the envelope.
#define RSP_S3_CH 256
#define RSP_S3_ROWS 16
#define RSP_S3_HMAX 64
struct S3Desc {          // kernel argument
    int P, G;
    int seg_a[3], seg_n[3];   // 0-based first column and length of each segment
    int r, s, H;              // refCells_R, saveCells_R, s + r
    int method;               // 0: greatest of, 1: smallest of
    int z0, z1;               // 0-based notched rows, inclusive (z0 > z1: none)
    double T;                 // T_CFAR
};
// The checks of the stage-3 calls and the descriptor for a map of P rows and segments of
// gates[0..2] columns.  RSP_OK, or RSP_ERR_INVALID with the message set.
int rsp_stage3_derive(int P, const int32_t* gates, const rsp_stage3_cfar_params* prm, S3Desc* out);

// Doppler CA-CFAR (k_vcfar, rsp_vcfar.hip).  A workgroup resolves RSP_VC_ROWS Doppler rows of
// RSP_VC_COLS range columns (4 waves, lanes across columns) from an LDS tile that holds those rows
// and the window's halo = r + h rows above and below: halo <= RSP_VC_HMAX is the envelope.  The
// tile is sized by the halo in use (vc_lds_bytes), not by RSP_VC_HMAX.
#define RSP_VC_COLS 64
#define RSP_VC_ROWS 32
#define RSP_VC_HMAX 32
struct VcDesc {          // kernel argument
    int P, G;
    int r, h, halo;      // refCells_V, guardCells_V / 2, r + h
    int method;          // 0: CA, 1: GOCA, 2: SOCA
    double T;            // T_CFAR
};
// Dynamic LDS bytes of k_vcfar's amplitude tile for reals of rs bytes
RSP_HD constexpr size_t vc_lds_bytes(int halo, size_t rs) { return (size_t)(RSP_VC_ROWS + 2 * halo) * RSP_VC_COLS * rs; }
// The checks of the Doppler CFAR calls and the descriptor for a map of P rows and G columns.
// RSP_OK, or RSP_ERR_INVALID with the message set.
int rsp_vcfar_derive(int P, int G, const rsp_vcfar_params* prm, VcDesc* out);

// Cross GOCA-CFAR as a map detector (k_xcfar, rsp_xcfar.hip).  A workgroup resolves RSP_XC_ROWS
// Doppler rows of RSP_XC_COLS range columns (4 waves, lanes across columns) from the cross its cells
// read, held in LDS: ROWS x (COLS + 2 hR') cells, hR' = hR rounded up to 4 cells so that tile rows
// start on a 16-byte unit of the map row, and 2 hV x COLS cells above and below.  hR <= RSP_XC_HMAX_R
// and hV <= RSP_XC_HMAX_V is the envelope (RSP_S3_HMAX and RSP_VC_HMAX).  The tile is sized by the
// halos in use (xc_lds_bytes): the reference's 15 / 15 takes 39 KiB in double (three workgroups per
// CU with the hit queue), the envelope's corner 80 KiB.
#define RSP_XC_COLS 64
#define RSP_XC_ROWS 32
#define RSP_XC_HMAX_R 64
#define RSP_XC_HMAX_V 32
struct XcDesc {          // kernel argument
    int P, G;
    int rR, gR, rV, gV;  // reference and guard cells along range and Doppler
    int hR, hV;          // the tile's halos: rR + gR and rV + gV, or 0 and 0 when no cell is under test
    int r0, r1, v0, v1;  // 0-based cells under test [r0, r1) x [v0, v1); all 0 when there are none
    double T;            // T_CFAR
};
RSP_HD constexpr int xc_tile_width(int hR) { return RSP_XC_COLS + 2 * ((hR + 3) & ~3); }
// Dynamic LDS bytes of k_xcfar's amplitude tile for reals of rs bytes
RSP_HD constexpr size_t xc_lds_bytes(int hR, int hV, size_t rs) {
    return ((size_t)RSP_XC_ROWS * xc_tile_width(hR) + (size_t)2 * hV * RSP_XC_COLS) * rs;
}
// The checks of the cross CFAR calls and the descriptor for a map of P rows and G columns.
// RSP_OK, or RSP_ERR_INVALID with the message set.
int rsp_xcfar_derive(int P, int G, const rsp_cfar_params* prm, XcDesc* out);

// Detection on any RD cube (k_pairsum, k_s9, rsp_detect.hip).  k_pairsum on a cube in MATLAB's layout
// [V x G x B]: a workgroup takes RSP_PS_ROWS Doppler rows of RSP_PS_COLS range cells, walks the B beams
// and turns each beam's magnitudes through an LDS tile of ROWS rows of COLS + RSP_PS_PAD elements.
#define RSP_PS_ROWS 64
#define RSP_PS_COLS 64
#define RSP_PS_PAD 1
RSP_HD constexpr size_t ps_lds_bytes(size_t rs) { return (size_t)RSP_PS_ROWS * (RSP_PS_COLS + RSP_PS_PAD) * rs; }
enum { DET_LAYOUT_MATLAB = 0, DET_LAYOUT_DEVICE = 1 };   // [V x G x B], Doppler index fastest | [B][V][G]
struct DetDesc {         // kernel argument of k_pairsum and k_s9
    int V, G, B;
    int vec;             // k_pairsum: 1 when its 16-byte units are aligned (complex single; see the kernel)
    int cplx;            // k_s9: 1 = the complex monopulse ratio
};
// The size checks of the detect calls (rsp_detect_describe's) and the CFAR descriptor of a V x G map.
// RSP_OK, or the refusal with its message set.
int rsp_detect_check_sizes(int64_t V, int64_t G, int64_t B, int precision, const rsp_cfar_params* prm, XcDesc* out);

// ---- pulse compression for any pulse and beam count (k_pc_pack, k2_pc, k_pc_unpack; rsp_pc.hip) ----
// k_pc_pack turns beams [P x N x B] (pulse index fastest) into k2_pc's z input for a Geometry that carries the
// caller's P and B; k_pc_unpack turns k2_pc's [B][P][G] result into pc [P x G x B].  Both are tiled
// transposes through LDS with 256 threads.
//   pack:   a workgroup takes one z chunk (RSP_PC_NZ compacted samples) of RSP_PCK_COLS pulses of one beam:
//           NZ source rows of up to COLS contiguous pulses in, COLS NZ contiguous z elements out.  LDS rows
//           (one per sample) are COLS + RSP_PCK_PAD elements apart.
//   unpack: a workgroup takes RSP_PCU_ROWS pulses of pcu_cols(prec) gates of one beam (512 bytes of a result
//           row: 64 complex singles, 32 complex doubles).  LDS rows (one per pulse) are cols + RSP_PCU_PAD
//           elements apart: an odd stride, k_pairsum's rule.  It walks up to RSP_PCU_GROUP such tiles along the
//           pulse axis, so that one workgroup writes a column's consecutive 512-byte runs.
#define RSP_PC_NZ 8
#define RSP_PCK_COLS 256
#define RSP_PCK_PAD 4
#define RSP_PCU_ROWS 64
#define RSP_PCU_PAD 1
#define RSP_PCU_GROUP 8   // pulse tiles one unpack workgroup walks: 512 pulses of its gates
RSP_HD constexpr int pcu_cols(int prec) { return prec == RSP_PREC_F64 ? 32 : 64; }
RSP_HD constexpr size_t pck_lds_bytes(int prec) {
    return (size_t)RSP_PC_NZ * (RSP_PCK_COLS + RSP_PCK_PAD) * (prec == RSP_PREC_F64 ? 16 : 8);
}
RSP_HD constexpr size_t pcu_lds_bytes(int prec) {
    return (size_t)RSP_PCU_ROWS * (pcu_cols(prec) + RSP_PCU_PAD) * (prec == RSP_PREC_F64 ? 16 : 8);
}
struct PcDesc {
    // k2_pc's kernel argument: the base's segments, sample intervals, N, G, Gp, precision and k2_pts with
    // the caller's P and B, NZ = RSP_PC_NZ, nzc, and the jobs of B P rows (njobs, jobs, nwg_k2)
    Geometry g;
    K2Rows rows;                 // {P, 0, P, 0, B P}
    int pack_tiles, pack_wg;     // pulse tiles of a chunk; workgroups = nzc x pack_tiles x B, chunk fastest
    int unpack_row_tiles, unpack_row_groups, unpack_col_tiles, unpack_wg;   // workgroups = col tiles x row groups x B, columns fastest
    size_t in_elems, z_elems, out_elems, mag_elems;      // beams, z, the result (either layout), the scratch magnitude map
};
// The checks of the rsp_pc calls that need no device, and everything their launches are sized by.  `base` is a
// derived plan Geometry: only what does not depend on its own P and B is read (see PcDesc::g).  rec (may be
// null): k2_pc's record table for the B P rows.  RSP_OK, or the refusal with its message set: RSP_ERR_INVALID
// for P < 1 or B < 1, RSP_ERR_UNSUPPORTED when the beams, z or the result reach 2 GB.
int rsp_pc_derive(const Geometry& base, int64_t P, int64_t B, PcDesc* out, std::vector<K2Rec>* rec);
void rsp_fill_pc_info(const PcDesc& d, rsp_pc_info* out);

// ---- digital down-conversion (k_ddc, rsp_ddc.hip) ----
// A workgroup takes TP pulses x TK outputs of one channel, TP = the least power of two >= min(P, 64); thread t
// has pulse t mod TP and k lane t / TP of KL, and accumulates KPT outputs, k lane + i KL: TK = KL KPT.  It
// stages rows = (TK - 1) D + LC input rows at a time: x as it is read, TP reals a row, and the row's NCO value,
// one complex; the L taps lie behind them.  RSP_DDC_LDS_BUDGET bounds the three together (four workgroups a CU).
// The host chooses KL (256 / TP, halved while KL lanes and 16 taps do not fit), then LC (L, or what fits: a
// longer filter is staged LC taps at a time) and then KPT (up to RSP_DDC_MAX_KPT, while the rows fit and the
// tile is not longer than the outputs).
#define RSP_DDC_THREADS 256
#define RSP_DDC_MAX_KPT 8
#define RSP_DDC_LOADS 8   // 16-byte loads a thread keeps in flight while it stages a tile
constexpr size_t RSP_DDC_LDS_BUDGET = 40 * 1024;
struct DdcDesc {          // kernel argument
    int P, N, C, No;
    int L, D, off, mode;
    int TP, lgTP, KL, KPT, TK, LC, rows;
    int k_tiles, p_tiles, threads;
    unsigned opitch;                // complex elements between the output's channel planes: P No, or k_dbf's pitch
    unsigned in_bytes, out_bytes;   // the buffer resources' ranges: P N C reals, C opitch complex elements
    unsigned ms_bytes;              // LDS: the NCO values, rounded up to 16 bytes; x follows, then the taps
    unsigned lds_bytes;
    uint64_t w, w0;
};
static_assert(sizeof(DdcDesc) == 112, "kernel-argument layout");
// The checks of the rsp_ddc calls and rsp_ddc_describe that need no device, and the kernel argument (mode, w
// and w0 left 0, the output contiguous).  precision: RSP_C128 / RSP_C64.  RSP_OK, or the refusal with its message set.
int rsp_ddc_derive(int64_t P, int64_t N, int64_t C, int64_t L, int64_t D, int64_t off, int precision, DdcDesc* out);
// The output's channel planes `opitch` >= P No complex elements apart (C opitch elements under 2 GB: the caller's check)
inline void ddc_set_opitch(DdcDesc* d, unsigned opitch, unsigned esz) {
    d->opitch = opitch;
    d->out_bytes = (unsigned)d->C * opitch * esz;
}
void rsp_fill_ddc_info(const DdcDesc& d, int precision, rsp_ddc_info* out);

// The checks of rsp_plan_create_ex that need no device and come before its device checks.
int rsp_plan_check_args(const rsp_sig_config* cfg, const rsp_cfar_params* cfar, const rsp_cluster_params* cluster,
                        const rsp_precomputed* pre, const rsp_plan_options* opt);
// The derivation for a device of ncu compute units (arguments already checked).  Returns RSP_OK or
// the status of the first refusal, its message set through rsp_set_error.
int rsp_plan_derive(const rsp_sig_config* cfg, const rsp_cfar_params* cfar, const rsp_cluster_params* cluster,
                    const rsp_precomputed* pre, const rsp_plan_options* opt, int ncu, PlanHost* out);

// The one filling routine of rsp_query_sizes / rsp_query_k1_route / rsp_query_k3_tiling /
// rsp_query_k2_layout and rsp_plan_describe / rsp_plan_describe_k3 / rsp_plan_describe_k2.
// gates = N_gate_narrow, N_gate_medium, N_gate_long: Geometry::segs holds the present segments
// only, in that order.
void rsp_fill_sizes(const Geometry& g, int det_bound, rsp_sizes* s);
void rsp_fill_k1_route(const Geometry& g, rsp_k1_route* out);
void rsp_fill_k3_tiling(const Geometry& g, rsp_k3_tiling* out);
void rsp_fill_k2_layout(const Geometry& g, const int32_t gates[RSP_MAX_SEG], rsp_k2_layout* out);
// rsp_query_k2_records / rsp_plan_describe_k2_records: the first min(cap, rec.size()) records into out
// (may be NULL when cap is 0), rec.size() into *n.
int rsp_fill_k2_records(const std::vector<K2Rec>& rec, rsp_k2_record* out, int32_t cap, int32_t* n);
// rsp_query_k2_row_set / rsp_plan_describe_k2_row_set: set `which` of rows / rec (all, band, edge)
int rsp_fill_k2_row_set(const K2Rows rows[3], const std::vector<K2Rec>* const rec[3], int32_t which, rsp_k2_row_set* set,
                        rsp_k2_record* out, int32_t cap, int32_t* n);
