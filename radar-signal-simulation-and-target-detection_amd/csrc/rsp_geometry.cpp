// rsp_geometry.cpp -- plan geometry, K1 routing and host tables of librsp (rsp_geometry.h): the
// analysis of the reference's precomputed_data that rsp_plan_create_ex runs before it touches the
// device, and rsp_plan_describe, which runs it alone.  Plain C++ (built and sanitized without HIP).
#include "rsp_geometry.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <utility>

__attribute__((visibility("hidden"))) int rsp_set_error(int code, const char* fmt, ...);   // rsp_host.cpp

namespace {

template <class... A>
int fail(int code, const char* fmt, A... a) { return rsp_set_error(code, fmt, a...); }

using cd = std::complex<double>;

bool is_pow2(int x) { return x > 0 && (x & (x - 1)) == 0; }
int ilog2i(int x) { int l = 0; while ((1 << l) < x) ++l; return l; }
size_t cplx_bytes(const Geometry& g) { return g.prec == RSP_PREC_F64 ? 16 : 8; }

// In-place double FFT (sign -1 forward, +1 inverse, unscaled); O(n^2) DFT if n is not 2^k.
void fft_d(std::vector<cd>& a, int sign) {
    const int n = (int)a.size();
    if (!is_pow2(n)) {
        std::vector<cd> o(n);
        for (int k = 0; k < n; ++k) {
            cd s = 0;
            for (int t = 0; t < n; ++t) s += a[t] * std::polar(1.0, sign * 2.0 * M_PI * ((double)((int64_t)t * k % n)) / n);
            o[k] = s;
        }
        a.swap(o);
        return;
    }
    for (int i = 1, j = 0; i < n; ++i) {
        int bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) std::swap(a[i], a[j]);
    }
    for (int len = 2; len <= n; len <<= 1) {
        for (int i = 0; i < n; i += len) {
            for (int k = 0; k < len / 2; ++k) {
                const cd w = std::polar(1.0, sign * 2.0 * M_PI * k / len);
                const cd u = a[i + k], v = a[i + k + len / 2] * w;
                a[i + k] = u + v;
                a[i + k + len / 2] = u - v;
            }
        }
    }
}

// Row stride (complex elements, P..P+15) of the factored slow-time DFT's LDS tile: the one whose
// pass-2 reads (k1_dft_rq: lane = subsequence (column, k2) of the first 64, element n + Q k2 of
// its column, and its mirror Q - n + Q k2) take the fewest ds_read_b128 cycles by the gfx950
// bank model (MI355X_MICROARCH.md LDS table: four 16-lane groups, 64 banks of 4 B; identical
// addresses broadcast).  Smallest stride on ties.  The reference frame (R = 4, Q = 83, B = 13):
// stride 332 = P itself is conflict-free.
int rq_pick_stride(int R, int Q, int ncols) {
    static const int grp_first[4][3][2] = {{{0, 4}, {12, 16}, {20, 28}}, {{4, 12}, {16, 20}, {28, 32}},
                                           {{32, 36}, {44, 48}, {52, 60}}, {{36, 44}, {48, 52}, {60, 64}}};
    const int P = R * Q, NS = std::min(ncols * R, 64), Qh = (Q - 1) / 2;
    int best = P, best_cost = INT32_MAX;
    for (int rs = P; rs < P + 16; ++rs) {
        long cost = 0;
        for (int n = 1; n <= Qh; ++n)
            for (int mirror = 0; mirror < 2; ++mirror)
                for (auto& grp : grp_first) {
                    int addr[16], na = 0;   // distinct 16-B addresses of the group's lanes
                    for (auto& rg : grp)
                        for (int l = rg[0]; l < rg[1]; ++l) {
                            if (l >= NS) continue;
                            const int c = l / R, k2 = l % R;
                            const int a = c * rs + Q * k2 + (mirror ? Q - n : n);
                            bool seen = false;   // a broadcast of the same address is free
                            for (int j = 0; j < na; ++j) seen = seen || addr[j] == a;
                            if (!seen) addr[na++] = a;
                        }
                    int cnt[16] = {0}, worst = 1;   // a 16-B slot covers 4 banks: slot a & 15
                    for (int j = 0; j < na; ++j) worst = std::max(worst, ++cnt[addr[j] & 15]);
                    cost += worst;
                }
        if (cost < best_cost) {
            best_cost = (int)cost;
            best = rs;
        }
    }
    return best;
}

// exp(-2 pi i e / n) with e reduced mod n and the angle formed in long double
cd root_of_unity(long long e, long long n) {
    e %= n;
    if (e < 0) e += n;
    const long double a = -2.0L * 3.141592653589793238462643383279502884L * (long double)e / (long double)n;
    return cd((double)std::cos(a), (double)std::sin(a));
}

void push_pass_twiddles(std::vector<cd>& out, int Ns, int R, bool cmp) {
    if (cmp) {
        for (int r = 1; r < R; r *= 2)
            for (int k = 0; k < Ns; ++k) out.push_back(root_of_unity((long long)k * r, (long long)Ns * R));
    } else {
        for (int k = 0; k < Ns; ++k)
            for (int r = 1; r < R; ++r) out.push_back(root_of_unity((long long)k * r, (long long)Ns * R));
    }
}

// Per-pass Stockham twiddle tables of a radix plan, concatenated as plan_tw_off() lays them out:
// pass q >= 1 owns Ns_q x (R_q - 1) entries T[k][r-1] = exp(-2 pi i k r / (Ns_q R_q)).  Compact
// tables (cmp): r = 1, 2, 4, 8 only, stored column-major, [i][k] = T[k][2^i] (load_tw in
// rsp_fft_passes.h).  The angle's numerator is reduced modulo the period first, so every entry is
// the correctly rounded double of the exact root of unity's angle.
void build_plan_twiddles(const RadixPlan& p, std::vector<cd>& out, bool cmp) {
    for (int q = 1; q < p.np; ++q) push_pass_twiddles(out, plan_ns(p, q), p.rad[q], cmp);
}

struct Interval { int lo, hi; };

// The overlap-save block sizes whose twiddle tables twM already holds, and their offsets in it
struct TwiddleSets {
    std::vector<int> sizes, offs;
};

// ---- pulse-compression segments (fsf:105-126) ---------------------------------------------

int build_fir_segment(SegDesc& s, const rsp_precomputed* pre, int N, int g1, std::vector<double>& taps) {
    s.type = 0;
    s.ga = 0; s.gb = g1;
    s.seg_lo = pre->seg_start_narrow - 1;
    if (s.seg_lo < 0 || s.seg_lo >= N) return fail(RSP_ERR_INVALID, "seg_start_narrow out of range");
    s.Ls = N - s.seg_lo;
    s.ntaps = pre->n_MF_narrow;
    s.delay = pre->fir_delay;
    if (s.ntaps < 1) return fail(RSP_ERR_INVALID, "empty MF_narrow");
    int lo = INT32_MAX, hi = -1;
    for (int gg = 0; gg < g1; ++gg) {
        int kk = (gg + s.delay) % s.Ls;
        if (kk < 0) kk += s.Ls;
        const int top = s.seg_lo + kk;
        const int bot = std::max(s.seg_lo, top - s.ntaps + 1);
        lo = std::min(lo, bot);
        hi = std::max(hi, top);
    }
    s.lo = lo; s.hi = hi;
    s.taps_off = (int)taps.size();
    for (int j = 0; j < s.ntaps; ++j) taps.push_back(pre->MF_narrow[j]);
    return RSP_OK;
}

int build_fft_segment(SegDesc& s, const double* mf_fft, int Nfft, int N, int ga, int gb, int seg_lo,
                      std::vector<cd>& H, std::vector<cd>& twM, TwiddleSets& tw, const char* name) {
    std::vector<cd> h(Nfft);
    for (int i = 0; i < Nfft; ++i) h[i] = cd(mf_fft[2 * i], mf_fft[2 * i + 1]);
    fft_d(h, +1);
    double hmax = 0;
    for (auto& v : h) { v /= (double)Nfft; hmax = std::max(hmax, std::abs(v)); }
    if (hmax == 0) return fail(RSP_ERR_INVALID, "%s matched filter is all zero", name);
    int Lh = 0;
    for (int i = 0; i < Nfft; ++i) if (std::abs(h[i]) > 1e-10 * hmax) Lh = i + 1;
    if (gb > Nfft)
        return fail(RSP_ERR_INVALID, "%s gates end at %d beyond N_fft %d (fsf:124-125 index out of range)", name, gb, Nfft);
    const int Ls = std::min(N - seg_lo, Nfft);   // fft(seg, Nfft) truncates or pads
    if (ga < Lh - 1 && Ls + (Lh - 1 - ga) > Nfft)
        return fail(RSP_ERR_UNSUPPORTED, "%s segment: circular aliasing reaches kept gates (L_s=%d L_h=%d N_fft=%d)", name, Ls, Lh, Nfft);
    s.type = 1;
    s.ga = ga; s.gb = gb; s.seg_lo = seg_lo;
    s.Lh = Lh;
    s.lo = std::max(seg_lo, seg_lo + ga - (Lh - 1));
    s.hi = std::min(seg_lo + Ls - 1, seg_lo + gb - 1);
    // overlap-save block size M = 2^k <= 2048 (so that a workgroup owns >= 2 adjacent rows:
    // 128 B contiguous loads of z), the mixed-radix 2560 = 16 x 10 x 16 (one row per workgroup)
    // or 4096 = 16 x 16 x 16 (one row per 4096-point workgroup: x4's 5 956-gate long segment in
    // 2 blocks instead of 5 x 2048); cost model blocks * M * (log2 M + 2)
    const int nout = gb - ga;
    double best = 1e300;
    int bestM = 0;
    const int cand[] = {64, 128, 256, 512, 1024, 2048, 2560, 4096};
    for (int M : cand) {
        const int V = M - Lh + 1;
        if (V < 1) continue;
        const int nb = (nout + V - 1) / V;
        const double cost = (double)nb * M * (std::log2((double)M) + 2);
        if (cost < best * 0.999) { best = cost; bestM = M; }
    }
    if (!bestM) {
        int maxM = 0;
        for (int M : cand) maxM = std::max(maxM, M);
        return fail(RSP_ERR_UNSUPPORTED, "%s filter length %d exceeds the largest overlap-save block (%d points)", name, Lh,
                    maxM);
    }
    const int M = bestM;
    const bool mix = !is_pow2(M);
    s.M = M; s.logM = mix ? 0 : ilog2i(M); s.V = M - Lh + 1;
    s.nblocks = (nout + s.V - 1) / s.V;
    // spectrum of h zero-padded to M, natural order, 1/M folded in
    std::vector<cd> hm(M, 0.0);
    for (int i = 0; i < Lh; ++i) hm[i] = h[i];
    fft_d(hm, -1);
    s.H_off = (int)H.size();
    for (auto& v : hm) H.push_back(v / (double)M);
    int ti = -1;
    for (size_t q = 0; q < tw.sizes.size(); ++q) if (tw.sizes[q] == M) ti = (int)q;
    if (ti < 0) {
        tw.sizes.push_back(M);
        tw.offs.push_back((int)twM.size());
        // compact tables of the forward FFT; a power-of-two block's inverse FFT (reversed radices)
        // has its own behind them, the 2560-point palindrome reads the forward ones
        const RadixPlan pl = mix ? plan_os_2560() : plan_os_pow2(s.logM);
        build_plan_twiddles(pl, twM, true);
        if (!mix) build_plan_twiddles(plan_rev(pl), twM, true);
        ti = (int)tw.sizes.size() - 1;
    }
    s.tw_off = tw.offs[ti];
    return RSP_OK;
}

// The segments of the stitched row with their taps, spectra and twiddles; the K2 workgroup size
// and each segment's rows per workgroup; the union U of the sample windows the segments read and
// each segment's offset into the compacted samples (K1 processes only these).
int derive_segments(const rsp_sig_config* cfg, const rsp_precomputed* pre, PlanHost& h, std::vector<Interval>& U) {
    Geometry& g = h.g;
    const int N = cfg->point_PRT;
    const int g1 = pre->N_gate_narrow, g2 = pre->N_gate_medium, g3 = pre->N_gate_long, G = pre->N_total_gate;
    const bool f64 = g.prec == RSP_PREC_F64;
    TwiddleSets tw;
    int rc;
    if (g1 > 0) {
        SegDesc s{};
        if ((rc = build_fir_segment(s, pre, N, g1, h.taps))) return rc;
        h.segs.push_back(s);
    }
    if (g2 > 0) {
        SegDesc s{};
        if ((rc = build_fft_segment(s, pre->MF_medium_fft, pre->N_fft_med, N, g1, g1 + g2, pre->seg_start_medium - 1, h.H,
                                    h.twM, tw, "medium")))
            return rc;
        h.segs.push_back(s);
    }
    if (g3 > 0) {
        SegDesc s{};
        if ((rc = build_fft_segment(s, pre->MF_long_fft, pre->N_fft_long, N, g1 + g2, G, pre->seg_start_long - 1, h.H, h.twM,
                                    tw, "long")))
            return rc;
        h.segs.push_back(s);
    }
    // K2 workgroup size in LDS points: a complex-double plan with a 2560-point block sizes every
    // workgroup for it (40 KB of LDS, no pads: 4 per CU, k2_pc's 128-VGPR budget), power-of-two
    // blocks then holding 2048 / M rows; otherwise RSP_K2_POINTS (4096: 2 per CU in complex double)
    g.k2_pts = RSP_K2_POINTS;
    for (auto& s : h.segs)
        if (f64 && s.type == 1 && s.M == 2560) g.k2_pts = RSP_K2_MIXPTS;
    for (auto& s : h.segs)   // a 4096-point block needs the 4096-point workgroups (2 per CU)
        if (s.type == 1 && s.M == 4096) g.k2_pts = RSP_K2_POINTS;
    // the narrow (direct-FIR) segment stages whole rows in the workgroup's LDS: when its window
    // does not fit a 2560-point workgroup the plan falls back to RSP_K2_POINTS workgroups (2 per
    // CU; k2_pc runs the 2560-point block in either sizing)
    for (auto& s : h.segs)
        if (s.type == 0 && g.k2_pts != RSP_K2_POINTS) {
            const int WP = s.hi - s.lo + 1 + s.ntaps - 1;
            if (WP + (s.ntaps + 1) / 2 > g.k2_pts) g.k2_pts = RSP_K2_POINTS;   // no pads at 2560
        }
    std::vector<Interval> need;
    for (auto& s : h.segs) {
        if (s.seg_lo < 0 || s.seg_lo >= N) return fail(RSP_ERR_INVALID, "segment start out of range");
        if (s.hi >= s.lo) need.push_back({s.lo, s.hi});
        if (s.type == 1) {
            const int pts = (g.k2_pts == RSP_K2_POINTS) ? RSP_K2_POINTS : 2048;   // k2_pc's PTS
            s.rows_per_wg = s.M == 2560 ? 1 : std::max(1, pts / s.M);
        } else {
            // up to 8 rows per workgroup (measured best of 1/2/4/8 at x2), within the workgroup's
            // LDS: rows * WP complex + the taps (ntaps reals = ntaps / 2 complex)
            const int WP = s.hi - s.lo + 1 + s.ntaps - 1;   // staged row: ntaps - 1 leading zeros
            const int lds_c = g.k2_pts == RSP_K2_POINTS ? k2_lds_data(g.k2_pts, RSP_K2_SH) : g.k2_pts;   // k2_pc's LDS
            s.rows_per_wg = std::max(1, std::min(8, (lds_c - (s.ntaps + 1) / 2) / WP));
            if (WP * s.rows_per_wg + (s.ntaps + 1) / 2 > lds_c)
                return fail(RSP_ERR_UNSUPPORTED, "narrow segment window %d samples too long", s.hi - s.lo + 1);
        }
    }
    // union of needed fast-time windows -> compacted sample list
    std::sort(need.begin(), need.end(), [](const Interval& a, const Interval& b) { return a.lo < b.lo; });
    for (auto& iv : need) {
        if (!U.empty() && iv.lo <= U.back().hi + 1) U.back().hi = std::max(U.back().hi, iv.hi);
        else U.push_back(iv);
    }
    std::vector<int> nof;
    for (auto& iv : U) for (int n = iv.lo; n <= iv.hi; ++n) nof.push_back(n);
    g.nU = (int)nof.size();
    for (auto& s : h.segs) {
        if (s.hi < s.lo) { s.off = 0; continue; }
        s.off = (int)(std::lower_bound(nof.begin(), nof.end(), s.lo) - nof.begin());
    }
    return RSP_OK;
}

// ---- K1 tile --------------------------------------------------------------------------------
// NT samples per [P][NT] slab.  complex64: LDS tile <= 80 KB (2 workgroups per CU for the tiled
// K1; the persistent K1 double-buffers it) and B*NT*P <= 8192 (16 FFT points per thread);
// complex128: the same bytes (NT halved) and B*NT*P <= 4096.  Also the slow-time transform's
// factorisation and row stride, the z layout and the sample intervals U as kernel arguments.
int derive_k1_tile(Geometry& g, const std::vector<Interval>& U) {
    const int B = g.B, P = g.P;
    const bool f64 = g.prec == RSP_PREC_F64;
    const size_t esz = cplx_bytes(g);
    g.pow2P = is_pow2(P) && P >= 16 && P <= 512;   // Stockham range of k1_fft; else a DFT
    // other P = R Q (R = 2 or 4, Q odd >= 3; the reference's 332 = 4 x 83): the factored DFT
    // when one tile column per beam and its tables fit the LDS; otherwise the direct DFT
    g.rqR = g.rqQ = g.twq_elems = 0;
    if (!g.pow2P) {
        int R = 1;
        while (P % (2 * R) == 0) R *= 2;
        const int Q = P / R, Qh = (Q - 1) / 2;
        const int twq = (Qh + 1 + RQ_RK - 1) / RQ_RK * Qh * RQ_RK;
        if (R <= 4 && Q >= 3 && ((size_t)B * (P + 15) + rq_table_elems(twq, P)) * esz <= RSP_LDS_BYTES) {
            g.rqR = R;
            g.rqQ = Q;
            g.twq_elems = twq;
        }
    }
    // pow2: + one pad per 16 (K1_SH), see rsp_k1.hip; factored DFT: the row stride in
    // P..P+15 whose pass-2 reads are conflict-free (rq_pick_stride)
    g.Ppad = g.pow2P ? P + P / 16 : (g.rqQ ? rq_pick_stride(g.rqR, g.rqQ, B) : P + 4);
    const int max_pts = f64 ? 4096 : 8192;
    const size_t tile_cap = f64 ? 72 * 1024 : 80 * 1024;
    const size_t tab_bytes = g.rqQ ? (size_t)rq_table_elems(g.twq_elems, P) * esz : 0;   // k1_dft_rq's LDS tables
    g.NT = 8;
    while (g.NT > 1 && ((size_t)B * g.NT * g.Ppad * esz > tile_cap || (g.pow2P && B * g.NT * P > max_pts) ||
                        (size_t)B * g.NT * g.Ppad * esz + tab_bytes > RSP_LDS_BYTES))
        g.NT >>= 1;
    if ((size_t)B * g.NT * g.Ppad * esz + tab_bytes > RSP_LDS_BYTES || (g.pow2P && B * g.NT * P > 8192))
        return fail(RSP_ERR_UNSUPPORTED, "B*P too large for the slow-time FFT tile");
    g.ntiles = (g.nU + g.NT - 1) / g.NT;
    // z chunks: NT samples (one K1 tile) per row slab
    g.NZ = g.NT;
    g.nzc = (g.nU + g.NZ - 1) / g.NZ;
    if ((int)U.size() > RSP_MAX_IVL) return fail(RSP_ERR_UNSUPPORTED, "too many sample intervals");
    g.nivl = (int)U.size();
    for (int q = 0, st = 0; q < g.nivl; ++q) {
        g.ivl_lo[q] = U[q].lo;
        g.ivl_start[q] = st;
        st += U[q].hi - U[q].lo + 1;
    }
    if (g.pow2P) g.logP = ilog2i(P);
    if (16 * (size_t)g.Ppad * esz > RSP_LDS_BYTES || (g.pow2P && 16 * P > 8192))   // 16 columns: the stage-2 path's tile
        return fail(RSP_ERR_UNSUPPORTED, "prtNum %d too large", P);
    return RSP_OK;
}

// ---- K2 jobs and dispatch order -------------------------------------------------------------
// K2 dispatch order.  (1) Workgroups of a job covering adjacent rows form groups of gs
// (below), at key (i + 1/2) / ngroups_j, so that the narrow FIR, medium and long jobs are
// interleaved in proportion through the launch.  (2) Workgroups go to the 8 XCDs
// round-robin by dispatch position, so the groups are laid out 8 at a time: positions
// 8 (gs c + m) + x hold member m of group 8c + x -- every row of a group on one XCD, whose
// L2 then serves the rest of every 128-B z line the first one fetched.  A z line holds
// 128 / (NT esz) adjacent rows, a workgroup rows_per_wg of them, so gs = the most
// workgroups one line spans over the jobs (x2: NT = 4, one-row long blocks -> 2; x4:
// NT = 1 -> 8).  Workgroups left over go last.
}  // namespace

int k2_build_records(const Geometry& g, const std::vector<SegDesc>& segs, int rows_total, std::vector<K2Job>* jobs_out,
                     std::vector<int>* order_out, std::vector<K2Rec>* rec) {
    std::vector<K2Job> jobs;
    int nwg_total = 0;
    for (size_t si = 0; si < segs.size(); ++si) {
        const SegDesc& s = segs[si];
        const int nwg = (rows_total + s.rows_per_wg - 1) / s.rows_per_wg;
        const int nbl = (s.type == 1) ? s.nblocks : 1;
        for (int blk = 0; blk < nbl; ++blk) {
            jobs.push_back(K2Job{(int)si, blk, nwg_total, nwg});
            nwg_total += nwg;
        }
    }
    const int esz = (int)cplx_bytes(g);
    int gs = 1;
    for (const K2Job& jb : jobs) {
        const int rw = std::max(segs[jb.seg].rows_per_wg, 1);
        gs = std::max(gs, std::min(8, 128 / std::max(rw * g.NZ * esz, 1)));
    }
    // (3) The overlap-save blocks of one row read overlapping sample windows (Lh - 1 samples
    // shared by neighbouring blocks: x4's long segment, 4 blocks): the groups of all blocks of
    // the same rows form one unit, placed on one XCD back to back, so that the shared lines
    // are L2 hits instead of second HBM fetches.  Units go to the XCD with the shortest queue
    // (round-robin when they are all the same size, x2) and the queues are interleaved:
    // dispatch position 8 s + x is the s-th workgroup of XCD x's queue.
    struct Unit { double key; std::vector<int> wgs; };
    std::vector<Unit> units;
    std::vector<int> single;
    for (int si = 0; si < (int)segs.size(); ++si) {
        std::vector<const K2Job*> blks;
        for (const K2Job& jb : jobs)
            if (jb.seg == si) blks.push_back(&jb);
        if (blks.empty()) continue;
        const int wc = blks[0]->wg_count, ng = wc / gs;   // every block of a segment covers all rows
        for (int i = 0; i < ng; ++i) {
            Unit u{(i + 0.5) / ng, {}};
            for (const K2Job* jb : blks)
                for (int m = 0; m < gs; ++m) u.wgs.push_back(jb->wg_begin + gs * i + m);
            units.push_back(std::move(u));
        }
        for (const K2Job* jb : blks)
            for (int w = ng * gs; w < wc; ++w) single.push_back(jb->wg_begin + w);
    }
    std::stable_sort(units.begin(), units.end(), [](const Unit& x, const Unit& y) { return x.key < y.key; });
    std::vector<int> q[8];
    for (const Unit& u : units) {
        int x = 0;
        for (int c = 1; c < 8; ++c)
            if (q[c].size() < q[x].size()) x = c;
        q[x].insert(q[x].end(), u.wgs.begin(), u.wgs.end());
    }
    std::vector<int> order;
    size_t qmax = 0;
    for (auto& v : q) qmax = std::max(qmax, v.size());
    for (size_t sl = 0; sl < qmax; ++sl)
        for (int x = 0; x < 8; ++x)
            if (sl < q[x].size()) order.push_back(q[x][sl]);
    for (int w : single) order.push_back(w);
    if ((int)order.size() != nwg_total)
        return fail(RSP_ERR_INVALID, "K2 dispatch order covers %d of %d workgroups", (int)order.size(), nwg_total);
    // The same order as records: what k2_pc would find for workgroup `wg` by searching the job list
    rec->clear();
    rec->reserve(order.size());
    for (int wg : order) {
        size_t ji = 0;
        while (ji + 1 < jobs.size() && wg >= jobs[ji + 1].wg_begin) ++ji;
        const K2Job& jb = jobs[ji];
        rec->push_back(K2Rec{jb.seg, jb.blk, (wg - jb.wg_begin) * segs[jb.seg].rows_per_wg, wg});
    }
    if (jobs_out) *jobs_out = std::move(jobs);
    if (order_out) *order_out = std::move(order);
    return RSP_OK;
}

K2Rows k2_row_set(const Geometry& g, int which) {
    const int hV = RSP_K3_FAST_HV;
    if (which == K2SET_ALL) return K2Rows{g.P, 0, g.P, 0, g.B * g.P};
    if (!k3_fast_params(g) || g.P <= 2 * hV) return K2Rows{0, 0, 0, 0, 0};
    if (which == K2SET_BAND) return K2Rows{g.P - 2 * hV, hV, g.P - 2 * hV, 0, g.B * (g.P - 2 * hV)};
    return K2Rows{2 * hV, 0, hV, g.P - 2 * hV, g.B * 2 * hV};
}

namespace {

// The all-rows jobs travel in the Geometry (g.jobs, g.nwg_k2); the segments must be final.
int derive_k2_jobs(PlanHost& h) {
    Geometry& g = h.g;
    int rc = k2_build_records(g, h.segs, g.B * g.P, &h.jobs, &h.k2order, &h.k2rec);
    if (rc) return rc;
    g.nseg = (int)h.segs.size();
    g.njobs = (int)h.jobs.size();
    if (g.nseg > RSP_MAX_SEG || g.njobs > RSP_MAX_JOBS)
        return fail(RSP_ERR_UNSUPPORTED, "%d overlap-save jobs exceed %d", g.njobs, RSP_MAX_JOBS);
    for (int q = 0; q < g.nseg; ++q) g.segs[q] = h.segs[q];
    for (int q = 0; q < g.njobs; ++q) g.jobs[q] = h.jobs[q];
    g.nwg_k2 = (int)h.k2rec.size();
    return RSP_OK;
}

// The band and edge sets' tables (after derive_k3_tiling: the sets follow K3's window)
int derive_k2_sets(PlanHost& h) {
    const Geometry& g = h.g;
    for (int w = 0; w < 3; ++w) h.k2rows[w] = k2_row_set(g, w);
    if (!h.k2rows[K2SET_BAND].n) return RSP_OK;
    int rc = k2_build_records(g, h.segs, h.k2rows[K2SET_BAND].total, nullptr, nullptr, &h.k2rec_band);
    return rc ? rc : k2_build_records(g, h.segs, h.k2rows[K2SET_EDGE].total, nullptr, nullptr, &h.k2rec_edge);
}

// ---- K3 tiling ------------------------------------------------------------------------------
#define RSP_K3_TILE_KB 48   // KB of S per K3 tile (48: 2 Doppler bands at P = 128, 3 workgroups per CU)
#define RSP_K3_RT_C128 32   // K3 tile width in range cells, complex double
int derive_k3_tiling(Geometry& g) {
    const size_t rsz = cplx_bytes(g) / 2;
    g.cfar_hR = (std::max(g.refR + g.guardR, 2) + 3) & ~3;   // halo, multiple of 4 (16-B tile loads)
    // tiles of RT range cells (64 complex single / 32 complex double: the fast path) x a band of
    // Doppler rows, <= RSP_K3_TILE_KB of S per tile (48 KB: 3 workgroups per CU; at P = 128 two
    // bands measured 78 vs 85 us per 8 x2 frames for one band at 2 workgroups per CU): at P = 128
    // one band holds every row; longer P (x4's 256) splits the rows into bands, each with the
    // rV + gV window rows on either side
    g.cfar_RT = rsz == 4 ? 64 : RSP_K3_RT_C128;
    // LDS row stride, 16-B aligned; complex double + 2 cells (bank spread, k3_cfar).
    // k3_cfar's compile-time path (the reference's 5/5/10/10) holds only the band's own cells
    // (its prefilter reads whichever range slice lies in the tile; the rare survivors and S9
    // read the windows from the magnitude maps)
    const bool k3_nohalo = k3_fast_params(g);
    const int hx = k3_nohalo ? 0 : 2;
    g.cfar_W = ((g.cfar_RT + hx * g.cfar_hR + 3) & ~3) + (rsz == 8 ? 2 : 0);
    const int hV = g.refV + g.guardV, ncut = std::max(g.P - 2 * hV, 1);
    const int hrows = k3_nohalo ? 0 : 2 * hV;
    const int rows_max = (int)((RSP_K3_TILE_KB * 1024) / ((size_t)g.cfar_W * rsz));
    if (rows_max - hrows < 1) return fail(RSP_ERR_UNSUPPORTED, "CFAR window %d x %d exceeds the LDS tile", hV, g.cfar_hR);
    g.cfar_nband = (ncut + rows_max - hrows - 1) / (rows_max - hrows);
    g.cfar_VB = (ncut + g.cfar_nband - 1) / g.cfar_nband;
    g.cfar_rows = std::min(g.P, g.cfar_VB + hrows);
    return RSP_OK;
}

// ---- tables ---------------------------------------------------------------------------------
// (taps, H and twM were built with their segments)
void build_tables(const rsp_precomputed* pre, PlanHost& h) {
    Geometry& g = h.g;
    const int C = g.C, B = g.B, P = g.P, G = g.G;
    // the DBF's MFMA A operands: conj(W), y = x * W' (fsf:95), in K1's row layout
    rsp_dbf_atab(pre->DBF_coeffs_data_C, B, C, 1, DBF_ROWS_SPLIT, h.atab);
    h.twP.resize(P);
    if (g.pow2P) build_plan_twiddles(plan_pow2(g.logP), h.twPp, false);
    g.twPp_elems = (int)h.twPp.size();
    if (g.pow2P && P >= 64 && P <= 256)   // k1_fft_dif (k1_dif: P = 64 .. 256): compact pass-A twiddles, column-major [i][n2]
        for (int i = 0; i < 4; ++i)
            for (int n2 = 0; n2 < P / 16; ++n2) h.twD.push_back(root_of_unity((long long)n2 << i, P));
    for (int i = 0; i < P; ++i) h.twP[i] = root_of_unity(i, P);
    // k1_dft_rq's pass-2 table: [fset][n - 1][r] = (cos, sin)(2 pi k1 n / Q), k1 = RQ_RK fset + r
    // (zero past (Q - 1) / 2)
    if (g.rqQ) {
        const int Q = g.rqQ, Qh = (Q - 1) / 2, nfs = g.twq_elems / (Qh * RQ_RK);
        for (int fs = 0; fs < nfs; ++fs)
            for (int n = 1; n <= Qh; ++n)
                for (int r = 0; r < RQ_RK; ++r) {
                    const int k1 = fs * RQ_RK + r;
                    const cd w = k1 <= Qh ? root_of_unity((long long)k1 * n, Q) : cd(0.0, 0.0);
                    h.twQ.push_back(cd(w.real(), -w.imag()));   // exp(-i theta) -> (cos, sin) theta
                }
    }
    h.win.assign(pre->MTD_win, pre->MTD_win + P);
    h.range_axis.assign(pre->range_axis, pre->range_axis + G);
    h.velocity_axis.assign(pre->velocity_axis, pre->velocity_axis + P);
    h.beam_angles.assign(pre->beam_angles_deg, pre->beam_angles_deg + B);
    h.klut.assign(std::max(B - 1, 1), 0.0);
    for (int i = 0; i + 1 < B; ++i) h.klut[i] = pre->k_slopes_LUT[i];
}

// ---- route helpers --------------------------------------------------------------------------

// sub-tiles per wave of the persistent K1 (one load round per tile): TPW, or 2 TPW
int k1p_tpw(const Geometry& g) {
    const int pt = g.prec == RSP_PREC_F64 ? 16 : 32;   // pulses per MFMA sub-tile
    const int tpw = k1_cfg(g.C, g.B).TPW;
    const int need = (g.NT * (g.P / pt) + (K1_THREADS / 64) - 1) / (K1_THREADS / 64);
    return need <= tpw ? tpw : (need <= 2 * tpw ? 2 * tpw : 0);
}

// sub-tiles per wave of the factored-DFT K1 (one load round per tile): ceil(sub-tiles / 8) <= 4
int k1q_tpw(const Geometry& g) {
    const int pt = g.prec == RSP_PREC_F64 ? 16 : 32;
    const int need = (g.NT * ((g.P + pt - 1) / pt) + (K1_THREADS / 64) - 1) / (K1_THREADS / 64);
    return need <= 4 ? need : 0;
}

bool k1q_fits(const Geometry& g) {
    return !g.pow2P && g.rqQ > 0 && k1q_tpw(g) > 0 && k1q_lds(g) <= RSP_LDS_BYTES && g.ncu > 0 && !g.k1_tiled;
}

}  // namespace

// per-lane A operands of the DBF MFMA (k1_dbf_mtd, k_dbf): lane l holds A[row l&15][channel 4j + l>>4];
// row m of block mb is (beam, part) by `layout`; y = sum_c a[b][c] x_c, a = conj(W[b][c]) (fsf:95) or W[b][c]
void rsp_dbf_atab(const double* W, int B, int C, int conj, int layout, std::vector<double>& atab) {
    typedef std::complex<double> cd;
    auto coef = [&](int b, int c) {
        const size_t i = (size_t)b + (size_t)B * c;
        return conj ? cd(W[2 * i], -W[2 * i + 1]) : cd(W[2 * i], W[2 * i + 1]);
    };
    const K1Cfg kc = k1_cfg(C, B);
    const int mblk = kc.MB, nj = kc.NJ;
    atab.assign((size_t)mblk * nj * 2 * 64, 0.0);
    for (int mb = 0; mb < mblk; ++mb)
        for (int j = 0; j < nj; ++j)
            for (int lane = 0; lane < 64; ++lane) {
                const int m = lane & 15, c = 4 * j + (lane >> 4);
                const int b = mb * 8 + (layout == DBF_ROWS_PAIR ? m >> 1 : m & 7);
                double wr = 0, wi = 0;
                if (b < B && c < C) {
                    wr = coef(b, c).real();
                    wi = coef(b, c).imag();
                }
                const bool im = layout == DBF_ROWS_PAIR ? (m & 1) != 0 : m >= 8;
                atab[((mb * nj + j) * 2 + 0) * 64 + lane] = im ? wi : wr;    // coefficient of Re(x_c)
                atab[((mb * nj + j) * 2 + 1) * 64 + lane] = im ? wr : -wi;   // coefficient of Im(x_c)
            }
}

int rsp_dbf_check_sizes(int64_t P, int64_t N, int64_t C, int64_t B, int precision) {
    if (precision != RSP_C64 && precision != RSP_C128)
        return fail(RSP_ERR_INVALID, "precision must be RSP_C128 or RSP_C64, got %d", precision);
    if (P < 1 || N < 1 || C < 1 || C > 32 || B < 1 || B > 16)
        return fail(RSP_ERR_INVALID, "bad sizes P=%lld N=%lld C=%lld B=%lld (P, N >= 1, 1<=C<=32, 1<=B<=16)", (long long)P,
                    (long long)N, (long long)C, (long long)B);
    // a plane of P N positions, one pad position in complex single; C (or B) of them under 2 GB
    const int64_t esz = precision == RSP_C128 ? 16 : 8, lim = (int64_t)1 << 31;
    if (P >= lim || N >= lim || P * N >= lim || (P * N + 1) * esz * (C > B ? C : B) >= lim)
        return fail(RSP_ERR_UNSUPPORTED, "%lld x %lld positions of %lld channels: the kernel addresses a cube with 32-bit offsets (< 2 GB)",
                    (long long)P, (long long)N, (long long)(C > B ? C : B));
    return RSP_OK;
}

int rsp_dbf_check_args(const void* plan, const void* cube, int dtype, const void* W, const void* out) {
    if (dtype != RSP_C64 && dtype != RSP_C128) return fail(RSP_ERR_INVALID, "unknown dtype %d", dtype);
    if (!W) return fail(RSP_ERR_INVALID, "null argument: W (the DBF weights, B x C)");
    if (!plan || !cube || !out) return fail(RSP_ERR_INVALID, "null argument");
    return RSP_OK;
}

DbfDesc dbf_desc(int S, int C, int B, int pitch, int opitch, int prec) {
    const unsigned esz = prec == RSP_PREC_F64 ? 16 : 8;
    return DbfDesc{S, C, B, pitch, opitch, (unsigned)C * (unsigned)pitch * esz, (unsigned)B * (unsigned)opitch * esz};
}

// ---- the stand-alone MTD of any length (k_mtd_any) ----
int rsp_mtd_check_sizes(int64_t P, int64_t G, int64_t n_maps, int64_t nfft, int precision, int* nfft_out) {
    if (precision != RSP_C64 && precision != RSP_C128)
        return fail(RSP_ERR_INVALID, "precision must be RSP_C128 or RSP_C64, got %d", precision);
    if (nfft == 0) nfft = P;
    if (P < 1 || G < 1 || n_maps < 1 || nfft < P)
        return fail(RSP_ERR_INVALID, "bad sizes P=%lld G=%lld n_maps=%lld nfft=%lld (P, G, n_maps >= 1, nfft >= P or 0)",
                    (long long)P, (long long)G, (long long)n_maps, (long long)nfft);
    if (nfft > RSP_MTD_MAX_NFFT)
        return fail(RSP_ERR_UNSUPPORTED, "nfft=%lld: a transform holds at most RSP_MTD_MAX_NFFT = %d points", (long long)nfft,
                    RSP_MTD_MAX_NFFT);
    // nfft >= P: the output is the larger side
    const int64_t esz = precision == RSP_C128 ? 16 : 8, lim = (int64_t)1 << 31;
    if (G >= lim || n_maps >= lim || G * n_maps >= lim || G * n_maps * nfft * esz >= lim)
        return fail(RSP_ERR_UNSUPPORTED, "%lld x %lld columns of %lld points: the kernel addresses a cube of less than 2 GB",
                    (long long)G, (long long)n_maps, (long long)nfft);
    if (nfft_out) *nfft_out = (int)nfft;
    return RSP_OK;
}

MtdDesc mtd_desc(int P, int G, int n_maps, int nfft, int shift, bool has_win, int prec) {
    MtdDesc d{};
    d.P = P;
    d.G = G;
    d.n_maps = n_maps;
    d.nfft = nfft;
    d.chirp = is_pow2(nfft) ? 0 : 1;
    d.L = d.chirp ? mtd_chirp_len(nfft) : nfft;
    d.lgL = ilog2i(d.L);
    d.cols = mtd_cols(d.L, prec);
    d.col_tiles = (G + d.cols - 1) / d.cols;
    d.shift = shift ? 1 : 0;
    d.has_win = has_win ? 1 : 0;
    return d;
}

namespace {
const long double kPiL = 3.141592653589793238462643383279502884L;
// one rounding from the long double value to the precision, held in a double
double round_prec(long double x, int prec) { return prec == RSP_PREC_F64 ? (double)x : (double)(float)x; }
// In-place forward FFT of n = 2^k points in long double (radix 2, roots from one table)
void fft_ld(std::vector<long double>& re, std::vector<long double>& im) {
    const int n = (int)re.size();
    std::vector<long double> rc(n / 2 + 1), rs(n / 2 + 1);
    for (int k = 0; k < n / 2; ++k) {
        rc[k] = cosl(-2.0L * kPiL * (long double)k / (long double)n);
        rs[k] = sinl(-2.0L * kPiL * (long double)k / (long double)n);
    }
    for (int i = 1, j = 0; i < n; ++i) {
        int bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) {
            std::swap(re[i], re[j]);
            std::swap(im[i], im[j]);
        }
    }
    for (int len = 2; len <= n; len <<= 1)
        for (int i = 0; i < n; i += len)
            for (int k = 0; k < len / 2; ++k) {
                const long double wr = rc[k * (n / len)], wi = rs[k * (n / len)];
                const int a = i + k, b = i + k + len / 2;
                const long double vr = re[b] * wr - im[b] * wi, vi = re[b] * wi + im[b] * wr;
                re[b] = re[a] - vr;
                im[b] = im[a] - vi;
                re[a] += vr;
                im[a] += vi;
            }
}
}  // namespace

void rsp_mtd_tables(int nfft, int prec, std::vector<cd>& out) {
    out.clear();
    if (is_pow2(nfft)) return;
    const int M = mtd_chirp_len(nfft);
    std::vector<long double> wr(nfft), wi(nfft), br(M, 0.0L), bi(M, 0.0L);
    for (int m = 0; m < nfft; ++m) {   // the phase as an integer mod 2 nfft before any floating point
        const int64_t e = ((int64_t)m * m) % (2 * (int64_t)nfft);
        const long double a = -kPiL * (long double)e / (long double)nfft;
        wr[m] = cosl(a);
        wi[m] = sinl(a);
        br[m] = wr[m];   // conj(w) wrapped round M: entries m and M - m
        bi[m] = -wi[m];
        if (m) {
            br[M - m] = wr[m];
            bi[M - m] = -wi[m];
        }
    }
    fft_ld(br, bi);
    out.reserve((size_t)nfft + M);
    for (int m = 0; m < nfft; ++m) out.push_back(cd(round_prec(wr[m], prec), round_prec(wi[m], prec)));
    for (int k = 0; k < M; ++k) out.push_back(cd(round_prec(br[k] / (long double)M, prec), round_prec(bi[k] / (long double)M, prec)));
}

void rsp_mtd_twiddles(int lgL, std::vector<cd>& out) {
    out.clear();
    build_plan_twiddles(plan_pow2(lgL), out, true);
    build_plan_twiddles(plan_rev(plan_pow2(lgL)), out, true);
}

size_t k1_tiled_lds(const Geometry& g, bool rq) {
    return ((size_t)g.B * g.NT * g.Ppad + (rq ? rq_table_elems(g.twq_elems, g.P) : g.P)) * cplx_bytes(g);
}

// tile buffers x 2 | FFT twiddles (<= P) | two MFMA row blocks' Atab when B > 8 (k1p_dbf_mtd ALDS)
size_t k1p_lds(const Geometry& g) {
    return ((size_t)2 * g.B * g.NT * g.Ppad + g.P) * cplx_bytes(g) +
           (g.B > 8 ? (size_t)2 * k1_cfg(g.C, g.B).NJ * 2 * 64 * (cplx_bytes(g) / 2) : 0);
}

// tile | twQ | W_P^i | Atab (MB x NJ x 2 x 64 <= 1024 reals: CP <= 16)
size_t k1q_lds(const Geometry& g) {
    return ((size_t)g.B * g.NT * g.Ppad + rq_table_elems(g.twq_elems, g.P)) * cplx_bytes(g) + (size_t)1024 * (cplx_bytes(g) / 2);
}

size_t mtd_cols_lds(const Geometry& g) { return ((size_t)16 * g.Ppad + g.P) * cplx_bytes(g); }

bool k1_persistent_fits(const Geometry& g) {
    const int pts = g.prec == RSP_PREC_F64 ? 8 : 16;   // FFT points per thread (k1p_pts)
    return g.pow2P && g.logP >= 6 && g.logP <= 8 && k1p_tpw(g) > 0 && k1p_lds(g) <= RSP_LDS_BYTES &&
           g.B * g.NT * g.P <= pts * K1_THREADS && g.ncu > 0 && !g.k1_tiled;
}

K1Route k1_route(const Geometry& g, int mode) {
    const K1Cfg kc = k1_cfg(g.C, g.B);
    K1Route r;
    r.lgp2 = g.pow2P ? g.logP : 0;   // k_mtd_cols<T, LGP>: the Stockham passes for P = 16 .. 512, else the direct DFT
    r.kernel = K1K_TILED;
    r.tpw = 0;
    r.transform = g.pow2P ? (k1_dif(g.logP, kc.CP) ? K1X_DIF : K1X_STOCKHAM) : (g.rqQ > 0 ? K1X_FACTORED : K1X_DIRECT);
    if (mode == 3 && k1_persistent_fits(g)) {
        // 2 TPW sub-tiles per wave only where an instantiation exists (K1Cfg::twice_ok); otherwise
        // the tiled kernel
        const bool twice = k1p_tpw(g) == 2 * kc.TPW;
        if (!twice || kc.twice_ok) {
            r.kernel = K1K_PERSISTENT;
            r.tpw = twice ? 2 * kc.TPW : kc.TPW;
            return r;
        }
    }
    // the persistent factored-DFT K1 for C <= 16 when one load round of at most 16 16-B cube loads
    // per lane covers a tile (register budget: no scratch); otherwise the tiled kernel
    if (kc.CP <= 16 && mode == 3 && k1q_fits(g) && k1q_tpw(g) * kc.NJ <= 16) {
        r.kernel = K1K_PERSISTENT_FACTORED;
        r.tpw = k1q_tpw(g);
    }
    return r;
}

int rsp_plan_check_args(const rsp_sig_config* cfg, const rsp_cfar_params* cfar, const rsp_cluster_params* cluster,
                        const rsp_precomputed* pre, const rsp_plan_options* opt) {
    if (!cfg || !cfar || !cluster || !pre || !opt) return fail(RSP_ERR_INVALID, "null argument");
    if (opt->precision != RSP_C64 && opt->precision != RSP_C128)
        return fail(RSP_ERR_INVALID, "precision must be RSP_C128 or RSP_C64, got %d", opt->precision);
    if (opt->flags & ~(RSP_PLAN_K1_TILED | RSP_PLAN_MONOPULSE_COMPLEX | RSP_PLAN_K2_ALL_ROWS))
        return fail(RSP_ERR_INVALID, "unknown plan flags 0x%x", opt->flags);
    const int C = cfg->channel_num, B = cfg->beam_num, P = cfg->prtNum, N = cfg->point_PRT;
    const int g1 = pre->N_gate_narrow, g2 = pre->N_gate_medium, g3 = pre->N_gate_long, G = pre->N_total_gate;
    if (C < 1 || C > 32 || B < 1 || B > 16 || P < 2 || N < 2)
        return fail(RSP_ERR_INVALID, "bad sizes C=%d B=%d P=%d N=%d (1<=C<=32, 1<=B<=16)", C, B, P, N);
    if (P % 2) return fail(RSP_ERR_UNSUPPORTED, "odd prtNum %d (complex64 pulse pairs are loaded as 16 B)", P);
    if (g1 < 0 || g2 < 0 || g3 < 0 || G != g1 + g2 + g3 || G < 1) return fail(RSP_ERR_INVALID, "gate counts inconsistent");
    if (!pre->DBF_coeffs_data_C || !pre->MF_narrow || !pre->MF_medium_fft || !pre->MF_long_fft || !pre->MTD_win ||
        !pre->range_axis || !pre->velocity_axis || !pre->beam_angles_deg || (B > 1 && !pre->k_slopes_LUT))
        return fail(RSP_ERR_INVALID, "precomputed_data field missing");
    if (opt->frames_per_launch < 1 || opt->frames_per_launch > RSP_MAX_F)
        return fail(RSP_ERR_INVALID, "frames_per_launch must be 1..%d", RSP_MAX_F);
    const size_t esz = opt->precision == RSP_C128 ? 16 : 8;
    if ((size_t)C * N * P * esz >= ((size_t)1 << 31))
        return fail(RSP_ERR_UNSUPPORTED, "echo cube of %zu bytes: the kernels address one frame with 32-bit offsets (< 2 GB)",
                    (size_t)C * N * P * esz);
    return RSP_OK;
}

int rsp_plan_derive(const rsp_sig_config* cfg, const rsp_cfar_params* cfar, const rsp_cluster_params*,
                    const rsp_precomputed* pre, const rsp_plan_options* opt, int ncu, PlanHost* out) {
    PlanHost& h = *out;
    h = PlanHost();
    Geometry& g = h.g;
    const int C = cfg->channel_num, B = cfg->beam_num, P = cfg->prtNum, N = cfg->point_PRT, G = pre->N_total_gate;
    g.prec = opt->precision == RSP_C128 ? RSP_PREC_F64 : RSP_PREC_F32;
    g.k1_tiled = (opt->flags & RSP_PLAN_K1_TILED) ? 1 : 0;
    g.mono_c = (opt->flags & RSP_PLAN_MONOPULSE_COMPLEX) ? 1 : 0;
    g.C = C; g.B = B; g.P = P; g.N = N; g.G = G;
    g.cpitch = N * P;
    g.Gp = (G + 3) & ~3;
    g.refR = cfar->refCells_R; g.guardR = cfar->guardCells_R; g.refV = cfar->refCells_V; g.guardV = cfar->guardCells_V;
    g.T = cfar->T_CFAR;
    g.max_dets = 1;   // per launch: the lane's list capacity (launch_batch)
    g.ncu = ncu;
    {   // the most detections a frame can have: every cell under test of every beam pair (fsf:192-213)
        const int64_t nv = std::max(P - 2 * (g.refV + g.guardV), 0), nr = std::max(G - 2 * (g.refR + g.guardR), 0);
        h.det_bound = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)std::max(B - 1, 0) * nv * nr, 1 << 30));
    }
    if (g.refR < 1 || g.refV < 1 || g.guardR < 0 || g.guardV < 0) return fail(RSP_ERR_INVALID, "bad CFAR window");
    std::vector<Interval> U;
    int rc;
    if ((rc = derive_segments(cfg, pre, h, U)) || (rc = derive_k1_tile(g, U)) || (rc = derive_k2_jobs(h)) ||
        (rc = derive_k3_tiling(g)))
        return rc;
    build_tables(pre, h);
    if ((rc = derive_k2_sets(h))) return rc;
    h.z_elems = (size_t)B * g.nzc * g.NZ * P;
    h.rdm_elems = (size_t)B * P * G;
    h.mag_elems = (size_t)B * P * g.Gp;
    return RSP_OK;
}

void rsp_fill_sizes(const Geometry& g, int det_bound, rsp_sizes* s) {
    s->cube_elems = (int64_t)g.cpitch * g.C;
    s->rdm_elems = (int64_t)g.P * g.G * g.B;
    s->cfar_map_elems = (int64_t)g.P * g.G * std::max(g.B - 1, 0);
    s->P = g.P; s->N = g.N; s->C = g.C; s->B = g.B; s->G = g.G;
    s->used_samples = g.nU;
    s->max_detections = det_bound;
    s->n_stages = 3;
    s->precision = g.prec == RSP_PREC_F64 ? RSP_C128 : RSP_C64;
    s->elem_bytes = (int32_t)cplx_bytes(g);
}

void rsp_fill_k1_route(const Geometry& g, rsp_k1_route* out) {
    static_assert(K1K_TILED == RSP_K1_KERNEL_TILED && K1K_PERSISTENT == RSP_K1_KERNEL_PERSISTENT &&
                      K1K_PERSISTENT_FACTORED == RSP_K1_KERNEL_PERSISTENT_FACTORED &&
                      K1X_STOCKHAM == RSP_K1_TRANSFORM_STOCKHAM && K1X_DIF == RSP_K1_TRANSFORM_DIF &&
                      K1X_FACTORED == RSP_K1_TRANSFORM_FACTORED && K1X_DIRECT == RSP_K1_TRANSFORM_DIRECT,
                  "K1Route's values are rsp.h's");
    const K1Route r = k1_route(g, 3);   // the frame chain's launch (launch_k1 mode 3)
    out->kernel = r.kernel;
    out->transform = r.transform;
    out->R = g.rqR;
    out->Q = g.rqQ;
    out->NT = g.NT;
    out->Ppad = g.Ppad;
    out->tiles_per_wave = r.tpw;
    out->stage2_lgp = r.lgp2;
}

void rsp_fill_k3_tiling(const Geometry& g, rsp_k3_tiling* out) {
    out->fast = k3_fast_params(g) ? 1 : 0;   // launch_k3_p's choice of instantiation
    out->RT = g.cfar_RT;
    out->hR = g.cfar_hR;
    out->W = g.cfar_W;
    out->n_tiles = k3_ntiles(g);
    out->n_bands = g.cfar_nband;
    out->VB = g.cfar_VB;
    out->rows = g.cfar_rows;
}

void rsp_fill_k2_layout(const Geometry& g, const int32_t gates[RSP_MAX_SEG], rsp_k2_layout* out) {
    *out = rsp_k2_layout{};
    out->k2_pts = g.k2_pts;
    out->wg_per_cu = k2_wg_per_cu(g);   // launch_k2_p's choice of instantiation
    out->NZ = g.NZ;
    out->nseg = g.nseg;
    out->njobs = g.njobs;
    out->nwg = g.nwg_k2;
    for (int slot = 0, q = 0; slot < RSP_MAX_SEG && q < g.nseg; ++slot) {
        if (gates[slot] <= 0) continue;   // derive_segments skips it
        const SegDesc& s = g.segs[q++];
        rsp_k2_segment& o = out->seg[slot];
        o.present = 1;
        o.type = s.type;
        o.ga = s.ga; o.gb = s.gb;
        o.seg_lo = s.seg_lo; o.lo = s.lo; o.hi = s.hi;
        o.Ls = s.Ls; o.ntaps = s.ntaps; o.delay = s.delay;
        o.Lh = s.Lh; o.M = s.M; o.V = s.V; o.nblocks = s.nblocks;
        o.rows_per_wg = s.rows_per_wg;
    }
}

extern "C" int32_t rsp_plan_describe(const rsp_sig_config* cfg, const rsp_cfar_params* cfar, const rsp_cluster_params* cluster,
                                     const rsp_precomputed* pre, const rsp_plan_options* opt, int32_t ncu, rsp_sizes* sizes,
                                     rsp_k1_route* route) {
    int rc = rsp_plan_check_args(cfg, cfar, cluster, pre, opt);
    if (rc) return rc;
    PlanHost h;
    if ((rc = rsp_plan_derive(cfg, cfar, cluster, pre, opt, ncu, &h))) return rc;
    if (sizes) rsp_fill_sizes(h.g, h.det_bound, sizes);
    if (route) rsp_fill_k1_route(h.g, route);
    return RSP_OK;
}

extern "C" int32_t rsp_plan_describe_k3(const rsp_sig_config* cfg, const rsp_cfar_params* cfar, const rsp_cluster_params* cluster,
                                        const rsp_precomputed* pre, const rsp_plan_options* opt, int32_t ncu,
                                        rsp_k3_tiling* tiling) {
    int rc = rsp_plan_check_args(cfg, cfar, cluster, pre, opt);
    if (rc) return rc;
    PlanHost h;
    if ((rc = rsp_plan_derive(cfg, cfar, cluster, pre, opt, ncu, &h))) return rc;
    if (tiling) rsp_fill_k3_tiling(h.g, tiling);
    return RSP_OK;
}

extern "C" int32_t rsp_plan_describe_k2(const rsp_sig_config* cfg, const rsp_cfar_params* cfar, const rsp_cluster_params* cluster,
                                        const rsp_precomputed* pre, const rsp_plan_options* opt, int32_t ncu,
                                        rsp_k2_layout* layout) {
    int rc = rsp_plan_check_args(cfg, cfar, cluster, pre, opt);
    if (rc) return rc;
    PlanHost h;
    if ((rc = rsp_plan_derive(cfg, cfar, cluster, pre, opt, ncu, &h))) return rc;
    const int32_t gates[RSP_MAX_SEG] = {pre->N_gate_narrow, pre->N_gate_medium, pre->N_gate_long};
    if (layout) rsp_fill_k2_layout(h.g, gates, layout);
    return RSP_OK;
}

int rsp_fill_k2_records(const std::vector<K2Rec>& rec, rsp_k2_record* out, int32_t cap, int32_t* n) {
    if (cap < 0 || (cap > 0 && !out)) return fail(RSP_ERR_INVALID, "bad record buffer (capacity %d)", cap);
    const size_t m = std::min((size_t)cap, rec.size());
    for (size_t i = 0; i < m; ++i) out[i] = rsp_k2_record{rec[i].seg, rec[i].blk, rec[i].row0, rec[i].wg};
    if (n) *n = (int32_t)rec.size();
    return RSP_OK;
}

extern "C" int32_t rsp_plan_describe_k2_records(const rsp_sig_config* cfg, const rsp_cfar_params* cfar,
                                                const rsp_cluster_params* cluster, const rsp_precomputed* pre,
                                                const rsp_plan_options* opt, int32_t ncu, rsp_k2_record* out, int32_t cap,
                                                int32_t* n) {
    int rc = rsp_plan_check_args(cfg, cfar, cluster, pre, opt);
    if (rc) return rc;
    PlanHost h;
    if ((rc = rsp_plan_derive(cfg, cfar, cluster, pre, opt, ncu, &h))) return rc;
    return rsp_fill_k2_records(h.k2rec, out, cap, n);
}

int rsp_fill_k2_row_set(const K2Rows rows[3], const std::vector<K2Rec>* const rec[3], int32_t which, rsp_k2_row_set* set,
                        rsp_k2_record* out, int32_t cap, int32_t* n) {
    if (which < 0 || which > 2) return fail(RSP_ERR_INVALID, "row set %d (RSP_K2_ROWS_ALL, _BAND or _EDGE)", which);
    const K2Rows& r = rows[which];
    if (set) *set = rsp_k2_row_set{r.n, r.base, r.split, r.gap, r.total, (int32_t)rec[which]->size()};
    return rsp_fill_k2_records(*rec[which], out, cap, n);
}

extern "C" int32_t rsp_plan_describe_k2_row_set(const rsp_sig_config* cfg, const rsp_cfar_params* cfar,
                                                const rsp_cluster_params* cluster, const rsp_precomputed* pre,
                                                const rsp_plan_options* opt, int32_t ncu, int32_t which,
                                                rsp_k2_row_set* set, rsp_k2_record* out, int32_t cap, int32_t* n) {
    int rc = rsp_plan_check_args(cfg, cfar, cluster, pre, opt);
    if (rc) return rc;
    PlanHost h;
    if ((rc = rsp_plan_derive(cfg, cfar, cluster, pre, opt, ncu, &h))) return rc;
    const std::vector<K2Rec>* const rec[3] = {&h.k2rec, &h.k2rec_band, &h.k2rec_edge};
    return rsp_fill_k2_row_set(h.k2rows, rec, which, set, out, cap, n);
}

// ---- stage-3 range CFAR (debug_simulated_data_processing_v2.m:419-511) ----
int rsp_stage3_derive(int P, const int32_t* gates, const rsp_stage3_cfar_params* prm, S3Desc* out) {
    if (!gates || !prm || !out) return fail(RSP_ERR_INVALID, "null argument");
    const int64_t G = (int64_t)gates[0] + gates[1] + gates[2];
    if (P < 1 || gates[0] < 0 || gates[1] < 0 || gates[2] < 0 || G < 1 || G > INT32_MAX)
        return fail(RSP_ERR_INVALID, "bad map shape P=%d segments %d, %d, %d", P, gates[0], gates[1], gates[2]);
    const int r = prm->refCells_R, s = prm->saveCells_R;
    if (r < 1 || s < 0) return fail(RSP_ERR_INVALID, "bad CFAR window refCells_R=%d saveCells_R=%d (r >= 1, s >= 0)", r, s);
    if (prm->CFARmethod_R != 0 && prm->CFARmethod_R != 1)
        return fail(RSP_ERR_INVALID, "CFARmethod_R must be 0 (greatest of) or 1 (smallest of), got %d", prm->CFARmethod_R);
    if (prm->MTD_0v_num < 0) return fail(RSP_ERR_INVALID, "MTD_0v_num must be >= 0, got %d", prm->MTD_0v_num);
    if (!std::isfinite(prm->T_CFAR) || prm->T_CFAR <= 0) return fail(RSP_ERR_INVALID, "T_CFAR must be finite and > 0, got %g", prm->T_CFAR);
    const int64_t H = (int64_t)r + s;
    if (H > RSP_S3_HMAX)
        return fail(RSP_ERR_INVALID, "CFAR window refCells_R + saveCells_R = %lld exceeds the kernel's tile halo %d", (long long)H,
                    RSP_S3_HMAX);
    S3Desc d{};
    d.P = P;
    d.G = (int)G;
    int a = 0;
    for (int k = 0; k < 3; ++k) {
        if (gates[k] > 0 && gates[k] < 2 * H)
            return fail(RSP_ERR_INVALID, "segment %d has %d columns, fewer than 2 (saveCells_R + refCells_R) = %lld", k, gates[k],
                        (long long)(2 * H));
        d.seg_a[k] = a;
        d.seg_n[k] = gates[k];
        a += gates[k];
    }
    d.r = r; d.s = s; d.H = (int)H;
    d.method = prm->CFARmethod_R;
    d.T = prm->T_CFAR;
    // zero_v_center = round(P / 2) + 1, MATLAB round: half away from zero (:447)
    const int64_t zc = (int64_t)std::floor(P / 2.0 + 0.5) + 1, z = prm->MTD_0v_num;
    d.z0 = (int)std::max<int64_t>(1, zc - z) - 1;
    d.z1 = (int)std::min<int64_t>(P, zc + z) - 1;
    *out = d;
    return RSP_OK;
}

extern "C" int32_t rsp_stage3_describe(const rsp_sig_config* cfg, const rsp_precomputed* pre,
                                       const rsp_stage3_cfar_params* params, rsp_stage3_info* info) {
    if (!cfg || !pre || !params) return fail(RSP_ERR_INVALID, "null argument");
    if (pre->N_total_gate != pre->N_gate_narrow + pre->N_gate_medium + pre->N_gate_long)
        return fail(RSP_ERR_INVALID, "gate counts inconsistent");
    const int32_t gates[3] = {pre->N_gate_narrow, pre->N_gate_medium, pre->N_gate_long};
    S3Desc d;
    int rc = rsp_stage3_derive(cfg->prtNum, gates, params, &d);
    if (rc || !info) return rc;
    info->P = d.P;
    info->G = d.G;
    for (int k = 0; k < 3; ++k) {
        info->seg_first[k] = d.seg_a[k] + 1;
        info->seg_len[k] = d.seg_n[k];
    }
    info->notch_first = d.z0 + 1;
    info->notch_last = d.z1 + 1;
    info->halo = d.H;
    info->max_halo = RSP_S3_HMAX;
    info->chunk = RSP_S3_CH;
    info->rows = RSP_S3_ROWS;
    return RSP_OK;
}

// ---- Doppler CA-CFAR (main_simulate_echoes_with_array_v3.m:278-314) ----
int rsp_vcfar_derive(int P, int G, const rsp_vcfar_params* prm, VcDesc* out) {
    if (!prm || !out) return fail(RSP_ERR_INVALID, "null argument");
    if (P < 1 || G < 1) return fail(RSP_ERR_INVALID, "bad map shape P=%d G=%d", P, G);
    const int r = prm->refCells_V, g = prm->guardCells_V;
    if (r < 1) return fail(RSP_ERR_INVALID, "refCells_V must be >= 1, got %d", r);
    if (g < 0 || (g & 1))
        return fail(RSP_ERR_INVALID, "guardCells_V must be >= 0 and even (the reference indexes with guardCells_V / 2), got %d", g);
    if (prm->method < 0 || prm->method > 2)
        return fail(RSP_ERR_INVALID, "method must be 0 (CA), 1 (GOCA) or 2 (SOCA), got %d", prm->method);
    if (!std::isfinite(prm->T_CFAR) || prm->T_CFAR <= 0) return fail(RSP_ERR_INVALID, "T_CFAR must be finite and > 0, got %g", prm->T_CFAR);
    const int64_t halo = (int64_t)r + g / 2;
    if (halo > RSP_VC_HMAX)
        return fail(RSP_ERR_INVALID, "CFAR window refCells_V + guardCells_V / 2 = %lld exceeds the kernel's tile halo %d",
                    (long long)halo, RSP_VC_HMAX);
    VcDesc d{};
    d.P = P;
    d.G = G;
    d.r = r; d.h = g / 2; d.halo = (int)halo;
    d.method = prm->method;
    d.T = prm->T_CFAR;
    *out = d;
    return RSP_OK;
}

extern "C" int32_t rsp_vcfar_describe(int32_t P, int32_t G, const rsp_vcfar_params* params, rsp_vcfar_info* info) {
    VcDesc d;
    if (!params) return fail(RSP_ERR_INVALID, "null argument");
    int rc = rsp_vcfar_derive(P, G, params, &d);
    if (rc || !info) return rc;
    info->P = d.P;
    info->G = d.G;
    info->halo = d.halo;
    info->max_halo = RSP_VC_HMAX;
    info->rows = RSP_VC_ROWS;
    info->cols = RSP_VC_COLS;
    info->row_tiles = (d.P + RSP_VC_ROWS - 1) / RSP_VC_ROWS;
    info->col_tiles = (d.G + RSP_VC_COLS - 1) / RSP_VC_COLS;
    return RSP_OK;
}

// ---- cross GOCA-CFAR as a map detector (fsf:192-213) ----
int rsp_xcfar_derive(int P, int G, const rsp_cfar_params* prm, XcDesc* out) {
    if (!prm || !out) return fail(RSP_ERR_INVALID, "null argument");
    if (P < 1 || G < 1) return fail(RSP_ERR_INVALID, "bad map shape P=%d G=%d", P, G);
    const int rR = prm->refCells_R, gR = prm->guardCells_R, rV = prm->refCells_V, gV = prm->guardCells_V;
    if (rR < 1) return fail(RSP_ERR_INVALID, "refCells_R must be >= 1, got %d", rR);
    if (rV < 1) return fail(RSP_ERR_INVALID, "refCells_V must be >= 1, got %d", rV);
    if (gR < 0) return fail(RSP_ERR_INVALID, "guardCells_R must be >= 0, got %d", gR);
    if (gV < 0) return fail(RSP_ERR_INVALID, "guardCells_V must be >= 0, got %d", gV);
    if (!std::isfinite(prm->T_CFAR) || prm->T_CFAR <= 0) return fail(RSP_ERR_INVALID, "T_CFAR must be finite and > 0, got %g", prm->T_CFAR);
    const int64_t hR = (int64_t)rR + gR, hV = (int64_t)rV + gV;
    XcDesc d{};
    d.P = P;
    d.G = G;
    d.rR = rR; d.gR = gR; d.rV = rV; d.gV = gV;
    d.T = prm->T_CFAR;
    if (G > 2 * hR && P > 2 * hV) {   // cells under test (fsf:192-193); otherwise no tile needs a halo
        if (hR > RSP_XC_HMAX_R)
            return fail(RSP_ERR_INVALID, "CFAR window refCells_R + guardCells_R = %lld exceeds the kernel's tile halo %d",
                        (long long)hR, RSP_XC_HMAX_R);
        if (hV > RSP_XC_HMAX_V)
            return fail(RSP_ERR_INVALID, "CFAR window refCells_V + guardCells_V = %lld exceeds the kernel's tile halo %d",
                        (long long)hV, RSP_XC_HMAX_V);
        d.hR = (int)hR; d.hV = (int)hV;
        d.r0 = (int)hR; d.r1 = G - (int)hR;
        d.v0 = (int)hV; d.v1 = P - (int)hV;
    }
    *out = d;
    return RSP_OK;
}

extern "C" int32_t rsp_xcfar_describe(int32_t P, int32_t G, const rsp_cfar_params* params, rsp_xcfar_info* info) {
    XcDesc d;
    if (!params) return fail(RSP_ERR_INVALID, "null argument");
    int rc = rsp_xcfar_derive(P, G, params, &d);
    if (rc || !info) return rc;
    const int64_t hR = (int64_t)d.rR + d.gR, hV = (int64_t)d.rV + d.gV;
    info->P = d.P;
    info->G = d.G;
    info->hR = (int32_t)std::min<int64_t>(hR, INT32_MAX);
    info->hV = (int32_t)std::min<int64_t>(hV, INT32_MAX);
    info->max_hR = RSP_XC_HMAX_R;
    info->max_hV = RSP_XC_HMAX_V;
    info->rows = RSP_XC_ROWS;
    info->cols = RSP_XC_COLS;
    info->row_tiles = (int32_t)(((int64_t)d.P + RSP_XC_ROWS - 1) / RSP_XC_ROWS);   // 64-bit: P up to INT32_MAX
    info->col_tiles = (int32_t)(((int64_t)d.G + RSP_XC_COLS - 1) / RSP_XC_COLS);
    const bool any = d.r1 > d.r0;
    info->r0 = any ? d.r0 + 1 : 1;   // 1-based, inclusive; first > last: none
    info->r1 = any ? d.r1 : 0;
    info->v0 = any ? d.v0 + 1 : 1;
    info->v1 = any ? d.v1 : 0;
    return RSP_OK;
}

// ---- detection on any RD cube (k_pairsum, k_xcfar, k_s9) ----
int rsp_detect_check_sizes(int64_t V, int64_t G, int64_t B, int precision, const rsp_cfar_params* prm, XcDesc* out) {
    if (precision != RSP_C64 && precision != RSP_C128)
        return fail(RSP_ERR_INVALID, "precision must be RSP_C128 or RSP_C64, got %d", precision);
    if (B < 2) return fail(RSP_ERR_INVALID, "B=%lld: a pair sum needs at least 2 beams", (long long)B);
    if (V < 1 || G < 1) return fail(RSP_ERR_INVALID, "bad cube shape V=%lld G=%lld B=%lld", (long long)V, (long long)G, (long long)B);
    const int64_t lim = (int64_t)1 << 31;
    XcDesc d;
    int rc = rsp_xcfar_derive((int)std::min(V, lim - 1), (int)std::min(G, lim - 1), prm, &d);
    if (rc) return rc;
    // the cube is the larger side (B complex planes against B - 1 real ones)
    const int64_t esz = precision == RSP_C128 ? 16 : 8;
    if (V >= lim || G >= lim || B >= lim || V * G >= lim || V * G * B >= lim || V * G * B * esz >= lim)
        return fail(RSP_ERR_UNSUPPORTED, "%lld x %lld x %lld cube: the kernels address a cube and its pair-sum maps of less than 2 GB each",
                    (long long)V, (long long)G, (long long)B);
    if ((V + RSP_XC_ROWS - 1) / RSP_XC_ROWS > 65535 || B - 1 > 65535)
        return fail(RSP_ERR_UNSUPPORTED, "%lld Doppler rows, %lld maps: the CFAR kernel's grid holds 65535 x %d rows and 65535 maps",
                    (long long)V, (long long)(B - 1), RSP_XC_ROWS);
    if (out) *out = d;
    return RSP_OK;
}

extern "C" int32_t rsp_detect_describe(int32_t V, int32_t G, int32_t B, int32_t precision, const rsp_cfar_params* params,
                                       rsp_detect_info* info) {
    XcDesc d;
    int rc = rsp_detect_check_sizes(V, G, B, precision, params, &d);
    if (rc || !info) return rc;
    *info = rsp_detect_info{};
    info->V = V;
    info->G = G;
    info->B = B;
    info->n_pairs = B - 1;
    info->rows = RSP_PS_ROWS;
    info->cols = RSP_PS_COLS;
    info->row_tiles = (V + RSP_PS_ROWS - 1) / RSP_PS_ROWS;
    info->col_tiles = (G + RSP_PS_COLS - 1) / RSP_PS_COLS;
    info->lds_bytes = (int32_t)ps_lds_bytes(precision == RSP_C128 ? 8 : 4);
    const bool any = d.r1 > d.r0;
    info->r0 = any ? d.r0 + 1 : 1;   // 1-based, inclusive; first > last: none (as rsp_xcfar_describe)
    info->r1 = any ? d.r1 : 0;
    info->v0 = any ? d.v0 + 1 : 1;
    info->v1 = any ? d.v1 : 0;
    info->cells_under_test = (int64_t)(d.r1 - d.r0) * (d.v1 - d.v0);
    info->max_detections = (int64_t)(B - 1) * info->cells_under_test;
    return RSP_OK;
}

extern "C" int32_t rsp_dbf_describe(int32_t P, int32_t N, int32_t C, int32_t B, int32_t precision, rsp_dbf_info* info) {
    int rc = rsp_dbf_check_sizes(P, N, C, B, precision);
    if (rc || !info) return rc;
    const int prec = precision == RSP_C128 ? RSP_PREC_F64 : RSP_PREC_F32;
    const K1Cfg kc = k1_cfg(C, B);
    const int S = P * N;
    info->positions = S;
    info->CP = kc.CP;
    info->BMAX = kc.BMAX;
    info->sub_tile = dbf_sub_tile(prec);
    info->tiles_per_wave = kc.TPW;
    info->waves = RSP_DBF_THREADS / 64;
    info->rounds = RSP_DBF_ROUNDS;
    info->wg_positions = dbf_wg_positions(C, B, prec);
    info->workgroups = dbf_workgroups(S, C, B, prec);
    info->tail_positions = S % info->sub_tile;
    info->row_layout = prec == RSP_PREC_F64 ? DBF_ROWS_SPLIT : DBF_ROWS_PAIR;
    info->pitch = dbf_pitch(S, prec);
    return RSP_OK;
}

extern "C" int32_t rsp_dbf_table(const double* W, int32_t B, int32_t C, int32_t conj, int32_t row_layout, double* out,
                                 int32_t cap, int32_t* n) {
    if (!W || !n || cap < 0 || (cap > 0 && !out)) return fail(RSP_ERR_INVALID, "null argument");
    if (C < 1 || C > 32 || B < 1 || B > 16) return fail(RSP_ERR_INVALID, "bad sizes C=%d B=%d (1<=C<=32, 1<=B<=16)", C, B);
    if (row_layout != DBF_ROWS_SPLIT && row_layout != DBF_ROWS_PAIR) return fail(RSP_ERR_INVALID, "unknown row layout %d", row_layout);
    std::vector<double> t;
    rsp_dbf_atab(W, B, C, conj, row_layout, t);
    *n = (int32_t)t.size();
    for (int i = 0; i < cap && i < (int)t.size(); ++i) out[i] = t[i];
    return RSP_OK;
}

extern "C" int32_t rsp_mtd_describe(int32_t P, int32_t G, int32_t nfft, int32_t precision, rsp_mtd_info* info) {
    int n = 0;
    int rc = rsp_mtd_check_sizes(P, G, 1, nfft, precision, &n);
    if (rc || !info) return rc;
    const int prec = precision == RSP_C128 ? RSP_PREC_F64 : RSP_PREC_F32;
    const MtdDesc d = mtd_desc(P, G, 1, n, 1, false, prec);
    info->P = P;
    info->G = G;
    info->nfft = n;
    info->route = d.chirp ? RSP_MTD_ROUTE_CHIRPZ : RSP_MTD_ROUTE_POW2;
    info->M = d.L;
    info->cols = d.cols;
    info->col_tiles = d.col_tiles;
    info->lds_bytes = (int32_t)mtd_lds_bytes(d.L, prec);
    info->table_elems = d.chirp ? n + d.L : 0;
    return RSP_OK;
}

extern "C" int32_t rsp_mtd_table(int32_t nfft, int32_t precision, double* out, int32_t cap, int32_t* n) {
    if (!n || cap < 0 || (cap > 0 && !out)) return fail(RSP_ERR_INVALID, "null argument");
    int rc = rsp_mtd_check_sizes(nfft, 1, 1, nfft, precision, nullptr);
    if (rc) return rc;
    std::vector<cd> t;
    rsp_mtd_tables(nfft, precision == RSP_C128 ? RSP_PREC_F64 : RSP_PREC_F32, t);
    *n = (int32_t)t.size();
    for (int i = 0; i < cap && i < (int)t.size(); ++i) {
        out[2 * i] = t[i].real();
        out[2 * i + 1] = t[i].imag();
    }
    return RSP_OK;
}

extern "C" int32_t rsp_plan_describe_dbf_table(const rsp_sig_config* cfg, const rsp_cfar_params* cfar,
                                               const rsp_cluster_params* cluster, const rsp_precomputed* pre,
                                               const rsp_plan_options* opt, int32_t ncu, double* out, int32_t cap, int32_t* n) {
    if (!n || cap < 0 || (cap > 0 && !out)) return fail(RSP_ERR_INVALID, "null argument");
    int rc = rsp_plan_check_args(cfg, cfar, cluster, pre, opt);
    if (rc) return rc;
    PlanHost h;
    if ((rc = rsp_plan_derive(cfg, cfar, cluster, pre, opt, ncu, &h))) return rc;
    *n = (int32_t)h.atab.size();
    for (int i = 0; i < cap && i < (int)h.atab.size(); ++i) out[i] = h.atab[i];
    return RSP_OK;
}

// ---- pulse compression for any pulse and beam count (k_pc_pack, k2_pc, k_pc_unpack) ----
int rsp_pc_derive(const Geometry& base, int64_t P, int64_t B, PcDesc* out, std::vector<K2Rec>* rec) {
    if (P < 1 || B < 1) return fail(RSP_ERR_INVALID, "bad sizes P=%lld B=%lld (P, B >= 1)", (long long)P, (long long)B);
    // beams, z and the result each under 2 GB: the kernels and k2_pc's buffer resources take 32-bit byte
    // offsets (rsp_plan_check_args' limit for a frame)
    const int64_t esz = base.prec == RSP_PREC_F64 ? 16 : 8, lim = (int64_t)1 << 31;
    const int64_t nzc = (base.nU + RSP_PC_NZ - 1) / RSP_PC_NZ, row = std::max<int64_t>(std::max<int64_t>(base.N, base.G), nzc * RSP_PC_NZ);
    if (P >= lim || B >= lim || P * B >= lim || P * B * row >= lim || P * B * row * esz >= lim)
        return fail(RSP_ERR_UNSUPPORTED,
                    "%lld pulses x %lld beams of %d samples, %d gates: the kernels address the beams, the compacted rows and the result with 32-bit offsets (< 2 GB each)",
                    (long long)P, (long long)B, base.N, base.G);
    PcDesc d{};
    Geometry& g = d.g;
    g = base;
    g.P = (int)P;
    g.B = g.C = (int)B;
    g.cpitch = g.N * g.P;
    g.NZ = RSP_PC_NZ;
    g.nzc = (int)nzc;
    std::vector<SegDesc> segs(g.segs, g.segs + g.nseg);
    std::vector<K2Job> jobs;
    std::vector<K2Rec> local;
    std::vector<K2Rec>& r = rec ? *rec : local;
    int rc = k2_build_records(g, segs, g.B * g.P, &jobs, nullptr, &r);
    if (rc) return rc;
    g.njobs = (int)jobs.size();   // segments x blocks: the base's count
    for (int q = 0; q < g.njobs && q < RSP_MAX_JOBS; ++q) g.jobs[q] = jobs[q];
    g.nwg_k2 = (int)r.size();
    d.rows = K2Rows{g.P, 0, g.P, 0, g.B * g.P};
    d.pack_tiles = (g.P + RSP_PCK_COLS - 1) / RSP_PCK_COLS;
    d.pack_wg = g.nzc * d.pack_tiles * g.B;
    d.unpack_row_tiles = (g.P + RSP_PCU_ROWS - 1) / RSP_PCU_ROWS;
    d.unpack_col_tiles = (g.G + pcu_cols(g.prec) - 1) / pcu_cols(g.prec);
    d.unpack_row_groups = (d.unpack_row_tiles + RSP_PCU_GROUP - 1) / RSP_PCU_GROUP;
    d.unpack_wg = d.unpack_col_tiles * d.unpack_row_groups * g.B;
    d.in_elems = (size_t)P * g.N * B;
    d.z_elems = (size_t)B * g.nzc * g.NZ * P;
    d.out_elems = (size_t)P * g.G * B;
    d.mag_elems = (size_t)P * g.Gp * B;
    if (out) *out = d;
    return RSP_OK;
}

void rsp_fill_pc_info(const PcDesc& d, rsp_pc_info* out) {
    const Geometry& g = d.g;
    *out = rsp_pc_info{};
    out->P = g.P; out->B = g.B; out->N = g.N; out->G = g.G;
    out->nU = g.nU;
    out->n_intervals = g.nivl;
    out->NZ = g.NZ;
    out->nzc = g.nzc;
    out->z_elems = (int64_t)d.z_elems;
    out->pack_rows = RSP_PC_NZ;
    out->pack_cols = RSP_PCK_COLS;
    out->unpack_rows = RSP_PCU_ROWS;
    out->unpack_cols = pcu_cols(g.prec);
    out->pack_wg = d.pack_wg;
    out->k2_wg = g.nwg_k2;
    out->unpack_wg = d.unpack_wg;
    out->k2_wg_per_cu = k2_wg_per_cu(g);
    out->pack_lds_bytes = (int32_t)pck_lds_bytes(g.prec);
    out->unpack_lds_bytes = (int32_t)pcu_lds_bytes(g.prec);
    static_assert(RSP_MAX_IVL == 4, "rsp_pc_info::ivl_lo / ivl_start");
    for (int q = 0; q < g.nivl; ++q) {
        out->ivl_lo[q] = g.ivl_lo[q];
        out->ivl_start[q] = g.ivl_start[q];
    }
}

extern "C" int32_t rsp_plan_describe_pc(const rsp_sig_config* cfg, const rsp_cfar_params* cfar, const rsp_cluster_params* cluster,
                                        const rsp_precomputed* pre, const rsp_plan_options* opt, int32_t ncu, int32_t P, int32_t B,
                                        rsp_pc_info* info) {
    if (!cfg) return fail(RSP_ERR_INVALID, "null argument");
    // The base: a plan of the same waveform for the smallest frame a plan takes (two pulses, one beam).  The
    // segments, the sample intervals and k2_pts, all this stage reads, depend on neither count.
    rsp_sig_config c2 = *cfg;
    c2.prtNum = 2;
    c2.beam_num = 1;
    int rc = rsp_plan_check_args(&c2, cfar, cluster, pre, opt);
    if (rc) return rc;
    PlanHost h;
    if ((rc = rsp_plan_derive(&c2, cfar, cluster, pre, opt, ncu, &h))) return rc;
    PcDesc d;
    if ((rc = rsp_pc_derive(h.g, P, B, &d, nullptr)) || !info) return rc;
    rsp_fill_pc_info(d, info);
    return RSP_OK;
}

// ---- digital down-conversion (k_ddc) ----
int rsp_ddc_derive(int64_t P, int64_t N, int64_t C, int64_t L, int64_t D, int64_t off, int precision, DdcDesc* out) {
    if (precision != RSP_C64 && precision != RSP_C128)
        return fail(RSP_ERR_INVALID, "precision must be RSP_C128 or RSP_C64, got %d", precision);
    if (P < 1 || N < 1 || C < 1)
        return fail(RSP_ERR_INVALID, "bad sizes P=%lld N=%lld C=%lld (P, N, C >= 1)", (long long)P, (long long)N, (long long)C);
    if (L < 1 || L > RSP_DDC_MAX_TAPS)
        return fail(RSP_ERR_INVALID, "L=%lld taps: 1 <= L <= RSP_DDC_MAX_TAPS = %d", (long long)L, RSP_DDC_MAX_TAPS);
    if (D < 1 || D > RSP_DDC_MAX_D) return fail(RSP_ERR_INVALID, "D=%lld: 1 <= D <= RSP_DDC_MAX_D = %d", (long long)D, RSP_DDC_MAX_D);
    if (off < 0 || off >= D) return fail(RSP_ERR_INVALID, "off=%lld: 0 <= off < D = %lld", (long long)off, (long long)D);
    // the input (reals) and the output (complex) each under 2 GB: the kernel's buffer resources take 32-bit
    // byte offsets.  No <= N, so the three counts and P N C bound every product below.
    const int64_t rs = precision == RSP_C128 ? 8 : 4, lim = (int64_t)1 << 31;
    const int64_t No = off < N ? (N - off + D - 1) / D : 0;
    if (P >= lim || N >= lim || C >= lim || P * N >= lim || P * N * C >= lim || P * N * C * rs >= lim ||
        P * No * C * 2 * rs >= lim)
        return fail(RSP_ERR_UNSUPPORTED,
                    "%lld pulses x %lld samples x %lld channels, %lld outputs a pulse: the kernel addresses the input and the result with 32-bit offsets (< 2 GB each)",
                    (long long)P, (long long)N, (long long)C, (long long)No);
    DdcDesc d{};
    d.P = (int)P; d.N = (int)N; d.C = (int)C; d.No = (int)No;
    d.L = (int)L; d.D = (int)D; d.off = (int)off;
    d.TP = 1;
    while (d.TP < 64 && d.TP < d.P) d.TP *= 2;
    d.lgTP = ilog2i(d.TP);
    // rows of TP reals and one complex NCO value that fit the budget beside the taps
    const int row_bytes = (int)rs * (d.TP + 2), R = (int)((RSP_DDC_LDS_BUDGET - 16 - L * rs) / row_bytes);
    d.KL = RSP_DDC_THREADS / d.TP;
    while (d.KL > 1 && (d.KL - 1) * d.D + std::min(d.L, 16) > R) d.KL /= 2;
    d.LC = std::min(d.L, R - (d.KL - 1) * d.D);
    d.KPT = 1;
    while (d.KPT < RSP_DDC_MAX_KPT && d.KL * d.KPT < d.No && (d.KL * (d.KPT + 1) - 1) * d.D + d.LC <= R) ++d.KPT;
    d.TK = d.KL * d.KPT;
    d.rows = (d.TK - 1) * d.D + d.LC;
    d.k_tiles = (d.No + d.TK - 1) / d.TK;   // No = 0 (N <= off): nothing to launch
    d.p_tiles = (d.P + d.TP - 1) / d.TP;
    d.threads = std::max(64, d.TP * d.KL);
    d.in_bytes = (unsigned)(P * N * C * rs);
    ddc_set_opitch(&d, (unsigned)(P * No), (unsigned)(2 * rs));
    d.ms_bytes = ((unsigned)d.rows * 2u * (unsigned)rs + 15u) & ~15u;
    d.lds_bytes = d.ms_bytes + (unsigned)d.rows * (unsigned)d.TP * (unsigned)rs + (unsigned)d.L * (unsigned)rs;
    if (out) *out = d;
    return RSP_OK;
}

void rsp_fill_ddc_info(const DdcDesc& d, int precision, rsp_ddc_info* out) {
    *out = rsp_ddc_info{};
    out->P = d.P; out->N = d.N; out->C = d.C; out->L = d.L; out->D = d.D; out->off = d.off;
    out->No = d.No;
    out->TP = d.TP; out->TK = d.TK;
    out->in_rows = d.rows;
    out->k_tiles = d.k_tiles; out->p_tiles = d.p_tiles;
    out->workgroups = d.k_tiles * d.p_tiles * d.C;
    out->lds_bytes = (int32_t)d.lds_bytes;
    out->tap_chunk = d.LC;
    out->threads = d.threads;
    out->k_per_thread = d.KPT;
    out->in_bytes = d.in_bytes;
    out->out_bytes = d.out_bytes;
}

extern "C" int32_t rsp_ddc_describe(int32_t P, int32_t N, int32_t C, int32_t L, int32_t D, int32_t off, int32_t precision,
                                    rsp_ddc_info* info) {
    DdcDesc d;
    const int rc = rsp_ddc_derive(P, N, C, L, D, off, precision, &d);
    if (rc || !info) return rc;
    rsp_fill_ddc_info(d, precision, info);
    return RSP_OK;
}

extern "C" int32_t rsp_ddc_phase_word(double f0, double fs, uint64_t* w) {
    if (!w) return fail(RSP_ERR_INVALID, "null argument");
    if (!std::isfinite(f0) || !std::isfinite(fs) || !(fs > 0))
        return fail(RSP_ERR_INVALID, "f0=%g fs=%g: both finite, fs > 0", f0, fs);
    // the fraction of a turn per sample in [0, 1), then 64 bits of it: the product is below 2^64 + 1/2, and a
    // value that rounds to 2^64 is the word 0
    long double t = (long double)f0 / (long double)fs;
    t -= std::floor(t);
    const long double s = std::nearbyint(std::ldexp(t, 64));
    *w = s >= 18446744073709551616.0L ? 0 : (uint64_t)s;
    return RSP_OK;
}
