// Stand-alone check of the stand-alone pulse compression's host code for the AddressSanitizer / UBSan build of
// tests/test_pc_host.py: plain C++, no device.
//
// rsp_plan_describe_pc and rsp_pc_derive on a small three-segment waveform, in either precision, over the
// pulse and beam counts of tests/_pc_cases.py (1, 2, 7, 16, 21, 63 .. 65, 130, 255 .. 257, 333; 1, 3, 13
// beams), the reference's 332 x 13, counts below 1, products that overflow 32 bits and the 2 GB edge from
// both sides:
//   * a refusal exactly when include/rsp.h says so, with the status it names and a message; the configuration's
//     own prtNum (odd, huge) and beam_num change nothing;
//   * the derived Geometry carries the caller's P and B, NZ = 8 and nzc = ceil(nU / 8); z, the result and the
//     scratch map are sized from them; the pack and unpack grids (the unpack's in groups of 8 pulse tiles) cover
//     every element once;
//   * the record table holds, per (segment, block), ceil(B P / rows_per_wg) workgroups whose first rows are the
//     multiples of rows_per_wg, each once, with distinct wg indices; the jobs in the Geometry describe the same
//     table; every row of the set {P, 0, P, 0, B P} maps to its own rho < B P.
// Exit status 0: all held; 1 with a message otherwise.  Sanitizer reports fail the run by themselves.
#include <algorithm>
#include <climits>
#include <cmath>
#include <complex>
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include "rsp_geometry.h"   // rsp.h

static int fail(const char* what, long long a = 0, long long b = 0, long long c = 0, long long d = 0) {
    std::printf("FAILED: %s (%lld, %lld, %lld, %lld)\n", what, a, b, c, d);
    return 1;
}

static std::vector<double> spectrum(int n, int lh) {   // DFT of a short filter, interleaved re/im
    std::vector<double> out(2 * (size_t)n);
    for (int k = 0; k < n; ++k) {
        std::complex<double> acc = 0;
        for (int t = 0; t < lh; ++t) acc += (1.0 + 0.1 * t) * std::polar(1.0, -2.0 * M_PI * k * t / n);
        out[2 * k] = acc.real();
        out[2 * k + 1] = acc.imag();
    }
    return out;
}

int main() {
    const int C = 8, N = 512, g1 = 20, g2 = 40, g3 = 61, G = g1 + g2 + g3, nf_med = 128, nf_long = 256, PB = 16, BB = 13;
    std::vector<double> W(2 * (size_t)BB * C, 0.5), taps(9, 0.25), win(PB, 1.0), ra(G, 1.0), va(PB, 1.0), ang(BB, 1.0), kl(BB, 1.0);
    const std::vector<double> mf_med = spectrum(nf_med, 12), mf_long = spectrum(nf_long, 40);
    rsp_cluster_params cl = {30.0, 0.4, 5.0};
    rsp_cfar_params cf = {5, 10, 5, 10, 8.0};
    rsp_precomputed pre = {};
    pre.DBF_coeffs_data_C = W.data();
    pre.MF_narrow = taps.data(); pre.n_MF_narrow = (int)taps.size(); pre.fir_delay = 4;
    pre.MF_medium_fft = mf_med.data(); pre.N_fft_med = nf_med;
    pre.MF_long_fft = mf_long.data(); pre.N_fft_long = nf_long;
    pre.N_gate_narrow = g1; pre.N_gate_medium = g2; pre.N_gate_long = g3; pre.N_total_gate = G;
    pre.seg_start_narrow = 10; pre.seg_start_medium = N + 1 - 100; pre.seg_start_long = N + 1 - 200;
    pre.MTD_win = win.data(); pre.range_axis = ra.data(); pre.velocity_axis = va.data();
    pre.deltaR = 6.0; pre.deltaV = 0.5;
    pre.beam_angles_deg = ang.data(); pre.k_slopes_LUT = kl.data();

    const long long Ps[] = {INT_MIN, -1, 0, 1, 2, 7, 16, 21, 63, 64, 65, 130, 255, 256, 257, 332, 333, 4096, 1 << 16, 1 << 18,
                            (1 << 18) + 1, 1 << 20, INT_MAX};
    const long long Bs[] = {INT_MIN, 0, 1, 3, 13, 64, 1 << 12, INT_MAX};
    const int precs[] = {RSP_C128, RSP_C64};
    long long cases = 0, accepted = 0;
    for (int prec : precs) {
        rsp_plan_options opt = {0, 1, prec, 0};
        const long long esz = prec == RSP_C128 ? 16 : 8, lim = 1ll << 31;
        // the base a plan of this waveform would hand to rsp_pc_derive
        rsp_sig_config cfg = {3e8, 25e6, 3e9, 2e-4, 0.1, 0.05, PB, N, C, BB};
        PlanHost h;
        if (rsp_plan_check_args(&cfg, &cf, &cl, &pre, &opt) != RSP_OK || rsp_plan_derive(&cfg, &cf, &cl, &pre, &opt, 256, &h) != RSP_OK)
            return fail("the base plan", prec);
        const Geometry& base = h.g;
        const long long nzc = (base.nU + 7) / 8, row = std::max<long long>(std::max<long long>(N, G), 8 * nzc);
        for (long long P : Ps) for (long long B : Bs) {
            ++cases;
            rsp_pc_info info;
            // a configuration whose own counts a plan refuses: odd, and far too large
            rsp_sig_config odd = cfg;
            odd.prtNum = 333 + 2 * (int)(cases % 1000) * 1000;
            odd.beam_num = 1 + (int)(cases % 16);
            const int rc = rsp_plan_describe_pc(&odd, &cf, &cl, &pre, &opt, 256, (int)P, (int)B, &info);
            const std::string msg = rsp_last_error();
            PcDesc d;
            std::vector<K2Rec> rec;
            const int rd = rsp_pc_derive(base, P, B, &d, &rec);
            if (rc != rd) return fail("describe_pc and rsp_pc_derive disagree", P, B, rc, rd);
            int want = RSP_OK;
            if (P < 1 || B < 1) want = RSP_ERR_INVALID;
            else if ((__int128)P * B * row * esz >= lim) want = RSP_ERR_UNSUPPORTED;
            if (rc != want) return fail("status", P, B, rc, want);
            if (rc != RSP_OK) {
                if (msg.empty()) return fail("no message", P, B, rc);
                continue;
            }
            ++accepted;
            const Geometry& g = d.g;
            if (g.P != P || g.B != B || g.NZ != RSP_PC_NZ || g.nzc != nzc || g.N != N || g.G != G || g.Gp != ((G + 3) & ~3) ||
                g.nU != base.nU || g.nivl != base.nivl || g.k2_pts != base.k2_pts || g.nseg != base.nseg)
                return fail("geometry", P, B);
            if (info.P != P || info.B != B || info.N != N || info.G != G || info.nU != g.nU || info.n_intervals != g.nivl ||
                info.NZ != 8 || info.nzc != nzc || info.z_elems != B * nzc * P * 8 || info.k2_wg != (int)rec.size() ||
                info.pack_wg != d.pack_wg || info.unpack_wg != d.unpack_wg)
                return fail("info", P, B);
            if (d.z_elems != (size_t)(B * nzc * P * 8) || d.out_elems != (size_t)(P * G * B) || d.in_elems != (size_t)(P * N * B) ||
                d.mag_elems != (size_t)(P * g.Gp * B))
                return fail("buffer sizes", P, B);
            if ((long long)d.z_elems * esz >= lim || (long long)d.in_elems * esz >= lim || (long long)d.out_elems * esz >= lim)
                return fail("a buffer of 2 GB was accepted", P, B);
            // the grids: pulse tiles x chunks x beams, and gate tiles x pulse tiles x beams
            const long long pt = (P + RSP_PCK_COLS - 1) / RSP_PCK_COLS, rt = (P + RSP_PCU_ROWS - 1) / RSP_PCU_ROWS;
            const long long ct = (G + pcu_cols(g.prec) - 1) / pcu_cols(g.prec);
            const long long rgr = (rt + RSP_PCU_GROUP - 1) / RSP_PCU_GROUP;
            if (d.pack_wg != nzc * pt * B || d.pack_tiles != pt || d.unpack_wg != ct * rgr * B || d.unpack_row_tiles != rt || d.unpack_row_groups != rgr ||
                d.unpack_col_tiles != ct)
                return fail("grids", P, B, d.pack_wg, d.unpack_wg);
            if (info.pack_lds_bytes != (long long)pck_lds_bytes(g.prec) || info.unpack_lds_bytes != (long long)pcu_lds_bytes(g.prec) ||
                (size_t)info.pack_lds_bytes > RSP_LDS_BYTES || (info.unpack_lds_bytes / esz / RSP_PCU_ROWS) % 2 != 1)
                return fail("LDS", info.pack_lds_bytes, info.unpack_lds_bytes);
            // the row set and the record table
            const long long rows = P * B;
            if (d.rows.n != P || d.rows.base != 0 || d.rows.split != P || d.rows.gap != 0 || d.rows.total != rows) return fail("row set", P, B);
            if (rows <= 4096) {
                std::set<int> rho;
                for (int i = 0; i < rows; ++i) rho.insert(k2_rho(d.rows, g.P, i));
                if ((long long)rho.size() != rows || *rho.begin() != 0 || *rho.rbegin() != rows - 1) return fail("rho", P, B);
            }
            long long nwg = 0;
            std::set<int> wgs;
            for (int q = 0; q < g.nseg; ++q) {
                const SegDesc& s = g.segs[q];
                const long long per = (rows + s.rows_per_wg - 1) / s.rows_per_wg, nb = s.type == 1 ? s.nblocks : 1;
                for (int blk = 0; blk < nb; ++blk) {
                    std::set<int> firsts;
                    for (const K2Rec& r : rec)
                        if (r.seg == q && r.blk == blk) {
                            if (r.row0 % s.rows_per_wg || r.row0 < 0 || r.row0 >= rows) return fail("row0", P, B, r.row0);
                            firsts.insert(r.row0);
                            wgs.insert(r.wg);
                        }
                    if ((long long)firsts.size() != per) return fail("records of a block", P, B, q, blk);
                    nwg += per;
                }
            }
            if (nwg != (long long)rec.size() || (long long)wgs.size() != nwg || g.nwg_k2 != nwg) return fail("record count", P, B, nwg);
            long long from_jobs = 0;
            for (int j = 0; j < g.njobs; ++j) {
                if (g.jobs[j].wg_begin != from_jobs) return fail("job order", P, B, j);
                from_jobs += g.jobs[j].wg_count;
            }
            if (from_jobs != nwg) return fail("jobs", P, B, from_jobs, nwg);
        }
    }
    if (rsp_plan_describe_pc(nullptr, &cf, &cl, &pre, nullptr, 256, 4, 1, nullptr) != RSP_ERR_INVALID) return fail("null config");
    std::printf("%lld cases, %lld accepted\n", cases, accepted);
    return accepted > 100 ? 0 : fail("grid too small", cases, accepted);
}
