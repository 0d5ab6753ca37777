// Stand-alone check of the pulse-compression row sets (rsp_plan_describe_k2_row_set) for the
// AddressSanitizer / UBSan build of tests/test_k2_row_sets.py: plain C++, no device.
//
// For plans over a grid of prtNum, beam counts, precisions and CFAR windows it asserts that
//   * the all-rows set is n = P with the records of rsp_plan_describe_k2_records;
//   * with the 5/5/10/10 window and P > 2 hV (hV = 15) the band set holds exactly the rows
//     [hV, P - hV) of every beam, the edge set the others, and the two together every (beam, row)
//     exactly once; otherwise both are empty;
//   * every table holds, per (segment, block), ceil(total / rows_per_wg) workgroups whose first rows
//     are the multiples of rows_per_wg, each once, and distinct `wg` indices 0 .. nwg - 1.
// Exit status 0: all held; 1 with a message otherwise.  Sanitizer reports fail the run by themselves.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <set>
#include <vector>

#include "rsp.h"

static const int HV = 15;

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

#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            fprintf(stderr, "P=%d B=%d prec=%d: ", P, B, prec); \
            fprintf(stderr, __VA_ARGS__);                     \
            fprintf(stderr, "\n");                            \
            return 1;                                         \
        }                                                     \
    } while (0)

static int one(int P, int B, int prec, bool fast_window) {
    const int C = 8, N = 512, g1 = 20, g2 = 40, g3 = 60, G = g1 + g2 + g3, nf_med = 128, nf_long = 256;
    std::vector<double> W(2 * (size_t)B * C, 0.5), taps(9, 0.25), win(P, 1.0), ra(G, 1.0), va(P, 1.0), ang(B, 1.0),
        kl(std::max(B - 1, 1), 1.0);
    const std::vector<double> mf_med = spectrum(nf_med, 12), mf_long = spectrum(nf_long, 40);
    rsp_sig_config cfg = {3e8, 25e6, 3e9, 2e-4, 0.1, 0.05, P, N, C, B};
    rsp_cluster_params cl = {30.0, 0.4, 5.0};
    rsp_cfar_params cf = {5, 10, 5, 10, 8.0};
    if (!fast_window) cf = {4, 3, 2, 1, 8.0};
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
    rsp_plan_options opt = {0, 1, prec, 0};
    rsp_k2_layout lay;
    CHECK(rsp_plan_describe_k2(&cfg, &cf, &cl, &pre, &opt, 256, &lay) == RSP_OK, "describe_k2: %s", rsp_last_error());
    int rows_per_wg[3], nblk[3], nseg = 0;
    for (int q = 0; q < 3; ++q)
        if (lay.seg[q].present) {
            rows_per_wg[nseg] = lay.seg[q].rows_per_wg;
            nblk[nseg++] = lay.seg[q].type ? lay.seg[q].nblocks : 1;
        }
    std::vector<int> seen((size_t)B * P, 0);
    for (int which = 0; which < 3; ++which) {
        rsp_k2_row_set rs;
        int32_t n = -1;
        CHECK(rsp_plan_describe_k2_row_set(&cfg, &cf, &cl, &pre, &opt, 256, which, &rs, nullptr, 0, &n) == RSP_OK,
              "set %d: %s", which, rsp_last_error());
        CHECK(n == rs.nwg && rs.total == B * rs.n, "set %d: n %d nwg %d total %d", which, n, rs.nwg, rs.total);
        std::vector<rsp_k2_record> rec(std::max(n, 1)), one_short(std::max(n, 1), rsp_k2_record{-7, -7, -7, -7});
        CHECK(rsp_plan_describe_k2_row_set(&cfg, &cf, &cl, &pre, &opt, 256, which, nullptr, rec.data(), n, &n) == RSP_OK, "records");
        if (n > 0) {   // a short buffer is filled to its capacity and no further
            CHECK(rsp_plan_describe_k2_row_set(&cfg, &cf, &cl, &pre, &opt, 256, which, nullptr, one_short.data(), n - 1, nullptr) == RSP_OK, "short");
            CHECK(one_short[n - 1].seg == -7, "set %d: wrote past the capacity", which);
        }
        const bool band_route = fast_window && P > 2 * HV;
        if (which == RSP_K2_ROWS_ALL) {
            CHECK(rs.n == P && rs.base == 0 && rs.gap == 0, "all-rows set");
            int32_t m = 0;
            std::vector<rsp_k2_record> old(std::max(n, 1));
            CHECK(rsp_plan_describe_k2_records(&cfg, &cf, &cl, &pre, &opt, 256, old.data(), n, &m) == RSP_OK && m == n, "records call");
            for (int i = 0; i < n; ++i)
                CHECK(old[i].seg == rec[i].seg && old[i].blk == rec[i].blk && old[i].row0 == rec[i].row0 && old[i].wg == rec[i].wg,
                      "all-rows record %d differs", i);
        } else if (!band_route) {
            CHECK(rs.n == 0 && rs.total == 0 && n == 0, "set %d of a plan without the band route: n %d", which, rs.n);
            continue;
        } else if (which == RSP_K2_ROWS_BAND) {
            CHECK(rs.n == P - 2 * HV && rs.base == HV && rs.gap == 0, "band set n %d base %d", rs.n, rs.base);
        } else {
            CHECK(rs.n == 2 * HV && rs.base == 0 && rs.split == HV && rs.gap == P - 2 * HV, "edge set");
        }
        // the rows of the set, through the documented mapping
        for (int i = 0; i < rs.total; ++i) {
            const int b = i / rs.n, j = i % rs.n, v = rs.base + j + (j >= rs.split ? rs.gap : 0);
            CHECK(b >= 0 && b < B && v >= 0 && v < P, "set %d row %d -> (%d, %d)", which, i, b, v);
            if (which == RSP_K2_ROWS_BAND) CHECK(v >= HV && v < P - HV, "band row %d", v);
            if (which == RSP_K2_ROWS_EDGE) CHECK(v < HV || v >= P - HV, "edge row %d", v);
            if (which != RSP_K2_ROWS_ALL) ++seen[(size_t)b * P + v];
        }
        // the table: per (segment, block) every multiple of rows_per_wg below total once
        std::set<int> wgs;
        std::set<std::vector<int>> keys;
        int want = 0;
        for (int s = 0; s < nseg; ++s) want += nblk[s] * ((rs.total + rows_per_wg[s] - 1) / rows_per_wg[s]);
        CHECK(n == want, "set %d: %d records, %d workgroups expected", which, n, want);
        for (int i = 0; i < n; ++i) {
            const rsp_k2_record& r = rec[i];
            CHECK(r.seg >= 0 && r.seg < nseg && r.blk >= 0 && r.blk < nblk[r.seg], "record %d: seg %d blk %d", i, r.seg, r.blk);
            CHECK(r.row0 >= 0 && r.row0 < rs.total && r.row0 % rows_per_wg[r.seg] == 0, "record %d: row0 %d", i, r.row0);
            CHECK(r.wg >= 0 && r.wg < n && wgs.insert(r.wg).second, "record %d: wg %d", i, r.wg);
            CHECK(keys.insert({r.seg, r.blk, r.row0}).second, "record %d repeats (%d, %d, %d)", i, r.seg, r.blk, r.row0);
        }
    }
    if (fast_window && P > 2 * HV)
        for (size_t i = 0; i < seen.size(); ++i) CHECK(seen[i] == 1, "row %zu covered %d times by band + edge", i, seen[i]);
    return 0;
}

int main() {
    const int Ps[] = {16, 30, 32, 34, 60, 62, 64, 128, 166, 256, 332};
    const int Bs[] = {1, 2, 3, 4, 13, 16};
    int n = 0;
    for (int P : Ps)
        for (int B : Bs)
            for (int prec : {RSP_C128, RSP_C64})
                for (bool fast : {true, false}) {
                    if (one(P, B, prec, fast)) return 1;
                    ++n;
                }
    // a set index out of range is refused
    rsp_k2_row_set rs;
    if (rsp_plan_describe_k2_row_set(nullptr, nullptr, nullptr, nullptr, nullptr, 256, 0, &rs, nullptr, 0, nullptr) == RSP_OK) return 1;
    printf("k2 row sets: %d plans checked\n", n);
    return 0;
}
