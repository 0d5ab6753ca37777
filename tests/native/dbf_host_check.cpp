// Stand-alone check of the stage-1 DBF's host code for the AddressSanitizer / UBSan build of
// tests/test_dbf_host.py: plain C++, no device.
//
//   * rsp_dbf_table over every (C, B) of the envelope, both conj values and both row layouts, with W in
//     a heap block of exactly 2 B C doubles (a read past it is a sanitizer report): the table has
//     MB x CP / 4 x 2 x 64 entries and y reconstructed from it alone equals the direct sum;
//   * rsp_dbf_describe over a grid of sizes: the workgroups cover the positions exactly once;
//   * the refusals of rsp_dbf_check_sizes / rsp_dbf_check_args;
//   * rsp_stage2_regate on C channels (the raw-cube calls' regating) with exactly sized blocks.
// Exit status 0: all held; 1 with a message otherwise.  Sanitizer reports fail the run by themselves.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "rsp_frame_host.h"   // rsp.h, rsp_geometry.h

typedef std::complex<double> cd;

static int fail(const char* what, int a = 0, int b = 0, int c = 0) {
    std::printf("FAILED: %s (%d, %d, %d)\n", what, a, b, c);
    return 1;
}

static int check_table(int C, int B, int conj, int layout) {
    std::unique_ptr<double[]> W(new double[2 * (size_t)B * C]);
    for (int i = 0; i < 2 * B * C; ++i) W[i] = std::sin(1.0 + 0.37 * i) + 0.01 * i;
    int32_t n = 0;
    if (rsp_dbf_table(W.get(), B, C, conj, layout, nullptr, 0, &n) != RSP_OK) return fail("size query", C, B);
    const int cp = C <= 8 ? 8 : (C <= 16 ? 16 : 32), nj = cp / 4, mbn = B <= 8 ? 1 : 2;
    if (n != mbn * nj * 2 * 64) return fail("table length", C, B, n);
    std::unique_ptr<double[]> t(new double[n]);
    if (rsp_dbf_table(W.get(), B, C, conj, layout, t.get(), n, &n) != RSP_OK) return fail("table", C, B);
    std::vector<cd> x(C);
    for (int c = 0; c < C; ++c) x[c] = cd(std::cos(0.3 * c + 0.1), std::sin(1.7 * c) - 0.2);
    for (int b = 0; b < B; ++b) {
        cd want = 0;
        for (int c = 0; c < C; ++c) {
            const cd w(W[2 * (b + (size_t)B * c)], W[2 * (b + (size_t)B * c) + 1]);
            want += (conj ? std::conj(w) : w) * x[c];
        }
        double part[2];
        for (int p = 0; p < 2; ++p) {
            const int mb = b / 8, bl = b % 8, m = layout == RSP_DBF_ROWS_PAIR ? 2 * bl + p : bl + 8 * p;
            double acc = 0;
            for (int c = 0; c < C; ++c) {
                const int lane = m + 16 * (c % 4), blk = mb * nj + c / 4;
                acc += t[(blk * 2 + 0) * 64 + lane] * x[c].real() + t[(blk * 2 + 1) * 64 + lane] * x[c].imag();
            }
            part[p] = acc;
        }
        if (std::abs(cd(part[0], part[1]) - want) > 1e-13 * (1.0 + std::abs(want))) return fail("reconstruction", C, B, b);
    }
    return 0;
}

int main() {
    int tables = 0, shapes = 0;
    for (int C = 1; C <= 32; ++C)
        for (int B = 1; B <= 16; ++B)
            for (int conj = 0; conj < 2; ++conj)
                for (int layout = 0; layout < 2; ++layout, ++tables)
                    if (check_table(C, B, conj, layout)) return 1;
    const int sizes[] = {1, 2, 15, 16, 17, 31, 32, 33, 35, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049, 100003};
    for (int prec : {RSP_C64, RSP_C128})
        for (int C : {1, 5, 8, 9, 16, 17, 32})
            for (int B : {1, 4, 8, 9, 16})
                for (int S : sizes)
                    for (int P : {1, 3, S}) {
                        if (S % P) continue;
                        rsp_dbf_info d;
                        if (rsp_dbf_describe(P, S / P, C, B, prec, &d) != RSP_OK) return fail("describe", C, B, S);
                        const long long wg = d.wg_positions;
                        if (d.positions != S || wg != (long long)d.waves * d.rounds * d.tiles_per_wave * d.sub_tile ||
                            (d.workgroups - 1) * wg >= S || d.workgroups * wg < S || d.tail_positions != S % d.sub_tile ||
                            d.pitch < S || d.pitch > S + 1 || (prec == RSP_C64 && d.pitch % 2))
                            return fail("coverage", C, B, S);
                        ++shapes;
                    }
    if (rsp_dbf_describe(2, 3, 0, 2, RSP_C128, nullptr) != RSP_ERR_INVALID || rsp_dbf_describe(2, 3, 33, 2, RSP_C128, nullptr) != RSP_ERR_INVALID ||
        rsp_dbf_describe(2, 3, 4, 17, RSP_C128, nullptr) != RSP_ERR_INVALID || rsp_dbf_describe(0, 3, 4, 2, RSP_C128, nullptr) != RSP_ERR_INVALID ||
        rsp_dbf_describe(2, 3, 4, 2, 9, nullptr) != RSP_ERR_INVALID || rsp_dbf_describe(1 << 14, 1 << 14, 32, 16, RSP_C128, nullptr) != RSP_ERR_UNSUPPORTED ||
        rsp_dbf_describe(1 << 20, 1 << 20, 1, 1, RSP_C64, nullptr) != RSP_ERR_UNSUPPORTED || rsp_dbf_describe(2, 3, 4, 2, RSP_C64, nullptr) != RSP_OK)
        return fail("describe refusals");
    int dummy = 0;
    if (rsp_dbf_check_args(&dummy, &dummy, RSP_C128, nullptr, &dummy) != RSP_ERR_INVALID ||
        rsp_dbf_check_args(&dummy, &dummy, 7, &dummy, &dummy) != RSP_ERR_INVALID ||
        rsp_dbf_check_args(nullptr, &dummy, RSP_C64, &dummy, &dummy) != RSP_ERR_INVALID ||
        rsp_dbf_check_args(&dummy, &dummy, RSP_C64, &dummy, &dummy) != RSP_OK)
        return fail("argument refusals");
    // regating of a raw cube: P = 3 pulses, N = 40 samples, C = 5 channels, gated columns 3..6, 10..10, 31..40
    {
        const int P = 3, N = 40, C = 5, ng = 4 + 1 + 10;
        const int32_t cols[6] = {3, 6, 10, 10, 31, 40};
        for (int dtype : {RSP_C64, RSP_C128}) {
            const size_t es = dtype == RSP_C128 ? 16 : 8;
            std::unique_ptr<unsigned char[]> in(new unsigned char[(size_t)P * ng * C * es]);
            for (size_t i = 0; i < (size_t)P * ng * C * es; ++i) in[i] = (unsigned char)(1 + i % 251);
            std::vector<unsigned char> full;
            if (rsp_stage2_regate(P, N, C, in.get(), dtype, ng, cols, full) != RSP_OK) return fail("regate");
            if (full.size() != (size_t)P * N * C * es) return fail("regated size");
            for (int c = 0; c < C; ++c) {
                int g = 0;
                for (int col = 0; col < N; ++col) {
                    const bool in_gate = (col >= 2 && col <= 5) || col == 9 || col >= 30;
                    const unsigned char* f = &full[((size_t)c * N + col) * P * es];
                    for (size_t k = 0; k < P * es; ++k)
                        if (f[k] != (in_gate ? in[((size_t)c * ng + g) * P * es + k] : 0)) return fail("regated bytes", c, col);
                    g += in_gate;
                }
            }
            const int32_t overlap[6] = {3, 6, 6, 6, 31, 40};
            if (rsp_stage2_regate(P, N, C, in.get(), dtype, ng, overlap, full) != RSP_ERR_INVALID) return fail("overlapping gates accepted");
            if (rsp_stage2_regate(P, N, C, in.get(), dtype, ng - 1, cols, full) != RSP_ERR_INVALID) return fail("column count accepted");
        }
    }
    std::printf("%d tables, %d shapes checked\n", tables, shapes);
    return 0;
}
