// Stand-alone check of the stand-alone MTD's host code for the AddressSanitizer / UBSan build of
// tests/test_mtd_abi.py: plain C++, no device.
//
// rsp_mtd_describe over P, G, nfft and both precisions, and rsp_mtd_table with cap = 0, a short cap and
// the full length into heap buffers of exactly cap entries (an overrun is the sanitizer's to report), at
// nfft = 1, 2, 3, 2047, 2048 and a few lengths between:
//   * a refusal exactly when include/rsp.h says so;
//   * route, M (the least power of two >= 2 nfft - 1 on the chirp-z route), col_tiles = ceil(G / cols),
//     lds_bytes within the 160 KiB of a CU, table_elems = nfft + M or 0, and *n = table_elems;
//   * a short read returns the head of the full table; w[0] = 1 and |w[m]| = 1 to rounding.
// Exit status 0: all held; 1 with a message otherwise.  Sanitizer reports fail the run by themselves.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rsp_geometry.h"   // rsp.h

static int fail(const char* what, long long a = 0, long long b = 0, long long c = 0, long long d = 0) {
    std::printf("FAILED: %s (%lld, %lld, %lld, %lld)\n", what, a, b, c, d);
    return 1;
}

int main() {
    const int Ps[] = {-1, 0, 1, 2, 3, 100, 332, 2047, 2048, 2049}, Gs[] = {0, 1, 5, 3404, 65536, 1 << 30};
    const int Ns[] = {0, 1, 2, 3, 16, 333, 512, 2047, 2048, 2049}, precs[] = {RSP_C64, RSP_C128, 7};
    long long cases = 0, accepted = 0;
    for (int P : Ps) for (int G : Gs) for (int nf : Ns) for (int pr : precs) {
        rsp_mtd_info info;
        const int rc = rsp_mtd_describe(P, G, nf, pr, &info);
        ++cases;
        const long long n = nf == 0 ? P : nf, esz = pr == RSP_C128 ? 16 : 8;
        const bool sizes = (pr == RSP_C64 || pr == RSP_C128) && P >= 1 && G >= 1 && n >= P;
        const bool ok = sizes && n <= RSP_MTD_MAX_NFFT && (long long)G * n * esz < (1LL << 31);
        if ((rc == RSP_OK) != ok) return fail("refusal", P, G, nf, pr);
        if (!ok) {
            const int want = !sizes ? RSP_ERR_INVALID : RSP_ERR_UNSUPPORTED;
            if (rc != want) return fail("refusal code", P, G, nf, rc);
            continue;
        }
        ++accepted;
        const bool pow2 = (n & (n - 1)) == 0;
        if (info.P != P || info.G != G || info.nfft != n) return fail("sizes echoed", P, G, nf);
        if (info.route != (pow2 ? RSP_MTD_ROUTE_POW2 : RSP_MTD_ROUTE_CHIRPZ)) return fail("route", P, G, nf);
        if (pow2 ? info.M != n : (info.M < 2 * n - 1 || info.M / 2 >= 2 * n - 1 || (info.M & (info.M - 1)))) return fail("M", n, info.M);
        if (info.cols < 1 || info.col_tiles != (G + info.cols - 1) / info.cols) return fail("tiles", G, info.cols, info.col_tiles);
        if (info.lds_bytes < (long long)info.cols * info.M * esz || info.lds_bytes > 160 * 1024) return fail("lds", n, info.lds_bytes);
        if (info.table_elems != (pow2 ? 0 : n + info.M)) return fail("table_elems", n, info.table_elems);
    }
    if (rsp_mtd_describe(332, 3404, 512, RSP_C128, nullptr) != RSP_OK) return fail("info may be NULL");

    for (int nf : {1, 2, 3, 5, 17, 332, 2047, 2048})
        for (int pr : {RSP_C64, RSP_C128}) {
            rsp_mtd_info info;
            if (rsp_mtd_describe(nf, 1, nf, pr, &info) != RSP_OK) return fail("describe", nf);
            int32_t n = -1;
            if (rsp_mtd_table(nf, pr, nullptr, 0, &n) != RSP_OK || n != info.table_elems) return fail("cap 0", nf, n);
            std::vector<double> full(2 * (size_t)n);   // exactly n entries (none for a power of two)
            int32_t n2 = -1;
            if (rsp_mtd_table(nf, pr, n ? full.data() : nullptr, n, &n2) != RSP_OK || n2 != n) return fail("full", nf, n2);
            if (n) {
                const int cap = n < 7 ? n - 1 : 7;
                double* head = new double[2 * (size_t)cap];   // a short cap: the head of the table
                if (rsp_mtd_table(nf, pr, head, cap, &n2) != RSP_OK || n2 != n) return fail("short", nf, n2);
                const bool same = std::memcmp(head, full.data(), 2 * (size_t)cap * sizeof(double)) == 0;
                delete[] head;
                if (!same) return fail("short read differs", nf);
                if (full[0] != 1.0 || full[1] != 0.0) return fail("w[0]", nf);
                const double u = pr == RSP_C128 ? 1.2e-16 : 6e-8;
                for (int m = 0; m < nf; ++m)
                    if (std::fabs(std::hypot(full[2 * m], full[2 * m + 1]) - 1.0) > 2 * u) return fail("|w|", nf, m);
                if (pr == RSP_C64)
                    for (double v : full)
                        if ((double)(float)v != v) return fail("not a single-precision value", nf);
            }
        }
    int32_t n = 0;
    if (rsp_mtd_table(0, RSP_C128, nullptr, 0, &n) != RSP_ERR_INVALID) return fail("nfft 0");
    if (rsp_mtd_table(2049, RSP_C128, nullptr, 0, &n) != RSP_ERR_UNSUPPORTED) return fail("nfft 2049");
    if (rsp_mtd_table(5, 3, nullptr, 0, &n) != RSP_ERR_INVALID) return fail("precision");
    if (rsp_mtd_table(5, RSP_C128, nullptr, 4, &n) != RSP_ERR_INVALID) return fail("null out with a cap");
    if (rsp_mtd_table(5, RSP_C128, nullptr, 0, nullptr) != RSP_ERR_INVALID) return fail("null n");
    std::printf("%lld cases, %lld accepted\n", cases, accepted);
    return 0;
}
