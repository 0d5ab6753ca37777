// Stand-alone check of the detector's host code for the AddressSanitizer / UBSan build of
// tests/test_detect_host.py: plain C++, no device.
//
// rsp_detect_describe and rsp_detect_check_sizes over a grid of V, G, B, precisions and windows (sizes
// whose products overflow 32 bits, one beam, the 2 GB edge in either precision, the CFAR envelope's corner
// and one step past it):
//   * a refusal exactly when include/rsp.h says so, with the status it names; the CFAR refusals carry
//     rsp_xcfar_describe's own message;
//   * the tiles cover the cube once; the cells under test are rsp_xcfar_describe's; max_detections =
//     (B - 1) x cells under test; the LDS tile has an odd row stride and fits a CU.
// Exit status 0: all held; 1 with a message otherwise.  Sanitizer reports fail the run by themselves.
#include <climits>
#include <cmath>
#include <cstdio>
#include <string>

#include "rsp_geometry.h"   // rsp.h

static int fail(const char* what, long long a = 0, long long b = 0, long long c = 0, long long d = 0) {
    std::printf("FAILED: %s (%lld, %lld, %lld, %lld)\n", what, a, b, c, d);
    return 1;
}

int main() {
    const int Vs[] = {0, 1, 31, 63, 64, 65, 333, 512, 1 << 13, 1 << 20, INT_MAX}, Gs[] = {-1, 1, 3, 4, 63, 64, 65, 3404, 1 << 13, 1 << 22};
    const int Bs[] = {-1, 0, 1, 2, 3, 13, 70000, INT_MAX};
    const rsp_cfar_params wins[] = {{5, 10, 5, 10, 8.0}, {1, 0, 1, 0, 1.5}, {20, 12, 40, 24, 1.2}, {20, 13, 40, 24, 1.2},
                                    {5, 10, 0, 10, 8.0}, {5, 10, 5, 10, NAN}};
    const int precs[] = {RSP_C128, RSP_C64, 0};
    long long cases = 0, accepted = 0;
    for (int V : Vs) for (int G : Gs) for (int B : Bs) for (const rsp_cfar_params& w : wins) for (int prec : precs) {
        rsp_detect_info info;
        XcDesc d;
        const int rc = rsp_detect_describe(V, G, B, prec, &w, &info);
        const std::string msg = rsp_last_error();
        const int rd = rsp_detect_check_sizes(V, G, B, prec, &w, &d);
        ++cases;
        if (rc != rd) return fail("describe and check_sizes disagree", V, G, B, rc);
        int want = RSP_OK;
        const long long esz = prec == RSP_C128 ? 16 : 8, lim = 1ll << 31;
        if (prec != RSP_C128 && prec != RSP_C64) want = RSP_ERR_INVALID;
        else if (B < 2 || V < 1 || G < 1) want = RSP_ERR_INVALID;
        else {
            rsp_xcfar_info xi;
            const int rx = rsp_xcfar_describe(V, G, &w, &xi);
            const std::string xmsg = rsp_last_error();
            if (rx != RSP_OK) {
                want = rx;
                if (rc == rx && msg != xmsg) return fail("the CFAR refusal's message", V, G, B);
            } else if ((__int128)V * G * B * esz >= lim || (V + 31) / 32 > 65535 || B - 1 > 65535)
                want = RSP_ERR_UNSUPPORTED;
            else {
                if (rc != RSP_OK) return fail("refused", V, G, B, rc);
                if (info.r0 != xi.r0 || info.r1 != xi.r1 || info.v0 != xi.v0 || info.v1 != xi.v1) return fail("cells under test", V, G, B);
                const long long cut = xi.r1 >= xi.r0 ? (long long)(xi.r1 - xi.r0 + 1) * (xi.v1 - xi.v0 + 1) : 0;
                if (info.cells_under_test != cut || info.max_detections != (B - 1) * cut) return fail("counts", V, G, B, cut);
            }
        }
        if (rc != want) return fail("status", V, G, B, rc);
        if (rc != RSP_OK) {
            if (msg.empty()) return fail("no message", V, G, B, rc);
            continue;
        }
        ++accepted;
        if (info.V != V || info.G != G || info.B != B || info.n_pairs != B - 1 || info.rows != RSP_PS_ROWS || info.cols != RSP_PS_COLS)
            return fail("info", V, G, B);
        if ((long long)(info.row_tiles - 1) * info.rows >= V || (long long)info.row_tiles * info.rows < V ||
            (long long)(info.col_tiles - 1) * info.cols >= G || (long long)info.col_tiles * info.cols < G)
            return fail("tiles", V, G, info.row_tiles, info.col_tiles);
        const long long rs = esz / 2;
        if (info.lds_bytes != (long long)ps_lds_bytes(rs) || (info.lds_bytes / rs / info.rows) % 2 != 1 || info.lds_bytes > RSP_LDS_BYTES)
            return fail("LDS", info.lds_bytes);
    }
    const rsp_cfar_params ref{5, 10, 5, 10, 8.0};
    if (rsp_detect_describe(64, 64, 2, RSP_C128, nullptr, nullptr) != RSP_ERR_INVALID) return fail("null params");
    if (rsp_detect_describe(332, 3404, 13, RSP_C128, &ref, nullptr) != RSP_OK) return fail("null info");
    std::printf("%lld cases, %lld accepted\n", cases, accepted);
    return accepted > 300 ? 0 : fail("grid too small", cases, accepted);
}
