// Stand-alone check of the cross GOCA-CFAR's host code for the AddressSanitizer / UBSan build of
// tests/test_xcfar_abi.py: plain C++, no device.
//
// rsp_xcfar_describe and rsp_xcfar_derive over a grid of P, G and windows (the envelope's corner, one
// step past it, windows whose sums overflow 32 bits):
//   * a refusal exactly when the definition of include/rsp.h says so;
//   * the tiles cover the map once; the cells under test are those of fsf:192-193, inside the map and
//     a halo away from its edges; the descriptor's tile halos are the window's, or 0 when no cell is
//     under test; the LDS tile of every accepted window fits the 160 KiB of a CU.
// Exit status 0: all held; 1 with a message otherwise.  Sanitizer reports fail the run by themselves.
#include <climits>
#include <cmath>
#include <cstdio>

#include "rsp_geometry.h"   // rsp.h

static int fail(const char* what, long long a = 0, long long b = 0, long long c = 0, long long d = 0) {
    std::printf("FAILED: %s (%lld, %lld, %lld, %lld)\n", what, a, b, c, d);
    return 1;
}

int main() {
    const int Ps[] = {0, 1, 2, 7, 16, 31, 32, 33, 64, 65, 70, 332, 100000}, Gs[] = {-1, 1, 3, 63, 64, 65, 128, 129, 140, 3404, 1 << 20};
    const int refs[] = {0, 1, 5, 40, 64, INT_MAX}, guards[] = {-1, 0, 1, 10, 24, 60, INT_MAX};
    const double Ts[] = {1.0, 0.0, -1.0, NAN, INFINITY};
    long long cases = 0, accepted = 0, empty = 0;
    for (int P : Ps) for (int G : Gs) for (int rR : refs) for (int gR : guards) for (int rV : refs) for (int gV : guards) {
        for (double T : Ts) {
            if (T != 1.0 && (rR != 5 || gV != 10)) continue;   // the T refusals on one window per map
            const rsp_cfar_params prm{rV, gV, rR, gR, T};
            rsp_xcfar_info info;
            XcDesc d;
            const int rc = rsp_xcfar_describe(P, G, &prm, &info), rd = rsp_xcfar_derive(P, G, &prm, &d);
            ++cases;
            const long long hR = (long long)rR + gR, hV = (long long)rV + gV;
            const bool shape = P >= 1 && G >= 1, window = rR >= 1 && rV >= 1 && gR >= 0 && gV >= 0;
            const bool any = shape && window && G > 2 * hR && P > 2 * hV;
            const bool ok = shape && window && std::isfinite(T) && T > 0 && (!any || (hR <= 64 && hV <= 32));
            if ((rc == RSP_OK) != ok || rc != rd) return fail("refusal", P, G, hR, hV);
            if (!ok) {
                if (rc != RSP_ERR_INVALID || !rsp_last_error()[0]) return fail("status / message", P, G, rc);
                continue;
            }
            ++accepted;
            if (info.P != P || info.G != G || info.rows != RSP_XC_ROWS || info.cols != RSP_XC_COLS || info.max_hR != 64 ||
                info.max_hV != 32)
                return fail("info", P, G);
            if ((long long)(info.row_tiles - 1) * info.rows >= P || (long long)info.row_tiles * info.rows < P ||
                (long long)(info.col_tiles - 1) * info.cols >= G || (long long)info.col_tiles * info.cols < G)
                return fail("tiles", P, G, info.row_tiles, info.col_tiles);
            if (!any) {
                ++empty;
                if (info.r0 <= info.r1 || info.v0 <= info.v1 || d.r0 != d.r1 || d.v0 != d.v1 || d.hR || d.hV)
                    return fail("no cell under test", P, G, hR, hV);
            } else {
                if (info.r0 != hR + 1 || info.r1 != G - hR || info.v0 != hV + 1 || info.v1 != P - hV || info.hR != hR || info.hV != hV)
                    return fail("cells under test", P, G, hR, hV);
                if (d.r0 != hR || d.r1 != G - hR || d.v0 != hV || d.v1 != P - hV || d.hR != hR || d.hV != hV)
                    return fail("descriptor", P, G, hR, hV);
            }
            if (xc_lds_bytes(d.hR, d.hV, 8) + 512 * 20 + 8 > RSP_LDS_BYTES) return fail("LDS", d.hR, d.hV);
        }
    }
    if (rsp_xcfar_describe(16, 64, nullptr, nullptr) != RSP_ERR_INVALID) return fail("null params");
    const rsp_cfar_params ref{5, 10, 5, 10, 8.0};
    if (rsp_xcfar_describe(332, 3404, &ref, nullptr) != RSP_OK) return fail("null info");
    std::printf("%lld cases, %lld accepted, %lld without a cell under test\n", cases, accepted, empty);
    return accepted > 1000 && empty > 1000 ? 0 : fail("grid too small", cases, accepted, empty);
}
