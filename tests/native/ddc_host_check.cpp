// Stand-alone check of the digital down-converter's host code for the AddressSanitizer / UBSan build of
// tests/test_ddc_host.py: plain C++, no device.
//
// rsp_ddc_describe / rsp_ddc_derive in either precision over pulse counts 1 .. 333 and INT_MAX, line lengths 1 ..
// 2^30, channel counts, tap counts 0 .. 513, decimations 0 .. 65 and every edge phase, products that overflow 32
// bits and the 2 GB edge from both sides:
//   * a refusal exactly when include/rsp.h says so, with the status it names and a message;
//   * No = ceil((N - off) / D); TP the least power of two >= min(P, 64); the tile TK = k lanes x k_per_thread, the
//     lanes a power of two with TP x lanes <= 256; in_rows = (TK - 1) D + tap_chunk, 1 <= tap_chunk <= L; the LDS
//     of a workgroup within the budget of 40 KiB and its three arrays inside it; the grid covers every output.
// rsp_ddc_phase_word: exact ratios, a negative carrier, the refusals.
// Exit status 0: all held; 1 with a message otherwise.  Sanitizer reports fail the run by themselves.
#include <climits>
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>

#include "rsp_geometry.h"   // rsp.h

static int fail(const char* what, long long a = 0, long long b = 0, long long c = 0, long long d = 0) {
    std::printf("FAILED: %s (%lld, %lld, %lld, %lld)\n", what, a, b, c, d);
    return 1;
}

int main() {
    const long long Ps[] = {INT_MIN, 0, 1, 2, 3, 5, 63, 64, 65, 130, 332, 333, 1 << 14, INT_MAX};
    const long long Ns[] = {-1, 0, 1, 2, 11, 12, 13, 1000, 23276, 50000, 1 << 14, 1 << 20, 1 << 30, INT_MAX};
    const long long Cs[] = {0, 1, 3, 16, 1 << 10, INT_MAX};
    const long long Ls[] = {-1, 0, 1, 2, 12, 16, 17, 64, 100, 511, 512, 513, INT_MAX};
    const long long Ds[] = {-1, 0, 1, 2, 4, 7, 63, 64, 65};
    const int precs[] = {RSP_C128, RSP_C64, 0, 7};
    long long cases = 0, accepted = 0;
    for (int prec : precs) {
        const long long rs = prec == RSP_C128 ? 8 : 4, lim = 1ll << 31;
        for (long long P : Ps) for (long long N : Ns) for (long long C : Cs) for (long long L : Ls) for (long long D : Ds) {
            const long long offs[] = {-1, 0, D / 2, D - 1, D};
            for (long long off : offs) {
                ++cases;
                rsp_ddc_info info;
                const int rc = rsp_ddc_describe((int)P, (int)N, (int)C, (int)L, (int)D, (int)off, prec, &info);
                const std::string msg = rsp_last_error();
                DdcDesc d;
                if (rsp_ddc_derive(P, N, C, L, D, off, prec, &d) != rc) return fail("describe and derive disagree", P, N, C, rc);
                int want = RSP_OK;
                const bool sizes_ok = P >= 1 && N >= 1 && C >= 1 && L >= 1 && L <= 512 && D >= 1 && D <= 64 && off >= 0 && off < D;
                if ((prec != RSP_C128 && prec != RSP_C64) || !sizes_ok) want = RSP_ERR_INVALID;
                else {
                    const __int128 in = (__int128)P * N * C * rs, no = off < N ? (N - off + D - 1) / D : 0;
                    if (in >= lim || (__int128)P * no * C * 2 * rs >= lim) want = RSP_ERR_UNSUPPORTED;
                }
                if (rc != want) return fail("status", P, N, C * 1000 + L, rc * 100 + want);
                if (rc != RSP_OK) {
                    if (msg.empty()) return fail("no message", P, N, C, rc);
                    continue;
                }
                ++accepted;
                const long long No = off < N ? (N - off + D - 1) / D : 0;
                long long TP = 1;
                while (TP < 64 && TP < P) TP *= 2;
                if (info.No != No || info.TP != TP || d.TP != TP || (1 << d.lgTP) != TP) return fail("No / TP", P, N, info.No, info.TP);
                if (info.P != P || info.N != N || info.C != C || info.L != L || info.D != D || info.off != off) return fail("echo", P, N, C);
                if (d.KL < 1 || (d.KL & (d.KL - 1)) || d.KL * TP > RSP_DDC_THREADS || d.KPT < 1 || d.KPT > RSP_DDC_MAX_KPT ||
                    d.TK != d.KL * d.KPT || info.TK != d.TK || info.k_per_thread != d.KPT)
                    return fail("tile", P, L, D, d.TK);
                if (d.LC < 1 || d.LC > L || info.tap_chunk != d.LC || d.rows != (d.TK - 1) * D + d.LC || info.in_rows != d.rows)
                    return fail("rows", P, L, D, d.rows);
                if (d.threads != std::max<long long>(64, TP * d.KL) || info.threads != d.threads || d.threads > RSP_DDC_THREADS)
                    return fail("threads", P, L, D, d.threads);
                // the three LDS arrays: NCO values | rows | taps
                if (d.ms_bytes % 16 || d.ms_bytes < (unsigned)(d.rows * 2 * rs) ||
                    d.lds_bytes != d.ms_bytes + (unsigned)(d.rows * TP * rs + L * rs) || d.lds_bytes > RSP_DDC_LDS_BUDGET ||
                    info.lds_bytes != (int)d.lds_bytes)
                    return fail("LDS", P, L, D, d.lds_bytes);
                if (info.k_tiles != (No + d.TK - 1) / d.TK || info.p_tiles != (P + TP - 1) / TP ||
                    info.workgroups != (long long)info.k_tiles * info.p_tiles * C || (long long)info.k_tiles * d.TK < No)
                    return fail("grid", P, N, info.k_tiles, info.p_tiles);
                if (info.in_bytes != P * N * C * rs || info.out_bytes != P * No * C * 2 * rs || d.in_bytes != info.in_bytes ||
                    d.out_bytes != info.out_bytes || info.in_bytes >= lim || info.out_bytes >= lim)
                    return fail("bytes", P, N, C);
            }
        }
    }
    if (rsp_ddc_describe(4, 8, 1, 12, 4, 0, RSP_C128, nullptr) != RSP_OK) return fail("info may be NULL");

    // the phase word
    uint64_t w = 1;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    if (rsp_ddc_phase_word(10e6, 100e6, &w) != RSP_OK || w != 1844674407370955162ull) return fail("1/10", (long long)w);
    if (rsp_ddc_phase_word(25e6, 100e6, &w) != RSP_OK || w != 1ull << 62) return fail("1/4");
    if (rsp_ddc_phase_word(50e6, 100e6, &w) != RSP_OK || w != 1ull << 63) return fail("1/2");
    if (rsp_ddc_phase_word(-25e6, 100e6, &w) != RSP_OK || w != 3ull << 62) return fail("-1/4");
    if (rsp_ddc_phase_word(0.0, 1.0, &w) != RSP_OK || w != 0) return fail("0");
    if (rsp_ddc_phase_word(100e6, 100e6, &w) != RSP_OK || w != 0) return fail("1 turn");
    if (rsp_ddc_phase_word(1e300, 1e-300, &w) != RSP_OK || w != 0) return fail("a huge ratio is whole turns");
    if (rsp_ddc_phase_word(std::nextafter(1.0, 0.0), 1.0, &w) != RSP_OK) return fail("just below a turn");
    const double bad[][2] = {{nan, 1.0}, {1.0, nan}, {inf, 1.0}, {1.0, inf}, {1.0, 0.0}, {1.0, -1.0}};
    for (const auto& b : bad)
        if (rsp_ddc_phase_word(b[0], b[1], &w) != RSP_ERR_INVALID || rsp_last_error()[0] == 0) return fail("phase word refusal");
    if (rsp_ddc_phase_word(1.0, 2.0, nullptr) != RSP_ERR_INVALID) return fail("null word");
    std::printf("%lld cases, %lld accepted\n", cases, accepted);
    return accepted > 1000 ? 0 : fail("grid too small", cases, accepted);
}
