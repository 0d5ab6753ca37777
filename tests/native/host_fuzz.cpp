// Host-only driver of librsp's plain-C++ parts (rsp_mat.cpp, rsp_host.cpp, rsp_geometry.cpp) for
// the AddressSanitizer / UBSan build of tests/test_host_asan.py.  Status codes are ignored: only
// memory errors (reported by the sanitizers, exit code != 0) fail the test.
//   host_fuzz mat FILE...     every MAT entry point on every file
//   host_fuzz cluster SEED    S10/S11 and inter-frame clustering on random lists
//   host_fuzz geometry SEED   rsp_plan_describe on random plan arguments, most of them valid
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "rsp.h"

static int mat(int argc, char** argv) {
    for (int i = 2; i < argc; ++i) {
        rsp_mat_var vars[8];
        int32_t nv = 0;
        rsp_mat_list(argv[i], vars, 8, &nv);
        for (int v = 0; v < nv && v < 8; ++v) {
            std::vector<double> d(64);
            std::vector<float> f(64);
            std::vector<char> c(64);
            rsp_mat_read(argv[i], vars[v].name, RSP_MAT_OUT_F64, d.data(), (int64_t)d.size());
            rsp_mat_read(argv[i], vars[v].name, RSP_MAT_OUT_F32, f.data(), (int64_t)f.size());
            rsp_mat_read(argv[i], vars[v].name, RSP_MAT_OUT_CHAR, c.data(), (int64_t)c.size());
        }
        int32_t dims[3] = {0, 0, 0}, na = 0;
        double ang[16];
        std::vector<double> cube(2 * 4096);
        rsp_mat_load_frame(argv[i], RSP_C128, cube.data(), 4096, dims, ang, 16, &na);
        rsp_mat_load_frame(argv[i], RSP_C64, cube.data(), 4096, dims, ang, 16, &na);
        rsp_mat_load_frame(argv[i], RSP_C128, nullptr, 0, dims, nullptr, 0, &na);
    }
    return 0;
}

static int cluster(unsigned seed) {
    std::mt19937_64 g(seed);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    rsp_cluster_params cp = {30.0, 0.4, 5.0};
    for (int rep = 0; rep < 20; ++rep) {
        const int n = (int)(u(g) * 3000);
        std::vector<rsp_detection> d(n);
        for (int i = 0; i < n; ++i) {
            const int c = (int)(u(g) * 8);
            d[i] = rsp_detection{(int32_t)(16 + u(g) * 90), (int32_t)(16 + u(g) * 2000), (int32_t)(1 + u(g) * 7), 0,
                                 1 + 99 * u(g), 1000.0 * c + 50 * u(g), 5.0 + 0.5 * c + 0.3 * u(g), 3.0 * c + 3 * u(g)};
        }
        std::vector<rsp_target> out(64);
        int32_t no = 0;
        rsp_cluster_detections(d.data(), n, &cp, out.data(), (int32_t)out.size(), &no);   // may overflow cap: status only
        std::vector<rsp_track_point> pts(n);
        for (int i = 0; i < n; ++i)
            pts[i] = rsp_track_point{d[i].Range, d[i].Velocity, d[i].Angle, d[i].amp, 10 * u(g), (int32_t)(u(g) * 20), 0};
        rsp_inter_frame_params ip = {30.0, 1.0, 2.0, 3.0, 2, 0};
        std::vector<rsp_track> tr(32);
        rsp_inter_frame_cluster(pts.data(), n, &ip, tr.data(), (int32_t)tr.size(), &no);
    }
    rsp_cluster_detections(nullptr, 0, &cp, nullptr, 0, nullptr);
    int32_t no = 0;
    rsp_cluster_detections(nullptr, 0, &cp, nullptr, 0, &no);
    return 0;
}

// Spectrum (n points, interleaved re/im) of a random filter of lh taps: the matched-filter
// arguments of a plan are DFTs of short filters.  zero: the all-zero filter.
static std::vector<double> filter_spectrum(std::mt19937_64& g, int n, int lh, bool zero) {
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    std::vector<std::complex<double>> h(lh);
    for (auto& v : h) v = zero ? 0.0 : std::complex<double>(u(g), u(g));
    std::vector<double> out(2 * (size_t)n);
    for (int k = 0; k < n; ++k) {
        const std::complex<double> w = std::polar(1.0, -2.0 * M_PI * k / n);
        std::complex<double> acc = 0, wp = 1;
        for (int t = 0; t < lh; ++t, wp *= w) acc += h[t] * wp;
        out[2 * k] = acc.real();
        out[2 * k + 1] = acc.imag();
    }
    return out;
}

// Every array is exactly as long as rsp.h says the plan reads it, so an over-read is a report.
static int geometry(unsigned seed) {
    std::mt19937_64 g(seed);
    auto ri = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(g); };
    int n_ok = 0, n_sets = 0;
    for (int rep = 0; rep < 2500; ++rep, ++n_sets) {
        const int C = ri(1, 32), B = ri(1, 16);
        // even P from 2 to 1100: every route's range, the small ones and the FFT sizes more often
        const int P = ri(0, 3) == 0 ? 16 << ri(0, 5) : 2 * (ri(0, 3) ? ri(1, 130) : ri(1, 550));
        const int N = ri(0, 3) ? ri(64, 2048) : ri(64, 8192);
        // N_fft: a power of two up to N rounded up, or (one in three) not one (the plan's O(n^2) DFT: kept short)
        auto pick_nfft = [&]() {
            if (ri(0, 2) == 0) return ri(48, 400);
            int n = 64;
            while (n < N && n < 8192 && ri(0, 3)) n *= 2;
            return n;
        };
        const int nf_med = pick_nfft(), nf_long = pick_nfft();
        // gates within both N_fft (fsf:124-125 indexes the segment's IFFT with the stitched gate)
        int g1 = ri(0, 3) ? ri(1, std::min(std::min(300, N / 4), std::min(nf_med / 2, nf_long / 4))) : 0;
        int g2 = ri(0, 5) ? ri(1, std::min(nf_med - g1, nf_long / 2)) : 0;
        int g3 = ri(0, 5) ? ri(1, nf_long - g1 - g2) : 0;
        if (g1 + g2 + g3 == 0) g1 = 1;
        int G = g1 + g2 + g3;
        int ntaps = ri(1, 64);
        const int lh_med = ri(1, std::max(1, std::min(nf_med / 2, 96))), lh_long = ri(1, std::max(1, std::min(nf_long / 2, 200)));
        // 1-based segment starts; the FFT segments end at N and are short enough for N_fft to
        // hold segment + filter (no circular aliasing)
        int st_n = ri(1, N);
        int st_m = N + 1 - ri(1, std::max(1, std::min(N, nf_med - lh_med)));
        int st_l = N + 1 - ri(1, std::max(1, std::min(N, nf_long - lh_long)));
        rsp_cfar_params cf = {5, 10, 5, 10, 8.0};
        if (ri(0, 2) == 0) cf = {ri(1, 6), ri(0, 10), ri(1, 6), ri(0, 10), 8.0};
        // deliberately out of range (one set in four)
        bool zero_med = false, zero_long = false;
        switch (ri(0, 51)) {
            case 0: st_n = 0; break;
            case 1: st_m = 0; break;
            case 2: st_l = N + ri(1, 5); break;
            case 3: st_n = N + 1; break;
            case 4: G += 1; break;
            case 5: G -= 1; break;
            case 6: ntaps = 0; break;
            case 7: zero_med = true; break;
            case 8: zero_long = true; break;
            case 9: g3 += nf_long; G += nf_long; break;          // gates beyond N_fft_long
            case 10: g2 += nf_med; G += nf_med; break;           // gates beyond N_fft_med
            case 11: cf.refCells_R = 0; break;
            case 12: st_m = N; st_l = N; break;                  // one-sample segments
            default: break;
        }
        std::uniform_real_distribution<double> u(-1.0, 1.0);
        auto reals = [&](size_t n) { std::vector<double> v(n); for (auto& x : v) x = u(g); return v; };
        const std::vector<double> W = reals(2 * (size_t)B * C), taps = reals(std::max(ntaps, 1)), win = reals(P),
                                  ra = reals(std::max(G, 1)), va = reals(P), ang = reals(B), kl = reals(std::max(B - 1, 1));
        const std::vector<double> mf_med = filter_spectrum(g, nf_med, lh_med, zero_med),
                                  mf_long = filter_spectrum(g, nf_long, lh_long, zero_long);
        rsp_sig_config cfg = {3e8, 25e6, 3e9, 2e-4, 0.1, 0.05, P, N, C, B};
        rsp_cluster_params cl = {30.0, 0.4, 5.0};
        rsp_precomputed pre = {};
        pre.DBF_coeffs_data_C = W.data();
        pre.MF_narrow = taps.data(); pre.n_MF_narrow = ntaps; pre.fir_delay = ri(0, 40);
        pre.MF_medium_fft = mf_med.data(); pre.N_fft_med = nf_med;
        pre.MF_long_fft = mf_long.data(); pre.N_fft_long = nf_long;
        pre.N_gate_narrow = g1; pre.N_gate_medium = g2; pre.N_gate_long = g3; pre.N_total_gate = G;
        pre.seg_start_narrow = st_n; pre.seg_start_medium = st_m; pre.seg_start_long = st_l;
        pre.MTD_win = win.data(); pre.range_axis = ra.data(); pre.velocity_axis = va.data();
        pre.deltaR = 6.0; pre.deltaV = 0.5;
        pre.beam_angles_deg = ang.data(); pre.k_slopes_LUT = kl.data();
        rsp_plan_options opt = {0, 1, ri(0, 1) ? RSP_C128 : RSP_C64, ri(0, 3)};
        rsp_sizes sz;
        rsp_k1_route rt;
        n_ok += rsp_plan_describe(&cfg, &cf, &cl, &pre, &opt, ri(0, 1) ? 256 : 0, &sz, &rt) == RSP_OK;
    }
    printf("geometry seed %u: %d of %d parameter sets accepted\n", seed, n_ok, n_sets);
    rsp_plan_describe(nullptr, nullptr, nullptr, nullptr, nullptr, 256, nullptr, nullptr);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "mat")) return mat(argc, argv);
    if (argc >= 3 && !strcmp(argv[1], "cluster")) return cluster((unsigned)atoi(argv[2]));
    if (argc >= 3 && !strcmp(argv[1], "geometry")) return geometry((unsigned)atoi(argv[2]));
    fprintf(stderr, "usage: host_fuzz mat FILE... | cluster SEED | geometry SEED\n");
    return 2;
}
