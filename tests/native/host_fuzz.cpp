// Host-only driver of librsp's plain-C++ parts (rsp_mat.cpp, rsp_host.cpp, rsp_geometry.cpp,
// rsp_music_geometry.cpp, rsp_frame_host.cpp) for the AddressSanitizer / UBSan build of
// tests/test_host_asan.py.  Status codes are ignored, except by the frame mode and the geometry
// mode's K2 layout, which check what they compute: elsewhere only memory errors (reported by the sanitizers, exit code != 0) fail the test.
//   host_fuzz mat FILE...     every MAT entry point on every file
//   host_fuzz cluster SEED    S10/S11 and inter-frame clustering on random lists
//   host_fuzz geometry SEED   rsp_plan_describe and rsp_plan_describe_k2 on random plan arguments, most of them valid
//   host_fuzz music SEED      the MUSIC host module on random line and planar plans, most of them valid
//   host_fuzz frame SEED      the frame chain's host module: layouts, capped copies, rows, hit order, regating
//   host_fuzz music-route line|planar c128|c64 N M S peaks|spectrum|eigs
//                             prints the route of one call (planar: nx = N, ny = 1, an S x 3 grid)
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "rsp.h"
#include "rsp_frame_host.h"
#include "rsp_music_geometry.h"

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
        const int ncu = ri(0, 1) ? 256 : 0;
        const int rc = rsp_plan_describe(&cfg, &cf, &cl, &pre, &opt, ncu, &sz, &rt);
        n_ok += rc == RSP_OK;
        // the K2 layout of the same arguments: the same verdict, and segments that tile the gates
        rsp_k2_layout k2;
        const int rc2 = rsp_plan_describe_k2(&cfg, &cf, &cl, &pre, &opt, ncu, &k2);
        if (rc2 != rc || rsp_plan_describe_k2(&cfg, &cf, &cl, &pre, &opt, ncu, nullptr) != rc) {
            fprintf(stderr, "geometry seed %u set %d: rsp_plan_describe %d, rsp_plan_describe_k2 %d\n", seed, rep, rc, rc2);
            return 1;
        }
        if (rc2 == RSP_OK) {
            const int gates[3] = {g1, g2, g3};
            int nseg = 0, njobs = 0, at = 0;
            bool ok = (k2.wg_per_cu == 4) == (k2.k2_pts == 2560) && (k2.wg_per_cu == 2) == (k2.k2_pts == 4096);
            for (int q = 0; q < 3; ++q) {
                const rsp_k2_segment& sg = k2.seg[q];
                ok = ok && (sg.present != 0) == (gates[q] > 0);
                if (!sg.present) continue;
                ++nseg;
                njobs += sg.type ? sg.nblocks : 1;
                ok = ok && sg.type == (q > 0) && sg.ga == at && sg.gb == at + gates[q] && sg.rows_per_wg >= 1;
                if (sg.type) ok = ok && sg.V == sg.M - sg.Lh + 1 && sg.V >= 1 && (sg.nblocks - 1) * sg.V < gates[q] && sg.nblocks * sg.V >= gates[q];
                at = sg.gb;
            }
            if (!ok || nseg != k2.nseg || njobs != k2.njobs || at != G) {
                fprintf(stderr, "geometry seed %u set %d: inconsistent K2 layout\n", seed, rep);
                return 1;
            }
        }
    }
    printf("geometry seed %u: %d of %d parameter sets accepted\n", seed, n_ok, n_sets);
    rsp_plan_describe(nullptr, nullptr, nullptr, nullptr, nullptr, 256, nullptr, nullptr);
    rsp_plan_describe_k2(nullptr, nullptr, nullptr, nullptr, nullptr, 256, nullptr);
    return 0;
}

// One MUSIC configuration of either kind; every array exactly as long as rsp.h says it is read.
struct MusicCase {
    bool planar = false;
    int N = 8, nx = 4, ny = 2, K = 16, M = 2, S = 67, nt = 9, np = 11, batch = 4, prec = RSP_C128;
    bool null_grid = false;
};

static int music_describe_case(const MusicCase& c, const std::vector<double>& g1, const std::vector<double>& g2,
                               rsp_music_config* lc, rsp_music2d_config* pc, MusicDesc* d) {
    if (c.planar) {
        *pc = rsp_music2d_config{c.nx, c.ny, c.K, c.M, c.np, c.nt, 0.5, 0.4, g1.data(), c.null_grid ? nullptr : g2.data(),
                                 c.batch, c.prec};
        return music_describe(pc, d);
    }
    *lc = rsp_music_config{c.N, c.K, c.M, c.S, 0.5, c.null_grid ? nullptr : g1.data(), c.batch, c.prec};
    return music_describe(lc, d);
}

// Everything the device-free module does for one accepted plan
static void music_exercise(std::mt19937_64& g, const MusicDesc& d, const rsp_music_config* lc, const rsp_music2d_config* pc) {
    auto ri = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(g); };
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    size_t bytes[MB_COUNT];
    music_buffer_bytes(d, bytes);
    const std::vector<double> tab = d.planar ? music_table(d, pc) : music_table(d, lc);
    std::vector<unsigned char> stage;
    music_in_precision(d, tab.data(), RSP_C128, tab.size(), stage);
    if (tab.size() * (d.xsz() / 2) != bytes[d.planar ? MB_EXY : MB_S1T]) abort();   // the table fills its buffer exactly
    for (int want = MU_WANT_PEAKS; want <= MU_WANT_EIGS; ++want) {
        const MusicRoute r = music_route(d, want);
        if (r.lds > RSP_LDS_BYTES || r.neig < 1 || r.neig > d.N) abort();
    }
    int want = 0;
    music_want_of_form(ri(-1, 3), &want);
    // scenes of both kinds on this plan (one of them is refused), n_src 0 and 9 among them
    rsp_music_scene ls = {ri(0, 9), ri(0, 1), ri(0, 1), 0, 10.0 * u(g), {}, {}};
    rsp_music2d_scene ps = {ri(0, 9), 1, ri(0, 1), 0, 10.0 * u(g), {}, {}, {}};
    for (int m = 0; m < 8; ++m) {
        ls.angles_rad[m] = ps.azim_rad[m] = 1.5 * u(g);
        ps.elev_rad[m] = 1.5 * u(g);
        ls.amplitudes[m] = ps.amplitudes[m] = 1.0 + 0.5 * u(g);
    }
    MusicSynth sy;
    music_scene(d, &ls, ri(0, 3), &sy);
    music_scene(d, &ps, ri(0, 3), &sy);
    // results: device-shaped random buffers into exactly sized outputs, every combination of nulls
    const int n_inst = ri(1, d.max_batch);
    std::vector<double> spec((size_t)n_inst * d.S), eig((size_t)n_inst * d.N), cov((size_t)2 * n_inst * d.N * d.N);
    std::vector<int32_t> pidx((size_t)n_inst * d.M), npk(n_inst);
    for (int mask = 0; mask < 32; ++mask) {
        rsp_music_out out = {mask & 1 ? spec.data() : nullptr, mask & 2 ? eig.data() : nullptr, mask & 4 ? pidx.data() : nullptr,
                             mask & 8 ? npk.data() : nullptr, mask & 16 ? cov.data() : nullptr};
        if (music_want(&out) != (mask & 2 ? MU_WANT_EIGS : mask & 1 ? MU_WANT_SPECTRUM : MU_WANT_PEAKS)) abort();
        MusicFetch f;
        music_fetch_plan(d, n_inst, &out, &f);
        for (int c = 0; c < f.n; ++c) {
            if (f.copy[c].bytes > bytes[f.copy[c].buf]) abort();   // never more than the device buffer holds
            unsigned char* dst = (unsigned char*)f.copy[c].dst;
            for (size_t b = 0; b < f.copy[c].bytes; ++b) dst[b] = (unsigned char)g();
        }
        music_unpack(d, n_inst, f, &out);
        if (!f.stage[2].empty()) music_fast_count((const int*)f.stage[2].data(), n_inst);
    }
    music_want(nullptr);
    // host snapshots of either type into the plan's precision
    const size_t reals = (size_t)2 * n_inst * d.K * d.N;
    std::vector<double> xd(reals);
    std::vector<float> xf(reals);
    for (size_t i = 0; i < reals; ++i) xf[i] = (float)(xd[i] = u(g));
    music_in_precision(d, xd.data(), RSP_C128, reals, stage);
    music_in_precision(d, xf.data(), RSP_C64, reals, stage);
}

static int music(unsigned seed) {
    std::mt19937_64 g(seed);
    auto ri = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(g); };
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    // the envelope's corners, accepted, first: N = 2 and 64, M = N - 1 and 8, S = 3 and 4096, a 1024 x 64 grid
    std::vector<MusicCase> cases(8);
    cases[0].N = 2; cases[0].M = 1;
    cases[1].N = 64; cases[1].M = 8; cases[1].S = 4096;
    cases[2].N = 5; cases[2].M = 4; cases[2].S = 3; cases[2].prec = RSP_C64;
    cases[3].N = 64; cases[3].M = 7; cases[3].S = 4095; cases[3].prec = RSP_C64;
    cases[4].planar = true; cases[4].nx = 2; cases[4].ny = 1; cases[4].M = 1; cases[4].nt = 1024; cases[4].np = 64;
    cases[5].planar = true; cases[5].nx = 8; cases[5].ny = 8; cases[5].M = 8; cases[5].nt = 3; cases[5].np = 3;
    cases[6].planar = true; cases[6].nx = 1; cases[6].ny = 64; cases[6].M = 7; cases[6].nt = 64; cases[6].np = 1024;
    cases[7].planar = true; cases[7].nx = 3; cases[7].ny = 1; cases[7].M = 2;
    const int n_forced = (int)cases.size();
    for (int rep = 0; rep < 300; ++rep) {
        MusicCase c;
        c.planar = rep < 32 ? rep >= 16 : ri(0, 1);   // every refusal below at least once for either kind
        c.nx = ri(1, 8); c.ny = ri(c.nx == 1 ? 2 : 1, 8);
        c.N = c.planar ? c.nx * c.ny : ri(0, 3) ? ri(2, 20) : ri(2, 64);
        c.M = ri(1, std::min(8, c.N - 1));
        c.K = ri(1, 40);
        c.S = ri(0, 7) ? ri(3, 300) : ri(3, 4096);
        c.nt = ri(3, 40); c.np = ri(3, 40);
        c.batch = ri(1, 4);
        c.prec = c.planar || ri(0, 1) ? RSP_C128 : RSP_C64;
        switch (rep < 32 ? rep % 16 : ri(0, 63)) {   // deliberately out of range (one in four of the random ones)
            case 0: c.N = 1; c.nx = c.ny = 1; break;
            case 1: c.N = 65; c.nx = 5; c.ny = 13; break;           // nx*ny = 65
            case 2: c.M = 0; break;
            case 3: c.M = c.N; break;
            case 4: c.M = 9; c.N = 16; c.nx = c.ny = 4; break;
            case 5: c.K = 0; break;
            case 6: c.S = 2; c.nt = 2; break;
            case 7: c.S = 4097; c.np = 1025; c.nt = 3; break;       // grid 1025 x 3
            case 8: c.nt = 1024; c.np = 65; break;                  // grid 1024 x 65
            case 9: c.null_grid = true; break;
            case 10: c.prec = 7; break;
            case 11: c.prec = RSP_C64; c.planar = true; break;      // C64 planar
            case 12: c.batch = 0; break;
            case 13: c.nx = 65; c.ny = 1; c.N = 65; break;
            case 14: c.nx = 0; c.N = 0; break;
            case 15: c.nt = 1025; c.np = 3; break;
            default: break;
        }
        cases.push_back(c);
    }
    int n_ok = 0;
    for (size_t i = 0; i < cases.size(); ++i) {
        const MusicCase& c = cases[i];
        // grids of exactly the lengths the tables read
        std::vector<double> g1(std::max(1, c.planar ? c.np : c.S)), g2(std::max(1, c.nt));
        for (auto& v : g1) v = 1.6 * u(g);
        for (auto& v : g2) v = 1.6 * u(g);
        rsp_music_config lc;
        rsp_music2d_config pc;
        MusicDesc d;
        const int rc = music_describe_case(c, g1, g2, &lc, &pc, &d);
        if (rc != RSP_OK && (int)i < n_forced) abort();   // the corners are inside the envelope
        if (rc != RSP_OK) continue;
        ++n_ok;
        music_exercise(g, d, &lc, &pc);
    }
    printf("music seed %u: %d of %d configurations accepted\n", seed, n_ok, (int)cases.size());
    music_describe((const rsp_music_config*)nullptr, nullptr);
    music_describe((const rsp_music2d_config*)nullptr, nullptr);
    return 0;
}

// ---- frame: the frame chain's host module (rsp_frame_host.h), results checked ----
#define FRAME_CHECK(cond, ...)                      \
    do {                                            \
        if (!(cond)) {                              \
            fprintf(stderr, "frame: " __VA_ARGS__); \
            fprintf(stderr, " [%s]\n", #cond);      \
            exit(1);                                \
        }                                           \
    } while (0)

template <class T>
static T frame_rnd(std::mt19937_64& g) {
    if constexpr (std::is_same<T, uint8_t>::value) return (uint8_t)(g() & 0xFF);
    else if constexpr (std::is_floating_point<T>::value) return (T)std::uniform_real_distribution<double>(-1.0, 1.0)(g);
    else return T(frame_rnd<typename T::value_type>(g), frame_rnd<typename T::value_type>(g));
}

// device [n][P][G] of S -> MATLAB [P x G x n] of D, buffers exactly as long as the layout says
template <class S, class D>
static void frame_to_matlab(std::mt19937_64& g, int P, int G, int n) {
    std::vector<S> in((size_t)n * P * G);
    for (auto& v : in) v = frame_rnd<S>(g);
    std::vector<D> out(in.size());
    rsp_transpose_planes(in.data(), P, G, n, out.data());
    for (int b = 0; b < n; ++b)
        for (int v = 0; v < P; ++v)
            for (int r = 0; r < G; ++r)
                FRAME_CHECK(out[v + (size_t)P * (r + (size_t)G * b)] == static_cast<D>(in[((size_t)b * P + v) * G + r]),
                            "to MATLAB, P %d G %d n %d at (%d, %d, %d)", P, G, n, v, r, b);
}

// MATLAB [P x G x n] doubles -> device [n][P][G] of D (narrowed: a (float) cast); in double, and back: the identity
template <class D>
static void frame_from_matlab(std::mt19937_64& g, int P, int G, int n) {
    std::vector<double> in((size_t)n * P * G), back(in.size());
    for (auto& v : in) v = frame_rnd<double>(g);
    std::vector<D> out(in.size());
    rsp_transpose_planes(in.data(), G, P, n, out.data());
    for (int b = 0; b < n; ++b)
        for (int v = 0; v < P; ++v)
            for (int r = 0; r < G; ++r)
                FRAME_CHECK(out[((size_t)b * P + v) * G + r] == (D)in[v + (size_t)P * (r + (size_t)G * b)],
                            "from MATLAB, P %d G %d n %d at (%d, %d, %d)", P, G, n, v, r, b);
    if (std::is_same<D, double>::value) {
        rsp_transpose_planes(out.data(), P, G, n, back.data());
        FRAME_CHECK(back == in, "there and back, P %d G %d n %d", P, G, n);
    }
}

static void frame_layouts(std::mt19937_64& g, int P, int G, int n) {
    typedef std::complex<float> cf;
    typedef std::complex<double> cd;
    frame_to_matlab<cf, cd>(g, P, G, n);
    frame_to_matlab<cd, cd>(g, P, G, n);
    frame_to_matlab<float, double>(g, P, G, n);
    frame_to_matlab<double, double>(g, P, G, n);
    frame_to_matlab<uint8_t, uint8_t>(g, P, G, n);
    frame_from_matlab<float>(g, P, G, n);
    frame_from_matlab<double>(g, P, G, n);
    // the cube conversion: 2 scalars per element, widened and narrowed
    std::vector<double> d((size_t)2 * P * G * n), wide(d.size());
    std::vector<float> f(d.size());
    for (auto& v : d) v = frame_rnd<double>(g);
    rsp_convert_reals(d.data(), RSP_C128, d.size(), f.data());
    rsp_convert_reals(f.data(), RSP_C64, f.size(), wide.data());
    for (size_t i = 0; i < d.size(); ++i) FRAME_CHECK(f[i] == (float)d[i] && wide[i] == f[i], "precision conversion at %zu", i);
}

static bool frame_same_target(const rsp_target& a, const rsp_target& b) { return !memcmp(&a, &b, sizeof a); }

// n records into caps of 0, n - 1, n and n + 1 with a guard record behind each, and a size query
static void frame_capped_copy(std::mt19937_64& g, int n) {
    std::vector<rsp_target> src(n);
    for (auto& t : src) t = rsp_target{frame_rnd<double>(g), frame_rnd<double>(g), frame_rnd<double>(g), frame_rnd<double>(g)};
    const rsp_target guard = {-1.0, -2.0, -3.0, -4.0};
    for (int cap : {0, n - 1, n, n + 1}) {
        if (cap < 0) continue;
        std::vector<rsp_target> dst((size_t)cap + 1, guard);
        int32_t got = -7;
        const int rc = rsp_capped_copy(dst.data(), src.data(), n, cap, &got, "%d targets > cap %d", n, cap);
        FRAME_CHECK(got == n, "capped copy: n_out %d of %d, cap %d", got, n, cap);
        FRAME_CHECK(rc == (n > cap ? RSP_ERR_OVERFLOW : RSP_OK), "capped copy: status %d, n %d cap %d", rc, n, cap);
        char want[64];
        snprintf(want, sizeof want, "%d targets > cap %d", n, cap);
        FRAME_CHECK(n <= cap || !strcmp(rsp_last_error(), want), "capped copy: message '%s'", rsp_last_error());
        for (int i = 0; i < std::min(n, cap); ++i) FRAME_CHECK(frame_same_target(dst[i], src[i]), "capped copy: record %d", i);
        for (int i = std::min(n, cap); i <= cap; ++i) FRAME_CHECK(frame_same_target(dst[i], guard), "capped copy: wrote record %d, n %d cap %d", i, n, cap);
    }
    int64_t got = -7;
    FRAME_CHECK(rsp_capped_copy((rsp_target*)nullptr, src.data(), n, 0, &got, "cap too small") == RSP_OK && got == n, "size query");
    FRAME_CHECK(rsp_capped_copy((rsp_target*)nullptr, src.data(), n, 0, (int32_t*)nullptr, "cap too small") == RSP_OK, "no count");
}

// queued frames with 0, 1 and several targets as rsp_results_rows packs them
static void frame_rows(std::mt19937_64& g) {
    auto ri = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(g); };
    const int nf = ri(3, 8);
    std::vector<std::vector<rsp_target>> fr(nf);
    std::vector<int> ids(nf);
    std::vector<double> want;   // built from the description: 5 doubles per row
    for (int f = 0; f < nf; ++f) {
        ids[f] = ri(-3, 1000);
        fr[f].resize(f == 0 ? 0 : f == 1 ? 1 : f == 2 ? 4 : ri(0, 5));
        for (auto& t : fr[f]) t = rsp_target{frame_rnd<double>(g), frame_rnd<double>(g), frame_rnd<double>(g), frame_rnd<double>(g)};
        for (const auto& t : fr[f]) want.insert(want.end(), {(double)ids[f], t.Range, t.Velocity, t.Angle, t.Power});
        if (fr[f].empty()) want.insert(want.end(), {(double)ids[f], NAN, NAN, NAN, NAN});
    }
    const int64_t total = (int64_t)want.size() / 5;
    auto pack = [&](double* rows, int64_t cap) {
        int64_t n = 0;
        for (int f = 0; f < nf; ++f) rsp_result_rows(ids[f], fr[f].data(), fr[f].size(), rows, cap, &n);
        return n;
    };
    FRAME_CHECK(pack(nullptr, 0) == total, "rows: size query");
    for (int64_t cap : {total, total - 1, (int64_t)0}) {
        std::vector<double> rows((size_t)5 * (cap + 1), -5.0);   // one guard row behind cap
        FRAME_CHECK(pack(rows.data(), cap) == total, "rows: count at cap %lld", (long long)cap);
        for (int64_t i = 0; i < 5 * (cap + 1); ++i) {
            const double w = i < 5 * cap ? want[i] : -5.0;
            FRAME_CHECK(std::isnan(w) ? std::isnan(rows[i]) : rows[i] == w, "rows: value %lld at cap %lld", (long long)i, (long long)cap);
        }
    }
}

static void frame_hits(std::mt19937_64& g) {
    auto ri = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(g); };
    const int B = ri(1, 4), G = ri(1, 12), P = ri(1, 9);
    std::vector<rsp_stage3_hit> want;   // beam, then r, then v
    for (int b = 1; b <= B; ++b)
        for (int r = 1; r <= G; ++r)
            for (int v = 1; v <= P; ++v)
                if (ri(0, 2)) want.push_back(rsp_stage3_hit{v, r, b, 0, frame_rnd<double>(g), frame_rnd<double>(g)});
    const int64_t n = (int64_t)want.size();
    for (int64_t cap : {n, n - 1, n + 1, (int64_t)1}) {
        if (cap < 1) continue;
        std::vector<rsp_stage3_hit> h = want, out((size_t)cap + 1, rsp_stage3_hit{-1, -1, -1, -1, 0.0, 0.0});
        std::shuffle(h.begin(), h.end(), g);
        rsp_s3_sorted_hits(h.data(), n, out.data(), cap);
        for (int64_t i = 0; i <= cap; ++i) {
            const rsp_stage3_hit w = i < std::min(n, cap) ? want[i] : rsp_stage3_hit{-1, -1, -1, -1, 0.0, 0.0};
            FRAME_CHECK(!memcmp(&out[i], &w, sizeof w), "hit order: record %lld of %lld, cap %lld", (long long)i, (long long)n, (long long)cap);
        }
    }
}

// One rsp_stage2_regate call on a gated input of exactly the size the columns say; status and
// message against `msg` (null: accepted, and every byte of the result is checked)
static void frame_regate_case(std::mt19937_64& g, int P, int N, int B, int dtype, int n_gated, const int32_t* cols, int want_rc,
                              const char* msg) {
    const size_t es = dtype == RSP_C64 ? 8 : 16, colb = (size_t)P * es;
    std::vector<unsigned char> iq(std::max<size_t>((size_t)std::max(n_gated, 0) * B * colb, 1)), full;
    for (auto& v : iq) v = (unsigned char)(1 + g() % 255);   // no zero byte: a gated column is told from the fill
    const int rc = rsp_stage2_regate(P, N, B, iq.data(), dtype, n_gated, cols, full);
    FRAME_CHECK(rc == want_rc, "regate: status %d, expected %d (%s)", rc, want_rc, msg ? msg : "accepted");
    if (msg) {
        FRAME_CHECK(!strcmp(rsp_last_error(), msg), "regate: message '%s', expected '%s'", rsp_last_error(), msg);
        return;
    }
    static const int32_t ref[6] = {83, 310, 311, 1033, 1034, 3486};
    const int32_t* c = cols ? cols : ref;
    FRAME_CHECK(full.size() == (size_t)N * B * colb, "regate: %zu bytes", full.size());
    for (int b = 0; b < B; ++b) {
        std::vector<int> from(N, -1);   // PRT column -> gated column
        int ng = 0;
        for (int k = 0; k < 3; ++k)
            for (int col = c[2 * k]; col <= c[2 * k + 1]; ++col) from[col - 1] = ng++;
        for (int col = 0; col < N; ++col)
            for (size_t i = 0; i < colb; ++i) {
                const unsigned char w = from[col] < 0 ? 0 : iq[((size_t)b * n_gated + from[col]) * colb + i];
                FRAME_CHECK(full[((size_t)b * N + col) * colb + i] == w, "regate: beam %d column %d byte %zu", b, col, i);
            }
    }
}

static void frame_regate(std::mt19937_64& g) {
    auto ri = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(g); };
    frame_regate_case(g, 2, 3486, 2, RSP_C64, 3404, nullptr, RSP_OK, nullptr);   // the reference's columns
    frame_regate_case(g, 1, 3486, 1, RSP_C128, 3404, nullptr, RSP_OK, nullptr);
    const int32_t ok[6] = {2, 4, 6, 6, 9, 12};   // 3 + 1 + 4 columns
    frame_regate_case(g, 3, 12, 2, 7, 8, ok, RSP_ERR_INVALID, "unknown dtype 7");
    const int32_t low[6] = {0, 4, 6, 6, 9, 12};
    frame_regate_case(g, 3, 12, 2, RSP_C64, 9, low, RSP_ERR_INVALID, "gate columns 0..4 of segment 0 outside the 12-sample PRT");
    frame_regate_case(g, 3, 11, 2, RSP_C64, 8, ok, RSP_ERR_INVALID, "gate columns 9..12 of segment 2 outside the 11-sample PRT");
    const int32_t over[6] = {2, 6, 6, 6, 9, 12};
    frame_regate_case(g, 3, 12, 2, RSP_C128, 10, over, RSP_ERR_INVALID,
                      "gate columns of segment 1 (6..6) overlap or precede segment 0 (..6)");
    frame_regate_case(g, 3, 12, 2, RSP_C128, 9, ok, RSP_ERR_INVALID, "gated input has 9 columns, the gate columns cover 8");
    for (int rep = 0; rep < 40; ++rep) {   // accepted: three ascending, disjoint segments inside a small PRT
        const int P = ri(1, 5), B = ri(1, 3), N = ri(3, 30);
        int cut[6];
        for (int& v : cut) v = ri(1, N);
        std::sort(cut, cut + 6);
        if (cut[2] == cut[1] || cut[4] == cut[3]) continue;   // segments would share a column
        const int32_t c[6] = {cut[0], cut[1], cut[2], cut[3], cut[4], cut[5]};
        const int n_gated = (c[1] - c[0] + 1) + (c[3] - c[2] + 1) + (c[5] - c[4] + 1);
        frame_regate_case(g, P, N, B, ri(0, 1) ? RSP_C64 : RSP_C128, n_gated, c, RSP_OK, nullptr);
    }
}

static int frame(unsigned seed) {
    std::mt19937_64 g(seed);
    auto ri = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(g); };
    const int corners[][3] = {{1, 1, 1}, {1, 70, 5}, {40, 1, 1}, {40, 70, 5}, {1, 1, 5}, {7, 1, 2}, {1, 9, 1}};
    for (const auto& c : corners) frame_layouts(g, c[0], c[1], c[2]);
    for (int rep = 0; rep < 300; ++rep) frame_layouts(g, ri(1, 40), ri(1, 70), ri(1, 5));
    for (int n = 0; n <= 6; ++n) frame_capped_copy(g, n);
    for (int rep = 0; rep < 50; ++rep) {
        frame_rows(g);
        frame_hits(g);
    }
    frame_regate(g);
    // the refusals of the stage-3 map count, and the synthesis constants and byte counts on exact-size arrays
    FRAME_CHECK(rsp_s3_check_cells(12, 20, 0) == RSP_ERR_INVALID && rsp_s3_check_cells(12, 20, 65536) == RSP_ERR_INVALID &&
                    rsp_s3_check_cells(32768, 32768, 2) == RSP_ERR_INVALID && rsp_s3_check_cells(12, 20, 13) == RSP_OK, "cell check");
    std::vector<rsp_target_in> tin(RSP_MAX_SYNTH_TARGETS, rsp_target_in{3000.0, 12.5, -4.0, 10.0});
    SynthTargets tg;
    rsp_synth_targets(SynthConsts{3e8, 25e6, 0.1, 0.05, 2e-4, 1.0}, tin.data(), (int)tin.size(), 1.0, &tg);
    FRAME_CHECK(tg.t[RSP_MAX_SYNTH_TARGETS - 1].delay == 500 && tg.t[0].fd_prt == 2.0 * 12.5 / 0.1 * 2e-4, "synthesis constants");
    int64_t by[3];
    rsp_stage3_bytes(100, 16, by);
    FRAME_CHECK(by[0] == 100 * 17 && by[1] == 100 * 33 && by[2] == 1600, "stage-3 bytes");
    printf("frame seed %u: ok\n", seed);
    return 0;
}

static int music_route_of(char** a) {
    MusicCase c;
    c.planar = !strcmp(a[0], "planar");
    c.prec = !strcmp(a[1], "c64") ? RSP_C64 : RSP_C128;
    c.N = c.nx = atoi(a[2]); c.ny = 1;
    c.M = atoi(a[3]);
    c.S = c.nt = atoi(a[4]); c.np = 3;
    const int want = !strcmp(a[5], "eigs") ? MU_WANT_EIGS : !strcmp(a[5], "spectrum") ? MU_WANT_SPECTRUM : MU_WANT_PEAKS;
    const std::vector<double> g1(std::max(3, c.S), 0.0), g2(std::max(3, c.nt), 0.0);
    rsp_music_config lc;
    rsp_music2d_config pc;
    MusicDesc d;
    if (music_describe_case(c, g1, g2, &lc, &pc, &d) != RSP_OK) {
        printf("refused=1\n");
        return 0;
    }
    const MusicRoute r = music_route(d, want);
    static const char* cov[] = {"f64", "f32_vec4", "f32"};
    static const char* eig[] = {"k_music_eig", "k_music_eig64", "k_music_sub64"};
    printf("stages=%d cov=%s eig=%s fast=%d neig=%d spec_tol=%g lds=%zu raise_lds=%d fast_flag=%d\n", r.n_stages, cov[r.cov],
           eig[r.eig], (int)r.fast, r.neig, r.spec_tol, r.lds, (int)r.raise_lds, (int)r.fast_flag);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "mat")) return mat(argc, argv);
    if (argc >= 3 && !strcmp(argv[1], "cluster")) return cluster((unsigned)atoi(argv[2]));
    if (argc >= 3 && !strcmp(argv[1], "geometry")) return geometry((unsigned)atoi(argv[2]));
    if (argc >= 3 && !strcmp(argv[1], "music")) return music((unsigned)atoi(argv[2]));
    if (argc >= 3 && !strcmp(argv[1], "frame")) return frame((unsigned)atoi(argv[2]));
    if (argc >= 8 && !strcmp(argv[1], "music-route")) return music_route_of(argv + 2);
    fprintf(stderr, "usage: host_fuzz mat FILE... | cluster SEED | geometry SEED | music SEED | frame SEED | music-route ...\n");
    return 2;
}
