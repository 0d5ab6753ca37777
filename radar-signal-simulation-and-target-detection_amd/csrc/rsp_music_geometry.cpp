// rsp_music_geometry.cpp -- the device-free half of a MUSIC plan (rsp_music_geometry.h): no HIP.
#include "rsp_music_geometry.h"

#include <cmath>
#include <cstring>

__attribute__((visibility("hidden"))) int rsp_set_error(int code, const char* fmt, ...);   // rsp_host.cpp

namespace {

// The refusals of both create functions, in the order each has always made them.  A planar
// description arrives with nx, ny and the grid; its N and S follow from them once they are in range.
int music_check(MusicDesc& d, int precision) {
    if (d.planar) {
        if (d.nx < 1 || d.ny < 1 || d.nx > MU_NMAX || d.ny > MU_NMAX || d.nx * d.ny < 2 || d.nx * d.ny > MU_NMAX)
            return rsp_set_error(RSP_ERR_UNSUPPORTED, "nx*ny = %d*%d outside 2..%d", d.nx, d.ny, MU_NMAX);
        d.N = d.nx * d.ny;
    } else if (d.N < 2 || d.N > MU_NMAX) {
        return rsp_set_error(RSP_ERR_UNSUPPORTED, "channel_num %d outside 2..%d", d.N, MU_NMAX);
    }
    if (d.M < 1 || d.M >= d.N || d.M > MU_MMAX)
        return rsp_set_error(RSP_ERR_UNSUPPORTED, "num_sources %d outside 1..min(%d, %s-1)", d.M, MU_MMAX,
                             d.planar ? "nx*ny" : "channel_num");
    if (d.planar) {
        const int np = d.n_phi, nt = d.n_theta;
        if (np < 3 || np > 1024 || nt < 3 || nt > 1024 || np * nt > M2_SMAX)
            return rsp_set_error(RSP_ERR_UNSUPPORTED, "grid n_phi %d x n_theta %d: each 3..1024, at most %d points", np,
                                 nt, M2_SMAX);
        d.S = nt * np;
        if (precision == RSP_C64)
            return rsp_set_error(RSP_ERR_UNSUPPORTED, "2-D MUSIC is complex double only (precision RSP_C128)");
        if (precision != RSP_C128) return rsp_set_error(RSP_ERR_INVALID, "precision must be RSP_C128, got %d", precision);
    }
    if (d.K < 1) return rsp_set_error(RSP_ERR_INVALID, "num_snapshots %d < 1", d.K);
    if (!d.planar && (d.S < 3 || d.S > MU_SCAN_MAX))
        return rsp_set_error(RSP_ERR_UNSUPPORTED, "n_scan %d outside 3..%d", d.S, MU_SCAN_MAX);
    if (d.max_batch < 1) return rsp_set_error(RSP_ERR_INVALID, "max_batch %d < 1", d.max_batch);
    if (!d.planar && precision != RSP_C128 && precision != RSP_C64)
        return rsp_set_error(RSP_ERR_INVALID, "precision must be RSP_C128 or RSP_C64, got %d", precision);
    d.f64 = precision == RSP_C128;
    d.Spad = d.planar ? 0 : (d.S + 7) & ~3;
    return RSP_OK;
}

void put_expi(std::vector<double>& v, size_t e, double ph) {
    v[2 * e] = std::cos(ph);
    v[2 * e + 1] = std::sin(ph);
}

// the part of a scene both kinds share: checks, amplitudes, the fixed noise scale
template <class SC>
int scene_common(const MusicDesc& d, bool planar_entry, const SC* sc, int n_inst, MusicSynth* out) {
    if (d.planar != planar_entry)
        return rsp_set_error(RSP_ERR_INVALID, "rsp_music_synthesize_device%s on a %s plan", planar_entry ? "_2d" : "",
                             d.planar ? "planar-array" : "line-array");
    if (sc->n_src < 1 || sc->n_src > MU_MMAX)
        return rsp_set_error(RSP_ERR_UNSUPPORTED, "n_src %d outside 1..%d", sc->n_src, MU_MMAX);
    if (n_inst < 1) return rsp_set_error(RSP_ERR_INVALID, "n_inst %d < 1", n_inst);
    *out = MusicSynth{sc->n_src, sc->complex_sources, sc->snr_measured ? 1 : 0, sc->snr_db,
                      std::sqrt(1.0 / std::pow(10.0, sc->snr_db / 10.0) / 2.0)};   // nsc_fixed
    for (int m = 0; m < sc->n_src; ++m) out->amp[m] = sc->amplitudes[m];
    out->src.assign((size_t)2 * sc->n_src * d.N, 0.0);
    return RSP_OK;
}

}  // namespace

int music_describe(const rsp_music_config* cfg, MusicDesc* out) {
    if (!cfg || !out || !cfg->scan_rad) return rsp_set_error(RSP_ERR_INVALID, "null argument");
    *out = MusicDesc();
    out->N = cfg->channel_num; out->K = cfg->num_snapshots; out->M = cfg->num_sources; out->S = cfg->n_scan;
    out->max_batch = cfg->max_batch;
    out->dl = cfg->d_over_lambda;
    return music_check(*out, cfg->precision);
}

int music_describe(const rsp_music2d_config* cfg, MusicDesc* out) {
    if (!cfg || !out || !cfg->phi_rad || !cfg->theta_rad) return rsp_set_error(RSP_ERR_INVALID, "null argument");
    *out = MusicDesc();
    out->planar = true;
    out->nx = cfg->nx; out->ny = cfg->ny; out->n_phi = cfg->n_phi; out->n_theta = cfg->n_theta;
    out->K = cfg->num_snapshots; out->M = cfg->num_sources;
    out->max_batch = cfg->max_batch;
    out->dxl = cfg->dx_over_lambda; out->dyl = cfg->dy_over_lambda;
    return music_check(*out, cfg->precision);
}

void music_buffer_bytes(const MusicDesc& d, size_t b[MB_COUNT]) {
    const size_t B = (size_t)d.max_batch, cs = d.xsz(), rs = cs / 2;
    b[MB_S1T] = (size_t)MU_NMAX * d.Spad * cs;
    b[MB_EXY] = d.planar ? (size_t)d.S * 2 * 16 : 0;
    b[MB_QS] = d.planar ? B * d.M * MU_NMAX * 16 : 0;
    b[MB_R] = B * MU_NMAX * MU_NMAX * cs;
    b[MB_SPEC] = B * d.S * rs;
    b[MB_EIG] = B * d.N * rs;
    b[MB_PEAKS] = B * MU_PK_ROW * sizeof(int);
    b[MB_SRC] = (size_t)MU_MMAX * MU_NMAX * 16;
    b[MB_AMP] = (size_t)MU_MMAX * sizeof(double);
    b[MB_X] = B * d.K * d.N * cs;
    b[MB_TRACE] = B * 8 * sizeof(unsigned long long);
}

// S1 = exp(1j k z sin(phi_list')) (MUSIC_1D.m:36), stored transposed [channel][angle]
std::vector<double> music_table(const MusicDesc& d, const rsp_music_config* cfg) {
    std::vector<double> s1((size_t)2 * MU_NMAX * d.Spad, 0.0);
    for (int c = 0; c < d.N; ++c)
        for (int s = 0; s < d.S; ++s) put_expi(s1, (size_t)c * d.Spad + s, 2.0 * M_PI * d.dl * c * std::sin(cfg->scan_rad[s]));
    return s1;
}

// per grid point r + n_theta c (theta fastest: Theta_vec, Phi_vec of MUSIC_2D.m:82-84) the two
// unit steps of the separable steering vector (MUSIC_2D.m:87-89)
std::vector<double> music_table(const MusicDesc& d, const rsp_music2d_config* cfg) {
    const double *theta_rad = cfg->theta_rad, *phi_rad = cfg->phi_rad;
    std::vector<double> exy((size_t)d.S * 4);
    for (int c = 0; c < d.n_phi; ++c)
        for (int r = 0; r < d.n_theta; ++r) {
            const double ct = std::cos(theta_rad[r]);
            const size_t g = (size_t)r + (size_t)d.n_theta * c;
            put_expi(exy, 2 * g, 2.0 * M_PI * d.dxl * (ct * std::cos(phi_rad[c])));
            put_expi(exy, 2 * g + 1, 2.0 * M_PI * d.dyl * (ct * std::sin(phi_rad[c])));
        }
    return exy;
}

int music_scene(const MusicDesc& d, const rsp_music_scene* sc, int n_inst, MusicSynth* out) {
    const int rc = scene_common(d, false, sc, n_inst, out);
    if (rc) return rc;
    for (int m = 0; m < sc->n_src; ++m)   // S = exp(1j k z sin(phi')) (MUSIC_1D.m:21)
        for (int c = 0; c < d.N; ++c)
            put_expi(out->src, (size_t)m * d.N + c, 2.0 * M_PI * d.dl * c * std::sin(sc->angles_rad[m]));
    return RSP_OK;
}

int music_scene(const MusicDesc& d, const rsp_music2d_scene* sc, int n_inst, MusicSynth* out) {
    const int rc = scene_common(d, true, sc, n_inst, out);
    if (rc) return rc;
    for (int m = 0; m < sc->n_src; ++m) {   // S(:, m), element iy + ny ix (MUSIC_2D.m:17-19,41-42)
        const double ct = std::cos(sc->elev_rad[m]);
        const double A = ct * std::cos(sc->azim_rad[m]), Bq = ct * std::sin(sc->azim_rad[m]);
        for (int ix = 0; ix < d.nx; ++ix)
            for (int iy = 0; iy < d.ny; ++iy)
                put_expi(out->src, (size_t)m * d.N + iy + d.ny * ix, 2.0 * M_PI * (d.dxl * ix * A + d.dyl * iy * Bq));
    }
    return RSP_OK;
}

int music_want(const rsp_music_out* out) {
    return !out ? MU_WANT_PEAKS : out->eigenvalues ? MU_WANT_EIGS : out->spectrum_db ? MU_WANT_SPECTRUM : MU_WANT_PEAKS;
}

int music_want_of_form(int what, int* want) {
    if (what != RSP_MUSIC_PEAKS && what != RSP_MUSIC_SPECTRUM && what != RSP_MUSIC_EIGENVALUES)
        return rsp_set_error(RSP_ERR_INVALID, "unknown profile form %d", what);
    *want = what == RSP_MUSIC_EIGENVALUES ? MU_WANT_EIGS : what == RSP_MUSIC_SPECTRUM ? MU_WANT_SPECTRUM : MU_WANT_PEAKS;
    return RSP_OK;
}

MusicRoute music_route(const MusicDesc& d, int want) {
    MusicRoute r{};
    r.n_stages = d.planar ? 4 : 2;
    r.cov = d.f64 ? MU_COV_F64 : d.N % 4 == 0 ? MU_COV_F32_VEC4 : MU_COV_F32;
    r.eig = d.planar ? MU_EIG_SUB64 : d.f64 ? MU_EIG_F64 : MU_EIG_F32;
    // The fast-path instantiation: never for a call that reads the eigenvalues, whatever N and M are
    // (an N <= 4 plan asks for neig = N <= 4 too), and never for complex single.  A planar call that
    // reads the spectrum runs the full eigensolver too: the fast path's 1e-12 subspace bound is turned
    // into a P_dB bound (spec_tol) from den_min inside k_music_eig64 only, and the 2-D scan is not there.
    r.fast = d.f64 && d.M <= 4 && (want == MU_WANT_PEAKS || (want == MU_WANT_SPECTRUM && !d.planar));
    r.neig = !d.f64 || want == MU_WANT_EIGS ? d.N : d.M;   // k_music_eig finds all N
    r.spec_tol = r.fast && want == MU_WANT_SPECTRUM ? 1e-8 : 0.0;
    r.lds = !d.f64 ? mu_eig_lds_bytes(d.M) : me_lds_bytes(d.M, d.planar ? 0 : d.S);
    r.raise_lds = r.lds > 64 * 1024;
    r.fast_flag = d.f64 && d.M < MU_MMAX;
    return r;
}

const void* music_in_precision(const MusicDesc& d, const void* src, int dtype, size_t reals, std::vector<unsigned char>& stage) {
    if ((dtype == RSP_C128) == d.f64) return src;
    stage.resize(reals * d.xsz() / 2);
    for (size_t i = 0; i < reals; ++i)
        if (d.f64) ((double*)stage.data())[i] = ((const float*)src)[i];
        else ((float*)stage.data())[i] = (float)((const double*)src)[i];
    return stage.data();
}

void music_fetch_plan(const MusicDesc& d, int n_inst, const rsp_music_out* out, MusicFetch* f) {
    const size_t rs = d.xsz() / 2, I = (size_t)n_inst;
    // `bytes` of buffer b: straight into the caller's array `direct`, or (null) into stage[q]
    auto add = [&](int q, int b, size_t bytes, void* direct) {
        if (!direct) f->stage[q].resize(bytes);
        f->copy[f->n].buf = b; f->copy[f->n].bytes = bytes; f->copy[f->n].dst = direct ? direct : f->stage[q].data();
        ++f->n;
    };
    if (out->spectrum_db) add(0, MB_SPEC, I * d.S * rs, d.f64 ? out->spectrum_db : nullptr);
    if (out->eigenvalues) add(1, MB_EIG, I * d.N * rs, d.f64 ? out->eigenvalues : nullptr);
    if (out->peak_idx || out->n_peaks) add(2, MB_PEAKS, I * MU_PK_ROW * sizeof(int), nullptr);
    if (out->covariance) add(3, MB_R, I * MU_NMAX * MU_NMAX * 2 * rs, nullptr);
}

void music_unpack(const MusicDesc& d, int n_inst, const MusicFetch& f, const rsp_music_out* out) {
    const int N = d.N, M = d.M;
    auto widen = [](const void* src, size_t n, double* dst) { for (size_t i = 0; i < n; ++i) dst[i] = ((const float*)src)[i]; };
    if (!f.stage[0].empty()) widen(f.stage[0].data(), (size_t)n_inst * d.S, out->spectrum_db);
    if (!f.stage[1].empty()) widen(f.stage[1].data(), (size_t)n_inst * N, out->eigenvalues);
    for (int i = 0; i < n_inst && !f.stage[2].empty(); ++i) {
        const int* row = (const int*)f.stage[2].data() + (size_t)i * MU_PK_ROW;
        if (out->n_peaks) out->n_peaks[i] = row[MU_PK_COUNT];
        for (int m = 0; m < M && out->peak_idx; ++m) out->peak_idx[(size_t)i * M + m] = row[MU_PK_PEAK0 + m];
    }
    for (int i = 0; i < n_inst && !f.stage[3].empty(); ++i)   // N x N column-major complex double per instance
        for (int b = 0; b < N; ++b) {
            const size_t e = 2 * ((size_t)i * MU_NMAX * MU_NMAX + (size_t)MU_NMAX * b);
            double* o = out->covariance + 2 * ((size_t)i * N * N + (size_t)N * b);
            if (d.f64) memcpy(o, (const double*)f.stage[3].data() + e, (size_t)2 * N * sizeof(double));
            else widen((const float*)f.stage[3].data() + e, (size_t)2 * N, o);
        }
}

int music_fast_count(const int* peaks, int n_inst) {
    int n = 0;
    for (int i = 0; i < n_inst; ++i) n += peaks[(size_t)i * MU_PK_ROW + MU_PK_FAST] == 1;
    return n;
}
