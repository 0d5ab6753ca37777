// rsp_music_geometry.h -- the device-free half of a MUSIC plan (line and planar arrays): the plan
// description and its checks, the buffer sizes, the host tables, the route of a call (which kernels
// it runs and with what) and the host conversions of snapshots and results.  Plain C++17 like
// rsp_geometry.h: rsp_music_geometry.cpp builds, runs and is sanitized without a GPU; the kernels
// (rsp_music.hip) include this header for the constants and the LDS formulae.
#pragma once
#include "rsp_geometry.h"   // rsp.h, RSP_HD

#define MU_NMAX 64          // channels (the leading dimension of R and of the steering tables)
#define MU_MMAX 8           // sources
#define MU_SCAN_MAX 4096    // scan points of a line plan
#define M2_SMAX 65536       // grid points of a planar plan
#define ME_VW 68            // padded length of a v / w buffer (k_music_eig64)

// One row of the peaks buffer per instance: [count | MU_MMAX peaks (1-based, 0 = none)].  With
// M < MU_MMAX the last peak slot is free, and the complex-double eigen kernels write there which
// path ran (1: the block-power fast path; MusicRoute::fast_flag, music_fast_count).
enum { MU_PK_COUNT = 0, MU_PK_PEAK0 = 1, MU_PK_FAST = MU_MMAX, MU_PK_ROW = MU_MMAX + 1 };

// Dynamic LDS of k_music_eig<M> (complex single)
RSP_HD constexpr size_t mu_eig_lds_bytes(int M) {
    return (size_t)MU_NMAX * MU_NMAX * 8 + MU_NMAX * 8 + 4 * MU_NMAX * 4 + (size_t)5 * M * MU_NMAX * 4 +
           (size_t)M * MU_NMAX * 8 + MU_NMAX * 16;
}
// k_music_eig64 / k_music_sub64: the inverse iteration's [5][64][M] LU / y array; the back-transform
// stages a wave's 16 reflectors ([16][ME_VW] complex) in the same space once the vectors have left it
RSP_HD constexpr int me_lu_doubles(int M) { return 5 * 64 * M > 32 * ME_VW ? 5 * 64 * M : 32 * ME_VW; }
RSP_HD constexpr size_t me_lds_bytes(int M, int S) {
    return (size_t)4 * ME_VW * 16 + 64 * 16 + 8 * 16 + 3 * 68 * 8 + 64 * 8 + (size_t)me_lu_doubles(M) * 8 + (size_t)M * 64 * 16 +
           ((size_t)S + 8) * 8 + 8 * 16;
}

// A plan, as both create functions fill it.  Planar: N = nx ny, S = n_theta n_phi, no S1T (Spad 0).
struct MusicDesc {
    bool planar = false;
    bool f64 = true;     // RSP_C128 (MATLAB's complex double, default) or RSP_C64
    int N = 0, K = 0, M = 0, S = 0, Spad = 0, max_batch = 0;
    int nx = 0, ny = 0, n_theta = 0, n_phi = 0;
    double dl = 0.0, dxl = 0.0, dyl = 0.0;
    size_t xsz() const { return f64 ? 16 : 8; }   // bytes of one snapshot sample
};
// The checks of rsp_music_create / rsp_music_create_2d that need no device, then the description.
// RSP_OK, or the status of the first refusal with its message set.
int music_describe(const rsp_music_config* cfg, MusicDesc* out);
int music_describe(const rsp_music2d_config* cfg, MusicDesc* out);

// Device buffers of a plan; 0 bytes: the plan has none.  create allocates all but MB_X (the host
// entry's staging, on first use) and MB_TRACE (diagnostic builds); destroy frees them all.
enum MusicBuf {
    MB_S1T,     // steering table [64][Spad] complex, zero rows for c >= N
    MB_EXY,     // [S][2] complex double: (ex, ey) of grid point r + n_theta c (k_music_scan2d)
    MB_QS,      // [max_batch][M][64] complex double signal subspace (k_music_sub64)
    MB_R,       // [max_batch][64][64] complex
    MB_SPEC,    // [max_batch][S] real
    MB_EIG,     // [max_batch][N] real
    MB_PEAKS,   // [max_batch][MU_PK_ROW] int
    MB_SRC,     // synthesis: source steering [MU_MMAX][N] complex double
    MB_AMP,     // [MU_MMAX] double
    MB_X,       // [max_batch][K][N] complex
    MB_TRACE,   // [max_batch][8] phase stamps
    MB_COUNT
};
void music_buffer_bytes(const MusicDesc& d, size_t bytes[MB_COUNT]);

// The steering table of a plan, complex as (re, im) pairs of doubles
std::vector<double> music_table(const MusicDesc& d, const rsp_music_config* cfg);     // MB_S1T: [64][Spad]
std::vector<double> music_table(const MusicDesc& d, const rsp_music2d_config* cfg);   // MB_EXY: [S][2]
// `reals` values of type dtype (RSP_C64: float, RSP_C128: double) in the plan's precision: src
// itself, or `stage` filled with them widened / narrowed (host snapshots; S1T of a complex-single plan)
const void* music_in_precision(const MusicDesc& d, const void* src, int dtype, size_t reals, std::vector<unsigned char>& stage);

// A synthesis call: the scene checks of the two synthesize entries and what k_music_synth takes
struct MusicSynth {
    int n_src = 0, complex_src = 0, snr_measured = 0;
    double snr_db = 0.0, nsc_fixed = 0.0, amp[MU_MMAX] = {};
    std::vector<double> src;   // source steering [n_src][N] complex
};
int music_scene(const MusicDesc& d, const rsp_music_scene* sc, int n_inst, MusicSynth* out);
int music_scene(const MusicDesc& d, const rsp_music2d_scene* sc, int n_inst, MusicSynth* out);

// What a call's caller reads: only the peak indices, also the pseudo-spectrum, or also all N eigenvalues
enum MusicWant { MU_WANT_PEAKS = 0, MU_WANT_SPECTRUM = 1, MU_WANT_EIGS = 2 };
int music_want(const rsp_music_out* out);
int music_want_of_form(int what, int* want);   // RSP_MUSIC_* of the profile entries; refuses others

// The route of a call: stages 0 .. n_stages - 1 of MusicStage in order, and what each is launched with
enum MusicStage { MU_ST_COV, MU_ST_EIG, MU_ST_SCAN2D, MU_ST_PEAKS2D };
enum MusicCov { MU_COV_F64, MU_COV_F32_VEC4, MU_COV_F32 };
enum MusicEig { MU_EIG_F32, MU_EIG_F64, MU_EIG_SUB64 };   // k_music_eig<M>, k_music_eig64<M, fast>, k_music_sub64<M, fast>
struct MusicRoute {
    int n_stages;       // 2 (line) or 4 (planar): also the timed stages of the profile entries
    int cov, eig;
    bool fast;          // the instantiation that may keep the block-power subspace instead of the eigensolver
    int neig;           // eigenvalues the kernel finds: all N when the caller reads them, else the M signal ones
    double spec_tol;    // a spectrum call keeps the fast subspace only where it bounds P_dB's error by this
    size_t lds;         // dynamic LDS bytes of the eigen kernel
    bool raise_lds;     // more than the 64 KiB a kernel gets without the attribute
    bool fast_flag;     // the eigen kernel writes MU_PK_FAST
};
MusicRoute music_route(const MusicDesc& d, int want);

// What a call copies back: n copies of `bytes` from buffer `buf` to dst -- the caller's array, or a
// stage[] (device-shaped: spectrum, eigenvalues, peaks rows, padded R) that music_unpack converts:
// the peaks rows -> n_peaks / peak_idx, the 64 x 64 R -> N x N column-major, complex single widened.
struct MusicFetch {
    std::vector<unsigned char> stage[4];
    struct { int buf; size_t bytes; void* dst; } copy[4];
    int n = 0;
};
void music_fetch_plan(const MusicDesc& d, int n_inst, const rsp_music_out* out, MusicFetch* f);
void music_unpack(const MusicDesc& d, int n_inst, const MusicFetch& f, const rsp_music_out* out);
// instances whose peaks row says the fast path ran (plans with MusicRoute::fast_flag)
int music_fast_count(const int* peaks, int n_inst);
