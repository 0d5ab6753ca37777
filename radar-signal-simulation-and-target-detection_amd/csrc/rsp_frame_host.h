// rsp_frame_host.h -- the device-free half of the frame chain's host runtime: the layouts of the
// maps a call returns, the precision conversions, the re-insertion of a gated stage-2 input, the
// result lists and rows, the synthesis constants of a target list and the profilers' byte counts.
// Plain C++17 like rsp_geometry.h: rsp_frame_host.cpp builds, runs and is sanitized without a GPU;
// the plan units (rsp_plan*.cpp) keep the hipMemcpy on either side of these.
#pragma once
#include "rsp_geometry.h"   // rsp.h, Geometry, SynthTargets

#include <cstring>

__attribute__((visibility("hidden"))) int rsp_set_error(int code, const char* fmt, ...);   // rsp_host.cpp

// n planes of rows x cols elements, cols fastest -> n planes of cols x rows, rows fastest:
// dst[i + rows * (j + cols * b)] = src[(b * rows + i) * cols + j].  A device map [n][P][G] to MATLAB's
// column-major [P x G x n] is (rows, cols) = (P, G); MATLAB to device is (G, P).  S and D: float,
// double, std::complex of either, uint8_t.  Each value is converted once, as the assignment of a
// float to a double (widening) or the cast of a double to float (narrowing): no arithmetic.
template <class S, class D>
void rsp_transpose_planes(const S* src, int rows, int cols, int n, D* dst) {
    for (int b = 0; b < n; ++b)
        for (int i = 0; i < rows; ++i) {
            const S* s = src + ((size_t)b * rows + i) * cols;
            D* d = dst + (size_t)b * rows * cols + i;
            for (int j = 0; j < cols; ++j) d[(size_t)rows * j] = static_cast<D>(s[j]);
        }
}

// `reals` scalars of src (dtype RSP_C64: float, RSP_C128: double) into dst in the other type: floats
// widened, doubles narrowed by a (float) cast.  A complex array is 2 scalars per element.
void rsp_convert_reals(const void* src, int dtype, size_t reals, void* dst);

// Gated stage-2 input [P x n_gated x B] -> full-PRT [P x N x B] in `full`, the gated columns at their
// PRT positions (cols: 1-based first and last column of the 3 segments; null: the reference's) and
// zeros elsewhere, after the checks of rsp_process_stage2_gated.
int rsp_stage2_regate(int P, int N, int B, const void* iq, int dtype, int n_gated, const int32_t* cols,
                      std::vector<unsigned char>& full);

// The map count the stage-3 kernel's 32-bit hit counter and grid admit
int rsp_s3_check_cells(int P, int G, int n_maps);
// The device's hit list (in no order) in beam, then find() order on [P x G] (r outer, v inner): sorts
// h[0 .. n) in place and copies its first min(n, cap) records to out.
void rsp_s3_sorted_hits(rsp_stage3_hit* h, int64_t n, rsp_stage3_hit* out, int64_t cap);

// A list of n records into a caller's array of cap: *n_out = n (when not null); with dst, the first
// min(n, cap) records, and RSP_ERR_OVERFLOW when n > cap, with the caller's message (fmt and its
// arguments).  dst null: a size query, RSP_OK.
template <class T, class N, class... A>
int rsp_capped_copy(T* dst, const T* src, int64_t n, int64_t cap, N* n_out, const char* fmt, A... a) {
    if (n_out) *n_out = (N)n;
    if (!dst) return RSP_OK;
    const int64_t m = n < cap ? n : cap;
    if (m > 0) memcpy(dst, src, sizeof(T) * (size_t)m);
    return n > cap ? rsp_set_error(RSP_ERR_OVERFLOW, fmt, a...) : RSP_OK;
}

// The rows of one frame for rsp_results_rows: (frame_idx, Range, Velocity, Angle, Power) per target,
// or one row of NaNs after frame_idx for a frame without targets.  Row *n on; written while rows is
// not null and *n < cap; *n counts every row.
void rsp_result_rows(int frame_idx, const rsp_target* t, size_t nt, double* rows, int64_t cap, int64_t* n);

// What S4 needs of the configuration, and the per-target constants of a target list (fsf:51-72)
struct SynthConsts {
    double c = 0, fs = 0, wavelength = 0, d = 0, prt = 0, p_signal_unscaled = 0;
};
void rsp_synth_targets(const SynthConsts& sc, const rsp_target_in* t, int nt, double p_noise, SynthTargets* out);

// Algorithmic bytes of rsp_profile_stages_rdm per launch of nf frames (DESIGN.md "Measurement"):
// the first min(cap, 3) of K1, K2, K3.  es: bytes of a complex element; rdm: K2 writes the complex
// RD map (the caller's maps, or the lane's own with the complex-ratio monopulse).  k2_rows: the
// Doppler rows per beam the K2 launch covers (the band route's rows under test; < 0: all P).
void rsp_stage_bytes(const Geometry& g, int es, int nf, bool rdm, int cap, int64_t* out, int k2_rows = -1);
// ... and of rsp_profile_stage3's three forms over `cells` cells
void rsp_stage3_bytes(int64_t cells, int es, int64_t out[3]);
