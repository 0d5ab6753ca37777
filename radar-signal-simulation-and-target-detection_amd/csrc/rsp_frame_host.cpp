// rsp_frame_host.cpp -- the device-free half of the frame chain's host runtime (rsp_frame_host.h): no HIP.
#include "rsp_frame_host.h"

#include <algorithm>
#include <cmath>

namespace {

double mround(double x) { return x < 0 ? -std::floor(-x + 0.5) : std::floor(x + 0.5); }

}  // namespace

void rsp_convert_reals(const void* src, int dtype, size_t reals, void* dst) {
    if (dtype == RSP_C64) {
        const float* a = (const float*)src;
        double* o = (double*)dst;
        for (size_t i = 0; i < reals; ++i) o[i] = a[i];
    } else {
        const double* a = (const double*)src;
        float* o = (float*)dst;
        for (size_t i = 0; i < reals; ++i) o[i] = (float)a[i];
    }
}

int rsp_stage2_regate(int P, int N, int B, const void* iq, int dtype, int n_gated, const int32_t* cols,
                      std::vector<unsigned char>& full) {
    if (dtype != RSP_C64 && dtype != RSP_C128) return rsp_set_error(RSP_ERR_INVALID, "unknown dtype %d", dtype);
    static const int32_t kRefCols[6] = {83, 310, 311, 1033, 1034, 3486};   // main_simulate_echoes_with_array_v2.m:257-264
    const int32_t* c = cols ? cols : kRefCols;
    int total = 0;
    for (int k = 0; k < 3; ++k) {
        if (c[2 * k] < 1 || c[2 * k + 1] < c[2 * k] || c[2 * k + 1] > N)
            return rsp_set_error(RSP_ERR_INVALID, "gate columns %d..%d of segment %d outside the %d-sample PRT", c[2 * k],
                                 c[2 * k + 1], k, N);
        if (k > 0 && c[2 * k] <= c[2 * k - 1])   // ascending and disjoint, like v2:257-264
            return rsp_set_error(RSP_ERR_INVALID, "gate columns of segment %d (%d..%d) overlap or precede segment %d (..%d)",
                                 k, c[2 * k], c[2 * k + 1], k - 1, c[2 * k - 1]);
        total += c[2 * k + 1] - c[2 * k] + 1;
    }
    if (total != n_gated)
        return rsp_set_error(RSP_ERR_INVALID, "gated input has %d columns, the gate columns cover %d", n_gated, total);
    // put the gated columns back at their PRT positions (zeros elsewhere): [P x N x B]
    const size_t es = dtype == RSP_C128 ? 16 : 8, colb = (size_t)P * es;
    full.assign((size_t)N * B * colb, 0);
    const unsigned char* src = static_cast<const unsigned char*>(iq);
    for (int b = 0; b < B; ++b) {
        int ng = 0;
        for (int k = 0; k < 3; ++k)
            for (int col = c[2 * k] - 1; col < c[2 * k + 1]; ++col, ++ng)
                memcpy(&full[((size_t)b * N + col) * colb], src + ((size_t)b * n_gated + ng) * colb, colb);
    }
    return RSP_OK;
}

int rsp_s3_check_cells(int P, int G, int n_maps) {
    if (n_maps < 1 || n_maps > 65535 || (int64_t)n_maps * P * G >= ((int64_t)1 << 31) || (P + RSP_S3_ROWS - 1) / RSP_S3_ROWS > 65535)
        return rsp_set_error(RSP_ERR_INVALID, "%d maps of %d x %d cells: 1 .. 65535 maps and fewer than 2^31 cells in all", n_maps,
                             P, G);
    return RSP_OK;
}

void rsp_s3_sorted_hits(rsp_stage3_hit* h, int64_t n, rsp_stage3_hit* out, int64_t cap) {
    std::sort(h, h + n, [](const rsp_stage3_hit& a, const rsp_stage3_hit& b) {
        if (a.beam_idx != b.beam_idx) return a.beam_idx < b.beam_idx;
        if (a.r_idx != b.r_idx) return a.r_idx < b.r_idx;
        return a.v_idx < b.v_idx;
    });
    if (std::min(n, cap) > 0) memcpy(out, h, sizeof(rsp_stage3_hit) * (size_t)std::min(n, cap));
}

void rsp_result_rows(int frame_idx, const rsp_target* t, size_t nt, double* rows, int64_t cap, int64_t* n) {
    for (size_t i = 0; i < std::max<size_t>(nt, 1); ++i, ++*n) {
        if (!rows || *n >= cap) continue;
        double* o = rows + 5 * *n;
        o[0] = frame_idx;
        if (nt) {
            o[1] = t[i].Range; o[2] = t[i].Velocity; o[3] = t[i].Angle; o[4] = t[i].Power;
        } else {   // an empty frame stays visible as one NaN row
            o[1] = o[2] = o[3] = o[4] = std::nan("");
        }
    }
}

void rsp_synth_targets(const SynthConsts& sc, const rsp_target_in* t, int nt, double p_noise, SynthTargets* out) {
    *out = SynthTargets{};
    for (int i = 0; i < nt; ++i) {   // fsf:51-72
        const double delay = 2.0 * t[i].Range / sc.c;
        out->t[i].delay = (int)mround(delay / (1.0 / sc.fs));
        out->t[i].fd_prt = 2.0 * t[i].Velocity / sc.wavelength * sc.prt;
        out->t[i].amp = std::sqrt(std::pow(10.0, t[i].SNR_dB / 10.0) * p_noise / sc.p_signal_unscaled);
        out->t[i].dphi = 2.0 * M_PI * sc.d * std::sin(t[i].ElevationAngle * M_PI / 180.0) / sc.wavelength;
    }
}

void rsp_stage_bytes(const Geometry& g, int es, int nf, bool rdm, int cap, int64_t* out, int k2_rows) {
    const int64_t kr = k2_rows < 0 ? g.P : k2_rows;                       // Doppler rows per beam K2 launches
    const int64_t rs = es / 2;                                            // real element bytes
    const int64_t cube = (int64_t)g.C * g.nU * g.P * es;                  // used fast-time samples
    const int64_t z = (int64_t)g.B * g.nU * g.P * es;                     // Doppler-domain rows
    const int64_t mag = (int64_t)g.B * g.P * g.G * rs;                    // |RD| map (the RDM stays on chip)
    if (cap > 0) out[0] = nf * (cube + z);
    // the complex RD map, when written, is read by K3 only at the detected cells (2 values per
    // detection, not a map-sized stream), so K3's bytes stay the magnitude maps
    if (cap > 1) out[1] = nf * ((z + mag) * kr / g.P + (rdm ? (int64_t)g.B * kr * g.G * es : 0));
    if (cap > 2) out[2] = nf * k3_map_bytes(g, (int)rs);   // the rows under test
}

// every cell read once (the halo re-reads are cache hits), every output cell written once
void rsp_stage3_bytes(int64_t cells, int es, int64_t out[3]) {
    out[0] = cells * (es / 2 + 8 + 1);
    out[1] = cells * (es + 8 + 8 + 1);
    out[2] = cells * es;
}
