// rsp_s9.h -- S9 of one detection (fun_parameter_estimation_9, fsf:237-290): the spline-refined range
// and velocity and the monopulse angle, shared by k3_cfar and k3_finish (rsp_k3.hip) and by the
// stand-alone detector's k_s9 (rsp_detect.hip), so that the two give the same bits on the same maps.
#pragma once
#include "rsp_device.h"

namespace {

// Peak of MATLAB interp1(...,'spline') (not-a-knot) sampled at step 1/interp over n
// equally spaced points (fsf:257-260, 272-275); returns the first-argmax abscissa.
template <int INTERP>
__device__ __forceinline__ double spline_peak(const double* y, int n) {
    // Piecewise-cubic coefficients per unit interval, then Horner at q / INTERP; the sample
    // grid and the first-argmax rule are the reference's (interp1 on cells(1):1/INTERP:cells(end)).
    constexpr double dx = 1.0 / INTERP;   // 1/8, 1/4: exact
    double c0[4], c1[4], c2[4], c3[4];   // value on [i, i+1]: ((c3 t + c2) t + c1) t + c0
    if (n == 5) {   // not-a-knot second derivatives, unit spacing (closed form of the 5x5 system)
        double Mv[5];
        Mv[1] = y[0] - 2.0 * y[1] + y[2];
        Mv[3] = y[2] - 2.0 * y[3] + y[4];
        Mv[2] = (6.0 * (y[1] - 2.0 * y[2] + y[3]) - Mv[1] - Mv[3]) * 0.25;
        Mv[0] = 2.0 * Mv[1] - Mv[2];
        Mv[4] = 2.0 * Mv[3] - Mv[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            c0[i] = y[i];
            c1[i] = (y[i + 1] - y[i]) - (2.0 * Mv[i] + Mv[i + 1]) * (1.0 / 6.0);
            c2[i] = 0.5 * Mv[i];
            c3[i] = (Mv[i + 1] - Mv[i]) * (1.0 / 6.0);
        }
    } else {          // n == 4: the single cubic through 4 points; n == 3: the parabola
        const double d1 = y[1] - y[0], d2_ = y[2] - 2.0 * y[1] + y[0];
        const double d3 = (n == 4) ? y[3] - 3.0 * y[2] + 3.0 * y[1] - y[0] : 0.0;
        // Newton form about x = 0 expanded at each integer knot i
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double x = i;
            c0[i] = y[0] + x * d1 + x * (x - 1.0) * 0.5 * d2_ + x * (x - 1.0) * (x - 2.0) * (1.0 / 6.0) * d3;
            c1[i] = d1 + (2.0 * x - 1.0) * 0.5 * d2_ + (3.0 * x * x - 6.0 * x + 2.0) * (1.0 / 6.0) * d3;
            c2[i] = 0.5 * d2_ + (3.0 * x - 3.0) * (1.0 / 6.0) * d3;
            c3[i] = (1.0 / 6.0) * d3;
        }
    }
    // samples q = 0 .. (n-1) INTERP in order (first argmax wins); sample q lies on interval
    // min(q / INTERP, n - 2) like ppval -- every array index is a compile-time constant
    double best = -INFINITY, bx = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i < n - 1) {
#pragma unroll
            for (int t = 0; t < INTERP; ++t) {
                const double tt = t * dx;
                const double val = ((c3[i] * tt + c2[i]) * tt + c1[i]) * tt + c0[i];
                if (val > best) {
                    best = val;
                    bx = (i * INTERP + t) * dx;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {   // the last sample: end of the last interval
        if (i == n - 2) {
            const double val = ((c3[i] + c2[i]) + c1[i]) + c0[i];
            if (val > best) bx = (n - 1);
        }
    }
    return bx;
}

// The axes, angles and K-LUT S9 reads (DevConsts fields), by value so that the out-of-line
// spill path below takes them in registers.
struct S9Consts {
    const double *range_axis, *velocity_axis, *beam_angles, *klut;
    double deltaR, deltaV;
};

// S9 of one detection from the workgroup's S tile (fsf:237-290).
// sval(v, r) = S at Doppler row v, range cell r (the tile, or the maps when the tile lacks it).
// RA / RB (RSP_PLAN_MONOPULSE_COMPLEX, else null): the complex RD map rows of beams pair, pair + 1.
template <class T, class SF>
__device__ __forceinline__ void s9_estimate(const S9Consts& k, SF sval, int P, int G, int Gp, int v, int r, int pair,
                                            const T* __restrict__ MA, const T* __restrict__ MB,
                                            const cx<T>* __restrict__ RA, const cx<T>* __restrict__ RB, DevDet* out) {
    // the 5-cell windows clipped to the map (fsf:241-250): cells first .. first + n - 1
    const int rfirst = max(r - 2, 0), nrc = min(r + 2, G - 1) - rfirst + 1;
    const int vfirst = max(v - 2, 0), nvc = min(v + 2, P - 1) - vfirst + 1;
    double yr[5], yv[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        yr[j] = j < nrc ? (double)sval(v, rfirst + j) : 0.0;
        yv[j] = j < nvc ? (double)sval(vfirst + j, r) : 0.0;
    }
    const double rmax = (nrc < 3) ? (double)r : rfirst + spline_peak<8>(yr, nrc);
    const double vmax = (nvc < 3) ? (double)v : vfirst + spline_peak<4>(yv, nvc);
    double ratio;
    if (RA) {   // complex ratio real((S_A - S_B) / (S_A + S_B + eps)) (main_plot_snr_vs_angle_error.m:455-462)
        const cx<T> a = RA[(size_t)v * G + r], b = RB[(size_t)v * G + r];
        const double nx = (double)a.x - (double)b.x, ny = (double)a.y - (double)b.y;
        const double dx = (double)a.x + (double)b.x + 2.220446049250313e-16, dy = (double)a.y + (double)b.y;
        ratio = (nx * dx + ny * dy) / (dx * dx + dy * dy);
    } else {    // amplitude monopulse on the integer cell (fsf:282-290)
        const double SA = (double)MA[(size_t)v * Gp + r];
        const double SB = (double)MB[(size_t)v * Gp + r];
        ratio = (SA - SB) / (SA + SB + 2.220446049250313e-16);
    }
    DevDet d;
    d.v_idx = v + 1;
    d.r_idx = r + 1;
    d.pair_idx = pair + 1;
    d.reserved = 0;
    d.amp = (double)sval(v, r);
    d.range = k.range_axis[r] + (rmax - r) * k.deltaR;
    d.velocity = k.velocity_axis[v] + (vmax - v) * k.deltaV;
    d.angle = 0.5 * (k.beam_angles[pair] + k.beam_angles[pair + 1]) + k.klut[pair] * ratio;
    *out = d;
}

}  // namespace
