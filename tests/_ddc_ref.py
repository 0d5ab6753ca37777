"""The digital down-converter's definition (include/rsp.h, "digital down-conversion") restated in numpy long
double, with the NCO's integer phase in Python ints: what tests/test_ddc.py holds k_ddc against, and what
tests/test_ddc_ref.py holds against known answers.

ddc_ref returns the exact-arithmetic value of every output part (long double: 64 bits of mantissa, 2^-11 of a
double's unit) and, per element, b = sum_j |h_j| |x[off + k D - j]|, the scale every rounding of the kernel is
relative to (|m| <= 1).  matlab_form is simulation_learn.m:79-102 as MATLAB evaluates it, in doubles.
"""
from fractions import Fraction

import numpy as np

LD = np.longdouble
TWO_PI = LD(2) * LD('3.14159265358979323846264338327950288')
U = {'c128': 2.0 ** -53, 'c64': 2.0 ** -24}   # unit roundoff of the plan's reals


def phase_word(f0, fs):
    """round(f0 / fs 2^64) mod 2^64 of the two doubles, exactly."""
    return int(round(Fraction(f0) / Fraction(fs) * 2 ** 64)) % 2 ** 64


def nco_u(N, w, w0=0):
    """u_n = floor(((w0 + n w) mod 2^64) / 2^11) 2^-53, n < N: exact doubles in [0, 1)."""
    return np.array([((w0 + n * w) % 2 ** 64) >> 11 for n in range(N)], np.float64) * 2.0 ** -53


def sincos_2pi(u):
    """(sin, cos)(2 pi u) in long double, u exact doubles in [0, 1]: the quarter turn is taken off exactly
    (q = round(4 u), u - q / 4 has no rounding), so that u = 1/4, 1/2, 3/4 give 0 and +-1 exactly."""
    u = np.asarray(u, np.float64)
    q = np.rint(4.0 * u)
    x = TWO_PI * (u - 0.25 * q).astype(LD)
    s, c = np.sin(x), np.cos(x)
    q = q.astype(np.int64) & 3
    s0 = np.where(q & 1, c, s)
    c0 = np.where(q & 1, s, c)
    return np.where(q & 2, -s0, s0), np.where((q + 1) & 2, -c0, c0)


def nco(N, w, w0=0, mode='iq'):
    """(Re m, Im m)[n] in long double: 'iq' cos - i sin, 'sin' sin + 0 i."""
    s, c = sincos_2pi(nco_u(N, w, w0))
    return (c, -s) if mode == 'iq' else (s, np.zeros(N, LD))


def cube3(x):
    x = np.asarray(x)
    return x[None, :, None] if x.ndim == 1 else (x[:, :, None] if x.ndim == 2 else x)


def ddc_ref(x, h, D, w, w0=0, mode='iq', off=0):
    """(Re y, Im y, b), long double [P, No, C], of real x [P, N, C] (or [P, N], [N]: then as [1, N, 1])."""
    x = cube3(x).astype(LD)
    h = np.asarray(h, np.float64).ravel().astype(LD)
    P, N, C = x.shape
    mr, mi = nco(N, w, w0, mode)
    vr, vi, ax = x * mr[None, :, None], x * mi[None, :, None], np.abs(x)
    yr, yi, b = (np.zeros((P, N, C), LD) for _ in range(3))
    for j in range(min(h.size, N)):
        yr[:, j:] += h[j] * vr[:, :N - j]
        yi[:, j:] += h[j] * vi[:, :N - j]
        b[:, j:] += abs(h[j]) * ax[:, :N - j]
    return yr[:, off::D], yi[:, off::D], b[:, off::D]


def ddc_ref_complex(x, h, D, w, w0=0, mode='iq', off=0):
    yr, yi, _ = ddc_ref(x, h, D, w, w0, mode, off)
    return yr.astype(np.float64) + 1j * yi.astype(np.float64)


def matlab_form(xt, f, fs, Num, D):
    """simulation_learn.m:76-102 in doubles: t2 = 0 : 1/fs : (N-1)/fs, xrt = xt .* sin(2*pi*f*t2), firxrt =
    filter(Num, 1, xrt), downsample(firxrt, D)."""
    xt = np.asarray(xt, np.float64).ravel()
    Num = np.asarray(Num, np.float64).ravel()
    t2 = np.arange(xt.size) * (1.0 / fs)
    xrt = xt * np.sin(2 * np.pi * f * t2)
    return np.convolve(xrt, Num)[:xt.size][::D]


def matlab_allowance(xt, f, fs, Num, D, u=2.0 ** -53):
    """b (3 u theta_max + (L + 6) u) per output of matlab_form against ddc_ref at phase_word(f, fs): the
    argument 2*pi*f*t2 carries three roundings (the step 1/fs times n, times 2 pi f in two products), each u of
    a value up to theta_max = 2 pi f (N - 1) / fs, and the sine moves by no more than its argument; the double
    filter is the L + 6 roundings of tests/test_ddc.py's bound.  (The NCO's own 2^-53 of a turn and the word's
    2^-65 N are below u theta_max.)"""
    xt = np.asarray(xt, np.float64).ravel()
    Num = np.asarray(Num, np.float64).ravel()
    b = np.convolve(np.abs(xt), np.abs(Num))[:xt.size][::D]
    theta_max = 2 * np.pi * f * (xt.size - 1) / fs
    return b * (3 * u * theta_max + (Num.size + 6) * u)


def lfm_cut(n0=6000, n=2000, seed=20250101):
    """A cut of simulation_learn.m's echo line (:11-48): the 10 MHz, 10 MHz-wide, 10 us LFM pulse of target 1
    (10 km: sample 6667) in white noise of power 1e-2, samples n0 .. n0 + n of the 50 000."""
    f, fs, B, T = 10e6, 100e6, 1e7, 1e-5
    t1 = np.arange(int(round(T * fs))) / fs
    y = np.sin(2 * np.pi * (f * t1 + 0.5 * (B / T) * t1 ** 2))
    n1 = int(round(2 * 10000 / 3e8 * fs))
    xt = np.zeros(50000)
    xt[n1:n1 + y.size] = y
    xt += np.sqrt(1e-2 / 2) * np.random.default_rng(seed).standard_normal(xt.size)
    return xt[n0:n0 + n].copy(), f, fs
