"""CPU tests of the stand-alone MTD's arithmetic without a device: the tables of rsp_mtd_table, and the
kernel's algorithm restated in numpy from those tables (tests/_mtd_ref.py) against the exact transform
over the case table of tests/_mtd_cases.py -- which is also where the tolerance constant of the GPU
tests comes from.

Where np.longdouble is no wider than double the exact transform is no better than the restatement in
complex double; the tests that need the wider type say so and run on the complex-single half alone."""
import functools

import numpy as np
import pytest

from rsp.plan import describe_mtd, mtd_table
from _mtd_cases import CASES, CASE_IDS, PRECS, U, C_TOL, G_MAIN, MAPS_MAIN, tolerance, kaiser32, gaussian, col_err
from _mtd_ref import exact, restated, shift_rows, LONGDOUBLE_OK

_PI = np.longdouble('3.141592653589793238462643383279502884')
_RT = {'c128': np.float64, 'c64': np.float32}
PRECS_HERE = PRECS if LONGDOUBLE_OK else ('c64',)


@functools.lru_cache(maxsize=None)
def _exact_main(P, nfft):
    return exact(gaussian(P, G_MAIN, MAPS_MAIN), kaiser32(P), nfft)


@functools.lru_cache(maxsize=None)
def _ratio(P, nfft, prec):
    """The restatement's largest column error at a case, in units of u log2(max(M, 2))."""
    M = describe_mtd(P, G_MAIN, nfft, prec)['M']
    got = restated(gaussian(P, G_MAIN, MAPS_MAIN), kaiser32(P), nfft, True, prec)
    return col_err(got, _exact_main(P, nfft)).max() / (U[prec] * np.log2(max(M, 2)))


@pytest.mark.parametrize('prec', PRECS_HERE)
def test_tolerance_constant(prec):
    """C_TOL of _mtd_cases.py is 4 x the restatement's largest err / (u log2 M) over the GPU case table."""
    worst = max(_ratio(P, n, prec) for P, n in CASES)
    print('%s: largest err / (u log2 M) = %.4f, 4 x = %.4f, C_TOL = %.4f' % (prec, worst, 4 * worst, C_TOL[prec]))
    assert abs(C_TOL[prec] / (4 * worst) - 1) <= 0.10


@pytest.mark.parametrize('prec', PRECS_HERE)
@pytest.mark.parametrize('P, nfft', CASES, ids=CASE_IDS)
def test_restated_meets_the_tolerance(P, nfft, prec):
    M = describe_mtd(P, G_MAIN, nfft, prec)['M']
    r = _ratio(P, nfft, prec)
    print('%d -> %d %s M=%d: err %.3g = %.3f u log2 M, tolerance %.3g' % (P, nfft, prec, M, r * U[prec] * np.log2(max(M, 2)),
                                                                          r, tolerance(prec, M)))
    assert r * U[prec] * np.log2(max(M, 2)) <= tolerance(prec, M)


def test_exact_is_the_definition():
    """exact() against numpy's FFT (to complex-double rounding), the shift for odd and even lengths,
    zero fill and the natural order."""
    for P, n in ((5, 7), (7, 7), (6, 6), (16, 16), (33, 64), (96, 96)):
        x, win = gaussian(P, 3, 2, seed=9), kaiser32(P)
        want = np.fft.fft(x * win[:, None, None], n, axis=0)
        got = exact(x, win, n, shift=False)
        assert np.abs(got - want).max() <= 64 * 2.0 ** -53 * np.abs(want).max()
        np.testing.assert_array_equal(exact(x, win, n, shift=True), np.fft.fftshift(got, axes=0))
        np.testing.assert_array_equal(shift_rows(got, n), np.fft.fftshift(got, axes=0))
    x = np.ones((1, 2))
    np.testing.assert_array_equal(exact(x, np.array([3.0]), 8), np.full((8, 2), 3.0))   # P = 1: every bin = win[0] x[0]


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('nfft', sorted({n for _, n in CASES if n & (n - 1)}))
def test_chirp_entries_to_the_bit(nfft, prec):
    """w[m] = exp(-i pi (m^2 mod 2 nfft) / nfft) evaluated in long double and rounded once."""
    w, _ = mtd_table(nfft, prec)
    m = np.arange(nfft, dtype=np.int64)
    ang = -_PI * ((m * m) % (2 * nfft)).astype(np.longdouble) / np.longdouble(nfft)
    R = _RT[prec]
    np.testing.assert_array_equal(w.real, np.cos(ang).astype(R).astype(np.float64))
    np.testing.assert_array_equal(w.imag, np.sin(ang).astype(R).astype(np.float64))


@pytest.mark.skipif(not LONGDOUBLE_OK, reason='needs a long double wider than double to judge 4 u in complex double')
@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('nfft', [3, 7, 15, 17, 33, 83, 129, 332, 333, 513, 1025, 2047])
def test_filter_spectrum(nfft, prec):
    """Bf is the M-point DFT of conj(w) wrapped round M, divided by M, to 4 u of its largest entry
    (the table is rounded once: u / 2 per part; the long double transforms account for the rest)."""
    w, Bf = mtd_table(nfft, prec)
    M = len(Bf)
    assert M == describe_mtd(nfft, 1, nfft, prec)['M']
    m = np.arange(nfft, dtype=np.int64)
    ang = -_PI * ((m * m) % (2 * nfft)).astype(np.longdouble) / np.longdouble(nfft)
    cw = np.cos(ang) - 1j * np.sin(ang)
    b = np.zeros(M, np.clongdouble)
    b[:nfft] = cw
    b[M - nfft + 1:] = cw[1:][::-1]
    want = exact(b.reshape(M, 1), None, M, shift=False)[:, 0] / M
    err = np.abs(Bf - want).max() / np.abs(want).max()
    print('nfft %d %s M %d: %.3g u' % (nfft, prec, M, err / U[prec]))
    assert err <= 4 * U[prec]
