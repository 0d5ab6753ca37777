"""Known answers for tests/_ddc_ref.py, the numpy restatement tests/test_ddc.py holds k_ddc against (CPU): the
NCO at the words whose values are exact, wrap-around of the phase, the filter and decimator against
numpy.convolve, rsp_ddc_phase_word against exact fractions, and the restatement against the three lines of
simulation_learn.m (:79, :95, :102) as MATLAB evaluates them, with FIR.mat's taps."""
import ctypes as ct
import os
from fractions import Fraction

import numpy as np
import pytest

import _ddc_ref as R
import rsp
from rsp import _abi, matio

HERE = os.path.dirname(os.path.abspath(__file__))
FIR = os.path.join(HERE, 'golden', 'ref_mat', 'FIR.mat')


def _num():
    return np.asarray(matio.load(FIR)['Num'], np.float64).ravel()


def test_fir_mat_holds_the_twelve_taps():
    assert _num().size == 12


@pytest.mark.parametrize('D, off', [(1, 0), (4, 0), (4, 3), (7, 6), (64, 63)])
def test_zero_word_is_filter_and_downsample(D, off):
    """w = 0, w0 = 0: m = 1, so y = downsample(filter(h, 1, x), D, off), the first N of the convolution."""
    rng = np.random.default_rng(1)
    x, h = rng.standard_normal(301), rng.standard_normal(13)
    yr, yi, b = R.ddc_ref(x, h, D, 0, 0, 'iq', off)
    want = np.convolve(x, h)[:x.size][off::D]
    assert yr.shape == (1, want.size, 1) and want.size == -(-(x.size - off) // D)
    assert np.abs(yr.ravel().astype(np.float64) - want).max() <= 16 * 2.0 ** -53 * float(b.max())
    assert not yi.any()
    assert np.allclose(b.ravel().astype(np.float64), np.convolve(np.abs(x), np.abs(h))[:x.size][off::D], rtol=1e-14)


def test_quarter_rate_word_is_exact():
    """w = 2^62 (fs / 4): m = 1, -i, -1, i, ... exactly, in both modes' parts."""
    mr, mi = R.nco(8, 2 ** 62, 0, 'iq')
    assert mr.tolist() == [1, 0, -1, 0, 1, 0, -1, 0] and mi.tolist() == [0, -1, 0, 1, 0, -1, 0, 1]
    sr, si = R.nco(8, 2 ** 62, 0, 'sin')
    assert sr.tolist() == [0, 1, 0, -1, 0, 1, 0, -1] and not si.any()
    x = np.arange(1.0, 9.0)
    yr, yi, _ = R.ddc_ref(x, [1.0], 1, 2 ** 62)
    assert yr.ravel().tolist() == [1, 0, -3, 0, 5, 0, -7, 0] and yi.ravel().tolist() == [0, -2, 0, 4, 0, -6, 0, 8]


def test_half_rate_word_alternates():
    mr, mi = R.nco(6, 2 ** 63, 0, 'iq')
    assert mr.tolist() == [1, -1, 1, -1, 1, -1] and not mi.any()
    mr, mi = R.nco(4, 2 ** 63, 2 ** 62, 'iq')   # a start phase of a quarter turn
    assert mr.tolist() == [0, 0, 0, 0] and mi.tolist() == [-1, 1, -1, 1]


def test_phase_wraps_modulo_two_to_the_64():
    """n w passes 2^64: the phase is what is left, so w = 2^64 - 2^62 (-fs / 4) runs the quarter turns backwards,
    and a word just below 2^63 drifts by 2^11 n, one unit of u per sample."""
    w = 2 ** 64 - 2 ** 62
    mr, mi = R.nco(5, w, 0, 'iq')
    assert mr.tolist() == [1, 0, -1, 0, 1] and mi.tolist() == [0, 1, 0, -1, 0]
    w = 2 ** 63 - 2 ** 11
    u = R.nco_u(5, w)
    assert u.tolist() == [0.0, 0.5 - 2.0 ** -53, 1.0 - 2 * 2.0 ** -53, 0.5 - 3 * 2.0 ** -53, 1.0 - 4 * 2.0 ** -53]
    assert (R.nco_u(4, 1, 2 ** 64 - 1) == [(2 ** 53 - 1) * 2.0 ** -53, 0.0, 0.0, 0.0]).all()   # w0 + w = 2^64: 0


@pytest.mark.parametrize('f0, fs', [(10e6, 100e6), (3.0, 8.0), (25e6, 100e6), (-10e6, 100e6), (0.0, 1.0), (70e6, 100e6)])
def test_phase_word_against_fractions(f0, fs):
    """Ratios whose 64-bit word the long double evaluation cannot miss: the exact value is an integer, or lies
    further from a half than a 64-bit mantissa resolves there (1/3 would be rounded twice, first to 64 bits --
    to a half -- and then to the integer)."""
    w = ct.c_uint64()
    assert _abi.lib().rsp_ddc_phase_word(f0, fs, ct.byref(w)) == _abi.RSP_OK
    assert w.value == R.phase_word(f0, fs) == rsp.ddc_phase_word(f0, fs)
    if (f0, fs) == (10e6, 100e6):
        assert w.value == int(round(Fraction(2 ** 64, 10))) == 1844674407370955162


def test_phase_word_refusals():
    w = ct.c_uint64()
    lib = _abi.lib()
    for f0, fs in ((float('nan'), 1.0), (1.0, float('inf')), (float('inf'), 1.0), (1.0, 0.0), (1.0, -2.0)):
        assert lib.rsp_ddc_phase_word(f0, fs, ct.byref(w)) == _abi.RSP_ERR_INVALID
    assert lib.rsp_ddc_phase_word(1.0, 2.0, None) == _abi.RSP_ERR_INVALID


def test_restatement_against_the_matlab_form():
    """simulation_learn.m:79-102 on a 2 000-sample cut of its LFM echo with FIR.mat's Num: the 64-bit NCO at
    phase_word(f, fs) in 'sin' mode against sin(2*pi*f*t2) in doubles, within b (3 u theta_max + (L + 6) u)."""
    xt, f, fs = R.lfm_cut()
    Num = _num()
    want = R.matlab_form(xt, f, fs, Num, 4)
    yr, yi, b = R.ddc_ref(xt, Num, 4, R.phase_word(f, fs), 0, 'sin')
    tol = R.matlab_allowance(xt, f, fs, Num, 4)
    err = np.abs(yr.ravel().astype(np.float64) - want)
    print('matlab form: max |y| %.3g, max err %.3g, least allowance %.3g' % (np.abs(want).max(), err.max(), tol.min()))
    assert want.size == 500 and np.abs(want).max() > 0.1
    assert (err <= tol).all()
    assert not yi.any()
    assert np.allclose(b.ravel().astype(np.float64), np.convolve(np.abs(xt), np.abs(Num))[:xt.size][::4], rtol=1e-14)
