"""The stand-alone MTD on the device (k_mtd_any, rsp_mtd.hip): `fftshift(fft(pc .* win, nfft, 1), 1)` for
any pulse count and any transform length, in both precisions, against the exact transform
(tests/_mtd_ref.py: the direct DFT in long double).

The error of a column is ||got - exact||_2 / ||exact||_2 -- a per-element relative error means nothing on
the chirp-z route, whose empty bins carry the column's absolute error -- and its tolerance is C u log2(max(M,
2)), M the transform length `describe_mtd` reports; tests/_mtd_cases.py holds the case table and says where
C comes from (measured on the CPU by tests/test_mtd_ref.py).  Every test asserts through `describe_mtd` that
it runs the route it is there for, and prints each figure before it asserts.

Where np.longdouble is no wider than double (np.finfo(np.longdouble).nmant < 63), `exact` is numpy's
complex128 FFT: good as it is for a complex-single plan; for a complex-double plan the tolerance then gains
numpy's own share, 0.91 u log2 nfft (the largest figure numpy's complex128 FFT showed against a long double
DFT on Gaussian columns of lengths 1 .. 2047).  No case is skipped.

Bit-for-bit properties (no tolerance): the shift, repeatability, maps one by one, a column alone against
the column inside a wider map, device memory against host memory, and nothing written outside the result.
Against the chain: `Plan.mtd` of `process_stage2`'s pc_out agrees with its mtd_out to twice the tolerance
(both approximate the same exact transform) on one scenario per stage-2 route.
"""
import functools

import numpy as np
import pytest

import rsp
from rsp import config as C
from rsp.plan import Plan, describe_mtd
from _mtd_cases import (CASES, CASE_IDS, COLUMN_CASES, PRECS, U, G_MAIN, MAPS_MAIN, tolerance, kaiser32, gaussian,
                        col_err)
from _mtd_ref import exact as _exact_ld, shift_rows, LONGDOUBLE_OK
from _scen import scenario, noisy_cube

pytestmark = pytest.mark.gpu

GUARD = 1 << 12                     # bytes on either side of a guarded device result; a multiple of 256
WORD = np.uint32(0x7FC5A3F1)        # the sentinel: a NaN as a float, and twice over as a double
NUMPY_SHARE = 0.91                  # numpy's complex128 FFT against u log2 nfft (see the module docstring)


def exact(pc, win, nfft, shift=True):
    if LONGDOUBLE_OK:
        return _exact_ld(pc, win, nfft, shift)
    x = np.asarray(pc, np.complex128)
    if win is not None:
        x = x * np.asarray(win, np.float64).reshape((-1,) + (1,) * (x.ndim - 1))
    X = np.fft.fft(x, nfft, axis=0)
    return shift_rows(X, nfft) if shift else X


def tol_for(prec, M, nfft):
    t = tolerance(prec, M)
    if not LONGDOUBLE_OK and prec == 'c128':
        t += NUMPY_SHARE * U[prec] * np.log2(max(nfft, 2))
    return t


@pytest.fixture(scope='module', params=PRECS)
def plan(request):
    s = scenario('plumbing')
    p = Plan(s['cfg'], s['cfar'], s['clus'], s['pre_p'], precision=request.param)
    yield p
    p.close()


@functools.lru_cache(maxsize=None)
def _exact_main(P, nfft):
    return exact(gaussian(P, G_MAIN, MAPS_MAIN), kaiser32(P), nfft)


def _info(plan, P, G, nfft, route=None):
    d = describe_mtd(P, G, nfft, plan.precision)
    want = 'pow2' if nfft & (nfft - 1) == 0 else 'chirpz'
    assert d['route'] == want and (route is None or route == want), d
    return d


def _check(plan, got, want, info, what):
    err = col_err(got, want).max()
    t = tol_for(plan.precision, info['M'], info['nfft'])
    print('%s %s %s M=%d: err %.3g = %.3f u log2 M, tolerance %.3g' % (
        what, plan.precision, info['route'], info['M'], err, err / (U[plan.precision] * np.log2(max(info['M'], 2))), t))
    assert np.isfinite(got).all()
    assert err <= t


@pytest.mark.parametrize('P, nfft', CASES, ids=CASE_IDS)
def test_cases_against_the_exact_transform(plan, P, nfft):
    """Gaussian columns with a Kaiser window, G = 5, n_maps = 2."""
    info = _info(plan, P, G_MAIN, nfft)
    x, win = gaussian(P, G_MAIN, MAPS_MAIN), kaiser32(P)
    got = plan.mtd(x, win, nfft=nfft)
    assert got.shape == (nfft, G_MAIN, MAPS_MAIN)
    _check(plan, got, _exact_main(P, nfft), info, '%d -> %d' % (P, nfft))
    if P == 1:   # every bin = win[0] x[0], and nothing else
        np.testing.assert_array_equal(got, np.broadcast_to(got[:1], got.shape))


@pytest.mark.parametrize('key', sorted(COLUMN_CASES), ids=['%s-%d' % k for k in sorted(COLUMN_CASES)])
def test_column_sweep(plan, key):
    """G = cols - 1, cols, cols + 1, 2 cols + 1 and 1 (cols: the columns of a workgroup), n_maps = 1 and 3.
    Where nfft > 512 at most 24 columns of a run, spread over it, are compared against the exact transform."""
    route, M = key
    P, nfft = COLUMN_CASES[key]
    cols = _info(plan, P, 1, nfft, route)['cols']
    win = kaiser32(P)
    for G in sorted({cols - 1, cols, cols + 1, 2 * cols + 1, 1} - {0}):
        for n_maps in (1, 3):
            info = _info(plan, P, G, nfft, route)
            assert info['M'] == M and info['col_tiles'] == -(-G // cols)
            x = gaussian(P, G, n_maps)
            got = plan.mtd(x, win, nfft=nfft).reshape(nfft, G * n_maps)
            pick = np.arange(G * n_maps)
            if nfft > 512 and len(pick) > 24:
                pick = np.unique(np.linspace(0, G * n_maps - 1, 24).round().astype(int))
            want = exact(x.reshape(P, G * n_maps)[:, pick], win, nfft)
            _check(plan, got[:, pick], want, info, '%d -> %d G=%d maps=%d' % (P, nfft, G, n_maps))


@pytest.mark.parametrize('nfft', [7, 16, 331, 332, 512])
def test_unit_tone(plan, nfft):
    """x[m] = exp(2 pi i k m / nfft), P = nfft, no window: the peak is nfft at row (k + floor(nfft / 2)) mod
    nfft.  The column's norm is the peak's, so the peak is off by no more than the column's tolerance times
    nfft, and by as much again for the rounding of the tone itself to the plan's precision (u nfft at worst)."""
    info = _info(plan, nfft, 2, nfft)
    pi = np.longdouble('3.141592653589793238462643383279502884')
    m = np.arange(nfft, dtype=np.int64)
    ks = (1, nfft // 3 + 1)
    ang = [2 * pi * ((k * m) % nfft).astype(np.longdouble) / nfft for k in ks]
    x = np.stack([np.cos(a) + 1j * np.sin(a) for a in ang], axis=1).astype(plan.cdtype)   # what the device holds
    got = plan.mtd(x, None, nfft=nfft)
    _check(plan, got, exact(x, None, nfft), info, 'tone, nfft %d' % nfft)
    t = tol_for(plan.precision, info['M'], nfft)
    for j, k in enumerate(ks):
        row = (k + nfft // 2) % nfft
        print('k=%d: peak at row %d, |peak - nfft| / nfft = %.3g' % (k, int(np.argmax(np.abs(got[:, j]))),
                                                                     abs(got[row, j] - nfft) / nfft))
        assert int(np.argmax(np.abs(got[:, j]))) == row
        assert abs(got[row, j] - nfft) <= 2 * t * nfft


@pytest.mark.parametrize('P, nfft', [(332, 332), (332, 512)])
def test_tone_above_noise(plan, P, nfft):
    """One column: a tone 120 dB (complex double) or 50 dB (complex single) above Gaussian noise."""
    info = _info(plan, P, 1, nfft)
    db = 120.0 if plan.precision == 'c128' else 50.0
    m = np.arange(P)
    x = (10 ** (db / 20) * np.exp(2j * np.pi * 0.1234 * m))[:, None] + gaussian(P, 1, 1, seed=4)[:, :, 0]
    x = x.astype(plan.cdtype)
    win = kaiser32(P)
    _check(plan, plan.mtd(x, win, nfft=nfft), exact(x, win, nfft), info, 'tone %g dB above noise, %d -> %d' % (db, P, nfft))


# ---- bit-for-bit properties -----------------------------------------------------------------------
BIT_CASES = [(15, 15), (5, 7), (100, 128), (331, 331), (332, 333), (332, 512), (333, 666)]


@pytest.mark.parametrize('P, nfft', BIT_CASES, ids=['%d-%d' % c for c in BIT_CASES])
def test_bit_for_bit_properties(plan, P, nfft):
    cols = _info(plan, P, 1, nfft)['cols']
    G = 2 * cols + 1
    x, win = gaussian(P, G, 3, seed=2), kaiser32(P)
    a = plan.mtd(x, win, nfft=nfft)
    # the same call twice
    np.testing.assert_array_equal(plan.mtd(x, win, nfft=nfft), a)
    # natural order is the shift undone
    np.testing.assert_array_equal(plan.mtd(x, win, nfft=nfft, shift=False), np.fft.ifftshift(a, axes=0))
    # three maps are three single-map calls
    for b in range(3):
        np.testing.assert_array_equal(plan.mtd(x[:, :, b], win, nfft=nfft), a[:, :, b])
    # a column does not depend on G or on its position in the map
    for j in sorted({0, cols - 1, cols, G - 1}):
        np.testing.assert_array_equal(plan.mtd(x[:, j:j + 1, 1], win, nfft=nfft)[:, 0], a[:, j, 1])
    # the window is applied: without it the result differs
    assert P == 1 or not np.array_equal(plan.mtd(x, None, nfft=nfft), a)


@pytest.mark.parametrize('P, nfft', [(5, 7), (332, 333), (332, 512), (331, 662)])
def test_device_memory_and_guard_bands(plan, P, nfft):
    """mtd_device on uploaded data equals mtd, and writes nothing outside [nfft x G x n_maps]: the result
    lies between two guard bands of sentinel words.  A second run starts one element further on, where a
    complex-single result is no longer 16-byte aligned (the one-element form of the stores)."""
    _info(plan, P, 1, nfft)
    esz = np.dtype(plan.cdtype).itemsize
    G, n_maps = 5, 2
    x, win = gaussian(P, G, n_maps, seed=3), kaiser32(P)
    want = plan.mtd(x, win, nfft=nfft)
    n_in, n_out = P * G * n_maps, nfft * G * n_maps
    d_in = plan.device_alloc((n_in + 1) * esz)
    d_out = plan.device_alloc(2 * GUARD + (n_out + 1) * esz)
    try:
        for off in (0, 1):   # elements
            total = (2 * GUARD + (n_out + 1) * esz) // 4
            plan.device_upload(d_out, np.full(total, WORD, np.uint32))
            plan.device_upload(d_in + off * esz, x.astype(plan.cdtype).ravel(order='F'))
            plan.mtd_device(d_in + off * esz, d_out + GUARD + off * esz, P, G, n_maps, win=win, nfft=nfft)
            w = plan.device_download(d_out, total, np.uint32)
            lo, hi = GUARD // 4 + off * esz // 4, GUARD // 4 + (off + n_out) * esz // 4
            assert (w[:lo] == WORD).all(), 'a store below the result: words %r' % (np.flatnonzero(w[:lo] != WORD)[:8],)
            assert (w[hi:] == WORD).all(), 'a store above the result: words %r' % (hi + np.flatnonzero(w[hi:] != WORD)[:8],)
            got = w[lo:hi].view(plan.cdtype).astype(np.complex128).reshape((nfft, G, n_maps), order='F')
            np.testing.assert_array_equal(got, want)
        with pytest.raises(rsp.RspError):   # overlapping input and output
            plan.mtd_device(d_in, d_in, P, G, n_maps, win=win, nfft=nfft)
    finally:
        plan.device_free(d_in)
        plan.device_free(d_out)


def test_input_dtype_and_arguments(plan):
    """complex64 into a complex-double plan (exact) and complex128 into a complex-single plan (narrowed);
    a window of the wrong length, a C-ordered `out` and nfft < P are refused."""
    P, nfft = 83, 96
    x, win = gaussian(P, 4, 1, seed=6), kaiser32(P)
    a = plan.mtd(x, win, nfft=nfft)
    np.testing.assert_array_equal(plan.mtd(x.astype(np.complex64), win, nfft=nfft), a)   # the parts are single-precision numbers
    out = np.empty((nfft, 4, 1), np.complex128, order='F')
    assert plan.mtd(x, win, nfft=nfft, out=out) is out
    np.testing.assert_array_equal(out, a)
    np.testing.assert_array_equal(plan.mtd(x[:, :, 0], win, nfft=nfft), a[:, :, 0])      # [P, G]
    with pytest.raises(ValueError):
        plan.mtd(x, win[:-1], nfft=nfft)
    with pytest.raises(ValueError):
        plan.mtd(x, win, nfft=nfft, out=np.empty((nfft, 4, 1), np.complex128))
    with pytest.raises(rsp.RspError):
        plan.mtd(x, win, nfft=P - 1)
    with pytest.raises(rsp.RspError):
        plan.mtd(x, win, nfft=2049)


def test_profile_mtd(plan):
    esz = 16 if plan.precision == 'c128' else 8
    for P, G, n_maps, nfft in ((83, 33, 2, 96), (100, 17, 3, 128)):
        r = plan.profile_mtd(P, G, n_maps, nfft, iters=3)
        assert r['stage'] == 'k_mtd_any' and r['ms'] > 0
        assert r['bytes'] == esz * G * n_maps * (P + nfft)


# ---- against the chain ----------------------------------------------------------------------------
@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('name', ['s-16s', 'f-166-b4', 'd-96'])
def test_against_the_stage2_mtd(name, prec):
    """`Plan.mtd(pc_out, MTD_win)` of `process_stage2`'s pc_out against its mtd_out (k_mtd_cols: Stockham at
    's-16s', the direct DFT at the other two): twice the tolerance, both approximate the same transform."""
    s = scenario(name)
    plan = Plan(s['cfg'], s['cfar'], s['clus'], s['pre_p'], precision=prec)
    try:
        rng = np.random.default_rng(11)
        iq = (rng.standard_normal((2, plan.P, plan.N, plan.B)).astype(np.float32))
        mtd, pc = plan.process_stage2(iq[0] + 1j * iq[1])
        win = np.asarray(s['pre_p']['MTD_win'], np.float64).ravel()
        info = describe_mtd(plan.P, plan.G, None, prec)
        assert info['route'] == ('pow2' if name == 's-16s' else 'chirpz')
        got = plan.mtd(pc, win)
    finally:
        plan.close()
    err = col_err(got, mtd).max()
    t = 2 * tolerance(prec, info['M'])
    print('%s %s P=%d %s M=%d: err %.3g, twice the tolerance %.3g, bit-equal: %s' % (
        name, prec, info['P'], info['route'], info['M'], err, t, np.array_equal(got, mtd)))
    assert err <= t


# ---- end to end -----------------------------------------------------------------------------------
def test_target_velocity_end_to_end():
    """One target on a plumbing frame: the raw-cube stage 2 up to the pulse compression, `mtd_doppler` with
    nfft = 2 P, `local_cfar_detector` on its modulus; the strongest hit lies within one row of the row
    `mtd_velocity_axis` gives for the target's velocity."""
    s = scenario('d-96')
    sc = s['cfg']['Sig_Config']
    P, nfft = sc['prtNum'], 2 * sc['prtNum']
    v_max = sc['wavelength'] / (2 * sc['prt'])
    rmax = sum(sc['point_prt_segments']) * sc['c'] / (2 * sc['fs'])
    ang = C.V8_BEAM_ANGLES[1]
    tg = dict(Range=0.45 * rmax, Velocity=0.2 * v_max, ElevationAngle=ang, SNR_dB=20.0)
    cube = noisy_cube(s, [tg], dtype=np.complex128)
    plan = Plan(s['cfg'], s['cfar'], s['clus'], s['pre_p'])
    try:
        _, pc = plan.process_raw_stage2(cube)
    finally:
        plan.close()
    assert describe_mtd(P, pc.shape[1], nfft)['route'] == 'chirpz'
    rdm = rsp.mtd_doppler(pc[:, :, 1], s['pre_p']['MTD_win'], nfft=nfft)
    assert rdm.shape == (nfft, pc.shape[1])
    det, thr = rsp.local_cfar_detector(np.abs(rdm), C.v3_cfar_params())
    assert det.any()
    amp = np.where(det, np.abs(rdm), 0.0)
    row = int(np.unravel_index(np.argmax(amp), amp.shape)[0])
    axis = rsp.mtd_velocity_axis(v_max, nfft)
    want = int(np.argmin(np.abs(axis - tg['Velocity'])))
    print('strongest hit at row %d (%.3f m/s), the axis puts %.3f m/s at row %d' % (row, axis[row], tg['Velocity'], want))
    assert abs(row - want) <= 1
