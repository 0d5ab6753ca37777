"""Planar-array MUSIC over the plan's envelope: array shapes, scan grids, batches and plateaus.

tests/test_music2d.py pins the 2-D path (k_music_sub64, k_music_scan2d, k_music_peaks2d, the planar
synthesis, music_table for planar plans) at seven cases: nx, ny >= 3 and N <= 25 (plus the 8 x 8
literal), batches of 4 (2), grids of 17 x 33, 18 x 34 and 91 x 181, dx = dy = lambda / 2 and one
two-pixel plateau.  This file walks the same path through the cases of tests/_music2d_shapes.py,
against the numpy restatement tests/_music2d_ref.py on the snapshots the device itself synthesised
(seed 20250101, instances 0 .. n-1, complex unit sources, awgn 10 dB 'measured', the asymmetric grid
G(nt, np): phi = linspace(-77, 80, np) deg, theta = linspace(2, 80, nt) deg):

  * array   line arrays inside the planar path (nx = 1, ny = 1), N = 2, N = 64 as 64 x 1, 2 x 32 and
            32 x 2, N = 63, M = 8 = MU_MMAX, M = N - 1, K < N, K = 1, K % 4 = 1, dx != dy;
  * batch   n = 1, 3, 5, 6 and n = 5 in a plan of 8: k_music_scan2d's partly filled groups of
            M2_IB = 4 instances; every instance bit-equal to the same instance of the n = 6 run;
  * grid    S = 9, 255, 256, 259 and 65 536 = M2_SMAX, columns of 31, 32 and 33 pixels, axes of 3
            and 1024, three 512 KB maps in flight;
  * plateau repeated grid angles: plateaus that k_music_peaks2d must drop pass by pass (70 passes
            on p-runs, 12 on p-stair), that span mask words, owner lanes and ballot rounds, whole
            rows, whole columns and the whole map;
  * few     fewer regional maxima than M: the `0 = none` peak slots and the NaN angles.

Tolerances are test_music2d.py's (imported): X 1e-12, R 1e-12, eigenvalues 1e-11 of the largest,
spectrum 1e-7 dB wherever the reference is above -60 dB (the whole map in every case here, which
test_music2d_shape_cases.py asserts on the CPU).  Peaks, n_peaks, rows, columns and angles are
compared exactly, after two preconditions on the reference's unique-grid map alone
(_music2d_shapes.check_preconditions): every pixel differs from its largest in-bounds neighbour by
>= 5e-7 dB, and the min(M, n_peaks) + 1 highest regional maxima differ pairwise by at least as
much.  A failed precondition fails the test.

Measured on an MI355X: spectrum error at most 6.7e-13 dB (a3x3-m8; 4.1e-13 on a64x1, below 1e-13
on every grid, plateau and batch case, 0 on the constant maps); every instance of every M <= 4 case
took the block-power fast path in the peaks-only call (printed, not asserted).
"""
import numpy as np
import pytest

import _music2d_shapes as m2s
from _music2d_shapes import CASES, CASE_IDS, SEED
from test_music2d import TOL

pytestmark = pytest.mark.gpu

KEYS = ('spectrum_db', 'eig', 'R', 'peaks', 'n_peaks', 'peak_rows', 'peak_cols', 'phi_e_deg', 'theta_e_deg')


def _run(c):
    """The device flow of test_music2d.py's fixture on a fresh plan: (plan, d_X, X, out, fast count
    after the full call).  The caller frees d_X and closes the plan."""
    from rsp.music import MusicPlan2D
    phi, theta = m2s.plan_grid(c)
    plan = MusicPlan2D(c['nx'], c['ny'], c['K'], c['M'], phi, theta, c['dxl'], c['dyl'], max_batch=c['max_batch'])
    d_X = None
    try:
        d_X = plan.device_alloc(c['n'])
        plan.synthesize_device(d_X, m2s.scene_for(c['M']), c['n'], inst0=0, seed=SEED)
        X = plan.download(d_X, c['n'])
        out = plan.process_device(d_X, c['n'], want_cov=True)
        return plan, d_X, X, out, plan.fast_count()
    except Exception:
        if d_X is not None:
            plan.device_free(d_X)
        plan.close()
        raise


@pytest.fixture(scope='module', params=CASE_IDS, ids=CASE_IDS)
def case(request):
    """One plan per case: the device outputs, the reference on the downloaded snapshots (unique
    grid) and what the plan's grid must give, computed once and shared by the tests below."""
    name = request.param
    c = dict(CASES[name], name=name)
    plan, d_X, X, out, fast = _run(c)
    try:
        phi, theta = m2s.plan_grid(c)
        rf = [m2s.reference(c, X[i]) for i in range(c['n'])]
        c.update(plan=plan, d_X=d_X, X=X, out=out, fast_after_full=fast, phi=phi, theta=theta, ref=rf,
                 want=[m2s.expected(c, r) for r in rf])
        yield c
    finally:
        plan.device_free(d_X)
        plan.close()


def test_shape_synthesis_matches_reference(case):
    c = case
    for i in range(c['n']):
        x = m2s.snapshots(c, i)
        assert c['X'][i].shape == x.shape == (c['nx'] * c['ny'], c['K'])
        err = np.abs(c['X'][i] - x).max() / np.abs(x).max()
        print('%s[%d]: X err %.2e' % (c['name'], i, err))
        assert err <= TOL['X']


def test_shape_covariance_and_eigenvalues(case):
    c = case
    N = c['nx'] * c['ny']
    assert c['out']['eig'].shape == (c['n'], N) and c['out']['R'].shape == (c['n'], N, N)
    for i in range(c['n']):
        R, d = c['ref'][i]['R'], c['ref'][i]['eig']
        er = np.abs(c['out']['R'][i] - R).max() / np.abs(R).max()
        ee = np.abs(c['out']['eig'][i] - d).max() / d.max()
        print('%s[%d]: R err %.2e eig err %.2e' % (c['name'], i, er, ee))
        assert er <= TOL['R']
        assert ee <= TOL['eig']


def test_shape_spectrum(case):
    c = case
    nt, npn = len(c['theta']), len(c['phi'])
    assert c['out']['spectrum_db'].shape == (c['n'], nt, npn)
    for i in range(c['n']):
        want, mask, peaks, n_peaks = c['want'][i]
        got = c['out']['spectrum_db'][i]
        live = want > -60.0
        top = peaks[peaks > 0] - 1
        assert live.any() and live.flatten(order='F')[top].all()
        err = np.abs(got[live] - want[live]).max()
        print('%s[%d]: spectrum err %.3e dB over %d of %d pixels' % (c['name'], i, err, live.sum(), live.size))
        assert err <= TOL['db']
        assert got.max() == 0.0


def _assert_plateaus(c):
    """A grid point's value depends only on its (theta, phi) and the instance: every repeat of a
    row or column equals its first occurrence bit for bit, so the plateaus are exact."""
    tm, pm = m2s.repeat_maps(c)
    tfirst = np.concatenate([[0], np.cumsum(c['rt'])[:-1]])[tm]
    pfirst = np.concatenate([[0], np.cumsum(c['rp'])[:-1]])[pm]
    sp = c['out']['spectrum_db']
    assert (tfirst != np.arange(len(tm))).any() or (pfirst != np.arange(len(pm))).any()
    assert np.array_equal(sp, sp[:, tfirst][:, :, pfirst])
    if c['name'] in ('p-const3', 'p-const'):   # the whole map one plateau
        assert (sp == 0.0).all()
        assert (c['out']['n_peaks'] == sp[0].size).all()
        assert (c['out']['peaks'] == [1, 2]).all()


def test_shape_peaks(case):
    c = case
    nt, M = len(c['theta']), c['M']
    o = c['out']
    assert o['peaks'].shape == (c['n'], M)
    for i in range(c['n']):
        r = c['ref'][i]
        m2s.check_preconditions(r['spectrum_db'], r['mask'], M, '%s[%d]' % (c['name'], i))
        want, mask, peaks, n_peaks = c['want'][i]
        k = min(M, n_peaks)
        top = peaks[:k] - 1
        print('%s[%d]: n_peaks %d, peaks %s' % (c['name'], i, o['n_peaks'][i], list(o['peaks'][i])))
        assert list(o['peaks'][i][:k]) == list(peaks[:k])
        assert o['n_peaks'][i] == n_peaks
        assert list(o['peak_rows'][i][:k]) == list(top % nt + 1)
        assert list(o['peak_cols'][i][:k]) == list(top // nt + 1)
        assert np.array_equal(o['phi_e_deg'][i][:k], np.rad2deg(c['phi'][top // nt]))
        assert np.array_equal(o['theta_e_deg'][i][:k], np.rad2deg(c['theta'][top % nt]))
        # fewer regional maxima than M: 0 = none in the remaining slots, NaN angles
        assert (o['peaks'][i][k:] == 0).all()
        assert (o['peak_rows'][i][k:] == 0).all() and (o['peak_cols'][i][k:] == 0).all()
        assert np.isnan(o['phi_e_deg'][i][k:]).all() and np.isnan(o['theta_e_deg'][i][k:]).all()
    if c['kind'] == 'few':
        assert (o['n_peaks'] < M).all()
    if c['kind'] == 'plateau':
        _assert_plateaus(c)


def test_shape_forms_of_call(case):
    c = case
    plan, n, M = c['plan'], c['n'], c['M']
    # the fixture's call read the spectrum and the eigenvalues: the full eigensolver
    assert c['fast_after_full'] == 0
    pk, npk = np.zeros((n, M), np.int32), np.zeros(n, np.int32)
    plan.peaks_device(c['d_X'], n, pk, npk)                  # peaks only
    fast = plan.fast_count()
    print('%s: fast count after the peaks-only call %d of %d (M = %d)' % (c['name'], fast, n, M))
    assert np.array_equal(pk, c['out']['peaks']) and np.array_equal(npk, c['out']['n_peaks'])
    assert 0 <= fast <= n
    if M > 4:
        assert fast == 0
    S = len(c['phi']) * len(c['theta'])
    spec = np.zeros((n, S), np.float64)
    pk[:], npk[:] = -1, -1
    plan.spectrum_device(c['d_X'], n, spec, pk, npk)          # spectrum without the eigenvalues
    assert plan.fast_count() == 0
    full = c['out']['spectrum_db']
    spec = spec.reshape(n, len(c['phi']), len(c['theta'])).transpose(0, 2, 1)
    assert np.abs(spec - full)[full > -60.0].max() <= TOL['db']
    assert np.array_equal(pk, c['out']['peaks']) and np.array_equal(npk, c['out']['n_peaks'])
    # rsp_music_process on host X == the device-resident path, and a second run == the first
    host = plan.process(c['X'], want_cov=True)
    assert plan.fast_count() == 0
    again = plan.process_device(c['d_X'], n, want_cov=True)
    assert plan.fast_count() == 0
    for o in (host, again):
        for k in KEYS:
            assert np.array_equal(o[k], c['out'][k], equal_nan=k.endswith('_deg')), k
    hp, hn = plan.peaks(c['X'])
    assert np.array_equal(hp, c['out']['peaks']) and np.array_equal(hn, c['out']['n_peaks'])


def test_batch_instances_do_not_depend_on_group_or_batch():
    """Every instance of every batch case (n = 1, 3, 5, 6, and n = 5 in a plan of 8) gives, bit for
    bit, what the same instance gives in the n = 6 run: k_music_scan2d's guards on a partly filled
    group of four neither change a stored value nor store past n_inst."""
    runs = {}
    for name, c in m2s.BATCH_CASES.items():
        plan, d_X, X, out, _ = _run(c)
        try:
            pk, npk = np.zeros((c['n'], c['M']), np.int32), np.zeros(c['n'], np.int32)
            plan.peaks_device(d_X, c['n'], pk, npk)
            runs[name] = dict(out, X=X, pk_only=pk, npk_only=npk)
        finally:
            plan.device_free(d_X)
            plan.close()
    full = runs[m2s.BATCH_FULL]
    for name, c in m2s.BATCH_CASES.items():
        n = c['n']
        for k in KEYS + ('X',):
            assert runs[name][k].shape[0] == n
            assert np.array_equal(runs[name][k], full[k][:n]), (name, k)
        assert np.array_equal(runs[name]['pk_only'], full['peaks'][:n]), name
        assert np.array_equal(runs[name]['npk_only'], full['n_peaks'][:n]), name
