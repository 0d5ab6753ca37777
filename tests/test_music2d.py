"""2-D MUSIC for planar arrays (MUSIC_2D.m) on the device against the numpy restatement
tests/_music2d_ref.py, on identical snapshots (synthesised on the device, downloaded, fed to the
reference).  Complex double; the tolerances are tests/test_music.py's for c128:

  * synthesis:   max |X_dev - X_ref| <= 1e-12 * max |X_ref|;
  * covariance:  max |R_dev - R| <= 1e-12 * max |R|;
  * eigenvalues: max |d_dev - d| <= 1e-11 * max d;
  * spectrum:    |dB_dev - dB| <= 1e-7 dB wherever the reference is above -60 dB (a set that must
                 be non-empty and hold the M top pixels);
  * peaks:       the same M linear indices in the same order and the same imregionalmax pixel
                 count -- exactly.  Exactness is asserted only after a precondition on the reference
                 map alone: no pixel equals its largest neighbour, and every pixel differs from its
                 largest neighbour by >= 1e-5 dB (100 x the spectrum tolerance), so that no
                 regional-maximum decision can flip within the tolerance; and the M + 1 highest
                 regional maxima differ pairwise by as much, so that neither can the top-M order.

The reference (Q_n form, LAPACK eigenvectors) is computed once per case in a module fixture.
"""
import ctypes as ct

import numpy as np
import pytest

import _music2d_ref as ref
from _music2d_shapes import height_gap

SEED = 20250101
TOL = dict(X=1e-12, R=1e-12, eig=1e-11, db=1e-7)
MARGIN_DB = 1e-5

PHI = np.deg2rad(np.linspace(-80.0, 80.0, 33))
THETA = np.deg2rad(np.linspace(0.0, 80.0, 17))
SRC = [(30.0, 20.0), (-60.0, 45.0), (0.0, 60.0), (-20.0, 10.0), (60.0, 70.0)]   # (phi, theta) deg
# the `dup` grid: phi = 30 deg (index 22) and theta = 45 deg (index 9) each listed twice, adjacent
PHI_MAP = np.concatenate([np.arange(23), np.arange(22, 33)])
THETA_MAP = np.concatenate([np.arange(10), np.arange(9, 17)])

#        id            nx ny  K     M  snr   n_inst
CASES = {'ura44': (4, 4, 64, 2, 10.0, 4),
         'ura35': (3, 5, 48, 2, 10.0, 4),          # N = 15: not a multiple of 4; nx != ny
         'ura53-m3': (5, 3, 48, 3, 10.0, 4),
         'ura55-m5': (5, 5, 128, 5, 10.0, 4),      # M > 4: no fast-path instantiation
         'ura44-snr70': (4, 4, 64, 2, 70.0, 4),    # den_min ~ 3e-8
         'dup': (4, 4, 64, 2, 10.0, 4),
         'literal': (8, 8, 1000, 2, 10.0, 2)}      # MUSIC_2D.m itself: 91 x 181 = 16 471 points


def _scene(M, snr):
    return {'azim_rad': np.deg2rad([s[0] for s in SRC[:M]]), 'elev_rad': np.deg2rad([s[1] for s in SRC[:M]]),
            'amplitudes': np.ones(M), 'complex_sources': 1, 'snr_db': snr, 'snr_measured': 1}


@pytest.fixture(scope='module', params=list(CASES), ids=list(CASES))
def case(request):
    from rsp.music import MusicPlan2D, music_2d_scene
    name = request.param
    nx, ny, K, M, snr, n = CASES[name]
    dxl = dyl = 0.5
    phi_u, theta_u = PHI, THETA                     # the grid the reference scans
    if name == 'literal':
        scene, phi_u, theta_u, dxl, dyl = music_2d_scene()
    else:
        scene = _scene(M, snr)
    phi, theta = (phi_u[PHI_MAP], theta_u[THETA_MAP]) if name == 'dup' else (phi_u, theta_u)
    plan = MusicPlan2D(nx, ny, K, M, phi, theta, dxl, dyl, max_batch=n)
    d_X = plan.device_alloc(n)
    plan.synthesize_device(d_X, scene, n, inst0=0, seed=SEED)
    X = plan.download(d_X, n)
    out = plan.process_device(d_X, n, want_cov=True)
    fast_after_full = plan.fast_count()
    rf = [ref.music_2d(X[i], M, nx, ny, phi_u, theta_u, dxl, dyl) for i in range(n)]
    yield dict(name=name, nx=nx, ny=ny, K=K, M=M, n=n, scene=scene, dxl=dxl, dyl=dyl, phi=phi, theta=theta,
               plan=plan, d_X=d_X, X=X, out=out, ref=rf, fast_after_full=fast_after_full)
    plan.device_free(d_X)
    plan.close()


def _expected_map(c, i):
    """The reference map on the plan's grid (for `dup`: the unique-grid map indexed by the
    duplicated grid)."""
    m = c['ref'][i]['spectrum_db']
    return m[THETA_MAP][:, PHI_MAP] if c['name'] == 'dup' else m


def _assert_margin(m, where, mask, M):
    """The preconditions of every exact peak comparison, on a reference map alone: the pixel-to-
    neighbour margin (the set of regional maxima) and the gap between the heights of the M + 1
    highest maxima (which of them are the top M, and in what order)."""
    gap = np.abs(m - ref.largest_neighbour(m))
    print('%s: min |P_dB - largest neighbour| = %.3e dB' % (where, gap.min()))
    assert gap.min() > 0.0, '%s: a pixel equals its largest neighbour' % where
    assert gap.min() >= MARGIN_DB, '%s: margin %.3e dB' % (where, gap.min())
    hg = height_gap(m, mask, M)
    print('%s: min gap between the %d highest regional maxima = %.3e dB' % (where, min(M, mask.sum()) + 1, hg))
    assert hg >= MARGIN_DB, '%s: height gap %.3e dB' % (where, hg)


@pytest.mark.gpu
def test_synthesis_matches_reference(case):
    c = case
    for i in range(c['n']):
        x = ref.synthesize_2d(c['scene'], c['nx'], c['ny'], c['K'], c['dxl'], c['dyl'], i, SEED)
        assert c['X'][i].shape == x.shape
        assert np.abs(c['X'][i] - x).max() <= TOL['X'] * np.abs(x).max()


@pytest.mark.gpu
def test_covariance_and_eigenvalues(case):
    c = case
    for i in range(c['n']):
        R, d = c['ref'][i]['R'], c['ref'][i]['eig']
        assert np.abs(c['out']['R'][i] - R).max() <= TOL['R'] * np.abs(R).max()
        assert np.abs(c['out']['eig'][i] - d).max() <= TOL['eig'] * d.max()


@pytest.mark.gpu
def test_spectrum(case):
    c = case
    nt, npn = len(c['theta']), len(c['phi'])
    assert c['out']['spectrum_db'].shape == (c['n'], nt, npn)
    for i in range(c['n']):
        want = _expected_map(c, i)
        got = c['out']['spectrum_db'][i]
        live = want > -60.0
        top = ref.top_peaks(want, ref.regional_max(want), c['M'])
        assert live.any() and live.flatten(order='F')[top].all()
        err = np.abs(got[live] - want[live]).max()
        print('%s[%d]: spectrum err %.3e dB over %d pixels' % (c['name'], i, err, live.sum()))
        assert err <= TOL['db']
        assert got.max() == 0.0


@pytest.mark.gpu
def test_peaks(case):
    c = case
    nt, M = len(c['theta']), c['M']
    for i in range(c['n']):
        got = c['out']['peaks'][i]
        if c['name'] == 'literal':
            # the count is ill-conditioned in the reference itself (theta = 90 deg: cos(theta) ~ 6e-17,
            # the whole row is a rounding-level plateau): only the top M and a lower bound
            assert list(got) == list(c['ref'][i]['peaks'])
            ang = sorted(zip(np.round(c['out']['phi_e_deg'][i], 9), np.round(c['out']['theta_e_deg'][i], 9)))
            assert ang == [(-60.0, 45.0), (30.0, 20.0)]
            assert c['out']['n_peaks'][i] >= M
            continue
        _assert_margin(c['ref'][i]['spectrum_db'], '%s[%d]' % (c['name'], i), c['ref'][i]['mask'], M)
        want = _expected_map(c, i)
        mask = ref.regional_max(want)
        top = ref.top_peaks(want, mask, M)
        assert list(got) == list(top + 1)
        assert c['out']['n_peaks'][i] == int(mask.sum())
        assert list(c['out']['peak_rows'][i]) == list(top % nt + 1)
        assert list(c['out']['peak_cols'][i]) == list(top // nt + 1)
        assert np.array_equal(c['out']['phi_e_deg'][i], np.rad2deg(c['phi'][top // nt]))
        assert np.array_equal(c['out']['theta_e_deg'][i], np.rad2deg(c['theta'][top % nt]))
    if c['name'] == 'dup':
        _assert_dup_plateaus(c)


def _assert_dup_plateaus(c):
    """`dup`: a grid point's value depends only on its (theta, phi) and the instance, so the
    duplicated row and column equal their twins bit for bit, and the strongest peak is a two-pixel
    plateau whose pixels are the top two, lower linear index first."""
    sp = c['out']['spectrum_db']
    assert np.array_equal(sp[:, 10, :], sp[:, 9, :])       # theta = 45 deg twice
    assert np.array_equal(sp[:, :, 23], sp[:, :, 22])      # phi = 30 deg twice
    for i in range(c['n']):
        a, b = c['out']['peaks'][i] - 1
        flat = sp[i].flatten(order='F')
        assert a < b and flat[a] == flat[b] == 0.0
        ra, ca, rb, cb = a % 18, a // 18, b % 18, b // 18
        assert max(abs(ra - rb), abs(ca - cb)) == 1         # 8-neighbours: one plateau


@pytest.mark.gpu
def test_forms_of_call(case):
    c = case
    plan, n, M = c['plan'], c['n'], c['M']
    # the fixture's call read the spectrum and the eigenvalues: the full eigensolver
    assert c['fast_after_full'] == 0
    pk, npk = np.zeros((n, M), np.int32), np.zeros(n, np.int32)
    plan.peaks_device(c['d_X'], n, pk, npk)                 # peaks only
    fast = plan.fast_count()
    assert np.array_equal(pk, c['out']['peaks'])
    if c['name'] != 'literal':
        assert np.array_equal(npk, c['out']['n_peaks'])
    if c['name'] in ('ura44', 'literal'):
        assert fast == n
    if M > 4:
        assert fast == 0
    spec = np.zeros((n, len(c['phi']) * len(c['theta'])), np.float64)
    plan.spectrum_device(c['d_X'], n, spec, pk, npk)         # spectrum without the eigenvalues
    assert plan.fast_count() == 0
    # (this form finds only the M signal eigenvalues, by another sectioning than the call that
    # reads all N: the same map to rounding, not bit for bit)
    full = c['out']['spectrum_db']
    spec = spec.reshape(n, len(c['phi']), len(c['theta'])).transpose(0, 2, 1)
    assert np.abs(spec - full)[full > -60.0].max() <= TOL['db']
    assert np.array_equal(pk, c['out']['peaks'])
    if c['name'] != 'literal':
        assert np.array_equal(npk, c['out']['n_peaks'])
    # rsp_music_process on host X == the device-resident path, and a second run == the first
    host = plan.process(c['X'], want_cov=True)
    again = plan.process_device(c['d_X'], n, want_cov=True)
    assert plan.fast_count() == 0
    for o in (host, again):
        for k in ('spectrum_db', 'eig', 'R', 'peaks', 'n_peaks'):
            assert np.array_equal(o[k], c['out'][k]), k
    hp, hn = plan.peaks(c['X'])
    assert np.array_equal(hp, c['out']['peaks'])


@pytest.mark.gpu
def test_profile_returns_four_stage_times(case):
    c = case
    for what in ('peaks', 'spectrum', 'eigenvalues'):
        pr = c['plan'].profile(c['d_X'], c['n'], iters=2, what=what)
        assert sorted(pr) == ['cov_ms', 'peaks_ms', 'scan_ms', 'subspace_ms']
        assert all(np.isfinite(v) and v > 0.0 for v in pr.values()), pr


@pytest.mark.gpu
def test_cross_plan_refusals():
    """The line-array and planar-array entry points refuse each other's plans (RSP_ERR_INVALID)."""
    from rsp import _abi
    from rsp.music import MusicPlan, MusicPlan2D
    lib = _abi.lib()
    p1 = MusicPlan(16, 64, 2, np.linspace(-1.0, 1.0, 50), 0.5, max_batch=1)
    p2 = MusicPlan2D(4, 4, 64, 2, PHI, THETA, max_batch=1)
    d1, d2 = p1.device_alloc(1), p2.device_alloc(1)
    try:
        ms = (ct.c_float * 4)()
        sc1 = _abi.MusicScene(1, 0, 1, 0, 10.0, (ct.c_double * 8)(0.1), (ct.c_double * 8)(1.0))
        sc2 = _abi.Music2DScene(1, 1, 1, 0, 10.0, (ct.c_double * 8)(0.1), (ct.c_double * 8)(0.2), (ct.c_double * 8)(1.0))
        inv = _abi.RSP_ERR_INVALID
        assert lib.rsp_music_synthesize_device(p2._h, ct.byref(sc1), 1, 0, ct.c_uint64(SEED), ct.c_void_p(d2)) == inv
        assert lib.rsp_music_synthesize_device_2d(p1._h, ct.byref(sc2), 1, 0, ct.c_uint64(SEED), ct.c_void_p(d1)) == inv
        assert lib.rsp_music_profile(p2._h, ct.c_void_p(d2), 1, 1, ms) == inv
        assert lib.rsp_music_profile_ex(p2._h, ct.c_void_p(d2), 1, 1, _abi.RSP_MUSIC_PEAKS, ms) == inv
        assert lib.rsp_music_profile_2d(p1._h, ct.c_void_p(d1), 1, 1, _abi.RSP_MUSIC_PEAKS, ms) == inv
        # and the right pairings still work
        p1.synthesize_device(d1, {'angles_rad': [0.1], 'snr_db': 10.0}, 1)
        p2.synthesize_device(d2, {'azim_rad': [0.1], 'elev_rad': [0.2], 'snr_db': 10.0}, 1)
        assert p1.profile(d1, 1, iters=1)['cov_ms'] > 0.0
        assert p2.profile(d2, 1, iters=1)['scan_ms'] > 0.0
    finally:
        p1.device_free(d1)
        p2.device_free(d2)
        p1.close()
        p2.close()


@pytest.mark.gpu
def test_music_2d_function_form():
    """MUSIC_2D(X1, M, nx, ny, ...) on one snapshot matrix equals the plan's outputs."""
    from rsp.music import MUSIC_2D
    scene = _scene(2, 10.0)
    X = ref.synthesize_2d(scene, 4, 4, 64, 0.5, 0.5, 0, SEED)
    phi_e, theta_e, PdB, EVA = MUSIC_2D(X, 2, 4, 4, PHI, THETA)
    r = ref.music_2d(X, 2, 4, 4, PHI, THETA, 0.5, 0.5)
    assert PdB.shape == (17, 33) and EVA.shape == (16,)
    assert np.array_equal(phi_e, r['phi_e_deg']) and np.array_equal(theta_e, r['theta_e_deg'])
    assert np.abs(EVA - r['eig']).max() <= TOL['eig'] * r['eig'].max()
