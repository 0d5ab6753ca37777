"""Line-array MUSIC over the plan's envelope: array, snapshot, source and scan sizes.

tests/test_music.py pins the path at three scenes, (N, K, M, S) = (64, 1024, 3, 200), (10, 1000, 3,
200) and (16, 256, 2, 401), plus complex-double special matrices at N = 16 and N <= 4 (M in {2, 3},
S <= 60).  The plan accepts N = 2..64, K >= 1, M = 1..min(8, N - 1), S = 3..4096; this file pins the
shapes below in both precisions against the complex128 oracle (oracle/music.py, np.linalg.eigh) on
the snapshots the device itself synthesised (4 instances, complex unit sources at
linspace(-60, 60, M) deg -- 20 deg when M = 1 --, awgn 10 dB 'measured', scan
linspace(-pi/2, pi/2, S)):

  id                  N    K   M     S   what it reaches
  n2-k7-m1-s33        2    7   1    33   smallest array, K % 4 = 3, K < 16 (waves without a step)
  n8-k1-m1-s65        8    1   1    65   one snapshot (rank 1), S one past a wave
  n12-k5-m2-s100     12    5   2   100   K < N: rank-deficient R, exact zero noise eigenvalues
  n9-k40-m8-s181      9   40   8   181   M = N - 1 = MU_MMAX: one-dimensional noise subspace
  n17-k37-m1-s67     17   37   1    67   first row past a 16-row block, K % 4 = 1
  n31-k130-m4-s129   31  130   4   129   last fast instantiation, K % 4 = 2, K past one synthesis chunk
  n33-k131-m5-s257   33  131   5   257   first non-fast M, S one past 256
  n48-k64-m6-s255    48   64   6   255   full third row block
  n49-k98-m7-s256    49   98   7   256   one row into the fourth block
  n63-k203-m8-s513   63  203   8   513   largest odd N, K % 4 = 3; the 8th peak in slot po[MU_MMAX]
  n4-k16-m1-s3        4   16   1     3   shortest scan
  n16-k64-m7-s4096   16   64   7  4096   longest scan; c128 dynamic LDS 65 696 B (above 64 KiB)
  n16-k64-m8-s4095   16   64   8  4095   the same (69 272 B) with the last stride partly filled

plus a duplicated scan grid (N = 16, K = 64, M = 3, S = 131: flat tops, plateaus at both ends), the
host entry's widening / narrowing of snapshots (n17, n33) and batch position / stale state (n33,
and n31 for the fast-path count).

Tolerances are those of tests/test_music.py.  Complex double: X 1e-12, R 1e-12, eigenvalues 1e-11
of the largest, spectrum 1e-7 dB (the oracle stays above -60 dB in every case here); complex single:
X 1e-6, R 2e-6, eigenvalues 2e-5, spectrum 0.02 dB.  Peaks:

  * self-consistency, exact, every instance, both precisions, every call form: the returned peaks
    and count are findpeaks + the stable-descending top M of the spectrum the device returned (the
    kernels pick peaks from the very values they store);
  * complex double against the oracle, exact, wherever the oracle's margin -- min(smallest
    |P_dB[s+1] - P_dB[s]|, smallest gap between the M + 1 highest peaks) -- is >= 5e-7 dB, 5 x the
    spectrum tolerance: every instance of every case with S <= 513 (a CPU test asserts that); the
    two S >= 4095 cases have margins of 8e-8 .. 6e-7 dB and compare only where they qualify;
  * complex single against the oracle: where the M + 1 highest peaks are >= 0.04 dB apart (2 x the
    tolerance; at least 3 of 4 instances in every case, asserted on the CPU) the sorted peak
    indices are within one sample of the oracle's.

The CPU tests at the top hold the preconditions (margins, qualifying counts, the duplicated grid's
reference answers, which cases exceed 64 KiB of LDS) and need no device.
"""
import os
import re

import numpy as np
import pytest

from oracle import music as mu

import _music_shapes as ms
from _music_shapes import CASES, CASE_IDS, DL, N_INST, SEED, TOL

PRECS = ('c128', 'c64')
KEYS = ('spectrum_db', 'eig', 'R', 'peaks', 'n_peaks')


def _oracle(X, M, scan):
    return [mu.music_1d(np.asarray(X[i]).astype(np.complex128), M, scan, DL) for i in range(len(X))]


# ---------------------------------------------------------------------------- CPU: preconditions
def test_case_table_is_inside_the_envelope_and_reaches_its_branches():
    for N, K, M, S in CASES.values():
        assert 2 <= N <= 64 and K >= 1 and 1 <= M <= min(8, N - 1) and 3 <= S <= 4096
    shapes = list(CASES.values())
    assert {K % 4 for _, K, _, _ in shapes} == {0, 1, 2, 3}            # every snapshot tail
    assert any(K == 1 for _, K, _, _ in shapes) and any(K < N for N, K, _, _ in shapes)
    assert {M for _, _, M, _ in shapes} == set(range(1, 9)) - {3}      # 3 is test_music.py's
    assert {2, 17, 33, 48, 49, 63} <= {N for N, _, _, _ in shapes}     # row-block edges of k_music_eig64
    assert any(N % 4 and N % 8 for N, _, _, _ in shapes)               # k_music_cov<false>, pad rows
    assert any(M == N - 1 for N, _, M, _ in shapes)
    assert {3, 4095, 4096} <= {S for _, _, _, S in shapes}


@pytest.mark.parametrize('case', CASE_IDS)
def test_reference_margins_qualify(case):
    """The oracle alone: which instances a device answer must match exactly.  Complex double: every
    instance of a case with S <= 513 has a margin >= 5e-7 dB (smallest here: 1.0e-6 n63 instance 3,
    2.0e-6 n49 instance 1, 2.4e-6 n48 instance 0).  Complex single: at least 3 of the 4 instances
    have their M + 1 highest peaks >= 0.04 dB apart (all do except n63 instance 3, 2.7e-3; n49
    instance 1, 0.029; n16-m8 instance 2, 6.0e-3) -- on the complex128 snapshots and on their
    complex64 rounding, which is what a complex-single plan's reference runs on."""
    N, K, M, S = CASES[case]
    X = ms.oracle_snapshots(case)
    scan = ms.scan_for(S)
    for Xr in (X, X.astype(np.complex64)):
        ref = _oracle(Xr, M, scan)
        assert min(r['spectrum_db'].min() for r in ref) > -60.0    # every scan point is 'live'
        margins = [ms.exact_margin(r['spectrum_db'], M) for r in ref]
        gaps = [ms.height_gap(r['spectrum_db'], M) for r in ref]
        print(case, 'margins', margins, 'gaps', gaps)
        if case not in ms.LONG_SCAN:
            assert min(margins) >= ms.EXACT_MARGIN_DB, margins
        assert sum(g >= ms.C64_GAP_DB for g in gaps) >= 3, gaps


def test_duplicated_grid_reference():
    """The plateau case's reference answers: the duplicated grid has 131 points; a repeated angle's
    oracle value is bit-identical to its first occurrence; findpeaks reports the first sample of each
    flat top (1-based 44, 65, 98: the sources at base indices 40, 60, 90), never the triple plateaus
    at the ends, and as many peaks (13) as on the unique grid; the unique grid's margins (>= 2e-4 dB
    here) make the complex-double comparison exact and every instance qualifies in complex single."""
    base, dup, first = ms.dup_grid()
    assert len(base) == 121 and len(dup) == 131
    assert np.allclose(np.rad2deg(base[[40, 60, 90]]), ms.DUP_SOURCES_DEG, atol=1e-12)
    assert np.array_equal(dup, dup[first]) and np.array_equal(np.unique(dup), base)
    assert list(first[:4]) == [0, 0, 0, 3] and list(first[-3:]) == [128, 128, 128]
    X = ms.dup_snapshots()
    for Xr in (X, X.astype(np.complex64)):
        uni = _oracle(Xr, ms.DUP_M, base)
        ref = _oracle(Xr, ms.DUP_M, dup)
        for u, r in zip(uni, ref):
            assert np.array_equal(r['spectrum_db'], r['spectrum_db'][first])
            assert ms.exact_margin(u['spectrum_db'], ms.DUP_M) >= ms.EXACT_MARGIN_DB
            assert ms.height_gap(u['spectrum_db'], ms.DUP_M) >= ms.C64_GAP_DB
            assert sorted(r['peaks']) == [44, 65, 98]
            assert sorted(u['peaks']) == [41, 61, 91]
            assert r['n_peaks'] == u['n_peaks'] == 13
            # the device's convention (zero padding, stable order) restated by top_peaks
            pk, n = ms.top_peaks(r['spectrum_db'], ms.DUP_M)
            assert list(pk) == list(r['peaks']) and n == r['n_peaks']


def test_long_scan_cases_exceed_64k_of_lds():
    """k_music_eig64's dynamic LDS (me_lds_bytes): M = 7 with S = 4096 needs 65 696 B and M = 8 with
    S = 4095 needs 69 272 B, so music_route has the launcher raise the kernel's dynamic-LDS limit for
    exactly these two cases; every other case stays within 64 KiB.  The restated formula is the source's
    (tests/test_host_asan.py::test_music_routes compares the compiled one)."""
    assert ms.me_lds_bytes(7, 4096) == 65696
    assert ms.me_lds_bytes(8, 4095) == 69272
    for case, (N, K, M, S) in CASES.items():
        assert (ms.me_lds_bytes(M, S) > 64 * 1024) == (case in ms.LONG_SCAN), case
    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..',
                        'radar-signal-simulation-and-target-detection_amd', 'csrc')
    flat = re.sub(r'\s+', ' ', open(os.path.join(csrc, 'rsp_music_geometry.h')).read())
    assert '#define ME_VW 68 ' in flat
    assert ('me_lu_doubles(int M) { return 5 * 64 * M > 32 * ME_VW ? 5 * 64 * M : 32 * ME_VW; }') in flat
    assert ('return (size_t)4 * ME_VW * 16 + 64 * 16 + 8 * 16 + 3 * 68 * 8 + 64 * 8 + (size_t)me_lu_doubles(M) * 8 + '
            '(size_t)M * 64 * 16 + ((size_t)S + 8) * 8 + 8 * 16;') in flat
    assert 'r.raise_lds = r.lds > 64 * 1024;' in open(os.path.join(csrc, 'rsp_music_geometry.cpp')).read()
    assert 'if (r.raise_lds) e = hipFuncSetAttribute(' in re.sub(r'\s+', ' ', open(os.path.join(csrc, 'rsp_music.hip')).read())


def test_f32_restatement_is_far_inside_the_complex_single_tolerances():
    """What single precision itself costs (every stage in complex64 / float32 on the host, LAPACK's
    eigh) against the complex128 oracle.  Measured: at most 1.0e-4 dB (n9-k40-m8, the sharpest
    nulls) and 9e-8 of the largest eigenvalue.  Asserted: a quarter of the documented complex-single
    tolerances (0.02 dB, 2e-5), so no case here would need a tolerance of its own under the rule
    'at most 4 x the restatement's error' -- a kernel that misses 0.02 dB is at fault, not the
    tolerance."""
    worst_db = worst_ev = 0.0
    for case, (N, K, M, S) in CASES.items():
        X = ms.oracle_snapshots(case).astype(np.complex64)
        scan = ms.scan_for(S)
        for i in range(N_INST):
            r = mu.music_1d(X[i].astype(np.complex128), M, scan, DL)
            ev, db = ms.f32_restatement(X[i], M, scan)
            worst_db = max(worst_db, np.abs(db - r['spectrum_db']).max())
            worst_ev = max(worst_ev, np.abs(ev - r['eig']).max() / r['eig'].max())
    print('f32 restatement: worst %.2e dB, %.2e of the largest eigenvalue' % (worst_db, worst_ev))
    assert worst_db <= TOL['c64']['db'] / 4 and worst_ev <= TOL['c64']['eig'] / 4


# ---------------------------------------------------------------------------- GPU: the shapes
def _run_forms(plan, scene, n):
    """The three call forms on device-synthesised snapshots: (X downloaded, full call with the
    covariance, spectrum-only call, peaks-only call, fast counts after each)."""
    d_X = plan.device_alloc(n)
    try:
        plan.synthesize_device(d_X, scene, n, inst0=0, seed=SEED)
        X = plan.download(d_X, n)
        full = plan.process_device(d_X, n, want_cov=True)
        fc_full = plan.fast_count()
    finally:
        plan.device_free(d_X)
    spec = plan.process(X, want_eig=False)
    fc_spec = plan.fast_count()
    pk, npk = plan.peaks(X)
    fc_peaks = plan.fast_count()
    return dict(X=X, full=full, spec=spec, peaks=(pk, npk), fast=dict(full=fc_full, spec=fc_spec, peaks=fc_peaks))


@pytest.fixture(scope='module')
def shapes():
    """get(case, prec): the plan of a case (max_batch 4), its downloaded snapshots, the three call
    forms' outputs and the oracle on the same snapshots -- built once per (case, precision)."""
    from rsp.music import MusicPlan
    cache = {}

    def get(case, prec):
        if (case, prec) not in cache:
            N, K, M, S = CASES[case]
            scan = ms.scan_for(S)
            plan = MusicPlan(N, K, M, scan, DL, max_batch=N_INST, precision=prec)
            c = dict(N=N, K=K, M=M, S=S, scan=scan, plan=plan, prec=prec, tol=TOL[prec], name=case)
            cache[(case, prec)] = c   # registered first: closed at teardown whatever happens below
            c.update(_run_forms(plan, ms.scene_for(M), N_INST))
            c['ref'] = _oracle(c['X'], M, scan)
        return cache[(case, prec)]

    yield get
    for c in cache.values():
        c['plan'].close()


def _assert_self_consistent(spec, peaks, n_peaks, M):
    for i in range(len(spec)):
        want, n = ms.top_peaks(spec[i], M)
        assert n_peaks[i] == n, (i, n_peaks[i], n)
        assert list(peaks[i]) == list(want), (i, list(peaks[i]), list(want))


def _forms(c):
    """(name, spectrum the form's peaks were picked from, peaks, n_peaks) of the three call forms;
    the peaks-only call returns no spectrum: the spectrum-only call's stands in."""
    return (('full', c['full']['spectrum_db'], c['full']['peaks'], c['full']['n_peaks']),
            ('spectrum', c['spec']['spectrum_db'], c['spec']['peaks'], c['spec']['n_peaks']),
            ('peaks', c['spec']['spectrum_db'], c['peaks'][0], c['peaks'][1]))


def _assert_peaks_match_oracle(c, ref, M, need_all_exact):
    """Section 'peaks against the oracle': complex double exact where the margin qualifies, complex
    single within one sample where the height gap qualifies."""
    margins = [ms.exact_margin(r['spectrum_db'], M) for r in ref]
    gaps = [ms.height_gap(r['spectrum_db'], M) for r in ref]
    print(c['name'], c['prec'], 'margins', margins, 'gaps', gaps)
    if c['prec'] == 'c128':
        ok = [m >= ms.EXACT_MARGIN_DB for m in margins]
        if need_all_exact:
            assert all(ok), margins
    else:
        ok = [g >= ms.C64_GAP_DB for g in gaps]
        assert sum(ok) >= 3, gaps
    for name, _, pk, npk in _forms(c):
        for i, r in enumerate(ref):
            if not ok[i]:
                continue
            want, n = ms.top_peaks(r['spectrum_db'], M)
            if c['prec'] == 'c128':
                assert list(pk[i]) == list(want), (name, i, list(pk[i]), list(want))
                assert npk[i] == n == r['n_peaks'], (name, i)
            else:
                assert np.abs(np.sort(pk[i]) - np.sort(want)).max() <= 1, (name, i, list(pk[i]), list(want))


@pytest.mark.gpu
@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('case', CASE_IDS)
def test_shape_synthesis_covariance_eigenvalues(shapes, case, prec):
    """k_music_synth (up to 8 sources, K not a multiple of its 128-snapshot chunk), the covariance
    kernels' snapshot and channel tails, and all N eigenvalues, against the oracle."""
    c = shapes(case, prec)
    tol = c['tol']
    for i in range(N_INST):
        x = ms.oracle_snapshots(case)[i]
        ex = np.abs(c['X'][i] - x).max() / np.abs(x).max()
        R, d = c['ref'][i]['R'], c['ref'][i]['eig']
        er = np.abs(c['full']['R'][i] - R).max() / np.abs(R).max()
        ee = np.abs(c['full']['eig'][i] - d).max() / d.max()
        print(case, prec, i, 'X %.2e R %.2e eig %.2e' % (ex, er, ee))
        assert ex <= tol['X']
        assert er <= tol['R']
        assert c['full']['eig'].shape == (N_INST, c['N']) and ee <= tol['eig']


@pytest.mark.gpu
@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('case', CASE_IDS)
def test_shape_spectrum(shapes, case, prec):
    """The full call's spectrum and the spectrum-only call's (want_eig=False) against the oracle; in
    complex double the two also agree to 1e-8 dB (the fast path's proven bound, or the same path)."""
    c = shapes(case, prec)
    assert 'eig' not in c['spec']
    for i in range(N_INST):
        ref = c['ref'][i]['spectrum_db']
        live = ref > -60.0
        assert live.all()
        ef = np.abs(c['full']['spectrum_db'][i][live] - ref[live]).max()
        es = np.abs(c['spec']['spectrum_db'][i][live] - ref[live]).max()
        ed = np.abs(c['spec']['spectrum_db'][i][live] - c['full']['spectrum_db'][i][live]).max()
        print(case, prec, i, 'full %.2e spectrum-only %.2e between %.2e dB' % (ef, es, ed))
        assert ef <= c['tol']['db']
        assert es <= c['tol']['db']
        if prec == 'c128':
            assert ed <= 1e-8


@pytest.mark.gpu
@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('case', CASE_IDS)
def test_shape_peaks_are_those_of_the_returned_spectrum(shapes, case, prec):
    """Exact, every instance, every call form: n_peaks and the M peak slots are findpeaks and the
    stable-descending top M (1-based, zero-padded) of the spectrum the device returned -- the
    stride and mask logic of the peak search at every S, and the 8th peak's slot at M = 8."""
    c = shapes(case, prec)
    for name, spec, pk, npk in _forms(c):
        assert pk.shape == (N_INST, c['M'])
        _assert_self_consistent(spec, pk, npk, c['M'])


@pytest.mark.gpu
@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('case', CASE_IDS)
def test_shape_peaks_match_oracle(shapes, case, prec):
    c = shapes(case, prec)
    _assert_peaks_match_oracle(c, c['ref'], c['M'], need_all_exact=case not in ms.LONG_SCAN)


@pytest.mark.gpu
@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('case', CASE_IDS)
def test_shape_fast_count(shapes, case, prec):
    """No instance is counted as answered by the block-power fast path after a call that reads the
    eigenvalues, nor after any call on a plan with M >= 5 (or in complex single).  For M <= 4 in
    complex double the count of the other forms is only bounded: whether the proof succeeds at
    these scenes is not known in advance."""
    c = shapes(case, prec)
    print(case, prec, 'fast counts', c['fast'])
    assert c['fast']['full'] == 0
    if c['M'] >= 5 or prec == 'c64':
        assert c['fast']['spec'] == 0 and c['fast']['peaks'] == 0
    else:
        assert 0 <= c['fast']['spec'] <= N_INST and 0 <= c['fast']['peaks'] <= N_INST


# ---------------------------------------------------------------------------- GPU: plateaus
@pytest.mark.gpu
@pytest.mark.parametrize('prec', PRECS)
def test_duplicated_scan_grid(prec):
    """Repeated scan angles: a lane's arithmetic depends only on its steering values, so a repeated
    angle's value is bit-identical to its first occurrence, and findpeaks' run-of-equal-values logic
    decides -- the first sample of each flat top (1-based 44, 65, 98), never the triple plateaus at
    the two ends, 13 peaks as on the unique grid."""
    from rsp.music import MusicPlan
    base, dup, first = ms.dup_grid()
    M = ms.DUP_M
    plan = MusicPlan(ms.DUP_N, ms.DUP_K, M, dup, DL, max_batch=N_INST, precision=prec)
    try:
        c = _run_forms(plan, ms.dup_scene(), N_INST)
    finally:
        plan.close()
    for i in range(N_INST):
        x = ms.dup_snapshots()[i]
        assert np.abs(c['X'][i] - x).max() <= TOL[prec]['X'] * np.abs(x).max()
    ref = _oracle(c['X'], M, dup)
    uni = _oracle(c['X'], M, base)
    for name, spec, pk, npk in _forms(c):
        assert np.array_equal(spec, spec[:, first]), name          # bit-identical repeats
        _assert_self_consistent(spec, pk, npk, M)
        for i in range(N_INST):
            live = ref[i]['spectrum_db'] > -60.0
            assert np.abs(spec[i][live] - ref[i]['spectrum_db'][live]).max() <= TOL[prec]['db']
            assert not ({1, 2, 3, 129, 130, 131} & set(int(p) for p in pk[i]))
            if prec == 'c128':
                assert sorted(pk[i]) == [44, 65, 98] and npk[i] == 13
    # the margins are the unique grid's (a duplicated grid has zero steps by construction)
    margins = [ms.exact_margin(u['spectrum_db'], M) for u in uni]
    gaps = [ms.height_gap(u['spectrum_db'], M) for u in uni]
    print('dup', prec, 'unique-grid margins', margins, 'gaps', gaps)
    assert min(margins) >= ms.EXACT_MARGIN_DB and min(gaps) >= ms.C64_GAP_DB
    for name, _, pk, npk in _forms(c):
        for i, r in enumerate(ref):
            if prec == 'c128':
                assert list(pk[i]) == list(r['peaks']), (name, i)
                assert npk[i] == r['n_peaks'] == uni[i]['n_peaks']
            else:
                assert np.abs(np.sort(pk[i]) - np.sort(r['peaks'])).max() <= 1, (name, i)


# ---------------------------------------------------------------------------- GPU: host entry
def _assert_same_outputs(a, b, sel=None):
    for k in KEYS:
        if k in a or k in b:
            want = b[k] if sel is None else b[k][sel]
            assert np.array_equal(a[k], want), k


@pytest.mark.gpu
@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('case', ['n17-k37-m1-s67', 'n33-k131-m5-s257'])
def test_host_entry_converts_snapshots_like_numpy(shapes, case, prec):
    """rsp_music_process widens complex64 snapshots into a complex-double plan and narrows
    complex128 ones into a complex-single plan: either equals, bit for bit, the call on snapshots
    numpy converted beforehand (spectrum, eigenvalues, covariance, peaks, count)."""
    c = shapes(case, prec)
    plan = c['plan']
    if prec == 'c128':
        X32 = c['X'].astype(np.complex64)
        assert not np.array_equal(X32.astype(np.complex128), c['X'])      # the rounding is not a no-op
        a = plan.process(X32, want_cov=True)                              # widened by the library
        b = plan.process(X32.astype(np.complex128), want_cov=True)
    else:
        X128 = np.array(ms.oracle_snapshots(case))                        # complex128 with low bits set
        assert not np.array_equal(X128.astype(np.complex64).astype(np.complex128), X128)
        a = plan.process(X128, want_cov=True)                             # narrowed by the library
        b = plan.process(X128.astype(np.complex64), want_cov=True)
    assert a['spectrum_db'].shape == (N_INST, c['S']) and np.isfinite(a['spectrum_db']).all()
    assert (a['n_peaks'] > 0).all() and (a['eig'][:, 0] > 0).all()
    _assert_same_outputs(a, b)


# ---------------------------------------------------------------------------- GPU: batch position
@pytest.mark.gpu
@pytest.mark.parametrize('prec', PRECS)
def test_batch_position_and_stale_state(shapes, prec):
    """An instance's outputs do not depend on where it sits in the batch, and a smaller call after a
    larger one returns (and counts) only its own instances."""
    c = shapes('n33-k131-m5-s257', prec)
    plan, X = c['plan'], c['X']
    perm = [2, 0, 3, 1]
    base = plan.process(X, want_cov=True)
    _assert_same_outputs(base, c['full'])                      # host upload == device-resident call
    _assert_same_outputs(plan.process(X[perm], want_cov=True), base, perm)
    sp = plan.process(X[perm], want_eig=False)
    assert np.array_equal(sp['spectrum_db'], c['spec']['spectrum_db'][perm])
    pk, npk = plan.peaks(X[perm])
    assert np.array_equal(pk, c['peaks'][0][perm]) and np.array_equal(npk, c['peaks'][1][perm])
    plan.process(X, want_cov=True)                             # 4 instances, then 1
    one = plan.process(X[3:4], want_cov=True)
    _assert_same_outputs(one, base, slice(3, 4))
    assert plan.fast_count() <= 1
    plan.peaks(X)
    pk1, npk1 = plan.peaks(X[3:4])
    assert np.array_equal(pk1, c['peaks'][0][3:4]) and np.array_equal(npk1, c['peaks'][1][3:4])
    assert plan.fast_count() <= 1


@pytest.mark.gpu
def test_fast_count_counts_the_last_call_only(shapes):
    """The M = 4 case in complex double, where the peaks-only call may take the fast path: the count
    after a 1-instance call is that instance's alone (0 or 1, never the previous 4-instance call's),
    and the flags of the instances run one at a time add up to the batch's count."""
    c = shapes('n31-k130-m4-s129', 'c128')
    plan, X = c['plan'], c['X']
    plan.peaks(X)
    n4 = plan.fast_count()
    assert n4 == c['fast']['peaks']
    singles = []
    for i in range(N_INST):
        pk, npk = plan.peaks(X[i:i + 1])
        singles.append(plan.fast_count())
        assert np.array_equal(pk, c['peaks'][0][i:i + 1]) and np.array_equal(npk, c['peaks'][1][i:i + 1])
    print('fast count of the batch', n4, 'one at a time', singles)
    assert all(s in (0, 1) for s in singles) and sum(singles) == n4
