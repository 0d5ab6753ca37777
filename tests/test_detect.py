"""The detector on any RD cube on the device (k_pairsum, k_xcfar, k_s9 and the host's S10 / S11:
Plan.detect, detect_device, mtd_detect, process_stage2_detect, rsp.detect_rdm, rsp.mtd_detect).

1. Against the frame chain, to the bit: Plan.process_cube's own RD map fed back through Plan.detect gives
   K3's pair-sum maps, K3's detection list field by field and the frame's final targets.  The other side
   is existing code (K2's magnitudes, K3).
2. Against the oracle (oracle.chain's S8-S11 on the same cube with the caller's axes) on shapes no plan
   reaches, with the rules and tolerances of tests/_parity.py unchanged.  tests/_detect_cases.py holds the
   table, test_detect_cases.py its preconditions.
3. A dense map: more than 65 536 hits, so that the hit list grows and k_xcfar's queue overflows.
4. The compositions equal the calls they are made of, to the bit.
5. The conventions of the synchronous calls.
"""
import ctypes as ct

import numpy as np
import pytest

import _detect_cases as dc
import _parity as par
import rsp
from rsp import _abi
from rsp.plan import Plan
from oracle import chain
from _scen import scenario, targets_for, noisy_cube, k3_noise_cube

pytestmark = pytest.mark.gpu

FIELDS = ('v_idx', 'r_idx', 'pair_idx', 'amp', 'Range', 'Velocity', 'Angle')
WORD = np.uint32(0x7FC5A3F1)   # a NaN as a float, and twice over as a double
GUARD = 1 << 12


@pytest.fixture(scope='module', params=dc.PRECS)
def plan(request):
    s = scenario('plumbing')
    p = Plan(s['cfg'], s['cfar'], s['clus'], s['pre_p'], precision=request.param)
    yield p
    p.close()


def _same_lists(a, b):
    assert len(a['detections']) == len(b['detections'])
    for x, y in zip(a['detections'], b['detections']):
        for f in FIELDS:
            assert x[f] == y[f], (f, x, y)
    assert a['final_targets'] == b['final_targets']


def _detect_case(plan, name, **kw):
    c = dc.CASES[name]
    ax = dc.axes(c['V'], c['G'], c['B'])
    return plan.detect(dc.cube(name, plan.precision), dc.cfar_dict(c), dc.CLUSTER, ax['range_axis'], ax['velocity_axis'], ax['deltaR'],
                       ax['deltaV'], ax['beam_angles_deg'], ax['k_slopes_LUT'], want_cfar=True, **kw)


# ---- 1. bit identity with the frame chain -------------------------------------------------------------
@pytest.mark.parametrize('prec', dc.PRECS)
@pytest.mark.parametrize('name, monopulse', [('small', 'amplitude'), ('fast-2band', 'amplitude'), ('small', 'complex')])
def test_bit_identity_with_the_frame_chain(name, monopulse, prec):
    s = scenario(name)
    cube = noisy_cube(s, targets_for(name), dtype=np.complex128) if name == 'small' else k3_noise_cube(s, 'c128')
    if prec == 'c64':
        cube = cube.astype(np.complex64)
    p = Plan(s['cfg'], s['cfar'], s['clus'], s['pre_p'], precision=prec, monopulse=monopulse)
    try:
        frame = p.process_cube(cube, want_rdm=True, want_cfar=True)
        got = p.detect(frame['rdm'], want_cfar=True)
    finally:
        p.close()
    n = len(frame['detections'])
    print(name, monopulse, prec, '%d detections, %d targets' % (n, len(frame['final_targets'])))
    assert n > (1000 if name == 'fast-2band' else 0)
    assert np.array_equal(got['cfar_maps'], frame['cfar_maps'])
    _same_lists(got, frame)


# ---- 2. oracle parity on shapes no plan reaches ---------------------------------------------------------
@pytest.mark.parametrize('name', dc.CASE_IDS)
def test_oracle_parity(plan, name):
    c = dc.CASES[name]
    got = _detect_case(plan, name)
    case = dc.parity_case(name, plan.precision, got)
    print(name, plan.precision, '%d device / %d oracle detections' % (len(got['detections']), len(case['st']['dets'])))
    assert got['cfar_maps'].shape == (c['V'], c['G'], c['B'] - 1)
    par.check_cfar_map(case)
    par.check_detection_sets(case)
    par.check_detection_order_and_estimates(case)
    par.check_final_targets(case)


@pytest.mark.parametrize('name', ['tile+1', 'b13'])
def test_oracle_parity_complex_monopulse(plan, name):
    got = _detect_case(plan, name, monopulse='complex')
    case = dc.parity_case(name, plan.precision, got, 'complex')
    par.check_detection_sets(case)
    par.check_detection_order_and_estimates(case)
    par.check_final_targets(case)


def test_no_cell_under_test_still_gives_the_maps(plan):
    for name in ('v1', 'short-g'):
        got = _detect_case(plan, name)
        assert got['detections'] == [] and got['final_targets'] == []
        x = dc.cube(name, plan.precision).astype(np.complex128)
        par.map_close(got['cfar_maps'], np.abs(x[:, :, :-1]) + np.abs(x[:, :, 1:]), par.MAP_TOL[plan.precision])


# ---- 3. dense ---------------------------------------------------------------------------------------------
def test_dense_map(plan):
    c = dc.DENSE
    x = dc.cube('dense', plan.precision)
    ax = dc.axes(c['V'], c['G'], c['B'])
    cfar = dc.cfar_dict(c)
    tight = dict(max_range_sep=0.0, max_vel_sep=0.0, max_angle_sep=0.0)   # only equal points cluster: the host's sweep stays short
    got = plan.detect(x, cfar, tight, ax['range_axis'], ax['velocity_axis'], ax['deltaR'], ax['deltaV'], ax['beam_angles_deg'],
                      ax['k_slopes_LUT'])
    x128 = x.astype(np.complex128)
    dets, S_all = chain.goca_cfar(x128, cfar)
    gk = [(d['v_idx'], d['r_idx'], d['pair_idx']) for d in got['detections']]
    ok = par.keys(dets)
    print('dense', plan.precision, '%d device / %d oracle hits' % (len(gk), len(ok)))
    assert len(ok) > 65536
    assert gk == sorted(gk, key=lambda k: (k[2], k[1], k[0])), 'not in fsf find() order'
    if plan.precision == 'c128':
        assert gk == ok
    else:
        mg = chain.cfar_margin(x128, cfar)
        for (v, r, p) in set(gk) ^ set(ok):
            assert mg[v - 1, r - 1, p - 1] < par.MARGIN, 'CFAR decision differs at (v=%d r=%d pair=%d)' % (v, r, p)
    # the estimates on a fixed sample of the oracle's hits (its per-hit spline is too slow for all of them)
    idx = np.random.default_rng(5).choice(len(ok), dc.DENSE_SAMPLE, replace=False)
    idx.sort()
    sample = dets[idx]
    est = chain.parameter_estimation(sample, S_all, x128, ax)
    by_key = {k: d for k, d in zip(gk, got['detections'])}
    sub = [by_key[k] for k in par.keys(sample) if k in by_key]
    assert len(sub) >= dc.DENSE_SAMPLE - (0 if plan.precision == 'c128' else 5)
    case = dict(prec=plan.precision, s=dict(cfar=cfar, pre_o=ax, clus=tight), st=dict(dets=sample, par=est, rdm=x128, S_all=S_all),
                gpu=dict(detections=sub))
    par.check_detection_order_and_estimates(case)
    assert 0 < len(got['final_targets']) <= len(gk)


# ---- 4. compositions ----------------------------------------------------------------------------------------
def _pc_cube(prec, P=332, G=40, B=3):
    rng = np.random.default_rng(21)
    pc = (rng.standard_normal((P, G, B)) + 1j * rng.standard_normal((P, G, B))) * np.sqrt(0.5)
    m = np.arange(P)
    for g, f, a in ((18, 0.113, 3.0), (22, -0.31, 2.0)):
        for b, s in ((0, 1.0), (1, 0.7), (2, 0.3)):
            pc[:, g, b] += a * s * np.exp(2j * np.pi * f * m + 0.4j * b)
    return pc.astype(np.complex64) if prec == 'c64' else pc


def test_mtd_detect_equals_mtd_then_detect(plan):
    P, G, B, nfft = 332, 40, 3, 512
    pc, win = _pc_cube(plan.precision), np.kaiser(P, 5.0)
    cfar = dict(refCells_R=5, guardCells_R=10, refCells_V=5, guardCells_V=10, T_CFAR=3.0)
    ax = dc.axes(nfft, G, B)
    ax['velocity_axis'] = rsp.mtd_velocity_axis(40.0, nfft)
    args = (cfar, dc.CLUSTER, ax['range_axis'], ax['velocity_axis'], ax['deltaR'], ax['deltaV'], ax['beam_angles_deg'],
            ax['k_slopes_LUT'])
    one = plan.mtd_detect(pc, win, nfft, *args, want_rdm=True, want_cfar=True)
    rdm = plan.mtd(pc, win, nfft=nfft)
    two = plan.detect(rdm, *args, want_cfar=True)
    assert np.array_equal(one['rdm'], rdm) and np.array_equal(one['cfar_maps'], two['cfar_maps'])
    _same_lists(one, two)
    # ... and the oracle on that cube
    dets, S_all = chain.goca_cfar(rdm, cfar)
    est = chain.parameter_estimation(dets, S_all, rdm, ax)
    fin = chain.cluster_stage2(chain.cluster_stage1(est, dc.CLUSTER), dc.CLUSTER)
    case = dict(prec=plan.precision, s=dict(cfar=cfar, pre_o=ax, clus=dc.CLUSTER), fin=fin,
                st=dict(rdm=rdm, dets=dets, S_all=S_all, par=est), gpu=one)
    print('mtd_detect', plan.precision, '%d detections, %d targets' % (len(one['detections']), len(one['final_targets'])))
    par.check_cfar_map(case)
    par.check_detection_sets(case)
    par.check_detection_order_and_estimates(case)
    par.check_final_targets(case)
    # the MATLAB-signature mirror returns the same
    pre = dict(ax)
    m = rsp.mtd_detect(pc, win, nfft, cfar, dc.CLUSTER, pre, v_max=40.0, precision=plan.precision, want_cfar=True)
    assert np.array_equal(m['cfar_maps'], one['cfar_maps'])
    _same_lists(m, one)


@pytest.mark.parametrize('prec', dc.PRECS)
def test_process_stage2_detect_equals_detect_of_stage2(prec):
    """The device layout [B][P][G] of the stage-2 result against MATLAB's layout of the same values."""
    s = scenario('small')
    cube = noisy_cube(s, targets_for('small'), dtype=np.complex128)
    beams = chain.dbf(cube, s['pre_o']['DBF_coeffs_data_C'])
    if prec == 'c64':
        beams = beams.astype(np.complex64)
    p = Plan(s['cfg'], s['cfar'], s['clus'], s['pre_p'], precision=prec)
    try:
        one = p.process_stage2_detect(beams, want_rdm=True, want_cfar=True)
        mtd, _ = p.process_stage2(beams)
        two = p.detect(mtd, want_cfar=True)
    finally:
        p.close()
    print('stage2 detect', prec, '%d detections' % len(one['detections']))
    assert len(one['detections']) > 0
    assert np.array_equal(one['rdm'], mtd) and np.array_equal(one['cfar_maps'], two['cfar_maps'])
    _same_lists(one, two)


def test_detect_rdm_mirror(plan):
    name = 'tile+1'
    c = dc.CASES[name]
    want = _detect_case(plan, name)
    got = rsp.detect_rdm(dc.cube(name, plan.precision), dc.cfar_dict(c), dc.CLUSTER, dc.axes(c['V'], c['G'], c['B']),
                         precision=plan.precision, want_cfar=True)
    assert np.array_equal(got['cfar_maps'], want['cfar_maps'])
    _same_lists(got, want)


# ---- 5. conventions --------------------------------------------------------------------------------------------
def _c_call(plan, name, out, rdm_ptr=None):
    c = dc.CASES[name]
    ax = dc.axes(c['V'], c['G'], c['B'])
    prm, keep = plan._detect_params(c['V'], c['G'], c['B'], dc.cfar_dict(c), dc.CLUSTER, ax['range_axis'], ax['velocity_axis'],
                                    ax['deltaR'], ax['deltaV'], ax['beam_angles_deg'], ax['k_slopes_LUT'], None)
    x = np.asfortranarray(dc.cube(name, plan.precision))
    dt = _abi.RSP_C64 if x.dtype == np.complex64 else _abi.RSP_C128
    return _abi.lib().rsp_detect(plan.h, c['V'], c['G'], c['B'], x.ctypes.data_as(ct.c_void_p), dt, ct.byref(prm), ct.byref(out))


def test_short_lists_behave_as_process_cube(plan):
    want = _detect_case(plan, 'tile')
    n, nt = len(want['detections']), len(want['final_targets'])
    assert n > 2 and nt > 1
    dets, tg = (_abi.Detection * n)(), (_abi.Target * nt)()
    out = _abi.FrameOut(dets=dets, dets_cap=2, targets=tg, targets_cap=nt)
    assert _c_call(plan, 'tile', out) == _abi.RSP_ERR_OVERFLOW
    assert b'detections exceed dets_cap 2' in _abi.lib().rsp_last_error()
    assert (out.n_dets, out.n_targets) == (n, nt)
    assert [dets[i].r_idx for i in range(2)] == [d['r_idx'] for d in want['detections'][:2]] and dets[2].r_idx == 0
    assert plan.last_detections() == want['detections'] and plan.last_targets() == want['final_targets']
    out = _abi.FrameOut(dets=dets, dets_cap=n, targets=tg, targets_cap=1)
    assert _c_call(plan, 'tile', out) == _abi.RSP_ERR_OVERFLOW and b'targets exceed targets_cap 1' in _abi.lib().rsp_last_error()
    out = _abi.FrameOut(dets=dets, dets_cap=n, targets=tg, targets_cap=nt)
    assert _c_call(plan, 'tile', out) == _abi.RSP_OK and (out.n_dets, out.n_targets) == (n, nt)
    assert dets[n - 1].Range == want['detections'][-1]['Range'] and tg[nt - 1].Power == want['final_targets'][-1]['Power']


def test_refusals_come_before_device_work(plan):
    lib = _abi.lib()
    buf = np.zeros(8, np.float64)
    out = _abi.FrameOut(rdm=buf.ctypes.data_as(ct.POINTER(ct.c_double)))
    assert _c_call(plan, 'tile', out) == _abi.RSP_ERR_INVALID and b'out->rdm must be NULL' in lib.rsp_last_error()
    c = dc.CASES['tile']
    x = dc.cube('tile', plan.precision)
    with pytest.raises(rsp.RspError, match='refCells_R must be >= 1'):
        plan.detect(x, dict(dc.cfar_dict(c), refCells_R=0), dc.CLUSTER, *[dc.axes(64, 64, 3)[k] for k in (
            'range_axis', 'velocity_axis', 'deltaR', 'deltaV', 'beam_angles_deg', 'k_slopes_LUT')])
    with pytest.raises(ValueError):    # the plan's own axes do not fit this cube
        plan.detect(x[:, :5, :])
    with pytest.raises(ValueError):
        plan.detect(x[:, :, :1])
    assert lib.rsp_detect(plan.h, 64, 64, 3, None, _abi.RSP_C128, None, None) == _abi.RSP_ERR_INVALID
    assert lib.rsp_detect_device(plan.h, 64, 64, 1, None, None, None) == _abi.RSP_ERR_INVALID and b'B=1' in lib.rsp_last_error()
    assert lib.rsp_mtd_detect(plan.h, 8, 64, 3, 4, None, _abi.RSP_C128, None, None, None) == _abi.RSP_ERR_INVALID
    assert lib.rsp_process_stage2_detect(plan.h, None, _abi.RSP_C128, None) == _abi.RSP_ERR_INVALID


@pytest.mark.parametrize('name', ['tile+1', 'v333-b2'])
def test_device_cube_and_guard_bands(plan, name):
    """detect_device on an uploaded cube equals detect; the cube and the guard bands around it stay as they
    were, and the host's cfar_maps lie between untouched sentinels."""
    c = dc.CASES[name]
    ax = dc.axes(c['V'], c['G'], c['B'])
    want = _detect_case(plan, name)
    x = np.asfortranarray(dc.cube(name, plan.precision)).astype(plan.cdtype)
    esz = x.dtype.itemsize
    total = (2 * GUARD + x.size * esz) // 4
    d = plan.device_alloc(total * 4)
    try:
        plan.device_upload(d, np.full(total, WORD, np.uint32))
        plan.device_upload(d + GUARD, x.ravel(order='F'))
        before = plan.device_download(d, total, np.uint32)
        got = plan.detect_device(d + GUARD, c['V'], c['G'], c['B'], dc.cfar_dict(c), dc.CLUSTER, ax['range_axis'], ax['velocity_axis'],
                                 ax['deltaR'], ax['deltaV'], ax['beam_angles_deg'], ax['k_slopes_LUT'], want_cfar=True)
        after = plan.device_download(d, total, np.uint32)
    finally:
        plan.device_free(d)
    assert np.array_equal(before, after) and (after[:GUARD // 4] == WORD).all() and (after[-(GUARD // 4):] == WORD).all()
    assert np.array_equal(got['cfar_maps'], want['cfar_maps'])
    _same_lists(got, want)
    # host outputs between sentinels
    n = c['V'] * c['G'] * (c['B'] - 1)
    host = np.full(n + 64, np.float64(-7.25))
    prm, keep = plan._detect_params(c['V'], c['G'], c['B'], dc.cfar_dict(c), dc.CLUSTER, ax['range_axis'], ax['velocity_axis'],
                                    ax['deltaR'], ax['deltaV'], ax['beam_angles_deg'], ax['k_slopes_LUT'], None)
    out = _abi.FrameOut(cfar_maps=host[32:].ctypes.data_as(ct.POINTER(ct.c_double)))
    xs = np.asfortranarray(dc.cube(name, plan.precision))
    assert _abi.lib().rsp_detect(plan.h, c['V'], c['G'], c['B'], xs.ctypes.data_as(ct.c_void_p),
                                 _abi.RSP_C64 if xs.dtype == np.complex64 else _abi.RSP_C128, ct.byref(prm), ct.byref(out)) == 0
    assert (host[:32] == -7.25).all() and (host[32 + n:] == -7.25).all()
    assert np.array_equal(host[32:32 + n].reshape((c['V'], c['G'], c['B'] - 1), order='F'), want['cfar_maps'])


@pytest.mark.parametrize('prec', dc.PRECS)
def test_a_queued_frame_is_drained_first(prec):
    s = scenario('small')
    cube = noisy_cube(s, targets_for('small'), dtype=np.complex128 if prec == 'c128' else np.complex64)
    p = Plan(s['cfg'], s['cfar'], s['clus'], s['pre_p'], precision=prec)
    try:
        frame = p.process_cube(cube, want_rdm=True)
        qcube = np.asfortranarray(cube)   # borrowed until the queue is drained
        p.enqueue_host(qcube, 7)
        got = p.detect(frame['rdm'])
        nf, nt = ct.c_int32(), ct.c_int64()
        _abi.check(_abi.lib().rsp_results_count(p.h, ct.byref(nf), ct.byref(nt)))   # reads the list, drains nothing
        assert (nf.value, nt.value) == (1, len(frame['final_targets']))
        res = p.results()
    finally:
        p.close()
    _same_lists(got, frame)
    assert len(res) == 1, res


def test_profile_detect(plan):
    V, G, B = 96, 130, 3
    cfar = dict(refCells_R=5, guardCells_R=10, refCells_V=5, guardCells_V=10, T_CFAR=8.0)
    r = plan.profile_detect(V, G, B, cfar, iters=3)
    esz = 16 if plan.precision == 'c128' else 8
    assert all(r[k][0] > 0 for k in ('k_pairsum', 'k_xcfar', 'k_s9'))
    assert r['k_pairsum'][1] == V * G * B * esz + V * G * (B - 1) * esz // 2 and r['k_xcfar'][1] == V * G * (B - 1) * esz // 2
    assert r['k_s9'][1] > 0 and r['k_s9'][1] % 48 == 0
