"""Stage 2 on the raw cube (rsp_process_raw_stage2*, Plan.process_raw_stage2*, rsp.process_frame_stage2):
K1 with its DBF stage and without the MTD (launch mode 1 of k1_dbf_mtd), then the launches of the beams
forms.

Cases (P, B, C) on the `plumbing` waveform (1024 samples, 512 gates), noise-only cubes:
  (16, 3, 12)    padded beams and channels, Stockham column transform
  (12, 3, 12)    a P that is no power of two (the direct column transform; 12 < a sub-tile's 16 / 32 pulses)
  (64, 13, 16)   the reference's 13 x 16: two MFMA row blocks
  (16, 4, 32)    eight channel groups
The two routes -- the fused call, and ``process_stage2(dbf(cube))`` -- must agree to the bit: the same
fused operations per beam sample (Dbf<T>), and the same launches after the corner turn.
"""
import numpy as np
import pytest

import rsp
from rsp import config as C
from rsp.plan import Plan
from rsp.precompute import precompute as product_precompute
from oracle import chain, precompute as oracle_precompute
from _parity import MAP_TOL, map_close
from _scen import SEED, plumbing_config, plumbing_weights, scenario

pytestmark = pytest.mark.gpu

CASES = {'p16-b3-c12': (16, 3, 12), 'p12-b3-c12': (12, 3, 12), 'p64-b13-c16': (64, 13, 16), 'p16-b4-c32': (16, 4, 32)}
GATE_COLS = ((101, 164), (301, 492), (601, 856))      # 64 + 192 + 256 = 512 of the 1024 PRT columns
STAGE3 = dict(refCells_R=5, saveCells_R=14, T_CFAR=1.5, CFARmethod_R=0, MTD_0v_num=1)   # test_stage3_cfar.FUSED_CFAR
VCFAR = dict(refCells_V=4, guardCells_V=6, T_CFAR=1.5)                                   # test_vcfar.WINDOWS[1]
_ORACLE = {}


def _plumbing(name):
    P, B, Cn = CASES[name]
    cfg = plumbing_config(P, B, Cn)
    W, ang, k = plumbing_weights(cfg)
    return cfg, np.asarray(W, np.complex128), ang, k


def _cube(cfg, prec):
    raw = chain.philox_noise(cfg, 1, SEED)
    return raw if prec == 'c128' else raw.astype(np.complex64)


def _oracle(name, prec, W, conj=True):
    """(MTD, PC) of the oracle for the case's cube beamformed with W; computed once per key."""
    key = (name, prec, W.tobytes(), conj)
    if key not in _ORACLE:
        cfg, W0, ang, k = _plumbing(name)
        pre = oracle_precompute.precompute(cfg, W0, ang, k, C.V8_FIR)
        x = _cube(cfg, prec).astype(np.complex128)
        pc = chain.pulse_compress(chain.dbf(x, W) if conj else x @ W.T, pre)
        _ORACLE[key] = (chain.mtd(pc, pre), pc)
        for a in _ORACLE[key]:
            a.setflags(write=False)
    return _ORACLE[key]


@pytest.fixture(scope='module', params=[(n, p) for n in CASES for p in ('c128', 'c64')], ids=lambda x: '%s-%s' % x)
def case(request):
    name, prec = request.param
    cfg, W, ang, k = _plumbing(name)
    plan = Plan(cfg, C.default_cfar_params(), C.default_cluster_params(), product_precompute(cfg, W, ang, k, C.V8_FIR),
                precision=prec)
    yield dict(name=name, prec=prec, cfg=cfg, W=W, plan=plan, cube=_cube(cfg, prec))
    plan.close()


def test_fused_route_equals_dbf_then_stage2_to_the_bit(case):
    plan, cube, W = case['plan'], case['cube'], case['W']
    for conj in (True, False):
        mtd, pc = plan.process_raw_stage2(cube, W, conj=conj)
        mtd2, pc2 = plan.process_stage2(plan.dbf(cube, W, conj=conj))
        assert np.abs(pc).max() > 0
        np.testing.assert_array_equal(pc, pc2)
        np.testing.assert_array_equal(mtd, mtd2)


def test_raw_stage2_against_the_oracle(case):
    plan, cube, W, tol = case['plan'], case['cube'], case['W'], MAP_TOL[case['prec']]
    mtd_o, pc_o = _oracle(case['name'], case['prec'], W)
    mtd, pc = plan.process_raw_stage2(cube, W)
    map_close(pc, pc_o, tol)
    map_close(mtd, mtd_o, tol)
    # the plan's own weights: the same table values, the same bits
    mtd_n, pc_n = plan.process_raw_stage2(cube)
    np.testing.assert_array_equal(mtd_n, mtd)
    np.testing.assert_array_equal(pc_n, pc)


def test_w_and_conj_of_the_call_replace_the_cached_table(case):
    """Four calls on one plan: (W, conj), (W2, conj), (W, plain), (W, conj) again.  Each is its own
    oracle's result, and the last equals the first to the bit."""
    plan, cube, W, tol = case['plan'], case['cube'], case['W'], MAP_TOL[case['prec']]
    rng = np.random.default_rng(17)
    W2 = W * np.exp(2j * np.pi * rng.random(W.shape)) + 0.01
    first = plan.process_raw_stage2(cube, W, conj=True)
    other = plan.process_raw_stage2(cube, W2, conj=True)
    plain = plan.process_raw_stage2(cube, W, conj=False)
    again = plan.process_raw_stage2(cube, W, conj=True)
    map_close(other[0], _oracle(case['name'], case['prec'], W2)[0], tol)
    map_close(plain[0], _oracle(case['name'], case['prec'], W, conj=False)[0], tol)
    scale = np.abs(first[0]).max()
    assert np.abs(other[0] - first[0]).max() > 1e3 * tol * scale
    assert np.abs(plain[0] - first[0]).max() > 1e3 * tol * scale
    np.testing.assert_array_equal(again[0], first[0])
    np.testing.assert_array_equal(again[1], first[1])


@pytest.mark.parametrize('prec', ['c128', 'c64'])
def test_three_argument_plan_takes_the_weights_of_the_call(prec):
    """A plan built by the 3-argument route has all-zero DBF weights (rsp._stage2_precompute): the raw
    call's W must be the one in use -- all zeros would mean the plan's table was."""
    name = 'p16-b3-c12'
    cfg, W, ang, k = _plumbing(name)
    cube = _cube(cfg, prec)
    v8 = rsp.stage2_config(cfg)
    plan = Plan(v8, C.default_cfar_params(), C.default_cluster_params(), rsp._stage2_precompute(v8), precision=prec)
    try:
        mtd, pc = plan.process_raw_stage2(cube, W)
        zero = plan.process_raw_stage2(cube)[0]
    finally:
        plan.close()
    assert not zero.any()
    mtd_o, pc_o = _oracle(name, prec, W)
    assert np.abs(mtd).max() > 0.5 * np.abs(mtd_o).max()
    map_close(pc, pc_o, MAP_TOL[prec])
    map_close(mtd, mtd_o, MAP_TOL[prec])


@pytest.mark.parametrize('prec', ['c128', 'c64'])
def test_small_scenario_against_the_oracle(prec):
    s = scenario('small')
    W = np.asarray(s['pre_o']['DBF_coeffs_data_C'], np.complex128)
    cube = _cube(s['cfg'], prec)
    plan = Plan(s['cfg'], s['cfar'], s['clus'], s['pre_p'], precision=prec)
    try:
        mtd, pc = plan.process_raw_stage2(cube, W)
    finally:
        plan.close()
    pc_o = chain.pulse_compress(chain.dbf(cube.astype(np.complex128), W), s['pre_o'])
    map_close(pc, pc_o, MAP_TOL[prec])
    map_close(mtd, chain.mtd(pc_o, s['pre_o']), MAP_TOL[prec])


def _gated(cube, cols):
    full = np.zeros_like(cube)
    for a, b in cols:
        full[:, a - 1:b, :] = cube[:, a - 1:b, :]
    return np.concatenate([cube[:, a - 1:b, :] for a, b in cols], axis=1), full


def test_gated_raw_input(case):
    plan, cube, W = case['plan'], case['cube'], case['W']
    gated, full = _gated(cube, GATE_COLS)
    assert gated.shape[1] == 512 and plan.N == 1024
    mtd, pc = plan.process_raw_stage2(gated, W, gate_cols=GATE_COLS)
    mtd_f, pc_f = plan.process_raw_stage2(full, W)
    np.testing.assert_array_equal(pc, pc_f)
    np.testing.assert_array_equal(mtd, mtd_f)
    assert np.abs(mtd - plan.process_raw_stage2(cube, W)[0]).max() > 0      # the gating removed something
    with pytest.raises(rsp.RspError) as e:
        plan.process_raw_stage2(gated, W, gate_cols=((101, 164), (150, 341), (601, 856)))
    assert e.value.code == rsp._abi.RSP_ERR_INVALID
    with pytest.raises(rsp.RspError):
        plan.process_raw_stage2(gated[:, :500], W, gate_cols=GATE_COLS)       # 500 columns, the gates cover 512


def _same_detection(a, b):
    assert a['n_hits'] == b['n_hits'] > 0
    for key in ('mtd', 'amp', 'flags', 'threshold', 'hits'):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


@pytest.mark.parametrize('prec', ['c128', 'c64'])
def test_raw_cfar_forms_equal_the_beams_forms(prec):
    """One noise-only cube per detector (the other cases add no path to the detectors)."""
    cfg, W, ang, k = _plumbing('p16-b3-c12')
    cube = _cube(cfg, prec)
    plan = Plan(cfg, C.default_cfar_params(), C.default_cluster_params(), product_precompute(cfg, W, ang, k, C.V8_FIR),
                precision=prec)
    try:
        beams = plan.dbf(cube, W)
        _same_detection(plan.process_raw_stage2_cfar(cube, STAGE3, W=W), plan.process_stage2_cfar(beams, STAGE3))
        _same_detection(plan.process_raw_stage2_vcfar(cube, VCFAR, W=W), plan.process_stage2_vcfar(beams, VCFAR))
        # hits alone, a gated cube and the plan's own weights
        gated, full = _gated(cube, GATE_COLS)
        a = plan.process_raw_stage2_vcfar(gated, VCFAR, method='goca', gate_cols=GATE_COLS, want=('hits',))
        b = plan.process_stage2_vcfar(plan.dbf(full, W), VCFAR, method='goca', want=('hits',))
        assert sorted(a) == ['hits', 'n_hits'] and a['n_hits'] == b['n_hits'] > 0
        np.testing.assert_array_equal(a['hits'], b['hits'])
        with pytest.raises(rsp.RspError):
            plan.process_raw_stage2_cfar(cube, dict(STAGE3, refCells_R=0), W=W)
    finally:
        plan.close()


@pytest.mark.parametrize('prec', ['c128', 'c64'])
def test_end_to_end_from_a_frame_file(tmp_path, prec):
    """save_frame -> load_frame -> rsp.process_frame_stage2: the scripts' first lines in one call."""
    name = 'p16-b3-c12'
    cfg, W, ang, k = _plumbing(name)
    cube = chain.philox_noise(cfg, 1, SEED)
    path = str(tmp_path / 'frame_sim_array_1.mat')
    rsp.matio.save_frame(path, cube, servo_angle=np.zeros(cube.shape[0]))
    raw, _ = rsp.matio.load_frame(path, dtype=np.complex128 if prec == 'c128' else np.complex64)
    np.testing.assert_array_equal(raw, _cube(cfg, prec))
    mtd, pc = rsp.process_frame_stage2(raw, np.zeros(cube.shape[0]), cfg, W, precision=prec)
    mtd_o, pc_o = _oracle(name, prec, W)
    map_close(pc, pc_o, MAP_TOL[prec])
    map_close(mtd, mtd_o, MAP_TOL[prec])
    # the result of Plan.process_raw_stage2 on a plan that has the weights (test_raw_stage2_against_the_oracle)
    plan = Plan(cfg, C.default_cfar_params(), C.default_cluster_params(), product_precompute(cfg, W, ang, k, C.V8_FIR),
                precision=prec)
    try:
        mtd_p, pc_p = plan.process_raw_stage2(raw)
    finally:
        plan.close()
    np.testing.assert_array_equal(mtd, mtd_p)
    np.testing.assert_array_equal(pc, pc_p)
    # equal to the two calls in a row, and the gated form to the full-PRT call on the regated cube
    mtd2, pc2 = rsp.process_stage2_mtd(rsp.dbf_beams(raw, W, precision=prec), None, cfg, precision=prec)
    np.testing.assert_array_equal(mtd, mtd2)
    np.testing.assert_array_equal(pc, pc2)
    gated, full = _gated(raw, GATE_COLS)
    mtd_g, _ = rsp.process_frame_stage2(gated, None, cfg, W, gate_cols=GATE_COLS, precision=prec)
    np.testing.assert_array_equal(mtd_g, rsp.process_frame_stage2(full, None, cfg, W, precision=prec)[0])
    plain = rsp.process_frame_stage2(raw, None, cfg, W, conj=False, precision=prec)[0]
    map_close(plain, _oracle(name, prec, W, conj=False)[0], MAP_TOL[prec])
