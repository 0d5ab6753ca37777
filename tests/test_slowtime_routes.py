"""GPU parity of every slow-time transform route the plan can take (K1 and the stage-2 column
transform), against the CPU oracle on identical inputs.

The frame chain picks one of five slow-time transforms from P = prtNum, B, C and the precision
(rsp_query_k1_route; DESIGN.md "Slow-time transform routes"); the configurations of
test_gpu_parity.py reach the persistent power-of-two kernel (P = 64, 128, 256) and the reference
frame's P = 332.  The cases of _scen.ROUTE_CASES reach the others with a default plan -- the tiled
Stockham passes (P = 16, 32, 512), the persistent factored kernel at each sub-tile count, the
tiled factored kernel (P = 166 at 4 beams; more than 16 channels), the direct DFT (P = 2 .. 1024)
-- and k_mtd_cols at LGP 4, 5, 7, 8, 9 and its direct branch.  Per case and precision:

  * Plan.k1_route() equals the case table, so that a change of the plan's heuristics cannot move
    a case off the kernel it is there to cover;
  * the assertions and tolerances of test_gpu_parity.py (_parity.py): maps, detection set,
    order, S9 estimates, final targets.  test_slowtime_route_cases.py checks on the CPU that
    the cases expected to have detections have them and that none lies within the margin in
    which a complex-single plan may flip a CFAR decision;
  * rsp_process_stage2 of the oracle's DBF output against the oracle's S6 and S7.

The bit-identity of the persistent and the tiled K1 and the queue path of the persistent cases
are test_gpu_parity.py's tests, parametrised over these cases.
"""
import ctypes as ct

import numpy as np
import pytest

from oracle import chain, precompute as oracle_precompute
from rsp import _abi, config as C
from rsp.plan import Plan, describe
from rsp.precompute import precompute as product_precompute

import _parity
from _parity import MAP_TOL, map_close
from _scen import ROUTE_CASES, scenario, targets_for, noisy_cube, plumbing_config, plumbing_weights

pytestmark = pytest.mark.gpu

CASES = [(n, p) for n, rc in ROUTE_CASES.items() for p in rc['precs']]

_cube_cache = {}


def _input_cube(name, s):
    """The noisy complex128 cube of frame 1 (one case at a time: its precisions are adjacent)."""
    if name not in _cube_cache:
        _cube_cache.clear()
        _cube_cache[name] = noisy_cube(s, targets_for(name), dtype=np.complex128)
    return _cube_cache[name]


def _device_cus():
    """Compute units of device 0, asked of the HIP runtime librsp.so is linked to (the call
    rsp_plan_create_ex makes; 63 = hipDeviceAttributeMultiprocessorCount of hip_runtime_api.h)."""
    n = ct.c_int(0)
    assert _abi.lib().hipDeviceGetAttribute(ct.byref(n), 63, 0) == 0 and n.value > 0
    return n.value


def _stage2(plan, iq, prec, pre_o, pc_o=None, mtd_o=None):
    """(device MTD, device PC, oracle MTD, oracle PC) of the beams iq [P, N, B]; pc_o / mtd_o: the
    oracle's S6 / S7 of iq where the caller has them (complex double)."""
    if prec == 'c64':   # the upload rounds the beams to complex single: the oracle takes the same
        iq = iq.astype(np.complex64).astype(np.complex128)
        pc_o = mtd_o = None
    if pc_o is None:
        pc_o = chain.pulse_compress(iq, pre_o)
    if mtd_o is None:
        mtd_o = chain.mtd(pc_o, pre_o)
    mtd, pc = plan.process_stage2(iq)
    return mtd, pc, mtd_o, pc_o


@pytest.fixture(scope='module', params=CASES, ids=['%s-%s' % c for c in CASES])
def case(request):
    name, prec = request.param
    s = scenario(name)
    cube = _input_cube(name, s)
    if prec == 'c64':
        cube = cube.astype(np.complex64)
    fin, st = chain.process_cube(cube.astype(np.complex128), s['cfg'], s['cfar'], s['clus'], s['pre_o'], keep=True)
    plan = Plan(s['cfg'], s['cfar'], s['clus'], s['pre_p'], precision=prec)
    try:
        route = plan.k1_route()
        sizes = {f: getattr(plan.sizes, f) for f, _ in _abi.Sizes._fields_}
        gpu = plan.process_cube(cube, frame_idx=1, want_rdm=True, want_cfar=True)
        gpu_mag = plan.process_cube(cube, frame_idx=1, want_rdm=False, want_cfar=True)
        s2 = _stage2(plan, st['iq'], prec, s['pre_o'], st['pc'], st['rdm'])
    finally:
        plan.close()
    st = {k: st[k] for k in ('rdm', 'S_all', 'dets', 'par')}
    yield dict(name=name, prec=prec, s=s, fin=fin, st=st, gpu=gpu, gpu_mag=gpu_mag, route=route, sizes=sizes, s2=s2,
               dets=ROUTE_CASES[name]['dets'], P=ROUTE_CASES[name]['P'])


def test_route(case):
    """The plan takes the kernel and transform the case is there for."""
    want = ROUTE_CASES[case['name']]['route'][case['prec']]
    got = case['route']
    print('%s %s: %r' % (case['name'], case['prec'], got))
    assert {k: got[k] for k in want} == want, got
    assert got['Ppad'] >= case['P'] and got['NT'] in (1, 2, 4, 8)
    if got['kernel'] != 'tiled':
        assert 1 <= got['tiles_per_wave'] <= 4
    # the device-free description for this device's CU count is the created plan's
    s = case['s']
    dsz, droute = describe(s['cfg'], s['cfar'], s['clus'], s['pre_p'], precision=case['prec'], ncu=_device_cus())
    assert droute == got
    assert {f: getattr(dsz, f) for f, _ in _abi.Sizes._fields_} == case['sizes']


def test_rdm_parity(case):
    _parity.check_rdm(case)


def test_cfar_map_parity(case):
    _parity.check_cfar_map(case)


def test_cfar_map_without_rdm(case):
    _parity.check_cfar_map_without_rdm(case)


def test_detection_sets(case):
    _parity.check_detection_sets(case)


def test_detection_order_and_estimates(case):
    _parity.check_detection_order_and_estimates(case)


def test_final_targets(case):
    _parity.check_final_targets(case)


def test_stage2_parity(case):
    """rsp_process_stage2 on the frame's beams: K1's transpose-only mode at the case's NT, K2, and
    k_mtd_cols' FFT instantiation (or direct branch) for the case's P."""
    mtd, pc, mtd_o, pc_o = case['s2']
    map_close(pc, pc_o, MAP_TOL[case['prec']])
    map_close(mtd, mtd_o, MAP_TOL[case['prec']])


@pytest.mark.parametrize('prec', ['c128', 'c64'])
@pytest.mark.parametrize('P', [128, 256])
def test_stage2_parity_lgp_7_8(P, prec):
    """k_mtd_cols at LGP 7 and 8 (the x2 and p256 pulse counts) on the small geometry."""
    cfg = plumbing_config(P, 4, 16)
    W, ang, k = plumbing_weights(cfg)
    pre_o = oracle_precompute.precompute(cfg, W, ang, k, C.V8_FIR)
    pre_p = product_precompute(cfg, W, ang, k, C.V8_FIR)
    s = dict(cfg=cfg, pre_o=pre_o)
    tg = [dict(Range=1200.0, Velocity=0.11 * cfg['Sig_Config']['wavelength'] / (2 * cfg['Sig_Config']['prt']),
               ElevationAngle=ang[1] + 1.0, SNR_dB=5.0)]
    iq = chain.dbf(noisy_cube(s, tg, dtype=np.complex128), W)
    plan = Plan(cfg, C.default_cfar_params(), C.default_cluster_params(), pre_p, precision=prec)
    try:
        route = plan.k1_route()
        mtd, pc, mtd_o, pc_o = _stage2(plan, iq, prec, pre_o)
    finally:
        plan.close()
    assert route['stage2_lgp'] == {128: 7, 256: 8}[P]
    map_close(pc, pc_o, MAP_TOL[prec])
    map_close(mtd, mtd_o, MAP_TOL[prec])


def test_p1024_complex_double_is_refused():
    """d-1024 runs in complex single only: a complex-double plan of 1024 pulses does not fit the
    stage-2 column kernel's LDS tile and is refused with a message that names prtNum."""
    s = scenario('d-1024')
    with pytest.raises(_abi.RspError) as e:
        Plan(s['cfg'], s['cfar'], s['clus'], s['pre_p'], precision='c128')
    assert e.value.code == _abi.RSP_ERR_UNSUPPORTED
    assert 'prtNum 1024' in str(e.value)
