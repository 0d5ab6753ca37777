"""GPU parity of the pulse-compression kernel k2_pc over overlap-save block counts, filter lengths
and the narrow FIR's edges (_scen.K2_CASES), against the CPU oracle on identical inputs.

The named configurations and the route / K3 cases run one block per segment in most block sizes,
35 FIR taps and gate counts that are multiples of 4; the cases here run what they leave out
(test_k2_cases.py lists the conditions and proves on the CPU that the table reaches them, and holds
the oracle's preconditions).  Per case and precision:

  * Plan.k2_layout() equals rsp.plan.describe_k2 and the case table, so that a change of the cost
    model cannot move a case off the path it is there to cover;
  * K2 alone: Plan.process_stage2 of the oracle's beams (K1 only transposes there, so `pc` is K2's
    output) against the oracle's S6 per segment and per block: for every block [g0, gend) of the
    layout, max |delta| over its gates is at most MAP_TOL[prec] of the oracle's maximum over that
    block's segment -- not over the map, whose maximum is a long-segment target peak that would
    hide a 1 % error in the narrow segment's gates.  The first and last gate of every block, and
    the last gate of the map when G is no multiple of 4, are checked on their own; a failure names
    the gate.  S7 of the same call with the map metric;
  * the frame chain with and without the complex RD map: _parity's map, CFAR-map and detection-set
    assertions, and the per-block metric on the RD map;
  * two frames per launch (`w4-mb-all`, `mb-pow2`): the queue's results equal the synchronous ones.

Each test prints the measured ratio per block (pytest -s).
"""
import numpy as np
import pytest

from oracle import chain
from rsp.plan import Plan, describe_k2, K2_SEGMENTS

import _parity
from _parity import MAP_TOL, map_close
from _scen import K2_CASES, scenario, k2_summary, k2_blocks, k2_cube, k3_oracle

pytestmark = pytest.mark.gpu

PRECS = ('c128', 'c64')
CASES = [(n, p) for n in K2_CASES for p in PRECS]
TWO_FRAME_CASES = ('w4-mb-all', 'mb-pow2')


def blocks_close(got, ref, L, tol, what):
    """The per-segment, per-block metric of this module on maps [P, G, B]."""
    G = ref.shape[1]
    bad, worst = [], 0.0
    for slot, blk, g0, gend in k2_blocks(L):
        sg = L['segments'][slot]
        scale = np.abs(ref[:, sg['ga']:sg['gb'], :]).max()
        err = np.abs(got[:, g0:gend, :] - ref[:, g0:gend, :]).max(axis=(0, 2))   # per gate
        worst = max(worst, err.max() / scale)
        print('%s %s block %d, gates [%d, %d): max err / segment max %.3g; first gate %.3g, last gate %.3g (tol %g)'
              % (what, K2_SEGMENTS[slot], blk, g0, gend, err.max() / scale, err[0] / scale, err[-1] / scale, tol))
        for g in sorted({g0, gend - 1, g0 + int(np.argmax(err))} | ({G - 1} if G % 4 and gend == G else set())):
            if not err[g - g0] <= tol * scale:
                bad.append('gate %d (%s block %d, gates [%d, %d)): err %.3g = %.3g of the segment maximum'
                           % (g, K2_SEGMENTS[slot], blk, g0, gend, err[g - g0], err[g - g0] / scale))
    print('%s worst block: %.3g of its segment maximum (tol %g)' % (what, worst, tol))
    assert not bad, '%s: %s' % (what, '; '.join(bad))


@pytest.fixture(scope='module', params=CASES, ids=['%s-%s' % c for c in CASES])
def case(request):
    name, prec = request.param
    s = scenario(name)
    described = describe_k2(s['cfg'], s['cfar'], s['clus'], s['pre_p'], precision=prec)
    cube = k2_cube(s, described, prec)
    pre_o = s['pre_o']
    iq = chain.dbf(cube.astype(np.complex128), pre_o['DBF_coeffs_data_C'])
    rdm_o, dets_o, S_all = k3_oracle(s, cube)
    if prec == 'c64':   # process_stage2's upload rounds the beams to complex single: the oracle takes the same
        iq = iq.astype(np.complex64).astype(np.complex128)
    pc_o = chain.pulse_compress(iq, pre_o)
    plan = Plan(s['cfg'], s['cfar'], s['clus'], s['pre_p'], precision=prec)
    try:
        layout = plan.k2_layout()
        mtd, pc = plan.process_stage2(iq)
        gpu = plan.process_cube(cube, frame_idx=1, want_rdm=True, want_cfar=True)
        gpu_mag = plan.process_cube(cube, frame_idx=1, want_rdm=False, want_cfar=True)
    finally:
        plan.close()
    yield dict(name=name, prec=prec, s=s, described=described, layout=layout, pc=pc, mtd=mtd, pc_o=pc_o,
               st=dict(rdm=rdm_o, dets=dets_o, S_all=S_all), gpu=gpu, gpu_mag=gpu_mag, dets='some')


def test_layout(case):
    """The plan runs the instantiation, the block sizes and the block counts the case is there for."""
    print('%s %s: %r' % (case['name'], case['prec'], case['layout']))
    assert case['layout'] == case['described']
    assert k2_summary(case['layout']) == K2_CASES[case['name']]['layout'][case['prec']]


def test_pc_blocks(case):
    """K2 alone, per segment and per block."""
    blocks_close(case['pc'], case['pc_o'], case['layout'], MAP_TOL[case['prec']],
                 'K2RATIO %s %s pc' % (case['name'], case['prec']))


def test_stage2_mtd(case):
    map_close(case['mtd'], chain.mtd(case['pc_o'], case['s']['pre_o']), MAP_TOL[case['prec']])


def test_rdm_parity(case):
    _parity.check_rdm(case)


def test_rdm_blocks(case):
    """The frame chain's RD map (StoreRowK with the complex map / StoreRdm), per segment and per block."""
    blocks_close(case['gpu']['rdm'], case['st']['rdm'], case['layout'], MAP_TOL[case['prec']],
                 'K2RATIO %s %s rdm' % (case['name'], case['prec']))


def test_cfar_map_parity(case):
    _parity.check_cfar_map(case)


def test_cfar_map_without_rdm(case):
    _parity.check_cfar_map_without_rdm(case)


def test_detection_sets(case):
    _parity.check_detection_sets(case)


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('name', TWO_FRAME_CASES)
def test_two_frames_per_launch(name, prec):
    """blockIdx.y with more than one job per segment: two different cubes in one launch give the
    synchronous results."""
    s = scenario(name)
    plan = Plan(s['cfg'], s['cfar'], s['clus'], s['pre_p'], frames_per_launch=2, precision=prec)
    L = plan.k2_layout()
    cubes = [k2_cube(s, L, prec, frame_idx=f) for f in (1, 2)]
    ptrs = [plan.device_alloc(plan.cube_bytes) for _ in cubes]
    try:
        for p, c in zip(ptrs, cubes):
            plan.upload_cube(p, c)
        for f, p in enumerate(ptrs):
            plan.enqueue(p, f + 1)
        plan.drain()
        res = plan.results()
        assert [r['frame_idx'] for r in res] == [1, 2]
        for f, c in enumerate(cubes):
            sync = plan.process_cube(c, frame_idx=f + 1)
            print('%s %s frame %d: %d detections, %d final targets' % (name, prec, f + 1, res[f]['n_dets'],
                                                                        len(res[f]['final_targets'])))
            assert res[f]['n_dets'] == len(sync['detections'])
            assert res[f]['final_targets'] == sync['final_targets']
        assert res[0]['n_dets'] + res[1]['n_dets'] > 0
    finally:
        for p in ptrs:
            plan.device_free(p)
        plan.close()
