"""CPU preconditions of the slow-time route cases (_scen.ROUTE_CASES) that the GPU parity module
test_slowtime_routes.py leans on: the oracle alone, no device.

  * a case marked 'some' has detections, one marked 'none' has none -- in the complex128 cube and
    in the complex64-rounded cube the c64 plans process;
  * no cell under test lies within 1e-4 of its CFAR threshold in either cube, so no c64 case can
    pass by excusing a flipped decision (test_gpu_parity.py's MARGIN).

A case that misses one gets other targets, not other thresholds.
"""
import numpy as np
import pytest

from oracle import chain

from _parity import MARGIN
from _scen import ROUTE_CASES, scenario, targets_for, noisy_cube, plumbing_weights


@pytest.mark.parametrize('name', list(ROUTE_CASES))
def test_route_case_preconditions(name):
    rc = ROUTE_CASES[name]
    s = scenario(name)
    sc = s['cfg']['Sig_Config']
    assert (sc['prtNum'], sc['beam_num'], sc['channel_num'], sc['point_PRT']) == (rc['P'], rc['B'], rc['C'], 1024)
    assert s['pre_o']['N_total_gate'] == s['pre_p']['N_total_gate'] == 512
    for k in ('MTD_win', 'velocity_axis', 'range_axis'):   # the product's precompute is the oracle's
        np.testing.assert_allclose(s['pre_p'][k], s['pre_o'][k], rtol=1e-13, atol=0)
    cube = noisy_cube(s, targets_for(name), dtype=np.complex128)
    for prec in rc['precs']:
        x = cube if prec == 'c128' else cube.astype(np.complex64).astype(np.complex128)
        fin, st = chain.process_cube(x, s['cfg'], s['cfar'], s['clus'], s['pre_o'], keep=True)
        n = len(st['dets'])
        mg = chain.cfar_margin(st['rdm'], s['cfar'])
        print('%s %s: %d detections, %d targets, smallest CFAR margin %.3g' % (name, prec, n, len(fin), mg.min()))
        if rc['dets'] == 'some':
            assert n > 0
        elif rc['dets'] == 'none':
            assert n == 0
        assert mg.min() >= MARGIN


def test_route_cases_cover_every_transform_by_default():
    """Every (kernel, transform) pair the plan can choose for P outside 64 / 128 / 256 has a case
    whose default plan takes it, in both precisions."""
    for prec in ('c128', 'c64'):
        got = {(rc['route'][prec]['kernel'], rc['route'][prec]['transform'])
               for rc in ROUTE_CASES.values() if prec in rc['precs']}
        assert got == {('tiled', 'stockham'), ('persistent_factored', 'factored'), ('tiled', 'factored'),
                       ('tiled', 'direct')}


def test_wide_array_weights_point_at_their_beams():
    """The synthetic weights of the 32-channel case: beam b's response peaks at its angle."""
    s = scenario('f-44-c32')
    W, ang, k = plumbing_weights(s['cfg'])
    sc = s['cfg']['Sig_Config']
    assert W.shape == (4, 32) and len(k) == 3
    for b, a in enumerate(ang):
        ph = np.exp(1j * np.deg2rad(chain.calculate_phase_shifts(a, s['cfg']['Array']['element_spacing'],
                                                                 sc['wavelength'], 32)))
        resp = np.abs(np.conj(W) @ ph)
        assert int(np.argmax(resp)) == b
