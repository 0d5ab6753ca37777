"""CPU preconditions of the slow-time route cases (_scen.ROUTE_CASES) that the GPU parity module
test_slowtime_routes.py leans on: the oracle alone, no device.

  * a case marked 'some' has detections, one marked 'none' has none -- in the complex128 cube and
    in the complex64-rounded cube the c64 plans process;
  * no cell under test lies within 1e-4 of its CFAR threshold in either cube, so no c64 case can
    pass by excusing a flipped decision (test_gpu_parity.py's MARGIN).

A case that misses one gets other targets, not other thresholds.

Also on the CPU, through the device-free rsp_plan_describe (rsp.plan.describe): the route of every
case and of the named configurations for a device of 256 compute units, and the plan's refusals
with their codes and messages.
"""
import copy

import numpy as np
import pytest

from oracle import chain
from rsp import _abi
from rsp.plan import describe

from _parity import MARGIN
from _scen import ROUTE_CASES, scenario, targets_for, noisy_cube, plumbing_weights

CASES = [(n, p) for n, rc in ROUTE_CASES.items() for p in rc['precs']]


def _describe(s, **kw):
    return describe(s['cfg'], s['cfar'], s['clus'], s['pre_p'], **kw)


@pytest.mark.parametrize('name,prec', CASES, ids=['%s-%s' % c for c in CASES])
def test_described_route(name, prec):
    """test_slowtime_routes.test_route's comparison, without a device."""
    sizes, got = _describe(scenario(name), precision=prec)
    want = ROUTE_CASES[name]['route'][prec]
    assert {k: got[k] for k in want} == want, got
    assert got['Ppad'] >= ROUTE_CASES[name]['P'] and got['NT'] in (1, 2, 4, 8)
    if got['kernel'] != 'tiled':
        assert 1 <= got['tiles_per_wave'] <= 4
    rc = ROUTE_CASES[name]
    assert (sizes.P, sizes.B, sizes.C, sizes.N, sizes.G) == (rc['P'], rc['B'], rc['C'], 1024, 512)
    assert sizes.elem_bytes == (16 if prec == 'c128' else 8)


# the persistent power-of-two kernel with the in-place DIF FFT (16 or more
# channels at P = 256), the persistent factored kernel with R = 4 at 3 sub-tiles per wave
_K1P = dict(kernel='persistent', transform='dif', R=0, Q=0)
NAMED = {'small': dict(_K1P, stage2_lgp=6), 'x2': dict(_K1P, stage2_lgp=7), 'p256': dict(_K1P, stage2_lgp=8),
         'x4': dict(_K1P, stage2_lgp=8),
         'reference': dict(kernel='persistent_factored', transform='factored', R=4, Q=83, tiles_per_wave=3,
                           stage2_lgp=0)}


@pytest.fixture(scope='module', params=list(NAMED))
def named(request):
    return request.param, scenario(request.param)


@pytest.mark.parametrize('prec', ['c128', 'c64'])
def test_named_configuration_routes(named, prec):
    name, s = named
    _, got = _describe(s, precision=prec)
    assert {k: got[k] for k in NAMED[name]} == NAMED[name], got
    assert 1 <= got['tiles_per_wave'] <= 4


def test_forced_tiled_routes_to_the_tiled_kernel(named):
    name, s = named
    _, dflt = _describe(s)
    _, got = _describe(s, k1_tiled=True)
    assert got['kernel'] == 'tiled' and got['tiles_per_wave'] == 0
    for k in ('transform', 'R', 'Q', 'NT', 'Ppad', 'stage2_lgp'):   # the same transform on the same tile
        assert got[k] == dflt[k]


def test_without_compute_units_the_plan_is_tiled():
    """ncu = 0 (the CU count could not be read): no persistent grid."""
    assert _describe(scenario('small'), ncu=0)[1]['kernel'] == 'tiled'


def _refused(s, code, text, **kw):
    with pytest.raises(_abi.RspError) as e:
        _describe(s, **kw)
    assert e.value.code == code
    assert text in str(e.value)


def test_p1024_complex_double_is_refused():
    _refused(scenario('d-1024'), _abi.RSP_ERR_UNSUPPORTED, 'prtNum 1024 too large', precision='c128')


def test_bad_arguments_are_refused():
    base = scenario('f-6')

    def with_cfg(**kw):
        s = copy.deepcopy(base)
        s['cfg']['Sig_Config'].update(kw)
        return s

    _refused(with_cfg(prtNum=7), _abi.RSP_ERR_UNSUPPORTED, 'odd prtNum 7 (complex64 pulse pairs are loaded as 16 B)')
    _refused(with_cfg(channel_num=33), _abi.RSP_ERR_INVALID, 'bad sizes C=33 B=4 P=6 N=1024 (1<=C<=32, 1<=B<=16)')
    s = copy.deepcopy(base)
    s['pre_p']['N_total_gate'] += 1
    _refused(s, _abi.RSP_ERR_INVALID, 'gate counts inconsistent')


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
