"""CPU preconditions of the K3 window cases (_scen.K3_CASES) that the GPU parity module
test_k3_windows.py leans on: the oracle and the device-free rsp_plan_describe_k3
(rsp.plan.describe_k3) alone, no device.

  * the tiling of every case and precision is the table's, the named configurations take the
    compile-time 5/5/10/10 kernel (x4 with two Doppler bands), and the windows that leave no cell
    under test describe without error;
  * every band of the described tiling has oracle hits on its first and on its last row under test
    (for `min` these are v = 1 and v = P - 2, S9's 4-point Doppler windows; for `bands-hv1` they
    include v = 63 and v = 64, where S9's rows leave the tile), and `rc17` and `min-r4` have hits on
    the first and the last range cell under test (for `min-r4` r = 1 and r = G - 2, S9's 4-point
    range windows);
  * `rc17-dense` puts more than K3_QCAP = 1024 hits into one (pair, tile) at either tile width;
  * in the complex128 cube every cell under test is at least 1e-9 from its threshold (1000 x the
    1e-12 map tolerance), so the exact comparison of the c128 detection lists is meaningful;
  * in the complex64-rounded cube at most max(2, 1 % of the hits) cells lie within MARGIN of their
    threshold, so the c64 comparison, which excuses exactly those cells, cannot hide a failure.

Each case prints what it measured (pytest -s): a changed noise stream shows as changed figures.
A case that misses a precondition gets another threshold or window, not a looser rule.
"""
import numpy as np
import pytest

from oracle import chain
from rsp.plan import describe_k3

from _parity import MARGIN, keys
from _scen import K3_CASES, scenario, k3_noise_cube, k3_oracle, k3_band_edges
from test_detection_capacity import _tile_max

PRECS = ('c128', 'c64')
CASES = [(n, p) for n in K3_CASES for p in PRECS]
EMPTY = ('empty-r', 'empty-v')
G = 512


def _describe(s, prec):
    return describe_k3(s['cfg'], s['cfar'], s['clus'], s['pre_p'], precision=prec)


@pytest.mark.parametrize('name,prec', CASES, ids=['%s-%s' % c for c in CASES])
def test_described_tiling(name, prec):
    """test_k3_windows.test_tiling's comparison, without a device (the empty windows included)."""
    assert _describe(scenario(name), prec) == K3_CASES[name]['tiling'][prec]


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('name', ['small', 'x2', 'x4', 'reference'])
def test_named_configurations_take_the_fast_kernel(name, prec):
    t = _describe(scenario(name), prec)
    assert t['fast'] and t['RT'] == (32 if prec == 'c128' else 64)
    assert t['rows'] == t['VB'] and t['n_tiles'] > 0
    # x4's 226 and the reference's 302 rows under test exceed one 48 KB tile in either precision
    assert t['n_bands'] == (2 if name in ('x4', 'reference') else 1)


def test_cases_cover_the_paths():
    """The table holds what its comment says: the fast kernel with two Doppler bands, the generic
    one with two bands and a 1-row Doppler halo, a range halo from the max(.., 2) rule, a first
    cell under test off the 4-cell grid with tile column 0 left of the map, two different divisors,
    one beam pair, and both empty regions."""
    til = {n: kc['tiling']['c128'] for n, kc in K3_CASES.items()}
    win = {n: kc['win'] for n, kc in K3_CASES.items()}
    assert til['fast-2band']['fast'] and til['fast-2band']['n_bands'] == 2
    assert not til['bands-hv1']['fast'] and til['bands-hv1']['n_bands'] == 2 and sum(win['bands-hv1'][2:]) == 1
    assert sum(win['min'][:2]) < 2 and til['min']['hR'] == 4
    assert sum(win['rc17'][:2]) % 4 and (sum(win['rc17'][:2]) & ~3) - til['rc17']['hR'] < 0
    assert win['div37'][0] != win['div37'][2] and K3_CASES['div37-b2']['B'] == 2
    assert G <= 2 * sum(win['empty-r'][:2]) and K3_CASES['empty-v']['P'] <= 2 * sum(win['empty-v'][2:])


@pytest.fixture(scope='module', params=list(K3_CASES))
def case(request):
    name = request.param
    return name, K3_CASES[name], scenario(name)


@pytest.mark.parametrize('prec', PRECS)
def test_preconditions(case, prec):
    name, kc, s = case
    P, win = kc['P'], kc['win']
    sc = s['cfg']['Sig_Config']
    assert (sc['prtNum'], sc['beam_num'], sc['channel_num'], sc['point_PRT']) == (P, kc['B'], 16, 1024)
    assert s['pre_o']['N_total_gate'] == s['pre_p']['N_total_gate'] == G
    rdm, dets, _ = k3_oracle(s, k3_noise_cube(s, prec))
    k = keys(dets)
    rc0, hV = win[0] + win[1], win[2] + win[3]
    ncells = max(P - 2 * hV, 0) * max(G - 2 * rc0, 0) * (kc['B'] - 1)
    if name in EMPTY:
        assert ncells == 0 and not k
        print('%s %s: 0 cells under test, 0 hits' % (name, prec))
        return
    mg = chain.cfar_margin(rdm, s['cfar'])
    assert np.isfinite(mg).sum() == ncells
    near = int((mg < MARGIN).sum())
    edges = k3_band_edges(P, win, kc['tiling'][prec])
    rows = np.array([v - 1 for v, _, _ in k])
    edge_hits = [(int((rows == a).sum()), int((rows == b).sum())) for a, b in edges]
    print('%s %s: %d hits of %d cells; first / last row of each band %s -> %s; %d cells with margin < %g; '
          'smallest margin %.3g' % (name, prec, len(k), ncells, edges, edge_hits, near, MARGIN, mg.min()))
    for (a, b), (na, nb) in zip(edges, edge_hits):
        assert na > 0 and nb > 0, 'no hit on band edge rows %d / %d' % (a, b)
    if name.startswith('min'):
        assert edges == [(1, P - 2)]
    if name == 'bands-hv1':
        assert edges == [(1, 63), (64, 126)]
    if name.startswith('rc17') or name == 'min-r4':
        cols = np.array([r - 1 for _, r, _ in k])
        n_lo, n_hi = int((cols == rc0).sum()), int((cols == G - rc0 - 1).sum())
        print('%s %s: %d hits at r = rc0, %d at r = G - rc0 - 1' % (name, prec, n_lo, n_hi))
        assert n_lo > 0 and n_hi > 0
    if name == 'rc17-dense':
        for rt in (32, 64):
            tm = _tile_max(k, rc0, rt)
            print('%s %s: most hits in one (pair, tile) at RT = %d: %d' % (name, prec, rt, tm))
            assert tm > 1024, 'no K3 tile past its LDS queue at RT = %d' % rt
    if prec == 'c128':
        assert mg.min() >= 1e-9
    else:
        assert near <= max(2, 0.01 * len(k)), '%d near-threshold cells of %d hits' % (near, len(k))
