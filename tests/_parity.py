"""The device-vs-oracle assertions shared by the GPU parity modules (test_gpu_parity.py,
test_slowtime_routes.py); the tolerances are documented in test_gpu_parity.py.

A `case` is a dict with: prec ('c128' / 'c64'), s (the _scen.scenario), fin / st (the oracle's
final targets and stages of the same cube), gpu / gpu_mag (Plan.process_cube with and without the
complex RD map) and optionally dets: 'some' (the oracle must have detections -- the default),
'none' (it has none, and so must the device) or 'any'.
"""
import numpy as np
import pytest

from oracle import chain

MAP_TOL = {'c128': 1e-12, 'c64': 2e-5}
MARGIN = 1e-4


def map_close(a, b, tol):
    scale = np.abs(b).max()
    err = np.abs(a - b).max()
    print('map max err / max %.3g (tol %g)' % (err / scale if scale else err, tol))
    assert err <= tol * scale, 'max err %.3g vs scale %.3g (tol %g)' % (err, scale, tol)
    if tol > 1e-9:
        rl2 = np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel())
        assert rl2 <= 1e-5, 'rel L2 %.3g' % rl2


def keys(dets):
    return [(int(d[0]), int(d[1]), int(d[2])) for d in dets]


def _gkeys(dets):
    return [(d['v_idx'], d['r_idx'], d['pair_idx']) for d in dets]


def check_rdm(case):
    map_close(case['gpu']['rdm'], case['st']['rdm'], MAP_TOL[case['prec']])


def check_cfar_map(case):
    """rdm_for_cfar_all as produced on the device (K3's S tile), not recomputed on the host."""
    map_close(case['gpu']['cfar_maps'], case['st']['S_all'], MAP_TOL[case['prec']])


def check_cfar_map_without_rdm(case):
    """K2 without the complex RD map stores the same magnitudes: the CFAR maps and the detection
    list are bit-identical to the run that also writes the RDM."""
    a, b = case['gpu_mag'], case['gpu']
    assert np.array_equal(a['cfar_maps'], b['cfar_maps']), 'max diff %g' % np.abs(a['cfar_maps'] - b['cfar_maps']).max()
    assert _gkeys(a['detections']) == _gkeys(b['detections'])


def _expected_count(case, n_oracle, n_device):
    want = case.get('dets', 'some')
    if want == 'some':
        assert n_oracle > 0
    elif want == 'none':
        assert n_oracle == 0 and n_device == 0, '%d oracle, %d device detections' % (n_oracle, n_device)


def check_detection_sets(case):
    o = set(keys(case['st']['dets']))
    g = set(_gkeys(case['gpu']['detections']))
    _expected_count(case, len(o), len(g))
    if case['prec'] == 'c128':
        assert o == g, 'CFAR decisions differ: oracle-only %r, device-only %r' % (sorted(o - g)[:8], sorted(g - o)[:8])
        return
    mg = chain.cfar_margin(case['st']['rdm'], case['s']['cfar'])
    for (v, r, p) in o ^ g:
        assert mg[v - 1, r - 1, p - 1] < MARGIN, 'CFAR decision differs at (v=%d r=%d pair=%d)' % (v, r, p)


def check_detection_order_and_estimates(case):
    pre = case['s']['pre_o']
    od = {k: (d, e) for k, d, e in zip(keys(case['st']['dets']), case['st']['dets'], case['st']['par'])}
    gd = case['gpu']['detections']
    gk = _gkeys(gd)
    assert gk == sorted(gk, key=lambda k: (k[2], k[1], k[0])), 'not in fsf find() order'
    if case['prec'] == 'c128':
        assert gk == keys(case['st']['dets'])
        for d in gd:
            raw, est = od[(d['v_idx'], d['r_idx'], d['pair_idx'])]
            assert d['amp'] == pytest.approx(raw[3], rel=1e-12)
            for f in ('Range', 'Velocity', 'Angle'):
                assert d[f] == pytest.approx(est[f], abs=1e-9), f
        return
    moved = 0
    n = 0
    for d in gd:
        k = (d['v_idx'], d['r_idx'], d['pair_idx'])
        if k not in od:
            continue
        n += 1
        raw, est = od[k]
        assert d['amp'] == pytest.approx(raw[3], rel=1e-4)
        assert d['Angle'] == pytest.approx(est['Angle'], abs=1e-3)
        dr, dv = abs(d['Range'] - est['Range']), abs(d['Velocity'] - est['Velocity'])
        if dr > 1e-6 * max(1.0, abs(est['Range'])) or dv > 1e-6:
            assert dr <= pre['deltaR'] / 8 + 1e-6 and dv <= pre['deltaV'] / 4 + 1e-9
            moved += 1
    if case.get('dets', 'some') == 'some':
        assert n > 0
    assert moved <= max(1, 0.02 * n)


def check_final_targets(case):
    fg = case['gpu']['final_targets']
    if case['prec'] == 'c128':
        fo = case['fin']
        assert len(fo) == len(fg)
        for a, b in zip(fo, fg):
            for f in ('Range', 'Velocity', 'Angle', 'Power'):
                assert b[f] == pytest.approx(a[f], rel=1e-9, abs=1e-9), f
        return
    o = set(keys(case['st']['dets']))
    g = set(_gkeys(case['gpu']['detections']))
    pre = case['s']['pre_o']
    if o == g:
        fo = case['fin']
        tol = dict(Range=pre['deltaR'] / 8, Velocity=pre['deltaV'] / 4, Angle=2e-3)
    else:   # near-threshold cells flipped: the clustering of the device's own detections
        par = [dict(Range=d['Range'], Velocity=d['Velocity'], Angle=d['Angle'], Power=d['amp'])
               for d in case['gpu']['detections']]
        fo = chain.cluster_stage2(chain.cluster_stage1(par, case['s']['clus']), case['s']['clus'])
        tol = dict(Range=1e-9, Velocity=1e-9, Angle=1e-9)
    assert len(fo) == len(fg)
    for a, b in zip(fo, fg):
        for f, t in tol.items():
            assert b[f] == pytest.approx(a[f], abs=t), f
        assert b['Power'] == pytest.approx(a['Power'], rel=1e-4)
