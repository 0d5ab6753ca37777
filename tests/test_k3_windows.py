"""K3 (GOCA-CFAR + compaction + S9, k3_cfar) against the oracle across window shapes, Doppler
bands and tile edges: the cases of _scen.K3_CASES, each in complex double and complex single, on a
noise-only cube whose hits cover every band's edge rows and the outermost range cells
(test_k3_window_cases.py asserts that on the CPU, and that the exact c128 comparison and the
near-threshold excuse of c64 are meaningful).

Per case and precision, one plan and Plan.process_cube with the RD map and the CFAR maps:
  * Plan.k3_tiling() equals the case table: the kernel (compile-time 5/5/10/10 or generic), the
    tile and the Doppler band count the case is there for;
  * the CFAR maps equal the oracle's rdm_for_cfar_all to MAP_TOL -- also where the window leaves no
    cell under test, so no launch and no early return may leave them unwritten;
  * c128: the detection list is the oracle's, cell for cell in find() order; c64: in find() order,
    and every cell that differs lies within MARGIN of its threshold in the oracle;
  * the empty windows give no detection and no target;
  * S9: Range / Velocity / amp / Angle of the device's detections equal chain.parameter_estimation
    on the device's OWN CFAR maps and RD map (cast to double), which isolates K3's S9 from the
    rounding upstream, so both precisions take Range, Velocity to 1e-9 and amp to 1e-12; Angle to
    1e-9 in c128 and to the project's 1e-3 in c64, where the device's monopulse reads K2's float
    magnitudes.  Checked: every detection on the first or last row of a Doppler band and on the
    first or last range cell under test, plus a seeded sample of 300 of the others (`rc17-dense`:
    the sample only);
  * the run without the RD map gives the same maps and the same list (K2's other store path).
"""
import numpy as np
import pytest

from oracle import chain
from rsp.plan import Plan

from _parity import MAP_TOL, MARGIN, keys, map_close, _gkeys
from _scen import K3_CASES, scenario, k3_noise_cube, k3_oracle, k3_band_edges

pytestmark = pytest.mark.gpu

CASES = [(n, p) for n in K3_CASES for p in ('c128', 'c64')]
EMPTY = ('empty-r', 'empty-v')
N_SAMPLE = 300


@pytest.fixture(scope='module', params=CASES, ids=['%s-%s' % c for c in CASES])
def case(request):
    name, prec = request.param
    s = scenario(name)
    cube = k3_noise_cube(s, prec)
    rdm, dets, S_all = k3_oracle(s, cube)
    plan = Plan(s['cfg'], s['cfar'], s['clus'], s['pre_p'], precision=prec)
    try:
        tiling = plan.k3_tiling()
        gpu = plan.process_cube(cube, frame_idx=1, want_rdm=True, want_cfar=True)
        gpu_mag = plan.process_cube(cube, frame_idx=1, want_rdm=False, want_cfar=True)
    finally:
        plan.close()
    return dict(name=name, prec=prec, kc=K3_CASES[name], s=s, rdm=rdm, dets=dets, S_all=S_all, tiling=tiling,
                gpu=gpu, gpu_mag=gpu_mag)


def test_tiling(case):
    assert case['tiling'] == case['kc']['tiling'][case['prec']]


def test_cfar_maps(case):
    map_close(case['gpu']['cfar_maps'], case['S_all'], MAP_TOL[case['prec']])


def test_detections(case):
    want, got = keys(case['dets']), _gkeys(case['gpu']['detections'])
    print('%s %s: %d oracle, %d device detections' % (case['name'], case['prec'], len(want), len(got)))
    if case['name'] in EMPTY:
        assert want == [] and got == [] and case['gpu']['final_targets'] == []
        return
    assert len(want) > 0
    assert got == sorted(got, key=lambda k: (k[2], k[1], k[0])), 'not in fsf find() order'
    assert len(set(got)) == len(got), 'a cell listed twice'
    if case['prec'] == 'c128':
        if got != want:
            o, g = set(want), set(got)
            assert o == g, 'CFAR decisions differ: oracle-only %r, device-only %r' % (sorted(o - g)[:8], sorted(g - o)[:8])
        assert got == want
        return
    mg = chain.cfar_margin(case['rdm'], case['s']['cfar'])
    diff = set(got) ^ set(want)
    print('%d cells differ' % len(diff))
    for (v, r, p) in sorted(diff):
        assert mg[v - 1, r - 1, p - 1] < MARGIN, 'CFAR decision differs at (v=%d r=%d pair=%d), margin %.3g' % (
            v, r, p, mg[v - 1, r - 1, p - 1])


def _s9_selection(case):
    """Indices into the device list: the band-edge rows and the outermost range cells under test
    (all of them, except in the dense case), plus a seeded sample of the others."""
    kc, gk = case['kc'], _gkeys(case['gpu']['detections'])
    G = case['S_all'].shape[1]
    rc0 = kc['win'][0] + kc['win'][1]
    rows = {v for e in k3_band_edges(kc['P'], kc['win'], case['tiling']) for v in e}
    edge = [i for i, (v, r, _) in enumerate(gk) if v - 1 in rows or r - 1 in (rc0, G - rc0 - 1)]
    if case['name'] == 'rc17-dense':
        edge = []
    rest = sorted(set(range(len(gk))) - set(edge))
    rng = np.random.default_rng(7)
    pick = rng.choice(len(rest), min(N_SAMPLE, len(rest)), replace=False) if rest else []
    return edge, sorted(rest[i] for i in pick)


def test_s9_estimates(case):
    if case['name'] in EMPTY:
        assert case['gpu']['detections'] == []
        return
    gd = case['gpu']['detections']
    edge, sample = _s9_selection(case)
    print('%s %s: S9 of %d edge and %d sampled detections' % (case['name'], case['prec'], len(edge), len(sample)))
    if case['name'] != 'rc17-dense':
        assert len(edge) > 0
    idx = edge + sample
    S_dev = np.asarray(case['gpu']['cfar_maps'], np.float64)
    rdm_dev = np.asarray(case['gpu']['rdm'], np.complex128)
    arr = np.array([[gd[i]['v_idx'], gd[i]['r_idx'], gd[i]['pair_idx'],
                     S_dev[gd[i]['v_idx'] - 1, gd[i]['r_idx'] - 1, gd[i]['pair_idx'] - 1]] for i in idx], float)
    est = chain.parameter_estimation(arr, S_dev, rdm_dev, case['s']['pre_o'])
    ang_tol = 1e-9 if case['prec'] == 'c128' else 1e-3
    for i, a, e in zip(idx, arr, est):
        d = gd[i]
        where = (d['v_idx'], d['r_idx'], d['pair_idx'])
        assert d['amp'] == pytest.approx(a[3], rel=1e-12, abs=0), where
        assert d['Range'] == pytest.approx(e['Range'], abs=1e-9, rel=0), ('Range', where)
        assert d['Velocity'] == pytest.approx(e['Velocity'], abs=1e-9, rel=0), ('Velocity', where)
        assert d['Angle'] == pytest.approx(e['Angle'], abs=ang_tol, rel=0), ('Angle', where)


def test_run_without_rdm(case):
    """K2 without the complex RD map stores the same magnitudes: the same maps, the same list (for
    `rc17-dense` through the overflow pass again)."""
    a, b = case['gpu_mag'], case['gpu']
    assert np.array_equal(a['cfar_maps'], b['cfar_maps'])
    assert _gkeys(a['detections']) == _gkeys(b['detections'])
