"""The queue's band route against the all-rows route, bit for bit.

A plan whose CFAR window is the compile-time 5/5/10/10 one pulse-compresses the Doppler rows under
test, [hV, P - hV) with hV = 15, runs K3 with the cells that read a row outside them deferred,
pulse-compresses the flagged edge rows and finishes those cells (launch_batch).  A row's values do
not depend on the launch that computes them and a cell's test and S9 read the same maps in the same
order, so every result must equal, field for field, what the same plan built with
RSP_PLAN_K2_ALL_ROWS (``k2_all_rows=True``: every row in one launch, one K3) gives.  That plan is
the reference here, never the route under test.

Scenes (_band_scenes.py): a target on each of the rows hV, hV + 1, 2 hV - 1, 2 hV, P - 2 hV - 1,
P - 2 hV, P - hV - 1 in every range segment and on a K3 tile's first cell; one scene inside
[2 hV, P - 2 hV); noise alone.  test_k2_row_sets.py checks on the CPU that the oracle finds those
targets on those rows.
"""
import numpy as np
import pytest

from rsp.plan import Plan

from _band_scenes import CONFIGS, HV, band_scenario, reads_edge, scene_cube, scenes
from _scen import scenario, targets_for, noisy_cube

pytestmark = pytest.mark.gpu

F = 2
DET_FIELDS = ('v_idx', 'r_idx', 'pair_idx', 'amp', 'Range', 'Velocity', 'Angle')


class _Pair:
    """The plan under test and its all-rows reference for one configuration and precision."""

    def __init__(self, name, prec, cfar=None):
        s = band_scenario(name) if name in CONFIGS else scenario(name)
        cfar = cfar or s['cfar']
        self.band = Plan(s['cfg'], cfar, s['clus'], s['pre_p'], frames_per_launch=F, precision=prec)
        self.ref = Plan(s['cfg'], cfar, s['clus'], s['pre_p'], frames_per_launch=F, precision=prec, k2_all_rows=True)
        self.prec = prec

    def close(self):
        self.band.close()
        self.ref.close()

    def cube(self, c):
        return c if self.prec == 'c128' else c.astype(np.complex64)


_pairs = {}


@pytest.fixture(scope='module')
def pairs():
    def get(name, prec):
        if (name, prec) not in _pairs:
            _pairs[(name, prec)] = _Pair(name, prec)
        return _pairs[(name, prec)]
    yield get
    for p in _pairs.values():
        p.close()
    _pairs.clear()


def _sorted_dets(res):
    """Raw detections as sorted tuples of every field, floats by their bits."""
    key = res['detections'][0].keys() if res['detections'] else DET_FIELDS
    for f in DET_FIELDS:
        assert f in key, (f, list(key))
    return sorted(tuple(d[f] if isinstance(d[f], int) else np.float64(d[f]).tobytes() for f in DET_FIELDS)
                  for d in res['detections'])


CASES = [(n, sc) for n in CONFIGS for sc in scenes(n)]


@pytest.mark.parametrize('prec', ['c128', 'c64'])
@pytest.mark.parametrize('name,scene', CASES, ids=['%s-%s' % c for c in CASES])
def test_one_frame_equals_all_rows(pairs, name, scene, prec):
    pr = pairs(name, prec)
    cube = pr.cube(scene_cube(name, scene))
    pr.band.band_counters(reset=True)
    pr.ref.band_counters(reset=True)
    got = pr.band.process_cube(cube, frame_idx=1)
    want = pr.ref.process_cube(cube, frame_idx=1)
    cb, cr = pr.band.band_counters(), pr.ref.band_counters()
    rows = scenes(name)[scene][1]
    print('%s %s %s: %d detections, counters %s' % (name, scene, prec, len(want['detections']), cb))
    assert _sorted_dets(got) == _sorted_dets(want)
    assert got['final_targets'] == want['final_targets']
    assert cb['frames'] == 1 and cb['band_frames'] == 1, cb
    assert cr == dict(frames=1, band_frames=0, edge_rows=0, deferred_cells=0)
    if scene.startswith('row'):
        # the target's own cell or, for rows 2 hV and P - 2 hV - 1, its main lobe's next row reads an edge row
        assert any(reads_edge(v + d, pr.band.P) for v in rows for d in (-1, 0, 1))
        assert len(want['detections']) > 0
        assert cb['edge_rows'] > 0 and cb['deferred_cells'] > 0, cb
    if scene == 'interior':
        assert len(want['detections']) > 0
        assert cb['edge_rows'] == 0 and cb['deferred_cells'] == 0, cb
    assert cb['edge_rows'] <= 2 * HV * pr.band.B


@pytest.mark.parametrize('prec', ['c128', 'c64'])
@pytest.mark.parametrize('name', CONFIGS)
def test_batches_of_different_scenes_equal_all_rows(pairs, name, prec):
    """Batches of two frames with different scenes (one frame's flags must not serve the other), and
    two empty frames on the lane that held the two busiest ones: 8 frames, 4 batches over 3 lanes,
    so the last batch reuses the first one's lane."""
    pr = pairs(name, prec)
    sc = [k for k in scenes(name) if k != 'empty']
    order = [sc[0], sc[-1]] + [sc[i % len(sc)] for i in range(1, 5)] + ['empty', 'empty']
    rows = {}
    for which, plan in (('band', pr.band), ('ref', pr.ref)):
        ptrs = {}
        try:
            for k in set(order):
                ptrs[k] = plan.device_alloc(plan.cube_bytes)
                plan.upload_cube(ptrs[k], pr.cube(scene_cube(name, k)))
            plan.band_counters(reset=True)
            plan.enqueue_many([ptrs[k] for k in order], range(40, 48))
            plan.drain()
            rows[which] = plan.results_rows()
        finally:
            for p in ptrs.values():
                plan.device_free(p)
    cb = pr.band.band_counters()
    print('%s %s: %d result rows, counters %s' % (name, prec, len(rows['ref']), cb))
    assert cb['frames'] == 8 and cb['band_frames'] == 8, cb
    assert np.array_equal(rows['band'], rows['ref'], equal_nan=True)
    assert np.isfinite(rows['ref'][:, 1]).sum() > 0
    # the frames of one scene give the same rows wherever they sit in a batch
    byf = {int(f): rows['band'][rows['band'][:, 0] == f][:, 1:] for f in range(40, 48)}
    for i, k in enumerate(order):
        j = order.index(k)
        assert np.array_equal(byf[40 + i], byf[40 + j], equal_nan=True), (i, j, k)


@pytest.mark.parametrize('prec', ['c128', 'c64'])
def test_deferred_list_overflow_equals_all_rows(prec):
    """A low T_CFAR on `small` (P = 64: every row under test reads an edge row): far more deferred
    cells than the lanes' initial lists hold (1024), so the lists grow and the phases run again; more
    detections than the initial device list (4096) too."""
    s = scenario('small')
    cube = noisy_cube(s, targets_for('small'), dtype=np.complex128 if prec == 'c128' else np.complex64)
    pr = _Pair('small', prec, cfar=dict(s['cfar'], T_CFAR=1.2))
    try:
        got = pr.band.process_cube(cube, frame_idx=1)
        want = pr.ref.process_cube(cube, frame_idx=1)
        cb = pr.band.band_counters()
        print('small T = 1.2 %s: %d detections, counters %s' % (prec, len(want['detections']), cb))
        assert cb['deferred_cells'] > 1024 and len(want['detections']) > 4096, (cb, len(want['detections']))
        assert _sorted_dets(got) == _sorted_dets(want)
        assert got['final_targets'] == want['final_targets']
        # the grown lists serve the next frame in one pass, with the same result
        again = pr.band.process_cube(cube, frame_idx=2)
        assert _sorted_dets(again) == _sorted_dets(want)
    finally:
        pr.close()


@pytest.mark.parametrize('prec', ['c128', 'c64'])
def test_no_row_under_test(prec):
    """prtNum = 16 <= 2 hV: no band, the all-rows route, no zero-size launch, no detections."""
    s = scenario('s-16')
    cube = noisy_cube(s, targets_for('s-16'), dtype=np.complex128 if prec == 'c128' else np.complex64)
    plan = Plan(s['cfg'], s['cfar'], s['clus'], s['pre_p'], frames_per_launch=F, precision=prec)
    try:
        for which in ('band', 'edge'):
            rs, rec = plan.k2_row_set(which)
            assert rs == dict(n=0, base=0, split=0, gap=0, total=0, nwg=0) and len(rec) == 0
        res = plan.process_cube(cube, frame_idx=1)
        assert res['detections'] == [] and res['final_targets'] == []
        d = plan.device_alloc(plan.cube_bytes)
        try:
            plan.upload_cube(d, cube)
            plan.enqueue_many([d] * 3, range(3))
            plan.drain()
            assert all(r['n_dets'] == 0 for r in plan.results())
        finally:
            plan.device_free(d)
        assert plan.band_counters() == dict(frames=4, band_frames=0, edge_rows=0, deferred_cells=0)
    finally:
        plan.close()


def test_want_rdm_takes_all_rows(pairs):
    """A frame whose RD map is asked for needs every row: the all-rows route, and the map complete."""
    pr = pairs('small', 'c128')
    cube = scene_cube('small', 'row%d' % HV)
    pr.band.band_counters(reset=True)
    got = pr.band.process_cube(cube, frame_idx=1, want_rdm=True)
    want = pr.ref.process_cube(cube, frame_idx=1, want_rdm=True)
    assert pr.band.band_counters()['band_frames'] == 0
    assert np.array_equal(got['rdm'], want['rdm'])
    assert _sorted_dets(got) == _sorted_dets(want)
