"""The cross GOCA-CFAR map detector on the device (k_xcfar, rsp_xcfar.hip) against the numpy
restatement tests/_xcfar_ref.py.

The result is defined to the bit (include/rsp.h): every comparison is ``np.array_equal`` -- in float64
for a complex-double plan, and with the float32 restatement widened to double for a complex-single
plan.  The fused calls are compared with the restatement run on the device's own amplitude map (the
device-map convention of test_stage3_cfar.py).  On the frame chain the flagged cells are the frame's
detections, with no near-threshold excuse: the same map and the same arithmetic (rsp_k3_arith.h).

Shapes (P, G) of the stand-alone call, hR = rR + gR and hV = rV + gV of the window:
  plumbing  16 x 512: the plan's own shape
  odd       33 x 193: G % 4 = 1, odd P (rows that do not start on 16 bytes: the one-element loads)
  bare      (2 hV + 1) x (2 hR + 1): one cell under test
  empty-v   2 hV x 64, empty-r 40 x 2 hR: no cell under test; all +Inf, no hits
  one       1 x 1
  tall      (rows + 5) x (cols + 5), rows and cols of the kernel's tile as rsp_xcfar_describe reports
            them: the map just spans two row tiles and two column tiles
  maxhalo   70 x 140 at the window 40/24/20/12 alone: hR = 64, hV = 32, the envelope's corner
Every window runs with its own T and with T = 1.5, where the maps' planted ties decide ``>`` against
``>=``.  The preconditions that make a case worth running are asserted on the restatement, so a change
of the seed cannot hollow a case out.
"""
import numpy as np
import pytest

import _xcfar_ref as ref
import rsp
from rsp import config as C
from rsp.plan import Plan, describe_xcfar
from rsp.precompute import precompute as product_precompute
from oracle import chain
from _scen import SEED, plumbing_config, plumbing_weights, scenario, k3_noise_cube

WINDOWS = [(5, 10, 5, 10, 1.0), (2, 1, 2, 1, 1.2), (3, 2, 1, 0, 1.3), (1, 0, 4, 3, 1.3), (8, 4, 2, 1, 1.2)]
MAXHALO = (40, 24, 20, 12, 1.2)
_TILE = describe_xcfar(1, 1, ref.cfar_dict(WINDOWS[0]))
SHAPES = ('plumbing', 'odd', 'bare', 'empty-v', 'empty-r', 'one', 'tall')
DTYPE = {'c128': np.float64, 'c64': np.float32}
TIE_T = 1.5
_MAPS, _REF = {}, {}


def _shape(shape, win):
    hR, hV = win[0] + win[1], win[2] + win[3]
    return {'plumbing': (16, 512), 'odd': (33, 193), 'bare': (2 * hV + 1, 2 * hR + 1), 'empty-v': (2 * hV, 64),
            'empty-r': (40, 2 * hR), 'one': (1, 1), 'tall': (_TILE['rows'] + 5, _TILE['cols'] + 5), 'maxhalo': (70, 140)}[shape]


def _maps(shape, win):
    key = (shape, win[:4])
    if key not in _MAPS:
        _MAPS[key] = ref.make_maps(*_shape(shape, win), n_maps=3, seed=SEED, cfar=ref.cfar_dict(win))
        _MAPS[key].setflags(write=False)
    return _MAPS[key]


def _ref(shape, win, prec, strict=True):
    key = (shape, win, prec, strict)
    if key not in _REF:
        _REF[key] = ref.goca_cfar_maps(_maps(shape, win), ref.cfar_dict(win), DTYPE[prec], strict)
    return _REF[key]


def _cases():
    out = [(s, w[:4] + (T,)) for s in SHAPES for w in WINDOWS for T in (w[4], TIE_T)]
    return out + [('maxhalo', MAXHALO), ('maxhalo', MAXHALO[:4] + (TIE_T,))]


_ID = lambda c: '%s-%d-%d-%d-%d-T%g' % ((c[0],) + c[1])   # noqa: E731


# ------------------------------------------------------------------ preconditions (CPU)
def test_tall_spans_two_tiles_each_way():
    for w in WINDOWS:
        d = describe_xcfar(*_shape('tall', w), ref.cfar_dict(w))
        assert d['row_tiles'] == d['col_tiles'] == 2 and d['r0'] <= d['r1'] and d['v0'] <= d['v1']
    d = describe_xcfar(70, 140, ref.cfar_dict(MAXHALO))
    assert (d['hR'], d['hV']) == (d['max_hR'], d['max_hV']) == (64, 32)


def _under_test(P, G, win):
    r0, r1, v0, v1 = ref.cells_under_test(P, G, ref.cfar_dict(win))
    return (r1 - r0) * (v1 - v0)


PRE = [(s, w) for s in ('odd', 'plumbing') for w in WINDOWS if _under_test(*_shape(s, w), w) >= 400]


@pytest.mark.parametrize('shape, win', PRE, ids=[_ID(c) for c in PRE])
def test_preconditions(shape, win):
    P, G = _shape(shape, win)
    cfar = ref.cfar_dict(win)
    r0, r1, v0, v1 = ref.cells_under_test(P, G, cfar)
    for prec in ('c128', 'c64'):
        f, t = _ref(shape, win, prec)
        cut = f[v0:v1, r0:r1]
        frac = cut.mean()
        by_slice = np.zeros(4, int)
        for b in range(3):
            which = ref.deciding_slice(_maps(shape, win)[:, :, b], cfar, DTYPE[prec])
            by_slice += np.bincount(which[cut[:, :, b] > 0], minlength=4)
        tied = dict(cfar, T_CFAR=TIE_T)
        ties = int((ref.goca_cfar_maps(_maps(shape, win), tied, DTYPE[prec])[0] !=
                    ref.goca_cfar_maps(_maps(shape, win), tied, DTYPE[prec], strict=False)[0]).sum())
        print(shape, win, prec, 'flagged %.3f of %d' % (frac, cut.size), 'decided by slice', by_slice.tolist(), 'ties', ties)
        assert 0.05 <= frac <= 0.40, 'fraction of flagged cells %.3f' % frac
        assert by_slice.min() >= 5, 'hits decided by each slice %r' % (by_slice.tolist(),)
        assert cut[0].any() and cut[-1].any(), 'no hit in the first / last row under test'
        if win[0] + win[1] <= 5:
            assert cut[:, 0].any() and cut[:, -1].any(), 'no hit in the first / last column under test'
        assert ties >= 2, '%d cells where > and >= differ' % ties
        assert not f[:v0].any() and not f[v1:].any() and not f[:, :r0].any() and not f[:, r1:].any()


def test_preconditions_cover_the_issue_cases():
    assert ('odd', WINDOWS[2]) in PRE and ('plumbing', WINDOWS[1]) in PRE and ('odd', WINDOWS[0]) in PRE


def test_maxhalo_has_a_hit_and_a_miss():
    for prec in ('c128', 'c64'):
        f, t = _ref('maxhalo', MAXHALO, prec)
        cut = f[32:38, 64:76]
        assert np.isfinite(t).sum() == 3 * 72 and 0 < int(cut.sum()) < cut.size


# ------------------------------------------------------------------ stand-alone call (GPU)
@pytest.fixture(scope='module', params=['c128', 'c64'])
def plan(request):
    cfg = plumbing_config(16, 3, 16)
    W, ang, k = plumbing_weights(cfg)
    p = Plan(cfg, C.default_cfar_params(), C.default_cluster_params(), product_precompute(cfg, W, ang, k, C.V8_FIR),
             precision=request.param)
    yield p
    p.close()


def _rows(h):
    return np.column_stack([h['v_idx'], h['r_idx'], h['beam_idx'], h['amp'], h['threshold']]) if len(h) else np.zeros((0, 5))


def _check(res, amp, want_f, want_t, dtype):
    assert res['flags'].dtype == np.uint8 and res['threshold'].dtype == np.float64
    assert res['flags'].shape == res['threshold'].shape == amp.shape
    assert np.array_equal(res['flags'], want_f), '%d flags differ' % int((res['flags'] != want_f).sum())
    assert np.array_equal(res['threshold'], want_t), '%d thresholds differ' % int((res['threshold'] != want_t).sum())
    want_h = ref.find_hits(amp, want_f, want_t, dtype)
    assert res['n_hits'] == len(want_h) == int(want_f.sum())
    assert np.array_equal(_rows(res['hits']), want_h), 'hit list differs from find() order'
    return want_h


@pytest.mark.gpu
@pytest.mark.parametrize('shape, win', _cases(), ids=[_ID(c) for c in _cases()])
def test_standalone(plan, shape, win):
    amp = _maps(shape, win)
    f, t = _ref(shape, win, plan.precision)
    res = plan.cross_cfar(amp, ref.cfar_dict(win))
    _check(res, amp, f, t, DTYPE[plan.precision])
    if shape in ('empty-v', 'empty-r', 'one'):
        assert res['n_hits'] == 0 and np.isposinf(res['threshold']).all()


@pytest.mark.gpu
def test_over_envelope_halo_on_a_map_without_cells_under_test(plan):
    amp = _maps('plumbing', WINDOWS[0])
    res = plan.cross_cfar(amp, ref.cfar_dict((100, 200, 30, 20, 1.0)))
    assert res['n_hits'] == 0 and not res['flags'].any() and np.isposinf(res['threshold']).all()


@pytest.mark.gpu
def test_hits_cap_smaller_than_the_total(plan):
    shape, win = 'odd', WINDOWS[2]
    amp = _maps(shape, win)
    f, t = _ref(shape, win, plan.precision)
    want = ref.find_hits(amp, f, t, DTYPE[plan.precision])
    assert len(want) > 40
    for cap in (1, 17, len(want) - 1, len(want), len(want) + 5):
        res = plan.cross_cfar(amp, ref.cfar_dict(win), hits_cap=cap)
        assert res['n_hits'] == len(want) and len(res['hits']) == min(cap, len(want))
        assert np.array_equal(_rows(res['hits']), want[:cap])
    res = plan.cross_cfar(amp, ref.cfar_dict(win), want_hits=False)
    assert res['n_hits'] == len(want) and len(res['hits']) == 0
    assert np.array_equal(res['flags'], f) and np.array_equal(res['threshold'], t)


@pytest.mark.gpu
def test_a_second_call_of_another_shape_and_window(plan):
    """The plan's device buffers are reused across calls: a larger map first, a smaller one with another
    window second, and back."""
    seq = [('plumbing', WINDOWS[1]), ('tall', WINDOWS[4]), ('odd', WINDOWS[0]), ('bare', WINDOWS[3]), ('plumbing', WINDOWS[1])]
    for shape, win in seq:
        amp = _maps(shape, win)
        _check(plan.cross_cfar(amp, ref.cfar_dict(win)), amp, *_ref(shape, win, plan.precision), DTYPE[plan.precision])


@pytest.mark.gpu
def test_refusals_come_before_device_work(plan):
    amp = _maps('plumbing', WINDOWS[1])
    for change in (dict(refCells_R=0), dict(refCells_V=0), dict(guardCells_R=-1), dict(guardCells_V=-1),
                   dict(T_CFAR=float('nan')), dict(T_CFAR=0.0), dict(refCells_R=60, guardCells_R=5)):
        with pytest.raises(rsp.RspError) as e:
            plan.cross_cfar(amp, dict(ref.cfar_dict(WINDOWS[1]), **change))
        assert e.value.code == rsp._abi.RSP_ERR_INVALID
    with pytest.raises(rsp.RspError) as e:
        plan.cross_cfar(amp, ref.cfar_dict(WINDOWS[1]), hits_cap=-1)
    assert e.value.code == rsp._abi.RSP_ERR_INVALID
    _check(plan.cross_cfar(amp, ref.cfar_dict(WINDOWS[1])), amp, *_ref('plumbing', WINDOWS[1], plan.precision),
           DTYPE[plan.precision])      # and the plan still works


@pytest.mark.gpu
def test_module_level_call():
    win = WINDOWS[2]
    amp = _maps('odd', win)[:, :, 0]
    for prec in ('c128', 'c64'):
        det, thr = rsp.goca_cfar_maps(amp, ref.cfar_dict(win), precision=prec)
        f, t = ref.goca_cfar_maps(amp, ref.cfar_dict(win), DTYPE[prec])
        assert det.dtype == bool and thr.dtype == np.float64 and det.shape == thr.shape == amp.shape
        assert np.array_equal(det, f.astype(bool)) and np.array_equal(thr, t)


# ------------------------------------------------------------------ stage 2 (GPU)
FUSED = ref.cfar_dict((3, 2, 2, 1, 1.3))


@pytest.mark.gpu
@pytest.mark.parametrize('prec', ['c128', 'c64'])
def test_stage2(prec):
    cfg = plumbing_config(16, 3, 16)
    W, ang, k = plumbing_weights(cfg)
    cube = chain.philox_noise(cfg, 1, SEED)
    if prec == 'c64':
        cube = cube.astype(np.complex64)
    p = Plan(cfg, C.default_cfar_params(), C.default_cluster_params(), product_precompute(cfg, W, ang, k, C.V8_FIR),
             precision=prec)
    try:
        iq = p.dbf(cube, W)
        mtd0, _ = p.process_stage2(iq)
        res = p.process_stage2_xcfar(iq, FUSED)
        only = p.process_stage2_xcfar(iq, FUSED, want=('hits',))
        n = p.N
        cols = ((1, 300), (301, 700), (701, n))     # the whole PRT as three gated pieces: the same frame
        gated = p.process_stage2_xcfar(iq, FUSED, gate_cols=cols, want=('flags', 'threshold'))
        raw = p.process_raw_stage2_xcfar(cube, FUSED, W=W)
    finally:
        p.close()
    assert np.array_equal(res['mtd'], mtd0)
    amp = res['amp']
    assert amp.shape == (16, 512, 3) and amp.dtype == np.float64
    if prec == 'c64':
        assert np.array_equal(amp, amp.astype(np.float32).astype(np.float64))
    f, t = ref.goca_cfar_maps(amp, FUSED, DTYPE[prec])
    want_h = _check(res, amp, f, t, DTYPE[prec])
    assert len(want_h) > 100 and not f.all()
    assert sorted(only) == ['hits', 'n_hits'] and only['n_hits'] == res['n_hits']
    assert np.array_equal(only['hits'], res['hits'])
    assert np.array_equal(gated['flags'], f) and np.array_equal(gated['threshold'], t)
    for key in ('mtd', 'amp', 'flags', 'threshold', 'hits'):
        assert np.array_equal(raw[key], res[key]), key
    assert raw['n_hits'] == res['n_hits']


# ------------------------------------------------------------------ the frame chain (GPU)
K3 = [(n, p) for n in ('div37', 'rc17', 'bands-hv1', 'fast-2band', 'empty-v') for p in ('c128', 'c64')]


@pytest.mark.gpu
@pytest.mark.parametrize('name, prec', K3, ids=['%s-%s' % c for c in K3])
def test_frame_chain_threshold_maps(name, prec):
    s = scenario(name)
    cube = k3_noise_cube(s, prec)
    plan = Plan(s['cfg'], s['cfar'], s['clus'], s['pre_p'], precision=prec)
    try:
        with pytest.raises(rsp.RspError) as e:
            plan.last_cfar_threshold()                      # a fresh plan
        assert e.value.code == rsp._abi.RSP_ERR_INVALID and 'did not ask for cfar_maps' in str(e.value)
        plain = plan.process_cube(cube, frame_idx=1)
        assert 'cfar_threshold' not in plain and 'cfar_flags' not in plain and 'cfar_maps' not in plain
        out = plan.process_cube(cube, frame_idx=1, want_threshold=True)
        again = plan.last_cfar_threshold()
        plan.process_cube(cube, frame_idx=1)                # a frame that did not ask for the maps
        with pytest.raises(rsp.RspError) as e:
            plan.last_cfar_threshold()
        assert e.value.code == rsp._abi.RSP_ERR_INVALID and 'did not ask for cfar_maps' in str(e.value)
    finally:
        plan.close()
    S, flags, thr = out['cfar_maps'], out['cfar_flags'], out['cfar_threshold']
    assert S.shape == flags.shape == thr.shape == (plan.P, plan.G, plan.B - 1)
    f, t = ref.goca_cfar_maps(S, s['cfar'], DTYPE[prec])
    assert np.array_equal(thr, t) and np.array_equal(flags, f)
    dets = out['detections']
    assert [(d['v_idx'], d['r_idx'], d['pair_idx']) for d in dets] == [(d['v_idx'], d['r_idx'], d['pair_idx'])
                                                                       for d in plain['detections']]
    want = ref.find_hits(S, flags, thr, DTYPE[prec])        # (pair, r, v) order
    got = np.array([(d['v_idx'], d['r_idx'], d['pair_idx'], d['amp']) for d in dets], float).reshape(-1, 4)
    print('%s %s: %d detections, %d flagged cells' % (name, prec, len(got), len(want)))
    assert np.array_equal(got, want[:, :4]), 'the flagged cells are not the frame\'s detections'
    assert (len(got) == 0) == (name == 'empty-v')
    assert np.array_equal(again['flags'], flags) and np.array_equal(again['threshold'], thr)
    assert again['n_hits'] == len(got) and np.array_equal(_rows(again['hits'])[:, :4], got)
