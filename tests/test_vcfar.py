"""The Doppler CA-CFAR of the stage-2 path on the device (k_vcfar, rsp_vcfar.hip) against the numpy
restatement tests/_vcfar_ref.py.

The result is defined to the bit (include/rsp.h): flags equal, thresholds ``np.array_equal`` -- in
float64 for a complex-double plan, and equal to the float32 restatement widened to double for a
complex-single plan.  The fused call is compared with the restatement run on the device's own
amplitude map (the device-map convention of test_stage3_cfar.py).

Shapes (P, G) of the stand-alone call:
  plumbing  16 x 512: the plan's own shape
  odd       33 x 193: G % 4 = 1, odd P
  short     5 x 70: P below the halo, every window clipped on both sides
  one       1 x 9: every threshold 0
  narrow    70 x 1: a single range column
  tall      (rows + 12) x (cols + 5), rows and cols of the kernel's tile as rsp_vcfar_describe reports
            them: the map just spans two row tiles and two column tiles
The preconditions that make a case worth running are asserted on the restatement, so a change of the
seed cannot hollow a case out.
"""
import numpy as np
import pytest

import _vcfar_ref as ref
import rsp
from rsp import config as C
from rsp.plan import Plan, describe_vcfar
from rsp.precompute import precompute as product_precompute
from oracle import chain
from _parity import MAP_TOL
from _scen import SEED, plumbing_config, plumbing_weights

WINDOWS = [(4, 6, 6.0), (4, 6, 1.5), (1, 0, 1.2), (5, 2, 1.5), (12, 40, 2.0)]   # (r, g, T); the first is the script's
_TILE = describe_vcfar(1, 1, dict(refCells_V=4, guardCells_V=6, T_CFAR=6.0))
SHAPES = {'plumbing': (16, 512), 'odd': (33, 193), 'short': (5, 70), 'one': (1, 9), 'narrow': (70, 1),
          'tall': (_TILE['rows'] + 12, _TILE['cols'] + 5)}
METHODS = {'ca': ref.CA, 'goca': ref.GOCA, 'soca': ref.SOCA}
DTYPE = {'c128': np.float64, 'c64': np.float32}
_MAPS, _REF = {}, {}


def _cfar(win):
    return dict(refCells_V=win[0], guardCells_V=win[1], T_CFAR=win[2])


def _maps(shape):
    if shape not in _MAPS:
        _MAPS[shape] = ref.make_maps(*SHAPES[shape], n_maps=3, seed=SEED)
        _MAPS[shape].setflags(write=False)
    return _MAPS[shape]


def _ref(shape, win, method, prec, strict=True):
    key = (shape, win, method, prec, strict)
    if key not in _REF:
        _REF[key] = ref.local_cfar_detector(_maps(shape), _cfar(win), METHODS[method], DTYPE[prec], strict)
    return _REF[key]


# ------------------------------------------------------------------ preconditions (CPU)
def test_tall_spans_two_tiles_each_way():
    P, G = SHAPES['tall']
    d = describe_vcfar(P, G, _cfar(WINDOWS[0]))
    assert d['row_tiles'] == d['col_tiles'] == 2
    assert describe_vcfar(*SHAPES['plumbing'], _cfar(WINDOWS[4]))['halo'] == 32 <= d['max_halo']


@pytest.mark.parametrize('shape', [s for s in SHAPES if SHAPES[s][0] >= 16])
def test_preconditions(shape):
    win = WINDOWS[1]
    P, G = SHAPES[shape]
    halo = win[0] + win[1] // 2
    for prec in ('c128', 'c64'):
        counts = []
        for method in METHODS:
            f, _ = _ref(shape, win, method, prec)
            loose, _ = _ref(shape, win, method, prec, strict=False)
            frac, first, last = f.mean(), int(f[:halo].sum()), int(f[P - halo:].sum())
            ties = int((f != loose).sum())
            print(shape, prec, method, 'hits', int(f.sum()), 'of', f.size, 'first', first, 'last', last, 'ties', ties)
            assert 0.10 <= frac <= 0.40, 'fraction of flagged cells %.3f' % frac
            assert first > 0 and last > 0, 'no hit in the first / last halo rows'
            assert ties >= 2, '%d cells where > and >= differ' % ties
            counts.append(int(f.sum()))
        assert len(set(counts)) == 3, 'CA, GOCA and SOCA hit counts %r' % (counts,)


def test_halo_32_on_plumbing_has_no_reference_cells():
    a = _maps('plumbing')
    for prec in ('c128', 'c64'):
        for method in METHODS:
            f, t = _ref('plumbing', WINDOWS[4], method, prec)
            assert not t.any() and np.array_equal(f.astype(bool), a.astype(DTYPE[prec]) > 0)
    assert (a == 0).sum() == 12


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
    assert np.array_equal(res['threshold'], want_t), 'max threshold diff %g' % np.abs(res['threshold'] - want_t).max()
    want_h = ref.find_hits(amp, want_f, want_t, dtype)
    assert res['n_hits'] == len(want_h) == int(want_f.sum())
    assert np.array_equal(_rows(res['hits']), want_h), 'hit list differs from find() order'
    return want_h


@pytest.mark.gpu
@pytest.mark.parametrize('method', list(METHODS))
@pytest.mark.parametrize('win', WINDOWS, ids=lambda w: 'r%d-g%d-T%g' % w)
@pytest.mark.parametrize('shape', list(SHAPES))
def test_standalone(plan, shape, win, method):
    amp = _maps(shape)
    f, t = _ref(shape, win, method, plan.precision)
    res = plan.doppler_cfar(amp, _cfar(win), method=method)
    _check(res, amp, f, t, DTYPE[plan.precision])


@pytest.mark.gpu
def test_hits_cap_smaller_than_the_total(plan):
    win, shape = WINDOWS[1], 'odd'
    amp = _maps(shape)
    f, t = _ref(shape, win, 'ca', plan.precision)
    want = ref.find_hits(amp, f, t, DTYPE[plan.precision])
    assert len(want) > 40
    for cap in (1, 17, len(want) - 1, len(want), len(want) + 5):
        res = plan.doppler_cfar(amp, _cfar(win), hits_cap=cap)
        assert res['n_hits'] == len(want) and len(res['hits']) == min(cap, len(want))
        assert np.array_equal(_rows(res['hits']), want[:cap])
    res = plan.doppler_cfar(amp, _cfar(win), want_hits=False)
    assert res['n_hits'] == len(want) and len(res['hits']) == 0
    assert np.array_equal(res['flags'], f) and np.array_equal(res['threshold'], t)


@pytest.mark.gpu
def test_more_hits_than_the_device_list_starts_with(plan):
    """A small T on the smallest-of flags most of 64 x 2048 cells, more than the 65536 records the
    device hit list starts with: it grows to the count and the kernel runs again."""
    amp = ref.make_maps(64, 2048, n_maps=1, seed=SEED)
    cf = dict(refCells_V=1, guardCells_V=0, T_CFAR=0.05)
    f, t = ref.local_cfar_detector(amp, cf, ref.SOCA, DTYPE[plan.precision])
    assert int(f.sum()) > 65536
    _check(plan.doppler_cfar(amp, cf, method='soca'), amp, f, t, DTYPE[plan.precision])


@pytest.mark.gpu
def test_refusals_come_before_device_work(plan):
    amp = _maps('plumbing')
    for change, method in ((dict(refCells_V=0), 'ca'), (dict(guardCells_V=5), 'ca'), (dict(guardCells_V=-2), 'ca'), ({}, 3),
                           (dict(T_CFAR=float('nan')), 'ca'), (dict(T_CFAR=0.0), 'ca'), (dict(refCells_V=30), 'ca')):
        with pytest.raises(rsp.RspError) as e:
            plan.doppler_cfar(amp, dict(_cfar(WINDOWS[0]), **change), method=method)
        assert e.value.code == rsp._abi.RSP_ERR_INVALID
    with pytest.raises(rsp.RspError) as e:
        plan.doppler_cfar(amp, _cfar(WINDOWS[0]), hits_cap=-1)
    assert e.value.code == rsp._abi.RSP_ERR_INVALID
    _check(plan.doppler_cfar(amp, _cfar(WINDOWS[0])), amp, *_ref('plumbing', WINDOWS[0], 'ca', plan.precision),
           DTYPE[plan.precision])      # and the plan still works


@pytest.mark.gpu
def test_reference_geometry_planted_cells():
    """One 332 x 3404 map through the literal mirror at the script's parameters (4 / 6, T = 6; its
    method field says 'GOCA' and is ignored): exact on a full-size map, and 20 planted cells of
    amplitude 40 are among the hits."""
    prm = rsp.config.v3_cfar_params()
    amp = ref.make_maps(332, 3404, n_maps=1, seed=SEED)[:, :, 0]
    rng = np.random.default_rng(SEED + 1)
    vs, rs = rng.integers(0, 332, 20), rng.choice(3404, 20, replace=False)      # one per column
    vs[:3], rs[:2] = (0, 331, 165), (0, 3403)                                   # the map's edges too
    amp[vs, rs] = 40.0
    f, t = ref.local_cfar_detector(amp, prm, ref.CA)
    det, thr = rsp.local_cfar_detector(amp, prm)
    assert det.dtype == bool and thr.dtype == np.float64 and det.shape == thr.shape == (332, 3404)
    assert np.array_equal(det, f.astype(bool)) and np.array_equal(thr, t)
    assert det[vs, rs].all()
    assert 20 <= int(det.sum()) < 20000
    other, _ = rsp.local_cfar_detector(amp, dict(prm, method='CA'))
    assert np.array_equal(other, det)


# ------------------------------------------------------------------ fused call (GPU)
FUSED_CFAR = dict(refCells_V=4, guardCells_V=6, T_CFAR=1.5)


@pytest.mark.gpu
@pytest.mark.parametrize('prec', ['c128', 'c64'])
@pytest.mark.parametrize('P, lgp', [(16, 4), (12, 0)], ids=['stockham-16', 'direct-12'])
def test_fused(P, lgp, prec):
    cfg = plumbing_config(P, 3, 16)
    W, ang, k = plumbing_weights(cfg)
    cube = chain.philox_noise(cfg, 1, SEED)
    iq = chain.dbf(cube, W)
    if prec == 'c64':
        iq = iq.astype(np.complex64)
    G = sum(cfg['Sig_Config']['point_prt_segments'])
    p = Plan(cfg, C.default_cfar_params(), C.default_cluster_params(), product_precompute(cfg, W, ang, k, C.V8_FIR),
             precision=prec)
    try:
        assert p.k1_route()['stage2_lgp'] == lgp
        mtd0, _ = p.process_stage2(iq)
        res = p.process_stage2_vcfar(iq, FUSED_CFAR)
        goca = p.process_stage2_vcfar(iq, FUSED_CFAR, method='goca', want=('flags', 'threshold'))
        only = p.process_stage2_vcfar(iq, FUSED_CFAR, want=('hits',))
        n = p.N
        cols = ((1, 300), (301, 700), (701, n))     # the whole PRT as three gated pieces: the same frame
        gated = p.process_stage2_vcfar(iq, FUSED_CFAR, gate_cols=cols, want=('flags', 'threshold'))
    finally:
        p.close()
    assert np.array_equal(res['mtd'], mtd0)
    amp = res['amp']
    assert amp.shape == (P, G, 3) and amp.dtype == np.float64
    scale = np.abs(mtd0).max()
    err = np.abs(amp - np.abs(mtd0)).max()
    print('amp max err / max %.3g' % (err / scale))
    assert err <= MAP_TOL[prec] * scale
    if prec == 'c64':
        assert np.array_equal(amp, amp.astype(np.float32).astype(np.float64))
    f, t = ref.local_cfar_detector(amp, FUSED_CFAR, ref.CA, DTYPE[prec])
    want_h = _check(res, amp, f, t, DTYPE[prec])
    assert len(want_h) > 100
    fg, tg = ref.local_cfar_detector(amp, FUSED_CFAR, ref.GOCA, DTYPE[prec])
    assert np.array_equal(goca['flags'], fg) and np.array_equal(goca['threshold'], tg) and not np.array_equal(fg, f)
    assert sorted(only) == ['hits', 'n_hits'] and only['n_hits'] == res['n_hits']
    assert np.array_equal(only['hits'], res['hits'])
    assert np.array_equal(gated['flags'], f) and np.array_equal(gated['threshold'], t)
    det, thr = rsp.local_cfar_detector(amp[:, :, 1], FUSED_CFAR, precision=prec)
    assert det.dtype == bool and thr.dtype == np.float64 and det.shape == thr.shape == amp.shape[:2]
    assert np.array_equal(det, f[:, :, 1].astype(bool)) and np.array_equal(thr, t[:, :, 1])
