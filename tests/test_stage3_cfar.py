"""The stage-3 range CFAR of the stage-2 path on the device (k_s3_cfar, rsp_stage3.hip) against the
numpy restatement tests/_stage3_ref.py.

The result is defined to the bit (include/rsp.h): flags equal, thresholds ``np.array_equal`` -- in
float64 for a complex-double plan, and equal to the float32 restatement widened to double for a
complex-single plan.  The fused call is compared with the restatement run on the device's own
amplitude map (the device-map convention of test_k3_windows.py: a last-bit difference in a
magnitude may legitimately flip a cell at its threshold).

Shapes of the stand-alone call (P, segments, first column of the zero stretch):
  plumbing  P = 16, segments (64, 192, 256): the plan's own shape, rsp_stage3_cfar
  odd       P = 33, segments (38, 60, 94): the narrow segment is exactly 2 (s + r) for r + s = 19,
            P is odd, the segment boundaries fall off a multiple of 4 (rsp_stage3_cfar_shape)
  chunk     one segment of CHUNK + 66 = 322 columns: just over one range chunk of the kernel, the
            zero stretch and the windows of the cells around column CHUNK span two chunks, and
            G % 4 = 2 takes the kernel's unvectorised stores
The preconditions that make a case worth running (hits at the segments' edges, ties at 0 >= 0,
greatest-of and smallest-of differing) are asserted on the restatement, so a change of the seed
cannot hollow a case out.
"""
import numpy as np
import pytest

import _stage3_ref as ref
import rsp
from rsp import config as C
from rsp.plan import Plan, describe_stage3
from rsp.precompute import precompute as product_precompute
from oracle import chain
from _parity import MAP_TOL
from _scen import SEED, plumbing_config, plumbing_weights

CHUNK = 256
SHAPES = {'plumbing': (16, (64, 192, 256), 256 + 30), 'odd': (33, (38, 60, 94), 98 + 20),
          'chunk': (16, (CHUNK + 66, 0, 0), CHUNK - 26)}
WINDOWS = [(5, 14, 3.0), (5, 14, 1.5), (1, 0, 1.2), (3, 1, 1.5), (4, 15, 2.0)]   # (r, s, T)
DTYPE = {'c128': np.float64, 'c64': np.float32}
_MAPS, _REF = {}, {}


def _cfar(win, method, z):
    return dict(refCells_R=win[0], saveCells_R=win[1], T_CFAR=win[2], CFARmethod_R=method, MTD_0v_num=z)


def _maps(shape):
    if shape not in _MAPS:
        P, segs, za = SHAPES[shape]
        _MAPS[shape] = ref.make_maps(P, segs, za, n_maps=3, seed=SEED)
        _MAPS[shape].setflags(write=False)
    return _MAPS[shape]


def _ref(shape, win, method, z, prec, strict=False):
    key = (shape, win, method, z, prec, strict)
    if key not in _REF:
        _REF[key] = ref.local_execute_cfar(_maps(shape), _cfar(win, method, z), SHAPES[shape][1], DTYPE[prec], strict)
    return _REF[key]


def _notches(P):
    return (0, 1, P)      # MTD_0v_num: row zc alone, three rows, every row


# ------------------------------------------------------------------ preconditions (CPU)
@pytest.mark.parametrize('win', WINDOWS, ids=lambda w: 'r%d-s%d-T%g' % w)
@pytest.mark.parametrize('shape', list(SHAPES))
def test_preconditions(shape, win):
    P, segs, _ = SHAPES[shape]
    H = win[0] + win[1]
    for prec in ('c128', 'c64'):
        counts = []
        for method in (0, 1):
            f, _ = _ref(shape, win, method, 1, prec)
            strict, _ = _ref(shape, win, method, 1, prec, strict=True)
            first = last = c = 0
            for n in segs:
                if n:
                    first += int(f[:, c:c + H].sum())
                    last += int(f[:, c + n - H:c + n].sum())
                c += n
            ties = int((f != strict).sum())
            print(shape, win, prec, 'method', method, 'hits', int(f.sum()), 'first', first, 'last', last, 'ties', ties)
            assert first > 0 and last > 0, 'no hit in the first / last s + r columns of a segment'
            assert 12 <= ties <= 50, '%d cells where >= and > differ' % ties
            counts.append(int(f.sum()))
        assert counts[0] != counts[1], 'greatest-of and smallest-of give the same hit count'
    every, _ = _ref(shape, win, 0, P, 'c128')
    assert not every.any()


def test_chunk_case_is_just_over_one_chunk():
    d = describe_stage3(16, SHAPES['chunk'][1], _cfar(WINDOWS[0], 0, 1))
    assert d['chunk'] == CHUNK and CHUNK < d['G'] < 2 * CHUNK and d['G'] % 4 != 0
    # hits whose windows span the two chunks: cells within s + r of column CHUNK
    f, _ = _ref('chunk', WINDOWS[1], 0, 1, 'c128')
    assert f[:, CHUNK - 19:CHUNK + 19].any()


# ------------------------------------------------------------------ stand-alone call (GPU)
@pytest.fixture(scope='module', params=['c128', 'c64'])
def plan(request):
    cfg = plumbing_config(16, 3, 16)
    W, ang, k = plumbing_weights(cfg)
    p = Plan(cfg, C.default_cfar_params(), C.default_cluster_params(), product_precompute(cfg, W, ang, k, C.V8_FIR),
             precision=request.param)
    yield p
    p.close()


def _check(res, amp, want_f, want_t, dtype):
    assert res['flags'].dtype == np.uint8 and res['threshold'].dtype == np.float64
    assert res['flags'].shape == res['threshold'].shape == amp.shape
    assert np.array_equal(res['flags'], want_f), '%d flags differ' % int((res['flags'] != want_f).sum())
    assert np.array_equal(res['threshold'], want_t), 'max threshold diff %g' % np.abs(res['threshold'] - want_t).max()
    want_h = ref.find_hits(amp, want_f, want_t, dtype)
    assert res['n_hits'] == len(want_h) == int(want_f.sum())
    h = res['hits']
    got = np.column_stack([h['v_idx'], h['r_idx'], h['beam_idx'], h['amp'], h['threshold']]) if len(h) else np.zeros((0, 5))
    assert np.array_equal(got, want_h), 'hit list differs from find() order'
    return want_h


@pytest.mark.gpu
@pytest.mark.parametrize('method', [0, 1], ids=['go', 'so'])
@pytest.mark.parametrize('win', WINDOWS, ids=lambda w: 'r%d-s%d-T%g' % w)
@pytest.mark.parametrize('shape', list(SHAPES))
def test_standalone(plan, shape, win, method):
    P, segs, _ = SHAPES[shape]
    amp = _maps(shape)
    for z in _notches(P):
        f, t = _ref(shape, win, method, z, plan.precision)
        res = plan.stage3_cfar(amp, _cfar(win, method, z), segments=None if shape == 'plumbing' else segs)
        _check(res, amp, f, t, DTYPE[plan.precision])


@pytest.mark.gpu
def test_hits_cap_smaller_than_the_total(plan):
    win, shape = WINDOWS[1], 'odd'
    P, segs, _ = SHAPES[shape]
    amp = _maps(shape)
    f, t = _ref(shape, win, 0, 1, plan.precision)
    want = ref.find_hits(amp, f, t, DTYPE[plan.precision])
    assert len(want) > 40
    for cap in (1, 17, len(want) - 1, len(want), len(want) + 5):
        res = plan.stage3_cfar(amp, _cfar(win, 0, 1), segments=segs, hits_cap=cap)
        h = res['hits']
        assert res['n_hits'] == len(want) and len(h) == min(cap, len(want))
        got = np.column_stack([h['v_idx'], h['r_idx'], h['beam_idx'], h['amp'], h['threshold']])
        assert np.array_equal(got, want[:cap])
    res = plan.stage3_cfar(amp, _cfar(win, 0, 1), segments=segs, want_hits=False)
    assert res['n_hits'] == len(want) and len(res['hits']) == 0


@pytest.mark.gpu
def test_more_hits_than_the_device_list_starts_with(plan):
    """A small T on the smallest-of flags most of 64 x 2048 cells, more than the 65536 records the
    device hit list starts with: it grows to the count and the kernel runs again."""
    segs = (0, 0, 2048)
    amp = ref.make_maps(64, segs, 100, n_maps=1, seed=SEED)
    cf = dict(refCells_R=1, saveCells_R=0, T_CFAR=0.05, CFARmethod_R=1, MTD_0v_num=0)
    f, t = ref.local_execute_cfar(amp, cf, segs, DTYPE[plan.precision])
    assert int(f.sum()) > 100000
    _check(plan.stage3_cfar(amp, cf, segments=segs), amp, f, t, DTYPE[plan.precision])


@pytest.mark.gpu
def test_refusals_come_before_device_work(plan):
    amp = _maps('plumbing')
    for change in (dict(refCells_R=0), dict(CFARmethod_R=3), dict(T_CFAR=float('nan')), dict(saveCells_R=90),
                   dict(refCells_R=20, saveCells_R=20)):     # 2 * 40 > the 64-column narrow segment
        with pytest.raises(rsp.RspError) as e:
            plan.stage3_cfar(amp, dict(_cfar(WINDOWS[0], 0, 1), **change))
        assert e.value.code == rsp._abi.RSP_ERR_INVALID


@pytest.mark.gpu
def test_reference_geometry_notch_and_flags():
    """332 x 3404 (segments 228, 723, 2453), window 5 / 14, T = 3, MTD_0v_num = 14: rows 153..181 are
    the notch, flags and thresholds exact on a full-size map (through rsp.local_execute_cfar's plan
    of the debug script's config, shared with process_stage2_mtd)."""
    cfg = rsp.debug_v3_config()
    cf = rsp.config.debug_v2_cfar_config(cfg)
    segs = (228, 723, 2453)
    amp = ref.make_maps(332, segs, 1000, n_maps=1, seed=SEED)[:, :, 0]
    f, t = ref.local_execute_cfar(amp, cf, segs)
    flag, thr = rsp.local_execute_cfar(amp, cf, cfg)
    assert flag.dtype == thr.dtype == np.float64 and flag.shape == thr.shape == (332, 3404)
    assert not flag[152:181].any() and not thr[152:181].any()
    assert thr[151].all() and thr[181].all()
    assert np.array_equal(flag, f) and np.array_equal(thr, t)
    assert 1000 < int(f.sum()) < 20000


# ------------------------------------------------------------------ fused call (GPU)
FUSED_CFAR = dict(refCells_R=5, saveCells_R=14, T_CFAR=1.5, CFARmethod_R=0, MTD_0v_num=1)


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
    segs = tuple(cfg['Sig_Config']['point_prt_segments'])
    p = Plan(cfg, C.default_cfar_params(), C.default_cluster_params(), product_precompute(cfg, W, ang, k, C.V8_FIR),
             precision=prec)
    try:
        assert p.k1_route()['stage2_lgp'] == lgp
        mtd0, _ = p.process_stage2(iq)
        res = p.process_stage2_cfar(iq, FUSED_CFAR)
        only = p.process_stage2_cfar(iq, FUSED_CFAR, want=('hits',))
        n = p.N
        cols = ((1, 300), (301, 700), (701, n))     # the whole PRT as three gated pieces: the same frame
        gated = p.process_stage2_cfar(iq, FUSED_CFAR, gate_cols=cols, want=('flags', 'threshold'))
    finally:
        p.close()
    assert np.array_equal(res['mtd'], mtd0)
    amp = res['amp']
    assert amp.shape == (P, sum(segs), 3) and amp.dtype == np.float64
    scale = np.abs(mtd0).max()
    err = np.abs(amp - np.abs(mtd0)).max()
    print('amp max err / max %.3g' % (err / scale))
    assert err <= MAP_TOL[prec] * scale
    if prec == 'c64':
        assert np.array_equal(amp, amp.astype(np.float32).astype(np.float64))
    f, t = ref.local_execute_cfar(amp, FUSED_CFAR, segs, DTYPE[prec])
    want_h = _check(res, amp, f, t, DTYPE[prec])
    assert len(want_h) > 100
    assert sorted(only) == ['hits', 'n_hits'] and only['n_hits'] == res['n_hits']
    assert np.array_equal(only['hits'], res['hits'])
    assert np.array_equal(gated['flags'], f) and np.array_equal(gated['threshold'], t)
    flag, thr = rsp.local_execute_cfar(amp[:, :, 1], FUSED_CFAR, cfg, precision=prec)
    assert flag.dtype == thr.dtype == np.float64 and flag.shape == thr.shape == amp.shape[:2]
    assert np.array_equal(flag, f[:, :, 1]) and np.array_equal(thr, t[:, :, 1])
