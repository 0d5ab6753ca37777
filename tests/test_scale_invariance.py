"""Power-of-two scale invariance: every stage up to the magnitude is linear and every CFAR is
homogeneous, so an input multiplied by 2^k must give outputs multiplied by 2^k and identical decisions,
bit for bit.  A stray epsilon, an absolute clamp or a flushed intermediate anywhere in K1, K2, the MTD,
the DBF, the DDC or a detector breaks that, and a map of amplitudes near 1 cannot show it.

k = +-300 for complex-double plans, +-24 for complex-single plans: the scaling of the input is exact
(np.ldexp), every intermediate stays a normal number, and k is even, so q = x^2 + y^2 moves by an even
exponent and the square root by a whole one.

  linear calls (output == output_0 2^k, every bit): Plan.dbf, Plan.ddc (both mixers), Plan.pulse_compress,
    Plan.mtd (a power of two and a chirp-z length), process_stage2 (mtd and pc), process_cube's rdm;
  detector calls (process_stage2_cfar / _vcfar / _xcfar, Plan.detect, process_cube with cfar_maps and
    thresholds): flags, hit indices, detection keys and their order identical; amp, thresholds and
    cfar_maps scaled exactly; Range and Velocity identical bits (the spline's first argmax is homogeneous);
  Angle holds the reference's absolute eps by definition (S + eps): compared to the bit only for k > 0 and
    only on detections whose pair sum S at k = 0 is at least 2 and has S + eps == S in double, which is how
    S9 forms the denominator (rsp_s9.h).  That follows from S >= 4 (half an ulp is 2^-51 > eps); in [2, 4)
    eps = 2^-52 is exactly half an ulp, the add is a tie, and it leaves S alone only where S's last bit is
    even: always for a complex-single plan's sums (floats widened; S = 2 exactly is left out, the
    unrounded sum may lie just below), for every other double in a complex-double plan.  Both conditions
    are evaluated on cfar_maps.  For k < 0 Angle is not compared.  Final targets under the same rule: for k > 0
    only (stage-1 clustering reads Angle, so at k < 0 the clusters themselves may differ, and at 2^-300 they
    do), their Angle only where all of the frame's detections qualify;
  Power scales by one exact power of two, the same for all targets.

Noise comes from chain.philox_noise on the host; the device synthesis is not homogeneous and not part of
this.  Shapes: the plumbing plan 16 x 1024 x 16 channels x 3 beams and the small stand-alone shapes of the
stages' own modules.
"""
import numpy as np
import pytest

import _cmag_cases as cc
import _ddc_cases as dd
import _detect_cases as dc
import _mtd_cases as mc
from oracle import chain
from rsp.plan import Plan

pytestmark = pytest.mark.gpu

K = {'c128': (300, -300), 'c64': (24, -24)}
CASES = [(p, k) for p in ('c128', 'c64') for k in K[p]]
IDS = ['%s-k%+d' % c for c in CASES]
RDT = {'c128': np.float64, 'c64': np.float32}
EPS_FREE_SUM = 2.0
EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(scope='module')
def plans():
    made = {}

    def get(prec):
        if prec not in made:
            s = cc.frame_scenario('plumbing')
            made[prec] = Plan(s['cfg'], s['cfar'], s['clus'], s['pre_p'], precision=prec)
        return made[prec]
    yield get
    for p in made.values():
        p.close()


def scaled(a, k):
    """a 2^k, exactly, in a's own dtype."""
    a = np.asarray(a)
    if np.iscomplexobj(a):
        out = np.empty_like(a)
        out.real, out.imag = np.ldexp(a.real, k), np.ldexp(a.imag, k)
        return out
    return np.ldexp(a, k)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype.itemsize % 8 == 0 else np.uint32)


def assert_scaled(got, base, k, what):
    want = scaled(base, k)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    assert np.isfinite(want).all(), what
    bad = bits(got) != bits(want)
    assert not bad.any(), '%s: %d of %d words differ from output_0 2^%d' % (what, int(bad.sum()), bad.size, k)


def assert_same(got, base, what):
    assert np.array_equal(bits(np.asarray(got)), bits(np.asarray(base))), what


def _noise(shape, prec, seed, cplx=True):
    rng = np.random.default_rng(cc.SEED + seed)
    x = rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if cplx else 0)
    return np.asfortranarray(x.astype(cc.CDTYPE[prec] if cplx else RDT[prec]))


def _cube(prec):
    return cc.frame_cube('plumbing', prec)


def _iq(prec):
    s = cc.frame_scenario('plumbing')
    return chain.dbf(_cube(prec).astype(np.complex128), s['W']).astype(cc.CDTYPE[prec])


# ------------------------------------------------------------------ linear calls
@pytest.mark.parametrize('prec, k', CASES, ids=IDS)
def test_dbf(plans, prec, k):
    W = cc.frame_scenario('plumbing')['W']
    x = _cube(prec)
    assert_scaled(plans(prec).dbf(scaled(x, k), W), plans(prec).dbf(x, W), k, 'dbf')
    y = _noise((5, 33, 7), prec, 1)                       # a stand-alone shape: odd sizes, 7 channels
    Wy = _noise((3, 7), 'c128', 2)
    assert_scaled(plans(prec).dbf(scaled(y, k), Wy, conj=False), plans(prec).dbf(y, Wy, conj=False), k, 'dbf 5x33x7')


@pytest.mark.parametrize('nco', ['iq', 'sin'])
@pytest.mark.parametrize('prec, k', CASES, ids=IDS)
def test_ddc(plans, prec, k, nco):
    x = _noise((5, 301, 2), prec, 3, cplx=False)
    h = dd.fir_mat()
    kw = dict(w=dd.TENTH, w0=12345, nco=nco, off=1)
    assert_scaled(plans(prec).ddc(scaled(x, k), h, 4, **kw), plans(prec).ddc(x, h, 4, **kw), k, 'ddc ' + nco)


@pytest.mark.parametrize('prec, k', CASES, ids=IDS)
def test_pulse_compress(plans, prec, k):
    iq = _iq(prec)
    assert_scaled(plans(prec).pulse_compress(scaled(iq, k)), plans(prec).pulse_compress(iq), k, 'pulse_compress')
    one = iq[:5, :, :2]                                    # another pulse and beam count
    assert_scaled(plans(prec).pulse_compress(scaled(one, k)), plans(prec).pulse_compress(one), k, 'pulse_compress 5x2')


@pytest.mark.parametrize('P, nfft', [(16, 16), (12, 20)], ids=['pow2-16', 'chirpz-12-20'])
@pytest.mark.parametrize('prec, k', CASES, ids=IDS)
def test_mtd(plans, prec, k, P, nfft):
    x = _noise((P, 37, 2), prec, 4)
    win = mc.kaiser32(P)
    assert_scaled(plans(prec).mtd(scaled(x, k), win, nfft=nfft), plans(prec).mtd(x, win, nfft=nfft), k, 'mtd %d -> %d' % (P, nfft))


@pytest.mark.parametrize('prec, k', CASES, ids=IDS)
def test_process_stage2(plans, prec, k):
    iq = _iq(prec)
    m0, p0 = plans(prec).process_stage2(iq)
    m1, p1 = plans(prec).process_stage2(scaled(iq, k))
    assert_scaled(p1, p0, k, 'stage-2 pc')
    assert_scaled(m1, m0, k, 'stage-2 mtd')


# ------------------------------------------------------------------ detector calls
def _assert_hits(h1, h0, k, what):
    assert len(h1) == len(h0) > 0, what
    for f in ('v_idx', 'r_idx', 'beam_idx'):
        assert np.array_equal(h1[f], h0[f]), '%s: hit %s' % (what, f)
    assert_scaled(h1['amp'], h0['amp'], k, what + ' hit amp')
    assert_scaled(h1['threshold'], h0['threshold'], k, what + ' hit threshold')


S2_CFAR = {'cfar': dict(refCells_R=5, saveCells_R=14, T_CFAR=1.5, CFARmethod_R=0, MTD_0v_num=1),
           'vcfar': dict(refCells_V=4, guardCells_V=6, T_CFAR=1.5),
           'xcfar': dict(refCells_R=3, guardCells_R=2, refCells_V=2, guardCells_V=1, T_CFAR=1.3)}


@pytest.mark.parametrize('which', list(S2_CFAR))
@pytest.mark.parametrize('prec, k', CASES, ids=IDS)
def test_stage2_detectors(plans, prec, k, which):
    p = plans(prec)
    call = {'cfar': p.process_stage2_cfar, 'vcfar': p.process_stage2_vcfar, 'xcfar': p.process_stage2_xcfar}[which]
    iq = _iq(prec)
    r0, r1 = call(iq, S2_CFAR[which]), call(scaled(iq, k), S2_CFAR[which])
    assert_scaled(r1['mtd'], r0['mtd'], k, which + ' mtd')
    assert_scaled(r1['amp'], r0['amp'], k, which + ' amp')
    assert np.array_equal(r1['flags'], r0['flags']), '%d flags differ' % int((r1['flags'] != r0['flags']).sum())
    finite = np.isfinite(r0['threshold'])
    assert np.array_equal(np.isfinite(r1['threshold']), finite)
    assert_scaled(np.where(finite, r1['threshold'], 0.0), np.where(finite, r0['threshold'], 0.0), k, which + ' threshold')
    assert r1['n_hits'] == r0['n_hits'] > 100
    _assert_hits(r1['hits'], r0['hits'], k, which)


def _angle_comparable(d0, maps0, prec):
    """Detections whose pair sum at k = 0 is at least 2 and absorbs eps (the module docstring)."""
    S = np.array([maps0[d['v_idx'] - 1, d['r_idx'] - 1, d['pair_idx'] - 1] for d in d0])
    amp = np.array([d['amp'] for d in d0])
    assert np.array_equal(S, amp), 'a detection whose amp is not its cell of cfar_maps'
    return (S >= EPS_FREE_SUM) & (S + EPS == S) & ((prec == 'c128') | (S != EPS_FREE_SUM))


def _assert_detections(o1, o0, k, what, prec):
    d0, d1 = o0['detections'], o1['detections']
    key = lambda d: (d['v_idx'], d['r_idx'], d['pair_idx'])   # noqa: E731
    assert len(d0) > 0 and [key(d) for d in d1] == [key(d) for d in d0], what + ': detection keys or their order'
    assert_scaled(o1['cfar_maps'], o0['cfar_maps'], k, what + ' cfar_maps')
    assert_scaled(np.array([d['amp'] for d in d1]), np.array([d['amp'] for d in d0]), k, what + ' amp')
    for f in ('Range', 'Velocity'):
        assert_same([d[f] for d in d1], [d[f] for d in d0], '%s: %s of the detections' % (what, f))
    ok = _angle_comparable(d0, o0['cfar_maps'], prec)
    print('%s: %d detections, %d of them compared in Angle, %d final targets' % (what, len(d0), int(ok.sum()), len(o0['final_targets'])))
    if k > 0:
        assert 2 * int(ok.sum()) >= len(d0), 'fewer than half of the detections have a pair sum that absorbs eps'
        assert_same([d['Angle'] for d, c in zip(d1, ok) if c], [d['Angle'] for d, c in zip(d0, ok) if c], what + ': Angle')
    if k < 0:       # Angle differs by definition, and stage-1 clustering reads it: the targets are not compared
        return None
    t0, t1 = o0['final_targets'], o1['final_targets']
    assert len(t1) == len(t0) > 0, what + ': final target count'
    for f in ('Range', 'Velocity'):
        assert_same([t[f] for t in t1], [t[f] for t in t0], '%s: %s of the final targets' % (what, f))
    if ok.all():
        assert_same([t['Angle'] for t in t1], [t['Angle'] for t in t0], what + ': Angle of the final targets')
    ratio = t1[0]['Power'] / t0[0]['Power']
    m, e = np.frexp(ratio)
    assert m == 0.5 and e - 1 != 0, '%s: Power ratio %r is no power of two' % (what, ratio)
    assert_same([t['Power'] for t in t1], [np.ldexp(t['Power'], int(e) - 1) for t in t0], what + ': Power')
    return int(e) - 1


@pytest.mark.parametrize('prec, k', CASES, ids=IDS)
def test_detect(plans, prec, k):
    name = 'tile+1'
    c = dc.CASES[name]
    x = dc.cube(name, prec)
    kw = dict(cfar=dc.cfar_dict(c), cluster=dc.CLUSTER, want_cfar=True, **dc.axes(c['V'], c['G'], c['B']))
    o0, o1 = plans(prec).detect(x, **kw), plans(prec).detect(scaled(x, k), **kw)
    pk = _assert_detections(o1, o0, k, 'detect %s' % name, prec)
    print('Power moved by 2^%r' % pk)


@pytest.mark.parametrize('prec, k', CASES, ids=IDS)
def test_process_cube(plans, prec, k):
    x = _cube(prec)
    kw = dict(frame_idx=1, want_rdm=True, want_cfar=True, want_threshold=True)
    o0, o1 = plans(prec).process_cube(x, **kw), plans(prec).process_cube(scaled(x, k), **kw)
    assert_scaled(o1['rdm'], o0['rdm'], k, 'rdm')
    assert np.array_equal(o1['cfar_flags'], o0['cfar_flags'])
    finite = np.isfinite(o0['cfar_threshold'])
    assert finite.any() and np.array_equal(np.isfinite(o1['cfar_threshold']), finite)
    assert_scaled(np.where(finite, o1['cfar_threshold'], 0.0), np.where(finite, o0['cfar_threshold'], 0.0), k, 'cfar_threshold')
    pk = _assert_detections(o1, o0, k, 'process_cube', prec)
    print('Power moved by 2^%r' % pk)
