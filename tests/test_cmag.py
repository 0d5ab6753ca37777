"""cmag (csrc/rsp_cmag.h), the one magnitude routine of the device code, per element against hypot in
long double (tests/_cmag_cases.py: reference, derived bound 3u / 4u, cases).  Every other test of the
suite checks magnitudes against a tolerance times max(map), which hides a relative error in the quiet
cells where it moves CFAR decisions.  Each test prints its worst error in u before asserting.

The call sites and the test that reaches each (file:line of the cmag call):
  rsp_detect.hip:77   k_pairsum, MATLAB layout (tile transpose)    test_direct, test_zero: chosen values
                      through Plan.detect on a cube whose second beam is zero, so that the pair-sum
                      map is cmag(x) + 0 = cmag(x); scales 2^-500 .. 2^500 (double), 2^-60 .. 2^60 (float)
  rsp_detect.hip:110  k_pairsum, device layout                      test_stage2_detect_pair_sums, on the
                      device's own stage-2 values.  No call feeds this layout chosen values; the scales
                      far from 1 are covered for it only by the arithmetic being the same inline function
  rsp_detect.hip:157  k_s9, the monopulse magnitudes                not observable per element: they enter
                      Angle only (test_detect.py compares it with the oracle)
  rsp_stage3.hip:78   k_s3_cfar, complex form                       test_stage2_amp[cfar]
  rsp_vcfar.hip:68    k_vcfar, complex form                         test_stage2_amp[vcfar]
  rsp_xcfar.hip:91    k_xcfar, complex form                         test_stage2_amp[xcfar]
  rsp_k2.hip:56, 92   k2_pc's last inverse pass (StoreRdm, the row-uniform store)
  rsp_k2.hip:189      k2_pc's row epilogue
  rsp_k2.hip:677, 687 k2_pc's narrow FIR (4 gates per lane, the tail)
                      test_frame_pair_sums[plumbing] (narrow FIR plus both overlap-save segments) and
                      [w4-mb128] (k2_pc<double, 4> beside a 2560-point block): cfar_maps against
                      |rdm_b| + |rdm_b+1| of the same call
The device-value tests run on noise plus targets with a 20 dB one: max / median of |rdm| >= 1e3
(test_cmag_cases.py), and the same is asserted here on the device's map.
"""
import numpy as np
import pytest

import _cmag_cases as cc
from _detect_cases import CLUSTER, axes
from oracle import chain
from rsp.plan import Plan

pytestmark = pytest.mark.gpu

MAG, PAIR = cc.MAG_BOUND_U * cc.SLACK, cc.PAIR_BOUND_U * cc.SLACK


@pytest.fixture(scope='module')
def plans():
    """The plumbing plan (16 pulses x 3 beams x 16 channels) per precision, made on first use."""
    made = {}

    def get(prec, name='plumbing'):
        if (prec, name) not in made:
            s = cc.frame_scenario(name)
            made[(prec, name)] = Plan(s['cfg'], s['cfar'], s['clus'], s['pre_p'], precision=prec)
        return made[(prec, name)]
    yield get
    for p in made.values():
        p.close()


def _is_float(a):
    return np.array_equal(a, a.astype(np.float32).astype(np.float64))


# ------------------------------------------------------------------ chosen values
@pytest.mark.parametrize('prec, e, shape', cc.direct_cases(), ids=['%s-e%d-%s' % c for c in cc.direct_cases()])
def test_direct(plans, prec, e, shape):
    cube = cc.direct_cube(prec, e, shape)
    V, G, B = cube.shape
    out = plans(prec).detect(cube, cfar=cc.WINDOW, cluster=CLUSTER, want_cfar=True, **axes(V, G, B))
    got = out['cfar_maps'][:, :, 0]
    rel = cc.mag_error(got, cube[:, :, 0])
    kind = cc.cell_kinds(V, G)
    for k, name in enumerate(cc.KINDS):
        cc.report('%s 2^%d %s %s' % (prec, e, shape, name), np.where(kind == k, rel, 0.0), prec, cc.MAG_BOUND_U)
    worst = cc.report('%s 2^%d %s' % (prec, e, shape), rel, prec, cc.MAG_BOUND_U)
    assert got.shape == (V, G) and (got > 0).all()
    assert worst <= MAG, 'a magnitude %.3f u from hypot (bound %g u)' % (worst, cc.MAG_BOUND_U)
    if prec == 'c64':
        assert _is_float(got)
    assert len(out['detections']) == 0 and len(out['final_targets']) == 0


@pytest.mark.parametrize('shape', list(cc.SHAPES))
@pytest.mark.parametrize('prec', ['c128', 'c64'])
def test_zero(plans, prec, shape):
    """0 stays 0: zeros of either sign come back as +0, and nothing is detected (0 > 0 is false)."""
    cube = cc.zero_cube(prec, shape)
    V, G, B = cube.shape
    out = plans(prec).detect(cube, cfar=cc.WINDOW, cluster=CLUSTER, want_cfar=True, **axes(V, G, B))
    got = out['cfar_maps'][:, :, 0]
    assert (got == 0).all() and not np.signbit(got).any()
    assert len(out['detections']) == 0


# ------------------------------------------------------------------ the device's own complex values
def _stage2_iq(prec):
    s = cc.frame_scenario('plumbing')
    iq = chain.dbf(cc.frame_cube('plumbing', prec).astype(np.complex128), s['W'])
    return iq.astype(cc.CDTYPE[prec])


S2_CFAR = {'cfar': dict(refCells_R=5, saveCells_R=14, T_CFAR=1.5, CFARmethod_R=0, MTD_0v_num=1),
           'vcfar': dict(refCells_V=4, guardCells_V=6, T_CFAR=1.5),
           'xcfar': dict(refCells_R=3, guardCells_R=2, refCells_V=2, guardCells_V=1, T_CFAR=1.3)}


@pytest.mark.parametrize('which', list(S2_CFAR))
@pytest.mark.parametrize('prec', ['c128', 'c64'])
def test_stage2_amp(plans, prec, which):
    """The complex forms of the three map detectors: ``amp`` against hypot(``mtd``) of the same call."""
    p = plans(prec)
    call = {'cfar': p.process_stage2_cfar, 'vcfar': p.process_stage2_vcfar, 'xcfar': p.process_stage2_xcfar}[which]
    res = call(_stage2_iq(prec), S2_CFAR[which], want=('mtd', 'amp'))
    mtd, amp = res['mtd'], res['amp']
    assert amp.shape == mtd.shape == (p.P, p.G, p.B) and amp.dtype == np.float64
    ratio = np.abs(mtd).max() / np.median(np.abs(mtd))
    rel = cc.mag_error(amp, mtd)
    worst = cc.report('%s stage2-%s amp (max / median %.3g)' % (prec, which, ratio), rel, prec, cc.MAG_BOUND_U)
    assert ratio >= cc.DYNAMIC_RANGE
    assert worst <= MAG, 'a magnitude %.3f u from hypot (bound %g u)' % (worst, cc.MAG_BOUND_U)
    if prec == 'c64':
        assert _is_float(amp) and _is_float(mtd.real) and _is_float(mtd.imag)


def _pair_check(label, prec, maps, rdm):
    assert maps.shape == rdm.shape[:2] + (rdm.shape[2] - 1,)
    ratio = np.abs(rdm).max() / np.median(np.abs(rdm))
    rel = cc.pair_error(maps, rdm[:, :, :-1], rdm[:, :, 1:])
    worst = cc.report('%s %s pair sums (max / median %.3g)' % (prec, label, ratio), rel, prec, cc.PAIR_BOUND_U)
    assert ratio >= cc.DYNAMIC_RANGE
    assert worst <= PAIR, 'a pair sum %.3f u from |a| + |b| (bound %g u)' % (worst, cc.PAIR_BOUND_U)
    if prec == 'c64':
        assert _is_float(maps)


@pytest.mark.parametrize('prec', ['c128', 'c64'])
@pytest.mark.parametrize('name', cc.FRAME_CASES)
def test_frame_pair_sums(plans, name, prec):
    """k2_pc's magnitude stores: ``cfar_maps`` against |rdm_b| + |rdm_b+1| of the same frame."""
    p = plans(prec, name)
    if name == 'w4-mb128' and prec == 'c128':
        L = p.k2_layout()
        assert L['wg_per_cu'] == 4 and L['k2_pts'] == 2560
    out = p.process_cube(cc.frame_cube(name, prec), frame_idx=1, want_rdm=True, want_cfar=True)
    _pair_check(name, prec, out['cfar_maps'], out['rdm'])
    assert len(out['detections']) > 0


@pytest.mark.parametrize('prec', ['c128', 'c64'])
def test_stage2_detect_pair_sums(plans, prec):
    """k_pairsum's device layout: ``cfar_maps`` against |rdm_b| + |rdm_b+1| of the same call."""
    out = plans(prec).process_stage2_detect(_stage2_iq(prec), want_rdm=True, want_cfar=True)
    _pair_check('stage2-detect', prec, out['cfar_maps'], out['rdm'])
