"""The three bit-defined map detectors on the device over the whole value range: k_s3_cfar
(Plan.stage3_cfar), k_vcfar (Plan.doppler_cfar: CA, GOCA, SOCA) and k_xcfar (Plan.cross_cfar) against
their numpy restatements run in the plan's dtype, on the value cases of tests/_cfar_value_cases.py:
subnormal maps, maps whose window sums overflow, double maps a complex-single plan narrows to 0,
subnormals and +Inf, 30 decades of dynamic range, constant maps that tie everywhere, zeros, and T_CFAR
far from 1.  Every other detector test of the suite feeds Rayleigh(1.0).

Flags: ``array_equal``.  Thresholds: ``array_equal`` (NaN never equal: a NaN threshold fails).  Hit
lists: equal in find() order, ``amp`` and ``threshold`` fields included.  The CPU halves
(test_stage3_ref.py, test_vcfar_ref.py, test_xcfar_ref.py ::test_value_case_preconditions) assert that
each case has the property it is named for.

Shapes, one per detector, the smallest that cross a tile along both axes: stage 3 P = 33 with segments
(38, 60, 350) (two range chunks) and window 5 / 14, greatest-of and smallest-of; Doppler CFAR 40 x 70
with window 4 / 6; cross CFAR 40 x 70 with windows 3 / 1 / 7 / 0 (two divisors) and 5 / 5 / 5 / 5.
(K3's one-quotient path for equal divisors is not k_xcfar's: test_xcfar.py::test_frame_chain_threshold_maps
ties K3 to k_xcfar's bits.)

Not compared, and asserted to be exactly that list: the complex-double cross CFAR on ``sub`` and
``tiny`` (_cfar_value_cases.LEFT_OUT and the reason there).  Their mismatch counts are printed.
"""
import numpy as np
import pytest

import _cfar_value_cases as vc
import _stage3_ref
from rsp import config as C
from rsp.plan import Plan
from rsp.precompute import precompute as product_precompute
from _scen import plumbing_config, plumbing_weights

pytestmark = pytest.mark.gpu

DTYPE = vc.DTYPE
LEFT_OUT = {('xcfar', 'c128', 'sub'), ('xcfar', 'c128', 'tiny')}      # the issue's list, restated here


@pytest.fixture(scope='module')
def plans():
    """One plan per precision, made when a test first asks for it."""
    made = {}

    def get(prec):
        if prec not in made:
            cfg = plumbing_config(16, 3, 16)
            W, ang, k = plumbing_weights(cfg)
            made[prec] = Plan(cfg, C.default_cfar_params(), C.default_cluster_params(),
                              product_precompute(cfg, W, ang, k, C.V8_FIR), precision=prec)
        return made[prec]
    yield get
    for p in made.values():
        p.close()


def _rows(h):
    return np.column_stack([h['v_idx'], h['r_idx'], h['beam_idx'], h['amp'], h['threshold']]) if len(h) else np.zeros((0, 5))


def _call(plan, det, variant, amp, T):
    prm = vc.params(det, variant, T)
    if det == 'stage3':
        return plan.stage3_cfar(amp, prm, segments=vc.S3_SEGS)
    if det == 'vcfar':
        return plan.doppler_cfar(amp, prm, method=variant)
    return plan.cross_cfar(amp, prm)


def _diff(res, want_f, want_t):
    return int((res['flags'] != want_f).sum()), int((~((res['threshold'] == want_t))).sum())


def _check(res, amp, want_f, want_t, dtype):
    assert res['flags'].dtype == np.uint8 and res['threshold'].dtype == np.float64
    assert res['flags'].shape == res['threshold'].shape == amp.shape
    nf, nt = _diff(res, want_f, want_t)
    assert not np.isnan(res['threshold']).any(), '%d NaN thresholds' % int(np.isnan(res['threshold']).sum())
    assert np.array_equal(res['flags'], want_f), '%d flags differ' % nf
    assert np.array_equal(res['threshold'], want_t, equal_nan=False), '%d thresholds differ' % nt
    with np.errstate(over='ignore', under='ignore'):
        want_h = _stage3_ref.find_hits(amp, want_f, want_t, dtype)
    assert res['n_hits'] == len(want_h) == int(want_f.sum())
    assert np.array_equal(_rows(res['hits']), want_h), 'hit list differs from find() order'


def _params():
    return [(d, v, p, c) for d in vc.DETECTORS for v in vc.VARIANTS[d] for p in ('c128', 'c64') for c in vc.cases(p)]


def _id(p):
    d, v, prec, c = p
    return '%s-%s-%s-%s' % (d, v if isinstance(v, str) else '%d-%d-%d-%d' % v, prec, c)


@pytest.mark.parametrize('det, variant, prec, case', _params(), ids=[_id(p) for p in _params()])
def test_value_case(plans, det, variant, prec, case):
    plan = plans(prec)
    amp = vc.value_map(case, prec, *vc.shape_of(det))
    for T in vc.thresholds_T(case, det, prec):
        want_f, want_t = vc.expected(det, variant, prec, case, T)
        res = _call(plan, det, variant, amp, T)
        nf, nt = _diff(res, want_f, want_t)
        print('%s %s %s %s T=%r: %d hits, %d flags and %d thresholds of %d differ, %d NaN thresholds'
              % (det, variant, prec, case, T, res['n_hits'], nf, nt, want_f.size, int(np.isnan(res['threshold']).sum())))
        if case not in vc.compared(det, prec):
            assert (det, prec, case) in LEFT_OUT
            continue                       # outside the stated domain: printed, not compared
        assert (det, prec, case) not in LEFT_OUT
        _check(res, amp, want_f, want_t, DTYPE[prec])
        if case == 'zero':
            assert res['n_hits'] == (int(vc.tested_cells(det, variant).sum()) if det == 'stage3' else 0)
        if case == 'huge':
            assert np.isposinf(res['threshold'][vc.tested_cells(det, variant)]).any()


def test_only_the_listed_triples_are_left_out():
    """Every (detector, precision, case) test_value_case is parametrised over is compared except the
    complex-double cross CFAR on ``sub`` and ``tiny`` (test_value_case asserts the same per case)."""
    ran = {(d, p, c) for d, v, p, c in _params() if c in vc.compared(d, p)}
    every = {(d, p, c) for d in vc.DETECTORS for p in ('c128', 'c64') for c in vc.cases(p)}
    assert {(d, p, c) for d, v, p, c in _params()} == every
    assert every - ran == LEFT_OUT == set(vc.LEFT_OUT)
