"""The numpy restatement of the cross GOCA-CFAR map detector (tests/_xcfar_ref.py) against the
reference's own loop and against the oracle of the frame chain.  No device.

  * float64: flags and thresholds equal a double loop over r and v written out here cell by cell as
    fsf:192-213 has it (mean = the slice summed left to right, divided by its length);
  * the hits on the pair sums of a 3-beam complex map are oracle.chain.goca_cfar's list, in its order;
  * float32: the thresholds are not the float64 thresholds of the same float32 maps rounded to single,
    so K3's x * RN(1 / n) is part of the definition;
  * the planted ties: exactly two cells per window shape where ``>`` and ``>=`` differ.
"""
import numpy as np
import pytest

import _xcfar_ref as ref
from oracle import chain

WINDOWS = [(5, 10, 5, 10), (2, 1, 2, 1), (3, 2, 1, 0), (1, 0, 4, 3), (8, 4, 2, 1), (40, 24, 20, 12)]


def _loop(A, cfar):
    """fsf:192-213 on one map, cell by cell (1-based r, v as there)."""
    T = cfar['T_CFAR']
    gR, gV, rR, rV = cfar['guardCells_R'], cfar['guardCells_V'], cfar['refCells_R'], cfar['refCells_V']
    nV, nR = A.shape
    det = np.zeros((nV, nR), np.uint8)
    thr = np.full((nV, nR), np.inf)

    def mean(x):
        s = 0.0
        for e in x:
            s = s + float(e)
        return s / len(x)

    for r in range(rR + gR + 1, nR - rR - gR + 1):
        for v in range(rV + gV + 1, nV - rV - gV + 1):
            cut = A[v - 1, r - 1]
            lead_r = A[v - 1, r - gR - rR - 1:r - gR - 1]
            trail_r = A[v - 1, r + gR:r + gR + rR]
            noise_r = max(mean(lead_r), mean(trail_r))
            lead_v = A[v - gV - rV - 1:v - gV - 1, r - 1]
            trail_v = A[v + gV:v + gV + rV, r - 1]
            noise_v = max(mean(lead_v), mean(trail_v))
            t = T * max(noise_r, noise_v)
            thr[v - 1, r - 1] = t
            if cut > t:
                det[v - 1, r - 1] = 1
    return det, thr


@pytest.mark.parametrize('win', [(2, 1, 2, 1, 1.2), (3, 2, 1, 0, 1.3), (1, 0, 4, 3, 1.3), (3, 1, 7, 0, 1.5)],
                         ids=lambda w: '%d-%d-%d-%d-T%g' % w)
def test_float64_equals_the_reference_loop(win):
    cfar = ref.cfar_dict(win)
    a = ref.make_maps(21, 40, 3, cfar=dict(cfar, T_CFAR=1.5))
    f, t = ref.goca_cfar_maps(a, cfar)
    assert f.shape == t.shape == a.shape and f.dtype == np.uint8 and t.dtype == np.float64
    for b in range(3):
        fl, tl = _loop(a[:, :, b], cfar)
        assert np.array_equal(f[:, :, b], fl) and np.array_equal(t[:, :, b], tl)
    assert 0 < int(f.sum()) < np.isfinite(t).sum()
    r0, r1, v0, v1 = ref.cells_under_test(21, 40, cfar)
    assert np.isfinite(t[v0:v1, r0:r1]).all() and np.isinf(t).sum() == t.size - 3 * (v1 - v0) * (r1 - r0)


def test_no_cell_under_test():
    for P, G in ((6, 64), (40, 6), (1, 1)):
        a = ref.make_maps(P, G, 2)
        f, t = ref.goca_cfar_maps(a, ref.cfar_dict((2, 1, 2, 1, 1.0)))
        assert not f.any() and np.isposinf(t).all()


@pytest.mark.parametrize('win', [(3, 1, 7, 0, 1.5), (5, 10, 5, 10, 1.1), (1, 0, 1, 0, 1.2)], ids=lambda w: '%d-%d-%d-%d-T%g' % w)
def test_hits_on_pair_sums_are_the_oracle_list(win):
    cfar = ref.cfar_dict(win)
    rng = np.random.default_rng(ref.SEED)
    rdm = rng.standard_normal((40, 70, 3)) + 1j * rng.standard_normal((40, 70, 3))
    dets, S_all = chain.goca_cfar(rdm, cfar)
    f, t = ref.goca_cfar_maps(S_all, cfar)
    hits = ref.find_hits(S_all, f, t)
    assert len(dets) > 20
    assert np.array_equal(hits[:, :4], dets)


def test_float32_form_is_part_of_the_definition():
    cfar = ref.cfar_dict((3, 2, 1, 0, 1.3))
    a32 = ref.make_maps(33, 193, 3).astype(np.float32)
    _, t32 = ref.goca_cfar_maps(a32, cfar, np.float32)
    _, t64 = ref.goca_cfar_maps(a32.astype(np.float64), dict(cfar, T_CFAR=float(np.float32(1.3))), np.float64)
    assert np.array_equal(t32, t32.astype(np.float32).astype(np.float64))
    cut = np.isfinite(t32)
    differ = int((t32[cut] != t64[cut].astype(np.float32)).sum())
    print('%d of %d float32 thresholds differ from the float64 ones rounded to single' % (differ, int(cut.sum())))
    assert differ > 0


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('win', WINDOWS, ids=lambda w: '%d-%d-%d-%d' % w)
def test_planted_ties(win, dtype):
    cfar = ref.cfar_dict(win + (1.5,))
    hR, hV = win[0] + win[1], win[2] + win[3]
    P, G = 2 * hV + 6, 2 * hR + 12
    a = ref.make_maps(P, G, 3, cfar=cfar)
    strict, t = ref.goca_cfar_maps(a, cfar, dtype)
    loose, _ = ref.goca_cfar_maps(a, cfar, dtype, strict=False)
    ties = np.argwhere(strict != loose)
    assert [tuple(x) for x in ties] == [(hV, hR, 1), (P - hV - 1, G - hR - 1, 1)]
    assert t[hV, hR, 1] == 3.0 and a[hV, hR, 1] == 3.0


# ------------------------------------------------------------------ the value cases (tests/_cfar_value_cases.py)
import _cfar_value_cases as vc   # noqa: E402

_VC = [(v, p, c) for v in vc.VARIANTS['xcfar'] for p in ('c128', 'c64') for c in vc.cases(p)]


@pytest.mark.parametrize('variant, prec, case', _VC, ids=['%d-%d-%d-%d-%s-%s' % (v + (p, c)) for v, p, c in _VC])
def test_value_case_preconditions(variant, prec, case):
    """No value case is hollow: the restatement has the property the case is named for (the left-out
    complex-double cases included: the restatement itself is defined there)."""
    vc.check_preconditions('xcfar', variant, case, prec)


def test_left_out_list_is_the_two_out_of_domain_cases():
    assert vc.LEFT_OUT == {('xcfar', 'c128', 'sub'), ('xcfar', 'c128', 'tiny')}
    for det in vc.DETECTORS:
        for prec in ('c128', 'c64'):
            want = [c for c in vc.cases(prec) if not (det == 'xcfar' and prec == 'c128' and c in ('sub', 'tiny'))]
            assert list(vc.compared(det, prec)) == want
    assert 'x900' in vc.compared('xcfar', 'c128') and 'narrowed' in vc.compared('xcfar', 'c64')


def test_fma_quotient_domain():
    """k3_quot's complex-double form in exact rational arithmetic against RN(x / n), n = 1 .. 64.
    Where the quotient is a normal number (x >= n 2^-1022) the two agree, at every scale up to the
    largest finite x; the residual is exact everywhere, subnormal or not.  Below, they differ on exact
    ties between two subnormals, which need an even n that is no power of two; odd n and powers of two
    agree at every scale.  The sums x are sums of a few random amplitudes, as a window forms them."""
    rng = np.random.default_rng(ref.SEED)
    fm = float(np.finfo(np.float64).max)
    above = below = 0
    bad_above, bad_below = [], {}
    for n in range(1, 65):
        lo = n * 2.0 ** -1022                   # the smallest x whose quotient is normal
        xs = [lo, float(np.nextafter(lo, 1.0)), lo * 1.5, fm, fm / 3, 1.0, 0.1 * n]
        for e in (-1016, -1000, -900, -300, -60, 0, 60, 300, 1000):
            xs += [float(x) for x in np.ldexp(rng.rayleigh(1.0, (25, 5)).sum(axis=1), e)]
        for x in xs:
            assert x >= lo
            q, exact = vc.fma_quotient(x, n)
            above += 1
            if q != vc.true_quotient(x, n) or not exact:
                bad_above.append((x, n))
        sub = [float(np.nextafter(lo, 0.0)), 2.0 ** -1074, 3 * 2.0 ** -1074]
        for e in (-1030, -1045, -1060, -1072):
            sub += [float(x) for x in np.ldexp(rng.rayleigh(1.0, (25, 5)).sum(axis=1), e)]
        for x in sub:
            if not 0 < x < lo:
                continue
            q, exact = vc.fma_quotient(x, n)
            assert exact, 'the residual of x = %r, n = %d is not exact' % (x, n)
            below += 1
            if q != vc.true_quotient(x, n):
                bad_below[n] = bad_below.get(n, 0) + 1
    print('quotient normal: %d mismatches of %d; quotient subnormal: %d of %d, by n: %r'
          % (len(bad_above), above, sum(bad_below.values()), below, sorted(bad_below.items())))
    assert not bad_above, bad_above[:5]
    assert sum(bad_below.values()) >= 20
    assert all(n % 2 == 0 and n & (n - 1) for n in bad_below), 'a mismatch at an odd n or a power of two'
    assert {6, 10} <= set(bad_below)


def test_fma_quotient_of_infinity_is_the_select():
    """fma(-Inf, n, +Inf) is NaN: the FMA form alone gives NaN for a sum that overflowed, the division
    +Inf.  k3_quot returns q0 = +Inf when the refined quotient is NaN; the restatement divides."""
    inf = np.float64(np.inf)
    with np.errstate(invalid='ignore'):
        q0 = inf * np.float64(1.0 / 5)
        r = -q0 * 5.0 + inf
    assert np.isposinf(q0) and np.isnan(r)
    assert np.isposinf(ref.quotient(np.array([inf]), 5, np.float64)).all()
