"""CPU preconditions of the per-element magnitude tests (tests/_cmag_cases.py; the device half is
test_cmag.py): the reference measures what it should, the direct cubes have the cells and the range
they claim, and the cubes for the device-value sites have the dynamic range at which a tolerance
relative to max(map) is blind.
"""
import numpy as np
import pytest

import _cmag_cases as cc
import _xcfar_ref
from rsp.plan import describe_detect, describe_k2


def test_reference_is_wider_than_double_or_exact():
    """hypot in long double resolves errors far below u; the rational fallback agrees with it."""
    rng = np.random.default_rng(cc.SEED)
    z = (rng.standard_normal((4, 5)) + 1j * rng.standard_normal((4, 5))) * 2.0 ** 300
    got = np.abs(z)
    exact = cc._isqrt_hypot_err(got, z.real, z.imag)
    assert (exact <= 2.0 * cc.U['c128']).all() and (exact > 0).any()           # libm's hypot: within one ulp
    if cc.WIDE:
        assert np.allclose(cc.mag_error(got, z), exact, rtol=0, atol=2.0 ** -63)
    # a planted error of 3 ulp is seen as such; zero against zero is 0, zero against a value inf
    bad = np.nextafter(np.nextafter(np.nextafter(got, np.inf), np.inf), np.inf)
    e = cc.mag_error(bad, z) / cc.U['c128']
    assert (e > 1.0).all() and (e < 8.0).all()          # 3 ulp = 3u .. 6u, on top of hypot's own -2u .. 2u
    assert cc.mag_error(np.zeros(1), np.zeros(1, complex))[0] == 0 and np.isinf(cc.mag_error(np.ones(1), np.zeros(1, complex))[0])
    assert cc.pair_error(np.array([3.0 + 5.0]), np.array([3.0 + 0j]), np.array([3.0 + 4.0j]))[0] == 0


def test_shapes_sit_on_the_pair_sum_tile():
    d = describe_detect(*cc.SHAPES['tile+'], 2, cc.WINDOW)
    assert (d['rows'], d['cols']) == (64, 64) and d['row_tiles'] == 1 and d['col_tiles'] == 3
    assert cc.SHAPES['tile+'][0] % 2 == 1 and cc.SHAPES['tile+'][1] % 64 == 2
    assert cc.SHAPES['tile-1'] == (d['rows'] - 1, d['cols'] - 1)
    for V, G in cc.SHAPES.values():
        assert describe_detect(V, G, 2, cc.WINDOW)['cells_under_test'] > 1000


@pytest.mark.parametrize('prec, e, shape', cc.direct_cases(), ids=['%s-e%d-%s' % c for c in cc.direct_cases()])
def test_direct_cube(prec, e, shape):
    cube = cc.direct_cube(prec, e, shape)
    assert cube.dtype == cc.CDTYPE[prec] and not cube[:, :, 1].any()
    x = cube[:, :, 0].astype(np.complex128)
    s = 2.0 ** e
    m = np.abs(x)
    assert 0.5 * s <= m.min() and m.max() <= 2 * s                             # within a factor 4
    kind = cc.cell_kinds(*cc.SHAPES[shape])
    ax = kind == 1
    assert ((x.real[ax] == 0) ^ (x.imag[ax] == 0)).all()
    assert all((sel(x[ax]) != 0).sum() > 50 for sel in (lambda z: np.where(z.real > 0, 1, 0), lambda z: np.where(z.real < 0, 1, 0),
                                                         lambda z: np.where(z.imag > 0, 1, 0), lambda z: np.where(z.imag < 0, 1, 0)))
    sk = kind == 2
    lo, hi = np.minimum(np.abs(x.real[sk]), np.abs(x.imag[sk])), np.maximum(np.abs(x.real[sk]), np.abs(x.imag[sk]))
    ratio = hi / lo
    assert (ratio > 2.0 ** (cc.SKEW[prec] - 0.01)).all() and (ratio < 2.0 ** (cc.SKEW[prec] + 0.01)).all()
    rd = np.float64 if prec == 'c128' else np.float32
    xr, xi = x.real.astype(rd), x.imag.astype(rd)
    q = xr * xr + xi * xi                                                       # in the plan's precision
    assert (hi.astype(rd) ** 2 + lo.astype(rd) ** 2 == hi.astype(rd) ** 2).all()    # the small square is lost
    assert np.isfinite(q).all() and (q >= np.finfo(rd).tiny).all()            # q normal and finite: the stated domain
    # no cell can pass the cross CFAR: T times the mean of any window exceeds every cell
    f, t = _xcfar_ref.goca_cfar_maps(m, cc.WINDOW, rd)
    assert not f.any() and np.isfinite(t).sum() > 1000


def test_zero_cube_has_every_sign():
    for prec in ('c128', 'c64'):
        z = cc.zero_cube(prec, 'tile+')
        assert not z.any()
        sr, si = np.signbit(z.real[:, :, 0]), np.signbit(z.imag[:, :, 0])
        assert all((sr == a).any() and ((sr == a) & (si == b)).any() for a in (0, 1) for b in (0, 1))


@pytest.mark.parametrize('prec', ['c128', 'c64'])
@pytest.mark.parametrize('name', cc.FRAME_CASES)
def test_frame_cubes_have_a_large_dynamic_range(name, prec):
    rdm = np.abs(cc.oracle_rdm(name, cc.frame_cube(name, prec)))
    ratio = rdm.max() / np.median(rdm)
    print('%s %s: max / median of |rdm| = %.3g' % (name, prec, ratio))
    assert ratio >= cc.DYNAMIC_RANGE
    # ... where the old tolerance MAP_TOL x max(map) admits a 100 % error in the median cell of a complex-single map
    assert 2e-5 * rdm.max() / np.median(rdm) >= 0.02


def test_w4_mb128_is_the_four_per_cu_kernel_with_a_2560_point_block():
    s = cc.frame_scenario('w4-mb128')
    L = describe_k2(s['cfg'], s['cfar'], s['clus'], s['pre_p'], precision='c128')
    assert L['wg_per_cu'] == 4 and L['k2_pts'] == 2560
    assert [sg['type'] for sg in L['segments']] == [0, 1, 1] and L['segments'][1]['nblocks'] == 3
    P = describe_k2(cc.frame_scenario('plumbing')['cfg'], cc.frame_scenario('plumbing')['cfar'], cc.frame_scenario('plumbing')['clus'],
                    cc.frame_scenario('plumbing')['pre_p'], precision='c128')
    assert [sg['type'] for sg in P['segments']] == [0, 1, 1]                   # narrow FIR plus both overlap-save segments


def test_docstring_lists_every_cmag_call_site():
    """The file:line list in test_cmag.py's docstring is the set of cmag calls in the device sources:
    a moved or added call fails here until the list (and the test that reaches it) is updated."""
    import glob
    import os
    import re
    import test_cmag
    from rsp import _abi
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(_abi.__file__))), 'csrc')
    found = set()
    for path in glob.glob(os.path.join(csrc, '*.hip')):
        for n, line in enumerate(open(path), 1):
            code = line.split('//')[0]
            if re.search(r'\bcmag\(', code):
                found.add((os.path.basename(path), n))
    listed = set()
    for name, nums in re.findall(r'(rsp_\w+\.hip):(\d+(?:, \d+)*)', test_cmag.__doc__):
        listed |= {(name, int(n)) for n in nums.split(', ')}
    assert listed == found, 'listed only %r, in the sources only %r' % (sorted(listed - found), sorted(found - listed))
    assert len(found) == 11
