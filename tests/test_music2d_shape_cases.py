"""CPU preconditions of the planar MUSIC shape cases (_music2d_shapes.CASES) that the GPU parity
module test_music2d_shapes.py leans on: the numpy restatement tests/_music2d_ref.py alone, on
snapshots from its synthesize_2d, no device.  The device's own snapshots differ from these by
about 1e-12 relative, so the margins carry over.

  * every case is inside the plan's envelope and the tables reach what their comments say;
  * on every instance's unique-grid reference map every pixel is above -60 dB (the spectrum
    comparison covers the whole map), no pixel equals its largest in-bounds neighbour and every pixel
    differs from it by >= 5e-7 dB (_music_shapes.EXACT_MARGIN_DB, 5 x the spectrum tolerance), and the
    min(M, n_peaks) + 1 highest regional maxima differ pairwise by at least as much: a device map
    within the tolerance has the reference's regional maxima, count and top-M order;
  * the restated drop-pass scheme of k_music_peaks2d (_music2d_shapes.drop_passes) gives the flood
    fill's mask on every plateau case, and needs >= 60 passes on `p-runs` and >= 10 on `p-stair`;
  * `few` and `few-m8` have fewer regional maxima than M in every instance.

Each case prints what it measured (pytest -s).  A case that misses a precondition gets another
shape or instance count, not a looser rule.
"""
import numpy as np
import pytest

import _music2d_ref as ref
import _music2d_shapes as m2s
from _music2d_shapes import CASES, CASE_IDS

MU_NMAX, MU_MMAX, M2_SMAX, M2_IB = 64, 8, 65536, 4   # csrc/rsp_music_geometry.h, rsp_music.hip


def test_case_tables_are_inside_the_envelope_and_reach_their_branches():
    for name, c in CASES.items():
        N = c['nx'] * c['ny']
        phi, theta = m2s.plan_grid(c)
        assert 2 <= N <= MU_NMAX and c['K'] >= 1 and 1 <= c['M'] <= min(MU_MMAX, N - 1), name
        assert 3 <= len(phi) <= 1024 and 3 <= len(theta) <= 1024 and len(phi) * len(theta) <= M2_SMAX, name
        assert 1 <= c['n'] <= c['max_batch'], name
    arr = list(m2s.ARRAY_CASES.values())
    shapes = {(c['nx'], c['ny']) for c in arr}
    assert {(2, 1), (1, 7), (64, 1), (2, 32), (32, 2), (7, 9)} <= shapes     # line arrays, N = 2, 64, 63
    assert {c['M'] for c in arr} == {1, 2, 3, 4, 5, 6, 8}
    assert any(c['M'] == c['nx'] * c['ny'] - 1 for c in arr)
    assert any(c['K'] == 1 for c in arr) and any(1 < c['K'] < c['nx'] * c['ny'] for c in arr)
    assert any(c['K'] > 128 for c in arr) and any(c['K'] % 4 == 1 for c in arr)
    assert any(c['dxl'] != c['dyl'] and c['nx'] != c['ny'] for c in arr)
    # batches: every remainder of n mod M2_IB, a batch below the plan's max_batch
    assert {c['n'] % M2_IB for c in m2s.BATCH_CASES.values()} == {1, 2, 3} and CASES[m2s.BATCH_FULL]['n'] == 6
    assert any(c['max_batch'] > c['n'] for c in m2s.BATCH_CASES.values())
    S = {c['nt'] * c['npn'] for c in m2s.GRID_CASES.values()}
    assert {9, 255, 256, 259, M2_SMAX} <= S
    assert {31, 32, 33} <= {c['nt'] for c in m2s.GRID_CASES.values()}
    axes = {a for c in m2s.GRID_CASES.values() for a in (c['nt'], c['npn'])}
    assert {3, 1024} <= axes
    assert any(c['nt'] * c['npn'] == M2_SMAX and c['n'] == 3 for c in m2s.GRID_CASES.values())


def test_plateau_grids_are_the_issue_sizes():
    sizes = {n: tuple(len(g) for g in m2s.plan_grid(c))[::-1] for n, c in m2s.PLATEAU_CASES.items()}
    assert sizes == {'p-runs': (119, 108), 'p-stair': (78, 78), 'p-rows': (17, 40), 'p-cols': (300, 9),
                     'p-const3': (3, 3), 'p-const': (20, 23)}
    for c in m2s.PLATEAU_CASES.values():
        phi, theta = m2s.plan_grid(c)
        up, ut = m2s.unique_grid(c)
        assert np.array_equal(np.unique(phi), up) and np.array_equal(np.unique(theta), ut)


@pytest.mark.parametrize('name', CASE_IDS)
def test_reference_preconditions(name):
    """Measured here (all instances of a table): array and batch cases neighbour margin 3.3e-5 ..
    0.2 dB and height gap >= 2.8e-2 dB; grid cases margin >= 9.3e-4 dB except the dense grids
    (1024, 3) 3.5e-6, (256, 256) 3.5e-5, (64, 1024) 2.2e-6, (1024, 64) 2.4e-6 / 4.7e-6 / 5.5e-6
    (its instance 4 would be 4.5e-7: hence 3 instances); plateau cases margin >= 3.8e-4 dB on the
    unique grid.  Every pixel is above -60 dB everywhere."""
    c = CASES[name]
    for i in range(c['n']):
        r = m2s.reference(c, m2s.snapshots(c, i))
        m = r['spectrum_db']
        where = '%s[%d]' % (name, i)
        print('%s: min P_dB %.2f' % (where, m.min()))
        assert m.min() > -60.0 and m.max() == 0.0
        m2s.check_preconditions(m, r['mask'], c['M'], where)
        assert r['n_peaks'] == int(r['mask'].sum()) >= 1


@pytest.mark.parametrize('name', list(m2s.PLATEAU_CASES))
def test_drop_passes_equal_the_flood_fill(name):
    """The device's scheme restated against imregionalmax by flood fill, on the maps the plateau
    cases scan; and how many passes it takes (measured: p-runs 70, p-stair 12, the others 1).
    n_peaks measured: p-runs 6, p-stair 161 .. 165, p-rows 40, p-cols 1200, p-const3 9, p-const 460."""
    c = CASES[name]
    for i in range(c['n']):
        r = m2s.reference(c, m2s.snapshots(c, i))
        m, mask, peaks, n_peaks = m2s.expected(c, r)
        got, passes = m2s.drop_passes(m)
        print('%s[%d]: %d x %d, %d passes, n_peaks %d, peaks %s' % (name, i, m.shape[0], m.shape[1], passes, n_peaks,
                                                                    list(peaks)))
        assert np.array_equal(got, mask)
        assert passes >= m2s.MIN_PASSES.get(name, 1)
        assert passes <= m.size
        # the unique grid itself has no ties: one pass, over no pixel
        gu, pu = m2s.drop_passes(r['spectrum_db'])
        assert pu == 1 and np.array_equal(gu, r['mask'])
    if name in ('p-const3', 'p-const'):
        assert (m == 0.0).all() and n_peaks == m.size and list(peaks) == [1, 2]
    if name == 'p-cols':
        assert n_peaks % 300 == 0
    if name == 'p-rows':
        assert n_peaks % 40 == 0


def test_drop_passes_on_hand_made_maps():
    """The restatement on maps whose answer is known by inspection: a plateau next to a higher
    pixel is eaten one ring per pass; an isolated plateau stays."""
    row = np.array([[5.0, 3.0, 3.0, 3.0, 3.0, 1.0, 2.0, 2.0, 0.0]])
    img = np.repeat(row, 3, axis=0)
    mask, passes = m2s.drop_passes(img)
    assert np.array_equal(mask, ref.regional_max(img))
    assert mask[:, 0].all() and not mask[:, 1:5].any() and mask[:, 6:8].all() and not mask[:, 8].any()
    # column 1 is no candidate (5 is larger); columns 2, 3, 4 drop one per pass, then the empty pass
    assert passes == 4
    flat = np.zeros((4, 5))
    mask, passes = m2s.drop_passes(flat)
    assert mask.all() and passes == 1


@pytest.mark.parametrize('name', list(m2s.FEW_CASES))
def test_few_cases_have_fewer_peaks_than_sources(name):
    """Measured: `few` 2 regional maxima in all four instances, `few-m8` 1."""
    c = CASES[name]
    counts = [m2s.reference(c, m2s.snapshots(c, i))['n_peaks'] for i in range(c['n'])]
    print(name, 'n_peaks', counts, 'M', c['M'])
    assert all(1 <= k < c['M'] for k in counts)
