"""CPU tests of the Doppler CA-CFAR's restatement tests/_vcfar_ref.py, of the device-free
rsp_vcfar_describe and of the literal mirror's handling of ``method``.

The restatement is compared with a plain three-loop transcription of
main_simulate_echoes_with_array_v3.m:278-314 and with a column worked by hand.
"""
import numpy as np
import pytest

import _vcfar_ref as ref
import rsp
from rsp.plan import describe_vcfar


def transcription(rdm_abs, params):
    """local_cfar_detector, line by line (:278-314), 1-based indices kept."""
    num_vel, num_range = rdm_abs.shape
    detection_map = np.zeros((num_vel, num_range), bool)
    threshold_map = np.zeros((num_vel, num_range))
    for r in range(1, num_range + 1):
        range_slice = rdm_abs[:, r - 1]
        for v in range(1, num_vel + 1):
            g_start1 = max(1, v - params['guardCells_V'] // 2)
            r_start1 = max(1, g_start1 - params['refCells_V'])
            r_end1 = g_start1 - 1
            g_end2 = min(num_vel, v + params['guardCells_V'] // 2)
            r_start2 = g_end2 + 1
            r_end2 = min(num_vel, r_start2 + params['refCells_V'] - 1)
            noise_cells = list(range_slice[r_start1 - 1:r_end1]) + list(range_slice[r_start2 - 1:r_end2])
            if not noise_cells:
                noise_level = 0.0
            else:
                s = noise_cells[0]                # mean: the cells added in order, one division
                for x in noise_cells[1:]:
                    s = s + x
                noise_level = s / type(s)(len(noise_cells))
            threshold = noise_level * params['T_CFAR']
            threshold_map[v - 1, r - 1] = threshold
            if rdm_abs[v - 1, r - 1] > threshold:
                detection_map[v - 1, r - 1] = True
    return detection_map, threshold_map


# r = 2, g = 2 (h = 1), T = 1 on the column 1..9, by hand:
#   v = 1, 2: no lead (gs = 1); v = 3 = h + 2: the lead is clipped to row 1 alone, n = 3;
#   v = 4..6: both windows whole, n = 4; v = 7: the trail is row 9 alone, n = 3; v = 8, 9: no trail, n = 2
HAND = dict(refCells_V=2, guardCells_V=2, T_CFAR=1.0)
HAND_COL = np.arange(1.0, 10.0)
HAND_CA = np.array([3.5, 4.5, 4.0, 4.0, 5.0, 6.0, 6.0, 5.5, 6.5])
HAND_GOCA = np.array([3.5, 4.5, 5.5, 6.5, 7.5, 8.5, 9.0, 5.5, 6.5])
HAND_SOCA = np.array([3.5, 4.5, 1.0, 1.5, 2.5, 3.5, 4.5, 5.5, 6.5])


def _map_9x5():
    a = np.random.default_rng(ref.SEED).rayleigh(1.0, (9, 5))
    a[:, 2] = HAND_COL
    return a


def test_windows_clip_at_the_ends():
    assert ref.windows(3, 9, 2, 2) == (1, 1, 5, 6)       # v = h + 2: one lead row left
    assert ref.windows(1, 9, 2, 2) == (1, 0, 3, 4)       # empty lead
    assert ref.windows(7, 9, 2, 2) == (4, 5, 9, 9)
    assert ref.windows(9, 9, 2, 2) == (6, 7, 10, 9)      # empty trail
    assert ref.windows(1, 1, 4, 6) == (1, 0, 2, 1)       # P = 1: both empty
    counts = [sum(max(0, e - s + 1) for s, e in (w[:2], w[2:])) for w in (ref.windows(v, 9, 2, 2) for v in range(1, 10))]
    assert counts == [2, 2, 3, 4, 4, 4, 3, 2, 2]         # n changes over the first and last rows


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_restatement_equals_the_transcription(dtype):
    a = _map_9x5()
    for prm in (HAND, dict(refCells_V=4, guardCells_V=6, T_CFAR=1.5), dict(refCells_V=1, guardCells_V=0, T_CFAR=1.2)):
        f, t = ref.local_cfar_detector(a, prm, ref.CA, dtype)
        if dtype is np.float64:
            df, dt = transcription(a, prm)
        else:   # the transcription in single: numpy float32 scalars round every operation
            p32 = dict(prm, T_CFAR=np.float32(prm['T_CFAR']))
            df, dt = transcription(a.astype(np.float32), p32)
        assert np.array_equal(t, dt.astype(np.float64)) and np.array_equal(f.astype(bool), df)
        assert f.dtype == np.uint8 and t.dtype == np.float64


def test_hand_worked_column():
    a = _map_9x5()
    for method, want in ((ref.CA, HAND_CA), (ref.GOCA, HAND_GOCA), (ref.SOCA, HAND_SOCA)):
        f, t = ref.local_cfar_detector(a, HAND, method)
        assert np.array_equal(t[:, 2], want), (method, t[:, 2])
        assert np.array_equal(f[:, 2], (HAND_COL > want).astype(np.uint8))
    f, _ = ref.local_cfar_detector(a, HAND, ref.CA)
    assert list(f[:, 2]) == [0, 0, 0, 0, 0, 0, 1, 1, 1]                 # rows 4..6 tie: 4 > 4 is false
    g, _ = ref.local_cfar_detector(a, HAND, ref.CA, strict=False)
    assert list(g[:, 2]) == [0, 0, 0, 1, 1, 1, 1, 1, 1]


def test_single_row_has_threshold_zero():
    a = np.array([[0.0, 2.0, 0.5]])
    for method in (ref.CA, ref.GOCA, ref.SOCA):
        f, t = ref.local_cfar_detector(a, dict(refCells_V=4, guardCells_V=6, T_CFAR=6.0), method)
        assert not t.any() and list(f[0]) == [0, 1, 1]                  # flagged exactly when A > 0


def test_make_maps_zero_run():
    a = ref.make_maps(33, 193)
    assert a.shape == (33, 193, 3) and not a[2:14, 3, 1].any() and a[1, 3, 1] > 0 and a[14, 3, 1] > 0
    assert (a[:, :, 0] > 0).all() and (a[:, :, 2] > 0).all()
    b = ref.make_maps(5, 1, n_maps=1)
    assert not b[2:5, 0, 0].any() and b[:2, 0, 0].all()


# ------------------------------------------------------------------ rsp_vcfar_describe
V3 = rsp.config.v3_cfar_params()


def test_v3_cfar_params_are_the_scripts():
    assert V3 == dict(refCells_V=4, guardCells_V=6, refCells_R=4, guardCells_R=6, T_CFAR=6.0, method='GOCA')


def test_describe_fields():
    d = describe_vcfar(332, 3404, V3)
    assert (d['P'], d['G'], d['halo']) == (332, 3404, 7)
    assert d['max_halo'] >= 32 and d['rows'] >= 1 and d['cols'] >= 1
    assert d['row_tiles'] == -(-332 // d['rows']) and d['col_tiles'] == -(-3404 // d['cols'])
    e = describe_vcfar(1, 1, dict(refCells_V=d['max_halo'], guardCells_V=0, T_CFAR=1.0), method='soca')
    assert (e['halo'], e['row_tiles'], e['col_tiles']) == (d['max_halo'], 1, 1)
    assert describe_vcfar(7, 9, dict(refCells_V=12, guardCells_V=40, T_CFAR=2.0))['halo'] == 32


@pytest.mark.parametrize('P, G, change, method', [
    (16, 64, dict(refCells_V=0), 'ca'), (16, 64, dict(refCells_V=-3), 'ca'),
    (16, 64, dict(guardCells_V=-2), 'ca'), (16, 64, dict(guardCells_V=5), 'ca'),
    (16, 64, {}, 3), (16, 64, {}, -1),
    (16, 64, dict(T_CFAR=float('nan')), 'ca'), (16, 64, dict(T_CFAR=float('inf')), 'ca'),
    (16, 64, dict(T_CFAR=0.0), 'ca'), (16, 64, dict(T_CFAR=-1.0), 'ca'),
    (16, 64, dict(refCells_V=10 ** 6), 'ca'), (16, 64, dict(guardCells_V=2 * 10 ** 6), 'ca'),
    (0, 64, {}, 'ca'), (16, 0, {}, 'ca'), (-1, -1, {}, 'ca')])
def test_describe_refusals(P, G, change, method):
    with pytest.raises(rsp.RspError) as e:
        describe_vcfar(P, G, dict(V3, **change), method=method)
    assert e.value.code == rsp._abi.RSP_ERR_INVALID and str(e.value)


def test_describe_refuses_a_halo_past_the_tile():
    m = describe_vcfar(16, 64, V3)['max_halo']
    describe_vcfar(16, 64, dict(refCells_V=m - 3, guardCells_V=6, T_CFAR=6.0))
    with pytest.raises(rsp.RspError) as e:
        describe_vcfar(16, 64, dict(refCells_V=m - 2, guardCells_V=6, T_CFAR=6.0))
    assert e.value.code == rsp._abi.RSP_ERR_INVALID and 'halo' in str(e.value)
    with pytest.raises(ValueError):
        describe_vcfar(16, 64, V3, method='os')


# ------------------------------------------------------------------ the literal mirror
def test_literal_mirror_ignores_method(monkeypatch):
    """rsp.local_cfar_detector always asks for the cell average, whatever params['method'] says (the
    reference's function never reads the field); checked without a device on a stand-in plan."""
    seen = []

    class FakePlan:
        def doppler_cfar(self, amp, cfar, method='ca', hits_cap=None, want_hits=True):
            seen.append((method, want_hits, cfar['refCells_V'], cfar['guardCells_V'], cfar['T_CFAR']))
            f, t = ref.local_cfar_detector(amp, cfar, ref.CA)
            return dict(flags=f, threshold=t, n_hits=int(f.sum()), hits=None)

    monkeypatch.setattr(rsp, '_plan_for', lambda *a, **k: FakePlan())
    a = _map_9x5()
    outs = [rsp.local_cfar_detector(a, dict(HAND, method=m)) for m in ('CA', 'GOCA', 'SOCA')]
    outs.append(rsp.local_cfar_detector(a, HAND))                        # no method field at all
    assert seen == [('ca', False, 2, 2, 1.0)] * 4
    for det, thr in outs:
        assert det.dtype == bool and thr.dtype == np.float64 and det.shape == thr.shape == a.shape
        assert np.array_equal(thr[:, 2], HAND_CA)


# ------------------------------------------------------------------ the value cases (tests/_cfar_value_cases.py)
import _cfar_value_cases as vc   # noqa: E402

_VC = [(v, p, c) for v in vc.VARIANTS['vcfar'] for p in ('c128', 'c64') for c in vc.cases(p)]


@pytest.mark.parametrize('variant, prec, case', _VC, ids=['%s-%s-%s' % x for x in _VC])
def test_value_case_preconditions(variant, prec, case):
    """No value case is hollow: the restatement has the property the case is named for."""
    vc.check_preconditions('vcfar', variant, case, prec)
