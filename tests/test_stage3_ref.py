"""The stage-3 range CFAR without a device: the numpy restatement tests/_stage3_ref.py pinned by
answers worked by hand, the reference script's config.cfar, and the device-free half of the C-ABI
(rsp_stage3_describe: segments, notch, envelope and refusals; struct sizes).

The GPU tests are tests/test_stage3_cfar.py.
"""
import ctypes as ct

import numpy as np
import pytest

import _stage3_ref as ref
import rsp
from rsp import _abi
from rsp.plan import describe_stage3, HIT_DTYPE

CFAR = dict(refCells_R=5, saveCells_R=14, T_CFAR=3.0, CFARmethod_R=0, MTD_0v_num=14)


# ------------------------------------------------------------------ known answers
# 3 rows x 12 columns, one segment, r = 2, s = 1 (s + r = 3), T = 2.  P = 3: zc = round(1.5) + 1 = 3,
# MTD_0v_num = 0 notches row 3 alone.
#   row 1 = 1, 2, .., 12 (the value of cell y is y).  mean(L) = ((y-3) + (y-2)) / 2 = y - 2.5,
#     mean(R) = ((y+2) + (y+3)) / 2 = y + 2.5.
#     y = 1..3:   L leaves the segment, so both means are mean(R):  threshold = 2 (y + 2.5) = 2y + 5
#     y = 10..12: R leaves the segment, so both means are mean(L):  threshold = 2 (y - 2.5) = 2y - 5
#     y = 4..9:   greatest of: 2y + 5; smallest of: 2y - 5
#     flag = y >= threshold: never for 2y + 5; for 2y - 5 iff y <= 5, so smallest-of flags y = 4, 5.
#   row 2 = zeros: threshold 0, and 0 >= 0 flags every cell.
#   row 3 is notched: flag 0, threshold 0 whatever it holds.
def _kat_map():
    a = np.zeros((3, 12))
    a[0] = np.arange(1, 13)
    a[2] = 100.0
    return a


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_known_answer_edges_take_the_opposite_window(dtype):
    y = np.arange(1, 13)
    for method in (0, 1):
        f, t = ref.local_execute_cfar(_kat_map(), dict(refCells_R=2, saveCells_R=1, T_CFAR=2.0, CFARmethod_R=method,
                                                       MTD_0v_num=0), (12, 0, 0), dtype)
        assert t.dtype == np.float64 and f.dtype == np.uint8
        assert t[0, :3].tolist() == (2.0 * (y[:3] + 2.5)).tolist()      # first s + r columns: mean(R) T
        assert t[0, 9:].tolist() == (2.0 * (y[9:] - 2.5)).tolist()      # last s + r columns: mean(L) T


def test_known_answer_greatest_of_and_smallest_of_differ():
    y = np.arange(1, 13)
    go, tg = ref.local_execute_cfar(_kat_map(), dict(refCells_R=2, saveCells_R=1, T_CFAR=2.0, CFARmethod_R=0, MTD_0v_num=0),
                                    (12, 0, 0))
    so, ts = ref.local_execute_cfar(_kat_map(), dict(refCells_R=2, saveCells_R=1, T_CFAR=2.0, CFARmethod_R=1, MTD_0v_num=0),
                                    (12, 0, 0))
    assert tg[0, 3:9].tolist() == (2.0 * y[3:9] + 5).tolist()
    assert ts[0, 3:9].tolist() == (2.0 * y[3:9] - 5).tolist()
    assert np.array_equal(tg[0, :3], ts[0, :3]) and np.array_equal(tg[0, 9:], ts[0, 9:])   # one window: no choice
    assert go[0].tolist() == [0] * 12
    assert so[0].tolist() == [0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0]


def test_known_answer_zero_row_flags_everywhere_and_notch_is_zero():
    for method in (0, 1):
        f, t = ref.local_execute_cfar(_kat_map(), dict(refCells_R=2, saveCells_R=1, T_CFAR=2.0, CFARmethod_R=method,
                                                       MTD_0v_num=0), (12, 0, 0))
        assert f[1].tolist() == [1] * 12 and t[1].tolist() == [0.0] * 12     # 0 >= 0
        assert f[2].tolist() == [0] * 12 and t[2].tolist() == [0.0] * 12     # notched, though 100 > anything
        strict, _ = ref.local_execute_cfar(_kat_map(), dict(refCells_R=2, saveCells_R=1, T_CFAR=2.0, CFARmethod_R=method,
                                                            MTD_0v_num=0), (12, 0, 0), strict=True)
        assert strict[1].tolist() == [0] * 12


def test_segments_have_edges_of_their_own():
    """Two segments of 6: every cell of either lies in its segment's first or last s + r = 3 columns,
    so each takes the one window that stays inside its segment."""
    a = np.arange(1, 13, dtype=float)[None, :].repeat(2, axis=0)
    f, t = ref.local_execute_cfar(a, dict(refCells_R=2, saveCells_R=1, T_CFAR=1.0, CFARmethod_R=0, MTD_0v_num=0), (6, 6, 0))
    # row 2 is the notch (zc = round(1) + 1 = 2); row 1: cells 1..3 and 7..9 use R, 4..6 and 10..12 use L
    y = np.arange(1, 13)
    want = np.where(((y - 1) % 6) < 3, y + 2.5, y - 2.5)
    assert t[0].tolist() == want.tolist() and t[1].tolist() == [0.0] * 12
    assert f[0].tolist() == [0, 0, 0, 1, 1, 1] * 2


def test_find_order_is_beam_then_range_outer_doppler_inner():
    a = np.zeros((2, 3, 2))
    fl = np.zeros((2, 3, 2), np.uint8)
    for v, r, b in ((1, 0, 0), (0, 2, 0), (0, 0, 0), (1, 1, 1)):
        fl[v, r, b] = 1
    h = ref.find_hits(a, fl, a)
    assert [tuple(int(x) for x in row[:3]) for row in h] == [(1, 1, 1), (2, 1, 1), (1, 3, 1), (2, 2, 2)]


def test_zero_velocity_centre_is_matlab_round():
    assert [ref.matlab_round(P / 2) + 1 for P in (332, 33, 16)] == [167, 18, 9]
    assert ref.notch_rows(332, 14) == (153, 181)
    assert ref.notch_rows(33, 0) == (18, 18)
    assert ref.notch_rows(16, 16) == (1, 16)


def test_debug_v2_cfar_config():
    c = rsp.config.debug_v2_cfar_config(rsp.debug_v3_config())
    assert c['MTD_0v_num'] == 14
    assert (c['T_CFAR'], c['refCells_R'], c['saveCells_R'], c['CFARmethod_R'], c['MTD_V']) == (3, 5, 14, 0, 3)
    assert c['deltaV'] == pytest.approx(0.2053, abs=1e-4)


# ------------------------------------------------------------------ rsp_stage3_describe (no device)
def test_struct_sizes():
    assert ct.sizeof(_abi.Stage3CfarParams) == 24
    assert ct.sizeof(_abi.Stage3Hit) == 32 == HIT_DTYPE.itemsize
    assert ct.sizeof(_abi.Stage3Info) == 56
    assert _abi.lib().rsp_abi_version() == 4


def test_describe_reference_frame():
    d = describe_stage3(332, (228, 723, 2453), CFAR)
    assert (d['P'], d['G']) == (332, 3404)
    assert d['seg_first'] == (1, 229, 952) and d['seg_len'] == (228, 723, 2453)
    assert d['notch'] == (153, 181)
    assert d['halo'] == 19
    assert d['max_halo'] >= 16 + 32          # the envelope includes r <= 16, s <= 32
    assert d['chunk'] % 4 == 0 and d['rows'] >= 1


def test_describe_odd_rows_and_clipped_notch():
    assert describe_stage3(33, (38, 60, 94), dict(CFAR, MTD_0v_num=0))['notch'] == (18, 18)
    assert describe_stage3(33, (38, 60, 94), dict(CFAR, MTD_0v_num=40))['notch'] == (1, 33)
    assert describe_stage3(16, (64, 192, 256), dict(CFAR, MTD_0v_num=1))['notch'] == (8, 10)
    d = describe_stage3(16, (0, 0, 300), dict(CFAR, MTD_0v_num=1))       # empty segments carry no constraint
    assert d['seg_len'] == (0, 0, 300) and d['seg_first'] == (1, 1, 1)


def test_describe_widest_window_of_the_envelope():
    d = describe_stage3(16, (96, 96, 96), dict(CFAR, refCells_R=16, saveCells_R=32))
    assert d['halo'] == 48


@pytest.mark.parametrize('change, text', [
    (dict(refCells_R=0), 'refCells_R=0'),
    (dict(saveCells_R=-1), 'saveCells_R=-1'),
    (dict(CFARmethod_R=2), 'CFARmethod_R must be 0'),
    (dict(CFARmethod_R=-1), 'CFARmethod_R must be 0'),
    (dict(MTD_0v_num=-1), 'MTD_0v_num must be >= 0'),
    (dict(T_CFAR=0.0), 'T_CFAR must be finite and > 0'),
    (dict(T_CFAR=-3.0), 'T_CFAR must be finite and > 0'),
    (dict(T_CFAR=float('nan')), 'T_CFAR must be finite and > 0'),
    (dict(T_CFAR=float('inf')), 'T_CFAR must be finite and > 0'),
])
def test_describe_refuses_bad_parameters(change, text):
    with pytest.raises(_abi.RspError) as e:
        describe_stage3(332, (228, 723, 2453), dict(CFAR, **change))
    assert e.value.code == _abi.RSP_ERR_INVALID and text in str(e.value)


def test_describe_refuses_a_segment_shorter_than_two_windows():
    assert describe_stage3(33, (38, 60, 94), CFAR)['seg_len'][0] == 38      # exactly 2 (s + r)
    with pytest.raises(_abi.RspError) as e:
        describe_stage3(33, (37, 60, 95), CFAR)
    assert e.value.code == _abi.RSP_ERR_INVALID
    assert 'segment 0 has 37 columns, fewer than 2 (saveCells_R + refCells_R) = 38' in str(e.value)


def test_describe_refuses_a_window_beyond_the_tile():
    top = describe_stage3(16, (200, 200, 200), CFAR)['max_halo']
    assert describe_stage3(16, (200, 200, 200), dict(CFAR, refCells_R=16, saveCells_R=top - 16))['halo'] == top
    with pytest.raises(_abi.RspError) as e:
        describe_stage3(16, (200, 200, 200), dict(CFAR, refCells_R=16, saveCells_R=top - 15))
    assert e.value.code == _abi.RSP_ERR_INVALID and "exceeds the kernel's tile halo %d" % top in str(e.value)


# ------------------------------------------------------------------ the value cases (tests/_cfar_value_cases.py)
import _cfar_value_cases as vc   # noqa: E402

_VC = [(v, p, c) for v in vc.VARIANTS['stage3'] for p in ('c128', 'c64') for c in vc.cases(p)]


@pytest.mark.parametrize('variant, prec, case', _VC, ids=['%s-%s-%s' % x for x in _VC])
def test_value_case_preconditions(variant, prec, case):
    """No value case is hollow: the restatement has the property the case is named for."""
    vc.check_preconditions('stage3', variant, case, prec)


def test_value_case_shape_spans_two_range_chunks():
    d = describe_stage3(vc.S3_P, vc.S3_SEGS, vc.params('stage3', 'go', 1.5))
    assert d['chunk'] < d['G'] < 2 * d['chunk'] and vc.S3_SEGS[0] == 2 * d['halo']
