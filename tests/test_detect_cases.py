"""CPU checks of the detector's case table (tests/_detect_cases.py): the preconditions that make each
case worth running on the device, asserted on the oracle so that a change of a seed cannot hollow a case
out, and the device-free describe call's refusals and tiling arithmetic."""
import numpy as np
import pytest

import _detect_cases as dc
from oracle import chain
from rsp import _abi
from rsp.plan import describe_detect, describe_xcfar

REF = dict(refCells_R=5, guardCells_R=10, refCells_V=5, guardCells_V=10, T_CFAR=8.0)


@pytest.mark.parametrize('name', dc.CASE_IDS)
def test_c128_margin_and_hit_counts(name):
    """The smallest cfar_margin over all cells under test is >= 1e-9, so the oracle and a complex-double
    device can differ only by rounding; a case meant to have hits has some, one meant to have none has none."""
    c = dc.CASES[name]
    for prec in dc.PRECS:
        st, fin = dc.oracle(name, prec)
        n = len(st['dets'])
        mg = chain.cfar_margin(st['rdm'], dc.cfar_dict(c))
        print(name, prec, '%d hits, %d targets, smallest margin %.3g' % (n, len(fin), mg.min()))
        if prec == 'c128':
            assert mg.min() >= 1e-9
        assert (n > 0) == (c['hits'] == 'some') and (len(fin) > 0) == (n > 0)
        assert n <= 400, 'the oracle\'s per-hit spline and BFS are slow'


def test_shapes_the_table_must_hold():
    tv, tg = dc.TILE_V, dc.TILE_G
    shapes = {(c['V'], c['G']) for c in dc.CASES.values()}
    assert {(tv - 1, tg - 1), (tv, tg), (tv + 1, tg + 1)} <= shapes
    assert {c['B'] for c in dc.CASES.values()} >= {2, 13}
    assert any(c['V'] == 333 for c in dc.CASES.values()) and any(c['V'] == 1 for c in dc.CASES.values())
    assert any(c['G'] % 2 == 0 for c in dc.CASES.values()) and any(c['G'] % 2 == 1 for c in dc.CASES.values())
    for name, G in (('g3', 3), ('g4', 4)):
        assert dc.CASES[name]['G'] == G and dc.CASES[name]['win'] == (1, 0, 1, 0)
    for name in ('v1', 'short-g'):
        assert dc.cells_under_test(dc.CASES[name]) == (0, 0, 0, 0)


@pytest.mark.parametrize('name', [n for n in dc.CASE_IDS if dc.CASES[n]['edges']])
def test_hits_in_the_first_and_last_cell_under_test(name):
    c = dc.CASES[name]
    r0, r1, v0, v1 = dc.cells_under_test(c)
    keys = {(int(d[0]), int(d[1])) for d in dc.oracle(name, 'c128')[0]['dets']}
    assert (v0 + 1, r0 + 1) in keys and (v1, r1) in keys


def test_spline_lengths_of_the_narrow_maps():
    """G = 3: every hit's range window has 3 cells; G = 4: 4 cells (fsf:241-250 clipped to the map)."""
    for name, n in (('g3', 3), ('g4', 4)):
        c = dc.CASES[name]
        dets = dc.oracle(name, 'c128')[0]['dets']
        assert len(dets) > 0
        for d in dets:
            r = int(d[1])
            assert min(r + 2, c['G']) - max(r - 2, 1) + 1 == n


def test_dense_case_exceeds_the_first_hit_list():
    dets, _ = chain.goca_cfar(dc.cube('dense', 'c128'), dc.cfar_dict(dc.DENSE))
    mg = chain.cfar_margin(dc.cube('dense', 'c128'), dc.cfar_dict(dc.DENSE))
    print('dense: %d hits, smallest margin %.3g' % (len(dets), mg.min()))
    assert len(dets) > 65536 and mg.min() >= 1e-9


# ---- rsp_detect_describe ---------------------------------------------------------------------------
@pytest.mark.parametrize('args, code, word', [
    ((64, 64, 1), _abi.RSP_ERR_INVALID, 'B=1: a pair sum needs at least 2 beams'),
    ((64, 64, 0), _abi.RSP_ERR_INVALID, 'B=0'),
    ((0, 64, 2), _abi.RSP_ERR_INVALID, 'bad cube shape V=0 G=64 B=2'),
    ((64, 0, 2), _abi.RSP_ERR_INVALID, 'bad cube shape V=64 G=0 B=2'),
    ((1 << 20, 1 << 10, 13), _abi.RSP_ERR_UNSUPPORTED, 'less than 2 GB'),
    ((1 << 14, 1 << 13, 2), _abi.RSP_ERR_UNSUPPORTED, 'less than 2 GB'),      # 2^27 x 2 x 16 B = 4 GB in complex double
])
def test_describe_size_refusals(args, code, word):
    with pytest.raises(_abi.RspError) as e:
        describe_detect(*args, REF)
    assert e.value.code == code and word in str(e.value), str(e.value)


def test_describe_precision_and_limits():
    assert describe_detect(1 << 13, 1 << 13, 2, REF, 'c64')['V'] == 1 << 13      # 2^26 x 2 x 8 B = 1 GB
    with pytest.raises(_abi.RspError):
        describe_detect(1 << 13, 1 << 13, 2, REF, 'c128')                        # 2 GB
    lib = _abi.lib()
    p = _abi.CfarParams(refCells_V=5, guardCells_V=10, refCells_R=5, guardCells_R=10, T_CFAR=8.0)
    assert lib.rsp_detect_describe(64, 64, 2, 7, p, None) == _abi.RSP_ERR_INVALID and b'precision' in lib.rsp_last_error()
    assert lib.rsp_detect_describe(64, 64, 2, _abi.RSP_C128, None, None) == _abi.RSP_ERR_INVALID
    assert lib.rsp_detect_describe(64, 64, 2, _abi.RSP_C128, p, None) == _abi.RSP_OK      # info may be NULL


@pytest.mark.parametrize('change', [dict(refCells_R=0), dict(refCells_V=-3), dict(guardCells_R=-1), dict(guardCells_V=-2),
                                    dict(T_CFAR=0.0), dict(T_CFAR=float('nan')), dict(refCells_R=41, guardCells_R=24),
                                    dict(refCells_V=20, guardCells_V=13)])
def test_describe_gives_the_cfar_refusals_with_their_messages(change):
    cf = dict(REF, **change)
    with pytest.raises(_abi.RspError) as a:
        describe_xcfar(332, 3404, cf)
    with pytest.raises(_abi.RspError) as b:
        describe_detect(332, 3404, 13, cf)
    assert a.value.code == b.value.code and str(a.value) == str(b.value)


def test_tiling_arithmetic():
    d = describe_detect(1, 1, 2, REF)
    rows, cols = d['rows'], d['cols']
    assert (rows, cols) == (dc.TILE_V, dc.TILE_G)
    assert d['lds_bytes'] == rows * (cols + 1) * 8 and describe_detect(1, 1, 2, REF, 'c64')['lds_bytes'] == rows * (cols + 1) * 4
    assert (d['lds_bytes'] // (rows * 8)) % 2 == 1      # the padding rule: an odd row stride in elements
    for V, G, rt, ct_ in ((rows - 1, cols - 1, 1, 1), (rows, cols, 1, 1), (rows + 1, cols + 1, 2, 2), (rows + 1, cols - 1, 2, 1),
                          (2 * rows, 3 * cols + 1, 2, 4), (1, 1, 1, 1), (512, 3404, 8, 54)):
        for B in (2, 13):
            d = describe_detect(V, G, B, REF)
            assert (d['V'], d['G'], d['B'], d['n_pairs'], d['row_tiles'], d['col_tiles']) == (V, G, B, B - 1, rt, ct_)
            x = describe_xcfar(V, G, REF)
            assert (d['r0'], d['r1'], d['v0'], d['v1']) == (x['r0'], x['r1'], x['v0'], x['v1'])
            cut = max(G - 30, 0) * max(V - 30, 0) if G > 30 and V > 30 else 0
            assert d['cells_under_test'] == cut and d['max_detections'] == (B - 1) * cut
    d = describe_detect(512, 3404, 13, REF)
    assert d['cells_under_test'] == 482 * 3374 and d['max_detections'] == 12 * 482 * 3374
