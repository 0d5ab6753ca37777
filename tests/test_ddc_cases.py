"""The case table of tests/_ddc_cases.py reaches the tile edges it is there for (CPU: describe_ddc makes no HIP
call), the tiling rule of rsp_geometry.h restated, and describe_ddc's refusals."""
import numpy as np
import pytest

import _ddc_cases as dd
import rsp
from rsp import _abi

BUDGET = 40 * 1024


@pytest.mark.parametrize('prec', dd.PRECS)
@pytest.mark.parametrize('name', sorted(dd.CASES))
def test_case_hits_its_tile_edge(name, prec):
    shape, d = dd.check_preconditions(name, prec)
    print(name, prec, shape['N'], d)


def test_the_table_covers_what_it_promises():
    for prec in dd.PRECS:
        r = {n: dd.resolve(n, prec) for n in dd.CASES}
        assert {d['TP'] for _, d in r.values()} >= {1, 2, 4, 8, 64}
        assert {d['p_tiles'] for _, d in r.values()} >= {1, 2, 3}
        assert {d['k_tiles'] for _, d in r.values()} >= {0, 1, 2, 3}
        assert {s['D'] for s, _ in r.values()} >= {1, 2, 4, 7, 64} and {s['L'] for s, _ in r.values()} >= {1, 2, 12, 13, 64, 512}
        assert {s['C'] for s, _ in r.values()} >= {1, 3, 16} and {s['mode'] for s, _ in r.values()} == {'iq', 'sin'}
        assert {(s['D'], s['off']) for s, _ in r.values()} >= {(2, 1), (4, 3), (7, 6), (64, 63)}
        assert any(s['N'] < s['L'] for s, _ in r.values()) and any(s['N'] == 1 for s, _ in r.values())
        assert {s['dtype'] for s, _ in r.values()} == {np.float32, np.float64}
        # a word whose phase wraps inside a tile: more than one turn over the staged rows
        s, d = r['w-wrap']
        assert s['w'] * d['in_rows'] > 2 ** 64
        # threads: a full workgroup, and the narrow ones of a large D
        assert {d['threads'] for _, d in r.values()} >= {64, 256}


def _tiling(P, No, L, D, prec):
    """rsp_ddc_derive's choice restated: (TP, TK, tap_chunk, threads, lds_bytes)."""
    rs = 8 if prec == 'c128' else 4
    TP = min(64, 1 << max(P - 1, 0).bit_length())
    R = (BUDGET - 16 - L * rs) // (rs * (TP + 2))
    KL = 256 // TP
    while KL > 1 and (KL - 1) * D + min(L, 16) > R:
        KL //= 2
    LC = min(L, R - (KL - 1) * D)
    KPT = 1
    while KPT < 8 and KL * KPT < No and (KL * (KPT + 1) - 1) * D + LC <= R:
        KPT += 1
    TK = KL * KPT
    rows = (TK - 1) * D + LC
    return TP, TK, LC, max(64, TP * KL), ((rows * 2 * rs + 15) & ~15) + rows * TP * rs + L * rs


@pytest.mark.parametrize('prec', dd.PRECS)
def test_tiling_rule_over_a_grid(prec):
    for P in (1, 2, 3, 5, 17, 63, 64, 65, 332):
        for L in (1, 12, 16, 17, 100, 512):
            for D in (1, 3, 4, 64):
                for N in (1, 50, 5000):
                    d = rsp.describe_ddc(P, N, 2, L, D, D - 1, prec)
                    No = max(0, -(-(N - (D - 1)) // D))
                    assert (d['TP'], d['TK'], d['tap_chunk'], d['threads'], d['lds_bytes']) == _tiling(P, No, L, D, prec), (P, L, D, N, d)
                    assert d['No'] == No and d['lds_bytes'] <= BUDGET and d['TK'] % d['k_per_thread'] == 0
                    assert d['in_bytes'] == P * N * 2 * (8 if prec == 'c128' else 4)
                    assert d['out_bytes'] == P * No * 2 * (16 if prec == 'c128' else 8)


def test_flagship_shapes():
    """332 x 23 276 x 16 at L = 12, D = 4 gives 5 819 samples a pulse; the reference's own line is 1 x 50 000."""
    d = rsp.describe_ddc(332, 23276, 16, 12, 4, 0, 'c128')
    assert (d['No'], d['TP'], d['TK'], d['in_rows'], d['p_tiles'], d['tap_chunk']) == (5819, 64, 16, 72, 6, 12)
    assert d['workgroups'] == 6 * -(-5819 // 16) * 16
    d = rsp.describe_ddc(1, 50000, 1, 12, 4, 0, 'c128')
    assert (d['No'], d['TP'], d['TK'], d['p_tiles'], d['threads']) == (12500, 1, 256, 1, 256)


@pytest.mark.parametrize('args, code, text', [
    ((0, 8, 1, 12, 4, 0), _abi.RSP_ERR_INVALID, 'bad sizes P=0 N=8 C=1'),
    ((4, 0, 1, 12, 4, 0), _abi.RSP_ERR_INVALID, 'bad sizes P=4 N=0 C=1'),
    ((4, 8, -1, 12, 4, 0), _abi.RSP_ERR_INVALID, 'bad sizes P=4 N=8 C=-1'),
    ((4, 8, 1, 0, 4, 0), _abi.RSP_ERR_INVALID, 'L=0 taps'),
    ((4, 8, 1, 513, 4, 0), _abi.RSP_ERR_INVALID, 'L=513 taps'),
    ((4, 8, 1, 12, 0, 0), _abi.RSP_ERR_INVALID, 'D=0'),
    ((4, 8, 1, 12, 65, 0), _abi.RSP_ERR_INVALID, 'D=65'),
    ((4, 8, 1, 12, 4, 4), _abi.RSP_ERR_INVALID, 'off=4'),
    ((4, 8, 1, 12, 4, -1), _abi.RSP_ERR_INVALID, 'off=-1'),
    ((1 << 14, 1 << 14, 1, 12, 4, 0), _abi.RSP_ERR_UNSUPPORTED, '32-bit offsets'),      # 2 GB of doubles in
    ((1 << 13, 1 << 14, 1, 12, 1, 0), _abi.RSP_ERR_UNSUPPORTED, '32-bit offsets'),      # 1 GB in, 2 GB out
])
def test_describe_refusals(args, code, text):
    with pytest.raises(_abi.RspError) as e:
        rsp.describe_ddc(*args, 'c128')
    assert e.value.code == code and text in str(e.value)


def test_the_2gb_edge_from_below_and_unknown_precision():
    assert rsp.describe_ddc((1 << 14) - 1, 1 << 14, 1, 12, 4, 0, 'c128')['in_bytes'] == ((1 << 14) - 1) * (1 << 17)
    assert rsp.describe_ddc(1 << 14, 1 << 14, 1, 12, 4, 0, 'c64')['in_bytes'] == 1 << 30   # floats: 1 GB
    assert _abi.lib().rsp_ddc_describe(4, 8, 1, 12, 4, 0, 7, None) == _abi.RSP_ERR_INVALID
    assert b'precision must be' in _abi.lib().rsp_last_error()
    assert _abi.lib().rsp_ddc_describe(4, 8, 1, 12, 4, 0, _abi.RSP_C128, None) == _abi.RSP_OK   # info may be NULL
