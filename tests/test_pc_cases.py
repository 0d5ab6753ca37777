"""CPU tests of the stand-alone pulse compression's case table (_pc_cases.py): describe_pc equals the
derivation restated in Python for every case the GPU tests launch, and the table reaches the paths it is
there for -- proved from describe_pc, without a device."""
import pytest

import rsp
from rsp import _abi
from rsp.plan import describe, describe_k2, describe_pc

import _pc_cases as pcc

CASES = [(n, P, B, prec) for n, P, B, precs in pcc.gpu_cases() for prec in precs]
_SCEN = {}


def scen(name):
    if name not in _SCEN:
        _SCEN[name] = pcc.pc_scenario(name)
    return _SCEN[name]


def info(name, P, B, prec):
    s = scen(name)
    return describe_pc(s['cfg'], s['cfar'], s['clus'], s['pre_p'], P, B, precision=prec)


@pytest.mark.parametrize('name, P, B, prec', CASES, ids=['%s-P%d-B%d-%s' % c for c in CASES])
def test_describe_pc_equals_the_restated_derivation(name, P, B, prec):
    s = scen(name)
    args = (s['cfg'], s['cfar'], s['clus'], s['pre_p'])
    L = describe_k2(*args, precision=prec)       # the scenario's own plan: the segments do not depend on its P, B
    sizes, _ = describe(*args, precision=prec)
    assert describe_pc(*args, P, B, precision=prec) == pcc.expected_info(L, sizes, P, B, prec)


def test_the_plans_own_pulse_and_beam_count_play_no_part():
    s = scen(pcc.ORACLE_CASE)
    ref = describe_pc(s['cfg'], s['cfar'], s['clus'], s['pre_p'], 333, 5)
    for P0 in (2, 16, 333, 1000001):
        cfg = pcc.with_prt_num(s['cfg'], P0)
        assert describe_pc(cfg, s['cfar'], s['clus'], s['pre_p'], 333, 5) == ref


def test_a_pulse_count_no_plan_takes():
    """describe refuses prtNum = 333; describe_pc of the same configuration succeeds at P = 333."""
    s = scen(pcc.ORACLE_CASE)
    cfg = pcc.with_prt_num(s['cfg'], 333)
    with pytest.raises(_abi.RspError) as e:
        describe(cfg, s['cfar'], s['clus'], s['pre_p'])
    assert e.value.code == _abi.RSP_ERR_UNSUPPORTED and 'odd prtNum 333' in str(e.value)
    d = describe_pc(cfg, s['cfar'], s['clus'], s['pre_p'], 333, 3)
    assert (d['P'], d['B'], d['nzc']) == (333, 3, 88)
    assert rsp.describe_pc is describe_pc


def test_coverage_the_table_must_reach():
    got = {(n, P, B, prec): info(n, P, B, prec) for n, P, B, prec in CASES}
    # a second interval that starts at a compacted index that is no multiple of NZ, and nU % NZ != 0
    d = info(pcc.ORACLE_CASE, 7, 3, 'c128')
    assert d['n_intervals'] >= 2 and d['ivl_start'][1] % d['NZ'] != 0, d
    assert d['nU'] % d['NZ'] != 0
    # a chunk that straddles the two intervals: its first and last slot lie on either side of the start
    c = d['ivl_start'][1] // d['NZ']
    assert c * d['NZ'] < d['ivl_start'][1] < (c + 1) * d['NZ'] <= d['nU']
    for prec in pcc.PRECS:
        Ps = {P for n, P, B, p in got if p == prec}
        # one below, on, one above either tile's pulse extent and the pulses one unpack workgroup walks
        for ext in (pcc.PACK_COLS, pcc.UNPACK_ROWS, pcc.UNPACK_ROWS * pcc.UNPACK_GROUP):
            assert {ext - 1, ext, ext + 1} <= Ps, (prec, ext)
        assert 1 in Ps
        Gs = {d['G'] % pcc.UNPACK_COLS[prec] for (n, P, B, p), d in got.items() if p == prec}
        assert {pcc.UNPACK_COLS[prec] - 1, 0, 1} <= Gs, (prec, Gs)
        assert any(d['G'] % 4 for d in got.values())
    assert any(P % 2 and P > 1 for n, P, B, p in got if p == 'c64')            # odd P in complex single
    assert {d['k2_wg_per_cu'] for d in got.values()} == {2, 4}                 # both k2_pc instantiations
    # a case whose last K2 workgroup has unused rows: B P is no multiple of some segment's rows_per_wg
    s = scen(pcc.ORACLE_CASE)
    L = describe_k2(s['cfg'], s['cfar'], s['clus'], s['pre_p'])
    assert any((3 * 16) % sg['rows_per_wg'] for sg in L['segments'] if sg is not None)
    # more than one pack tile along the pulse axis, with a last tile shorter than the first
    assert info(pcc.ORACLE_CASE, 333, 3, 'c128')['pack_wg'] == 2 * 88 * 3
    # two unpack workgroups along the pulse axis: the second walks one tile of one pulse
    d = info(pcc.ORACLE_CASE, 513, 3, 'c64')
    assert d['unpack_wg'] == -(-d['G'] // 64) * 2 * 3


@pytest.mark.parametrize('P, B, code, word', [
    (0, 3, _abi.RSP_ERR_INVALID, 'bad sizes P=0 B=3 (P, B >= 1)'),
    (-5, 3, _abi.RSP_ERR_INVALID, 'bad sizes P=-5 B=3 (P, B >= 1)'),
    (16, 0, _abi.RSP_ERR_INVALID, 'bad sizes P=16 B=0 (P, B >= 1)'),
    (16, -1, _abi.RSP_ERR_INVALID, 'bad sizes P=16 B=-1 (P, B >= 1)'),
    (1 << 20, 1 << 10, _abi.RSP_ERR_UNSUPPORTED, '1048576 pulses x 1024 beams of 1024 samples, 650 gates'),
    (2 ** 31 - 1, 2 ** 31 - 1, _abi.RSP_ERR_UNSUPPORTED, '32-bit offsets (< 2 GB each)'),
])
def test_refusals_and_messages(P, B, code, word):
    s = scen(pcc.ORACLE_CASE)
    with pytest.raises(_abi.RspError) as e:
        describe_pc(s['cfg'], s['cfar'], s['clus'], s['pre_p'], P, B)
    assert e.value.code == code
    assert word in str(e.value), str(e.value)


def test_two_gigabytes_is_by_the_precision_and_the_largest_of_the_three():
    """N = 1024 samples per row (the beams are the largest side of this case): 2^31 / 1024 / 16 = 131072 rows of
    complex double reach 2 GB, one fewer does not; complex single takes twice as many."""
    s = scen(pcc.ORACLE_CASE)
    args = (s['cfg'], s['cfar'], s['clus'], s['pre_p'])
    assert describe_pc(*args, 131071, 1, precision='c128')['P'] == 131071
    assert describe_pc(*args, 1, 262143, precision='c64')['B'] == 262143
    for P, B, prec in ((131072, 1, 'c128'), (1, 131072, 'c128'), (512, 512, 'c64')):
        with pytest.raises(_abi.RspError) as e:
            describe_pc(*args, P, B, precision=prec)
        assert e.value.code == _abi.RSP_ERR_UNSUPPORTED
