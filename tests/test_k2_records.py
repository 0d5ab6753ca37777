"""K2's per-workgroup records (rsp_plan_describe_k2_records), device-free.

k2_pc's workgroup blockIdx.x reads record blockIdx.x of a table the plan uploads: segment, block,
first row and its index `wg` in job order.  The table replaces the dispatch-order array and the
kernel's search of the job list, so for every configuration it must
  * hold every workgroup of the launch exactly once;
  * give, for each workgroup, the segment, block and first row that the job list (segment by
    segment, block by block, ceil(rows / rows_per_wg) workgroups each) gives for `wg`;
  * keep the dispatch order: `wg` in table order equals this file's restatement of the order's
    rules (rsp_geometry.cpp, derive_k2_order);
  * keep the rows that share a 128-byte line of the K1 -> K2 buffer on one XCD (workgroups go to the
    8 XCDs round-robin by dispatch position: index mod 8), for every position at which all 8 XCD
    queues of the order still hold workgroups.
"""
import numpy as np
import pytest

from rsp.plan import describe_k2, describe_k2_records, K2_RECORD_FIELDS

from _scen import scenario
import test_k2_blocks as blocks

NAMED = ('x2', 'x4', 'reference', 'p256')
CASES = [(n, p) for n in NAMED + tuple(sorted(blocks.CFGS)) for p in ('c128', 'c64')]
SEG, BLK, ROW0, WG = (K2_RECORD_FIELDS.index(f) for f in ('seg', 'blk', 'row0', 'wg'))


def _scen(name):
    return scenario(name) if name in NAMED else blocks._scen(name)


def _jobs(L, rows_total):
    """The job list of a layout: (seg, blk, wg_begin, wg_count, rows_per_wg) in job order."""
    jobs, wg = [], 0
    for si, s in enumerate(x for x in L['segments'] if x is not None):
        n = -(-rows_total // s['rows_per_wg'])
        for blk in range(s['nblocks'] if s['type'] == 1 else 1):
            jobs.append((si, blk, wg, n, s['rows_per_wg']))
            wg += n
    return jobs


def _order(jobs, NZ, esz):
    """The dispatch order's rules restated: groups of gs workgroups (one 128-B line's rows), the
    groups of all blocks of the same rows one unit, units by key to the shortest of 8 queues, the
    queues interleaved, leftovers last.  Returns (order, shortest queue)."""
    gs = 1
    for _, _, _, _, rw in jobs:
        gs = max(gs, min(8, 128 // max(rw * NZ * esz, 1)))
    units, single = [], []
    for si in sorted({j[0] for j in jobs}):
        blks = [j for j in jobs if j[0] == si]
        wc = blks[0][3]
        ng = wc // gs
        for i in range(ng):
            units.append(((i + 0.5) / ng, [j[2] + gs * i + m for j in blks for m in range(gs)]))
        for j in blks:
            single += [j[2] + w for w in range(ng * gs, wc)]
    units.sort(key=lambda u: u[0])   # stable
    q = [[] for _ in range(8)]
    for _, wgs in units:
        x = min(range(8), key=lambda c: (len(q[c]), c))
        q[x] += wgs
    order = [q[x][sl] for sl in range(max(len(v) for v in q)) for x in range(8) if sl < len(q[x])]
    return order + single, min(len(v) for v in q)


@pytest.mark.parametrize('name,prec', CASES)
def test_records_describe_every_workgroup(name, prec):
    s = _scen(name)
    args = (s['cfg'], s['cfar'], s['clus'], s['pre_p'])
    L = describe_k2(*args, precision=prec)
    rec = describe_k2_records(*args, precision=prec)
    sc = s['cfg']['Sig_Config']
    rows_total = sc['beam_num'] * sc['prtNum']
    jobs = _jobs(L, rows_total)
    assert len(jobs) == L['njobs'] and sum(j[3] for j in jobs) == L['nwg']
    # a permutation of all workgroups
    assert rec.shape == (L['nwg'], 4)
    assert np.array_equal(np.sort(rec[:, WG]), np.arange(L['nwg']))
    # each record is what the job list gives for its workgroup
    begins = np.array([j[2] for j in jobs])
    ji = np.searchsorted(begins, rec[:, WG], side='right') - 1
    assert np.array_equal(rec[:, SEG], np.array([j[0] for j in jobs])[ji])
    assert np.array_equal(rec[:, BLK], np.array([j[1] for j in jobs])[ji])
    rw = np.array([j[4] for j in jobs])[ji]
    assert np.array_equal(rec[:, ROW0], (rec[:, WG] - begins[ji]) * rw)
    assert (rec[:, ROW0] < rows_total).all()
    # every (segment, block) covers every row exactly once
    for j in jobs:
        m = (rec[:, SEG] == j[0]) & (rec[:, BLK] == j[1])
        assert np.array_equal(np.sort(rec[m, ROW0]), np.arange(j[3]) * j[4])
    # the dispatch order is the one the rules give
    esz = 16 if prec == 'c128' else 8
    order, qmin = _order(jobs, L['NZ'], esz)
    assert np.array_equal(rec[:, WG], np.array(order))
    # rows of one 128-B line on one XCD, while every XCD queue still holds workgroups; a line of
    # more rows than 8 workgroups (the order's cap on a group) is not kept together
    rpl = max(128 // (L['NZ'] * esz), 1)
    pos = np.arange(L['nwg'])
    checked = 0
    for j in jobs:
        if rpl > 8 * j[4]:
            continue
        m = (rec[:, SEG] == j[0]) & (rec[:, BLK] == j[1])
        line, x, p = rec[m, ROW0] // rpl, pos[m] % 8, pos[m]
        for ln in np.unique(line):
            k = line == ln
            if (p[k] < 8 * qmin).all():
                assert len(set(x[k])) == 1, (j, int(ln))
                checked += 1
    assert checked > 0


def test_records_buffer_protocol():
    """cap = 0 reports the count; a short buffer takes the first records only."""
    import ctypes as ct
    from rsp import _abi
    from rsp.plan import _marshal, _options
    s = scenario('small')
    keep = []
    cfg, cfar, cluster, pre = _marshal(s['cfg'], s['cfar'], s['clus'], s['pre_p'], keep)
    opt = _options(0, 1, 'c128', False, 'amplitude')
    full = describe_k2_records(s['cfg'], s['cfar'], s['clus'], s['pre_p'])
    n = ct.c_int32(-1)
    few = (_abi.K2Record * 5)()
    call = lambda out, cap: _abi.lib().rsp_plan_describe_k2_records(
        ct.byref(cfg), ct.byref(cfar), ct.byref(cluster), ct.byref(pre), ct.byref(opt), 256, out, cap, ct.byref(n))
    assert call(None, 0) == _abi.RSP_OK and n.value == len(full)
    assert call(few, 5) == _abi.RSP_OK and n.value == len(full)
    assert [[getattr(r, f) for f in K2_RECORD_FIELDS] for r in few] == full[:5].tolist()
    assert call(None, 5) == _abi.RSP_ERR_INVALID
    assert _abi.lib().rsp_query_k2_records(None, None, 0, None) == _abi.RSP_ERR_INVALID
