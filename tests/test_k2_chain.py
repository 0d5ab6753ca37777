"""k2_pc<double, 4>'s per-workgroup chain: the record lookup, the twiddles fetched a pass ahead in
the 2560-point block and the epilogue that takes four gates per lane and trip.

The configurations are x2's waveform (28 us long pulse: one 2560-point block) on 64 pulses and 4
beams, so that a case takes seconds.  They vary what the epilogue's trips and the record table see:
  * the long segment's kept gates: 1860 (x2: two trips of 4 x 256 gates, the second one short) and 1859;
  * the narrow segment's 228 or 229 gates, so that the first long gate (narrow + medium) is odd or even;
  * medium segments whose kept gates end a row in a trip of 3 (723 gates, M = 1024, two rows
    per workgroup), of 2 (401 gates, M = 512, four rows) and of 1 (101 gates, M = 128, 16 rows);
  * 'oddrows': 3 beams x 36 pulses = 108 rows, no multiple of the direct FIR's 8 rows per workgroup
    nor of the 128-point block's 16: the last workgroup of each has rows past the row set.
In complex single the same plans run the 2-per-CU instantiations, which share the record lookup.

Every stitched long gate must lie inside the long convolution's support (test_k2_blocks.py's header
says why); test_cases_are_what_they_claim checks that against the oracle's precompute alone, with
the plan's layout (describe_k2), on the CPU.

Tolerances are the project's (tests/_parity.py): RD map within 1e-12 of its maximum against the
complex128 oracle (2e-5 in complex single), CFAR detection lists identical in complex double, and
the magnitude-only launch bit-identical to the one that also writes the RD map.
"""
import functools

import numpy as np
import pytest

from oracle import chain
from rsp import config as C
from rsp.plan import Plan, describe_k2

import _parity
from _scen import oracle_precompute, product_precompute, SEED

X2_TAO = (0.16e-6, 8e-6, 28e-6)
# name: tao, point_prt_segments, (beams, pulses), medium block, medium rows per workgroup
CASES = {
    'long1860': (X2_TAO, (228, 723, 1860), (4, 64), 1024, 2),
    'long1859': (X2_TAO, (228, 723, 1859), (4, 64), 1024, 2),
    'narrow229': (X2_TAO, (229, 723, 1859), (4, 64), 1024, 2),
    'med401': ((0.16e-6, 4e-6, 28e-6), (228, 401, 1860), (4, 64), 512, 4),
    'oddrows': ((0.16e-6, 1e-6, 28e-6), (228, 101, 1860), (3, 36), 128, 16),
}
U, THREADS = 4, 256   # k2_epilogue: gates per lane and trip, lanes


@functools.lru_cache(maxsize=None)
def _scen(name):
    tao, segs, (B, P), _, _ = CASES[name]
    _, cfar, clus, _, _, _ = C.named_config('small')
    cfg = C.make_config(prtNum=P, point_PRT=4096, channel_num=16, beam_num=B, tao=tao, point_prt_segments=segs)
    W, ang, k = C.load_reference_dbf()[4:4 + B], list(C.V8_BEAM_ANGLES[4:4 + B]), list(C.V8_K_LUT[4:3 + B])
    return dict(cfg=cfg, cfar=cfar, clus=clus, pre_o=oracle_precompute.precompute(cfg, W, ang, k, C.V8_FIR),
                pre_p=product_precompute(cfg, W, ang, k, C.V8_FIR))


def _targets(cfg):
    """v8_2's targets inside the coverage, one in the medium gates and one in the last long gates."""
    sc = cfg['Sig_Config']
    g1, g2, g3 = sc['point_prt_segments']
    dr = sc['c'] / (2 * sc['fs'])
    rmax = 0.9 * (g1 + g2 + g3) * dr
    vmax = 0.45 * sc['wavelength'] / (2 * sc['prt'])
    out = [dict(t) for t in C.v8_2_targets() if t['Range'] < rmax and abs(t['Velocity']) < vmax]
    out.append(dict(Range=(g1 + 0.5 * g2) * dr, Velocity=0.2 * vmax, ElevationAngle=8.0, SNR_dB=12.0))
    out.append(dict(Range=(g1 + g2 + g3 - 40) * dr, Velocity=-0.3 * vmax, ElevationAngle=9.0, SNR_dB=12.0))
    return out


@functools.lru_cache(maxsize=None)
def _reference(name, prec):
    """The cube in the precision's input type and the oracle's result for it (shared, read-only)."""
    s = _scen(name)
    cube = chain.synthesize_echo(_targets(s['cfg']), s['cfg'], s['pre_o']) + chain.philox_noise(s['cfg'], 1, SEED)
    cube = cube.astype(np.complex128 if prec == 'c128' else np.complex64)
    fin, st = chain.process_cube(cube.astype(np.complex128), s['cfg'], s['cfar'], s['clus'], s['pre_o'], keep=True)
    cube.setflags(write=False)
    return cube, fin, st


def _filter_length(mf):
    a = np.abs(np.fft.ifft(np.asarray(mf)))
    return int(np.nonzero(a > 1e-10 * a.max())[0].max()) + 1


@pytest.mark.parametrize('name', sorted(CASES))
def test_cases_are_what_they_claim(name):
    s = _scen(name)
    tao, (g1, g2, g3), (B, P), med_M, med_rows = CASES[name]
    pre = s['pre_o']
    # every stitched long gate inside the long convolution's support: the oracle's precompute alone
    N = s['cfg']['Sig_Config']['point_PRT']
    # (gate g of a segment is output g of the convolution of its N - seg_start + 1 samples with Lh taps)
    assert g1 + g2 + g3 <= (N - pre['seg_start_long'] + 1) + _filter_length(pre['MF_long_fft']) - 1
    assert g1 + g2 <= (N - pre['seg_start_medium'] + 1) + _filter_length(pre['MF_medium_fft']) - 1
    # the plan is the one the case is about
    L = describe_k2(s['cfg'], s['cfar'], s['clus'], s['pre_p'], precision='c128')
    assert (L['wg_per_cu'], L['k2_pts']) == (4, 2560)
    nar, med, lng = L['segments']
    assert (lng['M'], lng['nblocks'], lng['rows_per_wg']) == (2560, 1, 1)
    assert (med['M'], med['nblocks'], med['rows_per_wg']) == (med_M, 1, med_rows)
    assert nar['type'] == 0 and nar['rows_per_wg'] == 8
    assert lng['ga'] == g1 + g2 and lng['gb'] - lng['ga'] == g3 and med['gb'] - med['ga'] == g2
    assert describe_k2(s['cfg'], s['cfar'], s['clus'], s['pre_p'], precision='c64')['wg_per_cu'] == 2
    # the epilogue's trips
    last = lambda n: -(-(n % (U * THREADS) or U * THREADS) // THREADS)   # gates per lane of a row's last trip
    if name == 'long1860':
        assert (g3 > U * THREADS, last(g3), lng['ga'] % 2) == (True, 4, 1)
    if name == 'long1859':
        assert g3 % 2 == 1 and last(g3) == 4
    if name == 'narrow229':
        assert lng['ga'] % 2 == 0 and last(g2) == 3
    if name == 'med401':
        assert last(g2) == 2
    if name == 'oddrows':
        assert last(g2) == 1 and (B * P) % nar['rows_per_wg'] != 0 and (B * P) % med['rows_per_wg'] != 0
    assert all(last(n) * THREADS >= n % (U * THREADS) for n in (g2, g3))
    assert {g2 % U, g3 % U} != {0}   # kept counts that are no multiple of the unroll


@pytest.mark.gpu
@pytest.mark.parametrize('prec', ['c128', 'c64'])
@pytest.mark.parametrize('name', sorted(CASES))
def test_k2_chain_matches_oracle(name, prec):
    s = _scen(name)
    cube, fin, st = _reference(name, prec)
    plan = Plan(s['cfg'], s['cfar'], s['clus'], s['pre_p'], precision=prec)
    try:
        assert plan.k2_layout()['wg_per_cu'] == (4 if prec == 'c128' else 2)
        rec = plan.k2_records()
        assert np.array_equal(np.sort(rec[:, 3]), np.arange(plan.k2_layout()['nwg']))
        gpu = plan.process_cube(cube, frame_idx=1, want_rdm=True, want_cfar=True)
        gpu_mag = plan.process_cube(cube, frame_idx=1, want_rdm=False, want_cfar=True)   # the magnitude-only store
    finally:
        plan.close()
    case = dict(prec=prec, s=s, fin=fin, st=st, gpu=gpu, gpu_mag=gpu_mag)
    _parity.check_rdm(case)
    _parity.check_cfar_map_without_rdm(case)
    got = [(d['v_idx'], d['r_idx'], d['pair_idx']) for d in gpu['detections']]
    print('%s %s: %d detections, %d final targets' % (name, prec, len(got), len(gpu['final_targets'])))
    if prec == 'c128':
        assert got == _parity.keys(st['dets']) and len(got) > 0
        assert len(gpu['final_targets']) == len(fin)
    else:
        _parity.check_detection_sets(case)
