"""CPU preconditions of the K2 cases (_scen.K2_CASES) that the GPU parity module test_k2_parity.py
leans on: the oracle and the device-free rsp_plan_describe_k2 (rsp.plan.describe_k2) alone, no
device.

  * the layout of every case and precision is the table's, its segments tile the stitched row and
    its job count is the blocks' sum;
  * the conditions a case is there for (K2_CASES[...]['why']) are derived from its described
    layout, and together the cases reach every one of CONDITIONS; together with the named
    configurations and test_k2_blocks.py they reach every (instantiation, M) pair k2_pc's dispatch
    can take.  Both are set comparisons;
  * every stitched gate lies inside its segment's convolution support (test_k2_blocks.py says why),
    no gate of the oracle's map is zero, and the targets stand out at the gates they were put on
    (the overlap-save segments; the narrow segment has no compression gain);
  * `fir-wrap`: the oracle's wrapped gates are non-zero and its narrow segment differs from the same
    filter without the circshift, so the test cannot pass on a kernel that ignores the delay;
  * the oracle's lfilter + np.roll equals a direct transcription of filter() + circshift
    (fsf:111-112) at the tap counts and delays of the three FIR cases;
  * the per-block metric of test_k2_parity.py fails on an error in the narrow segment that the map
    metric lets through.

Each case prints what it measured (pytest -s).
"""
import numpy as np
import pytest

from oracle import chain
from rsp.plan import describe_k2, K2_SEGMENTS

import test_k2_blocks
from _scen import (K2_CASES, K2_CONDITIONS, scenario, k2_summary, k2_blocks, k2_target_gates, k2_cube, k3_oracle)

PRECS = ('c128', 'c64')
CASES = [(n, p) for n in K2_CASES for p in PRECS]
FIR_CASES = ('fir-wrap', 'fir-8tap', 'fir-1tap')
TWO_FRAME_CASES = ('w4-mb-all', 'mb-pow2')   # test_k2_parity.test_two_frames_per_launch

# What no test ran through k2_pc before these cases, one name per condition:
CONDITIONS = frozenset((
    'w4-multiblock',        # k2_pc<double, 4> stitching more than one block of a segment
    'w4-2560-multiblock',   # ... the 2560-point block more than once per row
    'multiblock-multirow',  # more than one block with several rows per workgroup
    'zaddr-multiblock',     # the same with pass 0's butterflies per row, M / 16, no multiple of NZ:
                            # k2_fft_job's per-element zaddr loads (M = 64 at NZ = 8)
    'nz4',                  # more than one block at NZ = 4
    'lh-gt-half',           # Lh - 1 > M / 2: StoreRowK's rskip beyond its r < R / 2 cap
    'lh-1',                 # a one-tap overlap-save filter: Lh1 = 0
    'exact-full',           # every segment in several blocks, the last one exactly full
    'no-narrow', 'no-medium', 'no-long',
    'g-odd',                # G no multiple of 4: the magnitude maps' row stride Gp > G
    'fir-tail',             # the narrow segment's last 4-gate group is partial
    'fir-wrap-group',       # a whole 4-gate group whose circshift index wraps inside it
    'fir-neg-delay',        # a negative fir_delay
    'fir-even-taps',        # an even tap count (the tap loop runs ntaps - 1 times, unrolled by 4)
    'fir-1tap',             # one tap: no leading zeros, the tap loop's zero-trip case
))


def _describe(s, prec):
    return describe_k2(s['cfg'], s['cfar'], s['clus'], s['pre_p'], precision=prec)


def _instantiation(L, prec):
    return ('double' if prec == 'c128' else 'float', L['wg_per_cu'])


def conditions(L):
    """The CONDITIONS a described layout meets (k2_pc's branch conditions, restated)."""
    c = set()
    segs = L['segments']
    fft = [sg for sg in segs if sg is not None and sg['type'] == 1]
    for sg in fft:
        mb = sg['nblocks'] > 1
        if mb and L['wg_per_cu'] == 4:
            c.add('w4-multiblock')
            if sg['M'] == 2560:
                c.add('w4-2560-multiblock')
        if mb and sg['rows_per_wg'] > 1:
            c.add('multiblock-multirow')
        if mb and sg['M'] != 2560 and (sg['M'] // 16) % L['NZ']:   # pass 0 is radix 16 (plan_os_pow2)
            c.add('zaddr-multiblock')
        if mb and L['NZ'] == 4:
            c.add('nz4')
        if sg['Lh'] - 1 > sg['M'] // 2:
            c.add('lh-gt-half')
        if sg['Lh'] == 1:
            c.add('lh-1')
    if fft and all(sg['nblocks'] > 1 and sg['nblocks'] * sg['V'] == sg['gb'] - sg['ga'] for sg in fft):
        c.add('exact-full')
    for slot, nm in enumerate(K2_SEGMENTS):
        if segs[slot] is None:
            c.add('no-' + nm)
    if max(sg['gb'] for sg in segs if sg is not None) % 4:
        c.add('g-odd')
    fir = segs[0]
    if fir is not None:
        nout = fir['gb'] - fir['ga']
        if nout % 4:
            c.add('fir-tail')
        for q0 in range(0, nout - 3, 4):
            if (fir['ga'] + q0 + fir['delay']) % fir['Ls'] + 3 >= fir['Ls']:
                c.add('fir-wrap-group')
        if fir['delay'] < 0:
            c.add('fir-neg-delay')
        if fir['ntaps'] == 1:
            c.add('fir-1tap')
        elif fir['ntaps'] % 2 == 0:
            c.add('fir-even-taps')
    return c


@pytest.mark.parametrize('name,prec', CASES, ids=['%s-%s' % c for c in CASES])
def test_described_layout(name, prec):
    """test_k2_parity.test_layout's comparison, without a device."""
    kc = K2_CASES[name]
    s = scenario(name)
    sc = s['cfg']['Sig_Config']
    assert (sc['prtNum'], sc['beam_num'], sc['channel_num']) == (kc['P'], kc['B'], 8)
    L = _describe(s, prec)
    assert k2_summary(L) == kc['layout'][prec]
    present = [sg for sg in L['segments'] if sg is not None]
    assert L['nseg'] == len(present) and L['njobs'] == len(k2_blocks(L))
    assert (L['wg_per_cu'] == 4) == (L['k2_pts'] == 2560) and (prec == 'c128' or L['wg_per_cu'] == 2)
    at = 0
    for sg in present:   # the segments tile the stitched row
        assert sg['ga'] == at and sg['gb'] > sg['ga']
        at = sg['gb']
    assert at == s['pre_p']['N_total_gate']
    rows = kc['P'] * kc['B']
    assert L['nwg'] == sum(-(-rows // sg['rows_per_wg']) * (sg['nblocks'] if sg['type'] else 1) for sg in present)


def test_cases_cover_the_conditions():
    """Every condition a case names is one its described layout meets (in either precision), and the
    cases together name every condition of the list."""
    reached = set()
    for name, kc in K2_CASES.items():
        s = scenario(name)
        met = conditions(_describe(s, 'c128')) | conditions(_describe(s, 'c64'))
        assert kc['why'] <= met, '%s: %r not met by its layout (%r)' % (name, sorted(kc['why'] - met), sorted(met))
        reached |= kc['why']
    assert reached == K2_CONDITIONS == CONDITIONS


def test_suite_reaches_every_instantiation_and_block_size():
    """k2_pc's dispatch takes M = 64 .. 2048 and the 2560-point block in the three instantiations,
    and 4096 in the two 2-per-CU ones (a 4096-point block sizes the plan's workgroups for it).  The
    K2 cases, the named configurations and test_k2_blocks.py's together run every pair, and the
    K2 cases alone every pair the others leave out."""
    pow2 = (64, 128, 256, 512, 1024, 2048)
    required = {(t, w, M) for t, w in (('double', 4), ('double', 2), ('float', 2)) for M in pow2 + (2560,)}
    required |= {('double', 2, 4096), ('float', 2, 4096)}

    def pairs(s):
        out = set()
        for prec in PRECS:
            L = _describe(s, prec)
            out |= {_instantiation(L, prec) + (sg['M'],) for sg in L['segments'] if sg is not None and sg['type'] == 1}
        return out

    before = set()
    for name in ('small', 'p256', 'x2', 'x4', 'reference', 'plumbing'):
        before |= pairs(scenario(name))
    for name in test_k2_blocks.CFGS:
        before |= pairs(test_k2_blocks._scen(name))
    cases = set()
    for name in K2_CASES:
        cases |= pairs(scenario(name))
    print('pairs of the earlier suite: %s\npairs of the K2 cases: %s' % (sorted(before), sorted(cases)))
    assert before | cases == required
    assert required - before <= cases and required - before == {
        ('double', 4, 64), ('double', 2, 64), ('float', 2, 64), ('double', 2, 128)}


@pytest.fixture(scope='module', params=list(K2_CASES))
def case(request):
    name = request.param
    s = scenario(name)
    L = _describe(s, 'c128')
    cube = k2_cube(s, L, 'c128')
    pc = chain.pulse_compress(chain.dbf(cube, s['pre_o']['DBF_coeffs_data_C']), s['pre_o'])
    return name, s, L, pc


def test_oracle_preconditions(case):
    name, s, L, pc = case
    pre, N = s['pre_o'], s['cfg']['Sig_Config']['point_PRT']
    nfft = (None, pre['N_fft_med'], pre['N_fft_long'])
    gates = k2_target_gates(L)
    for slot, sg in enumerate(L['segments']):
        if sg is None:
            continue
        Ls = N - sg['seg_lo']
        if sg['type'] == 0:
            assert sg['gb'] - sg['ga'] <= Ls == sg['Ls']
        else:   # outputs 0 .. Ls + Lh - 2 of the convolution of Ls samples with Lh taps
            assert sg['gb'] <= min(Ls, nfft[slot]) + sg['Lh'] - 1 and sg['gb'] <= nfft[slot]
        a = np.abs(pc[:, sg['ga']:sg['gb'], :])
        assert a.min() > 0, '%s: the oracle has an all-zero gate in its %s segment' % (name, K2_SEGMENTS[slot])
        med = np.median(a)
        for g in gates:
            if sg['ga'] <= g < sg['gb']:
                pk = np.abs(pc[:, max(g - 2, sg['ga']):min(g + 3, sg['gb']), :]).max()
                print('%s %s segment: target at gate %d, peak / median %.1f' % (name, K2_SEGMENTS[slot], g, pk / med))
                if sg['type'] == 1 and sg['Lh'] >= 10:   # compression gain
                    assert pk > 3 * med
    assert all(any(sg is not None and sg['ga'] <= g < sg['gb'] for sg in L['segments']) for g in gates)
    fft = [sg for sg in L['segments'] if sg is not None and sg['type'] == 1]
    if fft:   # one target within Lh gates of a block boundary
        bounds = [g0 for sl, _, g0, _ in k2_blocks(L) if L['segments'][sl]['type'] == 1]
        lh = max(sg['Lh'] for sg in fft)
        assert any(0 <= g - b <= lh for g in gates for b in bounds)


def test_oracle_detections(case):
    """The oracle finds detections in every case (the GPU module asserts dets = 'some'), in both
    frames of the two-frames-per-launch cases, and in the complex128 cube no cell under test is
    within 1e-9 of its threshold (1000 x the 1e-12 map tolerance), so the exact comparison of the
    c128 detection sets is meaningful."""
    name, s, L, pc = case
    rdm = chain.mtd(pc, s['pre_o'])
    dets, _ = chain.goca_cfar(rdm, s['cfar'])
    mg = chain.cfar_margin(rdm, s['cfar'])
    print('%s: %d oracle detections, smallest margin %.3g' % (name, len(dets), mg.min()))
    assert len(dets) > 0 and mg.min() >= 1e-9
    if name in TWO_FRAME_CASES:
        _, dets2, _ = k3_oracle(s, k2_cube(s, L, 'c128', frame_idx=2))
        assert len(dets2) > 0


def test_block_metric_sees_what_the_map_metric_misses():
    """An error of 10 x the complex-single bound at one narrow gate (2e-4 of the narrow segment's
    maximum) passes _parity.map_close, which scales by the long segment's target peak, and fails
    test_k2_parity.blocks_close, with the gate in the message."""
    from _parity import MAP_TOL, map_close
    from test_k2_parity import blocks_close
    s = scenario('w4-mb128')
    L = _describe(s, 'c64')
    pc = chain.pulse_compress(chain.dbf(k2_cube(s, L, 'c128'), s['pre_o']['DBF_coeffs_data_C']), s['pre_o'])
    fir = L['segments'][0]
    nmax = np.abs(pc[:, fir['ga']:fir['gb'], :]).max()
    assert nmax <= 0.1 * np.abs(pc).max()
    bad = pc.copy()
    bad[3, 100, 1] += 2e-4 * nmax
    map_close(bad, pc, MAP_TOL['c64'])
    blocks_close(pc, pc, L, MAP_TOL['c64'], 'unchanged')
    with pytest.raises(AssertionError, match='gate 100 .narrow block 0'):
        blocks_close(bad, pc, L, MAP_TOL['c64'], 'one narrow gate off')


def test_fir_wrap_oracle_depends_on_the_shift():
    s = scenario('fir-wrap')
    L = _describe(s, 'c128')
    fir = L['segments'][0]
    wrapped = [g for g in range(fir['gb']) if g + fir['delay'] >= fir['Ls']]
    assert wrapped == list(range(1003, 1015))
    cube = k2_cube(s, L, 'c128')
    iq = chain.dbf(cube, s['pre_o']['DBF_coeffs_data_C'])
    pc = chain.pulse_compress(iq, s['pre_o'])
    assert np.abs(pc[:, wrapped, :]).min() > 0
    unshifted = chain.pulse_compress(iq, dict(s['pre_o'], fir_delay=0))
    d = np.abs(pc - unshifted).max() / np.abs(pc).max()
    print('fir-wrap: oracle with and without the circshift differ by %.3g of the maximum' % d)
    assert d > 0.1


@pytest.mark.parametrize('name', FIR_CASES)
def test_oracle_fir_equals_direct_transcription(name):
    """chain.pulse_compress's narrow segment == y = filter(h, 1, x); circshift(y, -delay) written
    out (fsf:111-112), on a random row.  Bound: a sum of ntaps products in double."""
    s = scenario(name)
    pre = s['pre_o']
    N = s['cfg']['Sig_Config']['point_PRT']
    rng = np.random.default_rng(7)
    x = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    h, d, lo, g1 = np.asarray(pre['MF_narrow'], float), pre['fir_delay'], pre['seg_start_narrow'] - 1, pre['N_gate_narrow']
    seg = x[lo:]
    y = np.array([sum(h[j] * seg[k - j] for j in range(len(h)) if k - j >= 0) for k in range(len(seg))])
    want = np.array([y[(g + d) % len(seg)] for g in range(g1)])
    got = chain.pulse_compress(x[None, :, None], pre)[0, :g1, 0]
    err = np.abs(got - want).max()
    print('%s: %d taps, delay %d: max |lfilter + roll - direct| = %.3g' % (name, len(h), d, err))
    assert err <= 4 * len(h) * np.finfo(float).eps * np.abs(h).sum() * np.abs(x).max()
