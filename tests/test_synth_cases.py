"""CPU preconditions of the synthesis cases (_synth_cases.SYNTH_CASES) and of the reference
(_synth_ref) that the GPU parity module test_synth.py leans on: the oracle alone, no device.

  * rsp.plan.describe accepts every case in both precisions, with the sizes the table names, and
    the table reaches the pulse-block, strip-tail, channel, seed and p_noise conditions it is there for;
  * the targets' sample delays, computed the oracle's way, are exactly the intended list;
  * a target with 0 < ds < N puts samples into the oracle's cube, the others none, ds = N - 1
    exactly one per pulse and channel;
  * _synth_ref's row form equals its whole-cube form bit for bit, and the whole-cube form at
    p_noise = 1 is oracle.chain.synthesize_echo + oracle.chain.philox_noise;
  * the seed's high word changes the noise;
  * the reference's own spread: S4 evaluated with the device's argument order (2 pi (fd prt) m,
    channel phasors e^{i c dphi}) differs from the oracle's order by at most 1e-11 of the cube
    maximum, two orders below the 1e-10 the device cube is held to.
"""
import copy

import numpy as np
import pytest

from oracle import chain
from rsp.plan import describe

import _synth_ref
from _scen import _route_targets
from _synth_cases import (SYNTH_CASES, PROPERTY_CASE, CHAIN_CASE, MAX_TARGETS, edge_delays, synth_scenario,
                          synth_targets, synth_delays, other_targets)

NAMES = list(SYNTH_CASES)
WITH_TARGETS = [n for n in NAMES if SYNTH_CASES[n]['nt']]   # a prefix of NAMES: the noise-only case is last


@pytest.fixture(scope='module')
def case(request):
    """(name, scenario, targets, oracle echo, oracle noise at p_noise = 1, _synth_ref's whole cube at
    the case's p_noise); module-scoped, so pytest runs a case's tests together and one case is held
    at a time."""
    name = request.param
    sy = SYNTH_CASES[name]
    s = synth_scenario(name)
    tg = synth_targets(name, s['cfg'])
    return (name, s, tg, chain.synthesize_echo(tg, s['cfg'], s['pre_o']),
            chain.philox_noise(s['cfg'], sy['frame_idx'], sy['seed']),
            _synth_ref.cube(tg, s['cfg'], s['pre_o'], sy['frame_idx'], sy['seed'], sy['p_noise']))


@pytest.mark.parametrize('prec', ['c128', 'c64'])
@pytest.mark.parametrize('name', NAMES)
def test_plan_accepts_the_case(name, prec):
    sy = SYNTH_CASES[name]
    s = synth_scenario(name)
    sizes, _ = describe(s['cfg'], s['cfar'], s['clus'], s['pre_p'], precision=prec)
    assert (sizes.P, sizes.N, sizes.C, sizes.B, sizes.G) == (sy['P'], sy['N'], sy['C'], sy['B'], 512)
    assert sizes.cube_elems == sy['P'] * sy['N'] * sy['C']
    assert len(s['pre_o']['tx_pulse']) == sy['N'] and s['pre_o']['tx_pulse'][0] == 1


def test_table_reaches_the_kernel_paths():
    """The shapes and arguments the cases are there for, from k_synth's layout: 64 pulse pairs per
    block, strips of 8 samples, workgroups of 32."""
    shapes = {(sy['P'], sy['N'], sy['C']) for sy in SYNTH_CASES.values()}
    assert shapes == {(2, 1024, 1), (6, 999, 5), (128, 1057, 16), (130, 1021, 3), (258, 1031, 32), (332, 1024, 16)}
    pairs = {sy['P'] // 2 for sy in SYNTH_CASES.values()}
    assert {1, 64, 65} <= pairs                                         # one lane; a full block; one lane of a second
    assert any(p > 128 and p % 64 not in (0, 1) for p in pairs)         # a partly active third block
    assert {sy['N'] % 32 for sy in SYNTH_CASES.values()} >= {0, 1, 7, 29}
    assert any(sy['N'] % 8 == 5 for sy in SYNTH_CASES.values())
    assert {1, 16, 32} <= {sy['C'] for sy in SYNTH_CASES.values()}
    assert sum(1 for sy in SYNTH_CASES.values() if sy['seed'] >> 32) >= 2
    assert {sy['p_noise'] for sy in SYNTH_CASES.values()} == {1.0, 4.0, 0.25}
    frames = [sy['frame_idx'] for sy in SYNTH_CASES.values()]
    assert min(frames) == 1 and max(frames) > 2 ** 16 and len(set(frames)) == len(frames)
    assert [n for n in NAMES if SYNTH_CASES[n]['nt'] == 0] == ['p6-n999-noise']
    assert [n for n in NAMES if SYNTH_CASES[n]['nt'] == MAX_TARGETS] == ['p128-n1057']
    assert all(sy['nt'] in (0, MAX_TARGETS) or 17 < sy['nt'] <= 24 for sy in SYNTH_CASES.values())
    assert SYNTH_CASES[PROPERTY_CASE]['P'] == 130 and SYNTH_CASES[CHAIN_CASE]['P'] == 332


@pytest.mark.parametrize('case', WITH_TARGETS, indirect=True)
def test_target_delays_are_the_intended_ones(case):
    name, s, tg = case[:3]
    sy = SYNTH_CASES[name]
    N = sy['N']
    want = synth_delays(name)
    assert len(tg) == sy['nt'] == len(want)
    assert want[:17] == [-3, 0, 1, 7, 8, 9, 31, 32, 33, N - 33, N - 9, N - 8, N - 1, N, N + 5, 100, 100] == edge_delays(N)
    assert all(0 < d < N for d in want[17:])
    # the oracle's way (chain.synthesize_echo): int(mround(2 R / c / ts))
    sc = s['cfg']['Sig_Config']
    got = [int(chain.mround(2 * t['Range'] / sc['c'] / (1.0 / sc['fs']))) for t in tg]
    assert got == want
    assert got == [_synth_ref.sample_delay(t, s['cfg']) for t in tg]
    # a quarter sample off the rounding tie, so a last-bit difference of the quotient cannot move one
    frac = np.array([2 * t['Range'] / sc['c'] * sc['fs'] for t in tg]) - np.array(want)
    np.testing.assert_allclose(frac, 0.25, atol=1e-9)
    vmax = sc['wavelength'] / (2 * sc['prt'])
    vel = np.array([t['Velocity'] for t in tg])
    assert (vel == 0).sum() == 1 and np.abs(vel).max() <= 6 * vmax and np.abs(vel).max() > 3 * vmax
    assert all(abs(t['ElevationAngle']) <= 40 and abs(t['SNR_dB']) <= 20 for t in tg)
    # the rewrite test's second list lies inside the window too
    assert all(0 < _synth_ref.sample_delay(t, s['cfg']) < N for t in other_targets(s['cfg']))


@pytest.mark.parametrize('case', WITH_TARGETS, indirect=True)
def test_targets_inside_the_window_reach_the_oracle_cube(case):
    """Per target, the oracle's cube of that target alone.  Its support does not depend on the
    pulse or the channel (unit-modulus phasors), so the cube is taken at 2 pulses x 2 channels of
    the case's N."""
    name, s, tg = case[:3]
    sy = SYNTH_CASES[name]
    cfg = copy.deepcopy(s['cfg'])
    cfg['Sig_Config'].update(prtNum=2, channel_num=2)
    N = sy['N']
    for t, ds in zip(tg, synth_delays(name)):
        nz = chain.synthesize_echo([t], cfg, s['pre_o']) != 0
        if 0 < ds < N:
            assert nz.any() and not nz[:, :ds, :].any() and nz[:, ds, :].all(), ds
            assert (nz == nz[:1, :, :1]).all()
        else:
            assert not nz.any(), ds
        if ds == N - 1:   # tx_pulse[0] = 1 alone
            assert nz.sum() == 4 and nz[:, N - 1, :].all()


@pytest.mark.parametrize('case', NAMES, indirect=True)
def test_whole_cube_form_is_the_oracle_at_unit_noise_floor(case):
    name, s, tg, echo, noise, whole = case
    sy = SYNTH_CASES[name]
    got = whole if sy['p_noise'] == 1.0 else _synth_ref.cube(tg, s['cfg'], s['pre_o'], sy['frame_idx'], sy['seed'])
    assert got.shape == (sy['P'], sy['N'], sy['C']) and got.dtype == np.complex128
    assert np.array_equal(got, echo + noise)
    # at the case's own p_noise: the echo's amplitude (fsf:62-63) and the noise (fsf:86) scale with its root
    scale = np.sqrt(sy['p_noise'])
    np.testing.assert_allclose(whole, scale * (echo + noise), rtol=0, atol=1e-14 * scale * np.abs(echo + noise).max())


def _sample_rows(sy, tg_delays, count=40, seed=7):
    """(n, c) of the window's and the strips' edges, the targets' first samples and random rows."""
    N, C_ = sy['N'], sy['C']
    rng = np.random.default_rng(seed)
    n = [0, 7, 8, N - 1, N - 1 - (N - 1) % 8, N - 1 - (N - 1) % 32]
    n += [d + k for d in tg_delays for k in (-1, 0, 1) if 0 <= d + k < N]
    n = np.array(n + list(rng.integers(0, N, count)))
    return n, rng.integers(0, C_, n.size)


@pytest.mark.parametrize('case', NAMES, indirect=True)
def test_row_form_equals_whole_cube_form(case):
    name, s, tg, _, _, whole = case
    sy = SYNTH_CASES[name]
    args = (sy['frame_idx'], sy['seed'], sy['p_noise'])
    n, c = _sample_rows(sy, synth_delays(name))
    got = _synth_ref.rows(tg, s['cfg'], s['pre_o'], n, c, *args)
    assert got.shape == (n.size, sy['P'])
    assert np.array_equal(got, whole[:, n, c].T)
    assert np.array_equal(_synth_ref.echo_rows(tg, s['cfg'], s['pre_o'], n, c, sy['p_noise']),
                          _synth_ref.echo_cube(tg, s['cfg'], s['pre_o'], sy['p_noise'])[:, n, c].T)


@pytest.mark.parametrize('case', [PROPERTY_CASE], indirect=True)
def test_p_noise_scales_echo_and_noise(case):
    """fsf:62-63, 86: both parts of the cube scale with sqrt(p_noise); 4 is an exact factor of 2."""
    name, s, tg, echo, noise, _ = case
    sy = SYNTH_CASES[name]
    assert np.array_equal(_synth_ref.echo_cube(tg, s['cfg'], s['pre_o'], 4.0), 2 * echo)
    assert np.array_equal(_synth_ref.noise_cube(s['cfg'], sy['frame_idx'], sy['seed'], 4.0), 2 * noise)
    np.testing.assert_allclose(_synth_ref.echo_cube(tg, s['cfg'], s['pre_o'], 0.25), 0.5 * echo, rtol=1e-15, atol=0)


@pytest.mark.parametrize('case', NAMES, indirect=True)
def test_seed_high_word_and_frame_change_the_noise(case):
    name, s, _, _, noise, _ = case
    sy = SYNTH_CASES[name]
    n, c = _sample_rows(sy, [])
    base = noise[:, n, c].T
    assert np.array_equal(_synth_ref.noise_rows(s['cfg'], n, c, sy['frame_idx'], sy['seed']), base)
    for frame_idx, seed in ((sy['frame_idx'], sy['seed'] & 0xFFFFFFFF), (sy['frame_idx'], sy['seed'] ^ (1 << 32)),
                            (sy['frame_idx'] + 1, sy['seed'])):
        if seed == sy['seed'] and frame_idx == sy['frame_idx']:
            continue   # a case whose seed has no high word: its low 32 bits are the seed
        other = _synth_ref.noise_rows(s['cfg'], n, c, frame_idx, seed)
        assert np.abs(other - base).max() > 1


def _echo_device_order(tg, cfg, pre, p_noise):
    """S4 with the argument order of rsp_synth_targets / k_synth_tab: fd_prt = 2 v / wavelength * prt,
    Doppler phasor of 2 pi fd_prt m, channel phasor of c dphi with dphi in radians, and the product
    amp * (tx * doppler) * channel."""
    sc = cfg['Sig_Config']
    P, N, C_ = sc['prtNum'], sc['point_PRT'], sc['channel_num']
    tx = pre['tx_pulse']
    raw = np.zeros((P, N, C_), complex)
    for t in tg:
        ds = _synth_ref.sample_delay(t, cfg)
        if not 0 < ds < N:
            continue
        fd_prt = 2.0 * t['Velocity'] / sc['wavelength'] * sc['prt']
        amp = np.sqrt(10.0 ** (t['SNR_dB'] / 10.0) * p_noise / pre['P_signal_unscaled'])
        dphi = 2.0 * np.pi * cfg['Array']['element_spacing'] * np.sin(t['ElevationAngle'] * np.pi / 180.0) / sc['wavelength']
        dop = np.exp(1j * (2.0 * np.pi * fd_prt * np.arange(P)))
        cp = np.exp(1j * (np.arange(C_) * dphi))
        nz = np.flatnonzero(tx[:N - ds])
        raw[:, ds + nz, :] += (amp * (tx[None, nz, None] * dop[:, None, None])) * cp[None, None, :]
    return raw


@pytest.mark.parametrize('case', WITH_TARGETS, indirect=True)
def test_reference_spread_between_argument_orders(case):
    name, s, tg, echo, noise, _ = case
    dev = _echo_device_order(tg, s['cfg'], s['pre_o'], 1.0)
    spread = np.abs(dev - echo).max() / np.abs(echo + noise).max()
    print('%s: argument-order spread %.3g of the cube maximum' % (name, spread))
    assert spread <= 1e-11


def test_chain_case_targets_are_detected():
    """test_synth.py's process_targets test compares detection lists: with its targets, seed and
    p_noise the oracle's list is not empty."""
    sy = SYNTH_CASES[CHAIN_CASE]
    s = synth_scenario(CHAIN_CASE)
    tg = _route_targets(s['cfg'], s['ang'])
    raw = _synth_ref.cube(tg, s['cfg'], s['pre_o'], sy['frame_idx'], (0xABCD << 32) | 17, sy['p_noise'])
    fin, st = chain.process_cube(raw, s['cfg'], s['cfar'], s['clus'], s['pre_o'], keep=True)
    print('%d detections, %d final targets' % (len(st['dets']), len(fin)))
    assert len(st['dets']) > 0 and len(fin) > 0
