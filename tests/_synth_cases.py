"""The synthesis cases: shapes, targets and generator arguments at which k_synth (S4 + S4.1 on the
device, rsp_frame_aux.hip) is compared with _synth_ref.  test_synth_cases.py holds the CPU
preconditions, test_synth.py the GPU parity.

k_synth gives a lane the pulse pair (m, m + 1), m = 2 (64 blockIdx.x + lane), a wave a strip of 8
fast-time samples of one channel and a workgroup four such strips (32 samples).  One case per path
of that layout which the named configurations' parity tests (P = 64 and 128, N a multiple of 32,
16 channels, seed 20250101, p_noise 1) do not reach.  Every case is on the `plumbing` waveform with
its own point_PRT = N; B beams and _scen._route_cfar's 'small' window, which the plan accepts at
that P (test_synth_cases.py asks rsp.plan.describe).

  nt        targets: the 17 of edge_delays plus random ones up to nt; 0: a noise-only frame
  frame_idx counter word 2 of the Philox block, from 1 to above 2^16
  seed      the Philox key; two cases carry a non-zero high word
  p_noise   the noise floor, of 1.0, 4.0, 0.25: the echo amplitude and the noise scale with it
"""
import numpy as np

from rsp import config as C
from rsp.precompute import precompute as product_precompute
from oracle import precompute as oracle_precompute

from _scen import _route_cfar, plumbing_weights

MAX_TARGETS = 64   # RSP_MAX_SYNTH_TARGETS: they travel in the kernel arguments


def _sy(P, N, C_, B, nt, frame_idx, seed, p_noise):
    return dict(P=P, N=N, C=C_, B=B, nt=nt, frame_idx=frame_idx, seed=seed, p_noise=p_noise)


SYNTH_CASES = {
    # one active lane of one pulse block, one channel: the other 63 lanes of every wave retire unwritten
    'p2-c1': _sy(2, 1024, 1, 2, 20, 1, 20250101, 1.0),
    # N % 32 = 7: the last workgroup has one wave with 7 samples (the `n < N` / break cut), three waves retire
    'p6-n999': _sy(6, 999, 5, 2, 20, 2, (0xABCD << 32) | 17, 4.0),
    # one exactly full pulse block (64 pairs); N = 33 * 32 + 1: a last workgroup of a single sample; the
    # target cap of 64
    'p128-n1057': _sy(128, 1057, 16, 4, MAX_TARGETS, 3, 20250101, 0.25),
    # a second pulse block with one active lane (65 pairs); N % 8 = 5: a last wave of 5 samples
    'p130-n1021': _sy(130, 1021, 3, 2, 22, 70001, 20250101, 1.0),
    # three pulse blocks (129 pairs = 2 * 64 + 1), 32 channels as x4 has them; the high seed word all ones
    'p258-c32': _sy(258, 1031, 32, 2, 20, 255, (0xFFFFFFFF << 32) | 0x80000001, 1.0),
    # the reference frame's pulse count: 166 pairs = 2 * 64 + 38, a partly active last pulse block
    'p332': _sy(332, 1024, 16, 4, 20, 100000, 20250101, 4.0),
    # the tail shape again without targets: no phasor table launch, the noise alone
    'p6-n999-noise': _sy(6, 999, 5, 2, 0, 65536, 20250101, 0.25),
}

PROPERTY_CASE = 'p130-n1021'   # the scaling, generator and rewrite properties of test_synth.py
CHAIN_CASE = 'p332'            # process_targets against process_cube of the device's cube


def edge_delays(N):
    """The sample delays every case with targets carries: refused ones (ds <= 0, ds >= N), the first
    and last samples of the window, one below / on / above the strip (8) and workgroup (32) edges
    from either end, and two targets at the same delay."""
    return [-3, 0, 1, 7, 8, 9, 31, 32, 33, N - 33, N - 9, N - 8, N - 1, N, N + 5, 100, 100]


def synth_config(sy):
    """The `plumbing` waveform at the case's P, N, C and B (rsp.config.make_config)."""
    return C.make_config(prtNum=sy['P'], point_PRT=sy['N'], channel_num=sy['C'], beam_num=sy['B'],
                         tao=(0.16e-6, 2e-6, 6e-6), gap_duration=(2.84e-6, 8e-6, 12e-6),
                         point_prt_segments=(64, 192, 256))


def range_of_delay(ds, cfg):
    """A range whose delay rounds to ds samples in numpy and in C++ alike: a quarter sample off the tie."""
    sc = cfg['Sig_Config']
    return (ds + 0.25) * sc['c'] / (2 * sc['fs'])


def synth_delays(name):
    """The intended sample delay of every target of a case, in target order."""
    sy = SYNTH_CASES[name]
    if sy['nt'] == 0:
        return []
    rng = np.random.default_rng([sy['P'], sy['N'], sy['C'], 1])
    edge = edge_delays(sy['N'])
    return edge + [int(d) for d in rng.integers(1, sy['N'], sy['nt'] - len(edge))]


def synth_targets(name, cfg):
    """The case's targets: velocities uniform in +-6 unambiguous velocities (Doppler arguments of
    thousands of radians, aliased tones), the one at ds = 1 exactly 0; elevation +-40 deg; SNR +-20 dB."""
    sy = SYNTH_CASES[name]
    sc = cfg['Sig_Config']
    vmax = sc['wavelength'] / (2 * sc['prt'])
    rng = np.random.default_rng([sy['P'], sy['N'], sy['C'], 2])
    tg = [dict(Range=float(range_of_delay(ds, cfg)), Velocity=float(rng.uniform(-6.0, 6.0) * vmax),
               ElevationAngle=float(rng.uniform(-40.0, 40.0)), SNR_dB=float(rng.uniform(-20.0, 20.0)))
          for ds in synth_delays(name)]
    if tg:
        tg[2]['Velocity'] = 0.0   # ds = 1
    return tg


def other_targets(cfg):
    """A second, shorter target list for the rewrite test: other delays, velocities and angles."""
    sc = cfg['Sig_Config']
    vmax = sc['wavelength'] / (2 * sc['prt'])
    return [dict(Range=float(range_of_delay(ds, cfg)), Velocity=v * vmax, ElevationAngle=a, SNR_dB=s)
            for ds, v, a, s in ((5, 1.7, -12.0, 6.0), (64, -3.3, 25.0, -4.0), (sc['point_PRT'] - 40, 0.4, 3.0, 12.0))]


def synth_scenario(name):
    """The dict _scen.scenario gives, for a synthesis case."""
    sy = SYNTH_CASES[name]
    cfg = synth_config(sy)
    W, ang, k = plumbing_weights(cfg)
    pre_o = oracle_precompute.precompute(cfg, W, ang, k, C.V8_FIR)
    pre_p = product_precompute(cfg, W, ang, k, C.V8_FIR)
    return dict(name=name, cfg=cfg, cfar=_route_cfar(sy['P'], 'small'), clus=C.default_cluster_params(),
                pre_o=pre_o, pre_p=pre_p, ang=ang)
