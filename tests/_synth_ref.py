"""Point-wise restatement of S4 (echo synthesis, fsf:45-78) and S4.1 (Philox noise, fsf:80-88) with
the noise floor ``p_noise`` as a parameter -- TEST INFRASTRUCTURE ONLY.

Plain numpy, complex128, written from fun_process_single_frame.m:45-88 and oracle/philox.py.  The
echo follows oracle.chain.synthesize_echo's formulas operation by operation; ``p_noise`` is applied
here (fsf:62-63: amplitude = sqrt(10^(SNR/10) * P_noise_floor / P_signal_unscaled); fsf:86: noise
scaled by sqrt(P_noise_floor / 2)), oracle.chain.synthesize_echo keeps its hard-coded 1.0.

Two forms of the same cube ``raw[m, n, c]`` ([P x N x C], MATLAB index order):

  * ``rows(...)``: the P pulses of each of an arbitrary set of (n, c) rows, [R, P].  A row costs
    O(P x targets), so a frame of the reference's size can be checked at sampled rows without its
    30 s full synthesis;
  * ``cube(...)``: the whole cube, target by target as the oracle does, with one Philox draw over
    all P N C samples.

test_synth_cases.py checks on the CPU that the two agree bit for bit and that ``cube`` at
p_noise = 1 is oracle.chain.synthesize_echo + oracle.chain.philox_noise.
"""
import numpy as np

from oracle.chain import calculate_phase_shifts
from oracle.philox import unit_normal_complex
from oracle.precompute import mround


def sample_delay(t, config):
    """fsf:53-54: the target's delay in fast-time samples, round(2 R / c / ts)."""
    sc = config['Sig_Config']
    return int(mround(2 * t['Range'] / sc['c'] / (1.0 / sc['fs'])))


def _target(t, config, pre, p_noise):
    """(ds, amp * doppler [P], base [N], channel phasors [C]) of one target (fsf:51-72)."""
    sc = config['Sig_Config']
    P, N, C = sc['prtNum'], sc['point_PRT'], sc['channel_num']
    tx = pre['tx_pulse']
    ds = sample_delay(t, config)
    fd = 2 * t['Velocity'] / sc['wavelength']
    dop = np.exp(1j * 2 * np.pi * fd * np.arange(P) * sc['prt'])                          # fsf:58
    amp = np.sqrt(10 ** (t['SNR_dB'] / 10) * p_noise / pre['P_signal_unscaled'])          # fsf:61-63
    base = np.zeros(N, complex)
    if 0 < ds < N:                                                                        # fsf:66-69
        ln = min(len(tx), N - ds)
        base[ds:ds + ln] = tx[:ln]
    ph = np.exp(1j * np.deg2rad(calculate_phase_shifts(
        t['ElevationAngle'], config['Array']['element_spacing'], sc['wavelength'], C)))   # fsf:71-72
    return ds, amp * dop, base, ph


def echo_rows(targets, config, pre, n, c, p_noise=1.0):
    """Noiseless S4 at rows (n[i], c[i]): [R, P] complex128, targets summed in order (fsf:51-78)."""
    n, c = np.asarray(n, np.int64), np.asarray(c, np.int64)
    out = np.zeros((n.size, config['Sig_Config']['prtNum']), complex)
    for t in targets:
        _, ad, base, ph = _target(t, config, pre, p_noise)
        out += ad[None, :] * base[n][:, None] * ph[c][:, None]
    return out


def noise_rows(config, n, c, frame_idx, seed, p_noise=1.0):
    """S4.1 at rows (n[i], c[i]): [R, P].  Row (n, c) is linear indices (c N + n) P .. + P - 1 of the
    cube's [C][N][P] storage (oracle/philox.py)."""
    sc = config['Sig_Config']
    P, N = sc['prtNum'], sc['point_PRT']
    out = np.empty((len(n), P), complex)
    for i, (ni, ci) in enumerate(zip(n, c)):
        out[i] = unit_normal_complex(P, frame_idx, seed, start=(int(ci) * N + int(ni)) * P) * np.sqrt(p_noise / 2)
    return out


def rows(targets, config, pre, n, c, frame_idx, seed, p_noise=1.0):
    """S4 + S4.1 at rows (n[i], c[i]): [R, P] complex128."""
    return echo_rows(targets, config, pre, n, c, p_noise) + noise_rows(config, n, c, frame_idx, seed, p_noise)


def echo_cube(targets, config, pre, p_noise=1.0):
    """Noiseless S4, the whole cube raw[m, n, c]."""
    sc = config['Sig_Config']
    raw = np.zeros((sc['prtNum'], sc['point_PRT'], sc['channel_num']), complex)
    for t in targets:
        _, ad, base, ph = _target(t, config, pre, p_noise)
        nz = np.flatnonzero(base)   # the other samples add (amp dop) * 0 * ph = 0
        raw[:, nz, :] += ad[:, None, None] * base[None, nz, None] * ph[None, None, :]
    return raw


def noise_cube(config, frame_idx, seed, p_noise=1.0):
    """S4.1, the whole cube: linear index = m + P (n + N c)."""
    sc = config['Sig_Config']
    P, N, C = sc['prtNum'], sc['point_PRT'], sc['channel_num']
    z = unit_normal_complex(P * N * C, frame_idx, seed) * np.sqrt(p_noise / 2)
    return z.reshape(C, N, P).transpose(2, 1, 0)


def cube(targets, config, pre, frame_idx, seed, p_noise=1.0):
    """S4 + S4.1, the whole cube raw[m, n, c] complex128."""
    return echo_cube(targets, config, pre, p_noise) + noise_cube(config, frame_idx, seed, p_noise)
