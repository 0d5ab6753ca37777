"""Shared scenario builders for the tests (oracle = checker, rsp = product)."""
import numpy as np

from rsp import config as C
from rsp.precompute import precompute as product_precompute
from oracle import chain, precompute as oracle_precompute

SEED = 20250101


# ---- slow-time transform routes -------------------------------------------------------------
# One case per route the plan can take for an even prtNum (rsp_query_k1_route), each on the
# `plumbing` waveform (1024 fast-time samples, 512 gates) so that a case stays sub-second on the
# device.  cfar: 'small' = 5/10 range cells with Doppler windows that leave cells under test at
# the case's P (_route_cfar); 'default' = the reference's 5/10/5/10.  route = what Plan.k1_route()
# must report, per precision where the two differ (the GPU tests assert it, so a change of the
# plan's heuristics cannot silently move a case off the kernel it is there to cover).
# dets: 'some' = the oracle finds detections (checked on the CPU by
# test_slowtime_route_cases.py), 'none' = it finds none, 'any' = not relied on (P <= 10: at
# most a few Doppler cells under test).
def _rc(P, B, C_, cfar, dets, both, c128=None, c64=None, precs=('c128', 'c64')):
    return dict(P=P, B=B, C=C_, cfar=cfar, dets=dets, precs=precs,
                route={'c128': dict(both, **(c128 or {})), 'c64': dict(both, **(c64 or {}))})


_K1Q = dict(kernel='persistent_factored', transform='factored')
_TRQ = dict(kernel='tiled', transform='factored', tiles_per_wave=0)
_DIR = dict(kernel='tiled', transform='direct', R=0, Q=0, tiles_per_wave=0, stage2_lgp=0)
_STK = dict(kernel='tiled', transform='stockham', R=0, Q=0, tiles_per_wave=0)
ROUTE_CASES = {
    # factored P = R Q, persistent k1q_dbf_mtd
    'f-6': _rc(6, 4, 16, 'small', 'any', dict(_K1Q, R=2, Q=3, stage2_lgp=0)),       # Qh = 1: one pipelined step
    'f-12': _rc(12, 3, 12, 'small', 'some', dict(_K1Q, R=4, Q=3, stage2_lgp=0)),    # padded beams and channels
    'f-10': _rc(10, 4, 16, 'small', 'any', dict(_K1Q, R=2, Q=5, stage2_lgp=0)),     # Qh even
    'f-20': _rc(20, 4, 16, 'small', 'some', dict(_K1Q, R=4, Q=5, stage2_lgp=0)),
    'f-50': _rc(50, 4, 16, 'small', 'some', dict(_K1Q, R=2, Q=25, NT=8, stage2_lgp=0),   # KH = 13 = 6 + 6 + 1
                c128=dict(tiles_per_wave=4), c64=dict(tiles_per_wave=2)),
    # P = 166 at B = 4: 6 sub-tiles per wave > 4, so the tiled factored kernel by default
    'f-166-b4': _rc(166, 4, 16, 'small', 'some', dict(_TRQ, R=2, Q=83, stage2_lgp=0),
                    c128=dict(NT=4), c64=dict(NT=8)),
    'f-166-b8': _rc(166, 8, 16, 'small', 'some', dict(_K1Q, R=2, Q=83, stage2_lgp=0),
                    c128=dict(NT=2, tiles_per_wave=3), c64=dict(NT=4, tiles_per_wave=3)),
    'f-44-c32': _rc(44, 4, 32, 'small', 'some', dict(_TRQ, R=4, Q=11, stage2_lgp=0)),   # C > 16: no k1q
    # direct O(P^2) DFT
    'd-2': _rc(2, 4, 16, 'small', 'none', _DIR),      # no Doppler cell under test
    'd-4': _rc(4, 4, 16, 'small', 'any', _DIR),
    'd-8': _rc(8, 4, 16, 'small', 'any', _DIR),
    'd-24': _rc(24, 4, 16, 'small', 'some', _DIR),    # R = 8
    'd-96': _rc(96, 4, 16, 'small', 'some', _DIR),    # R = 32
    # a power of two above the Stockham range.  Complex single only: the stage-2 column kernel holds
    # 16 columns of P + 4 in LDS, so a complex-double plan ends at P = 636 (RSP_ERR_UNSUPPORTED)
    'd-1024': _rc(1024, 2, 8, 'small', 'some', dict(_DIR, NT=4), precs=('c64',)),
    # tiled Stockham passes
    's-16': _rc(16, 4, 16, 'default', 'none', dict(_STK, stage2_lgp=4)),    # K3 fast path, empty Doppler band
    # K3 fast path, 2 rows under test: the three targets lie outside them, so a fourth near zero Doppler
    's-32': _rc(32, 4, 16, 'default', 'some', dict(_STK, stage2_lgp=5)),
    's-16s': _rc(16, 4, 16, 'small', 'some', dict(_STK, stage2_lgp=4)),
    's-512-b4': _rc(512, 4, 16, 'small', 'some', dict(_STK, stage2_lgp=9), c128=dict(NT=2), c64=dict(NT=4)),
    's-512-b13': _rc(512, 13, 16, 'small', 'some', dict(_STK, stage2_lgp=9, NT=1)),
}


def _route_cfar(P, kind):
    if kind == 'default':
        return C.default_cfar_params()
    rv, gv = (1, 0) if P < 12 else ((1, 1) if P < 32 else (2, 2))
    return dict(refCells_V=rv, guardCells_V=gv, refCells_R=5, guardCells_R=10, T_CFAR=8.0, method='GOCA')


def plumbing_config(P, B, C_):
    """The `plumbing` waveform (rsp.config.named_config) at P pulses, B beams, C_ channels."""
    return C.make_config(prtNum=P, point_PRT=1024, channel_num=C_, beam_num=B,
                         tao=(0.16e-6, 2e-6, 6e-6), gap_duration=(2.84e-6, 8e-6, 12e-6),
                         point_prt_segments=(64, 192, 256))


def plumbing_weights(cfg):
    """(W, beam angles, K-LUT): rows 0:B, columns 0:C of the reference DBF table with its angles
    and LUT entries for C <= 16; synthetic tapered steering weights at the same angles with the
    amplitude-calibrated slopes for more channels (as the x4 config)."""
    sc = cfg['Sig_Config']
    B, C_ = sc['beam_num'], sc['channel_num']
    ang = list(C.V8_BEAM_ANGLES[:B])
    if C_ <= 16:
        return C.load_reference_dbf()[:B, :C_], ang, list(C.V8_K_LUT[:B - 1])
    import scipy.signal.windows as sw
    d, wl = cfg['Array']['element_spacing'], sc['wavelength']
    W = C.steering_weights(ang, C_, d, wl, taper=sw.taylor(C_, nbar=4, sll=30, norm=False))
    return W, ang, list(C.calibrate_k_slopes_amplitude(W, ang, d, wl))


def _route_scenario(name):
    rc = ROUTE_CASES[name]
    cfg = plumbing_config(rc['P'], rc['B'], rc['C'])
    W, ang, k = plumbing_weights(cfg)
    return cfg, _route_cfar(rc['P'], rc['cfar']), C.default_cluster_params(), W, ang, k


def _route_targets(cfg, ang, slow=False):
    """Three targets placed from the case's own axes (unambiguous range and velocity); slow: a
    fourth near zero Doppler."""
    sc = cfg['Sig_Config']
    rmax = sum(sc['point_prt_segments']) * sc['c'] / (2 * sc['fs'])
    vmax = sc['wavelength'] / (2 * sc['prt'])
    B = sc['beam_num']
    tg = [dict(Range=0.15 * rmax, Velocity=0.11 * vmax, ElevationAngle=ang[1] + 1.0, SNR_dB=5.0),
          dict(Range=0.45 * rmax, Velocity=-0.2 * vmax, ElevationAngle=ang[min(2, B - 1)] - 0.5, SNR_dB=0.0),
          dict(Range=0.8 * rmax, Velocity=0.3 * vmax, ElevationAngle=ang[0] + 0.5, SNR_dB=10.0)]
    if slow:   # between Doppler cells -1 and 0: the only two rows the 5/10 window tests at P = 32
        tg.append(dict(Range=0.6 * rmax, Velocity=-0.5 * vmax / sc['prtNum'], ElevationAngle=ang[1] - 1.0, SNR_dB=10.0))
    return tg


def scenario(name):
    cfg, cfar, clus, W, ang, k = _route_scenario(name) if name in ROUTE_CASES else C.named_config(name)
    pre_o = oracle_precompute.precompute(cfg, W, ang, k, C.V8_FIR)
    pre_p = product_precompute(cfg, W, ang, k, C.V8_FIR)
    return dict(name=name, cfg=cfg, cfar=cfar, clus=clus, pre_o=pre_o, pre_p=pre_p)


def targets_for(name):
    """v8_2's five targets (v8_2:28-51), clipped to the config's coverage; a route case's own three."""
    if name in ROUTE_CASES:
        cfg, _, _, _, ang, _ = _route_scenario(name)
        return _route_targets(cfg, ang, slow=name == 's-32')
    cfg = C.named_config(name)[0]
    sc = cfg['Sig_Config']
    G = sum(sc['point_prt_segments'])
    rmax = 0.9 * G * sc['c'] / (2 * sc['fs'])
    vmax = 0.45 * sc['wavelength'] / (2 * sc['prt'])
    out = []
    for t in C.v8_2_targets():
        if t['Range'] < rmax and abs(t['Velocity']) < vmax:
            out.append(dict(t))
    if not out:
        out = [dict(Range=0.5 * rmax, Velocity=0.3 * vmax, ElevationAngle=10.0, SNR_dB=10.0)]
    return out


def noisy_cube(s, targets, frame_idx=1, seed=SEED, dtype=np.complex64):
    raw = chain.synthesize_echo(targets, s['cfg'], s['pre_o']) + chain.philox_noise(s['cfg'], frame_idx, seed)
    return raw.astype(dtype)


def det_key_set(dets):
    return {(int(d[0]), int(d[1]), int(d[2])) for d in dets}


def device_cube(plan, targets, frame_idx=1, seed=SEED):
    """S4 + S4.1 synthesised on the device in the plan's precision, downloaded as [P, N, C]."""
    ptr = plan.device_alloc(plan.cube_bytes)
    try:
        plan.synthesize_device(ptr, targets, frame_idx=frame_idx, seed=seed)
        plan.sync()
        flat = plan.device_download(ptr, plan.sizes.cube_elems, plan.cdtype)
    finally:
        plan.device_free(ptr)
    return flat.reshape((plan.P, plan.N, plan.C), order='F').astype(np.complex128)
