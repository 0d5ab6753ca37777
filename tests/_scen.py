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


# ---- K3 (CFAR + S9) window shapes, Doppler bands and tile edges --------------------------------
# One case per path of k3_cfar that the named configurations and the route cases do not reach, each
# on the `plumbing` waveform with 16 channels and a noise-only cube (k3_noise_cube): at these
# thresholds the hits are spread over the whole map, so every band's first and last row under test
# and the outermost range cells carry some.  win = (refR, guardR, refV, guardV); tiling = what
# Plan.k3_tiling() / rsp.plan.describe_k3 must report per precision (the tests assert it, so a
# change of derive_k3_tiling cannot silently move a case off the path it is there for).
# test_k3_window_cases.py holds the oracle's preconditions and prints the measured figures.
#   min         1/0 windows: S9's 4-point Doppler windows at v = 1 and v = P - 2, the max(.., 2) range halo
#   min-r4      the same at T = 0.9: also hits on the outermost range cells under test, r = 1 and
#               r = G - 2 (S9's 4-point range windows; at T = 1.2 these two gates never hit)
#   div37       refR != refV: noise2's two quotients, divisors 3 and 7
#   div37-b2    the same with one beam pair
#   rc17        refR + guardR = 17, no multiple of 4: the first tile starts left of the first cell
#               under test and tile column 0 left of the map
#   rc17-dense  more than K3_QCAP = 1024 hits per tile: the generic kernel's overflow pass
#   bands-hv1   two Doppler bands with a 1-row Doppler halo: S9's rows v +- 2 leave the tile
#   fast-2band  the halo-less 5/10/5/10 kernel with two Doppler bands and thousands of hits
#   empty-r, empty-v   no range cell / no Doppler cell under test
def _k3(P, B, win, T, both, c128, c64):
    return dict(P=P, B=B, C=16, win=win, T=T, tiling={'c128': dict(both, **c128), 'c64': dict(both, **c64)})


_G32 = dict(RT=32, n_tiles=16)
_G64 = dict(RT=64, n_tiles=8)
K3_CASES = {
    'min': _k3(16, 3, (1, 0, 1, 0), 1.2, dict(fast=False, hR=4, n_bands=1, VB=14, rows=16),
               dict(_G32, W=42), dict(_G64, W=72)),
    'min-r4': _k3(16, 3, (1, 0, 1, 0), 0.9, dict(fast=False, hR=4, n_bands=1, VB=14, rows=16),
                  dict(_G32, W=42), dict(_G64, W=72)),
    'div37': _k3(32, 3, (3, 1, 7, 0), 1.5, dict(fast=False, hR=4, n_bands=1, VB=18, rows=32),
                 dict(_G32, W=42), dict(_G64, W=72)),
    'div37-b2': _k3(32, 2, (3, 1, 7, 0), 1.5, dict(fast=False, hR=4, n_bands=1, VB=18, rows=32),
                    dict(_G32, W=42), dict(_G64, W=72)),
    'rc17': _k3(64, 3, (6, 11, 3, 2), 2.0, dict(fast=False, hR=20, n_bands=1, VB=54, rows=64),
                dict(RT=32, n_tiles=15, W=74), dict(_G64, W=104)),
    'rc17-dense': _k3(64, 3, (6, 11, 3, 2), 0.5, dict(fast=False, hR=20, n_bands=1, VB=54, rows=64),
                      dict(RT=32, n_tiles=15, W=74), dict(_G64, W=104)),
    'bands-hv1': _k3(128, 3, (8, 20, 1, 0), 1.5, dict(fast=False, hR=28, n_bands=2, VB=63, rows=65),
                     dict(RT=32, n_tiles=15, W=90), dict(_G64, W=120)),
    'fast-2band': _k3(256, 3, (5, 10, 5, 10), 2.0, dict(fast=True, hR=16, n_bands=2, VB=113, rows=113),
                      dict(_G32, W=34), dict(_G64, W=64)),
    # G = 512 = 2 (100 + 156): no range tile
    'empty-r': _k3(16, 3, (100, 156, 1, 0), 2.0, dict(fast=False, hR=256, n_tiles=0),
                   dict(RT=32, W=546, n_bands=2, VB=7, rows=9), dict(RT=64, W=576, n_bands=1, VB=14, rows=16)),
    # P = 16 = 2 * 8: the band has no row under test (VB = 1 is derive_k3_tiling's floor)
    'empty-v': _k3(16, 3, (1, 0, 8, 0), 1.0, dict(fast=False, hR=4, n_bands=1, VB=1, rows=16),
                   dict(_G32, W=42), dict(_G64, W=72)),
}


def k3_scenario(name):
    kc = K3_CASES[name]
    cfg = plumbing_config(kc['P'], kc['B'], kc['C'])
    W, ang, k = plumbing_weights(cfg)
    rR, gR, rV, gV = kc['win']
    cfar = dict(refCells_R=rR, guardCells_R=gR, refCells_V=rV, guardCells_V=gV, T_CFAR=kc['T'], method='GOCA')
    return cfg, cfar, C.default_cluster_params(), W, ang, k


def k3_noise_cube(s, prec):
    """The noise-only cube of a K3 case: complex128, or rounded to complex64 for the c64 plans."""
    raw = chain.philox_noise(s['cfg'], 1, SEED)
    return raw if prec == 'c128' else raw.astype(np.complex64)


def k3_oracle(s, cube):
    """(rdm, detections, S_all) of the oracle's S5..S8 (process_cube's S9 loop over every hit of
    the dense case takes minutes)."""
    pre = s['pre_o']
    rdm = chain.mtd(chain.pulse_compress(chain.dbf(cube.astype(np.complex128), pre['DBF_coeffs_data_C']), pre), pre)
    dets, S_all = chain.goca_cfar(rdm, s['cfar'])
    return rdm, dets, S_all


def k3_band_edges(P, win, tiling):
    """First and last Doppler row under test (0-based) of every band of a tiling, as k3_cfar's v0, v1."""
    hV = win[2] + win[3]
    out = []
    for b in range(tiling['n_bands']):
        v0, v1 = hV + b * tiling['VB'], min(hV + (b + 1) * tiling['VB'], P - hV)
        out.append((v0, v1 - 1))
    return out


def scenario(name):
    if name in ROUTE_CASES:
        cfg, cfar, clus, W, ang, k = _route_scenario(name)
    elif name in K3_CASES:
        cfg, cfar, clus, W, ang, k = k3_scenario(name)
    else:
        cfg, cfar, clus, W, ang, k = C.named_config(name)
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
