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


# ---- K2 (pulse compression) block counts, filter lengths and FIR edges -------------------------
# One case per path of k2_pc that the named configurations, the route / K3 cases and
# test_k2_blocks.py do not reach.  Every case has 8 channels and, unless it says otherwise, 16
# pulses x 3 beams: 48 rows, so that workgroups of 32 or 64 rows have a partly filled last one, and
# K1 picks NT = 8.  args = rsp.config.make_config's arguments; pre = entries set in both precompute
# dicts (the narrow FIR's taps and shift).  layout = what Plan.k2_layout() / rsp.plan.describe_k2
# must report, per precision where the two differ: wg_per_cu (4: k2_pc<T, 4>, 2: k2_pc<T, 2>),
# k2_pts, NZ and, per segment, (M, Lh, V, nblocks, rows_per_wg), for the narrow FIR (ntaps, delay,
# Ls, rows_per_wg), None for a segment without gates.  The tests assert it, so a change of
# build_fft_segment's cost model cannot silently move a case off the path it is there for.
# test_k2_cases.py holds the oracle's preconditions and the coverage the table must reach.
_PW = dict(gap_duration=(2.84e-6, 4e-6, 6e-6))
_PLUMB = dict(point_PRT=1024, tao=(0.16e-6, 2e-6, 6e-6), gap_duration=(2.84e-6, 8e-6, 12e-6))
_POW2 = dict(point_PRT=2048, tao=(0.16e-6, 1e-6, 2e-6), **_PW)
_V8FIR = (35, 17)   # C.V8_FIR's taps and fir_delay


def _fft(M, Lh, nblocks, rows):
    return dict(M=M, Lh=Lh, V=M - Lh + 1, nblocks=nblocks, rows_per_wg=rows)


def _fir(Ls, rows, ntaps=_V8FIR[0], delay=_V8FIR[1]):
    return dict(ntaps=ntaps, delay=delay, Ls=Ls, rows_per_wg=rows)


def _k2(args, both, c128=None, c64=None, pre=None, P=16, B=3, why=()):
    return dict(P=P, B=B, C=8, args=args, pre=pre or {}, why=frozenset(why),
                layout={'c128': dict(both, **(c128 or {})), 'c64': dict(both, **(c64 or {}))})


_US = 1e-6
_X2_LONG = _fft(2560, 700, 1, 1)
_W4 = dict(wg_per_cu=4, k2_pts=2560)    # complex double beside a 2560-point block: k2_pc<double, 4>
_W2 = dict(wg_per_cu=2, k2_pts=4096)    # k2_pc<T, 2>
_NZ8 = dict(_W2, NZ=8)
_POW2_SEGS = dict(_POW2, point_prt_segments=(62, 301, 1203))
_POW2_FFT = (_fft(128, 25, 3, 32), _fft(256, 50, 6, 16))
_TAPS8 = [3.0, -1.0, 4.0, 1.5, -5.0, 9.0, 2.0, -6.0]


def _w4(narrow, medium, long_):
    """k2_pc<double, 4> in complex double (2048 / M rows per workgroup), k2_pc<float, 2> in complex
    single (4096 / M rows); the 2560-point block takes one row in either."""
    wide = [sg if sg['M'] == 2560 else dict(sg, rows_per_wg=2 * sg['rows_per_wg']) for sg in (medium, long_)]
    return dict(both=dict(NZ=8), c128=dict(_W4, seg=(narrow, medium, long_)), c64=dict(_W2, seg=(narrow, *wide)))


K2_CASES = {
    # k2_pc<double, 4> with more than one block per segment: 128 x 3 (16 rows per workgroup, last
    # block 93 gates) beside 2560 x 1
    'w4-mb128': _k2(dict(point_PRT=4096, tao=(0.16 * _US, 1 * _US, 28 * _US), point_prt_segments=(228, 301, 1860)),
                    **_w4(_fir(4092, 8), _fft(128, 25, 3, 16), _X2_LONG),
                    why=('w4-multiblock', 'multiblock-multirow')),
    # the same with a 10-tap medium filter: 64 x 3 in k2_pc<double, 4> (32 rows per workgroup)
    'w4-m64': _k2(dict(point_PRT=4096, tao=(0.16 * _US, 0.4 * _US, 28 * _US), point_prt_segments=(228, 120, 1860)),
                  **_w4(_fir(4092, 8), _fft(64, 10, 3, 32), _X2_LONG),
                  why=('w4-multiblock', 'zaddr-multiblock')),
    # 512 x 4 (last block 61 gates) and the 2560-point block twice (last block 1839 gates)
    'w4-mb-all': _k2(dict(point_PRT=8192, point_prt_segments=(228, 1000, 3700)),
                     **_w4(_fir(8188, 8), _fft(512, 200, 4, 4), _fft(2560, 700, 2, 1)),
                     why=('w4-multiblock', 'w4-2560-multiblock', 'multiblock-multirow')),
    # 2560 x 3; G = 5949 is no multiple of 4 and the narrow segment's last 4-gate group has 2 gates
    'w4-3blk': _k2(dict(point_PRT=8192, point_prt_segments=(226, 723, 5000)),
                   **_w4(_fir(8188, 8), _fft(1024, 200, 1, 2), _fft(2560, 700, 3, 1)),
                   why=('w4-2560-multiblock', 'g-odd', 'fir-tail')),
    # 2-per-CU workgroups of 32 and 16 rows with 3 and 6 blocks; g1 = 62 ends in a partial 4-gate group
    'mb-pow2': _k2(_POW2_SEGS, dict(_NZ8, seg=(_fir(2044, 8), *_POW2_FFT)), why=('multiblock-multirow', 'fir-tail')),
    # the same blocks behind the persistent K1 (P = 128, B = 8): NT = 4 in complex double
    'mb-pow2-nt4': _k2(_POW2_SEGS, dict(_W2, seg=(_fir(2044, 8), *_POW2_FFT)), c128=dict(NZ=4), c64=dict(NZ=8),
                       P=128, B=8, why=('multiblock-multirow', 'nz4')),
    # every last block exactly full: 3 x 104 and 6 x 207 gates
    'exact-v': _k2(dict(_POW2, point_prt_segments=(62, 312, 1242)), dict(_NZ8, seg=(_fir(2044, 8), *_POW2_FFT)),
                   why=('exact-full',)),
    # 64 x 3 (Lh = 10, last block 10 gates, 64 rows per workgroup: 48 of them in use) and 128 x 5
    'm64-mb': _k2(dict(point_PRT=1024, tao=(0.16 * _US, 0.4 * _US, 1 * _US), point_prt_segments=(30, 120, 500), **_PW),
                  dict(_NZ8, seg=(_fir(1020, 8), _fft(64, 10, 3, 64), _fft(128, 25, 5, 32))),
                  why=('zaddr-multiblock', 'multiblock-multirow', 'fir-tail')),
    # a one-tap medium filter: Lh1 = 0, V = M
    'lh1': _k2(dict(point_PRT=1024, tao=(0.16 * _US, 0.04 * _US, 1 * _US), point_prt_segments=(30, 50, 600), **_PW),
               dict(_NZ8, seg=(_fir(1020, 8), _fft(64, 1, 1, 64), _fft(128, 25, 6, 32))), why=('lh-1',)),
    # the 700-tap long filter in a 1024-point block: V = 325, Lh - 1 > M / 2
    'lh-heavy': _k2(dict(point_PRT=4096, point_prt_segments=(228, 723, 100)),
                    dict(_NZ8, seg=(_fir(4092, 8), _fft(1024, 200, 1, 4), _fft(1024, 700, 1, 4))), why=('lh-gt-half',)),
    # a segment without gates: nseg = 2, the job list and k2order without it
    'no-narrow': _k2(dict(_PLUMB, point_prt_segments=(0, 192, 256)),
                     dict(_NZ8, seg=(None, _fft(256, 50, 1, 16), _fft(512, 150, 1, 8))), why=('no-narrow',)),
    'no-medium': _k2(dict(_PLUMB, point_prt_segments=(64, 0, 256)),
                     dict(_NZ8, seg=(_fir(1020, 8), None, _fft(512, 150, 1, 8))), why=('no-medium',)),
    'no-long': _k2(dict(_PLUMB, point_prt_segments=(64, 192, 0)),
                   dict(_NZ8, seg=(_fir(1020, 8), _fft(256, 50, 1, 16), None)), why=('no-long',)),
    # narrow only, whole-row window: g1 + fir_delay > Ls = 1020, so gates 1003 .. 1014 wrap to the
    # segment's start and the 4-gate group 1000 .. 1003 straddles the wrap; 1015 is no multiple of 4
    'fir-wrap': _k2(dict(_PLUMB, point_prt_segments=(1015, 0, 0)), dict(_NZ8, seg=(_fir(1020, 3), None, None)),
                    why=('fir-wrap-group', 'fir-tail', 'g-odd', 'no-medium', 'no-long')),
    # 8 distinct, non-symmetric taps (an even count below the 4-deep unroll's multiple) and a negative
    # shift: gates 0 .. 2 wrap to the segment's end
    'fir-8tap': _k2(_POW2_SEGS, dict(_NZ8, seg=(_fir(2044, 2, 8, -3), *_POW2_FFT)),
                    pre=dict(MF_narrow=_TAPS8, fir_delay=-3), why=('fir-wrap-group', 'fir-neg-delay', 'fir-even-taps')),
    # one tap, no shift: PADL = 0, the tap loop's zero-trip case
    'fir-1tap': _k2(_POW2_SEGS, dict(_NZ8, seg=(_fir(2044, 8, 1, 0), *_POW2_FFT)),
                    pre=dict(MF_narrow=[2.0], fir_delay=0), why=('fir-1tap',)),
}
# every condition the cases are there for (test_k2_cases.py derives them from describe_k2)
K2_CONDITIONS = frozenset().union(*(kc['why'] for kc in K2_CASES.values()))


def k2_scenario(name):
    kc = K2_CASES[name]
    cfg = C.make_config(prtNum=kc['P'], channel_num=kc['C'], beam_num=kc['B'], **kc['args'])
    W, ang, k = plumbing_weights(cfg)
    return cfg, _route_cfar(kc['P'], 'small'), C.default_cluster_params(), W, ang, k


def k2_summary(L):
    """Plan.k2_layout() / describe_k2 reduced to the fields a K2_CASES layout records."""
    def seg(sg):
        if sg is None:
            return None
        return {k: sg[k] for k in (('ntaps', 'delay', 'Ls', 'rows_per_wg') if sg['type'] == 0 else
                                   ('M', 'Lh', 'V', 'nblocks', 'rows_per_wg'))}
    return dict(wg_per_cu=L['wg_per_cu'], k2_pts=L['k2_pts'], NZ=L['NZ'], seg=tuple(seg(sg) for sg in L['segments']))


def k2_blocks(L):
    """(segment slot, block, g0, gend) of every K2 job of a layout: the narrow segment as one
    block, an overlap-save segment's blocks as k2_fft_job's g0 = ga + blk V, gend = min(gb, g0 + V)."""
    out = []
    for slot, sg in enumerate(L['segments']):
        if sg is None:
            continue
        if sg['type'] == 0:
            out.append((slot, 0, sg['ga'], sg['gb']))
            continue
        for b in range(sg['nblocks']):
            g0 = sg['ga'] + b * sg['V']
            out.append((slot, b, g0, min(sg['gb'], g0 + sg['V'])))
    return out


def k2_target_gates(L):
    """The gates a K2 case's targets sit on: the middle of every present segment, and one within Lh
    gates of a block boundary (just past the first boundary inside a segment of several blocks;
    else just past the start of the first overlap-save segment)."""
    segs = [sg for sg in L['segments'] if sg is not None]
    gates = [(sg['ga'] + sg['gb']) // 2 for sg in segs]
    fft = [sg for sg in segs if sg['type'] == 1]
    multi = [sg for sg in fft if sg['nblocks'] > 1]
    if multi:
        gates.append(multi[-1]['ga'] + multi[-1]['V'] + min(2, multi[-1]['Lh'] - 1))
    elif fft:
        gates.append(fft[0]['ga'] + min(fft[0]['Lh'], fft[0]['gb'] - fft[0]['ga']) // 2)
    return gates


def k2_targets(s, L):
    """Three or four targets of a K2 case, placed from the case's own axes on k2_target_gates."""
    pre, sc = s['pre_o'], s['cfg']['Sig_Config']
    ang, B = pre['beam_angles_deg'], sc['beam_num']
    vmax = sc['wavelength'] / (2 * sc['prt'])
    vel, snr = (0.11, -0.2, 0.3, -0.36), (8.0, 5.0, 10.0, 6.0)
    return [dict(Range=float(pre['range_axis'][max(g, 1)]), Velocity=vel[i % 4] * vmax,
                 ElevationAngle=float(ang[i % B]) + 0.5, SNR_dB=snr[i % 4])
            for i, g in enumerate(k2_target_gates(L))]


def k2_cube(s, L, prec, frame_idx=1):
    """The cube of a K2 case: its targets plus Philox noise, complex128, or rounded to complex64
    for the c64 plans."""
    raw = chain.synthesize_echo(k2_targets(s, L), s['cfg'], s['pre_o']) + chain.philox_noise(s['cfg'], frame_idx, SEED)
    return raw if prec == 'c128' else raw.astype(np.complex64)


def scenario(name):
    if name in ROUTE_CASES:
        cfg, cfar, clus, W, ang, k = _route_scenario(name)
    elif name in K3_CASES:
        cfg, cfar, clus, W, ang, k = k3_scenario(name)
    elif name in K2_CASES:
        cfg, cfar, clus, W, ang, k = k2_scenario(name)
    else:
        cfg, cfar, clus, W, ang, k = C.named_config(name)
    pre_o = oracle_precompute.precompute(cfg, W, ang, k, C.V8_FIR)
    pre_p = product_precompute(cfg, W, ang, k, C.V8_FIR)
    for key, val in K2_CASES.get(name, {}).get('pre', {}).items():   # a K2 case's own narrow FIR
        pre_o[key] = pre_p[key] = val
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


def device_cube(plan, targets, frame_idx=1, seed=SEED, p_noise=1.0):
    """S4 + S4.1 synthesised on the device in the plan's precision, downloaded as [P, N, C]."""
    ptr = plan.device_alloc(plan.cube_bytes)
    try:
        plan.synthesize_device(ptr, targets, frame_idx=frame_idx, seed=seed, p_noise=p_noise)
        plan.sync()
        flat = plan.device_download(ptr, plan.sizes.cube_elems, plan.cdtype)
    finally:
        plan.device_free(ptr)
    return flat.reshape((plan.P, plan.N, plan.C), order='F').astype(np.complex128)
