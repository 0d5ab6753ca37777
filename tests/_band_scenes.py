"""Scenes for the band-route tests (test_k2_band_route.py on the device, test_k2_row_sets.py on the
CPU): configurations whose CFAR window is the compile-time 5/5/10/10 one, and targets placed on chosen
Doppler rows from the plan's own velocity axis.

hV = refCells_V + guardCells_V = 15.  The queue pulse-compresses rows [hV, P - hV) and, of the rows
outside them, those a detection reads: a cell at row v reads one when v < 2 hV or v >= P - 2 hV.
"""
import numpy as np

from rsp import config as C
from rsp.precompute import precompute as product_precompute
from oracle import chain, precompute as oracle_precompute

from _scen import scenario, SEED

HV = 15


def p128_scenario():
    """P = 128 with 4 beams: rows 15 .. 112 under test, 30 .. 97 of them away from the edges."""
    cfg = C.make_config(prtNum=128, point_PRT=3072, channel_num=16, beam_num=4, point_prt_segments=(228, 723, 836))
    W, ang, k = C.load_reference_dbf()[4:8], list(C.V8_BEAM_ANGLES[4:8]), list(C.V8_K_LUT[4:7])
    return dict(name='p128', cfg=cfg, cfar=C.default_cfar_params(), clus=C.default_cluster_params(),
                pre_o=oracle_precompute.precompute(cfg, W, ang, k, C.V8_FIR),
                pre_p=product_precompute(cfg, W, ang, k, C.V8_FIR))


CONFIGS = ('small', 'p128', 's-32')
_cache = {}


def band_scenario(name):
    if name not in _cache:
        _cache[name] = p128_scenario() if name == 'p128' else scenario(name)
    return _cache[name]


def edge_rows(P):
    """The Doppler rows (0-based) the issue names, those of them under test at this P."""
    rows = (HV, HV + 1, 2 * HV - 1, 2 * HV, P - 2 * HV - 1, P - 2 * HV, P - HV - 1)
    return sorted({v for v in rows if HV <= v < P - HV})


def reads_edge(v, P):
    return v < 2 * HV or v >= P - 2 * HV


def scene_gates(s):
    """One gate in each range segment, and the first cell of a K3 tile of either precision (tiles
    start at 12 + 32 k in complex double, 12 + 64 k in complex single) inside the medium segment."""
    g1, g2, g3 = s['cfg']['Sig_Config']['point_prt_segments']
    tile = 12 + 64 * ((g1 + g2 // 2) // 64)
    assert g1 <= tile < g1 + g2
    return (g1 // 2, g1 + g2 // 3, g1 + g2 + g3 // 2, tile)


def row_targets(s, rows, snr=12.0):
    """A target on every (row, gate) pair: rows cycle over scene_gates, beams over the pairs."""
    pre, sc = s['pre_o'], s['cfg']['Sig_Config']
    ang = pre['beam_angles_deg']
    gates = scene_gates(s)
    P = sc['prtNum']
    out = []
    for i, v in enumerate(rows):
        # the centre of Doppler row v after fftshift: f_d = 2 V / wavelength = (v - P / 2) / (P prt).  The
        # plan's velocity axis (linspace over P points) lies up to 3/4 of a row off these centres, so
        # its entry v would put the target between rows.
        vel = (v - P // 2) * sc['wavelength'] / (2.0 * sc['prt'] * P)
        assert abs(vel - float(pre['velocity_axis'][v])) < float(pre['deltaV'])
        for j, g in enumerate(gates):
            out.append(dict(Range=float(pre['range_axis'][g]), Velocity=vel,
                            ElevationAngle=float(ang[(i + j) % (len(ang) - 1)]) + 0.7, SNR_dB=snr))
    return out


def scenes(name):
    """{scene name: (targets, rows)}: one scene per edge row, 'interior' where P has such rows, and
    'empty' (noise alone)."""
    s = band_scenario(name)
    P = s['cfg']['Sig_Config']['prtNum']
    out = {'row%d' % v: (row_targets(s, [v]), [v]) for v in edge_rows(P)}
    inner = [v for v in (2 * HV + 8, P // 2 + 3, P - 2 * HV - 9) if not reads_edge(v - 3, P) and not reads_edge(v + 3, P)]
    if inner:
        out['interior'] = (row_targets(s, inner), inner)
    out['empty'] = ([], [])
    return out


_cubes = {}


def scene_cube(name, scene, frame_idx=1):
    """The scene's cube, complex128 (tests round it for a complex-single plan), made once."""
    key = (name, scene, frame_idx)
    if key not in _cubes:
        s = band_scenario(name)
        tg = scenes(name)[scene][0]
        noise = chain.philox_noise(s['cfg'], frame_idx, SEED)
        _cubes[key] = (chain.synthesize_echo(tg, s['cfg'], s['pre_o']) + noise) if tg else noise
    return _cubes[key]
