"""Case table of the detector on any RD cube (test_detect_cases.py checks its preconditions on the CPU,
test_detect.py runs it on the device): seeded Gaussian cubes with a few injected peaks, caller-given axes,
and the oracle's S8-S11 on the same cube.

TILE is k_pairsum's tile (rsp_detect_describe): the shapes sit one below, on and one above it along
each axis.  A case: V, G, B, the window (rR, gR, rV, gV), T_CFAR, the seed, and `peaks`: (v, g, beam,
amplitude) 0-based, added to beams `beam` and `beam + 1` (the second at 0.6 of the amplitude, so that the
monopulse ratio is not 0).  'edges' in a case: peaks in the first and in the last cell under test of both
axes.  hits: 'some' / 'none' as tests/_parity.py reads it.
"""
import functools

import numpy as np

from oracle import chain
from rsp.plan import describe_detect

REF_WIN = (5, 10, 5, 10)
_D = describe_detect(64, 64, 2, dict(refCells_R=5, guardCells_R=10, refCells_V=5, guardCells_V=10, T_CFAR=8.0))
TILE_V, TILE_G = _D['rows'], _D['cols']
PRECS = ('c128', 'c64')


def _c(V, G, B, win, T, seed, peaks=(), edges=False, hits='some'):
    return dict(V=V, G=G, B=B, win=win, T=T, seed=seed, peaks=tuple(peaks), edges=edges, hits=hits)


W21 = (2, 1, 2, 1)
CASES = {
    # tile - 1, tile, tile + 1 along both axes (G = 63 / 65: rows that do not start on 16 bytes; V = 63 / 65:
    # columns of a complex-single cube that do not; 64: both aligned)
    'tile-1': _c(TILE_V - 1, TILE_G - 1, 3, W21, 1.7, 1, [(20, 30, 0, 40.0), (40, 10, 1, 25.0)], edges=True),
    'tile': _c(TILE_V, TILE_G, 3, W21, 1.7, 2, [(20, 30, 0, 40.0), (40, 10, 1, 25.0)], edges=True),
    'tile+1': _c(TILE_V + 1, TILE_G + 1, 3, W21, 1.7, 3, [(20, 30, 0, 40.0), (60, 55, 1, 25.0)], edges=True),
    # mixed: one axis across the tile edge, the other short
    'v+1-g-1': _c(TILE_V + 1, TILE_G - 1, 2, W21, 1.7, 4, [(50, 20, 0, 30.0)]),
    'v-1-g+1': _c(TILE_V - 1, TILE_G + 1, 2, W21, 1.7, 5, [(10, 60, 0, 30.0)]),
    # odd V over several row tiles with the reference's window; B = 2
    'v333-b2': _c(333, 40, 2, REF_WIN, 1.45, 6, [(100, 20, 0, 60.0), (300, 17, 0, 45.0)], edges=True),
    # B = 13
    'b13': _c(40, 48, 13, W21, 2.0, 7, [(12, 20, 3, 40.0), (30, 40, 11, 35.0)]),
    # the 3- and 4-point splines: G = 3 and 4 with the window 1/0/1/0
    'g3': _c(40, 3, 3, (1, 0, 1, 0), 2.5, 8, [(10, 1, 0, 30.0), (25, 1, 1, 30.0)]),
    'g4': _c(40, 4, 3, (1, 0, 1, 0), 2.5, 9, [(10, 1, 0, 30.0), (25, 2, 1, 30.0)]),
    # no cell under test: one Doppler row; a range axis shorter than the window
    'v1': _c(1, 50, 3, W21, 4.0, 10, [(0, 20, 0, 50.0)], hits='none'),
    'short-g': _c(48, 30, 3, REF_WIN, 4.0, 11, [(20, 15, 0, 50.0)], hits='none'),
}
CASE_IDS = list(CASES)

# more than 65 536 hits: the hit list grows and k_xcfar's LDS queue overflows in every workgroup
DENSE = _c(256, 300, 3, (1, 0, 1, 0), 0.55, 12)
DENSE_SAMPLE = 500

CLUSTER = dict(max_range_sep=30.0, max_vel_sep=0.7, max_angle_sep=4.0)


def cfar_dict(c):
    rR, gR, rV, gV = c['win']
    return dict(refCells_R=rR, guardCells_R=gR, refCells_V=rV, guardCells_V=gV, T_CFAR=c['T'], method='GOCA')


def cells_under_test(c):
    """0-based [r0, r1) x [v0, v1), empty when the window does not fit (fsf:192-193)."""
    rR, gR, rV, gV = c['win']
    r0, r1, v0, v1 = rR + gR, c['G'] - rR - gR, rV + gV, c['V'] - rV - gV
    return (r0, r1, v0, v1) if r1 > r0 and v1 > v0 else (0, 0, 0, 0)


def axes(V, G, B):
    """Caller-given axes of a [V, G, B] cube, in the oracle's precomputed_data form."""
    vmax = 40.0
    return dict(range_axis=100.0 + 7.5 * np.arange(G), velocity_axis=np.linspace(-vmax / 2, vmax / 2, V) if V > 1 else np.zeros(1),
                deltaR=7.5, deltaV=vmax / V, beam_angles_deg=np.linspace(-6.0, 30.0, B), k_slopes_LUT=5.0 + 0.3 * np.arange(B - 1))


def _peaks(c):
    pk = list(c['peaks'])
    if c['edges']:
        r0, r1, v0, v1 = cells_under_test(c)
        pk += [(v0, r0, 0, 45.0), (v1 - 1, r1 - 1, c['B'] - 2, 45.0)]
    return pk


@functools.lru_cache(maxsize=None)
def _cube(name, prec):
    c = DENSE if name == 'dense' else CASES[name]
    rng = np.random.default_rng(1000 + c['seed'])
    x = (rng.standard_normal((c['V'], c['G'], c['B'])) + 1j * rng.standard_normal((c['V'], c['G'], c['B']))) * np.sqrt(0.5)
    for v, g, b, a in _peaks(c):
        x[v, g, b] += a * np.exp(0.7j)
        x[v, g, b + 1] += 0.6 * a * np.exp(1.9j)
    if prec == 'c64':
        x = x.astype(np.complex64)
    x = np.asfortranarray(x)
    x.setflags(write=False)
    return x


def cube(name, prec):
    """The case's cube: complex128, or rounded to complex64 for a complex-single plan."""
    return _cube(name, prec)


@functools.lru_cache(maxsize=None)
def oracle(name, prec, monopulse='amplitude'):
    """The oracle's S8-S11 on the case's cube (as the plan of `prec` receives it), in tests/_parity.py's
    `st` / `fin` form; computed once and shared."""
    c = CASES[name]
    x = cube(name, prec).astype(np.complex128)
    pre = axes(c['V'], c['G'], c['B'])
    dets, S_all = chain.goca_cfar(x, cfar_dict(c))
    par = chain.parameter_estimation(dets, S_all, x, pre, monopulse)
    fin = chain.cluster_stage2(chain.cluster_stage1(par, CLUSTER), CLUSTER)
    return dict(rdm=x, dets=dets, S_all=S_all, par=par), fin


def parity_case(name, prec, gpu, monopulse='amplitude'):
    """The `case` dict tests/_parity.py's assertions take."""
    c = CASES[name]
    st, fin = oracle(name, prec, monopulse)
    return dict(prec=prec, s=dict(cfar=cfar_dict(c), pre_o=axes(c['V'], c['G'], c['B']), clus=CLUSTER), fin=fin, st=st, gpu=gpu,
                dets=c['hits'])
