"""Cases and the reference of the per-element magnitude tests (test_cmag.py on the device,
test_cmag_cases.py on the CPU).

Reference: hypot in np.longdouble (64-bit significand) of the values the device holds -- complex-single
inputs widened exactly first; where long double is no wider than double, the exact rationals with
math.isqrt instead.

Bound (derived, not measured), u = 2^-53 (complex double) or 2^-24 (complex single):
q = fl(fl(x^2) + fl(y^2)) carries at most 2u + u^2 relative error, the square root halves that, the root
step adds at most 1 ulp <= 2u (the documented accuracy of v_sqrt_f32; for the double refinement of
v_rsq_f64 a supposition these tests check):
    |got - exact| <= 3u (1 + 2^-10) exact                       a magnitude
    |got - (|a| + |b|)| <= 4u (1 + 2^-10) (|a| + |b|)           a pair sum RN(|a| + |b|)
valid while q is a normal, finite number (include/rsp.h, "Value domain").  The 2^-10 covers the
reference's own error (2^-64 relative, 2^-11 u of a double).

Direct cases: a cube [V x G x 2] whose second beam is all zeros, so that Plan.detect's pair-sum map is
cmag(x) + 0 = cmag(x) exactly.  Per scale s = 2^e every magnitude lies in [s / 2, 2 s] (a factor 4), so
with T_CFAR = 1e3 no cell can pass the cross CFAR and the case measures the magnitude alone.  Three
kinds of cell, mixed over the map by index: random phases; cells on the axes (+-m, 0), (0, +-m); cells
with |x| >> |y| (or |y| >> |x|) by 2^30 (double) / 2^13 (float), where the small square is lost.
"""
import functools
import math
from fractions import Fraction

import numpy as np

from oracle import chain
from _scen import SEED, K2_CASES, plumbing_config, plumbing_weights, _route_cfar, scenario, k2_targets
from rsp import config as C
from rsp.plan import describe_k2
from rsp.precompute import precompute as product_precompute
from oracle import precompute as oracle_precompute

U = {'c128': 2.0 ** -53, 'c64': 2.0 ** -24}
SLACK = 1.0 + 2.0 ** -10
MAG_BOUND_U, PAIR_BOUND_U = 3.0, 4.0            # in u, before the slack
CDTYPE = {'c128': np.complex128, 'c64': np.complex64}
EXPONENTS = {'c128': (-500, -300, -60, 0, 60, 300, 500), 'c64': (-60, -30, 0, 30, 60)}
SKEW = {'c128': 30, 'c64': 13}
SHAPES = {'tile+': (33, 130), 'tile-1': (63, 63)}    # k_pairsum's tile is 64 x 64 (test_cmag_cases.py asserts it)
WINDOW = dict(refCells_R=2, guardCells_R=1, refCells_V=2, guardCells_V=1, T_CFAR=1e3, method='GOCA')
DYNAMIC_RANGE = 1e3                                # max / median of |rdm| the device-value cubes must reach
WIDE = np.finfo(np.longdouble).nmant > 52


# ---- the reference ---------------------------------------------------------------------------------
def _isqrt_hypot_err(got, x, y, extra=80):
    """|got - hypot(x, y)| / hypot(x, y) per element with exact rationals (the fallback)."""
    out = np.zeros(got.shape)
    for i in np.ndindex(got.shape):
        fx, fy, fg = Fraction(float(x[i])), Fraction(float(y[i])), Fraction(float(got[i]))
        q = fx * fx + fy * fy
        if q == 0:
            out[i] = 0.0 if fg == 0 else np.inf
            continue
        d = q.denominator
        k = extra + max(0, d.bit_length())            # sqrt(q) = isqrt(q d 4^k) / (d 2^k), to 2^-k relative and better
        root = Fraction(math.isqrt(q.numerator * d << (2 * k)), d << k)
        out[i] = float(abs(fg - root) / root)
    return out


def mag_error(got, z):
    """|got - |z|| / |z| per element (0 where both are 0, inf where only |z| is), z as the device holds it."""
    got = np.asarray(got, np.float64)
    x, y = np.asarray(z.real, np.float64), np.asarray(z.imag, np.float64)     # widening a float is exact
    if not WIDE:
        return _isqrt_hypot_err(got, x, y)
    exact = np.hypot(x.astype(np.longdouble), y.astype(np.longdouble))
    err = np.abs(got.astype(np.longdouble) - exact)
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = np.where(exact > 0, err / exact, np.where(err > 0, np.inf, 0.0))
    return rel.astype(np.float64)


def pair_error(got, a, b):
    """|got - (|a| + |b|)| / (|a| + |b|) per element."""
    got = np.asarray(got, np.float64)
    if not WIDE:
        out = np.zeros(got.shape)
        for i in np.ndindex(got.shape):
            # rational |a| + |b| to 2^-80: through the two roots
            s = Fraction(0)
            for z in (a[i], b[i]):
                q = Fraction(float(z.real)) ** 2 + Fraction(float(z.imag)) ** 2
                if q:
                    d = q.denominator
                    k = 80 + d.bit_length()
                    s += Fraction(math.isqrt(q.numerator * d << (2 * k)), d << k)
            out[i] = float(abs(Fraction(float(got[i])) - s) / s) if s else (0.0 if got[i] == 0 else np.inf)
        return out
    ld = np.longdouble
    exact = (np.hypot(np.asarray(a.real, np.float64).astype(ld), np.asarray(a.imag, np.float64).astype(ld)) +
             np.hypot(np.asarray(b.real, np.float64).astype(ld), np.asarray(b.imag, np.float64).astype(ld)))
    err = np.abs(got.astype(ld) - exact)
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = np.where(exact > 0, err / exact, np.where(err > 0, np.inf, 0.0))
    return rel.astype(np.float64)


def report(label, rel, prec, bound_u):
    """Print the worst error in u and where it is; return it (the caller asserts)."""
    worst = float(rel.max()) / U[prec] if rel.size else 0.0
    at = np.unravel_index(int(np.argmax(rel)), rel.shape) if rel.size else ()
    print('%s: worst %.4f u at %r (bound %g u), mean %.4f u' % (label, worst, tuple(int(i) for i in at), bound_u,
                                                                float(rel.mean()) / U[prec] if rel.size else 0.0))
    return worst


# ---- direct cases -----------------------------------------------------------------------------------
KINDS = ('phase', 'axis', 'skew')


def cell_kinds(V, G):
    """Kind index of every cell: the three kinds interleaved along both axes, so that every tile row and
    column holds all of them."""
    v, g = np.meshgrid(np.arange(V), np.arange(G), indexing='ij')
    return (v + g) % 3


@functools.lru_cache(maxsize=None)
def direct_cube(prec, e, shape):
    """The cube [V x G x 2] of scale 2^e as the plan of ``prec`` receives it (read-only)."""
    V, G = SHAPES[shape]
    rng = np.random.default_rng(SEED + 7 * e + V)
    m = 2.0 ** rng.uniform(-0.9, 0.9, (V, G))                     # magnitudes in (s / 2, 2 s), rounding included
    ph = rng.uniform(0, 2 * np.pi, (V, G))
    sx, sy = rng.choice([-1.0, 1.0], (V, G)), rng.choice([-1.0, 1.0], (V, G))
    swap = rng.integers(0, 2, (V, G)).astype(bool)
    kind = cell_kinds(V, G)
    x, y = m * np.cos(ph), m * np.sin(ph)
    ax, ay = np.where(swap, 0.0, sx * m), np.where(swap, sy * m, 0.0)
    big, small = sx * m, sy * m * 2.0 ** -SKEW[prec]
    kx, ky = np.where(swap, small, big), np.where(swap, big, small)
    re = np.where(kind == 0, x, np.where(kind == 1, ax, kx))
    im = np.where(kind == 0, y, np.where(kind == 1, ay, ky))
    cube = np.zeros((V, G, 2), np.complex128, order='F')
    cube[:, :, 0] = np.ldexp(re, e) + 1j * np.ldexp(im, e)       # the scaling is exact
    cube = np.asfortranarray(cube.astype(CDTYPE[prec]))
    cube.setflags(write=False)
    return cube


def zero_cube(prec, shape):
    """All zeros, of every sign combination."""
    V, G = SHAPES[shape]
    kind = cell_kinds(V, G)
    re = np.where(kind == 1, -0.0, 0.0)
    im = np.where((kind + np.arange(G)[None, :]) % 2 == 0, -0.0, 0.0)
    cube = np.zeros((V, G, 2), np.complex128, order='F')
    cube.real[:, :, 0], cube.imag[:, :, 0] = re, im
    cube.real[:, :, 1] = -0.0
    return np.asfortranarray(cube.astype(CDTYPE[prec]))


def direct_cases():
    return [(p, e, s) for p in ('c128', 'c64') for s in SHAPES for e in EXPONENTS[p]]


# ---- cubes for the sites that take the device's own complex values -------------------------------------
STRONG_SNR_DB = 20.0
FRAME_CASES = ('plumbing', 'w4-mb128')


def plumbing3():
    """The `plumbing` waveform at 16 pulses x 3 beams x 16 channels as a scenario dict (narrow FIR plus
    both overlap-save segments)."""
    cfg = plumbing_config(16, 3, 16)
    W, ang, k = plumbing_weights(cfg)
    return dict(name='plumbing', cfg=cfg, cfar=_route_cfar(16, 'small'), clus=C.default_cluster_params(), W=W,
                pre_o=oracle_precompute.precompute(cfg, W, ang, k, C.V8_FIR), pre_p=product_precompute(cfg, W, ang, k, C.V8_FIR))


@functools.lru_cache(maxsize=None)
def frame_scenario(name):
    return plumbing3() if name == 'plumbing' else scenario(name)


def _strong_targets(s, layout=None):
    """Targets of a case with a strong one (STRONG_SNR_DB) among them: the map's dynamic range is large."""
    pre, sc = s['pre_o'], s['cfg']['Sig_Config']
    if layout is not None:
        tg = [dict(t) for t in k2_targets(s, layout)]
    else:
        G = sum(sc['point_prt_segments'])
        vmax = sc['wavelength'] / (2 * sc['prt'])
        ang = pre['beam_angles_deg']
        tg = [dict(Range=float(pre['range_axis'][g]), Velocity=v * vmax, ElevationAngle=float(ang[i % len(ang)]) + 0.5, SNR_dB=5.0)
              for i, (g, v) in enumerate(((30, 0.11), (150, -0.2), (G - 100, 0.3)))]
    tg[2]['SNR_dB'] = STRONG_SNR_DB       # in the long segment: the largest compression gain
    return tg


@functools.lru_cache(maxsize=None)
def frame_cube(name, prec):
    """Targets plus Philox noise [P x N x C] as the plan of ``prec`` receives it (a K2 case's targets sit
    where its layout of that precision puts them: _scen.k2_targets)."""
    s = frame_scenario(name)
    layout = describe_k2(s['cfg'], s['cfar'], s['clus'], s['pre_p'], precision=prec) if name in K2_CASES else None
    raw = chain.synthesize_echo(_strong_targets(s, layout), s['cfg'], s['pre_o']) + chain.philox_noise(s['cfg'], 1, SEED)
    raw = raw.astype(CDTYPE[prec])
    raw.setflags(write=False)
    return raw


def oracle_rdm(name, cube):
    s = frame_scenario(name)
    pre = s['pre_o']
    return chain.mtd(chain.pulse_compress(chain.dbf(cube.astype(np.complex128), pre['DBF_coeffs_data_C']), pre), pre)
