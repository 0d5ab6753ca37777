"""Value cases of the three bit-defined map detectors (stage-3 range CFAR, Doppler CFAR, cross
GOCA-CFAR): amplitude maps far from 1, shared by the CPU preconditions (test_stage3_ref.py,
test_vcfar_ref.py, test_xcfar_ref.py) and the device comparison (test_cfar_value_range.py).

Every other map of the suite is Rayleigh(1.0); these probe the value domain include/rsp.h states.
``cases(prec)`` names the cases of a precision, ``value_map(case, prec, P, G)`` gives the seeded
double map [P x G x N_MAPS] a caller hands the plan, ``thresholds_T(case, det, prec)`` the T_CFAR
values the case runs with.

  case      map                                            what it probes
  tiny      Rayleigh x the smallest normal of the dtype    means and thresholds on either side of the
                                                           normal / subnormal boundary
  sub       Rayleigh x 2^-140 (c64) / 2^-1060 (c128)       every cell, sum and threshold subnormal
  x900      Rayleigh x 2^-900 (c128 only)                  the lowest scale at which the complex-double
                                                           cross CFAR is asserted; far inside its domain
  huge      Rayleigh x max / 8                             some window sums overflow to +Inf, others do
                                                           not; no cell is +Inf itself
  narrowed  (c64 only) a double map with cells below the   the restatement narrows first, as the upload
            float subnormals, inside them, above FLT_MAX   does: 0, subnormals and +Inf on the device
  wide      log-uniform, 30 decades (c128) / 12 (c64)      the summation order decides the bits
  const     every cell 0.1                                 r 0.1 / r rounds; ties everywhere: >= against
                                                           >, at T = 1 and its two neighbours
  zero      all zeros                                      stage 3 flags every un-notched cell (a hit
                                                           list far past the LDS queue), the others none
  T-edge    Rayleigh(1), T = 1e-30 and T = 1e30; for a      T is no float: it is rounded first.  At 1e+-30
            complex-single plan also 1e-40 and 2e38        nothing under- or overflows in either precision;
                                                           1e-40 is a subnormal float and makes every float
                                                           threshold subnormal, 2e38 overflows some float
                                                           thresholds to +Inf and not others

Left out, and asserted to be exactly this list (LEFT_OUT): the complex-double cross CFAR on ``sub`` and
``tiny``.  Its quotient is k3_quot's FMA form, which is RN(x / n) only where the quotient is a normal
number (x >= n 2^-1022; test_xcfar_ref.py::test_fma_quotient_domain shows both sides in exact rational
arithmetic): below, an exact tie between two subnormals (n even and no power of two) rounds the other
way.  The hot path is not slowed for amplitudes below 1e-292; include/rsp.h states the domain instead.
The windows of these tests have odd divisors (3, 7, 5), where the rational emulation finds no
difference at any scale, so the device comparison prints the mismatch count of the two left-out cases
without asserting it.
"""
import functools
from fractions import Fraction

import numpy as np

SEED = 20250101
N_MAPS = 2
DTYPE = {'c128': np.float64, 'c64': np.float32}
DETECTORS = ('stage3', 'vcfar', 'xcfar')

# the shapes: the smallest that cross a tile of the kernel along both axes
S3_P, S3_SEGS, S3_WIN = 33, (38, 60, 94 + 256), (5, 14)     # two range chunks of 256; window r / s
VC_SHAPE, VC_WIN = (40, 70), (4, 6)                        # refCells_V / guardCells_V
XC_SHAPE, XC_WINDOWS = (40, 70), ((3, 1, 7, 0), (5, 5, 5, 5))   # two different divisors; equal ones
VC_METHODS = ('ca', 'goca', 'soca')

_COMMON = ('tiny', 'sub', 'huge', 'wide', 'const', 'zero', 'T-edge')
CASES = {'c128': _COMMON + ('x900',), 'c64': _COMMON + ('narrowed',)}
LEFT_OUT = frozenset({('xcfar', 'c128', 'sub'), ('xcfar', 'c128', 'tiny')})
SUB_EXP = {'c128': -1060, 'c64': -140}
X900_EXP = -900
WIDE_DECADES = {'c128': 30, 'c64': 12}
# tiny: T puts the thresholds on both sides of the smallest normal (the greatest-of means are larger)
TINY_T = {'stage3': 0.7, 'vcfar': 0.8, 'xcfar': 0.6}
T_EDGE = (1e-30, 1e30)
T_EDGE_C64 = (1e-40, 2e38)      # threshold underflow and overflow in float


def cases(prec):
    return CASES[prec]


def compared(det, prec):
    """The cases of a detector and precision that are compared to the bit."""
    return tuple(c for c in CASES[prec] if (det, prec, c) not in LEFT_OUT)


def thresholds_T(case, det, prec):
    """T_CFAR values (doubles, as a caller gives them) of a case."""
    one = DTYPE[prec](1)
    if case == 'const':     # 1 and its neighbours in the plan's precision
        return (1.0, float(np.nextafter(one, DTYPE[prec](2))), float(np.nextafter(one, DTYPE[prec](0))))
    if case == 'T-edge':
        return T_EDGE + (T_EDGE_C64 if prec == 'c64' else ())
    if case == 'tiny':
        return (TINY_T[det],)
    if case == 'huge':
        return (1.0,)
    return (1.5,)


@functools.lru_cache(maxsize=None)
def _map(case, prec, P, G):
    rng = np.random.default_rng(SEED + sum(map(ord, case)))
    shape = (P, G, N_MAPS)
    fi = np.finfo(DTYPE[prec])
    if case == 'zero':
        a = np.zeros(shape)
    elif case == 'const':
        a = np.full(shape, 0.1)
    elif case == 'wide':
        d = WIDE_DECADES[prec] / 2
        a = 10.0 ** rng.uniform(-d, d, shape)
    elif case == 'narrowed':
        assert prec == 'c64'
        a = rng.rayleigh(1.0, shape) * 2.0 ** -135          # inside the float subnormals
        kind = rng.uniform(size=shape)
        a[kind < 0.10] *= 1e-8                                # below the smallest float subnormal: 0 on the device
        big = kind > 0.99
        a[big] = 1e39 * (1.0 + rng.uniform(size=int(big.sum())))   # above FLT_MAX: +Inf on the device
    else:
        scale = {'tiny': float(fi.tiny), 'sub': 2.0 ** SUB_EXP[prec], 'x900': 2.0 ** X900_EXP,
                 'huge': float(fi.max) / 8, 'T-edge': 1.0}[case]
        a = rng.rayleigh(1.0, shape) * scale
    a = np.asfortranarray(a)
    a.setflags(write=False)
    return a


def value_map(case, prec, P, G):
    """The case's map [P x G x N_MAPS] in double, as the caller holds it (read-only, shared)."""
    assert case in CASES[prec], (case, prec)
    return _map(case, prec, P, G)


def narrow(a, prec):
    """``a`` as the device holds it: rounded to the plan's precision, widened back to double."""
    with np.errstate(over='ignore', under='ignore'):
        return np.asarray(a).astype(DTYPE[prec]).astype(np.float64)


def is_subnormal(x, prec):
    x = np.abs(np.asarray(x, np.float64))
    return (x > 0) & (x < float(np.finfo(DTYPE[prec]).tiny))


def is_normal(x, prec):
    x = np.abs(np.asarray(x, np.float64))
    return np.isfinite(x) & (x >= float(np.finfo(DTYPE[prec]).tiny))


def check_preconditions(det, variant, case, prec):
    """The property a case is named for, on the restatement alone (``restatement`` and ``tested_cells``
    below).  Prints and returns the counts per T."""
    run, m, ge_is_native = restatement(det, variant, prec), tested_cells(det, variant), not NATIVE_STRICT[det]
    amp = value_map(case, prec, *shape_of(det))
    dev = narrow(amp, prec)
    out = {}
    for T in thresholds_T(case, det, prec):
        with np.errstate(all='ignore'):
            f, t = run(amp, T, True, False)
            fl, _ = run(amp, T, False, False)
        tt = t[m]
        assert not np.isnan(t).any()
        c = dict(cells=int(m.sum()), sub_thr=int(is_subnormal(tt, prec).sum()), normal_thr=int(is_normal(tt, prec).sum()),
                 inf_thr=int(np.isposinf(tt).sum()), zero_thr=int((tt == 0).sum()), strict_hits=int(f[m].sum()),
                 loose_hits=int(fl[m].sum()))
        if case == 'wide':
            with np.errstate(all='ignore'):
                _, tr = run(amp, T, True, True)
            c['order_changes'] = int((tr[m] != tt).sum())
        out[T] = c
        print(det, variant, prec, case, 'T=%r' % T, c)
    first = out[thresholds_T(case, det, prec)[0]]
    if case == 'tiny':
        assert first['sub_thr'] >= 100 and first['normal_thr'] >= 100, first
    elif case == 'sub':
        assert is_subnormal(dev, prec).all(), 'a cell that is not subnormal'
        assert first['sub_thr'] == first['cells'] and first['normal_thr'] == 0 and first['inf_thr'] == 0, first
    elif case == 'x900':
        assert first['normal_thr'] == first['cells'] and float(np.min(t[m])) >= 2.0 ** (X900_EXP - 4), first
    elif case == 'huge':
        assert np.isfinite(dev).all(), 'a cell that is +Inf itself'
        assert first['inf_thr'] >= 10 and first['normal_thr'] >= 10, first     # both present
        if ge_is_native:   # >= flags a cell under an infinite threshold only if it is +Inf itself
            assert not (fl[m] & np.isposinf(t[m])).any()
    elif case == 'narrowed':
        assert np.isfinite(amp).all() and (amp > 0).all()
        n0, ns, ni = int((dev == 0).sum()), int(is_subnormal(dev, prec).sum()), int(np.isposinf(dev).sum())
        print(det, prec, case, 'device cells: zero %d subnormal %d +Inf %d of %d' % (n0, ns, ni, dev.size))
        assert n0 >= 50 and ns >= 1000 and ni >= 20
        assert first['inf_thr'] >= 20 and first['sub_thr'] >= 100, first
    elif case == 'wide':
        assert first['order_changes'] >= 0.10 * first['cells'], first
    elif case == 'const':
        assert any(c['strict_hits'] != c['loose_hits'] for c in out.values()), out
    elif case == 'zero':
        assert first['zero_thr'] == first['cells']
        assert first['strict_hits'] == 0 and first['loose_hits'] == first['cells']
    elif case == 'T-edge':
        for T, c in out.items():
            assert float(DTYPE['c64'](T)) != T, 'T = %r is a float' % T
        for T in T_EDGE:
            assert out[T]['normal_thr'] == out[T]['cells'], out[T]
        assert out[T_EDGE[0]]['strict_hits'] == first['cells'] and out[T_EDGE[1]]['strict_hits'] == 0
        if prec == 'c64':
            lo, hi = out[T_EDGE_C64[0]], out[T_EDGE_C64[1]]
            assert is_subnormal(DTYPE[prec](T_EDGE_C64[0]), prec) and np.isfinite(DTYPE[prec](T_EDGE_C64[1]))
            assert lo['sub_thr'] == lo['cells'], lo                          # underflow: every threshold subnormal
            assert hi['inf_thr'] >= 10 and hi['normal_thr'] >= 10, hi        # overflow: some +Inf, some not
    return out


# ---- the restatements, by detector and variant -----------------------------------------------------
VARIANTS = {'stage3': ('go', 'so'), 'vcfar': VC_METHODS, 'xcfar': XC_WINDOWS}
NATIVE_STRICT = {'stage3': False, 'vcfar': True, 'xcfar': True}    # stage 3 tests >=, the other two >


def shape_of(det):
    return (S3_P, sum(S3_SEGS)) if det == 'stage3' else (VC_SHAPE if det == 'vcfar' else XC_SHAPE)


def params(det, variant, T):
    """The parameter dict of a detector's variant, as the Plan call takes it."""
    if det == 'stage3':
        return dict(refCells_R=S3_WIN[0], saveCells_R=S3_WIN[1], T_CFAR=T, CFARmethod_R=VARIANTS[det].index(variant),
                    MTD_0v_num=1)
    if det == 'vcfar':
        return dict(refCells_V=VC_WIN[0], guardCells_V=VC_WIN[1], T_CFAR=T)
    return dict(refCells_R=variant[0], guardCells_R=variant[1], refCells_V=variant[2], guardCells_V=variant[3], T_CFAR=T)


def tested_cells(det, variant):
    """Boolean mask [P x G x N_MAPS] of the cells the detector tests."""
    import _stage3_ref
    import _xcfar_ref
    P, G = shape_of(det)
    m = np.ones((P, G, N_MAPS), bool)
    if det == 'stage3':
        z0, z1 = _stage3_ref.notch_rows(P, 1)
        m[z0 - 1:z1] = False
    elif det == 'xcfar':
        r0, r1, v0, v1 = _xcfar_ref.cells_under_test(P, G, params(det, variant, 1.0))
        m[:] = False
        m[v0:v1, r0:r1] = True
    return m


def restatement(det, variant, prec):
    """run(amp, T, strict, reverse) -> (flags uint8, thresholds float64) of the numpy restatement in the
    precision's dtype.  strict: ``>`` (False: ``>=``); reverse: every window summed in the opposite
    order, by running on the flipped map and flipping back (the windows are mirror-symmetric)."""
    import _stage3_ref
    import _vcfar_ref
    import _xcfar_ref
    dt = DTYPE[prec]

    def run(amp, T, strict=NATIVE_STRICT[det], reverse=False):
        prm = params(det, variant, T)
        a = np.asarray(amp)
        if det == 'stage3':
            a = a[:, ::-1] if reverse else a
            segs = S3_SEGS[::-1] if reverse else S3_SEGS
            f, t = _stage3_ref.local_execute_cfar(a, prm, segs, dt, strict=strict)
            return (f[:, ::-1], t[:, ::-1]) if reverse else (f, t)
        if det == 'vcfar':
            a = a[::-1] if reverse else a
            f, t = _vcfar_ref.local_cfar_detector(a, prm, VC_METHODS.index(variant), dt, strict=strict)
            return (f[::-1], t[::-1]) if reverse else (f, t)
        a = a[::-1, ::-1] if reverse else a
        f, t = _xcfar_ref.goca_cfar_maps(a, prm, dt, strict=strict)
        return (f[::-1, ::-1], t[::-1, ::-1]) if reverse else (f, t)
    return run


@functools.lru_cache(maxsize=None)
def expected(det, variant, prec, case, T):
    """(flags, thresholds) of the restatement with the detector's own comparison; computed once."""
    with np.errstate(all='ignore'):
        f, t = restatement(det, variant, prec)(value_map(case, prec, *shape_of(det)), T)
    f.setflags(write=False)
    t.setflags(write=False)
    return f, t


# ---- k3_quot's FMA form in exact rational arithmetic ---------------------------------------------
def fma_quotient(x, n):
    """The complex-double quotient of rsp_k3_arith.h on a double x >= 0 and a count n, every step
    rounded once from its exact rational value: q0 = RN(x RN(1/n)); r = RN(x - q0 n);
    q = RN(q0 + r RN(1/n)).  Returns (q, whether r was exact)."""
    inv = 1.0 / n
    q0 = float(Fraction(x) * Fraction(inv))
    r_exact = Fraction(x) - Fraction(q0) * n
    r = float(r_exact)
    return float(Fraction(q0) + Fraction(r) * Fraction(inv)), Fraction(r) == r_exact


def true_quotient(x, n):
    """RN(x / n)."""
    return float(Fraction(x) / n)
