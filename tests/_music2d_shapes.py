"""Shapes, scenes, grids and reference quantities of tests/test_music2d_shapes.py and
tests/test_music2d_shape_cases.py -- TEST INFRASTRUCTURE ONLY.

Everything here is host arithmetic on ``tests/_music2d_ref.py`` (complex128, ``np.linalg.eigh``):
the case tables, the scene every case shares, the scan grids, the repeat maps of the plateau cases,
the two preconditions of an exact peak comparison (neighbour margin, height gap) and a numpy
restatement of k_music_peaks2d's drop-pass scheme that also counts the passes.  No device code is
touched.
"""
import functools

import numpy as np

import _music2d_ref as ref
from _music_shapes import EXACT_MARGIN_DB

SEED = 20250101
SNR_DB = 10.0
# (phi, theta) in degrees; a case with M sources has the first M (the first five are test_music2d.py's)
SRC = [(30.0, 20.0), (-60.0, 45.0), (0.0, 60.0), (-20.0, 10.0), (60.0, 70.0), (45.0, 35.0), (-40.0, 65.0),
       (10.0, 40.0)]


def scene_for(M):
    """Complex unit-amplitude sources at SRC[:M], awgn 10 dB 'measured'."""
    return {'azim_rad': np.deg2rad([s[0] for s in SRC[:M]]), 'elev_rad': np.deg2rad([s[1] for s in SRC[:M]]),
            'amplitudes': np.ones(M), 'complex_sources': 1, 'snr_db': SNR_DB, 'snr_measured': 1}


def grid(nt, npn):
    """G(nt, np): (phi [np], theta [nt]) in radians.  Asymmetric in phi on purpose: a line array's
    map is mirror-symmetric in phi, and on a symmetric grid the mirror pixels are bit-equal on the
    device and only ulp-equal in BLAS, which would leave the top-M order undefined."""
    return np.deg2rad(np.linspace(-77.0, 80.0, npn)), np.deg2rad(np.linspace(2.0, 80.0, nt))


def _case(kind, nx, ny, K, M, n, nt=17, npn=33, dxl=0.5, dyl=0.5, max_batch=None, rt=None, rp=None):
    """nt, npn: the unique grid G(nt, npn) the reference scans.  rt, rp: per unique theta / phi
    index the number of times the plan's grid lists it (None: once each)."""
    rt = np.ones(nt, np.int64) if rt is None else np.asarray(rt, np.int64)
    rp = np.ones(npn, np.int64) if rp is None else np.asarray(rp, np.int64)
    assert len(rt) == nt and len(rp) == npn
    return dict(kind=kind, nx=nx, ny=ny, K=K, M=M, n=n, nt=nt, npn=npn, dxl=dxl, dyl=dyl,
                max_batch=n if max_batch is None else max_batch, rt=rt, rp=rp)


# ---- the array cases: G(17, 33), 2 instances
#  id          nx  ny    K  M   what it reaches
#  a2x1         2   1   16  1   N = 2, ny = 1 (the inner steering loop of length 1)
#  a1x7         1   7   20  2   nx = 1 (the outer loop of length 1), prime N
#  a64x1       64   1  128  3   N = 64 along x
#  a2x32        2  32   96  4   N = 64, the last fast-path M
#  a32x2       32   2   96  5   N = 64, no fast path
#  a7x9         7   9  130  8   N = 63, M = MU_MMAX, K past one synthesis chunk
#  a3x3-m8      3   3   40  8   M = N - 1
#  a5x5-k7      5   5    7  2   K < N: rank-deficient R
#  a4x4-k1      4   4    1  1   K = 1
#  a6x5         6   5   33  6   N = 30, K % 4 = 1
#  dxdy         3   5   48  2   dx/lambda = 0.4, dy/lambda = 0.6; 4 instances
ARRAY_CASES = {
    'a2x1': _case('array', 2, 1, 16, 1, 2),
    'a1x7': _case('array', 1, 7, 20, 2, 2),
    'a64x1': _case('array', 64, 1, 128, 3, 2),
    'a2x32': _case('array', 2, 32, 96, 4, 2),
    'a32x2': _case('array', 32, 2, 96, 5, 2),
    'a7x9': _case('array', 7, 9, 130, 8, 2),
    'a3x3-m8': _case('array', 3, 3, 40, 8, 2),
    'a5x5-k7': _case('array', 5, 5, 7, 2, 2),
    'a4x4-k1': _case('array', 4, 4, 1, 1, 2),
    'a6x5': _case('array', 6, 5, 33, 6, 2),
    'dxdy': _case('array', 3, 5, 48, 2, 4, dxl=0.4, dyl=0.6),
}

# ---- the batch cases: 4 x 4, K = 64, M = 2, G(17, 33); k_music_scan2d packs 4 instances per workgroup
BATCH_FULL = 'b6'          # every instance of every batch case is bit-equal to the same instance of this run
BATCH_CASES = {
    'b1': _case('batch', 4, 4, 64, 2, 1),
    'b3': _case('batch', 4, 4, 64, 2, 3),
    'b5': _case('batch', 4, 4, 64, 2, 5),
    'b6': _case('batch', 4, 4, 64, 2, 6),
    'b5-mb8': _case('batch', 4, 4, 64, 2, 5, max_batch=8),
}

# ---- the grid cases: 4 x 4, K = 64, M = 2, one instance unless stated
#  (3, 3)        S = 9: one partly filled workgroup, the smallest axes
#  (3, 1024)     the longest phi axis, columns of 3
#  (1024, 3)     the longest theta axis
#  (16, 16)      S = 256: one full workgroup, one ballot round
#  (15, 17)      S = 255
#  (7, 37)       S = 259: three pixels into a second round
#  (31, 9), (32, 9), (33, 9)   a column one short of, equal to, one past a 32-pixel mask word
#  (256, 256), (64, 1024), (1024, 64)   S = 65 536 = M2_SMAX: the last ballot writes words 2046, 2047;
#                the last with 3 instances, so the 512 KB maps of three workgroups are in flight at once
GRID_SHAPES = [(3, 3, 1), (3, 1024, 1), (1024, 3, 1), (16, 16, 1), (15, 17, 1), (7, 37, 1), (31, 9, 1), (32, 9, 1),
               (33, 9, 1), (256, 256, 1), (64, 1024, 1), (1024, 64, 3)]
GRID_CASES = {'g%dx%d' % (nt, npn): _case('grid', 4, 4, 64, 2, n, nt, npn) for nt, npn, n in GRID_SHAPES}

# ---- the plateau cases: 4 x 4, K = 64, 2 instances; the plan's grid lists unique theta index i
# rt[i] times and unique phi index j rp[j] times
PLATEAU_CASES = {
    # 119 x 108; plateaus of up to 70 x 65 pixels: several mask words, owner lanes and ballot rounds
    'p-runs': _case('plateau', 4, 4, 64, 2, 2, 9, 11, rt=[1, 40, 1, 1, 3, 1, 1, 70, 1],
                    rp=[1, 1, 33, 1, 1, 1, 2, 1, 1, 65, 1]),
    # 78 x 78; plateaus of every size from 1 x 12 to 12 x 1
    'p-stair': _case('plateau', 4, 4, 64, 3, 2, 12, 12, rt=np.arange(1, 13), rp=np.arange(12, 0, -1)),
    'p-rows': _case('plateau', 4, 4, 64, 2, 2, 17, 1, rp=[40]),       # every row one plateau
    'p-cols': _case('plateau', 4, 4, 64, 2, 2, 1, 9, rt=[300]),       # every column one plateau
    'p-const3': _case('plateau', 4, 4, 64, 2, 2, 1, 1, rt=[3], rp=[3]),      # the whole 3 x 3 map one plateau
    'p-const': _case('plateau', 4, 4, 64, 2, 2, 1, 1, rt=[20], rp=[23]),     # the same at S = 460
}
MIN_PASSES = {'p-runs': 60, 'p-stair': 10}   # drop passes the restated scheme must need at least

# ---- fewer regional maxima than M: G(3, 3), 4 instances
FEW_CASES = {
    'few': _case('few', 5, 5, 128, 5, 4, 3, 3),
    'few-m8': _case('few', 7, 9, 130, 8, 4, 3, 3),
}

CASES = {}
for _t in (ARRAY_CASES, BATCH_CASES, GRID_CASES, PLATEAU_CASES, FEW_CASES):
    CASES.update(_t)
CASE_IDS = list(CASES)


# ---- grids and repeat maps
def unique_grid(c):
    """(phi, theta) the reference scans."""
    return grid(c['nt'], c['npn'])


def repeat_maps(c):
    """(theta_map, phi_map): per row / column of the plan's grid its unique-grid index."""
    return np.repeat(np.arange(c['nt']), c['rt']), np.repeat(np.arange(c['npn']), c['rp'])


def plan_grid(c):
    """(phi, theta) of the plan: the unique grid with every index repeated rt / rp times."""
    phi, theta = unique_grid(c)
    tm, pm = repeat_maps(c)
    return phi[pm], theta[tm]


def expand(c, m):
    """A unique-grid map on the plan's grid."""
    tm, pm = repeat_maps(c)
    return m[tm][:, pm]


# ---- preconditions of an exact peak comparison, on a reference map alone
def neighbour_margin(m):
    """Smallest |pixel - its largest in-bounds 8-neighbour| (inf for a 1 x 1 map)."""
    return float(np.abs(m - ref.largest_neighbour(m)).min())


def height_gap(m, mask, M):
    """Smallest gap between consecutive heights among the min(M, n_peaks) + 1 highest regional maxima
    (inf with fewer than two): below it a perturbation changes neither which maxima are the top M
    nor their order."""
    h = np.sort(m[mask])[::-1][:min(M, int(mask.sum())) + 1]
    return float(np.min(-np.diff(h))) if len(h) > 1 else np.inf


def check_preconditions(m, mask, M, where, margin_db=EXACT_MARGIN_DB):
    """Print and assert both on a unique-grid reference map; returns (margin, gap)."""
    mg, gap = neighbour_margin(m), height_gap(m, mask, M)
    print('%s: neighbour margin %.3e dB, height gap %.3e dB, n_peaks %d' % (where, mg, gap, int(mask.sum())))
    assert mg > 0.0, '%s: a pixel equals its largest neighbour' % where
    assert mg >= margin_db, '%s: neighbour margin %.3e dB' % (where, mg)
    assert gap >= margin_db, '%s: height gap %.3e dB' % (where, gap)
    return mg, gap


# ---- k_music_peaks2d's drop passes, restated
def _neighbours(a, fill):
    """The 8 in-bounds-or-`fill` neighbour planes of a."""
    nr, nc = a.shape
    pad = np.full((nr + 2, nc + 2), fill, a.dtype)
    pad[1:-1, 1:-1] = a
    return [pad[dr:dr + nr, dc:dc + nc] for dr in (0, 1, 2) for dc in (0, 1, 2) if dr != 1 or dc != 1]


def drop_passes(img):
    """(mask, passes): the device's scheme.  Candidates are the pixels with no larger in-bounds
    neighbour; a pass drops every candidate that touches an equal-valued non-candidate (all reads
    from the mask the previous pass left: two masks, read one, write the other), until a pass drops
    nothing.  The count includes that final pass, so a map without ties takes one."""
    img = np.asarray(img, np.float64)
    cand = img >= ref.largest_neighbour(img)
    eq = [u == img for u in _neighbours(img, np.nan)]          # NaN: out of bounds never equals
    passes = 0
    while True:
        passes += 1
        drop = np.zeros(img.shape, bool)
        for e, cn in zip(eq, _neighbours(cand, True)):
            drop |= e & ~cn
        drop &= cand
        if not drop.any():
            return cand, passes
        cand = cand & ~drop


# ---- the reference on host-synthesised snapshots (the CPU preconditions)
@functools.lru_cache(maxsize=None)
def _snapshots(nx, ny, K, M, dxl, dyl, inst):
    X = ref.synthesize_2d(scene_for(M), nx, ny, K, dxl, dyl, inst, SEED)
    X.setflags(write=False)
    return X


def snapshots(c, inst):
    return _snapshots(c['nx'], c['ny'], c['K'], c['M'], c['dxl'], c['dyl'], inst)


def expected(c, r):
    """From music_2d's result r on the unique grid, what the plan's grid must give: (map, mask,
    peaks [M] 1-based and zero-padded, n_peaks)."""
    if (c['rt'] == 1).all() and (c['rp'] == 1).all():
        m, mask = r['spectrum_db'], r['mask']
    else:
        m = expand(c, r['spectrum_db'])
        mask = ref.regional_max(m)
    top = ref.top_peaks(m, mask, c['M'])
    peaks = np.zeros(c['M'], np.int64)
    peaks[:len(top)] = top + 1
    return m, mask, peaks, int(mask.sum())


def reference(c, X):
    """music_2d on the unique grid of one instance's snapshots."""
    phi, theta = unique_grid(c)
    return ref.music_2d(X, c['M'], c['nx'], c['ny'], phi, theta, c['dxl'], c['dyl'])
