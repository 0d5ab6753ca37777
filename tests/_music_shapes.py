"""Shapes, scenes and reference quantities of tests/test_music_shapes.py -- TEST INFRASTRUCTURE ONLY.

Everything here is host arithmetic on ``oracle/music.py`` (complex128, ``np.linalg.eigh``): the case
table, the scene every case shares, the duplicated scan grid of the plateau case, the margins that
decide where a device answer must equal the oracle's exactly, and the restated LDS arithmetic of
``me_lds_bytes`` (csrc/rsp_music_geometry.h).  No device code is touched.
"""
import functools

import numpy as np

from oracle import music as mu

SEED = 20250101
N_INST = 4
DL = 0.5

# id: (N, K, M, S) -- see the module docstring of test_music_shapes.py for what each one reaches
CASES = {
    'n2-k7-m1-s33': (2, 7, 1, 33),
    'n8-k1-m1-s65': (8, 1, 1, 65),
    'n12-k5-m2-s100': (12, 5, 2, 100),
    'n9-k40-m8-s181': (9, 40, 8, 181),
    'n17-k37-m1-s67': (17, 37, 1, 67),
    'n31-k130-m4-s129': (31, 130, 4, 129),
    'n33-k131-m5-s257': (33, 131, 5, 257),
    'n48-k64-m6-s255': (48, 64, 6, 255),
    'n49-k98-m7-s256': (49, 98, 7, 256),
    'n63-k203-m8-s513': (63, 203, 8, 513),
    'n4-k16-m1-s3': (4, 16, 1, 3),
    'n16-k64-m7-s4096': (16, 64, 7, 4096),
    'n16-k64-m8-s4095': (16, 64, 8, 4095),
}
CASE_IDS = list(CASES)
LONG_SCAN = ('n16-k64-m7-s4096', 'n16-k64-m8-s4095')   # S >= 4095: no minimum of exact instances

# tolerances of tests/test_music.py (its module docstring)
TOL = {'c128': dict(X=1e-12, R=1e-12, eig=1e-11, db=1e-7),
       'c64': dict(X=1e-6, R=2e-6, eig=2e-5, db=0.02)}
EXACT_MARGIN_DB = 5e-7   # c128: 5 x the spectrum tolerance -- a passing spectrum cannot reorder such samples
C64_GAP_DB = 0.04        # c64: 2 x the spectrum tolerance between the heights of the M + 1 highest peaks


def scene_for(M):
    """Complex unit-amplitude sources at linspace(-60, 60, M) deg (20 deg when M = 1), awgn 10 dB
    'measured'."""
    ang = np.array([20.0]) if M == 1 else np.linspace(-60.0, 60.0, M)
    return {'angles_rad': np.deg2rad(ang), 'amplitudes': np.ones(M), 'complex_sources': 1, 'snr_db': 10.0,
            'snr_measured': 1}


def scan_for(S):
    return np.linspace(-np.pi / 2, np.pi / 2, S)


@functools.lru_cache(maxsize=None)
def oracle_snapshots(case):
    """The oracle's snapshots of a case, [N_INST, N, K] complex128 (read-only)."""
    N, K, M, _ = CASES[case]
    X = np.stack([mu.synthesize(scene_for(M), N, K, DL, i, SEED) for i in range(N_INST)])
    X.setflags(write=False)
    return X


# ---- the duplicated scan grid (plateaus)
DUP_N, DUP_K, DUP_M = 16, 64, 3
DUP_SOURCES_DEG = (-30.0, 0.0, 45.0)
DUP_REPEATS = {0: 3, 120: 3, 60: 3, 40: 2, 90: 2, 10: 2, 77: 2}   # base-grid index: occurrences


def dup_scene():
    s = scene_for(DUP_M)
    s['angles_rad'] = np.deg2rad(np.array(DUP_SOURCES_DEG))
    return s


def dup_grid():
    """(base grid [121], duplicated grid [131], first[131]): first[s] is the index in the duplicated
    grid of the first occurrence of s's angle."""
    base = np.linspace(-np.pi / 2, np.pi / 2, 121)
    cnt = np.ones(121, np.int64)
    for k, c in DUP_REPEATS.items():
        cnt[k] = c
    dup = np.repeat(base, cnt)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    return base, dup, np.repeat(start, cnt)


@functools.lru_cache(maxsize=None)
def dup_snapshots():
    X = np.stack([mu.synthesize(dup_scene(), DUP_N, DUP_K, DL, i, SEED) for i in range(N_INST)])
    X.setflags(write=False)
    return X


# ---- reference quantities
def top_peaks(spec, M):
    """(peaks [M] int, n_peaks): MUSIC_1D.m:43-47 on a spectrum -- findpeaks, stable descending sort,
    the first M, 1-based and zero-padded when findpeaks finds fewer (the device's convention)."""
    spec = np.asarray(spec, np.float64)
    pk = mu.findpeaks(spec)
    top = pk[np.argsort(-spec[pk], kind='stable')][:M] + 1
    out = np.zeros(M, np.int64)
    out[:len(top)] = top
    return out, len(pk)


def height_gap(spec, M):
    """Smallest gap between consecutive heights among the M + 1 highest peaks of a spectrum (inf
    with fewer than two peaks): below it, a perturbation cannot change which peaks are the top M
    nor their order."""
    spec = np.asarray(spec, np.float64)
    h = np.sort(spec[mu.findpeaks(spec)])[::-1][:M + 1]
    return float(np.min(-np.diff(h))) if len(h) > 1 else np.inf


def exact_margin(spec, M):
    """min(smallest |P_dB[s+1] - P_dB[s]| over the scan, height_gap): a device spectrum within less
    than half of it everywhere has the oracle's findpeaks set, count and top-M order."""
    spec = np.asarray(spec, np.float64)
    return min(float(np.abs(np.diff(spec)).min()), height_gap(spec, M))


def f32_restatement(X, M, scan):
    """MUSIC_1D.m:28-41 with every stage in single precision (X cast to complex64, R formed in
    complex64, LAPACK's complex64 eigh, the residual form of the denominator |a - Q_s Q_s^H a|^2):
    what complex-single arithmetic costs against the complex128 oracle, whatever the kernel.
    Returns (eigenvalues descending, spectrum_db) as float64."""
    X = np.asarray(X).astype(np.complex64)
    N, K = X.shape
    R = (X @ X.conj().T) / np.float32(K)
    R = (np.float32(0.5) * (R + R.conj().T)).astype(np.complex64)
    w, V = np.linalg.eigh(R)
    order = np.argsort(-w, kind='stable')
    Qs = V[:, order[:M]]
    a = mu.steering(N, DL, scan).astype(np.complex64)
    res = a - Qs @ (Qs.conj().T @ a)
    den = np.sum(res.real ** 2 + res.imag ** 2, axis=0, dtype=np.float32)
    P = np.float32(1.0) / den
    return w[order].astype(np.float64), (np.float32(10.0) * np.log10(P / P.max())).astype(np.float64)


# ---- csrc/rsp_music_geometry.h: me_lds_bytes (dynamic LDS of k_music_eig64), restated
ME_VW = 68


def me_lds_bytes(M, S):
    lu = max(5 * 64 * M, 32 * ME_VW)                           # me_lu_doubles
    return (4 * ME_VW * 16 + 64 * 16 + 8 * 16 + 3 * 68 * 8 + 64 * 8 + lu * 8 + M * 64 * 16
            + (S + 8) * 8 + 8 * 16)
