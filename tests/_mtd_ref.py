"""References of the stand-alone MTD (rsp_mtd): the exact transform and the kernel's algorithm restated.

exact(pc, win, nfft, shift)      the direct DFT in np.longdouble: the phase of term (k, m) is the integer
                                 (k m) mod nfft before any floating point, the roots of unity come from one
                                 table of nfft long doubles, the sums run in long double.
restated(pc, win, nfft, shift,   what k_mtd_any computes, in numpy at the plan's precision and from
         prec)                   rsp_mtd_table's tables alone, every operation rounded to the precision:
                                 x win (w), zero fill, a radix-2 FFT, and on the chirp-z route the product
                                 with Bf, the unscaled inverse FFT and w on the way out.  The device runs
                                 radix-16/8/4 passes with fused multiply-adds: the same order of growth
                                 of the error, other constants.

Where np.longdouble is no wider than double (np.finfo(np.longdouble).nmant < 63), `exact` cannot serve a
complex-double plan as it stands; LONGDOUBLE_OK says so and the tests widen their tolerance by numpy's
own measured share (tests/test_mtd.py says how).
"""
import numpy as np

from rsp.plan import mtd_table

LONGDOUBLE_OK = np.finfo(np.longdouble).nmant >= 63
_CT = {'c128': np.complex128, 'c64': np.complex64}
_RT = {'c128': np.float64, 'c64': np.float32}


def _roots_ld(n, sign=-1):
    k = np.arange(n, dtype=np.longdouble)
    pi = np.arctan(np.longdouble(1)) * 4
    ang = sign * 2 * pi * k / np.longdouble(n)
    return np.cos(ang) + 1j * np.sin(ang)


def shift_rows(X, nfft):
    """MATLAB's fftshift along axis 0: row v holds frequency (v - floor(nfft / 2)) mod nfft."""
    return X[(np.arange(nfft) - nfft // 2) % nfft]


def exact(pc, win, nfft, shift=True):
    pc = np.asarray(pc)
    shp = pc.shape
    P = shp[0]
    x = pc.reshape(P, -1).astype(np.clongdouble)
    if win is not None:
        x = x * np.asarray(win, np.longdouble).reshape(P, 1)
    roots = _roots_ld(nfft)
    m = np.arange(P, dtype=np.int64)
    out = np.empty((nfft, x.shape[1]), np.clongdouble)
    step = max(1, (1 << 18) // max(P, 1))
    for k0 in range(0, nfft, step):
        k = np.arange(k0, min(nfft, k0 + step), dtype=np.int64)
        out[k0:k0 + len(k)] = roots[(k[:, None] * m[None, :]) % nfft] @ x
    if shift:
        out = shift_rows(out, nfft)
    return out.reshape((nfft,) + shp[1:])


def _fft_r2(a, inv, prec):
    """Radix-2 decimation-in-time FFT along axis 0 (a power of two), unscaled, in the precision's type."""
    T = _CT[prec]
    n = a.shape[0]
    lg = n.bit_length() - 1
    rev = np.zeros(n, np.int64)
    for b in range(lg):
        rev |= ((np.arange(n) >> b) & 1) << (lg - 1 - b)
    a = a[rev].astype(T)
    ln = 2
    while ln <= n:
        h = ln // 2
        tw = _roots_ld(ln, 1 if inv else -1)[:h].astype(T)
        a = a.reshape(n // ln, ln, -1)
        u, v = a[:, :h], (a[:, h:] * tw[None, :, None]).astype(T)
        a = np.concatenate(((u + v).astype(T), (u - v).astype(T)), axis=1).reshape(n, -1)
        ln *= 2
    return a


def restated(pc, win, nfft, shift=True, prec='c128'):
    T, R = _CT[prec], _RT[prec]
    pc = np.asarray(pc)
    shp = pc.shape
    P = shp[0]
    x = pc.reshape(P, -1).astype(T)
    if win is not None:
        x = (x * np.asarray(win).astype(R).reshape(P, 1)).astype(T)
    if nfft & (nfft - 1) == 0:
        a = np.zeros((nfft, x.shape[1]), T)
        a[:P] = x
        X = _fft_r2(a, False, prec) if nfft > 1 else a
    else:
        w, Bf = mtd_table(nfft, prec)
        w, Bf = w.astype(T), Bf.astype(T)
        M = len(Bf)
        a = np.zeros((M, x.shape[1]), T)
        a[:P] = (x * w[:P, None]).astype(T)
        A = (_fft_r2(a, False, prec) * Bf[:, None]).astype(T)
        X = (_fft_r2(A, True, prec)[:nfft] * w[:, None]).astype(T)
    if shift:
        X = shift_rows(X, nfft)
    return X.reshape((nfft,) + shp[1:])
