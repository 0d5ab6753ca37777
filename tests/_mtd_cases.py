"""The case table of the stand-alone MTD (k_mtd_any, rsp_mtd.hip) and the tolerance of its tests.

A case is (P, nfft): P pulses transformed to nfft rows.  The groups (tests/test_mtd.py runs every case
in both precisions on the device; tests/test_mtd_ref.py runs the restatement over the same table):

  tiny      the smallest rows; P = 1 gives every bin = win[0] x[0]; the odd sizes a plan refuses
  pow2      every pass count of plan_pow2; v7_7's own call (332 -> 512); zero fill (100 -> 2048)
  edges     for M = 32 .. 4096, nfft = M / 2 - 1 and M / 2 + 1: 2 nfft - 1 against the chirp-z length M,
            the wrap-around of the circular convolution
  project   the reference's P and its factors, the lengths VERDICT names, a prime

Inputs are Gaussian columns with a Kaiser window, both rounded to single precision, so that a
complex-single and a complex-double plan see the same values and share one exact transform.

The tolerance of a column's error ||got - exact||_2 / ||exact||_2 is C u log2(max(M, 2)), u = 2^-53
(c128) or 2^-24 (c64), M the transform length `describe_mtd` reports.  C is 4 x the largest value of
err / (u log2 M) that the restatement of the kernel's algorithm (tests/_mtd_ref.py: restated) shows
against the exact transform over this table with the inputs below (G = 5, n_maps = 2);
tests/test_mtd_ref.py recomputes it and asserts the constants here are 4 x it within 10 %.  The
factor 4 covers what differs between the device and the restatement in constants and not in order: the
radices, FMA contraction, the table rounding.
"""
import functools

import numpy as np

TINY = [(1, 1), (2, 2), (3, 3), (5, 7), (7, 7), (1, 8), (15, 15)]
POW2 = [(16, 16), (32, 32), (128, 128), (512, 512), (1024, 1024), (2048, 2048), (332, 512), (100, 2048)]
EDGES = [(n, n) for n in (17, 31, 33, 63, 65, 127, 129, 255, 257, 511, 513, 1023, 1025, 2047)]
PROJECT = [(n, n) for n in (83, 96, 166, 200, 320, 331, 332)] + [(332, 333)] + [(n, n) for n in (384, 636, 1000)]
CASES = TINY + POW2 + EDGES + PROJECT
CASE_IDS = ['%d-%d' % c for c in CASES]

# One case per route and per length of the LDS transform: these run the column sweep (G around the
# columns of a workgroup, n_maps 1 and 3).  {(route, M): (P, nfft)}
COLUMN_CASES = {('pow2', 1): (1, 1), ('pow2', 2): (2, 2), ('pow2', 8): (1, 8), ('pow2', 16): (16, 16), ('pow2', 32): (32, 32),
                ('pow2', 128): (128, 128), ('pow2', 512): (332, 512), ('pow2', 1024): (1024, 1024),
                ('pow2', 2048): (100, 2048),
                ('chirpz', 8): (3, 3), ('chirpz', 16): (5, 7), ('chirpz', 32): (15, 15), ('chirpz', 64): (17, 17),
                ('chirpz', 128): (33, 33), ('chirpz', 256): (83, 83), ('chirpz', 512): (129, 129),
                ('chirpz', 1024): (332, 332), ('chirpz', 2048): (513, 513), ('chirpz', 4096): (1025, 1025)}

PRECS = ('c128', 'c64')
U = {'c128': 2.0 ** -53, 'c64': 2.0 ** -24}
# 4 x the restatement's largest err / (u log2 M) over CASES (test_mtd_ref.py::test_tolerance_constant)
C_TOL = {'c128': 2.79, 'c64': 3.32}
G_MAIN, MAPS_MAIN = 5, 2


def tolerance(prec, M):
    return C_TOL[prec] * U[prec] * np.log2(max(M, 2))


def kaiser32(P, beta=5.0):
    """A Kaiser window whose values are single-precision numbers."""
    return np.kaiser(P, beta).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def gaussian(P, G, n_maps, seed=0):
    """Gaussian columns [P, G, n_maps] (Fortran order) whose parts are single-precision numbers."""
    rng = np.random.default_rng(1000003 * seed + 4099 * P + 17 * G + n_maps)
    x = rng.standard_normal((2, P, G, n_maps)).astype(np.float32)
    x = np.asfortranarray((x[0] + 1j * x[1]).astype(np.complex128))
    x.setflags(write=False)
    return x


def col_err(got, want):
    """||got - want||_2 / ||want||_2 of every column (axis 0), in double."""
    d = np.asarray(got, np.clongdouble) - np.asarray(want, np.clongdouble)
    num = np.sqrt((np.abs(d) ** 2).sum(axis=0))
    den = np.sqrt((np.abs(np.asarray(want, np.clongdouble)) ** 2).sum(axis=0))
    return (num / den).astype(np.float64)
