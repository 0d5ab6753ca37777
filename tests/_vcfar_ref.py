"""CPU restatement of the Doppler cell-averaging CFAR of the stage-2 path (include/rsp.h restates
the semantics; the reference vendors it as local_cfar_detector in
main_simulate_echoes_with_array_v3.m:278-314).  numpy, with ``dtype`` (np.float64 or np.float32)
carried through every operation: one IEEE add per window row in ascending order starting from the
first row that exists, one division by the count (CA) or one per window (GOCA, SOCA), one
multiplication by T rounded to ``dtype``, ``>``.  The device result is defined to the bit by these
operations, so the tests compare with ``np.array_equal``.
"""
import numpy as np

from _stage3_ref import find_hits  # noqa: F401  (the hit lists of the tests: beam, then find() order)

SEED = 20250101
CA, GOCA, SOCA = 0, 1, 2


def windows(v, P, r, g):
    """The 1-based inclusive (r_start1, r_end1, r_start2, r_end2) of row ``v`` (1-based) of a map of
    ``P`` rows: the five index lines of the reference (:289-297), g / 2 an integer."""
    h = g // 2
    g_start1 = max(1, v - h)
    r_start1 = max(1, g_start1 - r)
    r_end1 = g_start1 - 1
    g_end2 = min(P, v + h)
    r_start2 = g_end2 + 1
    r_end2 = min(P, r_start2 + r - 1)
    return r_start1, r_end1, r_start2, r_end2


def _running(a, rows, acc, dtype):
    """acc + a[rows[0]] + a[rows[1]] + ..., one rounded add per row (acc None: start from the first)."""
    for i in rows:
        acc = a[i].copy() if acc is None else (acc + a[i]).astype(dtype, copy=False)
    return acc


def local_cfar_detector(amp, cfar, method=CA, dtype=np.float64, strict=True):
    """(flags uint8, thresholds float64) of an amplitude map [P x G] or [P x G x n].  ``cfar``: the
    reference's fields refCells_V, guardCells_V, T_CFAR (its ``method`` is not read); ``method``: 0
    CA (the reference), 1 GOCA, 2 SOCA.  ``amp`` is rounded to ``dtype`` first, as the upload of a
    complex-single plan does; thresholds are widened to double.  ``strict`` False: test ``>=``
    instead of ``>`` (for the tests' preconditions only)."""
    a = np.asarray(amp)
    if a.ndim == 3:
        out = [local_cfar_detector(a[:, :, b], cfar, method, dtype, strict) for b in range(a.shape[2])]
        return np.stack([o[0] for o in out], axis=2), np.stack([o[1] for o in out], axis=2)
    r, g, T = int(cfar['refCells_V']), int(cfar['guardCells_V']), dtype(cfar['T_CFAR'])
    assert r >= 1 and g >= 0 and g % 2 == 0, 'an odd guardCells_V indexes with a non-integer'
    P, G = a.shape
    a = a.astype(dtype)
    zero = np.zeros(G, dtype)
    thr = np.zeros((P, G), dtype)
    for v in range(1, P + 1):
        s1, e1, s2, e2 = windows(v, P, r, g)
        lead, trail = range(s1 - 1, e1), range(s2 - 1, e2)      # 0-based rows, ascending
        nL, nT = len(lead), len(trail)
        if method == CA:
            total = _running(a, trail, _running(a, lead, None, dtype), dtype)
            noise = (total / dtype(nL + nT)).astype(dtype, copy=False) if nL + nT else zero
        else:
            mL = (_running(a, lead, None, dtype) / dtype(nL)).astype(dtype, copy=False) if nL else None
            mT = (_running(a, trail, None, dtype) / dtype(nT)).astype(dtype, copy=False) if nT else None
            if nL and nT:
                noise = np.maximum(mL, mT) if method == GOCA else np.minimum(mL, mT)
            else:
                noise = mL if nL else (mT if nT else zero)
        thr[v - 1] = (noise * T).astype(dtype, copy=False)
    flags = (a > thr) if strict else (a >= thr)
    return flags.astype(np.uint8), thr.astype(np.float64)


# ---- the maps of the tests ---------------------------------------------------------------------
def make_maps(P, G, n_maps=3, seed=SEED):
    """Rayleigh amplitude maps [P x G x n_maps] from a fixed seed with a run of exact zeros in rows
    3..14 (1-based, clipped to P) of column min(4, G) of the last map but one (the only map when
    there is one): cells whose every reference cell lies in the run have threshold 0 and amplitude 0,
    where ``>`` and ``>=`` differ."""
    a = np.random.default_rng(seed).rayleigh(1.0, (P, G, n_maps))
    a[2:min(14, P), min(4, G) - 1, max(n_maps - 2, 0)] = 0.0
    return a
