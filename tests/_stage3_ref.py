"""CPU restatement of the stage-3 range CFAR of the stage-2 path (include/rsp.h restates the
semantics; the reference vendors it as local_execute_cfar / executeCFAR_2D / Function_CFAR1D_sub in
debug_simulated_data_processing_v2.m:419-511).  numpy, with ``dtype`` (np.float64 or np.float32)
carried through every operation: one IEEE add per window cell in ascending column order, one
division by r, one multiplication by T rounded to ``dtype``, ``>=``.  The device result is defined
to the bit by these operations, so the tests compare with ``np.array_equal``.
"""
import numpy as np

FIELDS = ('refCells_R', 'saveCells_R', 'T_CFAR', 'CFARmethod_R', 'MTD_0v_num')


def matlab_round(x):
    """MATLAB round: half away from zero."""
    return int(np.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def notch_rows(P, z):
    """1-based (first, last) rows of the zero-velocity notch, clipped to 1..P (:446-450)."""
    zc = matlab_round(P / 2) + 1
    return max(1, zc - z), min(P, zc + z)


def window_means(seg, r, dtype):
    """M[:, j] = mean of seg[:, j : j + r] for every start column j: the r cells added in ascending
    order starting from the first, then one division."""
    n = seg.shape[1]
    m = n - r + 1
    acc = seg[:, 0:m].astype(dtype, copy=True)
    for q in range(1, r):
        acc = (acc + seg[:, q:q + m]).astype(dtype, copy=False)
    return (acc / dtype(r)).astype(dtype, copy=False)


def cfar_segment(seg, r, s, T, method, dtype, strict=False):
    """Function_CFAR1D_sub (:467-511) on one segment [rows x n]: (flags, thresholds)."""
    rows, n = seg.shape
    thr = np.zeros((rows, n), dtype)
    if n == 0:
        return np.zeros((rows, n), bool), thr
    H = s + r
    assert n >= 2 * H, 'the reference indexes out of range when a segment is shorter than 2 (s + r)'
    M = window_means(seg, r, dtype)
    y = np.arange(n)                      # 0-based cell
    jl, jr = y - H, y + s + 1             # start columns of the trailing / leading window
    hasl, hasr = jl >= 0, y + H <= n - 1
    il = np.where(hasl, jl, jr)
    ir = np.where(hasr, jr, jl)
    ml, mr = M[:, il], M[:, ir]
    u = np.maximum(ml, mr) if method == 0 else np.minimum(ml, mr)
    thr = (u * dtype(T)).astype(dtype, copy=False)
    return (seg > thr) if strict else (seg >= thr), thr


def local_execute_cfar(amp, cfar, segments, dtype=np.float64, strict=False):
    """(flags uint8, thresholds float64) of an amplitude map [P x G] or [P x G x n].  ``segments``:
    (narrow, medium, long) column counts; ``cfar``: the reference's fields.  ``amp`` is rounded to
    ``dtype`` first, as the upload of a complex-single plan does; thresholds are widened to double.
    ``strict``: test ``>`` instead of ``>=`` (for the tests' preconditions only)."""
    a = np.asarray(amp)
    if a.ndim == 3:
        out = [local_execute_cfar(a[:, :, b], cfar, segments, dtype, strict) for b in range(a.shape[2])]
        return np.stack([o[0] for o in out], axis=2), np.stack([o[1] for o in out], axis=2)
    r, s, T, method, z = (cfar[k] for k in FIELDS)
    P, G = a.shape
    assert sum(segments) == G
    a = a.astype(dtype)
    z0, z1 = notch_rows(P, int(z))
    keep = np.ones(P, bool)
    keep[z0 - 1:z1] = False               # z0 > z1: an empty notch
    flags = np.zeros((P, G), np.uint8)
    thr = np.zeros((P, G), np.float64)
    c = 0
    for n in segments:
        f, t = cfar_segment(a[keep, c:c + n], int(r), int(s), T, int(method), dtype, strict)
        flags[keep, c:c + n] = f
        thr[keep, c:c + n] = t
        c += n
    return flags, thr


def find_hits(amp, flags, thr, dtype=np.float64):
    """The hit list in beam-then-find() order (r outer, v inner), as rows (v, r, beam, amp, threshold)
    with 1-based indices; amp as tested (rounded to ``dtype``, widened to double)."""
    a = np.asarray(amp).astype(dtype).astype(np.float64)
    if a.ndim == 2:
        a, flags, thr = a[:, :, None], flags[:, :, None], thr[:, :, None]
    out = []
    for b in range(a.shape[2]):
        r, v = np.nonzero(flags[:, :, b].T)     # row-major over the transpose: r outer, v inner
        out.append(np.column_stack([v + 1, r + 1, np.full(v.size, b + 1), a[v, r, b], thr[v, r, b]]))
    return np.concatenate(out, axis=0) if out else np.zeros((0, 5))


# ---- the maps of the tests ---------------------------------------------------------------------
ZERO_STRETCH = 50   # cells: with windows up to s + r = 19 on either side, 12 .. 50 of them tie at 0 >= 0


def make_maps(P, segments, zero_at, n_maps=3, seed=20250101):
    """Rayleigh amplitude maps [P x G x n_maps] from a fixed seed with a stretch of ZERO_STRETCH
    exact zeros in row 2 (1-based; never notched for MTD_0v_num <= 1 at P >= 8) of the last map but
    one (the only map when there is one), starting at 0-based column ``zero_at``."""
    rng = np.random.default_rng(seed)
    a = rng.rayleigh(1.0, (P, sum(segments), n_maps))
    a[1, zero_at:zero_at + ZERO_STRETCH, max(n_maps - 2, 0)] = 0.0
    return a
