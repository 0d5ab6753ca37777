"""CPU restatement of the cross GOCA-CFAR map detector (include/rsp.h restates the semantics; the
reference vendors it as fun_run_goca_cfar_8 in fun_process_single_frame.m:172-223, test at :192-213).
numpy, with ``dtype`` (np.float64 or np.float32) carried through every operation: one IEEE add per
window cell in ascending index order starting from +0, the quotient of the greater sum of either
axis (float64: one correctly rounded division by the count; float32: one multiplication by
RN(1 / count), K3's form), the greater of the two, one multiplication by T rounded to ``dtype``,
``>``.  Cells the reference never tests have flag 0 and threshold +Inf.  The device result is defined
to the bit by these operations, so the tests compare with ``np.array_equal``.
"""
import numpy as np

from _stage3_ref import find_hits  # noqa: F401  (the hit lists of the tests: map, then find() order)

SEED = 20250101
FIELDS = ('refCells_R', 'guardCells_R', 'refCells_V', 'guardCells_V')


def cfar_dict(win):
    """cfar_params of a window (rR, gR, rV, gV, T)."""
    return dict(refCells_R=win[0], guardCells_R=win[1], refCells_V=win[2], guardCells_V=win[3], T_CFAR=win[4])


def cells_under_test(P, G, cfar):
    """0-based (r0, r1, v0, v1): the cells under test are [r0, r1) x [v0, v1) (fsf:192-193); all 0
    when there are none."""
    rR, gR, rV, gV = (int(cfar[k]) for k in FIELDS)
    hR, hV = rR + gR, rV + gV
    if G <= 2 * hR or P <= 2 * hV:
        return 0, 0, 0, 0
    return hR, G - hR, hV, P - hV


def quotient(x, n, dtype):
    """The mean of a slice sum over n cells as the device forms it."""
    if dtype == np.float64:
        return (x / dtype(n)).astype(dtype, copy=False)
    return (x * (dtype(1) / dtype(n))).astype(dtype, copy=False)      # x * RN(1 / n)


def slice_sums(a, cfar, dtype):
    """(lr, tr, lv, tv) over the cells under test of one map ``a`` [P x G] of ``dtype``: each sum one
    rounded add per cell in ascending index order, starting from +0."""
    rR, gR, rV, gV = (int(cfar[k]) for k in FIELDS)
    P, G = a.shape
    r0, r1, v0, v1 = cells_under_test(P, G, cfar)
    hR, hV = rR + gR, rV + gV
    lr, tr, lv, tv = (np.zeros((v1 - v0, r1 - r0), dtype) for _ in range(4))
    for q in range(rR):
        lr = (lr + a[v0:v1, r0 - hR + q:r1 - hR + q]).astype(dtype, copy=False)
        tr = (tr + a[v0:v1, r0 + gR + 1 + q:r1 + gR + 1 + q]).astype(dtype, copy=False)
    for q in range(rV):
        lv = (lv + a[v0 - hV + q:v1 - hV + q, r0:r1]).astype(dtype, copy=False)
        tv = (tv + a[v0 + gV + 1 + q:v1 + gV + 1 + q, r0:r1]).astype(dtype, copy=False)
    return lr, tr, lv, tv


def goca_cfar_maps(amp, cfar, dtype=np.float64, strict=True):
    """(flags uint8, thresholds float64) of an amplitude map [P x G] or [P x G x n].  ``cfar``: the
    reference's fields refCells_R, guardCells_R, refCells_V, guardCells_V, T_CFAR.  ``amp`` and T are
    rounded to ``dtype`` first, as the upload of a complex-single plan does; thresholds are widened to
    double.  ``strict`` False: test ``>=`` instead of ``>`` (for the tests' preconditions only)."""
    a = np.asarray(amp)
    if a.ndim == 3:
        out = [goca_cfar_maps(a[:, :, b], cfar, dtype, strict) for b in range(a.shape[2])]
        return np.stack([o[0] for o in out], axis=2), np.stack([o[1] for o in out], axis=2)
    rR, gR, rV, gV = (int(cfar[k]) for k in FIELDS)
    T = dtype(cfar['T_CFAR'])
    assert rR >= 1 and rV >= 1 and gR >= 0 and gV >= 0 and np.isfinite(T) and T > 0
    P, G = a.shape
    a = a.astype(dtype)
    flags = np.zeros((P, G), np.uint8)
    thr = np.full((P, G), np.inf, np.float64)
    r0, r1, v0, v1 = cells_under_test(P, G, cfar)
    if r1 > r0:
        lr, tr, lv, tv = slice_sums(a, cfar, dtype)
        nR = quotient(np.maximum(lr, tr), rR, dtype)
        nV = quotient(np.maximum(lv, tv), rV, dtype)
        t = (np.maximum(nR, nV) * T).astype(dtype, copy=False)
        cut = a[v0:v1, r0:r1]
        flags[v0:v1, r0:r1] = (cut > t) if strict else (cut >= t)
        thr[v0:v1, r0:r1] = t
    return flags, thr


def deciding_slice(amp, cfar, dtype=np.float64):
    """Per cell under test of one map [P x G]: which of the four slice means (0 lr, 1 tr, 2 lv, 3 tv)
    is the greatest, the first one on a tie."""
    a = np.asarray(amp).astype(dtype)
    rR, rV = int(cfar['refCells_R']), int(cfar['refCells_V'])
    lr, tr, lv, tv = slice_sums(a, cfar, dtype)
    m = np.stack([quotient(lr, rR, dtype), quotient(tr, rR, dtype), quotient(lv, rV, dtype), quotient(tv, rV, dtype)])
    return np.argmax(m, axis=0)


# ---- the maps of the tests ---------------------------------------------------------------------
def make_maps(P, G, n_maps, seed=SEED, cfar=None):
    """Rayleigh(1.0) amplitude maps [P x G x n_maps] from a fixed seed.  With ``cfar``: ties planted at
    the first and the last cell under test of the last map but one (the only map when there is one):
    the cell's own row over r +- hR and its own column over v +- hV are 2.0 and the cell itself 3.0, so
    with T_CFAR = 1.5 every slice mean is 2.0 and the threshold exactly 3.0, where ``>`` and ``>=``
    differ."""
    a = np.random.default_rng(seed).rayleigh(1.0, (P, G, n_maps))
    if cfar is not None:
        r0, r1, v0, v1 = cells_under_test(P, G, cfar)
        hR, hV = r0, v0
        m = max(n_maps - 2, 0)
        for v, r in ((v0, r0), (v1 - 1, r1 - 1)) if r1 > r0 else ():
            a[v, r - hR:r + hR + 1, m] = 2.0
            a[v - hV:v + hV + 1, r, m] = 2.0
            a[v, r, m] = 3.0
    return a
