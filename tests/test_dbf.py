"""The stand-alone DBF on the device (k_dbf, rsp_dbf.hip) against ``oracle.chain.dbf`` (``x @ W'``) and
``x @ W.'``, within the project's tolerance for complex maps (``_parity.MAP_TOL`` of the map maximum).

Shapes (P, N), each with every (C, B) of the host test, both precisions and both ``conj`` values:
  (1, 1)     one position
  (5, 7)     35 positions: odd, two f64 sub-tiles and a tail of 3, one f32 sub-tile with a tail
  (2, 8)     16: exactly one f64 sub-tile
  (2, 16)    32: exactly one f32 sub-tile
  (3, 11)    33: one past an f32 sub-tile; odd, so complex single pads its planes' pitch
  (64, 33)   2112: several workgroups in complex double, several rounds and waves in either
  (1, wg+1)  one position more than a workgroup's share (``describe_dbf``): a second workgroup of one lane
Weights and data are random complex, so the ``conj`` and plain results differ by far more than the
tolerance; that is asserted too.  The output lies between two sentinel planes that must stay untouched.
"""
import numpy as np
import pytest

from rsp import config as C
from rsp.plan import Plan, describe_dbf
from rsp.precompute import precompute as product_precompute
from oracle import chain
from _parity import MAP_TOL, map_close
from _scen import plumbing_config, plumbing_weights

pytestmark = pytest.mark.gpu

CB = [(1, 1), (3, 1), (5, 3), (12, 3), (16, 8), (16, 9), (16, 13), (32, 16)]
SHAPES = [(1, 1), (5, 7), (2, 8), (2, 16), (3, 11), (64, 33)]
SENTINEL = complex(-7.25, 1234.5)


@pytest.fixture(scope='module', params=['c128', 'c64'])
def plan(request):
    cfg = plumbing_config(16, 3, 16)
    W, ang, k = plumbing_weights(cfg)
    p = Plan(cfg, C.default_cfar_params(), C.default_cluster_params(), product_precompute(cfg, W, ang, k, C.V8_FIR),
             precision=request.param)
    yield p
    p.close()


def _data(P, N, Cn, B, seed=3):
    rng = np.random.default_rng(seed + 1000 * Cn + 10 * B + P * N)
    x = rng.standard_normal((P, N, Cn)) + 1j * rng.standard_normal((P, N, Cn))
    W = rng.standard_normal((B, Cn)) + 1j * rng.standard_normal((B, Cn))
    return x, W


def _run(plan, x, W, conj):
    P, N, _ = x.shape
    B = W.shape[0]
    big = np.full((P, N, B + 2), SENTINEL, np.complex128, order='F')
    out = big[:, :, 1:B + 1]
    got = plan.dbf(x, W, conj=conj, out=out)
    assert got is out
    assert (big[:, :, 0] == SENTINEL).all() and (big[:, :, B + 1] == SENTINEL).all(), 'a sentinel plane was written'
    assert not (out == SENTINEL).any(), 'an output element was not written'
    return out.copy()


@pytest.mark.parametrize('Cn,B', CB)
def test_dbf_against_the_oracle(plan, Cn, B):
    prec, tol = plan.precision, MAP_TOL[plan.precision]
    wg = describe_dbf(1, 1, Cn, B, prec)['wg_positions']
    for P, N in SHAPES + [(1, wg + 1)]:
        x, W = _data(P, N, Cn, B)
        if prec == 'c64':   # the values the device computes on: the comparison is then of the arithmetic alone
            x = x.astype(np.complex64)
        want = {True: chain.dbf(x.astype(np.complex128), W), False: x.astype(np.complex128) @ W.T}
        got = {cj: _run(plan, x, W, cj) for cj in (True, False)}
        for cj in (True, False):
            print('P=%d N=%d C=%d B=%d conj=%d' % (P, N, Cn, B, cj), end=' ')
            map_close(got[cj], want[cj], tol)
        scale = np.abs(want[True]).max()
        assert np.abs(got[True] - got[False]).max() > 1e3 * tol * scale, 'conj and plain results do not differ'


@pytest.mark.parametrize('P,N', [(5, 7), (64, 33)])
def test_input_dtype_is_converted_to_the_plan_precision(plan, P, N):
    """complex64 into a complex-double plan (widened: exact) and complex128 into a complex-single plan
    (narrowed as upload_cube narrows: the result is that of the rounded cube)."""
    x, W = _data(P, N, 16, 13, seed=5)
    other = np.complex64 if plan.precision == 'c128' else np.complex128
    xo = x.astype(other)
    seen = xo.astype(np.complex64) if plan.precision == 'c64' else xo     # what the device holds
    got = _run(plan, xo, W, True)
    map_close(got, chain.dbf(seen.astype(np.complex128), W), MAP_TOL[plan.precision])
    np.testing.assert_array_equal(got, _run(plan, seen, W, True))


def test_weights_and_shapes_are_checked(plan):
    x, W = _data(4, 6, 5, 3)
    with pytest.raises(ValueError):
        plan.dbf(x, W[:, :4])
    with pytest.raises(ValueError):
        plan.dbf(x, W, out=np.zeros((4, 6, 3), np.complex128))   # C order


def test_profile_dbf(plan):
    P, N, Cn, B = 64, 33, 16, 13
    r = plan.profile_dbf(P, N, Cn, B, iters=3)
    esz = 16 if plan.precision == 'c128' else 8
    assert r['stage'] == 'k_dbf' and r['ms'] > 0
    assert r['bytes'] == esz * P * N * (Cn + B)
