"""The host conversions around the frame chain's synchronous calls (csrc/rsp_frame_host.cpp), on the
device: an input whose precision is not the plan's, and the layout of the map a call returns.

The `plumbing` waveform at P = 12, B = 3, C = 16 (the smallest shape the routes accept; test_fused
runs it too), three targets over noise, a CFAR window that leaves Doppler cells under test at P = 12.

Input precision.  A complex-double plan widens a complex64 input on the host, float to double; a
complex-single plan narrows a complex128 input, double to float by a cast.  numpy's astype does the
same to each value, so the call on the other precision's array and the call on the array converted
beforehand see the same device input and return the same bits: stage-2 maps, detections, targets.

Map layout.  process_cube's `rdm` goes through the library's [B][P][G] -> [P x G x B] transpose;
Plan.rdm_from_device downloads the map a queued frame wrote and transposes it in numpy.  The two
are independent paths to the same array and must agree to the bit.
"""
import numpy as np
import pytest

from rsp import config as C
from rsp.plan import Plan
from rsp.precompute import precompute as product_precompute
from oracle import chain, precompute as oracle_precompute
from _scen import SEED, plumbing_config, plumbing_weights, _route_cfar, _route_targets

pytestmark = pytest.mark.gpu
P, B, NCH = 12, 3, 16
_IN = {}


def _inputs():
    """(cfg, product precompute, cube [P, N, C], beams [P, N, B]) in complex128, computed once."""
    if not _IN:
        cfg = plumbing_config(P, B, NCH)
        W, ang, k = plumbing_weights(cfg)
        pre_o = oracle_precompute.precompute(cfg, W, ang, k, C.V8_FIR)
        cube = chain.synthesize_echo(_route_targets(cfg, ang), cfg, pre_o) + chain.philox_noise(cfg, 1, SEED)
        iq = chain.dbf(cube, W)
        for a in (cube, iq):
            a.setflags(write=False)
        _IN.update(cfg=cfg, pre=product_precompute(cfg, W, ang, k, C.V8_FIR), cube=cube, iq=iq)
    return _IN


@pytest.fixture(scope='module', params=['c128', 'c64'])
def plan(request):
    s = _inputs()
    p = Plan(s['cfg'], _route_cfar(P, 'small'), C.default_cluster_params(), s['pre'], precision=request.param)
    yield p
    p.close()


def _other_then_own(plan, a):
    """``a`` in the precision the plan does not have, and that array converted to the plan's."""
    other = a.astype(np.complex64) if plan.precision == 'c128' else a.astype(np.complex128)
    assert other.dtype != plan.cdtype
    return other, other.astype(plan.cdtype)


def test_stage2_input_of_the_other_precision(plan):
    other, own = _other_then_own(plan, _inputs()['iq'])
    mtd_o, pc_o = plan.process_stage2(other)
    mtd, pc = plan.process_stage2(own)
    assert np.abs(mtd).max() > 0 and np.abs(pc).max() > 0
    assert np.array_equal(mtd_o, mtd) and np.array_equal(pc_o, pc)


def test_cube_input_of_the_other_precision(plan):
    other, own = _other_then_own(plan, _inputs()['cube'])
    got = plan.process_cube(other, frame_idx=3)
    want = plan.process_cube(own, frame_idx=3)
    print(plan.precision, len(want['detections']), 'detections', len(want['final_targets']), 'targets')
    assert len(want['detections']) > 0 and len(want['final_targets']) > 0
    assert got['detections'] == want['detections'] and got['final_targets'] == want['final_targets']


def test_rdm_layout_against_the_queue_and_numpy(plan):
    cube = _inputs()['cube'].astype(plan.cdtype)
    sz = plan.sizes
    d_cube = plan.device_alloc(plan.cube_bytes)
    d_rdm = plan.device_alloc(sz.rdm_elems * sz.elem_bytes)
    try:
        plan.upload_cube(d_cube, cube)
        plan.enqueue_many([d_cube], [5], rdms=[d_rdm])
        plan.drain()
        plan.results()
        queued = plan.rdm_from_device(d_rdm)
    finally:
        plan.device_free(d_cube)
        plan.device_free(d_rdm)
    rdm = plan.process_cube(cube, frame_idx=5, want_rdm=True)['rdm']
    assert rdm.shape == queued.shape == (P, sz.G, B) and rdm.dtype == np.complex128
    assert np.abs(rdm).max() > 0
    assert np.array_equal(rdm, queued.astype(np.complex128))
