"""GPU test of the order of refusals in the CFAR call family: the three detectors (stage-3 range CFAR, Doppler
CA-CFAR, cross GOCA-CFAR) x the stage-2 entries on beams, on gated beams and on a raw cube, on one small plan
in complex double.  Every entry checks its arguments (null, negative hits_cap), then the detector's
parameters, then the gate columns, then runs; a refused call leaves the plan as it was."""
import numpy as np
import pytest

import rsp
from rsp import config as C
from rsp.plan import Plan, describe_stage3, describe_vcfar, describe_xcfar
from rsp.precompute import precompute as product_precompute
from oracle import chain
from _scen import SEED, plumbing_config, plumbing_weights

S3 = dict(refCells_R=5, saveCells_R=14, T_CFAR=1.5, CFARmethod_R=0, MTD_0v_num=1)
VC = dict(refCells_V=4, guardCells_V=6, T_CFAR=1.5)
XC = dict(refCells_R=3, guardCells_R=2, refCells_V=2, guardCells_V=1, T_CFAR=1.3)
KEYS = ('mtd', 'amp', 'flags', 'threshold', 'hits')


def _refusal(fn, *a, **kw):
    with pytest.raises(rsp.RspError) as e:
        fn(*a, **kw)
    return e.value.code, str(e.value)


@pytest.mark.gpu
def test_refusal_order_and_plan_state():
    cfg = plumbing_config(16, 3, 16)
    W, ang, k = plumbing_weights(cfg)
    cube = chain.philox_noise(cfg, 1, SEED)
    segs = tuple(cfg['Sig_Config']['point_prt_segments'])
    p = Plan(cfg, C.default_cfar_params(), C.default_cluster_params(), product_precompute(cfg, W, ang, k, C.V8_FIR))
    try:
        P, G, N = p.P, p.G, p.N
        iq = p.dbf(cube, W)
        cols = ((1, 300), (301, 700), (701, N))          # the whole PRT as three gated pieces
        bad_cols = ((1, 300), (301, 700), (701, N + 5))  # ... and past its end
        # detector -> (good parameters, one bad parameter, its describe_* call, beams entry, raw-cube entry)
        dets = {
            's3': (S3, dict(S3, refCells_R=0), lambda c: describe_stage3(P, segs, c), p.process_stage2_cfar,
                   p.process_raw_stage2_cfar),
            'vc': (VC, dict(VC, guardCells_V=3), lambda c: describe_vcfar(P, G, c), p.process_stage2_vcfar,
                   p.process_raw_stage2_vcfar),
            'xc': (XC, dict(XC, refCells_V=0), lambda c: describe_xcfar(P, G, c), p.process_stage2_xcfar,
                   p.process_raw_stage2_xcfar),
        }
        # entry shape -> (input, keyword arguments of a valid call, of one with bad gate columns or None)
        shapes = {
            'beams': (iq, {}, None),
            'gated': (iq, dict(gate_cols=cols), dict(gate_cols=bad_cols)),
            'raw': (cube, dict(W=W, gate_cols=cols), dict(W=W, gate_cols=bad_cols)),
        }
        regate = {'gated': _refusal(p.process_stage2, iq, gate_cols=bad_cols),
                  'raw': _refusal(p.process_raw_stage2, cube, W=W, gate_cols=bad_cols)}
        for r in regate.values():
            assert r[0] == rsp._abi.RSP_ERR_INVALID and 'outside the %d-sample PRT' % N in r[1], r

        def entry(det, shape):
            return dets[det][3] if shape != 'raw' else dets[det][4]

        table = [(d, s) for d in dets for s in shapes]
        before = {(d, s): entry(d, s)(shapes[s][0], dets[d][0], **shapes[s][1]) for d, s in table}
        for d, s in table:
            good, bad, describe, _, _ = dets[d]
            x, kw, kw_bad = shapes[s]
            fn = entry(d, s)
            want = _refusal(describe, bad)
            assert want[0] == rsp._abi.RSP_ERR_INVALID
            # (a) the parameter is refused first, whatever the gate columns are
            assert _refusal(fn, x, bad, **(kw_bad or kw)) == want, (d, s)
            # (b) valid parameters: the gate columns' refusal is the re-insertion's
            if kw_bad:
                assert _refusal(fn, x, good, **kw_bad) == regate[s], (d, s)
            # (c) the argument check comes before either
            code, msg = _refusal(fn, x, bad, hits_cap=-1, **(kw_bad or kw))
            assert code == rsp._abi.RSP_ERR_INVALID and 'negative hits_cap' in msg, (d, s, msg)
        # (d) the plan is as it was: the stage-2 result is still there, and every entry returns the same bits
        prof = p.profile_stage3(S3, iters=1)
        assert sorted(prof) == ['fused_all', 'fused_hits', 'real'] and all(ms > 0 for ms, _ in prof.values())
        for d, s in table:
            after = entry(d, s)(shapes[s][0], dets[d][0], **shapes[s][1])
            assert after['n_hits'] == before[d, s]['n_hits'] > 0, (d, s)
            for key in KEYS:
                assert np.array_equal(after[key], before[d, s][key]), (d, s, key)
    finally:
        p.close()
