"""Timing of the stage-3 range CFAR of the stage-2 path (usage: stage3_prof.py [iters] [--no-baseline]
[--out FILE]).

At the reference frame (debug_simulated_data_processing_v3.m's config: 13 beams, 332 x 3404 maps)
and at `plumbing`, on complex Gaussian noise beams: one fused call (rsp_process_stage2_cfar) leaves
the MTD result on the device, then k_s3_cfar is timed alone with HIP events (rsp_profile_stage3) in
its three forms -- real amplitudes in, flags and thresholds out (`real`); the stage-2 result in,
amplitudes, flags and thresholds out (`fused_all`); the stage-2 result in, the hit list alone
(`fused_hits`).  Per form: ms, the algorithmic bytes (every input cell read once, every output cell
written once) and bytes / time as a fraction of the stream-copy rate rsp_hbm_copy_probe measures on
the same card (the figure `bench.py --full` reports as roofline.stream_copy_GBps).

Unless --no-baseline, also one wall-clock run each, at the reference frame, of what a user of the
stage-2 path had to do before (`Plan.process_stage2`, |.| on the host and the numpy restatement
tests/_stage3_ref.py on the downloaded map) and of the fused call with only the hit list requested.
Prints one JSON line; --out also writes it to FILE.
"""
import ctypes as ct
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'radar-signal-simulation-and-target-detection_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import rsp  # noqa: E402
from rsp import _abi, config as C  # noqa: E402
from rsp.plan import Plan  # noqa: E402

args = sys.argv[1:]
out_path = args[args.index('--out') + 1] if '--out' in args else None
baseline = '--no-baseline' not in args
iters = int(args[0]) if args and args[0].isdigit() else 20


def stream_copy_gbps(dev=0):
    best = 0.0
    for _ in range(3):   # as bench.py --full: the best of 3 probes of 20 copies of 1 GiB
        g = ct.c_double()
        if _abi.lib().rsp_hbm_copy_probe(dev, 1 << 30, 20, ct.byref(g)) == 0:
            best = max(best, g.value)
    return best


def noise_beams(P, N, B, seed=20250101):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((P, N, B)) + 1j * rng.standard_normal((P, N, B))) / np.sqrt(2.0)


def run(name, cfg, pre, cfar, copy_gbps, with_baseline):
    plan = Plan(cfg, C.default_cfar_params(), C.default_cluster_params(), pre)
    res = dict(config=name, P=plan.P, G=plan.G, B=plan.B, cfar={k: cfar[k] for k in
                                                                ('refCells_R', 'saveCells_R', 'T_CFAR', 'CFARmethod_R',
                                                                 'MTD_0v_num')})
    try:
        iq = noise_beams(plan.P, plan.N, plan.B)
        t0 = time.perf_counter()
        first = plan.process_stage2_cfar(iq, cfar, want=('hits',))
        t1 = time.perf_counter()
        res['n_hits'] = first['n_hits']
        for form, (ms, nbytes) in plan.profile_stage3(cfar, iters=iters).items():
            gbps = nbytes / (ms * 1e-3) / 1e9
            res[form] = dict(ms=ms, bytes=nbytes, GBps=gbps, frac_of_stream_copy=gbps / copy_gbps if copy_gbps else None)
        if with_baseline:
            import _stage3_ref as ref
            segs = tuple(cfg['Sig_Config']['point_prt_segments'])
            t2 = time.perf_counter()
            hits = plan.process_stage2_cfar(iq, cfar, want=('hits',))
            t3 = time.perf_counter()
            mtd, _ = plan.process_stage2(iq)
            t4 = time.perf_counter()
            flags, _ = ref.local_execute_cfar(np.abs(mtd), cfar, segs)
            t5 = time.perf_counter()
            res['baseline'] = dict(process_stage2_s=t4 - t3, host_abs_and_numpy_cfar_s=t5 - t4, total_s=t5 - t3,
                                   n_hits=int(flags.sum()))
            res['fused_hits_only_call'] = dict(first_call_s=t1 - t0, call_s=t3 - t2, n_hits=hits['n_hits'],
                                               speedup_vs_baseline=(t5 - t3) / (t3 - t2))
    finally:
        plan.close()
    return res


copy = stream_copy_gbps()
ref_cfg = C.stage2_config(C.debug_v3_config())
out = dict(iters=iters, stream_copy_GBps=copy, runs=[
    run('reference', ref_cfg, rsp._stage2_precompute(ref_cfg), C.debug_v2_cfar_config(C.debug_v3_config()), copy, baseline)])
pcfg, _, _, W, ang, k = C.named_config('plumbing')
out['runs'].append(run('plumbing', pcfg, rsp.precompute(pcfg, W, ang, k, C.V8_FIR),
                       C.debug_v2_cfar_config(pcfg), copy, False))
line = json.dumps(out)
print(line)
if out_path:
    with open(out_path, 'w') as f:
        f.write(line + '\n')
