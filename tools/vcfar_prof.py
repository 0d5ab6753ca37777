"""Timing of the Doppler CA-CFAR of the stage-2 path (usage: vcfar_prof.py [iters] [--no-baseline]
[--out FILE]; default FILE profiles/vcfar_prof.json).

At the reference frame (debug_simulated_data_processing_v3.m's config: 13 beams, 332 x 3404 maps), on
complex Gaussian noise beams, with the window of main_simulate_echoes_with_array_v3.m:30-35 (4 / 6,
T = 6): one fused call (rsp_process_stage2_vcfar) leaves the MTD result on the device, then k_vcfar
is timed alone with HIP events (rsp_profile_vcfar) in its three forms -- real amplitudes in, flags
and thresholds out (`real`); the stage-2 result in, amplitudes, flags and thresholds out
(`fused_all`); the stage-2 result in, the hit list alone (`fused_hits`) -- and, in the same run, the
stream-copy probe and the sibling kernel k_s3_cfar (rsp_profile_stage3, the debug script's window),
which moves the same algorithmic bytes per form.  Per form: ms, bytes, GB/s, the fraction of the
stream-copy rate and the time ratio to the sibling form.

Unless --no-baseline, also one wall-clock run each of what a user of the stage-2 path had to do
before (`Plan.process_stage2`, |.| on the host and the numpy restatement tests/_vcfar_ref.py on the
downloaded map) and of the fused call with only the hit list requested.  Prints one JSON line and
writes it to FILE.
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
from rsp.plan import Plan, describe_vcfar  # noqa: E402

args = sys.argv[1:]
out_path = args[args.index('--out') + 1] if '--out' in args else os.path.join(ROOT, 'profiles', 'vcfar_prof.json')
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


def forms(prof, copy_gbps, sibling=None):
    out = {}
    for form, (ms, nbytes) in prof.items():
        gbps = nbytes / (ms * 1e-3) / 1e9
        out[form] = dict(ms=ms, bytes=nbytes, GBps=gbps, frac_of_stream_copy=gbps / copy_gbps if copy_gbps else None)
        if sibling:
            out[form]['time_ratio_to_s3'] = ms / sibling[form]['ms']
    return out


copy = stream_copy_gbps()
cfg = C.stage2_config(C.debug_v3_config())
cfar = C.v3_cfar_params()
s3_cfar = C.debug_v2_cfar_config(C.debug_v3_config())
plan = Plan(cfg, C.default_cfar_params(), C.default_cluster_params(), rsp._stage2_precompute(cfg))
tile = describe_vcfar(plan.P, plan.G, cfar)
res = dict(iters=iters, stream_copy_GBps=copy, config='reference', P=plan.P, G=plan.G, B=plan.B, tile=tile,
           halo_reread_factor=(tile['rows'] + 2 * tile['halo']) / tile['rows'],
           cfar={k: cfar[k] for k in ('refCells_V', 'guardCells_V', 'T_CFAR')})
try:
    iq = noise_beams(plan.P, plan.N, plan.B)
    t0 = time.perf_counter()
    first = plan.process_stage2_vcfar(iq, cfar, want=('hits',))
    t1 = time.perf_counter()
    res['n_hits'] = first['n_hits']
    res['k_s3_cfar'] = forms(plan.profile_stage3(s3_cfar, iters=iters), copy)
    for method in ('ca', 'goca', 'soca'):
        res['k_vcfar_' + method] = forms(plan.profile_vcfar(cfar, method=method, iters=iters), copy, res['k_s3_cfar'])
    if baseline:
        import _vcfar_ref as ref
        t2 = time.perf_counter()
        hits = plan.process_stage2_vcfar(iq, cfar, want=('hits',))
        t3 = time.perf_counter()
        mtd, _ = plan.process_stage2(iq)
        t4 = time.perf_counter()
        flags, _ = ref.local_cfar_detector(np.abs(mtd), cfar, ref.CA)
        t5 = time.perf_counter()
        res['baseline'] = dict(process_stage2_s=t4 - t3, host_abs_and_numpy_cfar_s=t5 - t4, total_s=t5 - t3,
                               n_hits=int(flags.sum()))
        res['fused_hits_only_call'] = dict(first_call_s=t1 - t0, call_s=t3 - t2, n_hits=hits['n_hits'],
                                           speedup_vs_baseline=(t5 - t3) / (t3 - t2))
finally:
    plan.close()
line = json.dumps(res)
print(line)
with open(out_path, 'w') as f:
    f.write(line + '\n')
