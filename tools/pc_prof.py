"""Timing of the stand-alone pulse compression (usage: pc_prof.py [iters] [--reps N] [--out FILE]; default
FILE profiles/pc_prof.json).

In complex double and complex single, on the reference waveform (N = 5819 samples, G = 3404 gates, 13 beams):

  * the three launches alone, by HIP events (rsp_profile_pc: one warm-up launch, then `iters` launches
    between two events), at main_simulate_echoes_with_array_v7_7.m's 332 pulses and at 333: `reps` such
    measurements each (default 7), their median, smallest and largest ms, the algorithmic bytes and GB/s at
    the median; for k_pc_pack and k_pc_unpack, which only move data, the stream-copy probe
    (rsp_hbm_copy_probe) at the same byte count -- half of it read, half written -- in the same run, and
    the ratio of the two rates;
  * end to end from host memory to host memory at 332 pulses: Plan.pulse_compress beside Plan.process_stage2
    (PC_results and MTD_results: before this stage the only way to PC_results), wall-clock seconds, `reps`
    calls each after one warm-up call, median / smallest / largest, and whether the two PC_results are equal
    to the bit.
Prints one JSON line and writes it to FILE.
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

from rsp import _abi, config as C  # noqa: E402
from rsp.plan import Plan  # noqa: E402
from rsp.precompute import precompute  # noqa: E402
if os.environ.get('AB_LIB'):   # timing experiments only: an A/B variant of librsp.so
    _abi.LIB_PATH = os.environ['AB_LIB']

args = sys.argv[1:]
out_path = args[args.index('--out') + 1] if '--out' in args else os.path.join(ROOT, 'profiles', 'pc_prof.json')
reps = int(args[args.index('--reps') + 1]) if '--reps' in args else 7
iters = int(args[0]) if args and args[0].isdigit() else 50
PULSES = (332, 333)
B = 13


def stream_copy_gbps(nbytes, dev=0):
    """The best of 3 probes of 20 copies that move `nbytes` in all (read + written)."""
    best = 0.0
    for _ in range(3):
        g = ct.c_double()
        if _abi.lib().rsp_hbm_copy_probe(dev, max(nbytes // 2, 1 << 20), 20, ct.byref(g)) == 0:
            best = max(best, g.value)
    return best


def wall(call, n):
    call()
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        call()
        t.append(time.perf_counter() - t0)
    t.sort()
    return dict(s=float(np.median(t)), s_min=t[0], s_max=t[-1], s_all=t)


res = dict(iters=iters, reps=reps, kernel={}, end_to_end={})
cfg, cfar, cluster, W, ang, k = C.named_config('reference')
pre = precompute(cfg, W, ang, k, C.V8_FIR)
for prec in ('c128', 'c64'):
    plan = Plan(cfg, cfar, cluster, pre, precision=prec)
    try:
        for P in PULSES:
            runs = [plan.profile_pc(P, B, iters=iters) for _ in range(reps)]
            info = plan.pc_layout(P, B)
            for stage in ('k_pc_pack', 'k2_pc', 'k_pc_unpack'):
                ms = sorted(r[stage][0] for r in runs)
                med, nbytes = float(np.median(ms)), runs[0][stage][1]
                gbps = nbytes / (med * 1e-3) / 1e9
                d = dict(P=P, B=B, ms=med, ms_min=ms[0], ms_max=ms[-1], ms_all=ms, bytes=nbytes, GBps=gbps)
                if stage != 'k2_pc':
                    copy = stream_copy_gbps(nbytes)
                    d.update(stream_copy_GBps=copy, frac_of_stream_copy=gbps / copy if copy else None)
                res['kernel']['%s-P%d-%s' % (stage, P, prec)] = d
            res['kernel']['layout-P%d-%s' % (P, prec)] = info
        rng = np.random.default_rng(3)
        iq = np.asfortranarray((rng.standard_normal((plan.P, plan.N, B)) + 1j * rng.standard_normal((plan.P, plan.N, B)))
                               .astype(plan.cdtype))
        out = np.empty((plan.P, plan.G, B), np.complex128, order='F')
        # at the plan's own P and B the two give the same bits (the timed calls do the work they are timed for)
        res['end_to_end']['bit_equal-P%d-%s' % (plan.P, prec)] = bool(
            np.array_equal(plan.pulse_compress(iq, out=out), plan.process_stage2(iq)[1]))
        res['end_to_end']['pulse_compress-P%d-%s' % (plan.P, prec)] = wall(lambda: plan.pulse_compress(iq, out=out), reps)
        res['end_to_end']['process_stage2-P%d-%s' % (plan.P, prec)] = wall(lambda: plan.process_stage2(iq), reps)
    finally:
        plan.close()
line = json.dumps(res)
print(line)
with open(out_path, 'w') as f:
    f.write(line + '\n')
