"""Timing of the stage-1 DBF of the stage-2 path (usage: dbf_prof.py [iters] [--no-wall] [--out FILE];
default FILE profiles/dbf_prof.json).

k_dbf alone, by HIP events (rsp_profile_dbf), in complex double and complex single, at the raw frame
of the stage-2 scripts (16 channels x 13 beams x 3486 samples x 332 pulses) and at x2's shape (16 x 8 x
4096 x 128): ms, algorithmic bytes (element bytes x P N x (C + B)), GB/s, and beside each the
stream-copy probe (rsp_hbm_copy_probe) at the same byte count -- half of it read, half written -- in
the same run, with the ratio of the two rates.

Unless --no-wall, also the wall time of one call of `Plan.process_raw_stage2(cube)` beside
`Plan.process_stage2(Plan.dbf(cube, W))` on plans of the `reference` and `x2` configurations (complex
double, a noise cube; the median of 5 rounds in which the routes alternate, after one round that is
dropped for its buffer growth), and whether the two routes returned the same bits.  Prints one JSON line and writes it to FILE.
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
from rsp.plan import Plan, describe_dbf  # noqa: E402
from rsp.precompute import precompute  # noqa: E402
if os.environ.get('AB_LIB'):   # timing experiments only: an A/B variant of librsp.so
    _abi.LIB_PATH = os.environ['AB_LIB']

args = sys.argv[1:]
out_path = args[args.index('--out') + 1] if '--out' in args else os.path.join(ROOT, 'profiles', 'dbf_prof.json')
wall = '--no-wall' not in args
iters = int(args[0]) if args and args[0].isdigit() else 200
WALL_REPS = 5
SHAPES = {'reference': (332, 3486, 16, 13), 'x2': (128, 4096, 16, 8)}   # (P, N, C, B)


def stream_copy_gbps(nbytes, dev=0):
    """The best of 3 probes of 20 copies that move `nbytes` in all (read + written)."""
    best = 0.0
    for _ in range(3):
        g = ct.c_double()
        if _abi.lib().rsp_hbm_copy_probe(dev, max(nbytes // 2, 1 << 20), 20, ct.byref(g)) == 0:
            best = max(best, g.value)
    return best


def named_plan(name, precision):
    cfg, cfar, cluster, W, ang, k = C.named_config(name)
    return Plan(cfg, cfar, cluster, precompute(cfg, W, ang, k, C.V8_FIR), precision=precision), np.asarray(W, complex)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


res = dict(iters=iters, kernel={}, wall={})
for prec in ('c128', 'c64'):
    plan, _ = named_plan('small', prec)   # the plan gives the device and the precision only
    try:
        for name, (P, N, Cn, B) in SHAPES.items():
            r = plan.profile_dbf(P, N, Cn, B, iters=iters)
            gbps = r['bytes'] / (r['ms'] * 1e-3) / 1e9
            copy = stream_copy_gbps(r['bytes'])
            res['kernel']['%s-%s' % (name, prec)] = dict(
                P=P, N=N, C=Cn, B=B, ms=r['ms'], bytes=r['bytes'], GBps=gbps, stream_copy_GBps=copy,
                frac_of_stream_copy=gbps / copy if copy else None, tiling=describe_dbf(P, N, Cn, B, prec))
    finally:
        plan.close()
if wall:
    for name in ('reference', 'x2'):
        plan, W = named_plan(name, 'c128')
        try:
            rng = np.random.default_rng(20250101)
            shp = (plan.P, plan.N, plan.C)
            cube = np.asfortranarray((rng.standard_normal(shp) + 1j * rng.standard_normal(shp)) / np.sqrt(2.0))
            t = dict(raw=[], dbf=[], s2=[])
            for rep in range(WALL_REPS + 1):   # the routes alternate; the first round (buffer growth) is dropped
                t_raw, raw = timed(lambda: plan.process_raw_stage2(cube))
                t_dbf, beams = timed(lambda: plan.dbf(cube, W))
                t_s2, two = timed(lambda: plan.process_stage2(beams))
                if rep:
                    t['raw'].append(t_raw), t['dbf'].append(t_dbf), t['s2'].append(t_s2)
            both = [a + b for a, b in zip(t['dbf'], t['s2'])]
            med = {k: float(np.median(v)) for k, v in dict(t, both=both).items()}
            res['wall'][name] = dict(P=plan.P, N=plan.N, C=plan.C, B=plan.B, reps=WALL_REPS,
                                     process_raw_stage2_s=med['raw'], dbf_s=med['dbf'], process_stage2_s=med['s2'],
                                     dbf_plus_process_stage2_s=med['both'], raw_over_two_calls=med['raw'] / med['both'],
                                     process_raw_stage2_all_s=t['raw'], dbf_plus_process_stage2_all_s=both,
                                     same_bits=bool(np.array_equal(raw[0], two[0]) and np.array_equal(raw[1], two[1])))
        finally:
            plan.close()
line = json.dumps(res)
print(line)
with open(out_path, 'w') as f:
    f.write(line + '\n')
