"""Timing of the digital down-converter (usage: ddc_prof.py [iters] [--reps N] [--out FILE]; default FILE
profiles/ddc_prof.json).

k_ddc alone, by HIP events (rsp_profile_ddc: one warm-up launch, then `iters` launches between two events), in
complex double and complex single, with FIR.mat's 12 taps and decimation by 4 (simulation_learn.m:94-102), at
332 pulses x 23 276 samples x 16 channels (5 819 samples a pulse out) and at the reference's own line, 1 x
50 000 x 1: `reps` such measurements each (default 7), their median, smallest and largest ms, the algorithmic
bytes (input reals + output complex, in the plan's precision) and GB/s at the median, and beside each the
stream-copy probe (rsp_hbm_copy_probe) at the same byte count -- half of it read, half written -- in the same
run, with the ratio of the two rates.  The kernel reads reals of the plan's precision whatever the caller's
dtype, which the host call converts: `host_call` has the wall time of Plan.ddc (conversion, upload, kernel,
download, widening) for float32 and float64 input at the line and at one channel of the cube.  Prints one JSON
line and writes it to FILE.
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
from rsp.plan import Plan, describe_ddc  # noqa: E402
from rsp.precompute import precompute  # noqa: E402
if os.environ.get('AB_LIB'):   # timing experiments only: an A/B variant of librsp.so
    _abi.LIB_PATH = os.environ['AB_LIB']

args = sys.argv[1:]
out_path = args[args.index('--out') + 1] if '--out' in args else os.path.join(ROOT, 'profiles', 'ddc_prof.json')
reps = int(args[args.index('--reps') + 1]) if '--reps' in args else 7
iters = int(args[0]) if args and args[0].isdigit() else 50
L, D = 12, 4
SHAPES = {'cube-332x23276x16': (332, 23276, 16), 'line-1x50000': (1, 50000, 1)}
HOST_SHAPES = {'line-1x50000': (1, 50000, 1), 'cube-332x23276x1': (332, 23276, 1)}


def stream_copy_gbps(nbytes, dev=0):
    """The best of 3 probes of 20 copies that move `nbytes` in all (read + written)."""
    best = 0.0
    for _ in range(3):
        g = ct.c_double()
        if _abi.lib().rsp_hbm_copy_probe(dev, max(nbytes // 2, 1 << 20), 20, ct.byref(g)) == 0:
            best = max(best, g.value)
    return best


res = dict(iters=iters, reps=reps, L=L, D=D, kernel={}, host_call={})
for prec in ('c128', 'c64'):
    cfg, cfar, cluster, W, ang, k = C.named_config('small')   # the plan gives the device and the precision only
    plan = Plan(cfg, cfar, cluster, precompute(cfg, W, ang, k, C.V8_FIR), precision=prec)
    try:
        for name, (P, N, Cn) in SHAPES.items():
            runs = [plan.profile_ddc(P, N, Cn, L, D, iters=iters) for _ in range(reps)]
            ms = sorted(r['ms'] for r in runs)
            med, nbytes = float(np.median(ms)), runs[0]['bytes']
            gbps = nbytes / (med * 1e-3) / 1e9
            copy = stream_copy_gbps(nbytes)
            res['kernel']['%s-%s' % (name, prec)] = dict(
                P=P, N=N, C=Cn, ms=med, ms_min=ms[0], ms_max=ms[-1], ms_all=ms, bytes=nbytes, GBps=gbps,
                stream_copy_GBps=copy, frac_of_stream_copy=gbps / copy if copy else None,
                tiling=describe_ddc(P, N, Cn, L, D, 0, prec))
        h = np.ones(L) / L
        for name, (P, N, Cn) in HOST_SHAPES.items():
            for dt in (np.float32, np.float64):
                x = np.asfortranarray(np.random.default_rng(1).standard_normal((P, N, Cn)).astype(dt))
                plan.ddc(x, h, D, f0=10e6, fs=100e6)   # buffers sized
                t = []
                for _ in range(5):
                    t0 = time.perf_counter()
                    plan.ddc(x, h, D, f0=10e6, fs=100e6)
                    t.append((time.perf_counter() - t0) * 1e3)
                res['host_call']['%s-%s-%s' % (name, np.dtype(dt).name, prec)] = dict(P=P, N=N, C=Cn, wall_ms=float(np.median(t)))
    finally:
        plan.close()
line = json.dumps(res)
print(line)
with open(out_path, 'w') as f:
    f.write(line + '\n')
