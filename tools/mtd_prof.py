"""Timing of the stand-alone MTD (usage: mtd_prof.py [iters] [--reps N] [--out FILE]; default FILE
profiles/mtd_prof.json).

k_mtd_any alone, by HIP events (rsp_profile_mtd: one warm-up launch, then `iters` launches between two
events), in complex double and complex single, at the reference stage-2 shape 332 pulses x 3404 gates x 13
beams with nfft = 332 (chirp-z, M = 1024) and nfft = 512 (main_simulate_echoes_with_array_v7_7.m's
FFTnum_MTD), and at 256 -> 256: `reps` such measurements each (default 7), their median, smallest and
largest ms, the algorithmic bytes (element bytes x G n_maps x (P + nfft)) and GB/s at the median, and
beside each the stream-copy probe (rsp_hbm_copy_probe) at the same byte count -- half of it read, half
written -- in the same run, with the ratio of the two rates.  `butterfly_factor` is the chirp-z route's
2 M log2 M / (nfft log2 nfft), its butterflies over a native transform's.  Prints one JSON line and writes
it to FILE.
"""
import ctypes as ct
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'radar-signal-simulation-and-target-detection_amd'))

from rsp import _abi, config as C  # noqa: E402
from rsp.plan import Plan, describe_mtd  # noqa: E402
from rsp.precompute import precompute  # noqa: E402
if os.environ.get('AB_LIB'):   # timing experiments only: an A/B variant of librsp.so
    _abi.LIB_PATH = os.environ['AB_LIB']

args = sys.argv[1:]
out_path = args[args.index('--out') + 1] if '--out' in args else os.path.join(ROOT, 'profiles', 'mtd_prof.json')
reps = int(args[args.index('--reps') + 1]) if '--reps' in args else 7
iters = int(args[0]) if args and args[0].isdigit() else 100
SHAPES = {'reference-332': (332, 3404, 13, 332), 'reference-512': (332, 3404, 13, 512), 'p256': (256, 3404, 13, 256)}


def stream_copy_gbps(nbytes, dev=0):
    """The best of 3 probes of 20 copies that move `nbytes` in all (read + written)."""
    best = 0.0
    for _ in range(3):
        g = ct.c_double()
        if _abi.lib().rsp_hbm_copy_probe(dev, max(nbytes // 2, 1 << 20), 20, ct.byref(g)) == 0:
            best = max(best, g.value)
    return best


res = dict(iters=iters, reps=reps, kernel={})
for prec in ('c128', 'c64'):
    cfg, cfar, cluster, W, ang, k = C.named_config('small')   # the plan gives the device and the precision only
    plan = Plan(cfg, cfar, cluster, precompute(cfg, W, ang, k, C.V8_FIR), precision=prec)
    try:
        for name, (P, G, n_maps, nfft) in SHAPES.items():
            runs = [plan.profile_mtd(P, G, n_maps, nfft, iters=iters) for _ in range(reps)]
            ms = sorted(r['ms'] for r in runs)
            med, nbytes = float(np.median(ms)), runs[0]['bytes']
            gbps = nbytes / (med * 1e-3) / 1e9
            copy = stream_copy_gbps(nbytes)
            info = describe_mtd(P, G, nfft, prec)
            M = info['M']
            res['kernel']['%s-%s' % (name, prec)] = dict(
                P=P, G=G, n_maps=n_maps, nfft=nfft, ms=med, ms_min=ms[0], ms_max=ms[-1], ms_all=ms, bytes=nbytes, GBps=gbps,
                stream_copy_GBps=copy, frac_of_stream_copy=gbps / copy if copy else None,
                butterfly_factor=2 * M * math.log2(M) / (nfft * math.log2(nfft)) if info['route'] == 'chirpz' else 1.0,
                tiling=info)
    finally:
        plan.close()
line = json.dumps(res)
print(line)
with open(out_path, 'w') as f:
    f.write(line + '\n')
