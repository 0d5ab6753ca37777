"""Timing of the detector on an RD cube (usage: detect_prof.py [iters] [--reps N] [--out FILE]; default FILE
profiles/detect_prof.json).

The three device stages alone, by HIP events (rsp_profile_detect: one warm-up launch, then `iters`
launches between two events, on the library's test cube): k_pairsum on a cube in MATLAB's layout, k_xcfar
on its pair-sum maps (hits only) and k_s9 on the hits, in complex double and complex single, at
  v7_7    512 x 3404 x 13  main_simulate_echoes_with_array_v7_7.m's zero-padded cube,
  stage2  332 x 3404 x 13  the stage-2 result,
  x2      128 x 2811 x 8   the x2 configuration's RD maps,
with the reference's window 5/10/5/10 and T_CFAR = 8: `reps` such measurements each (default 7), their
median, smallest and largest ms, the algorithmic bytes and GB/s at the median; for k_pairsum and k_xcfar
the stream-copy probe (rsp_hbm_copy_probe) at the same byte count in the same run, with the ratio of the
two rates.  At x2 also K3's time per frame from rsp_profile_stages on 8 synthesised frames (one launch of 8
frames, divided by 8): the fused kernel that does the three stages' work on the frame chain.  Prints one
JSON line and writes it to FILE.
"""
import ctypes as ct
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'radar-signal-simulation-and-target-detection_amd'))

from rsp import _abi, config as C  # noqa: E402
from rsp.plan import Plan, describe_detect  # noqa: E402
from rsp.precompute import precompute  # noqa: E402
if os.environ.get('AB_LIB'):   # timing experiments only: an A/B variant of librsp.so
    _abi.LIB_PATH = os.environ['AB_LIB']

args = sys.argv[1:]
out_path = args[args.index('--out') + 1] if '--out' in args else os.path.join(ROOT, 'profiles', 'detect_prof.json')
reps = int(args[args.index('--reps') + 1]) if '--reps' in args else 7
iters = int(args[0]) if args and args[0].isdigit() else 50
SHAPES = {'v7_7': (512, 3404, 13), 'stage2': (332, 3404, 13), 'x2': (128, 2811, 8)}
CFAR = dict(refCells_R=5, guardCells_R=10, refCells_V=5, guardCells_V=10, T_CFAR=8.0)
STAGES = ('k_pairsum', 'k_xcfar', 'k_s9')


def stream_copy_gbps(nbytes, dev=0):
    """The best of 3 probes of 20 copies that move `nbytes` in all (read + written)."""
    best = 0.0
    for _ in range(3):
        g = ct.c_double()
        if _abi.lib().rsp_hbm_copy_probe(dev, max(nbytes // 2, 1 << 20), 20, ct.byref(g)) == 0:
            best = max(best, g.value)
    return best


def k3_ms_per_frame(prec):
    """K3 of the x2 plan on 8 synthesised frames per launch (rsp_profile_stages), per frame."""
    cfg, cfar, clus, W, ang, k = C.named_config('x2')
    plan = Plan(cfg, cfar, clus, precompute(cfg, W, ang, k, C.V8_FIR), frames_per_launch=8, precision=prec)
    try:
        assert (plan.P, plan.G, plan.B) == SHAPES['x2']
        cubes = [plan.device_alloc(plan.cube_bytes) for _ in range(8)]
        tg = C.v8_2_targets()
        for i, p in enumerate(cubes):
            plan.synthesize_device(p, tg, 1 + i)
            tg = C.evolve_targets(tg, cfg)
        st = plan.profile_stages(cubes, iters=iters)
        for p in cubes:
            plan.device_free(p)
        return st[2]['ms'] / st[2]['frames']
    finally:
        plan.close()


res = dict(iters=iters, reps=reps, cfar=CFAR, kernel={})
for prec in ('c128', 'c64'):
    cfg, cfar, cluster, W, ang, k = C.named_config('small')   # the plan gives the device and the precision only
    plan = Plan(cfg, cfar, cluster, precompute(cfg, W, ang, k, C.V8_FIR), precision=prec)
    try:
        for name, (V, G, B) in SHAPES.items():
            runs = [plan.profile_detect(V, G, B, CFAR, iters=iters) for _ in range(reps)]
            entry = dict(V=V, G=G, B=B, tiling=describe_detect(V, G, B, CFAR, prec), hits=runs[0]['k_s9'][1] // 48)
            for st in STAGES:
                ms = sorted(r[st][0] for r in runs)
                med, nbytes = float(np.median(ms)), runs[0][st][1]
                e = dict(ms=med, ms_min=ms[0], ms_max=ms[-1], ms_all=ms, bytes=nbytes, GBps=nbytes / (med * 1e-3) / 1e9)
                if st != 'k_s9':
                    copy = stream_copy_gbps(nbytes)
                    e.update(stream_copy_GBps=copy, frac_of_stream_copy=e['GBps'] / copy if copy else None)
                entry[st] = e
            entry['ms_total'] = sum(entry[st]['ms'] for st in STAGES)
            res['kernel']['%s-%s' % (name, prec)] = entry
    finally:
        plan.close()
    res['kernel']['x2-%s' % prec]['k3_ms_per_frame'] = k3_ms_per_frame(prec)
line = json.dumps(res)
print(line)
with open(out_path, 'w') as f:
    f.write(line + '\n')
