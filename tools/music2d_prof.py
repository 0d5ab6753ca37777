"""Stage timing of the 2-D MUSIC path at MUSIC_2D.m's size (usage: music2d_prof.py [n_inst] [iters] [what]).

Synthesises n_inst instances of the MUSIC_2D.m scene (8 x 8 array, 1000 snapshots, 91 x 181 scan
grid) on the device, runs once, then times k_music_cov64, k_music_sub64, k_music_scan2d and
k_music_peaks2d with HIP events (rsp_music_profile_2d) for the form of call `what`
(peaks | spectrum | eigenvalues) and prints one JSON line.

Flop model of the scan (residual form, per grid point and instance, N elements, M sources):
pass 1, the M projection coefficients: 8 N M; pass 2, the residual and its squared norm:
N (8 M + 4); the steering recurrence (6 flops per element and pass) is shared by the 4 instances of
a workgroup: 2 * 6 N / 4.  Share of peak: against the 78.6 TFLOP/s f64 vector peak.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'radar-signal-simulation-and-target-detection_amd'))

if os.environ.get('AB_LIB'):   # timing experiments only: an A/B variant of librsp.so
    from rsp import _abi  # noqa: E402
    _abi.LIB_PATH = os.environ['AB_LIB']
from rsp.music import MusicPlan2D, music_2d_scene  # noqa: E402

F64_VECTOR_PEAK = 78.6e12

n_inst = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
what = sys.argv[3] if len(sys.argv) > 3 else 'peaks'   # form of call timed: peaks | spectrum | eigenvalues
nx = ny = 8
K, M = 1000, 2
scene, phi, theta, dxl, dyl = music_2d_scene()
N, S = nx * ny, len(phi) * len(theta)
plan = MusicPlan2D(nx, ny, K, M, phi, theta, dxl, dyl, max_batch=n_inst)
d_X = plan.device_alloc(n_inst)
plan.synthesize_device(d_X, scene, n_inst, inst0=0, seed=20250101)
plan.process_device(d_X, n_inst, fetch=False)
pr = plan.profile(d_X, n_inst, iters=iters, what=what)
fast = plan.fast_count()
scan_flops = (8.0 * N * M + N * (8.0 * M + 4.0) + 2 * 6.0 * N / 4) * S * n_inst
cov_flops = 8.0 * N * (N + 1) / 2 * K * n_inst
total_ms = pr['cov_ms'] + pr['subspace_ms'] + pr['scan_ms'] + pr['peaks_ms']
pr.update(n_inst=n_inst, what=what, n_scan=S, fast_count=fast,
          scan_tflops=scan_flops / (pr['scan_ms'] * 1e-3) / 1e12,
          scan_frac_f64_vector_peak=scan_flops / (pr['scan_ms'] * 1e-3) / F64_VECTOR_PEAK,
          cov_tflops=cov_flops / (pr['cov_ms'] * 1e-3) / 1e12,
          inst_per_s=n_inst / (total_ms * 1e-3))
print(json.dumps(pr))
plan.device_free(d_X)
plan.close()
