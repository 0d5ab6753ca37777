"""bench.py --gpus N (CPU): the launch decision and its error exits.  No GPU is touched: the
errors are raised before any HIP call, and device counting does not create a HIP context."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

import bench  # noqa: E402


@pytest.mark.parametrize('gpus,env,vis,same,backend,want', [
    (1, None, 0, False, 'nccl', 'run'),
    (1, 1, 1, False, 'nccl', 'run'),
    (8, 8, 8, False, 'nccl', 'run'),        # a torchrun rank of the driver's N = 8 run
    (2, None, 8, False, 'nccl', 'spawn'),   # bare `bench.py --gpus 2` on a node
    (2, None, 1, True, 'gloo', 'spawn'),    # rehearsal: two ranks on the one GPU
    (8, None, 1, False, 'nccl', 'error'),   # fewer visible devices than asked for
    (2, 4, 4, False, 'nccl', 'error'),      # WORLD_SIZE differs from --gpus
    (2, None, 1, True, 'nccl', 'error'),    # RCCL refuses two ranks on one device
    (0, None, 1, False, 'nccl', 'error'),
])
def test_launch_mode(gpus, env, vis, same, backend, want):
    mode, msg = bench.launch_mode(gpus, env, vis, same, backend)
    assert mode == want, msg
    assert (msg is not None) == (want == 'error')


def _run(args, **env):
    e = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        e.pop(k, None)
    e.update(env)
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, env=e, capture_output=True,
                          text=True, timeout=240)


def test_world_size_mismatch_exits_nonzero():
    r = _run(['--gpus', '2'], WORLD_SIZE='3', RANK='0', LOCAL_RANK='0')
    assert r.returncode == 2 and 'WORLD_SIZE=3' in r.stderr
    assert r.stdout == ''


def test_too_few_visible_devices_exits_nonzero():
    """This container has no GPU: --gpus 8 without --same-device must refuse, naming the count."""
    r = _run(['--gpus', '8'], HIP_VISIBLE_DEVICES='')
    assert r.returncode == 2 and '--gpus 8 but only' in r.stderr
    assert r.stdout == ''


_PROBE = r'''
import sys
sys.path.insert(0, %r)
import bench
def spawn(gpus, argv):   # stands in for torch.distributed.run: report what this process has loaded
    maps = open('/proc/self/maps').read()
    print('SPAWN', gpus, 'hip=%%d' %% ('libamdhip64' in maps), 'torch=%%d' %% ('torch' in sys.modules))
    return 0
bench.spawn_ranks = spawn
sys.argv = ['bench.py'] + sys.argv[1:]
rc = bench.main()
maps = open('/proc/self/maps').read()
print('END rc=%%d hip=%%d' %% (rc, 'libamdhip64' in maps))
'''


@pytest.mark.parametrize('args,want', [
    (['--gpus', '2', '--same-device', '--dist-backend', 'gloo'], 'SPAWN 2 hip=0 torch=0'),
    (['--gpus', '8'], 'END rc=2 hip=0'),   # counts the devices, refuses, never loads HIP
])
def test_launcher_never_loads_hip(args, want):
    """The `--gpus N` parent decides and spawns without the HIP runtime in its address space
    (no torch.cuda / amdsmi / hipGetDeviceCount): its fork/exec of torchrun can never follow a
    GPU initialisation."""
    e = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        e.pop(k, None)
    r = subprocess.run([sys.executable, '-c', _PROBE % ROOT] + args, env=e, capture_output=True, text=True,
                       timeout=120)
    assert want in r.stdout, (r.stdout, r.stderr)
    assert 'hip=1' not in r.stdout


def test_want_rdm_with_e2e_refused():
    """--want-rdm --e2e would report RD-map bytes the host queue never writes."""
    r = _run(['--want-rdm', '--e2e'])
    assert r.returncode == 2 and '--want-rdm with --e2e' in r.stderr
    assert r.stdout == ''


@pytest.mark.parametrize('args,msg', [
    (['--want-spectrum'], '--want-spectrum applies to --config music5 only'),
    (['--config', 'music5', '--want-spectrum', '--want-eig'], '--want-spectrum applies to --config music5 only'),
    (['--want-eig'], '--want-eig applies to --config music5 only'),
])
def test_music_call_forms_refused_elsewhere(args, msg):
    r = _run(args)
    assert r.returncode == 2 and msg in r.stderr
    assert r.stdout == ''


def test_visible_gpus_honours_visible_devices_env(monkeypatch):
    monkeypatch.setenv('HIP_VISIBLE_DEVICES', '')
    assert bench.visible_gpus() == 0


def test_pmc_traffic_staleness(tmp_path):
    """roofline.traffic is quoted only while the kernel's code hash equals the one the PMC file
    recorded at measurement; git_blob is the file's `git hash-object`."""
    import hashlib
    import json
    f = tmp_path / 'pmc.json'
    body = {'k2_pc': 1000, 'k1p_dbf_mtd': 2000, '_frames_per_launch': 8,
            '_kernel_hashes': {'k2_pc': 'aaaa', 'k1p_dbf_mtd': 'bbbb'}}
    f.write_text(json.dumps(body))
    raw = f.read_bytes()
    blob = hashlib.sha1(b'blob %d\0' % len(raw) + raw).hexdigest()
    tr, fpl, src = bench.pmc_traffic(str(f), ['k2_pc'], now={'k2_pc': 'aaaa'})
    assert (tr, fpl, src['fresh'], src['git_blob']) == (1000, 8, True, blob)
    tr, _, src = bench.pmc_traffic(str(f), ['k2_pc'], now={'k2_pc': 'cccc'})          # kernel rebuilt since
    assert tr is None and not src['fresh'] and 'changed' in src['stale_reason']
    tr, _, src = bench.pmc_traffic(str(f), ['k1_dbf_mtd', 'k1p_dbf_mtd'], now={'k1p_dbf_mtd': 'bbbb'})
    assert tr == 2000 and src['kernel'] == 'k1p_dbf_mtd'
    del body['_kernel_hashes']
    f.write_text(json.dumps(body))
    tr, _, src = bench.pmc_traffic(str(f), ['k2_pc'], now={'k2_pc': 'aaaa'})          # no hashes recorded
    assert tr is None and 'no kernel hash' in src['stale_reason']
    assert bench.pmc_traffic(str(tmp_path / 'missing.json'), ['k2_pc']) == (None, None, None)


def test_kernel_hashes_refuse_a_kernel_defined_twice():
    """tools/kernel_hashes.py merges the kernels of the library's code objects (one per device
    translation unit); a mangled name that two of them define is an error, not a silent overwrite."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_hashes
    a = {'_Z5k2_pcv': b'\x01', '_Z7k3_cfarv': b'\x02'}
    assert kernel_hashes.merge(dict(a), {'_Z7k_synthv': b'\x03'}) == dict(a, _Z7k_synthv=b'\x03')
    with pytest.raises(SystemExit, match='_Z5k2_pcv'):
        kernel_hashes.merge(dict(a), {'_Z5k2_pcv': b'\x01', '_Z7k_synthv': b'\x03'})


def test_music_traffic_scales_with_the_launch(tmp_path):
    """config #5's roofline traffic is the PMC file's bytes per launch scaled from the instances
    that launch held (_instances_per_launch, 1024 when absent) to the bench's --batch."""
    import json
    f = tmp_path / 'pmc_music.json'
    f.write_text(json.dumps({'k_music_cov64': 4000, '_instances_per_launch': 4096,
                             '_kernel_hashes': {'k_music_cov64': 'aaaa'}}))
    tr, src = bench.music_traffic('c128', 1024, path=str(f), now={'k_music_cov64': 'aaaa'})
    assert tr == 1000 and src['instances_per_launch_measured'] == 4096
    f.write_text(json.dumps({'k_music_cov64': 1000, '_kernel_hashes': {'k_music_cov64': 'aaaa'}}))
    tr, _ = bench.music_traffic('c128', 4096, path=str(f), now={'k_music_cov64': 'aaaa'})
    assert tr == 4000
    tr, src = bench.music_traffic('c128', 4096, path=str(f), now={'k_music_cov64': 'bbbb'})
    assert tr is None and not src['fresh']


@pytest.mark.parametrize('prec,rb', [('c128', 8), ('c64', 4)])
def test_k3_stage_bytes_match_pmc_traffic(prec, rb):
    """K3's stated bytes (bench.k3_map_bytes = rsp_internal.h k3_map_bytes: the rows under test of
    every beam's magnitude map) agree with the HBM bytes the PMC passes measured for k3_cfar at x2
    (profiles/pmc_traffic_x2_<prec>.json, 8 frames per launch) within 5 %: VERDICT r5 -- the old
    figure counted every map row, 1.30x the measured traffic."""
    import json
    from rsp import config as C
    cfg, cfar, _, _, _, _ = C.named_config('x2')
    sc = cfg['Sig_Config']
    G = sum(sc['point_prt_segments'])
    per_frame = bench.k3_map_bytes(sc['prtNum'], G, sc['beam_num'], cfar, rb)
    # 8 beams x 98 rows under test (128 - 2 x 15) x the tiled columns from cell 12: 87 tiles of 32
    # (2784 cells) in complex double, 44 tiles of 64 clipped at G = 2811 (2799 cells) in single
    assert per_frame == {8: 8 * 98 * 2784 * 8, 4: 8 * 98 * 2799 * 4}[rb]
    with open(os.path.join(ROOT, 'profiles', 'pmc_traffic_x2_%s.json' % prec)) as f:
        tj = json.load(f)
    measured = tj['k3_cfar'] / float(tj.get('_frames_per_launch', 8))
    assert abs(per_frame / measured - 1.0) < 0.05, (per_frame, measured)
    # a window other than the reference's reads whole maps
    wide = dict(cfar, refCells_R=6)
    assert bench.k3_map_bytes(sc['prtNum'], G, sc['beam_num'], wide, rb) == sc['beam_num'] * sc['prtNum'] * G * rb


def test_stage_timing_needs_full():
    """--stage-timing reports its spans in the roofline stages, which only --full builds."""
    r = _run(['--stage-timing'])
    assert r.returncode == 2 and '--stage-timing' in r.stderr and '--full' in r.stderr
    assert r.stdout == ''


def test_plain_run_defaults():
    """--full and --dump-outputs are off unless asked for."""
    a = bench.parse(['--gpus', '1', '--steps', '20', '--warmup', '5'])
    assert a.full is False and a.dump_outputs is None and (a.steps, a.warmup) == (20, 5)
    assert bench.parse(['--full', '--dump-outputs', 'd']).dump_outputs == 'd'


def test_dump_outputs_writes_float64_npy(tmp_path):
    """--dump-outputs files: one .npy per name, float64, complex as [..., 2] re/im, bounded in all."""
    import numpy as np
    d = tmp_path / 'out' / 'deeper'
    rows = np.array([[1, 2.5, -3, 0.25, 9], [1, np.nan, np.nan, np.nan, np.nan]])
    bench.dump_outputs(str(d), {'final_targets': rows, 'peaks': np.arange(6, dtype=np.int32).reshape(2, 3),
                                'rdm_sample': np.array([1 + 2j, 3 - 4j], np.complex64)})
    got = np.load(d / 'final_targets.npy')
    assert got.dtype == np.float64 and np.array_equal(got, rows, equal_nan=True)
    assert np.array_equal(np.load(d / 'peaks.npy'), np.arange(6.0).reshape(2, 3))
    assert np.array_equal(np.load(d / 'rdm_sample.npy'), [[1, 2], [3, -4]])
    assert sorted(p.name for p in d.iterdir()) == ['final_targets.npy', 'peaks.npy', 'rdm_sample.npy']
    with pytest.raises(ValueError):
        bench.dump_outputs(str(d), {'big': np.broadcast_to(np.float64(0), (bench.DUMP_MAX_BYTES // 8 + 1,))})
