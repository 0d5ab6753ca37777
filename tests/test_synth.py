"""GPU parity of k_synth (S4 echo synthesis + S4.1 Philox noise on the device, rsp_frame_aux.hip)
against _synth_ref, the point-wise numpy restatement of fsf:45-88, at the shapes of
_synth_cases.SYNTH_CASES and on the reference frame.

The device cube is the input of the parity tests of the large configurations, of the benchmark and
of the drop-in 'frame' call, so a wrong cube at their shapes passes every test that feeds the same
cube to the oracle and to the chain.  Here the cube itself is compared, at pulse counts of more
than one block of 64 pulse pairs, fast-time lengths that are no multiple of the 8-sample strip or
the 32-sample workgroup, delays on the strip and window edges, 1, 3, 5 and 32 channels, 64-bit
seeds, frame indices above 2^16 and p_noise other than 1.  Per case and precision:

  * the cube is synthesised into the middle of a buffer filled with a sentinel, with a guard band
    of GUARD bytes on either side: both bands come back untouched and no real or imaginary part of
    the cube still holds the sentinel;
  * max |device - reference| <= 1e-10 (c128) / 1e-5 (c64) of max |reference|, element by element
    (test_gpu_parity.py's tolerances for this kernel); a failure names the worst (m, n, c);
  * the c64 cube is the c128 device cube rounded to complex64: no part differs from it by more
    than one float ulp of that part (the differing parts are counted and printed).

test_synth_cases.py checks the cases' preconditions and the reference's own spread on the CPU.
"""
import numpy as np
import pytest

from rsp import _abi
from rsp.plan import Plan

import _synth_ref
from _scen import scenario, targets_for, device_cube, _route_targets, SEED
from _synth_cases import (SYNTH_CASES, PROPERTY_CASE, CHAIN_CASE, MAX_TARGETS, synth_scenario, synth_targets,
                          other_targets)

pytestmark = pytest.mark.gpu

TOL = {'c128': 1e-10, 'c64': 1e-5}   # of max |reference|
GUARD = 1 << 16                      # bytes on either side of the cube; a multiple of 256, so the cube stays aligned
WORD = np.uint32(0x7FC5A3F1)         # the sentinel: a NaN as a float, and twice over as a double
PRECS = ('c128', 'c64')
NAMES = list(SYNTH_CASES)


def _plan(s, prec):
    return Plan(s['cfg'], s['cfar'], s['clus'], s['pre_p'], precision=prec)


def _guarded_alloc(plan):
    """A device buffer of guard band, cube, guard band, every 32-bit word the sentinel."""
    total = plan.cube_bytes + 2 * GUARD
    ptr = plan.device_alloc(total)
    plan.device_upload(ptr, np.full(total // 4, WORD, np.uint32))
    return ptr


def _guarded_download(plan, ptr):
    """(low band, cube, high band) of a _guarded_alloc buffer as 32-bit words."""
    w = plan.device_download(ptr, (plan.cube_bytes + 2 * GUARD) // 4, np.uint32)
    g = GUARD // 4
    return w[:g], w[g:-g], w[-g:]


def _cube(plan, words):
    """The words of a device cube as raw[m, n, c] in the plan's precision."""
    return words.view(plan.cdtype).reshape((plan.P, plan.N, plan.C), order='F')


def _synth(plan, tg, frame_idx, seed, p_noise, ptr=None):
    """(low band, cube words, high band) after one synthesis into a fresh sentinel-filled buffer, or
    into the cube of the buffer ``ptr``, which the caller frees."""
    own = ptr is None
    if own:
        ptr = _guarded_alloc(plan)
    try:
        plan.synthesize_device(ptr + GUARD, tg, frame_idx=frame_idx, seed=seed, p_noise=p_noise)
        return _guarded_download(plan, ptr)
    finally:
        if own:
            plan.device_free(ptr)


def _untouched(band):
    return bool((band == WORD).all())


def _sentinel_parts(words, prec):
    """How many real or imaginary parts of a cube still hold the sentinel."""
    if prec == 'c64':
        return int((words == WORD).sum())
    both = (np.uint64(WORD) << np.uint64(32)) | np.uint64(WORD)
    return int((words.view(np.uint64) == both).sum())


def _assert_close(dev, ref, prec, what):
    """max |dev - ref| <= TOL max |ref| over arrays indexed like the cube; prints the figure and, on
    failure, names the worst element."""
    d = np.abs(dev.astype(np.complex128) - ref)
    i = np.unravel_index(np.argmax(d), d.shape)   # a NaN (the sentinel) counts as the largest
    scale = np.abs(ref).max()
    print('%s %s: max |delta| %.3g of max |ref| at %r' % (what, prec, d[i] / scale, tuple(int(x) for x in i)))
    assert d[i] <= TOL[prec] * scale, \
        '%s %s: worst element (m, n, c) = %r: device %r, reference %r, |delta| = %.3g of max |ref| > %g' % (
            what, prec, tuple(int(x) for x in i), dev[i], ref[i], d[i] / scale, TOL[prec])


@pytest.fixture(scope='module', params=NAMES)
def case(request):
    """A case's reference cube (computed once, left unchanged) and the downloaded buffers of both precisions."""
    name = request.param
    sy = SYNTH_CASES[name]
    s = synth_scenario(name)
    tg = synth_targets(name, s['cfg'])
    args = (sy['frame_idx'], sy['seed'], sy['p_noise'])
    ref = _synth_ref.cube(tg, s['cfg'], s['pre_o'], *args)
    ref.setflags(write=False)
    runs = {}
    for prec in PRECS:
        plan = _plan(s, prec)
        try:
            assert (plan.P, plan.N, plan.C) == ref.shape
            lo, words, hi = _synth(plan, tg, *args)
            runs[prec] = dict(lo=lo, hi=hi, words=words, cube=_cube(plan, words))
        finally:
            plan.close()
    return dict(name=name, sy=sy, ref=ref, runs=runs)


@pytest.mark.parametrize('prec', PRECS)
def test_guard_bands_untouched(case, prec):
    lo, hi = case['runs'][prec]['lo'], case['runs'][prec]['hi']
    assert lo.nbytes == hi.nbytes == GUARD >= 4096 and GUARD % 256 == 0
    assert _untouched(lo), 'a store below the cube: words %r' % (np.flatnonzero(lo != WORD)[:8],)
    assert _untouched(hi), 'a store above the cube: words %r' % (np.flatnonzero(hi != WORD)[:8],)


@pytest.mark.parametrize('prec', PRECS)
def test_every_element_written(case, prec):
    run = case['runs'][prec]
    assert run['cube'].shape == case['ref'].shape
    left = _sentinel_parts(run['words'], prec)
    assert left == 0, '%d real / imaginary parts still hold the sentinel' % left
    assert np.isfinite(run['words'].view(np.float64 if prec == 'c128' else np.float32)).all()


@pytest.mark.parametrize('prec', PRECS)
def test_cube_matches_reference(case, prec):
    _assert_close(case['runs'][prec]['cube'], case['ref'], prec, case['name'])


def test_c64_cube_is_the_rounded_c128_cube(case):
    """The two instantiations do the same double arithmetic and differ in the final conversion alone."""
    a = case['runs']['c64']['words'].view(np.float32)
    b = case['runs']['c128']['words'].view(np.float64).astype(np.float32)
    diff = np.abs(a.astype(np.float64) - b.astype(np.float64))
    outside = diff > np.spacing(np.abs(b)).astype(np.float64)
    print('%s: %d of %d parts differ from the rounded c128 cube, %d by more than one ulp'
          % (case['name'], int((a != b).sum()), a.size, int(outside.sum())))
    P, N, _ = case['ref'].shape
    where = [((i // 2) % P, (i // 2) // P % N, (i // 2) // (P * N), 'im' if i % 2 else 're')
             for i in np.flatnonzero(outside)[:10]]
    assert not outside.any(), '%d parts outside one float ulp, first at (m, n, c, part) %r' % (outside.sum(), where)


# ---- properties, on the case with a second pulse block and a 5-sample last wave ----------------
@pytest.fixture(scope='module', params=PRECS)
def prop(request):
    s = synth_scenario(PROPERTY_CASE)
    plan = _plan(s, request.param)
    yield dict(prec=request.param, s=s, sy=SYNTH_CASES[PROPERTY_CASE], plan=plan, tg=synth_targets(PROPERTY_CASE, s['cfg']))
    plan.close()


def test_p_noise_scales_the_whole_cube(prop):
    """p_noise = 4 doubles the echo (rsp_synth_targets' amplitude, fsf:62-63) and the noise (fsf:86)."""
    plan, sy = prop['plan'], prop['sy']
    one = _cube(plan, _synth(plan, prop['tg'], sy['frame_idx'], sy['seed'], 1.0)[1])
    four = _cube(plan, _synth(plan, prop['tg'], sy['frame_idx'], sy['seed'], 4.0)[1])
    _assert_close(four, 2 * one.astype(np.complex128), prop['prec'], 'p_noise 4 against twice p_noise 1')
    quarter = _cube(plan, _synth(plan, prop['tg'], sy['frame_idx'], sy['seed'], 0.25)[1])
    _assert_close(quarter, 0.5 * one.astype(np.complex128), prop['prec'], 'p_noise 1/4 against half p_noise 1')


def test_frame_index_and_seed_high_word_reach_the_generator(prop):
    plan, sy = prop['plan'], prop['sy']
    f, seed = sy['frame_idx'], sy['seed']
    base = _cube(plan, _synth(plan, prop['tg'], f, seed, 1.0)[1])
    for what, args in (('frame_idx + 1', (f + 1, seed)), ('seed + 2**32', (f, seed + 2 ** 32))):
        other = _cube(plan, _synth(plan, prop['tg'], args[0], args[1], 1.0)[1])
        assert np.abs(other - base).max() > 1, what


def test_second_synthesis_leaves_nothing_of_the_first(prop):
    """Other, fewer targets into the same buffer: the shared phasor table is rewritten in stream
    order, its stale rows past the new count are not read, and every element is overwritten."""
    plan, sy, s = prop['plan'], prop['sy'], prop['s']
    tg2 = other_targets(s['cfg'])
    args = (sy['frame_idx'] + 7, sy['seed'], sy['p_noise'])
    ptr = _guarded_alloc(plan)
    try:
        _synth(plan, prop['tg'], sy['frame_idx'], sy['seed'], sy['p_noise'], ptr=ptr)
        lo, again, hi = _synth(plan, tg2, *args, ptr=ptr)
    finally:
        plan.device_free(ptr)
    assert _untouched(lo) and _untouched(hi)
    fresh = _synth(plan, tg2, *args)[1]
    assert np.array_equal(again, fresh)
    _assert_close(_cube(plan, again), _synth_ref.cube(tg2, s['cfg'], s['pre_o'], *args), prop['prec'], 'second synthesis')


def test_one_target_too_many_is_refused_before_anything_is_written(prop):
    plan, sy = prop['plan'], prop['sy']
    tg = (prop['tg'] * 3)[:MAX_TARGETS + 1]
    assert len(tg) == 65
    ptr = _guarded_alloc(plan)
    try:
        with pytest.raises(_abi.RspError) as e:
            plan.synthesize_device(ptr + GUARD, tg, frame_idx=sy['frame_idx'], seed=sy['seed'])
        assert e.value.code == _abi.RSP_ERR_INVALID
        plan.sync()
        assert all(_untouched(part) for part in _guarded_download(plan, ptr))
        # and the cap itself is taken
        plan.synthesize_device(ptr + GUARD, tg[:MAX_TARGETS], frame_idx=sy['frame_idx'], seed=sy['seed'])
        lo, cube, hi = _guarded_download(plan, ptr)
        assert _untouched(lo) and _untouched(hi) and _sentinel_parts(cube, prop['prec']) == 0
    finally:
        plan.device_free(ptr)


# ---- the 'frame' call ------------------------------------------------------------------------------
def test_process_targets_is_process_cube_of_the_device_cube():
    """rsp_process_targets runs the synthesis and the chain on one stream; the same kernels on the
    downloaded and re-uploaded cube give the same bits, so every field of every detection and
    final target is identical, at a 64-bit seed and p_noise = 4."""
    sy = SYNTH_CASES[CHAIN_CASE]
    s = synth_scenario(CHAIN_CASE)
    tg = _route_targets(s['cfg'], s['ang'])
    seed = (0xABCD << 32) | 17
    plan = _plan(s, 'c128')
    try:
        a = plan.process_targets(tg, frame_idx=sy['frame_idx'], seed=seed, p_noise=sy['p_noise'])
        cube = device_cube(plan, tg, frame_idx=sy['frame_idx'], seed=seed, p_noise=sy['p_noise'])
        b = plan.process_cube(cube, frame_idx=sy['frame_idx'])
    finally:
        plan.close()
    print('%d detections, %d final targets' % (len(a['detections']), len(a['final_targets'])))
    assert len(a['detections']) > 0 and len(a['final_targets']) > 0
    assert a['detections'] == b['detections']
    assert a['final_targets'] == b['final_targets']


# ---- the reference frame, at sampled rows ------------------------------------------------------------
def test_reference_frame_rows_match_reference():
    """The cube test_gpu_parity.py and test_config3.py take from the device (16C x 5819N x 332P,
    frame 1, the default seed): 166 pulse pairs = 2 * 64 + 38 and N = 181 * 32 + 27 together.  Rows
    (n, c) of P pulses are downloaded at their offsets and compared with _synth_ref's row form --
    no 495 MB download and no full numpy synthesis."""
    s = scenario('reference')
    tg = targets_for('reference')
    sc = s['cfg']['Sig_Config']
    P, N, C_ = sc['prtNum'], sc['point_PRT'], sc['channel_num']
    assert (P, N, C_) == (332, 5819, 16)
    rng = np.random.default_rng(5819)
    rows = [(n, c) for n in (0, N - 1) for c in range(C_)]                            # the window's ends, every channel
    rows += [(n, c) for n in (5792, 5799, 5800, 5815, 5816, N - 1) for c in (0, 7, 15)]   # the last workgroup's strips
    delays = [_synth_ref.sample_delay(t, s['cfg']) for t in tg]
    assert all(1 < d < N - 1 for d in delays)
    rows += [(d + k, c) for d in delays for k in (-1, 0, 1) for c in (0, 5, 15)]     # each target's first sample
    rows += list(zip(rng.integers(0, N, 200), rng.integers(0, C_, 200)))
    n, c = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    plan = _plan(s, 'c128')
    try:
        assert (plan.P, plan.N, plan.C) == (P, N, C_)
        ptr = plan.device_alloc(plan.cube_bytes)
        try:
            plan.synthesize_device(ptr, tg, frame_idx=1, seed=SEED)
            dev = np.stack([plan.device_download(ptr + 16 * (int(ci) * N + int(ni)) * P, P, np.complex128)
                            for ni, ci in zip(n, c)])
        finally:
            plan.device_free(ptr)
    finally:
        plan.close()
    ref = _synth_ref.rows(tg, s['cfg'], s['pre_o'], n, c, 1, SEED)
    d = np.abs(dev - ref)
    i = np.unravel_index(np.argmax(d), d.shape)
    scale = np.abs(ref).max()
    print('reference frame, %d rows: max |delta| %.3g of max |ref|' % (n.size, d[i] / scale))
    assert d[i] <= TOL['c128'] * scale, 'worst element (m, n, c) = %r: device %r, reference %r' % (
        (int(i[1]), int(n[i[0]]), int(c[i[0]])), dev[i], ref[i])
