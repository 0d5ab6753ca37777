"""The stand-alone pulse compression on the device (k_pc_pack, k2_pc on a record table of its own, k_pc_unpack:
Plan.pulse_compress, pulse_compress_device, pc_mtd_detect, raw_detect, rsp.pulse_compress).

1. To the bit against the plan: at a case's own P and B, Plan.pulse_compress equals Plan.process_stage2's
   PC_results.  The k2_pc code and the rounding of the input are the same and K1 mode 0 only transposes
   (tests/test_k2_parity.py relies on the same fact), so a mismatch is a pack or unpack bug, never tolerance.
2. Row independence, to the bit: a sub-cube's result is the sub-cube of the result, which pins odd P against
   even P, one pack tile against two and a short last tile against a full one without a tolerance.
3. Against the oracle at pulse counts no plan takes, with test_k2_parity.py's per-segment, per-block metric and
   _parity.MAP_TOL, the project's own figure for k2_pc.
4. The device form between canaries, and (P, B) changing between calls.
5. The compositions equal the calls they are made of, to the bit.
6. Refusals, and the plan's other calls before and after.
tests/_pc_cases.py holds the table, test_pc_cases.py proves the paths it reaches.
"""
import ctypes as ct

import numpy as np
import pytest

import _detect_cases as dc
import _pc_cases as pcc
import rsp
from rsp import _abi, config as C
from rsp.plan import Plan
from rsp.precompute import precompute as product_precompute
from oracle import chain
from _parity import MAP_TOL
from _scen import plumbing_weights

pytestmark = pytest.mark.gpu

FIELDS = ('v_idx', 'r_idx', 'pair_idx', 'amp', 'Range', 'Velocity', 'Angle')
WORD = np.uint32(0x7FC5A3F1)   # a NaN as a float, and twice over as a double
GUARD = 1 << 12


def make_plan(name, prec):
    s = pcc.pc_scenario(name)
    return s, Plan(s['cfg'], s['cfar'], s['clus'], s['pre_p'], precision=prec)


@pytest.fixture(scope='module')
def bases():
    """Per precision, the plan of the oracle case (P = 16, B = 3 of its own: neither plays a part), its layout
    and the scenario with the oracle's precomputed data."""
    out = {}
    for prec in pcc.PRECS:
        s, p = make_plan(pcc.ORACLE_CASE, prec)
        out[prec] = dict(s=s, plan=p, prec=prec, L=p.k2_layout())
    yield out
    for b in out.values():
        b['plan'].close()


@pytest.fixture(params=pcc.PRECS)
def base(request, bases):
    return bases[request.param]


def _same_lists(a, b):
    assert len(a['detections']) == len(b['detections'])
    for x, y in zip(a['detections'], b['detections']):
        for f in FIELDS:
            assert x[f] == y[f], (f, x, y)
    assert a['final_targets'] == b['final_targets']


# ---- 1. to the bit against the plan ---------------------------------------------------------------------
@pytest.mark.parametrize('prec', pcc.PRECS)
@pytest.mark.parametrize('name', pcc.BIT_CASES + ('pc-g511', 'pc-g513'))
def test_bit_identity_with_process_stage2(name, prec):
    s, p = make_plan(name, prec)
    try:
        iq = pcc.beams(s, p.P, p.B, prec)
        want = p.process_stage2(iq)[1]
        got = p.pulse_compress(iq)
        info = p.pc_layout(p.P, p.B)
        again = p.process_stage2(iq)[1]
    finally:
        p.close()
    print(name, prec, info)
    assert info == rsp.describe_pc(s['cfg'], s['cfar'], s['clus'], s['pre_p'], 16, 3, precision=prec)
    assert np.abs(want).max() > 0
    assert np.array_equal(got, want), 'first mismatch at %r' % (np.argwhere(got != want)[:4].tolist(),)
    assert np.array_equal(again, want)


# ---- 2. row independence ------------------------------------------------------------------------------------
@pytest.mark.parametrize('P, sub', [(16, 7), (130, 65), (257, 255), (257, 256), (513, 511), (513, 512)])
def test_a_sub_cube_gives_the_sub_cube_of_the_result(base, P, sub):
    p = base['plan']
    iq = pcc.beams(base['s'], P, 3, base['prec'])
    full = p.pulse_compress(iq)
    assert np.array_equal(p.pulse_compress(iq[:sub]), full[:sub])
    assert np.array_equal(p.pulse_compress(iq[:, :, :1]), full[:, :, :1])
    assert np.array_equal(p.pulse_compress(iq[sub:, :, 1:]), full[sub:, :, 1:])


# ---- 3. the oracle at pulse counts no plan takes -----------------------------------------------------------------
def _oracle_check(base, P, B):
    iq = pcc.beams(base['s'], P, B, base['prec'], seed=100 + P + B)
    got = base['plan'].pulse_compress(iq)
    want = chain.pulse_compress(iq, base['s']['pre_o'])
    assert got.shape == want.shape == (P, base['plan'].G, B)
    pcc.blocks_close(got, want, base['L'], MAP_TOL[base['prec']], 'PCRATIO %s P=%d B=%d' % (base['prec'], P, B))


@pytest.mark.parametrize('prec, P', [(prec, P) for prec in pcc.PRECS for P in pcc.ORACLE_P if P != 333 or prec == 'c128'])
def test_oracle_parity_over_pulse_counts(bases, prec, P):
    _oracle_check(bases[prec], P, 3)


@pytest.mark.parametrize('B', pcc.ORACLE_B)
def test_oracle_parity_over_beam_counts(base, B):
    _oracle_check(base, 7, B)


@pytest.mark.parametrize('prec', pcc.PRECS)
@pytest.mark.parametrize('name', pcc.G_EDGE_CASES)
def test_oracle_parity_at_the_gate_tile_edges(name, prec):
    """G one below, on and one above a multiple of the unpack tile's width, at an odd P."""
    s, p = make_plan(name, prec)
    try:
        iq = pcc.beams(s, 21, 3, prec)
        got = p.pulse_compress(iq)
        L = p.k2_layout()
    finally:
        p.close()
    pcc.blocks_close(got, chain.pulse_compress(iq, s['pre_o']), L, MAP_TOL[prec], 'PCRATIO %s %s' % (name, prec))


# ---- 4. the device form -------------------------------------------------------------------------------------------
def _device_pc(p, iq):
    """pulse_compress_device of iq between canaries: (result [P, G, B] as complex128, the words before, after)."""
    P, N, B = iq.shape
    x = np.asfortranarray(iq).astype(p.cdtype)
    esz = x.dtype.itemsize
    nout = P * p.G * B
    total = (2 * GUARD + nout * esz) // 4
    d_in, d_out = p.device_alloc(x.size * esz), p.device_alloc(total * 4)
    try:
        p.device_upload(d_in, x.ravel(order='F'))
        p.device_upload(d_out, np.full(total, WORD, np.uint32))
        p.pulse_compress_device(d_in, d_out + GUARD, P, B)
        words = p.device_download(d_out, total, np.uint32)
        back = p.device_download(d_in, x.size, p.cdtype)
    finally:
        p.device_free(d_in)
        p.device_free(d_out)
    assert np.array_equal(back, x.ravel(order='F')), 'the beams were written'
    body = words[GUARD // 4:GUARD // 4 + nout * esz // 4].view(p.cdtype)
    return body.reshape((P, p.G, B), order='F').astype(np.complex128), words[:GUARD // 4], words[-(GUARD // 4):]


def test_device_form_between_canaries_and_changing_sizes(base):
    p = base['plan']
    a, b = pcc.beams(base['s'], 16, 3, base['prec'], seed=1), pcc.beams(base['s'], 7, 1, base['prec'], seed=2)
    want_a, want_b = p.pulse_compress(a), p.pulse_compress(b)
    assert p.pc_layout(7, 1)['k2_wg'] != p.pc_layout(16, 3)['k2_wg']
    for iq, want in ((a, want_a), (b, want_b), (a, want_a)):   # 16 x 3 -> 7 x 1 -> 16 x 3: record tables rebuilt, scratch kept
        got, lo, hi = _device_pc(p, iq)
        assert (lo == WORD).all() and (hi == WORD).all(), 'written outside the P G B output elements'
        assert np.array_equal(got, want)
        assert np.array_equal(p.pulse_compress(iq), want)
    odd = pcc.beams(base['s'], 65, 3, base['prec'], seed=3)    # odd P: columns off 16 bytes in complex single
    got, lo, hi = _device_pc(p, odd)
    assert (lo == WORD).all() and (hi == WORD).all()
    assert np.array_equal(got, p.pulse_compress(odd))


def test_profile_pc(base):
    p = base['plan']
    r = p.profile_pc(65, 3, iters=2)
    d = p.pc_layout(65, 3)
    esz = 16 if base['prec'] == 'c128' else 8
    assert all(r[k][0] > 0 for k in ('k_pc_pack', 'k2_pc', 'k_pc_unpack'))
    assert r['k_pc_pack'][1] == esz * (65 * d['nU'] * 3 + d['z_elems'])
    assert r['k_pc_unpack'][1] == 2 * esz * 65 * d['G'] * 3


# ---- 5. compositions ------------------------------------------------------------------------------------------------
def _chain_args(G, B, nfft):
    ax = dc.axes(nfft, G, B)
    return (pcc.CHAIN_CFAR, dc.CLUSTER, ax['range_axis'], ax['velocity_axis'], ax['deltaR'], ax['deltaV'], ax['beam_angles_deg'],
            ax['k_slopes_LUT']), ax


@pytest.mark.parametrize('P, nfft', [(21, 32), (16, 16)])
def test_pc_mtd_detect_equals_its_parts(base, P, nfft):
    p = base['plan']
    raw, W = pcc.echo_cube(base['s'], P, base['prec'])
    iq, win = p.dbf(raw, W), np.kaiser(P, 4.0)
    args, ax = _chain_args(p.G, 3, nfft)
    one = p.pc_mtd_detect(iq, win, nfft, *args, want_rdm=True, want_cfar=True)
    two = p.mtd_detect(p.pulse_compress(iq), win, nfft, *args, want_rdm=True, want_cfar=True)
    print('pc_mtd_detect', base['prec'], P, nfft, '%d detections, %d targets' % (len(one['detections']), len(one['final_targets'])))
    assert len(one['detections']) > 0 and len(one['final_targets']) > 0
    assert one['rdm'].shape == (nfft, p.G, 3)
    assert np.array_equal(one['rdm'], two['rdm']) and np.array_equal(one['cfar_maps'], two['cfar_maps'])
    _same_lists(one, two)
    if P == 21:   # the MATLAB-signature mirror, on a configuration whose prtNum no plan takes
        cfg = pcc.with_prt_num(base['s']['cfg'], P)
        pre = dict(base['s']['pre_p'], **ax)
        m = rsp.beams_detect(iq, win, nfft, pcc.CHAIN_CFAR, dc.CLUSTER, cfg, pre, precision=base['prec'], want_rdm=True,
                             want_cfar=True)
        assert np.array_equal(m['rdm'], one['rdm']) and np.array_equal(m['cfar_maps'], one['cfar_maps'])
        _same_lists(m, one)


def test_raw_detect_equals_dbf_then_pc_mtd_detect(base):
    p, s = base['plan'], base['s']
    P, nfft = 21, 32
    cube, W = pcc.echo_cube(s, P, base['prec'])
    win = np.kaiser(P, 4.0)
    args, ax = _chain_args(p.G, W.shape[0], nfft)
    two = p.pc_mtd_detect(p.dbf(cube, W), win, nfft, *args, want_rdm=True, want_cfar=True)
    one = p.raw_detect(cube, W, True, win, nfft, *args, want_rdm=True, want_cfar=True)
    own = p.raw_detect(cube, None, True, win, nfft, *args, want_rdm=True)   # the plan's own weights are W
    print('raw_detect', base['prec'], '%d detections, %d targets' % (len(one['detections']), len(one['final_targets'])))
    assert len(one['detections']) > 0 and len(one['final_targets']) > 0
    assert np.array_equal(one['rdm'], two['rdm']) and np.array_equal(one['cfar_maps'], two['cfar_maps'])
    _same_lists(one, two)
    assert np.array_equal(own['rdm'], one['rdm'])
    pre = dict(s['pre_p'], **ax)
    m = rsp.raw_detect(cube, W, win, nfft, pcc.CHAIN_CFAR, dc.CLUSTER, pcc.with_prt_num(s['cfg'], P), pre,
                       precision=base['prec'], want_rdm=True)
    assert np.array_equal(m['rdm'], one['rdm'])
    _same_lists(m, one)


def test_module_level_pulse_compress_on_a_config_no_plan_takes(bases):
    """rsp.pulse_compress with prtNum = 333 runs and equals the Plan method (complex double)."""
    base = bases['c128']
    s = base['s']
    cfg = pcc.with_prt_num(s['cfg'], 333)
    W, ang, k = plumbing_weights(cfg)
    pre = product_precompute(cfg, W, ang, k, C.V8_FIR)
    with pytest.raises(rsp.RspError):
        Plan(cfg, s['cfar'], s['clus'], pre).close()
    iq = pcc.beams(s, 333, 3, 'c128', seed=5)
    assert np.array_equal(rsp.pulse_compress(iq, cfg, pre), base['plan'].pulse_compress(iq))


# ---- 6. refusals, and the plan's other calls ------------------------------------------------------------------------
def test_refusals_and_the_other_calls_before_and_after(base):
    p, s, lib = base['plan'], base['s'], _abi.lib()
    cube = pcc.beams(s, p.P, p.C, base['prec'], seed=9)      # [P, N, C]: a raw frame of noise
    iq = pcc.beams(s, p.P, p.B, base['prec'], seed=10)
    frame0, st0 = p.process_cube(cube, want_rdm=True), p.process_stage2(iq)
    x = np.zeros(64)
    xp, xd = x.ctypes.data_as(ct.c_void_p), x.ctypes.data_as(ct.POINTER(ct.c_double))
    assert lib.rsp_pc(p.h, 0, 3, xp, _abi.RSP_C128, xd) == _abi.RSP_ERR_INVALID and b'bad sizes P=0 B=3' in lib.rsp_last_error()
    assert lib.rsp_pc(p.h, 16, -1, xp, _abi.RSP_C128, xd) == _abi.RSP_ERR_INVALID
    assert lib.rsp_pc(p.h, 1 << 20, 1 << 10, xp, _abi.RSP_C128, xd) == _abi.RSP_ERR_UNSUPPORTED     # sizes first: nothing is read
    assert b'32-bit offsets (< 2 GB each)' in lib.rsp_last_error()
    assert lib.rsp_pc(p.h, 1 << 20, 1 << 10, None, 99, None) == _abi.RSP_ERR_UNSUPPORTED
    assert lib.rsp_pc(p.h, 16, 3, None, 99, None) == _abi.RSP_ERR_INVALID and b'unknown dtype 99' in lib.rsp_last_error()
    assert lib.rsp_pc(p.h, 16, 3, None, _abi.RSP_C128, xd) == _abi.RSP_ERR_INVALID and b'null argument' in lib.rsp_last_error()
    assert lib.rsp_pc_device(p.h, 16, 3, None, None) == _abi.RSP_ERR_INVALID
    assert lib.rsp_pc_device(p.h, 1 << 20, 1 << 10, None, None) == _abi.RSP_ERR_UNSUPPORTED
    assert lib.rsp_profile_pc(p.h, 0, 1, 1, (ct.c_float * 3)(), None) == _abi.RSP_ERR_INVALID
    assert lib.rsp_pc_mtd_detect(p.h, 16, 1, 16, xp, _abi.RSP_C128, None, None, None) == _abi.RSP_ERR_INVALID
    assert b'B=1' in lib.rsp_last_error()                                                              # the detector's own refusal
    assert lib.rsp_pc_mtd_detect(p.h, 16, 3, 8, xp, _abi.RSP_C128, None, None, None) == _abi.RSP_ERR_INVALID   # nfft < P
    assert lib.rsp_raw_detect(p.h, 16, 40, 3, 16, xp, _abi.RSP_C128, None, 1, None, None, None) == _abi.RSP_ERR_INVALID
    d = p.device_alloc(1 << 16)
    try:
        assert lib.rsp_pc_device(p.h, 1, 1, ct.c_void_p(d), ct.c_void_p(d + 64)) == _abi.RSP_ERR_INVALID
        assert b'overlap' in lib.rsp_last_error()
    finally:
        p.device_free(d)
    with pytest.raises(rsp.RspError) as e:
        p.pc_layout(0, 1)
    assert e.value.code == _abi.RSP_ERR_INVALID
    with pytest.raises(ValueError):
        p.pulse_compress(iq[:, :100, :])
    assert p.pc_layout(333, 13) == rsp.describe_pc(s['cfg'], s['cfar'], s['clus'], s['pre_p'], 333, 13, precision=base['prec'])
    got = p.pulse_compress(iq)
    frame1, st1 = p.process_cube(cube, want_rdm=True), p.process_stage2(iq)
    assert np.array_equal(got, st0[1])
    assert np.array_equal(frame1['rdm'], frame0['rdm']) and frame1['detections'] == frame0['detections']
    assert frame1['final_targets'] == frame0['final_targets']
    assert np.array_equal(st1[0], st0[0]) and np.array_equal(st1[1], st0[1])
