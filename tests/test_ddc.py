"""The digital down-converter on the device (k_ddc: Plan.ddc, ddc_device, ddc_raw_detect,
rsp.mix_filter_downsample).

1. Every case of tests/_ddc_cases.py in both precisions against tests/_ddc_ref.py, the definition in long
   double: per element and per part |got - exact| <= (L + 6) u b, b = sum_j |h_j| |x[off + k D - j]|, u = 2^-53 or
   2^-24.  One u for each rounding of the definition -- the tap, the NCO value, the product, the L fused steps,
   the store -- and two of slack for second-order terms and the 1.4e-16 of the sincos routine.  A wrong tap, row
   or phase misses it by orders of magnitude.  The case asserts its tiling through describe_ddc first.
2. Exact cases: h = [1], D = 1, w = 2^62 gives x m to the bit; the real mixer's imaginary part is +0.
3. To the bit: a pulse alone (lanes along k) against the same pulse inside 64- and 130-pulse cubes (lanes along
   pulses); y(D, off)[k] against y(1, 0)[off + k D]; a channel alone against the channel in the cube; a second
   run; the device form against the host form, between guard words, while (P, N, D) change.
4. ddc_raw_detect against raw_detect(ddc(x)), field by field, and its refusal of a wrong line length.
5. The reference's own line: rsp.mix_filter_downsample against simulation_learn.m:79-102 in doubles.
"""
import ctypes as ct

import numpy as np
import pytest

import _ddc_cases as dd
import _ddc_ref as R
import _detect_cases as dc
import _pc_cases as pcc
import rsp
from rsp import _abi
from rsp.plan import Plan

pytestmark = pytest.mark.gpu

FIELDS = ('v_idx', 'r_idx', 'pair_idx', 'amp', 'Range', 'Velocity', 'Angle')
WORD = np.uint32(0x7FC5A3F1)   # a NaN as a float, and twice over as a double
GUARD = 1 << 12


@pytest.fixture(scope='module')
def plans():
    """Per precision, a plan of the plumbing waveform (1024 samples a pulse, 8 channels): for the down-converter
    it gives the device and the precision only."""
    s = pcc.pc_scenario(pcc.ORACLE_CASE)
    out = {prec: Plan(s['cfg'], s['cfar'], s['clus'], s['pre_p'], precision=prec) for prec in dd.PRECS}
    yield dict(out, s=s)
    for prec in dd.PRECS:
        out[prec].close()


@pytest.fixture(params=dd.PRECS)
def prec(request):
    return request.param


def bits(a):
    """The doubles of a real array as 64-bit words: equality of these tells +0 from -0."""
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def in_plan_precision(x, prec):
    """x as the plan holds it: rounded to float for a complex-single plan, as the upload does."""
    return np.asarray(x, dd.RDT[prec]).astype(np.float64)


def ratio(got, x, h, D, w, w0, mode, off, prec):
    """max over elements and parts of |got - exact| / (u b); where b = 0 the result must be 0."""
    yr, yi, b = R.ddc_ref(in_plan_precision(x, prec), h, D, w, w0, mode, off)
    got = R.cube3(got) if got.ndim < 3 else got
    assert got.shape == yr.shape, (got.shape, yr.shape)
    if not got.size:
        return 0.0
    er = np.abs(got.real.astype(R.LD) - yr)
    ei = np.abs(got.imag.astype(R.LD) - yi)
    zero = b == 0
    assert not er[zero].any() and not ei[zero].any()
    den = np.where(zero, 1, b) * R.LD(R.U[prec])
    return float(max((er / den).max(), (ei / den).max()))


# ---- 1. the cases against the definition -------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(dd.CASES))
def test_case_against_the_definition(plans, name, prec):
    shape, d = dd.check_preconditions(name, prec)
    _, x, h = dd.inputs(name, prec)
    got = plans[prec].ddc(x, h, shape['D'], w=shape['w'], w0=shape['w0'], nco=shape['mode'], off=shape['off'])
    assert got.shape == (shape['P'], d['No'], shape['C']) and got.dtype == np.complex128
    r = ratio(got, x, h, shape['D'], shape['w'], shape['w0'], shape['mode'], shape['off'], prec)
    print('DDCRATIO %s %s: err / (u b) = %.3g of the %d allowed; tile %d x %d, %d rows, %d workgroups'
          % (name, prec, r, shape['L'] + 6, d['TP'], d['TK'], d['in_rows'], d['workgroups']))
    assert r <= shape['L'] + 6
    if shape['mode'] == 'sin' and got.size:
        assert not got.imag.any() and not np.signbit(got.imag).any()
    if got.size:
        assert np.abs(got).max() > 0


# ---- 2. exact cases --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', [1, 3, 65])
def test_unit_tap_quarter_rate_is_the_product_to_the_bit(plans, prec, P):
    """h = [1], D = 1, w = 2^62: m is 1, -i, -1, i exactly, so y = fma(1, x m, 0) = x m + 0."""
    T = dd.RDT[prec]
    x = np.asfortranarray(np.random.default_rng(5).standard_normal((P, 301, 2)).astype(T))
    got = plans[prec].ddc(x, [1.0], 1, w=2 ** 62)
    mr, mi = R.nco(301, 2 ** 62)
    want = (x * mr.astype(T)[None, :, None] + T(0)) + 1j * (x * mi.astype(T)[None, :, None] + T(0))
    assert want.real.dtype == T
    assert np.array_equal(bits(got.real), bits(want.real)) and np.array_equal(bits(got.imag), bits(want.imag))


def test_real_mixer_has_a_positive_zero_imaginary_part(plans, prec):
    x = -np.abs(np.random.default_rng(6).standard_normal((5, 200, 2)))
    h = -np.abs(dd.fir_mat())
    got = plans[prec].ddc(x, h, 4, f0=10e6, fs=100e6, nco='sin', off=1)
    assert got.shape == (5, 50, 2) and np.abs(got.real).max() > 0
    assert (bits(got.imag) == 0).all()


# ---- 3. to the bit -----------------------------------------------------------------------------------------------
def test_a_pulse_alone_equals_the_pulse_inside_a_cube(plans, prec):
    """P = 1 runs lanes along k, P = 64 and P = 130 along pulses, in one, and in three pulse tiles; the line spans
    more than two k tiles of the P = 1 tiling and many of the others."""
    p = plans[prec]
    tk1 = rsp.describe_ddc(1, 1 << 16, 1, 12, 4, 1, prec)['TK']
    N = 4 * (2 * tk1 + 5) + 3
    x = np.asfortranarray(np.random.default_rng(7).standard_normal((130, N, 1)).astype(dd.RDT[prec]))
    h = dd.fir_mat()
    kw = dict(w=dd.TENTH, w0=12345, off=1)
    y130, y64 = p.ddc(x, h, 4, **kw), p.ddc(x[:64], h, 4, **kw)
    assert rsp.describe_ddc(130, N, 1, 12, 4, 1, prec)['p_tiles'] == 3 and rsp.describe_ddc(1, N, 1, 12, 4, 1, prec)['k_tiles'] == 3
    assert np.array_equal(y64, y130[:64])
    for q in (0, 63, 64, 129):
        y1 = p.ddc(x[q:q + 1], h, 4, **kw)
        assert np.array_equal(y1[0], y130[q]), q
    assert np.array_equal(p.ddc(x[63, :, 0], h, 4, **kw), y64[63, :, 0])   # a line as a vector


@pytest.mark.parametrize('P', [1, 3, 64])
@pytest.mark.parametrize('D, off', [(4, 0), (4, 3), (7, 2), (7, 6), (64, 63)])
def test_decimated_outputs_are_the_undecimated_ones(plans, prec, P, D, off):
    """y(D, off)[k] == y(1, 0)[off + k D]: the two tilings cut the line at different places."""
    p = plans[prec]
    tk = rsp.describe_ddc(P, 1 << 16, 2, 12, D, off, prec)['TK']
    N = D * (tk + 3) + off + 1
    x = np.asfortranarray(np.random.default_rng(8).standard_normal((P, N, 2)).astype(dd.RDT[prec]))
    h = dd.fir_mat()
    full = p.ddc(x, h, 1, w=dd.TENTH)
    dec = p.ddc(x, h, D, w=dd.TENTH, off=off)
    assert rsp.describe_ddc(P, N, 2, 12, D, off, prec)['k_tiles'] >= 2
    assert np.array_equal(dec, full[:, off::D])


def test_channels_runs_and_modes_agree(plans, prec):
    p = plans[prec]
    x = np.asfortranarray(np.random.default_rng(9).standard_normal((65, 700, 3)).astype(dd.RDT[prec]))
    h = dd.fir_mat()
    y = p.ddc(x, h, 4, w=dd.TENTH)
    for c in range(3):
        assert np.array_equal(p.ddc(x[:, :, c], h, 4, w=dd.TENTH), y[:, :, c])
    assert np.array_equal(p.ddc(x, h, 4, w=dd.TENTH), y)                       # a second run
    assert np.array_equal(p.ddc(x, h, 4, f0=10e6, fs=100e6), y)                # the word of f0 / fs
    s = p.ddc(x, h, 4, w=dd.TENTH, nco='sin')
    assert np.array_equal(s.real, -y.imag)                                     # Im of cos - i sin is -sin
    x32 = np.asfortranarray(x.astype(np.float32))                              # the same values as floats and as doubles
    assert np.array_equal(p.ddc(x32.astype(np.float64), h, 4, w=dd.TENTH), p.ddc(x32, h, 4, w=dd.TENTH))


def _device_ddc(p, prec, x, h, D, **kw):
    """ddc_device of x between guard words: (result [P, No, C] as complex128, the words before, the words after)."""
    T = dd.RDT[prec]
    P, N, C = x.shape
    xs = np.asfortranarray(x.astype(T))
    off = kw.get('off', 0)
    No = max(0, -(-(N - off) // D))
    esz = 2 * xs.dtype.itemsize
    nout = P * No * C
    total = (2 * GUARD + nout * esz) // 4
    d_in, d_out = p.device_alloc(xs.nbytes), p.device_alloc(total * 4)
    try:
        p.device_upload(d_in, xs.ravel(order='F'))
        p.device_upload(d_out, np.full(total, WORD, np.uint32))
        p.ddc_device(d_in, d_out + GUARD, P, N, C, h, D, **kw)
        words = p.device_download(d_out, total, np.uint32)
        back = p.device_download(d_in, xs.size, T)
    finally:
        p.device_free(d_in)
        p.device_free(d_out)
    assert np.array_equal(back, xs.ravel(order='F')), 'the input was written'
    body = words[GUARD // 4:GUARD // 4 + nout * esz // 4].view(p.cdtype)
    return body.reshape((P, No, C), order='F').astype(np.complex128), words[:GUARD // 4], words[-(GUARD // 4):]


def test_device_form_between_guard_words_while_sizes_change(plans, prec):
    p = plans[prec]
    rng = np.random.default_rng(10)
    h = dd.fir_mat()
    shapes = [((65, 301, 2), 4, 3), ((3, 77, 1), 7, 0), ((130, 1000, 1), 1, 0), ((65, 301, 2), 4, 3), ((1, 5000, 3), 64, 17)]
    for shp, D, off in shapes:
        x = rng.standard_normal(shp).astype(dd.RDT[prec])
        kw = dict(w=dd.TENTH, w0=99, off=off)
        want = p.ddc(x, h, D, **kw)
        got, lo, hi = _device_ddc(p, prec, x, h, D, **kw)
        assert (lo == WORD).all() and (hi == WORD).all(), 'written outside the P No C output elements'
        assert np.array_equal(got, want), (shp, D, off)
    got, lo, hi = _device_ddc(p, prec, rng.standard_normal((4, 3, 2)), h, 4, w=1, off=3)   # N <= off: no output
    assert got.size == 0 and (lo == WORD).all() and (hi == WORD).all()


def test_profile_ddc(plans, prec):
    r = plans[prec].profile_ddc(65, 2000, 3, 12, 4, iters=2)
    d = rsp.describe_ddc(65, 2000, 3, 12, 4, 0, prec)
    assert r['stage'] == 'k_ddc' and r['ms'] > 0 and r['bytes'] == d['in_bytes'] + d['out_bytes']


# ---- 4. the composition ---------------------------------------------------------------------------------------------
def _same_lists(a, b):
    assert len(a['detections']) == len(b['detections'])
    for x, y in zip(a['detections'], b['detections']):
        for f in FIELDS:
            assert x[f] == y[f], (f, x, y)
    assert a['final_targets'] == b['final_targets']


def _if_cube(cube, D, w):
    """The baseband cube imaged to an IF: x = Re(cube upsampled by D (zeros between) x e^{+i theta}), theta the
    NCO's own phase, so that cos - i sin brings every D-th sample back."""
    P, N, C = cube.shape
    up = np.zeros((P, N * D, C), np.complex128)
    up[:, ::D] = cube
    s, c = R.sincos_2pi(R.nco_u(N * D, w))
    return np.asfortranarray((up * (c.astype(np.float64) + 1j * s.astype(np.float64))[None, :, None]).real)


def test_ddc_raw_detect_equals_ddc_then_raw_detect(plans, prec):
    p, s = plans[prec], plans['s']
    P, nfft, D = 21, 32, 4
    cube, W = pcc.echo_cube(s, P, prec)
    x = _if_cube(cube.astype(np.complex128), D, dd.TENTH)
    h = D * dd.fir_mat()   # the zeros between the samples take 1 / D of the passband gain
    win = np.kaiser(P, 4.0)
    ax = dc.axes(nfft, p.G, W.shape[0])
    args = (pcc.CHAIN_CFAR, dc.CLUSTER, ax['range_axis'], ax['velocity_axis'], ax['deltaR'], ax['deltaV'], ax['beam_angles_deg'],
            ax['k_slopes_LUT'])
    iq = p.ddc(x, h, D, w=dd.TENTH)
    assert iq.shape == (P, p.N, W.shape[1])
    two = p.raw_detect(iq, W, True, win, nfft, *args, want_rdm=True, want_cfar=True)
    one = p.ddc_raw_detect(x, h, D, w=dd.TENTH, W=W, conj=True, win=win, nfft=nfft, cfar=args[0], cluster=args[1],
                           range_axis=args[2], velocity_axis=args[3], deltaR=args[4], deltaV=args[5], beam_angles_deg=args[6],
                           k_slopes_LUT=args[7], want_rdm=True, want_cfar=True)
    print('ddc_raw_detect', prec, '%d detections, %d targets' % (len(one['detections']), len(one['final_targets'])))
    assert np.abs(one['rdm']).max() > 0
    assert np.array_equal(one['rdm'], two['rdm']) and np.array_equal(one['cfar_maps'], two['cfar_maps'])
    _same_lists(one, two)
    again = p.ddc_raw_detect(x.astype(np.float32), h, D, w=dd.TENTH, W=W, win=win, nfft=nfft, cfar=args[0], cluster=args[1],
                             range_axis=args[2], velocity_axis=args[3], deltaR=args[4], deltaV=args[5], beam_angles_deg=args[6],
                             k_slopes_LUT=args[7], want_rdm=True)
    if prec == 'c64':   # the plan rounds the doubles to the same floats
        assert np.array_equal(again['rdm'], one['rdm'])


def test_ddc_raw_detect_refuses_another_line_length(plans, prec):
    p = plans[prec]
    x = np.zeros((4, 4 * p.N - 4, 8))
    with pytest.raises(_abi.RspError) as e:
        p.ddc_raw_detect(x, dd.fir_mat(), 4, w=1, W=np.ones((3, 8), complex), nfft=4,
                         range_axis=np.zeros(p.G), velocity_axis=np.zeros(4), beam_angles_deg=np.zeros(3), k_slopes_LUT=np.zeros(2))
    assert e.value.code == _abi.RSP_ERR_INVALID and 'No = %d' % (p.N - 1) in str(e.value) and 'point_PRT is %d' % p.N in str(e.value)


def test_refusals_on_a_live_plan_and_the_plan_afterwards(plans, prec):
    p, lib = plans[prec], _abi.lib()
    x = np.zeros(64)
    xp, xd = x.ctypes.data_as(ct.c_void_p), x.ctypes.data_as(ct.POINTER(ct.c_double))
    taps = np.ones(12)
    prm = _abi.DdcParams(w=1, w0=0, mode=0, D=4, off=0, L=12, h=taps.ctypes.data_as(ct.POINTER(ct.c_double)))
    assert lib.rsp_ddc(p.h, 4, 8, 1, xp, _abi.RSP_C64, ct.byref(prm), xd) == _abi.RSP_ERR_INVALID
    assert b'unknown dtype 1' in lib.rsp_last_error()
    assert lib.rsp_ddc(p.h, 4, 8, 1, xp, _abi.RSP_R64, ct.byref(prm), None) == _abi.RSP_ERR_INVALID
    assert b'null argument' in lib.rsp_last_error()
    prm.mode = 2
    assert lib.rsp_ddc(p.h, 4, 8, 1, xp, _abi.RSP_R64, ct.byref(prm), xd) == _abi.RSP_ERR_INVALID
    assert b'mode must be' in lib.rsp_last_error()
    prm.mode = 0
    d = p.device_alloc(1 << 12)
    try:
        assert lib.rsp_ddc_device(p.h, 4, 8, 1, ct.c_void_p(d), ct.byref(prm), ct.c_void_p(d + 64)) == _abi.RSP_ERR_INVALID
        assert b'overlap' in lib.rsp_last_error()
        assert lib.rsp_ddc_device(p.h, 4, 8, 1, ct.c_void_p(d), ct.byref(prm), ct.c_void_p(d + 2052)) == _abi.RSP_ERR_INVALID
        assert b'aligned' in lib.rsp_last_error()
    finally:
        p.device_free(d)
    with pytest.raises(ValueError):
        p.ddc(np.zeros(8, complex), taps, 4, w=1)
    with pytest.raises(ValueError):
        p.ddc(np.zeros(8), taps, 4)
    y = p.ddc(np.ones(8), [1.0], 1, w=0)   # the plan still runs
    assert np.array_equal(y, np.ones(8, complex))


# ---- 5. the reference's own line -------------------------------------------------------------------------------------
def test_mix_filter_downsample_against_the_matlab_form():
    xt, f, fs = R.lfm_cut()
    Num = dd.fir_mat()
    got = rsp.mix_filter_downsample(xt, f, fs, Num, 4)
    want = R.matlab_form(xt, f, fs, Num, 4)
    tol = R.matlab_allowance(xt, f, fs, Num, 4)
    err = np.abs(got - want)
    print('mix_filter_downsample: max |y| %.3g, max err %.3g, max err / allowance %.3g' % (np.abs(want).max(), err.max(), (err / tol).max()))
    assert got.shape == want.shape == (500,) and got.dtype == np.float64
    assert (err <= tol).all()
