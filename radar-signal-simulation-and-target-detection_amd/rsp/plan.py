"""Host-side plan object over the C-ABI (include/rsp.h).

Arrays use MATLAB index order (the reference's), stored column-major so they are
passed to the library exactly as a MEX gateway would pass mxArray data:
echo cube ``[P, N, C]``, range-Doppler maps ``[P, G, B]``, CFAR maps
``[P, G, B-1]``.
"""
import ctypes as ct
import numpy as np

from . import _abi
from ._abi import check, lib


def _dptr(a):
    return a.ctypes.data_as(ct.POINTER(ct.c_double))


def _complex_arg(a):
    """A complex array as the library takes it: (Fortran-ordered array, its void pointer, dtype
    code).  complex64 stays; everything else becomes complex128."""
    c64 = np.asarray(a).dtype == np.complex64
    a = np.asfortranarray(a, None if c64 else np.complex128)
    return a, a.ctypes.data_as(ct.c_void_p), _abi.RSP_C64 if c64 else _abi.RSP_C128


def _gate_cols_arg(gate_cols):
    """((first, last), ...) of the three segments as the six int32 the gated calls take."""
    return (ct.c_int32 * 6)(*[int(x) for fl in gate_cols for x in fl])


def _with_hits(call, first_cap, hits_cap, want_hits):
    """The stage-3 calls' hit list: ``call(cap, hits_ptr, maps)`` runs the C function (``maps``
    False: with None for every map pointer) and returns the total.  The first call takes ``hits_cap``
    records (None: ``first_cap``); when the caller set no capacity and the total is larger, a second
    one fetches the whole list, and nothing else.  Returns (total, the hits that came back)."""
    cap = (int(hits_cap) if hits_cap is not None else first_cap) if want_hits else 0
    hits = np.zeros(max(cap, 1), HIT_DTYPE)
    total = call(cap, hits.ctypes.data_as(ct.POINTER(_abi.Stage3Hit)) if cap else None, True)
    if want_hits and hits_cap is None and total > cap:
        cap, hits = total, np.zeros(total, HIT_DTYPE)
        total = call(cap, hits.ctypes.data_as(ct.POINTER(_abi.Stage3Hit)), False)
    return total, hits[:min(total, cap)]


def _det_dict(d):
    return {'v_idx': d.v_idx, 'r_idx': d.r_idx, 'pair_idx': d.pair_idx, 'amp': d.amp,
            'Range': d.Range, 'Velocity': d.Velocity, 'Angle': d.Angle}


def _tgt_dict(t):
    return {'Range': t.Range, 'Velocity': t.Velocity, 'Angle': t.Angle, 'Power': t.Power}


def _marshal(config, cfar_params, cluster_params, pre, keep):
    """The C structs of rsp_plan_create_ex / rsp_plan_describe; the arrays they borrow go to ``keep``."""
    sc = config['Sig_Config']

    def arr(x, cplx=False):
        a = np.ascontiguousarray(np.asarray(x, np.complex128 if cplx else np.float64))
        if cplx:
            a = a.view(np.float64)
        keep.append(a)
        return _dptr(a)

    cfg = _abi.SigConfig(c=sc['c'], fs=sc['fs'], fc=sc['fc'], prt=sc['prt'], wavelength=sc['wavelength'],
                         element_spacing=config['Array']['element_spacing'], prtNum=sc['prtNum'],
                         point_PRT=sc['point_PRT'], channel_num=sc['channel_num'], beam_num=sc['beam_num'])
    cfar = _abi.CfarParams(refCells_V=cfar_params['refCells_V'], guardCells_V=cfar_params['guardCells_V'],
                           refCells_R=cfar_params['refCells_R'], guardCells_R=cfar_params['guardCells_R'],
                           T_CFAR=cfar_params['T_CFAR'])
    cluster = _abi.ClusterParams(max_range_sep=cluster_params['max_range_sep'],
                                 max_vel_sep=cluster_params['max_vel_sep'],
                                 max_angle_sep=cluster_params['max_angle_sep'])
    W = np.asarray(pre['DBF_coeffs_data_C'], np.complex128)
    Wcm = np.asfortranarray(W).ravel(order='F')      # B x C column-major (MATLAB)
    klut = np.asarray(pre['k_slopes_LUT'], float)
    pre_c = _abi.Precomputed(
        tx_pulse=arr(pre['tx_pulse'], True) if 'tx_pulse' in pre else None,
        P_signal_unscaled=pre.get('P_signal_unscaled', 0.0),
        DBF_coeffs_data_C=arr(Wcm, True), MF_narrow=arr(pre['MF_narrow']), n_MF_narrow=len(pre['MF_narrow']),
        fir_delay=int(pre['fir_delay']), MF_medium_fft=arr(pre['MF_medium_fft'], True),
        N_fft_med=int(pre['N_fft_med']), MF_long_fft=arr(pre['MF_long_fft'], True),
        N_fft_long=int(pre['N_fft_long']), N_gate_narrow=int(pre['N_gate_narrow']),
        N_gate_medium=int(pre['N_gate_medium']), N_gate_long=int(pre['N_gate_long']),
        N_total_gate=int(pre['N_total_gate']), seg_start_narrow=int(pre['seg_start_narrow']),
        seg_start_medium=int(pre['seg_start_medium']), seg_start_long=int(pre['seg_start_long']),
        MTD_win=arr(pre['MTD_win']), range_axis=arr(pre['range_axis']), velocity_axis=arr(pre['velocity_axis']),
        deltaR=float(pre['deltaR']), deltaV=float(pre['deltaV']), beam_angles_deg=arr(pre['beam_angles_deg']),
        k_slopes_LUT=arr(klut if klut.size else np.zeros(1)))
    return cfg, cfar, cluster, pre_c


def _options(device, frames_per_launch, precision, k1_tiled, monopulse, k2_all_rows=False):
    if precision not in ('c128', 'c64'):
        raise ValueError("precision must be 'c128' or 'c64'")
    opt = _abi.PlanOptions()
    check(lib().rsp_plan_options_default(ct.byref(opt)))
    opt.device, opt.frames_per_launch = int(device), int(frames_per_launch)
    opt.precision = _abi.RSP_C128 if precision == 'c128' else _abi.RSP_C64
    if monopulse not in ('amplitude', 'complex'):
        raise ValueError("monopulse must be 'amplitude' (fsf:282-290) or 'complex' "
                         "(main_plot_snr_vs_angle_error.m:455-462), got %r" % (monopulse,))
    opt.flags = (_abi.RSP_PLAN_K1_TILED if k1_tiled else 0) | \
        (_abi.RSP_PLAN_MONOPULSE_COMPLEX if monopulse == 'complex' else 0) | \
        (_abi.RSP_PLAN_K2_ALL_ROWS if k2_all_rows else 0)
    return opt


def _route_dict(r):
    return dict(kernel=_abi.K1_KERNELS[r.kernel], transform=_abi.K1_TRANSFORMS[r.transform], R=r.R, Q=r.Q,
                NT=r.NT, Ppad=r.Ppad, tiles_per_wave=r.tiles_per_wave, stage2_lgp=r.stage2_lgp)


def describe(config, cfar_params, cluster_params, precomputed_data, precision='c128', k1_tiled=False, ncu=256):
    """What a plan of these arguments would be on a device of ``ncu`` compute units, without a
    device (rsp_plan_describe): ``(sizes, route)`` as ``Plan.sizes`` and ``Plan.k1_route()``.
    Refusals raise RspError with the code and message rsp_plan_create_ex would give."""
    keep = []
    cfg, cfar, cluster, pre = _marshal(config, cfar_params, cluster_params, precomputed_data, keep)
    opt = _options(0, 1, precision, k1_tiled, 'amplitude')
    s, r = _abi.Sizes(), _abi.K1Route()
    check(lib().rsp_plan_describe(ct.byref(cfg), ct.byref(cfar), ct.byref(cluster), ct.byref(pre), ct.byref(opt),
                                  int(ncu), ct.byref(s), ct.byref(r)))
    return s, _route_dict(r)


def _tiling_dict(t):
    return dict(fast=bool(t.fast), RT=t.RT, hR=t.hR, W=t.W, n_tiles=t.n_tiles, n_bands=t.n_bands, VB=t.VB,
                rows=t.rows)


def describe_k3(config, cfar_params, cluster_params, precomputed_data, precision='c128', k1_tiled=False, ncu=256):
    """``Plan.k3_tiling()`` of the plan these arguments would give, without a device
    (rsp_plan_describe_k3); refusals as ``describe``."""
    keep = []
    cfg, cfar, cluster, pre = _marshal(config, cfar_params, cluster_params, precomputed_data, keep)
    opt = _options(0, 1, precision, k1_tiled, 'amplitude')
    t = _abi.K3Tiling()
    check(lib().rsp_plan_describe_k3(ct.byref(cfg), ct.byref(cfar), ct.byref(cluster), ct.byref(pre), ct.byref(opt),
                                     int(ncu), ct.byref(t)))
    return _tiling_dict(t)


K2_SEGMENTS = ('narrow', 'medium', 'long')   # rsp_k2_layout.seg's slots


def _k2_dict(L):
    segs = [{k: getattr(s, k) for k, _ in _abi.K2Segment._fields_ if k != 'present'} if s.present else None
            for s in L.seg]
    return dict(k2_pts=L.k2_pts, wg_per_cu=L.wg_per_cu, NZ=L.NZ, nseg=L.nseg, njobs=L.njobs, nwg=L.nwg, segments=segs)


def describe_k2(config, cfar_params, cluster_params, precomputed_data, precision='c128', k1_tiled=False, ncu=256):
    """``Plan.k2_layout()`` of the plan these arguments would give, without a device
    (rsp_plan_describe_k2); refusals as ``describe``."""
    keep = []
    cfg, cfar, cluster, pre = _marshal(config, cfar_params, cluster_params, precomputed_data, keep)
    opt = _options(0, 1, precision, k1_tiled, 'amplitude')
    L = _abi.K2Layout()
    check(lib().rsp_plan_describe_k2(ct.byref(cfg), ct.byref(cfar), ct.byref(cluster), ct.byref(pre), ct.byref(opt),
                                     int(ncu), ct.byref(L)))
    return _k2_dict(L)


K2_RECORD_FIELDS = ('seg', 'blk', 'row0', 'wg')   # rsp_k2_record


def _k2_records(call):
    n = ct.c_int32(0)
    check(call(None, 0, ct.byref(n)))
    rec = (_abi.K2Record * max(n.value, 1))()
    check(call(rec, n.value, ct.byref(n)))
    return np.array([[getattr(r, f) for f in K2_RECORD_FIELDS] for r in rec[:n.value]], dtype=np.int32).reshape(-1, 4)


def describe_k2_records(config, cfar_params, cluster_params, precomputed_data, precision='c128', k1_tiled=False,
                        ncu=256):
    """``Plan.k2_records()`` of the plan these arguments would give, without a device
    (rsp_plan_describe_k2_records); refusals as ``describe``."""
    keep = []
    cfg, cfar, cluster, pre = _marshal(config, cfar_params, cluster_params, precomputed_data, keep)
    opt = _options(0, 1, precision, k1_tiled, 'amplitude')
    return _k2_records(lambda out, cap, n: lib().rsp_plan_describe_k2_records(
        ct.byref(cfg), ct.byref(cfar), ct.byref(cluster), ct.byref(pre), ct.byref(opt), int(ncu), out, cap, n))


K2_ROW_SETS = {'all': 0, 'band': 1, 'edge': 2}   # RSP_K2_ROWS_*


def _k2_row_set(call):
    rs = _abi.K2RowSet()
    rec = _k2_records(lambda out, cap, n: call(ct.byref(rs), out, cap, n))
    return {k: getattr(rs, k) for k, _ in _abi.K2RowSet._fields_}, rec


def k2_set_rows(rs, P):
    """(beam, Doppler row), 0-based, of every row of the row-set dict ``rs``: an int array [total, 2]."""
    i = np.arange(rs['total'])
    j = i % max(rs['n'], 1)
    return np.stack([i // max(rs['n'], 1), rs['base'] + j + np.where(j >= rs['split'], rs['gap'], 0)], axis=1)


def describe_k2_row_set(config, cfar_params, cluster_params, precomputed_data, which, precision='c128',
                        k1_tiled=False, ncu=256):
    """``Plan.k2_row_set(which)`` of the plan these arguments would give, without a device
    (rsp_plan_describe_k2_row_set); refusals as ``describe``."""
    keep = []
    cfg, cfar, cluster, pre = _marshal(config, cfar_params, cluster_params, precomputed_data, keep)
    opt = _options(0, 1, precision, k1_tiled, 'amplitude')
    return _k2_row_set(lambda rs, out, cap, n: lib().rsp_plan_describe_k2_row_set(
        ct.byref(cfg), ct.byref(cfar), ct.byref(cluster), ct.byref(pre), ct.byref(opt), int(ncu),
        K2_ROW_SETS[which], rs, out, cap, n))


HIT_DTYPE = np.dtype([('v_idx', np.int32), ('r_idx', np.int32), ('beam_idx', np.int32), ('reserved', np.int32),
                      ('amp', np.float64), ('threshold', np.float64)])   # rsp_stage3_hit
STAGE3_WANT = ('mtd', 'amp', 'flags', 'threshold', 'hits')


def _stage3_params(cfar):
    """rsp_stage3_cfar_params from the reference's config.cfar field names
    (debug_simulated_data_processing_v2.m:103-127)."""
    return _abi.Stage3CfarParams(refCells_R=int(cfar['refCells_R']), saveCells_R=int(cfar['saveCells_R']),
                                 CFARmethod_R=int(cfar['CFARmethod_R']), MTD_0v_num=int(cfar['MTD_0v_num']),
                                 T_CFAR=float(cfar['T_CFAR']))


def describe_stage3(P, segments, cfar):
    """What the stage-3 range CFAR does with a map of ``P`` Doppler rows and range segments of
    ``segments`` = (narrow, medium, long) columns, without a device (rsp_stage3_describe):
    ``seg_first`` (1-based) and ``seg_len`` of each segment, the notched rows ``notch`` = (first,
    last) 1-based and clipped to 1..P, the window's ``halo`` = s + r, the kernel's ``max_halo``,
    ``chunk`` (range cells per workgroup) and ``rows``.  Refusals raise RspError with the code and
    message the CFAR calls give."""
    n1, n2, n3 = (int(x) for x in segments)
    cfg = _abi.SigConfig(prtNum=int(P))
    pre = _abi.Precomputed(N_gate_narrow=n1, N_gate_medium=n2, N_gate_long=n3, N_total_gate=n1 + n2 + n3)
    prm, info = _stage3_params(cfar), _abi.Stage3Info()
    check(lib().rsp_stage3_describe(ct.byref(cfg), ct.byref(pre), ct.byref(prm), ct.byref(info)))
    return dict(P=info.P, G=info.G, seg_first=tuple(info.seg_first), seg_len=tuple(info.seg_len),
                notch=(info.notch_first, info.notch_last), halo=info.halo, max_halo=info.max_halo,
                chunk=info.chunk, rows=info.rows)


VCFAR_METHODS = {'ca': 0, 'goca': 1, 'soca': 2}


def _vcfar_params(cfar, method='ca'):
    """rsp_vcfar_params from the reference's cfar_params field names
    (main_simulate_echoes_with_array_v3.m:30-35) and ``method``: 'ca' (what the reference computes),
    'goca' or 'soca', any letter case, or the C value 0, 1, 2.  ``cfar['method']`` is not read."""
    if isinstance(method, str):
        if method.lower() not in VCFAR_METHODS:
            raise ValueError("method must be 'ca', 'goca' or 'soca', got %r" % (method,))
        method = VCFAR_METHODS[method.lower()]
    return _abi.VcfarParams(refCells_V=int(cfar['refCells_V']), guardCells_V=int(cfar['guardCells_V']),
                            method=int(method), T_CFAR=float(cfar['T_CFAR']))


def describe_vcfar(P, G, cfar, method='ca'):
    """What the Doppler CA-CFAR does with a map of ``P`` Doppler rows and ``G`` range columns, without
    a device (rsp_vcfar_describe): the window's ``halo`` = refCells_V + guardCells_V / 2, the kernel's
    ``max_halo``, the ``rows`` and ``cols`` of a workgroup's tile and ``row_tiles``, ``col_tiles``.
    Refusals raise RspError with the code and message the CFAR calls give."""
    prm, info = _vcfar_params(cfar, method), _abi.VcfarInfo()
    check(lib().rsp_vcfar_describe(int(P), int(G), ct.byref(prm), ct.byref(info)))
    return {k: getattr(info, k) for k, _ in _abi.VcfarInfo._fields_}


def _xcfar_params(cfar):
    """rsp_cfar_params from the reference's cfar_params field names (v8:45-47; ``method`` is not read:
    fun_process_single_frame has only 'GOCA')."""
    return _abi.CfarParams(refCells_V=int(cfar['refCells_V']), guardCells_V=int(cfar['guardCells_V']),
                           refCells_R=int(cfar['refCells_R']), guardCells_R=int(cfar['guardCells_R']),
                           T_CFAR=float(cfar['T_CFAR']))


def describe_xcfar(P, G, cfar):
    """What the cross GOCA-CFAR map detector does with a map of ``P`` Doppler rows and ``G`` range
    columns, without a device (rsp_xcfar_describe): the window's halos ``hR`` = refCells_R +
    guardCells_R and ``hV``, the kernel's ``max_hR`` and ``max_hV``, the ``rows`` and ``cols`` of a
    workgroup's tile, ``row_tiles``, ``col_tiles`` and the 1-based inclusive bounds ``r0``..``r1``,
    ``v0``..``v1`` of the cells under test (r0 > r1 and v0 > v1: none).  Refusals raise RspError with
    the code and message the CFAR calls give."""
    prm, info = _xcfar_params(cfar), _abi.XcfarInfo()
    check(lib().rsp_xcfar_describe(int(P), int(G), ct.byref(prm), ct.byref(info)))
    return {k: getattr(info, k) for k, _ in _abi.XcfarInfo._fields_}


def describe_detect(V, G, B, cfar, precision='c128'):
    """What the detector on an RD cube does with ``V`` Doppler rows, ``G`` range cells and ``B`` beams in
    a plan of ``precision``, without a device (rsp_detect_describe): ``n_pairs`` = B - 1 pair-sum maps, the
    ``rows`` x ``cols`` tile of k_pairsum (cube in MATLAB's layout), ``row_tiles``, ``col_tiles``, its
    ``lds_bytes``, the 1-based inclusive bounds ``r0``..``r1``, ``v0``..``v1`` of the cells under test
    (r0 > r1 and v0 > v1: none), ``cells_under_test`` per map and ``max_detections``.  Refusals raise
    RspError with the code and message ``Plan.detect`` gives."""
    prm, info = _xcfar_params(cfar), _abi.DetectInfo()
    check(lib().rsp_detect_describe(int(V), int(G), int(B), _prec_code(precision), ct.byref(prm), ct.byref(info)))
    return {k: getattr(info, k) for k, _ in _abi.DetectInfo._fields_ if k != 'reserved'}


DBF_ROW_LAYOUTS = {'split': _abi.RSP_DBF_ROWS_SPLIT, 'pair': _abi.RSP_DBF_ROWS_PAIR}


def describe_dbf(P, N, C, B, precision='c128'):
    """How k_dbf covers a [P, N, C] cube into B beams in a plan of ``precision``, without a device
    (rsp_dbf_describe): ``positions`` = P N, ``CP``, ``BMAX``, ``sub_tile`` (positions per MFMA
    sub-tile), ``tiles_per_wave``, ``waves``, ``rounds``, ``wg_positions``, ``workgroups``,
    ``tail_positions`` (of the last, partly filled sub-tile), ``row_layout`` ('split' / 'pair') and
    ``pitch``.  Refusals raise RspError with the code and message ``Plan.dbf`` gives."""
    if precision not in ('c128', 'c64'):
        raise ValueError("precision must be 'c128' or 'c64'")
    info = _abi.DbfInfo()
    check(lib().rsp_dbf_describe(int(P), int(N), int(C), int(B), _abi.RSP_C128 if precision == 'c128' else _abi.RSP_C64,
                                 ct.byref(info)))
    d = {k: getattr(info, k) for k, _ in _abi.DbfInfo._fields_}
    d['row_layout'] = {v: k for k, v in DBF_ROW_LAYOUTS.items()}[d['row_layout']]
    return d


def _table(call):
    n = ct.c_int32(0)
    check(call(None, 0, ct.byref(n)))
    t = np.empty(max(n.value, 1), np.float64)
    check(call(_dptr(t), n.value, ct.byref(n)))
    return t[:n.value].reshape(-1, 2, 64)


def dbf_table(W, conj=True, row_layout='split'):
    """The DBF's matrix-core A operands for weights ``W`` [B, C] (rsp_dbf_table): a float64 array
    [MB * CP / 4, 2, 64]; entry [mb * CP / 4 + j, e, lane] is the coefficient of Re x_c (e = 0) or Im x_c
    (e = 1), c = 4 j + lane // 16, in MFMA row lane % 16 of block mb.  ``row_layout`` 'split': that row
    is beam 8 mb + m % 8, part m // 8 (K1's); 'pair': beam 8 mb + m // 2, part m % 2."""
    W = np.asarray(W, np.complex128)
    B, C = W.shape
    Wcm = np.asfortranarray(W).ravel(order='F').view(np.float64)
    return _table(lambda out, cap, n: lib().rsp_dbf_table(_dptr(Wcm), B, C, 1 if conj else 0, DBF_ROW_LAYOUTS[row_layout],
                                                          out, cap, n))


MTD_ROUTES = {_abi.RSP_MTD_ROUTE_POW2: 'pow2', _abi.RSP_MTD_ROUTE_CHIRPZ: 'chirpz', _abi.RSP_MTD_ROUTE_DIRECT: 'direct'}


def _prec_code(precision):
    if precision not in ('c128', 'c64'):
        raise ValueError("precision must be 'c128' or 'c64'")
    return _abi.RSP_C128 if precision == 'c128' else _abi.RSP_C64


def describe_mtd(P, G, nfft=None, precision='c128'):
    """How k_mtd_any transforms a [P, G] map to ``nfft`` rows (None: P) in a plan of ``precision``,
    without a device (rsp_mtd_describe): ``P``, ``G``, ``nfft`` as resolved, ``route`` ('pow2' /
    'chirpz'), ``M`` (points of the transform in LDS: nfft, or the chirp-z length), ``cols`` (columns
    per workgroup), ``col_tiles``, ``lds_bytes`` and ``table_elems``.  Refusals raise RspError with the
    code and message ``Plan.mtd`` gives."""
    info = _abi.MtdInfo()
    check(lib().rsp_mtd_describe(int(P), int(G), int(nfft or 0), _prec_code(precision), ct.byref(info)))
    d = {k: getattr(info, k) for k, _ in _abi.MtdInfo._fields_}
    d['route'] = MTD_ROUTES[d['route']]
    return d


def _pc_dict(info):
    d = {k: getattr(info, k) for k, _ in _abi.PcInfo._fields_}
    for k in ('ivl_lo', 'ivl_start'):
        d[k] = list(d[k])[:info.n_intervals]
    return d


def describe_pc(config, cfar_params, cluster_params, precomputed_data, P, B, precision='c128', ncu=256):
    """How the stand-alone pulse compression covers ``P`` pulses of ``B`` beams of this waveform, without a
    device (rsp_plan_describe_pc): the fields of rsp_pc_info as a dict.  The configuration's own prtNum
    and beam_num are not read, so one that ``describe`` refuses for its pulse count is accepted.
    Refusals raise RspError with the code and message ``Plan.pulse_compress`` gives."""
    keep = []
    cfg, cfar, cluster, pre = _marshal(config, cfar_params, cluster_params, precomputed_data, keep)
    opt = _options(0, 1, precision, False, 'amplitude')
    info = _abi.PcInfo()
    check(lib().rsp_plan_describe_pc(ct.byref(cfg), ct.byref(cfar), ct.byref(cluster), ct.byref(pre), ct.byref(opt),
                                     int(ncu), int(P), int(B), ct.byref(info)))
    return _pc_dict(info)


def describe_ddc(P, N, C, L, D, off=0, precision='c128'):
    """How k_ddc covers a real cube [P, N, C] with ``L`` taps, decimation ``D`` and phase ``off`` in a plan of
    ``precision``, without a device (rsp_ddc_describe): the fields of rsp_ddc_info as a dict -- ``No``, the
    tile ``TP`` x ``TK``, ``in_rows``, ``k_tiles``, ``p_tiles``, ``workgroups``, ``lds_bytes``, ``tap_chunk``,
    ``threads``, ``k_per_thread``, ``in_bytes`` and ``out_bytes``.  Refusals raise RspError with the code and
    message ``Plan.ddc`` gives."""
    info = _abi.DdcInfo()
    check(lib().rsp_ddc_describe(int(P), int(N), int(C), int(L), int(D), int(off), _prec_code(precision), ct.byref(info)))
    return {k: getattr(info, k) for k, _ in _abi.DdcInfo._fields_}


def ddc_phase_word(f0, fs):
    """The NCO's phase step for a carrier ``f0`` sampled at ``fs``: round(f0 / fs 2^64) mod 2^64
    (rsp_ddc_phase_word)."""
    w = ct.c_uint64()
    check(lib().rsp_ddc_phase_word(float(f0), float(fs), ct.byref(w)))
    return int(w.value)


DDC_MODES = {'iq': _abi.RSP_DDC_NCO_IQ, 'sin': _abi.RSP_DDC_NCO_SIN}


def _ddc_params(h, D, f0, fs, w, w0, nco, off):
    """rsp_ddc_params and the tap array it borrows; the phase step is ``w`` or, from ``f0`` and ``fs``,
    ``ddc_phase_word``'s."""
    if nco not in DDC_MODES:
        raise ValueError("nco must be 'iq' or 'sin', got %r" % (nco,))
    if (w is None) != (f0 is not None and fs is not None) or (w is not None and (f0 is not None or fs is not None)):
        raise ValueError('give either w or both f0 and fs')
    if w is None:
        w = ddc_phase_word(f0, fs)
    taps = np.ascontiguousarray(np.asarray(h, np.float64).ravel())
    keep = taps if taps.size else np.zeros(1)
    prm = _abi.DdcParams(w=int(w) % 2 ** 64, w0=int(w0) % 2 ** 64, mode=DDC_MODES[nco], D=int(D), off=int(off),
                         L=int(taps.size), h=_dptr(keep))
    return prm, keep


def _real_arg(x):
    """A real array as rsp_ddc takes it: (Fortran-ordered array, its void pointer, dtype code).  float32
    stays; everything else becomes float64."""
    r32 = np.asarray(x).dtype == np.float32
    a = np.asfortranarray(x, None if r32 else np.float64)
    return a, a.ctypes.data_as(ct.c_void_p), _abi.RSP_R32 if r32 else _abi.RSP_R64


def mtd_table(nfft, precision='c128'):
    """The chirp-z tables of length ``nfft`` as the kernel reads them (rsp_mtd_table): ``(w, Bf)``,
    complex128 arrays that hold the values rounded to ``precision``: w[m] = exp(-i pi (m^2 mod 2 nfft) /
    nfft), m < nfft, and Bf, the M-point DFT of conj(w) wrapped round M, divided by M.  A power-of-two
    ``nfft`` has none: two empty arrays."""
    code, n = _prec_code(precision), ct.c_int32(0)
    check(lib().rsp_mtd_table(int(nfft), code, None, 0, ct.byref(n)))
    t = np.empty(2 * max(n.value, 1), np.float64)
    check(lib().rsp_mtd_table(int(nfft), code, _dptr(t), n.value, ct.byref(n)))
    t = t[:2 * n.value].view(np.complex128)
    k = int(nfft) if n.value else 0
    return t[:k].copy(), t[k:].copy()


def describe_dbf_table(config, cfar_params, cluster_params, precomputed_data, precision='c128', ncu=256):
    """The A operands a plan of these arguments uploads for K1, without a device
    (rsp_plan_describe_dbf_table): as ``dbf_table(W, True, 'split')``."""
    keep = []
    cfg, cfar, cluster, pre = _marshal(config, cfar_params, cluster_params, precomputed_data, keep)
    opt = _options(0, 1, precision, False, 'amplitude')
    return _table(lambda out, cap, n: lib().rsp_plan_describe_dbf_table(
        ct.byref(cfg), ct.byref(cfar), ct.byref(cluster), ct.byref(pre), ct.byref(opt), int(ncu), out, cap, n))


class Plan:
    """One device plan = the reference's per-frame kernel bound to fixed config/precompute.

    Parameters mirror ``fun_process_single_frame(targets, config, cfar_params,
    cluster_params, precomputed_data, frame_idx)`` (fun_process_single_frame.m:13).
    ``precision``: 'c128' (complex double, MATLAB's arithmetic; default) or 'c64'.
    ``k1_tiled``: force the one-tile-per-workgroup K1 (parity tests compare it with the
    persistent K1 the plan otherwise picks).
    ``monopulse``: 'amplitude' (fsf:282-290, the default) or 'complex' -- S9's angle from
    real((S_A - S_B) / (S_A + S_B + eps)) of the complex map, the estimator of the inline S9 in
    main_plot_snr_vs_angle_error.m:455-462 (RSP_PLAN_MONOPULSE_COMPLEX).
    ``k2_all_rows``: pulse-compress every Doppler row of every frame (RSP_PLAN_K2_ALL_ROWS) instead
    of the rows under test plus the edge rows a detection reads; same results, for tests and timing.
    """

    def __init__(self, config, cfar_params, cluster_params, precomputed_data, device=0, frames_per_launch=1,
                 precision='c128', k1_tiled=False, monopulse='amplitude', k2_all_rows=False):
        self.config = config
        self.cfar_params, self.cluster_params, self.precomputed_data = cfar_params, cluster_params, precomputed_data
        self.monopulse = monopulse
        self._keep = []
        self.cfg, self.cfar, self.cluster, self.pre = _marshal(config, cfar_params, cluster_params, precomputed_data,
                                                               self._keep)
        opt = _options(device, frames_per_launch, precision, k1_tiled, monopulse, k2_all_rows)
        h = ct.c_void_p()
        check(lib().rsp_plan_create_ex(ct.byref(self.cfg), ct.byref(self.cfar), ct.byref(self.cluster),
                                       ct.byref(self.pre), ct.byref(opt), ct.byref(h)))
        self.h = h
        s = _abi.Sizes()
        check(lib().rsp_query_sizes(self.h, ct.byref(s)))
        self.sizes = s
        self.P, self.N, self.C, self.B, self.G = s.P, s.N, s.C, s.B, s.G
        self.precision = precision
        self.frames_per_launch = int(frames_per_launch)   # F: frames per kernel launch (1..RSP_MAX_F)
        self.cdtype = np.complex128 if precision == 'c128' else np.complex64   # device cube / map element
        self.cube_bytes = s.cube_elems * s.elem_bytes

    def close(self):
        if getattr(self, 'h', None):
            lib().rsp_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def k1_route(self):
        """The slow-time transform this plan runs (rsp_query_k1_route): ``kernel`` ('tiled',
        'persistent', 'persistent_factored'), ``transform`` ('stockham', 'dif', 'factored',
        'direct'), ``R``, ``Q`` (P = R Q of the factored transform, else 0), ``NT``, ``Ppad``,
        ``tiles_per_wave`` (0 for the tiled kernel) and ``stage2_lgp`` (process_stage2's
        column transform: log2 P, or 0 for the direct DFT)."""
        r = _abi.K1Route()
        check(lib().rsp_query_k1_route(self.h, ct.byref(r)))
        return _route_dict(r)

    def k3_tiling(self):
        """How this plan tiles the CFAR/S9 kernel (rsp_query_k3_tiling): ``fast`` (the compile-time
        5/5/10/10 kernel with halo-less tiles, else the generic one), ``RT`` range cells under test
        per tile, ``hR`` range halo, ``W`` LDS row stride, ``n_tiles`` range tiles, ``n_bands``
        Doppler bands of ``VB`` cells under test, ``rows`` Doppler rows per tile."""
        t = _abi.K3Tiling()
        check(lib().rsp_query_k3_tiling(self.h, ct.byref(t)))
        return _tiling_dict(t)

    def k2_layout(self):
        """How this plan lays out the pulse-compression kernel (rsp_query_k2_layout): ``k2_pts`` LDS
        points per workgroup, ``wg_per_cu`` (4: k2_pc<T, 4>, 2: k2_pc<T, 2>), ``NZ``, ``nseg``,
        ``njobs``, ``nwg`` and ``segments``: for narrow, medium, long (K2_SEGMENTS) a dict of
        ``type, ga, gb, seg_lo, lo, hi, Ls, ntaps, delay, Lh, M, V, nblocks, rows_per_wg``, or None
        for a segment without gates."""
        L = _abi.K2Layout()
        check(lib().rsp_query_k2_layout(self.h, ct.byref(L)))
        return _k2_dict(L)

    def k2_records(self):
        """The pulse-compression workgroups in dispatch order (rsp_query_k2_records): an int32 array
        [nwg, 4] of ``K2_RECORD_FIELDS``, row i what workgroup i of a k2_pc launch reads."""
        return _k2_records(lambda out, cap, n: lib().rsp_query_k2_records(self.h, out, cap, n))

    def k2_row_set(self, which):
        """Row set ``which`` ('all', 'band', 'edge') of the pulse-compression launches and its record
        table (rsp_query_k2_row_set): ``(rows, records)``, rows a dict of ``n, base, split, gap, total,
        nwg`` (all 0 for 'band' / 'edge' in a plan without the band route), records as ``k2_records``."""
        return _k2_row_set(lambda rs, out, cap, n: lib().rsp_query_k2_row_set(self.h, K2_ROW_SETS[which], rs, out,
                                                                              cap, n))

    def band_counters(self, reset=False):
        """What the band route did since the last reset (rsp_band_counters_get): ``frames``,
        ``band_frames``, ``edge_rows`` computed on demand, ``deferred_cells``."""
        c = _abi.BandCounters()
        check(lib().rsp_band_counters_get(self.h, ct.byref(c)))
        if reset:
            check(lib().rsp_band_counters_reset(self.h))
        return {k: getattr(c, k) for k, _ in _abi.BandCounters._fields_}

    # ---- synchronous frame paths ---------------------------------------------------------
    def _frame_out(self, want_rdm, want_cfar):
        o = _abi.FrameOut()
        bufs = {}
        if want_rdm:
            bufs['rdm'] = np.empty((self.P, self.G, self.B), np.complex128, order='F')
            o.rdm = bufs['rdm'].ctypes.data_as(ct.POINTER(ct.c_double))
        if want_cfar and self.B > 1:
            bufs['cfar'] = np.empty((self.P, self.G, self.B - 1), np.float64, order='F')
            o.cfar_maps = _dptr(bufs['cfar'])
        # detections and final targets have no fixed count: read after the frame (rsp_last_*)
        o.dets, o.dets_cap, o.targets, o.targets_cap = None, 0, None, 0
        return o, bufs, None, None

    def last_detections(self):
        """Every detection of the last synchronous frame (rsp_last_detections; no capacity limit)."""
        n = ct.c_int32()
        check(lib().rsp_last_detections(self.h, None, 0, ct.byref(n)))
        dets = (_abi.Detection * max(n.value, 1))()
        check(lib().rsp_last_detections(self.h, dets, n.value, ct.byref(n)))
        return [_det_dict(dets[i]) for i in range(n.value)]

    def last_targets(self):
        """The final targets of the last synchronous frame (rsp_last_targets)."""
        n = ct.c_int32()
        check(lib().rsp_last_targets(self.h, None, 0, ct.byref(n)))
        tg = (_abi.Target * max(n.value, 1))()
        check(lib().rsp_last_targets(self.h, tg, n.value, ct.byref(n)))
        return [_tgt_dict(tg[i]) for i in range(n.value)]

    def _collect(self, o, bufs, dets, tg, want_threshold=False):
        res = {'final_targets': self.last_targets(), 'detections': self.last_detections()}
        assert len(res['detections']) == o.n_dets and len(res['final_targets']) == o.n_targets
        if 'rdm' in bufs:
            res['rdm'] = bufs['rdm']
        if 'cfar' in bufs:
            res['cfar_maps'] = bufs['cfar']
        if want_threshold:
            t = self.last_cfar_threshold(want_hits=False)
            res['cfar_threshold'], res['cfar_flags'] = t['threshold'], t['flags']
        return res

    def process_cube(self, cube, frame_idx=1, want_rdm=False, want_cfar=False, want_threshold=False):
        """S5..S11 on a noisy echo cube ``cube[m, n, c]`` (MATLAB [P x N x C]).  ``cfar_maps``
        (want_cfar) is rdm_for_cfar_all as the device's K3 thresholds it (fsf:184-187).
        ``want_threshold`` implies ``want_cfar`` and adds ``cfar_threshold`` and ``cfar_flags``
        [P, G, B - 1]: ``last_cfar_threshold`` on those maps."""
        cube = np.asarray(cube)
        if cube.shape != (self.P, self.N, self.C):
            raise ValueError('cube shape %r != (P, N, C) = %r' % (cube.shape, (self.P, self.N, self.C)))
        a, ap, dt = _complex_arg(cube)
        o, bufs, dets, tg = self._frame_out(want_rdm, want_cfar or want_threshold)
        check(lib().rsp_process_cube(self.h, ap, dt, _abi.RSP_LAYOUT_PNC, int(frame_idx), ct.byref(o)))
        return self._collect(o, bufs, dets, tg, want_threshold)

    def process_targets(self, targets, frame_idx=1, seed=20250101, p_noise=1.0, want_rdm=False, want_cfar=False,
                        want_threshold=False):
        """fsf:13 path: device S4 synthesis + S4.1 Philox noise + S5..S11.  ``want_threshold`` as
        ``process_cube``."""
        tin = self._targets_in(targets)
        o, bufs, dets, tg = self._frame_out(want_rdm, want_cfar or want_threshold)
        check(lib().rsp_process_targets(self.h, tin, len(targets), int(frame_idx), int(seed), float(p_noise),
                                        ct.byref(o)))
        return self._collect(o, bufs, dets, tg, want_threshold)

    @staticmethod
    def _targets_in(targets):
        arr = (_abi.TargetIn * max(len(targets), 1))()
        for i, t in enumerate(targets):
            arr[i] = _abi.TargetIn(t['Range'], t['Velocity'], t['ElevationAngle'], t['SNR_dB'])
        return arr

    def process_stage2(self, iq_beams, gate_cols=None):
        """process_stage2_mtd backing: beams ``iq[m, n, b]`` -> (MTD [P,G,B], PC [P,G,B]).
        ``gate_cols``: ((first, last), ...) 1-based PRT columns of the segments of a gated
        input (rsp_process_stage2_gated); None: ``n`` is the full PRT."""
        iq = np.asarray(iq_beams)
        a, ap, dt = _complex_arg(iq)
        mtd = np.empty((self.P, self.G, self.B), np.complex128, order='F')
        pc = np.empty((self.P, self.G, self.B), np.complex128, order='F')
        mo, po = mtd.ctypes.data_as(ct.POINTER(ct.c_double)), pc.ctypes.data_as(ct.POINTER(ct.c_double))
        if gate_cols is None:
            if iq.shape != (self.P, self.N, self.B):
                raise ValueError('iq shape %r != (P, N, B) = %r' % (iq.shape, (self.P, self.N, self.B)))
            check(lib().rsp_process_stage2(self.h, ap, dt, mo, po))
        else:
            cols = _gate_cols_arg(gate_cols)
            if iq.shape[0] != self.P or iq.shape[2] != self.B:
                raise ValueError('iq shape %r: expected (P, n, B) with P=%d B=%d' % (iq.shape, self.P, self.B))
            check(lib().rsp_process_stage2_gated(self.h, ap, dt, iq.shape[1], cols, mo, po))
        return mtd, pc

    def _stage2_detect(self, iq, nch, gate_cols, prm, want, hits_cap, full_fn, gated_fn=None, raw=None):
        """The fused stage-2 + detector calls: ``iq`` [P, n, nch] (beams, or the raw cube with ``raw`` =
        (W pointer or None, conj)), ``prm`` the detector's C parameters, ``full_fn`` / ``gated_fn`` the C
        entries of the beams forms (raw: ``full_fn`` takes n_gated and cols itself).  Returns the dict
        ``process_stage2_cfar`` documents."""
        want = set(want)
        if not want <= set(STAGE3_WANT):
            raise ValueError('want: unknown output(s) %r' % (sorted(want - set(STAGE3_WANT)),))
        iq = np.asarray(iq)
        what = ('iq', 'B') if raw is None else ('cube', 'C')
        a, iqp, dt = _complex_arg(iq)
        shp = (self.P, self.G, self.B)
        if gate_cols is None and iq.shape != (self.P, self.N, nch):
            raise ValueError('%s shape %r != (P, N, %s) = %r' % (what[0], iq.shape, what[1], (self.P, self.N, nch)))
        if gate_cols is not None and (iq.ndim != 3 or iq.shape[0] != self.P or iq.shape[2] != nch):
            raise ValueError('%s shape %r: expected (P, n, %s) with P=%d %s=%d'
                             % (what[0], iq.shape, what[1], self.P, what[1], nch))
        res, ptr = {}, {}
        for name, dtype in (('mtd', np.complex128), ('amp', np.float64), ('flags', np.uint8), ('threshold', np.float64)):
            if name in want:
                res[name] = np.empty(shp, dtype, order='F')
                ptr[name] = res[name].ctypes.data_as(ct.POINTER(ct.c_uint8 if name == 'flags' else ct.c_double))
            else:
                ptr[name] = None
        total = ct.c_int64()

        def call(cap, hp, maps):
            m = ptr if maps else dict.fromkeys(ptr)
            tail = (ct.byref(prm), m['mtd'], m['amp'], m['flags'], m['threshold'], hp, cap, ct.byref(total))
            if raw is not None:
                ng, cols = (0, None) if gate_cols is None else (iq.shape[1], _gate_cols_arg(gate_cols))
                check(full_fn(self.h, iqp, dt, ng, cols, raw[0], raw[1], *tail))
            elif gate_cols is None:
                check(full_fn(self.h, iqp, dt, *tail))
            else:
                check(gated_fn(self.h, iqp, dt, iq.shape[1], _gate_cols_arg(gate_cols), *tail))
            return total.value

        res['n_hits'], hits = _with_hits(call, max(4096, self.P * self.G * self.B // 8), hits_cap, 'hits' in want)
        if 'hits' in want:
            res['hits'] = hits
        return res

    # ---- stage-3 range CFAR of the stage-2 path ---------------------------------------------
    def stage3_cfar(self, amp, cfar, segments=None, hits_cap=None, want_hits=True):
        """local_execute_cfar (debug_simulated_data_processing_v2.m:419-511) on real amplitude maps
        ``amp`` [P, G] or [P, G, n] (rsp_stage3_cfar; include/rsp.h restates the semantics).
        ``cfar``: refCells_R, saveCells_R, T_CFAR, CFARmethod_R, MTD_0v_num.  ``segments``:
        (narrow, medium, long) column counts of a map whose shape is not the plan's
        (rsp_stage3_cfar_shape); None: the plan's P and gate counts.  Returns ``flags`` (uint8) and
        ``threshold`` (float64) shaped like ``amp``, ``n_hits`` and ``hits``: a HIT_DTYPE array in
        beam-then-find() order, all of them, or the first ``hits_cap``."""
        a = np.asarray(amp, np.float64)
        shape = a.shape
        if a.ndim == 2:
            a = a[:, :, None]
        if a.ndim != 3:
            raise ValueError('amp must be [P, G] or [P, G, n], got shape %r' % (shape,))
        P, G, n = a.shape
        if segments is None:
            if (P, G) != (self.P, self.G):
                raise ValueError('amp shape %r: expected (P, G) = %r (or give segments)' % (shape, (self.P, self.G)))
        elif sum(int(x) for x in segments) != G:
            raise ValueError('segments %r do not add up to the %d columns of amp' % (tuple(segments), G))
        a = np.asfortranarray(a)
        prm = _stage3_params(cfar)
        flags = np.empty((P, G, n), np.uint8, order='F')
        thr = np.empty((P, G, n), np.float64, order='F')
        fp_, tp = flags.ctypes.data_as(ct.POINTER(ct.c_uint8)), _dptr(thr)
        total = ct.c_int64()

        def call(cap, hp, maps):
            tail = (_dptr(a), n, ct.byref(prm), fp_ if maps else None, tp if maps else None, hp, cap, ct.byref(total))
            if segments is None:
                check(lib().rsp_stage3_cfar(self.h, *tail))
            else:
                gates = (ct.c_int32 * 3)(*[int(x) for x in segments])
                check(lib().rsp_stage3_cfar_shape(self.h, P, gates, *tail))
            return total.value

        n_hits, hits = _with_hits(call, max(4096, a.size // 8), hits_cap, want_hits)
        return dict(flags=flags.reshape(shape, order='F'), threshold=thr.reshape(shape, order='F'),
                    n_hits=n_hits, hits=hits)

    def process_stage2_cfar(self, iq_beams, cfar, gate_cols=None, want=STAGE3_WANT, hits_cap=None):
        """process_stage2_mtd followed by the stage-3 range CFAR on |MTD_results| of every beam,
        without leaving the device (rsp_process_stage2_cfar / _gated_cfar).  ``iq_beams`` and
        ``gate_cols`` as ``process_stage2``; ``cfar`` as ``stage3_cfar``.  ``want`` names the
        outputs to bring back: 'mtd' (complex [P, G, B]), 'amp' (the map that was tested), 'flags'
        (uint8), 'threshold', 'hits' (HIT_DTYPE array, beam then find() order; with ``hits_cap``
        its first entries); ``n_hits`` always.  A call that wants the hits alone downloads nothing
        else."""
        return self._stage2_detect(iq_beams, self.B, gate_cols, _stage3_params(cfar), want, hits_cap,
                                   lib().rsp_process_stage2_cfar, lib().rsp_process_stage2_gated_cfar)

    def profile_stage3(self, cfar, iters=20):
        """HIP-event time of k_s3_cfar over the B beams of the plan's last stage-2 result
        (rsp_profile_stage3): {'real': (ms, bytes), 'fused_all': ..., 'fused_hits': ...} -- the
        real-amplitude form writing flags and thresholds, the complex form writing amplitudes,
        flags and thresholds, and the complex form with the hit list alone."""
        prm = _stage3_params(cfar)
        ms, by = (ct.c_float * 3)(), (ct.c_int64 * 3)()
        check(lib().rsp_profile_stage3(self.h, ct.byref(prm), int(iters), ms, by))
        return {k: (ms[i], by[i]) for i, k in enumerate(('real', 'fused_all', 'fused_hits'))}

    # ---- Doppler CA-CFAR of the stage-2 path --------------------------------------------------
    def doppler_cfar(self, amp, cfar, method='ca', hits_cap=None, want_hits=True):
        """local_cfar_detector (main_simulate_echoes_with_array_v3.m:278-314) on real amplitude maps
        ``amp`` [P, G] or [P, G, n] of any shape (rsp_vcfar; include/rsp.h restates the semantics):
        the plan gives the device and the precision.  ``cfar``: refCells_V, guardCells_V, T_CFAR;
        ``method``: 'ca' (the reference), 'goca' or 'soca'.  Returns ``flags`` (uint8) and
        ``threshold`` (float64) shaped like ``amp``, ``n_hits`` and ``hits``: a HIT_DTYPE array in
        map-then-find() order, all of them, or the first ``hits_cap``."""
        a = np.asarray(amp, np.float64)
        shape = a.shape
        if a.ndim == 2:
            a = a[:, :, None]
        if a.ndim != 3:
            raise ValueError('amp must be [P, G] or [P, G, n], got shape %r' % (shape,))
        P, G, n = a.shape
        a = np.asfortranarray(a)
        prm = _vcfar_params(cfar, method)
        flags = np.empty((P, G, n), np.uint8, order='F')
        thr = np.empty((P, G, n), np.float64, order='F')
        fp_, tp = flags.ctypes.data_as(ct.POINTER(ct.c_uint8)), _dptr(thr)
        total = ct.c_int64()

        def call(cap, hp, maps):
            check(lib().rsp_vcfar(self.h, P, G, _dptr(a), n, ct.byref(prm), fp_ if maps else None, tp if maps else None,
                                  hp, cap, ct.byref(total)))
            return total.value

        n_hits, hits = _with_hits(call, max(4096, a.size // 8), hits_cap, want_hits)
        return dict(flags=flags.reshape(shape, order='F'), threshold=thr.reshape(shape, order='F'),
                    n_hits=n_hits, hits=hits)

    def process_stage2_vcfar(self, iq_beams, cfar, method='ca', gate_cols=None, want=STAGE3_WANT, hits_cap=None):
        """process_stage2_mtd followed by the Doppler CA-CFAR on |MTD_results| of every beam, without
        leaving the device (rsp_process_stage2_vcfar / _gated_vcfar).  ``iq_beams``, ``gate_cols``,
        ``want`` and ``hits_cap`` as ``process_stage2_cfar``; ``cfar`` and ``method`` as
        ``doppler_cfar``."""
        return self._stage2_detect(iq_beams, self.B, gate_cols, _vcfar_params(cfar, method), want, hits_cap,
                                   lib().rsp_process_stage2_vcfar, lib().rsp_process_stage2_gated_vcfar)

    def profile_vcfar(self, cfar, method='ca', iters=20):
        """HIP-event time of k_vcfar over the B beams of the plan's last stage-2 result
        (rsp_profile_vcfar), in the three forms of ``profile_stage3``."""
        prm = _vcfar_params(cfar, method)
        ms, by = (ct.c_float * 3)(), (ct.c_int64 * 3)()
        check(lib().rsp_profile_vcfar(self.h, ct.byref(prm), int(iters), ms, by))
        return {k: (ms[i], by[i]) for i, k in enumerate(('real', 'fused_all', 'fused_hits'))}

    # ---- cross GOCA-CFAR as a map detector ------------------------------------------------------
    def cross_cfar(self, amp, cfar, hits_cap=None, want_hits=True):
        """fun_run_goca_cfar_8's test (fsf:192-213) on real amplitude maps ``amp`` [P, G] or [P, G, n]
        of any shape (rsp_xcfar; include/rsp.h restates the semantics): the plan gives the device and
        the precision.  ``cfar``: refCells_R, guardCells_R, refCells_V, guardCells_V, T_CFAR.  Returns
        ``flags`` (uint8) and ``threshold`` (float64, +Inf where the reference tests no cell) shaped
        like ``amp``, ``n_hits`` and ``hits``: a HIT_DTYPE array in map-then-find() order, all of them,
        or the first ``hits_cap``."""
        a = np.asarray(amp, np.float64)
        shape = a.shape
        if a.ndim == 2:
            a = a[:, :, None]
        if a.ndim != 3:
            raise ValueError('amp must be [P, G] or [P, G, n], got shape %r' % (shape,))
        P, G, n = a.shape
        a = np.asfortranarray(a)
        prm = _xcfar_params(cfar)
        flags = np.empty((P, G, n), np.uint8, order='F')
        thr = np.empty((P, G, n), np.float64, order='F')
        fp_, tp = flags.ctypes.data_as(ct.POINTER(ct.c_uint8)), _dptr(thr)
        total = ct.c_int64()

        def call(cap, hp, maps):
            check(lib().rsp_xcfar(self.h, P, G, _dptr(a), n, ct.byref(prm), fp_ if maps else None, tp if maps else None,
                                  hp, cap, ct.byref(total)))
            return total.value

        n_hits, hits = _with_hits(call, max(4096, a.size // 8), hits_cap, want_hits)
        return dict(flags=flags.reshape(shape, order='F'), threshold=thr.reshape(shape, order='F'),
                    n_hits=n_hits, hits=hits)

    def process_stage2_xcfar(self, iq_beams, cfar, gate_cols=None, want=STAGE3_WANT, hits_cap=None):
        """process_stage2_mtd followed by the cross GOCA-CFAR on |MTD_results| of every beam, without
        leaving the device (rsp_process_stage2_xcfar / _gated_xcfar).  ``iq_beams``, ``gate_cols``,
        ``want`` and ``hits_cap`` as ``process_stage2_cfar``; ``cfar`` as ``cross_cfar``."""
        return self._stage2_detect(iq_beams, self.B, gate_cols, _xcfar_params(cfar), want, hits_cap,
                                   lib().rsp_process_stage2_xcfar, lib().rsp_process_stage2_gated_xcfar)

    def last_cfar_threshold(self, hits_cap=None, want_hits=True):
        """The threshold K3 tested every cell of the last synchronous frame against
        (rsp_last_cfar_threshold): the cross GOCA-CFAR with the plan's own cfar_params on the pair-sum
        maps of that frame, which must have asked for them (``want_cfar``).  Returns ``flags`` and
        ``threshold`` [P, G, B - 1], ``n_hits`` and ``hits`` as ``cross_cfar``, beam_idx = the pair."""
        shp = (self.P, self.G, max(self.B - 1, 1))
        flags, thr = np.empty(shp, np.uint8, order='F'), np.empty(shp, np.float64, order='F')
        fp_, tp = flags.ctypes.data_as(ct.POINTER(ct.c_uint8)), _dptr(thr)
        total = ct.c_int64()

        def call(cap, hp, maps):
            check(lib().rsp_last_cfar_threshold(self.h, fp_ if maps else None, tp if maps else None, hp, cap,
                                                ct.byref(total)))
            return total.value

        n_hits, hits = _with_hits(call, max(4096, flags.size // 8), hits_cap, want_hits)
        return dict(flags=flags, threshold=thr, n_hits=n_hits, hits=hits)

    def profile_xcfar(self, cfar, iters=20):
        """HIP-event time of k_xcfar over the B beams of the plan's last stage-2 result
        (rsp_profile_xcfar), in the three forms of ``profile_stage3``."""
        prm = _xcfar_params(cfar)
        ms, by = (ct.c_float * 3)(), (ct.c_int64 * 3)()
        check(lib().rsp_profile_xcfar(self.h, ct.byref(prm), int(iters), ms, by))
        return {k: (ms[i], by[i]) for i, k in enumerate(('real', 'fused_all', 'fused_hits'))}

    # ---- stage-1 DBF of the stage-2 path, and stage 2 on the raw cube ----------------------------
    def dbf(self, cube, W, conj=True, out=None):
        """The stage-2 scripts' DBF loop (rsp_dbf; include/rsp.h restates the semantics): raw
        ``cube[m, n, c]`` of any shape [P, N, C] and weights ``W`` [B, C] (DBF_coeffs_data_C) ->
        beams [P, N, B] complex128, ``cube[m, n, :] @ W'`` (``conj``, debug_simulated_data_processing.m:
        166-175) or ``@ W.'`` (main_test_with_simulated_data.m:207-214).  The plan gives the device and
        the precision only.  ``out``: a Fortran-contiguous complex128 [P, N, B] array to write into."""
        cube = np.asarray(cube)
        W = np.asarray(W, np.complex128)
        if cube.ndim == 2:
            cube = cube[:, :, None]
        if cube.ndim != 3 or W.ndim != 2 or W.shape[1] != cube.shape[2]:
            raise ValueError('cube %r and W %r: expected [P, N, C] and [B, C]' % (cube.shape, W.shape))
        a, ap, dt = _complex_arg(cube)
        P, N, C = cube.shape
        B = W.shape[0]
        Wcm = np.asfortranarray(W).ravel(order='F').view(np.float64)   # B x C column-major (MATLAB)
        if out is None:
            out = np.empty((P, N, B), np.complex128, order='F')
        elif out.shape != (P, N, B) or out.dtype != np.complex128 or not out.flags.f_contiguous:
            raise ValueError('out must be a Fortran-contiguous complex128 array of shape %r' % ((P, N, B),))
        check(lib().rsp_dbf(self.h, P, N, C, B, ap, dt, _dptr(Wcm), 1 if conj else 0,
                            out.ctypes.data_as(ct.POINTER(ct.c_double))))
        return out

    def profile_dbf(self, P, N, C, B, iters=20):
        """HIP-event time of k_dbf alone on a [P, N, C] cube into B beams (rsp_profile_dbf):
        {'stage', 'ms', 'bytes'}, bytes = element bytes x P N x (C + B)."""
        ms, by = ct.c_float(), ct.c_int64()
        check(lib().rsp_profile_dbf(self.h, int(P), int(N), int(C), int(B), int(iters), ct.byref(ms), ct.byref(by)))
        return {'stage': 'k_dbf', 'ms': float(ms.value), 'bytes': int(by.value)}

    # ---- the MTD as a stand-alone stage: a slow-time transform of any length ----------------------
    @staticmethod
    def _mtd_win(win, P):
        if win is None:
            return None, None
        w = np.ascontiguousarray(np.asarray(win, np.float64).ravel())
        if w.size != P:
            raise ValueError('win has %d entries, the cube %d pulses' % (w.size, P))
        return w, _dptr(w)

    def mtd(self, pc, win=None, nfft=None, shift=True, out=None):
        """``fftshift(fft(pc .* win, nfft, 1), 1)`` (rsp_mtd; v7_7:501-503, fsf:131-135): ``pc`` [P, G]
        or [P, G, n_maps] of any shape, ``win`` P reals (None: none), ``nfft`` any length P ..
        RSP_MTD_MAX_NFFT (None: P), ``shift`` False for natural order -> complex128 [nfft, G(, n_maps)].
        The plan gives the device and the precision only.  ``out``: a Fortran-contiguous complex128
        array of the result's shape to write into."""
        pc = np.asarray(pc)
        if pc.ndim not in (2, 3):
            raise ValueError('pc %r: expected [P, G] or [P, G, n_maps]' % (pc.shape,))
        a, ap, dt = _complex_arg(pc)
        P, G = pc.shape[:2]
        n_maps = pc.shape[2] if pc.ndim == 3 else 1
        n = int(nfft) if nfft else P
        wk, wp = self._mtd_win(win, P)
        shp = (n,) + pc.shape[1:]
        if out is None:
            out = np.empty(shp, np.complex128, order='F')
        elif out.shape != shp or out.dtype != np.complex128 or not out.flags.f_contiguous:
            raise ValueError('out must be a Fortran-contiguous complex128 array of shape %r' % (shp,))
        check(lib().rsp_mtd(self.h, P, G, n_maps, n, ap, dt, wp, 1 if shift else 0, _dptr(out)))
        return out

    def mtd_device(self, d_pc, d_out, P, G, n_maps=1, win=None, nfft=None, shift=True):
        """The same on device memory in the plan's precision (rsp_mtd_device): ``d_pc`` [P, G, n_maps]
        -> ``d_out`` [nfft, G, n_maps], pulse index fastest; the two must not overlap."""
        wk, wp = self._mtd_win(win, int(P))
        check(lib().rsp_mtd_device(self.h, int(P), int(G), int(n_maps), int(nfft or 0), ct.c_void_p(d_pc), wp,
                                   1 if shift else 0, ct.c_void_p(d_out)))

    def profile_mtd(self, P, G, n_maps=1, nfft=None, iters=20):
        """HIP-event time of k_mtd_any alone on a [P, G, n_maps] cube of zeros (rsp_profile_mtd):
        {'stage', 'ms', 'bytes'}, bytes = element bytes x G n_maps x (P + nfft)."""
        ms, by = ct.c_float(), ct.c_int64()
        check(lib().rsp_profile_mtd(self.h, int(P), int(G), int(n_maps), int(nfft or 0), int(iters), ct.byref(ms),
                                    ct.byref(by)))
        return {'stage': 'k_mtd_any', 'ms': float(ms.value), 'bytes': int(by.value)}

    # ---- detection on any RD cube: pair sums, cross CFAR, S9, clustering ---------------------------
    def _detect_params(self, V, G, B, cfar, cluster, range_axis, velocity_axis, deltaR, deltaV, beam_angles_deg,
                       k_slopes_LUT, monopulse):
        """rsp_detect_params for a [V, G, B] cube; every None falls back to the plan's own where the
        shape agrees (range_axis: G == plan.G, velocity_axis: V == plan.P, angles and K-LUT: B == plan.B).
        Returns (struct, the arrays it borrows)."""
        pre = self.precomputed_data

        def pick(x, name, n, own_n):
            if x is None:
                if n != own_n:
                    raise ValueError('%s is needed: the cube has %d entries along it, the plan %d' % (name, n, own_n))
                x = pre[name]
            a = np.ascontiguousarray(np.asarray(x, np.float64).ravel())
            if a.size != n:
                raise ValueError('%s has %d entries, expected %d' % (name, a.size, n))
            return a if a.size else np.zeros(1)

        cfar = self.cfar_params if cfar is None else cfar
        cluster = self.cluster_params if cluster is None else cluster
        monopulse = self.monopulse if monopulse is None else monopulse
        if monopulse not in ('amplitude', 'complex'):
            raise ValueError("monopulse must be 'amplitude' or 'complex', got %r" % (monopulse,))
        keep = [pick(range_axis, 'range_axis', G, self.G), pick(velocity_axis, 'velocity_axis', V, self.P),
                pick(beam_angles_deg, 'beam_angles_deg', B, self.B), pick(k_slopes_LUT, 'k_slopes_LUT', B - 1, self.B - 1)]
        prm = _abi.DetectParams(
            cfar=_xcfar_params(cfar),
            cluster=_abi.ClusterParams(max_range_sep=cluster['max_range_sep'], max_vel_sep=cluster['max_vel_sep'],
                                       max_angle_sep=cluster['max_angle_sep']),
            range_axis=_dptr(keep[0]), velocity_axis=_dptr(keep[1]),
            deltaR=float(pre['deltaR'] if deltaR is None else deltaR),
            deltaV=float(pre['deltaV'] if deltaV is None else deltaV),
            beam_angles_deg=_dptr(keep[2]), k_slopes_LUT=_dptr(keep[3]), monopulse=1 if monopulse == 'complex' else 0)
        return prm, keep

    def _detect_out(self, V, G, B, want_cfar, rdm_shape=None):
        o, bufs = _abi.FrameOut(), {}
        if rdm_shape is not None:
            bufs['rdm'] = np.empty(rdm_shape, np.complex128, order='F')
            o.rdm = bufs['rdm'].ctypes.data_as(ct.POINTER(ct.c_double))
        if want_cfar:
            bufs['cfar'] = np.empty((V, G, B - 1), np.float64, order='F')
            o.cfar_maps = _dptr(bufs['cfar'])
        o.dets, o.dets_cap, o.targets, o.targets_cap = None, 0, None, 0   # no fixed count: rsp_last_*
        return o, bufs

    @staticmethod
    def _cube3(a, what):
        a = np.asarray(a)
        if a.ndim != 3 or a.shape[2] < 2:
            raise ValueError('%s %r: expected [rows, G, B] with B >= 2' % (what, a.shape))
        return a

    def detect(self, rdm, cfar=None, cluster=None, range_axis=None, velocity_axis=None, deltaR=None, deltaV=None,
               beam_angles_deg=None, k_slopes_LUT=None, monopulse=None, want_cfar=False):
        """fsf S8-S11 (fun_run_goca_cfar_8, fun_parameter_estimation_9, the two clustering stages) on a
        complex RD cube ``rdm`` [V, G, B] of any shape (rsp_detect; include/rsp.h restates the semantics):
        the plan gives the device and the precision, and its own ``cfar`` / ``cluster`` parameters, axes,
        cell sizes, angles, K-LUT and ``monopulse`` ('amplitude' / 'complex') wherever the argument is
        None and the shape agrees.  Returns ``detections`` and ``final_targets`` as ``process_cube``, and
        with ``want_cfar`` ``cfar_maps`` [V, G, B - 1]."""
        rdm = self._cube3(rdm, 'rdm')
        V, G, B = rdm.shape
        prm, keep = self._detect_params(V, G, B, cfar, cluster, range_axis, velocity_axis, deltaR, deltaV,
                                        beam_angles_deg, k_slopes_LUT, monopulse)
        a, ap, dt = _complex_arg(rdm)
        o, bufs = self._detect_out(V, G, B, want_cfar)
        check(lib().rsp_detect(self.h, V, G, B, ap, dt, ct.byref(prm), ct.byref(o)))
        return self._collect(o, bufs, None, None)

    def detect_device(self, d_rdm, V, G, B, cfar=None, cluster=None, range_axis=None, velocity_axis=None, deltaR=None,
                      deltaV=None, beam_angles_deg=None, k_slopes_LUT=None, monopulse=None, want_cfar=False):
        """The same on a device cube [V, G, B] in the plan's precision and MATLAB's layout, Doppler index
        fastest (rsp_detect_device): ``mtd_device``'s output."""
        V, G, B = int(V), int(G), int(B)
        prm, keep = self._detect_params(V, G, B, cfar, cluster, range_axis, velocity_axis, deltaR, deltaV,
                                        beam_angles_deg, k_slopes_LUT, monopulse)
        o, bufs = self._detect_out(V, G, B, want_cfar)
        check(lib().rsp_detect_device(self.h, V, G, B, ct.c_void_p(d_rdm), ct.byref(prm), ct.byref(o)))
        return self._collect(o, bufs, None, None)

    def mtd_detect(self, pc, win=None, nfft=None, cfar=None, cluster=None, range_axis=None, velocity_axis=None,
                   deltaR=None, deltaV=None, beam_angles_deg=None, k_slopes_LUT=None, monopulse=None, want_rdm=False,
                   want_cfar=False):
        """``mtd`` of ``pc`` [P, G, B] to ``nfft`` rows and ``detect`` on the result without leaving the
        device (rsp_mtd_detect; v7_7 sections 7-10): ``velocity_axis`` has nfft entries.  ``want_rdm`` adds
        the cube ``rdm`` [nfft, G, B]."""
        pc = self._cube3(pc, 'pc')
        P, G, B = pc.shape
        n = int(nfft) if nfft else P
        prm, keep = self._detect_params(n, G, B, cfar, cluster, range_axis, velocity_axis, deltaR, deltaV,
                                        beam_angles_deg, k_slopes_LUT, monopulse)
        wk, wp = self._mtd_win(win, P)
        a, ap, dt = _complex_arg(pc)
        o, bufs = self._detect_out(n, G, B, want_cfar, (n, G, B) if want_rdm else None)
        check(lib().rsp_mtd_detect(self.h, P, G, B, n, ap, dt, wp, ct.byref(prm), ct.byref(o)))
        return self._collect(o, bufs, None, None)

    def process_stage2_detect(self, iq_beams, gate_cols=None, want_rdm=False, want_cfar=False):
        """process_stage2_mtd followed by ``detect`` on MTD_results without leaving the device, with the
        plan's own parameters (rsp_process_stage2_detect).  ``iq_beams`` and ``gate_cols`` as
        ``process_stage2`` (a gated input is put back at its PRT columns here); ``want_rdm`` adds
        MTD_results as ``rdm`` [P, G, B]."""
        iq = np.asarray(iq_beams)
        if gate_cols is not None:
            if iq.ndim != 3 or iq.shape[0] != self.P or iq.shape[2] != self.B:
                raise ValueError('iq shape %r: expected (P, n, B) with P=%d B=%d' % (iq.shape, self.P, self.B))
            cols = np.concatenate([np.arange(f - 1, l) for f, l in gate_cols])
            if cols.size != iq.shape[1] or cols.min() < 0 or cols.max() >= self.N:
                raise ValueError('gate_cols cover %d columns of a %d-sample PRT, the input has %d' % (cols.size, self.N, iq.shape[1]))
            full = np.zeros((self.P, self.N, self.B), iq.dtype if iq.dtype == np.complex64 else np.complex128, order='F')
            full[:, cols, :] = iq
            iq = full
        if iq.shape != (self.P, self.N, self.B):
            raise ValueError('iq shape %r != (P, N, B) = %r' % (iq.shape, (self.P, self.N, self.B)))
        a, ap, dt = _complex_arg(iq)
        o, bufs = self._detect_out(self.P, self.G, self.B, want_cfar and self.B > 1,
                                   (self.P, self.G, self.B) if want_rdm else None)
        check(lib().rsp_process_stage2_detect(self.h, ap, dt, ct.byref(o)))
        return self._collect(o, bufs, None, None)

    def profile_detect(self, V, G, B, cfar=None, iters=20):
        """HIP-event times of the detector's three kernels on the library's test cube of [V, G, B]
        (rsp_profile_detect): {'k_pairsum' | 'k_xcfar' | 'k_s9': (ms, bytes)}."""
        prm = _xcfar_params(self.cfar_params if cfar is None else cfar)
        ms, by = (ct.c_float * 3)(), (ct.c_int64 * 3)()
        check(lib().rsp_profile_detect(self.h, int(V), int(G), int(B), ct.byref(prm), int(iters), ms, by))
        return {k: (float(ms[i]), int(by[i])) for i, k in enumerate(('k_pairsum', 'k_xcfar', 'k_s9'))}

    # ---- pulse compression as a stand-alone stage: any pulse count, any beam count -----------------
    def pc_layout(self, P, B):
        """How the three launches of ``pulse_compress`` cover ``P`` pulses of ``B`` beams
        (rsp_query_pc): the fields of rsp_pc_info as a dict, as ``describe_pc``."""
        info = _abi.PcInfo()
        check(lib().rsp_query_pc(self.h, int(P), int(B), ct.byref(info)))
        return _pc_dict(info)

    def _beams3(self, a, what='iq_beams'):
        a = np.asarray(a)
        if a.ndim == 2:
            a = a[:, :, None]
        if a.ndim != 3 or a.shape[1] != self.N:
            raise ValueError('%s %r: expected [P, N, B] with N=%d' % (what, a.shape, self.N))
        return a

    def pulse_compress(self, iq_beams, out=None):
        """Section 6 of main_simulate_echoes_with_array_v7_7.m (fsf:99-127) on a beam cube ``iq_beams``
        [P, N, B] with any pulse count P and any beam count B, taken from the array's shape
        (rsp_pc): -> PC_results [P, G, B] complex128.  The plan gives the device, the precision, N, the
        gate layout and the filter tables; its own prtNum and beam_num play no part.  ``out``: a
        Fortran-contiguous complex128 [P, G, B] array to write into."""
        iq = self._beams3(iq_beams)
        P, _, B = iq.shape
        a, ap, dt = _complex_arg(iq)
        shp = (P, self.G, B)
        if out is None:
            out = np.empty(shp, np.complex128, order='F')
        elif out.shape != shp or out.dtype != np.complex128 or not out.flags.f_contiguous:
            raise ValueError('out must be a Fortran-contiguous complex128 array of shape %r' % (shp,))
        check(lib().rsp_pc(self.h, P, B, ap, dt, _dptr(out)))
        return out

    def pulse_compress_device(self, d_beams, d_pc, P, B):
        """The same on device memory in the plan's precision (rsp_pc_device): ``d_beams`` [P, N, B] ->
        ``d_pc`` [P, G, B], pulse index fastest on both sides (what ``mtd_device`` reads); the two must
        not overlap."""
        check(lib().rsp_pc_device(self.h, int(P), int(B), ct.c_void_p(d_beams), ct.c_void_p(d_pc)))

    def pc_mtd_detect(self, iq_beams, win=None, nfft=None, cfar=None, cluster=None, range_axis=None, velocity_axis=None,
                      deltaR=None, deltaV=None, beam_angles_deg=None, k_slopes_LUT=None, monopulse=None, want_rdm=False,
                      want_cfar=False):
        """``mtd_detect(pulse_compress(iq_beams), ...)`` without leaving the device (rsp_pc_mtd_detect; v7_7
        sections 6-10): ``iq_beams`` [P, N, B], the rest as ``mtd_detect``."""
        iq = self._beams3(iq_beams)
        P, _, B = iq.shape
        G, n = self.G, int(nfft) if nfft else P
        prm, keep = self._detect_params(n, G, B, cfar, cluster, range_axis, velocity_axis, deltaR, deltaV,
                                        beam_angles_deg, k_slopes_LUT, monopulse)
        wk, wp = self._mtd_win(win, P)
        a, ap, dt = _complex_arg(iq)
        o, bufs = self._detect_out(n, G, B, want_cfar, (n, G, B) if want_rdm else None)
        check(lib().rsp_pc_mtd_detect(self.h, P, B, n, ap, dt, wp, ct.byref(prm), ct.byref(o)))
        return self._collect(o, bufs, None, None)

    def raw_detect(self, cube, W=None, conj=True, win=None, nfft=None, cfar=None, cluster=None, range_axis=None,
                   velocity_axis=None, deltaR=None, deltaV=None, beam_angles_deg=None, k_slopes_LUT=None,
                   monopulse=None, want_rdm=False, want_cfar=False):
        """``pc_mtd_detect(dbf(cube, W, conj), ...)`` without leaving the device (rsp_raw_detect; v7_7
        sections 5-10): ``cube`` [P, N, C] raw, ``W`` [B, C] (None: the plan's DBF_coeffs_data_C, for a
        cube of the plan's C channels)."""
        cube = self._beams3(cube, 'cube')
        P, _, C = cube.shape
        if W is None:
            B, wk, wp = self.B, None, None
        else:
            W = np.asarray(W, np.complex128)
            if W.ndim != 2 or W.shape[1] != C:
                raise ValueError('cube %r and W %r: expected [P, N, C] and [B, C]' % (cube.shape, W.shape))
            B = W.shape[0]
            wk = np.asfortranarray(W).ravel(order='F').view(np.float64)   # B x C column-major (MATLAB)
            wp = _dptr(wk)
        G, n = self.G, int(nfft) if nfft else P
        prm, keep = self._detect_params(n, G, B, cfar, cluster, range_axis, velocity_axis, deltaR, deltaV,
                                        beam_angles_deg, k_slopes_LUT, monopulse)
        mk, mp = self._mtd_win(win, P)
        a, ap, dt = _complex_arg(cube)
        o, bufs = self._detect_out(n, G, B, want_cfar, (n, G, B) if want_rdm else None)
        check(lib().rsp_raw_detect(self.h, P, C, B, n, ap, dt, wp, 1 if conj else 0, mp, ct.byref(prm), ct.byref(o)))
        return self._collect(o, bufs, None, None)

    def profile_pc(self, P, B, iters=20):
        """HIP-event times of the three launches of ``pulse_compress`` on zeros (rsp_profile_pc):
        {'k_pc_pack' | 'k2_pc' | 'k_pc_unpack': (ms, bytes)}."""
        ms, by = (ct.c_float * 3)(), (ct.c_int64 * 3)()
        check(lib().rsp_profile_pc(self.h, int(P), int(B), int(iters), ms, by))
        return {k: (float(ms[i]), int(by[i])) for i, k in enumerate(('k_pc_pack', 'k2_pc', 'k_pc_unpack'))}

    # ---- digital down-conversion as a stand-alone stage: NCO mixer, FIR, decimator -----------------
    @staticmethod
    def _real3(x, what='x'):
        x = np.asarray(x)
        if np.iscomplexobj(x):
            raise ValueError('%s is complex: the down-converter takes real samples' % what)
        shape = x.shape
        if x.ndim == 1:
            x = x[None, :, None]
        elif x.ndim == 2:
            x = x[:, :, None]
        if x.ndim != 3:
            raise ValueError('%s %r: expected [N], [P, N] or [P, N, C]' % (what, shape))
        return x, shape

    def ddc(self, x, h, D, *, f0=None, fs=None, w=None, w0=0, nco='iq', off=0):
        """The receiver's digital down-converter (rsp_ddc; simulation_learn.m:79-102): real samples ``x``
        [P, N, C] (or [P, N], or one line [N]; float32 stays, everything else is taken as float64) times the
        NCO ``nco`` -- 'iq': cos - i sin, 'sin': the reference's single real mixer -- of phase step ``w``
        (2^-64 turns per sample; or ``f0`` and ``fs``, ``ddc_phase_word``) from start phase ``w0``, through
        ``filter(h, 1, .)`` and ``downsample(., D, off)`` -> complex128 of the input's shape with
        No = ceil((N - off) / D) samples.  The plan gives the device and the precision only;
        include/rsp.h has the arithmetic."""
        x3, shape = self._real3(x)
        P, N, C = x3.shape
        prm, keep = _ddc_params(h, D, f0, fs, w, w0, nco, off)
        a, ap, dt = _real_arg(x3)
        No = max(0, -(-(N - prm.off) // prm.D)) if prm.D >= 1 else 0
        out = np.empty((P, No, C), np.complex128, order='F')
        buf = out if out.size else np.empty(1, np.complex128)
        check(lib().rsp_ddc(self.h, P, N, C, ap, dt, ct.byref(prm), _dptr(buf)))
        return out.reshape({1: (No,), 2: (P, No), 3: (P, No, C)}[len(shape)], order='F')

    def ddc_device(self, d_x, d_out, P, N, C, h, D, *, f0=None, fs=None, w=None, w0=0, nco='iq', off=0):
        """The same on device memory in the plan's precision (rsp_ddc_device): ``d_x`` [P, N, C] reals ->
        ``d_out`` [P, No, C] complex, pulse index fastest on both sides; the two must not overlap."""
        prm, keep = _ddc_params(h, D, f0, fs, w, w0, nco, off)
        check(lib().rsp_ddc_device(self.h, int(P), int(N), int(C), ct.c_void_p(d_x), ct.byref(prm), ct.c_void_p(d_out)))

    def ddc_raw_detect(self, x, h, D, *, f0=None, fs=None, w=None, w0=0, nco='iq', off=0, W=None, conj=True, win=None,
                       nfft=None, cfar=None, cluster=None, range_axis=None, velocity_axis=None, deltaR=None, deltaV=None,
                       beam_angles_deg=None, k_slopes_LUT=None, monopulse=None, want_rdm=False, want_cfar=False):
        """``raw_detect(ddc(x, ...), ...)`` without leaving the device (rsp_ddc_raw_detect): ``x`` [P, N, C]
        real IF samples whose down-converted length No is the plan's point_PRT; the arguments are ``ddc``'s
        followed by ``raw_detect``'s, the result is ``raw_detect``'s."""
        x3, shape = self._real3(x)
        if len(shape) != 3:
            raise ValueError('x %r: expected [P, N, C]' % (shape,))
        P, N, C = x3.shape
        dprm, dkeep = _ddc_params(h, D, f0, fs, w, w0, nco, off)
        if W is None:
            B, wk, wp = self.B, None, None
        else:
            W = np.asarray(W, np.complex128)
            if W.ndim != 2 or W.shape[1] != C:
                raise ValueError('x %r and W %r: expected [P, N, C] and [B, C]' % (shape, W.shape))
            B = W.shape[0]
            wk = np.asfortranarray(W).ravel(order='F').view(np.float64)   # B x C column-major (MATLAB)
            wp = _dptr(wk)
        G, n = self.G, int(nfft) if nfft else P
        prm, keep = self._detect_params(n, G, B, cfar, cluster, range_axis, velocity_axis, deltaR, deltaV,
                                        beam_angles_deg, k_slopes_LUT, monopulse)
        mk, mp = self._mtd_win(win, P)
        a, ap, dt = _real_arg(x3)
        o, bufs = self._detect_out(n, G, B, want_cfar, (n, G, B) if want_rdm else None)
        check(lib().rsp_ddc_raw_detect(self.h, P, N, C, ap, dt, ct.byref(dprm), B, n, wp, 1 if conj else 0, mp,
                                       ct.byref(prm), ct.byref(o)))
        return self._collect(o, bufs, None, None)

    def profile_ddc(self, P, N, C, L, D, off=0, iters=20):
        """HIP-event time of k_ddc alone on a [P, N, C] cube of zeros (rsp_profile_ddc): {'stage', 'ms',
        'bytes'}, bytes = the input plus the output in the plan's precision."""
        ms, by = ct.c_float(), ct.c_int64()
        check(lib().rsp_profile_ddc(self.h, int(P), int(N), int(C), int(L), int(D), int(off), int(iters), ct.byref(ms),
                                    ct.byref(by)))
        return {'stage': 'k_ddc', 'ms': float(ms.value), 'bytes': int(by.value)}

    def _raw_weights(self, W):
        """(array kept alive, pointer) of the weights of a raw-cube call; None: the plan's own."""
        if W is None:
            return None, None
        W = np.asarray(W, np.complex128)
        if W.shape != (self.B, self.C):
            raise ValueError('W shape %r != (B, C) = %r' % (W.shape, (self.B, self.C)))
        Wcm = np.asfortranarray(W).ravel(order='F').view(np.float64)
        return Wcm, _dptr(Wcm)

    def process_raw_stage2(self, cube, W=None, conj=True, gate_cols=None):
        """``process_stage2(dbf(cube, W, conj))`` in one call, bit for bit (rsp_process_raw_stage2):
        the DBF runs inside the corner turn and the beams never reach device memory in PRT order.
        ``cube[m, n, c]`` is the raw frame [P, N, C] (or gated, with ``gate_cols`` as
        ``process_stage2``); ``W`` [B, C], None: the plan's DBF_coeffs_data_C.  Returns (MTD [P,G,B],
        PC [P,G,B])."""
        cube = np.asarray(cube)
        a, ap, dt = _complex_arg(cube)
        keep, wp = self._raw_weights(W)
        mtd = np.empty((self.P, self.G, self.B), np.complex128, order='F')
        pc = np.empty((self.P, self.G, self.B), np.complex128, order='F')
        mo, po = mtd.ctypes.data_as(ct.POINTER(ct.c_double)), pc.ctypes.data_as(ct.POINTER(ct.c_double))
        if gate_cols is None:
            if cube.shape != (self.P, self.N, self.C):
                raise ValueError('cube shape %r != (P, N, C) = %r' % (cube.shape, (self.P, self.N, self.C)))
            ng, cols = 0, None
        else:
            if cube.ndim != 3 or cube.shape[0] != self.P or cube.shape[2] != self.C:
                raise ValueError('cube shape %r: expected (P, n, C) with P=%d C=%d' % (cube.shape, self.P, self.C))
            ng, cols = cube.shape[1], _gate_cols_arg(gate_cols)
        check(lib().rsp_process_raw_stage2(self.h, ap, dt, ng, cols, wp, 1 if conj else 0, mo, po))
        return mtd, pc

    def process_raw_stage2_cfar(self, cube, cfar, W=None, conj=True, gate_cols=None, want=STAGE3_WANT, hits_cap=None):
        """``process_stage2_cfar`` on the raw cube (rsp_process_raw_stage2_cfar): ``cube``, ``W``, ``conj``
        and ``gate_cols`` as ``process_raw_stage2``, the rest as ``process_stage2_cfar``."""
        keep, wp = self._raw_weights(W)
        return self._stage2_detect(cube, self.C, gate_cols, _stage3_params(cfar), want, hits_cap,
                                   lib().rsp_process_raw_stage2_cfar, raw=(wp, 1 if conj else 0))

    def process_raw_stage2_vcfar(self, cube, cfar, method='ca', W=None, conj=True, gate_cols=None, want=STAGE3_WANT,
                                 hits_cap=None):
        """``process_stage2_vcfar`` on the raw cube (rsp_process_raw_stage2_vcfar): ``cube``, ``W``,
        ``conj`` and ``gate_cols`` as ``process_raw_stage2``, the rest as ``process_stage2_vcfar``."""
        keep, wp = self._raw_weights(W)
        return self._stage2_detect(cube, self.C, gate_cols, _vcfar_params(cfar, method), want, hits_cap,
                                   lib().rsp_process_raw_stage2_vcfar, raw=(wp, 1 if conj else 0))

    def process_raw_stage2_xcfar(self, cube, cfar, W=None, conj=True, gate_cols=None, want=STAGE3_WANT, hits_cap=None):
        """``process_stage2_xcfar`` on the raw cube (rsp_process_raw_stage2_xcfar): ``cube``, ``W``,
        ``conj`` and ``gate_cols`` as ``process_raw_stage2``, the rest as ``process_stage2_xcfar``."""
        keep, wp = self._raw_weights(W)
        return self._stage2_detect(cube, self.C, gate_cols, _xcfar_params(cfar), want, hits_cap,
                                   lib().rsp_process_raw_stage2_xcfar, raw=(wp, 1 if conj else 0))

    # ---- device-resident queue -------------------------------------------------------------
    def device_alloc(self, nbytes):
        p = ct.c_void_p()
        check(lib().rsp_device_alloc(self.h, int(nbytes), ct.byref(p)))
        return p.value

    def device_free(self, ptr):
        check(lib().rsp_device_free(self.h, ct.c_void_p(ptr)))

    def device_upload(self, ptr, host):
        host = np.ascontiguousarray(host)
        check(lib().rsp_device_upload(self.h, ct.c_void_p(ptr), host.ctypes.data_as(ct.c_void_p), host.nbytes))

    def device_download(self, ptr, count, dtype):
        out = np.empty(int(count), dtype)
        check(lib().rsp_device_download(self.h, out.ctypes.data_as(ct.c_void_p), ct.c_void_p(ptr), out.nbytes))
        return out

    def upload_cube(self, ptr, cube):
        """Upload a [P, N, C] cube column-major, in the plan's precision, to device pointer ``ptr``."""
        a = np.asfortranarray(np.asarray(cube).astype(self.cdtype))
        check(lib().rsp_device_upload(self.h, ct.c_void_p(ptr), a.ctypes.data_as(ct.c_void_p), a.nbytes))

    def synthesize_device(self, ptr, targets, frame_idx, seed=20250101, p_noise=1.0):
        tin = self._targets_in(targets)
        check(lib().rsp_synthesize_device(self.h, tin, len(targets), int(frame_idx), int(seed), float(p_noise),
                                          ct.c_void_p(ptr)))

    def profile_synthesis(self, ptr, targets, iters=20):
        """rsp_profile_synthesis: device ms of one S4 + S4.1 synthesis into ``ptr`` (HIP events
        over ``iters`` launches) and the cube bytes it writes."""
        tin = self._targets_in(targets)
        ms, by = ct.c_float(), ct.c_int64()
        check(lib().rsp_profile_synthesis(self.h, tin, len(targets), int(iters), ct.c_void_p(ptr), ct.byref(ms),
                                          ct.byref(by)))
        return {'stage': 'k_synth', 'ms': float(ms.value), 'bytes': int(by.value), 'frames': 1}

    def enqueue(self, ptr, frame_idx):
        check(lib().rsp_enqueue_device(self.h, ct.c_void_p(ptr), int(frame_idx)))

    def enqueue_many(self, ptrs, frame_ids, rdms=None):
        """rsp_enqueue_device_n: device cubes ptrs[i] as frames frame_ids[i], one C call.  With
        ``rdms`` (device pointers, one per frame, rdm_elems complex elements each) every frame's
        complex RD map is written there (rsp_enqueue_device_rdm_n), complete after drain()."""
        n = len(ptrs)
        arr = (ct.c_void_p * max(n, 1))(*ptrs)
        ids = (ct.c_int32 * max(n, 1))(*[int(f) for f in frame_ids])
        if rdms is None:
            check(lib().rsp_enqueue_device_n(self.h, arr, ids, n))
        else:
            if len(rdms) != n:
                raise ValueError('one RD map per frame')
            ra = (ct.c_void_p * max(n, 1))(*rdms)
            check(lib().rsp_enqueue_device_rdm_n(self.h, arr, ids, ra, n))

    def rdm_from_device(self, ptr):
        """A device RD map ([B][P][G], plan precision, as rsp_enqueue_device_rdm writes it) as the
        MATLAB-shaped [P, G, B] complex array of rdm_13beam (fsf:135)."""
        sz = self.sizes
        m = self.device_download(ptr, sz.rdm_elems, self.cdtype).reshape(sz.B, sz.P, sz.G)
        return np.transpose(m, (1, 2, 0))

    def host_alloc(self, nbytes):
        """Pinned host memory (rsp_host_alloc); returns the address."""
        p = ct.c_void_p()
        check(lib().rsp_host_alloc(self.h, int(nbytes), ct.byref(p)))
        return p.value

    def host_free(self, ptr):
        check(lib().rsp_host_free(self.h, ct.c_void_p(ptr)))

    def host_cube(self, ptr):
        """A numpy [P, N, C] view (column-major, plan precision) of host memory at ``ptr``."""
        P, N, C = self.P, self.N, self.sizes.C
        buf = (ct.c_char * (P * N * C * np.dtype(self.cdtype).itemsize)).from_address(ptr)
        return np.ndarray((P, N, C), self.cdtype, buffer=buf, order='F')

    def enqueue_host(self, ptr_or_cube, frame_idx):
        """rsp_enqueue_host: a host cube (address, or a Fortran-ordered array in the plan's
        precision) that must stay unchanged until drain()."""
        if isinstance(ptr_or_cube, np.ndarray):
            a = ptr_or_cube
            if a.dtype != np.dtype(self.cdtype) or not a.flags.f_contiguous:
                raise ValueError('enqueue_host needs a Fortran-ordered %s cube' % np.dtype(self.cdtype))
            ptr = a.ctypes.data
        else:
            ptr = ptr_or_cube
        dt = _abi.RSP_C128 if np.dtype(self.cdtype) == np.complex128 else _abi.RSP_C64
        check(lib().rsp_enqueue_host(self.h, ct.c_void_p(ptr), dt, int(frame_idx)))

    def drain(self):
        check(lib().rsp_drain(self.h))

    def sync(self):
        check(lib().rsp_device_sync(self.h))

    def results(self, clear=True):
        nf, nt = ct.c_int32(), ct.c_int64()
        check(lib().rsp_results_count(self.h, ct.byref(nf), ct.byref(nt)))
        out = []
        cap = 4096
        buf = (_abi.Target * cap)()
        for i in range(nf.value):
            fi, n, nd = ct.c_int32(), ct.c_int32(), ct.c_int32()
            check(lib().rsp_results_get(self.h, i, ct.byref(fi), None, 0, ct.byref(n), ct.byref(nd)))
            if n.value > cap:
                cap = n.value
                buf = (_abi.Target * cap)()
            check(lib().rsp_results_get(self.h, i, ct.byref(fi), buf, cap, ct.byref(n), ct.byref(nd)))
            out.append({'frame_idx': fi.value, 'n_dets': nd.value,
                        'final_targets': [_tgt_dict(buf[j]) for j in range(n.value)]})
        if clear:
            check(lib().rsp_results_clear(self.h))
        return out

    def results_rows(self, clear=True):
        """The queued results as an [n, 5] float64 array (frame_idx, Range, Velocity, Angle,
        Power; one NaN row per frame without targets) in one C call (rsp_results_rows)."""
        n = ct.c_int64()
        check(lib().rsp_results_rows(self.h, None, 0, ct.byref(n)))
        rows = np.empty((max(n.value, 1), 5), np.float64)
        check(lib().rsp_results_rows(self.h, rows.ctypes.data_as(ct.POINTER(ct.c_double)), n.value, ct.byref(n)))
        if clear:
            check(lib().rsp_results_clear(self.h))
        return rows[:n.value]

    def set_stage_timing(self, on=True):
        """Live HIP-event timing of K1/K2/K3 of every queued batch (resets the sums)."""
        check(lib().rsp_set_stage_timing(self.h, 1 if on else 0))

    def stage_times(self):
        """Sums of the live stage timing: [{'stage', 'ms_total', 'launches', 'frames'}]."""
        n = self.sizes.n_stages
        ms = (ct.c_double * n)()
        nl, nf = ct.c_int64(), ct.c_int64()
        check(lib().rsp_stage_times(self.h, ms, n, ct.byref(nl), ct.byref(nf)))
        return [{'stage': lib().rsp_stage_name(i).decode(), 'ms_total': ms[i], 'launches': nl.value,
                 'frames': nf.value} for i in range(n)]

    def profile_stages(self, d_cubes, iters=20, d_rdms=None):
        """Per-stage HIP-event timing; d_cubes = device pointer or list of pointers (batched).
        d_rdms: K2 also writes each frame's complex RD map there (rsp_profile_stages_rdm)."""
        if not isinstance(d_cubes, (list, tuple)):
            d_cubes = [d_cubes]
        n = self.sizes.n_stages
        ms = (ct.c_float * n)()
        by = (ct.c_int64 * n)()
        arr = (ct.c_void_p * len(d_cubes))(*d_cubes)
        nf = ct.c_int32()
        if d_rdms:   # the C call reads min(len(d_cubes), F) maps: a shorter list would be read past its end
            need = min(len(d_cubes), self.frames_per_launch)
            if len(d_rdms) < need or any(r is None or not int(r) for r in d_rdms[:need]):
                raise ValueError('d_rdms needs %d non-null device maps (one per frame of the batch)' % need)
        ra = (ct.c_void_p * len(d_rdms))(*d_rdms) if d_rdms else None
        check(lib().rsp_profile_stages_rdm(self.h, arr, len(d_cubes), ra, int(iters), ms, by, n, ct.byref(nf)))
        return [{'stage': lib().rsp_stage_name(i).decode(), 'ms': ms[i], 'bytes': by[i], 'frames': nf.value}
                for i in range(n)]


def process_targets_multi(plans, frames, seed=20250101, p_noise=1.0, cap=1024):
    """rsp_process_targets_multi: frames = [(targets, frame_idx), ...] split over ``plans`` (one
    host thread each, typically one plan per device); returns the final targets of every frame,
    in order."""
    n = len(frames)
    tins = [Plan._targets_in(t) for t, _ in frames]
    tptr = (ct.POINTER(_abi.TargetIn) * max(n, 1))(*[ct.cast(t, ct.POINTER(_abi.TargetIn)) for t in tins])
    nt = (ct.c_int32 * max(n, 1))(*[len(t) for t, _ in frames])
    fi = (ct.c_int32 * max(n, 1))(*[int(f) for _, f in frames])
    out = (_abi.Target * (max(n, 1) * cap))()
    nout = (ct.c_int32 * max(n, 1))()
    ph = (ct.c_void_p * len(plans))(*[p.h for p in plans])
    check(lib().rsp_process_targets_multi(ph, len(plans), tptr, nt, fi, n, int(seed), float(p_noise), out, cap, nout))
    return [[_tgt_dict(out[j * cap + i]) for i in range(nout[j])] for j in range(n)]
