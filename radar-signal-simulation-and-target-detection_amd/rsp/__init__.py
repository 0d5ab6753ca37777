"""rsp -- MI355X-native per-frame radar signal processing (host side).

Drop-in for the MATLAB reference's per-frame chain
(XuZerui2023/Radar-Signal-Simulation-and-Target-Detection, Simulation/):

* ``fun_process_single_frame(targets, config, cfar_params, cluster_params,
  precomputed_data, frame_idx)``  -- fun_process_single_frame.m:13
* ``process_stage2_mtd(iq_data, angle, config)``  -- process_stage2_mtd.m:1
* ``dbf_beams(raw_iq_data, DBF_coeffs_data_C)`` / ``process_frame_stage2(raw_iq_data, angle, config,
  DBF_coeffs_data_C)`` -- the DBF loop every stage-2 script runs first
  (debug_simulated_data_processing.m:166-175), alone or fused with process_stage2_mtd
* ``mtd_doppler(pc_results, MTD_win, nfft)`` / ``mtd_velocity_axis(v_max, nfft)`` -- the windowed,
  zero-padded slow-time FFT of any length and its velocity axis
  (main_simulate_echoes_with_array_v7_7.m:501-503, :190; fsf:134-135)
* ``detect_rdm(rdm_13beam, cfar_params, cluster_params, precomputed_data)`` / ``mtd_detect(pc_results,
  MTD_win, nfft, ...)`` -- fun_run_goca_cfar_8, fun_parameter_estimation_9 and the two clustering stages
  (fsf:172-407) on a range-Doppler cube of any shape, alone or behind the zero-padded MTD
  (main_simulate_echoes_with_array_v7_7.m:501-...)
* ``pulse_compress(iq_data_13beam, config, precomputed_data)`` / ``beams_detect(iq_data_13beam, MTD_win,
  nfft, ...)`` / ``raw_detect(raw_iq_data, DBF_coeffs_data_C, MTD_win, nfft, ...)`` -- the three-segment
  pulse compression of any number of pulses and beams (main_simulate_echoes_with_array_v7_7.m:362-486), alone
  or as the front of the zero-padded MTD and the detector, from the beams or from the raw frame
* ``mix_filter_downsample(xt, f, fs, Num, D)`` -- the digital down-converter in front of all of it: NCO
  mixer, FIR and decimator of the real IF samples (simulation_learn.m:79-102)
* ``precompute(...)`` -- the driver's "%% 3" section (v8:79-155)
* ``load_frame`` / ``save_frame`` -- the ``frame_sim_array_%d.mat`` load/save pair
  (main_simulate_echoes_with_array_v2.m:285, debug_simulated_data_processing_v3.m:20-22)

All compute runs in librsp.so (HIP kernels for gfx950 behind the C-ABI in
include/rsp.h).  There is no CPU fallback.
"""
import collections
import hashlib

import numpy as np

from .config import (named_config, make_config, default_cfar_params, default_cluster_params,
                     v8_2_targets, evolve_targets, V8_FIR, stage2_config, debug_v3_config,
                     debug_v2_cfar_config, v3_cfar_params)
from .precompute import precompute
from .plan import (Plan, process_targets_multi, describe_vcfar, describe_dbf, describe_xcfar, describe_mtd, mtd_table,
                   describe_detect, describe_pc, describe_ddc, ddc_phase_word)
from ._abi import RspError
from .matio import load_frame, save_frame
from .music import MusicPlan, MUSIC_1D, MusicPlan2D, MUSIC_2D
from .tracks import inter_frame_cluster, default_inter_frame_params
from . import matio

# main_simulate_echoes_with_array_v2.m:257-264: PRT columns of the three gated segments
REFERENCE_GATE_COLS = ((83, 310), (311, 1033), (1034, 3486))

_PLANS = collections.OrderedDict()   # content fingerprint -> Plan (most recently used last)
_MAX_PLANS = 4


def _fingerprint(*objs):
    """SHA-1 over the contents of nested dicts / lists / scalars / numpy arrays, so that a plan
    is reused only for equal inputs (an in-place edit or a new dict with other values makes a
    new plan; a garbage-collected dict's reused id() cannot alias an old one)."""
    h = hashlib.sha1()

    def feed(o):
        if isinstance(o, dict):
            h.update(b'{')
            for k in sorted(o, key=str):
                feed(str(k))
                feed(o[k])
            h.update(b'}')
        elif isinstance(o, (list, tuple)):
            h.update(b'[')
            for x in o:
                feed(x)
            h.update(b']')
        elif isinstance(o, np.ndarray):
            h.update(b'A' + str(o.dtype).encode() + str(o.shape).encode())
            h.update(np.ascontiguousarray(o).tobytes())
        else:
            h.update(b'S' + type(o).__name__.encode() + repr(o).encode())
    for o in objs:
        feed(o)
    return h.hexdigest()


def _plan_for(config, cfar_params, cluster_params, precomputed_data, device=0, precision='c128'):
    key = _fingerprint(config, cfar_params, cluster_params, precomputed_data, device, precision)
    p = _PLANS.pop(key, None)
    if p is None:
        p = Plan(config, cfar_params, cluster_params, precomputed_data, device=device, precision=precision)
        while len(_PLANS) >= _MAX_PLANS:
            _PLANS.popitem(last=False)[1].close()
    _PLANS[key] = p
    return p


def fun_process_single_frame(targets, config, cfar_params, cluster_params, precomputed_data, frame_idx,
                             seed=20250101, device=0, precision='c128'):
    """fun_process_single_frame.m:13 -- returns ``final_targets`` (list of dicts with
    Range, Velocity, Angle, Power).  Echo synthesis (S4) and noise (S4.1) run on the
    device; MATLAB ``randn`` is replaced by the documented Philox stream (seed, frame_idx).
    Complex double by default, like MATLAB."""
    p = _plan_for(config, cfar_params, cluster_params, precomputed_data, device, precision)
    return p.process_targets(targets, frame_idx=frame_idx, seed=seed)['final_targets']


def _stage2_precompute(config):
    """precomputed_data for the stage-2 path built from ``config`` alone (the 3-argument call):
    waveform, matched filters, segment geometry and MTD window of v8:79-135; the DBF weights,
    beam angles and K-LUT are not used by stage 2 and are zero.  ``config`` is already in the
    v8 form (config.stage2_config)."""
    sc = config['Sig_Config']
    B, C = int(sc['beam_num']), int(sc['channel_num'])
    return precompute(config, np.zeros((B, C), complex), np.zeros(B), np.zeros(max(B - 1, 0)), V8_FIR)


def process_stage2_mtd(iq_data, angle, config, precomputed_data=None, gate_cols=None, device=0, precision='c128'):
    """process_stage2_mtd.m:1 -- ``[MTD_results, PC_results] = process_stage2_mtd(iq_data, angle, config)``.

    ``iq_data[m, n, b]`` is beamformed fast-time data (the DBF of
    debug_simulated_data_processing_v3.m:146-152), either the full PRT (``n`` = point_PRT) or
    gated like the v2 ``.mat`` frames (main_simulate_echoes_with_array_v2.m:256-267: PRT columns
    83:310, 311:1033, 1034:3486 side by side, n = 3404; other gatings via ``gate_cols``, 1-based
    inclusive (first, last) per segment).  Gated columns are put back at their PRT positions
    (zeros elsewhere).  ``angle`` (servo angle) is unused, as in the reference.  Returns
    complex [P, G, B] arrays, G = N_total_gate (process_stage2_mtd.m:29-30 pre-sizes 332 x 3404
    x 13 for the reference config).

    The reference's arithmetic (fun_MTD_produce -> fun_lss_pulse_compression / fun_Process_MTD,
    debug_simulated_data_processing_v2.m:259-405) is un-vendored; this backs it with the
    per-frame chain's own S6 pulse compression + S7 MTD (fsf:99-136).  ``precomputed_data``
    defaults to the one v8:79-135 builds from ``config``."""
    config = stage2_config(config)   # the v3 debug script's config form too (point_PRT = 3404, no gaps / Array)
    if precomputed_data is None:
        precomputed_data = _stage2_precompute(config)
    p = _plan_for(config, default_cfar_params(), default_cluster_params(), precomputed_data, device, precision)
    iq = np.asarray(iq_data)
    if iq.ndim == 2:
        iq = iq[:, :, None]
    if iq.shape[1] == p.N:
        return p.process_stage2(iq)
    return p.process_stage2(iq, gate_cols=gate_cols if gate_cols is not None else REFERENCE_GATE_COLS)


def dbf_beams(raw_iq_data, DBF_coeffs_data_C, conj=True, device=0, precision='c128'):
    """The DBF loop of the stage-2 scripts: ``iq_data_13beam(i, :, :) = squeeze(raw_iq_data(i, :, :)) *
    DBF_coeffs_data_C'`` for every pulse i (debug_simulated_data_processing.m:166-175,
    debug_simulated_data_processing_v3.m:144-152), or with ``conj=False`` the plain transpose ``.'``
    of main_test_with_simulated_data.m:207-214 (one beam of it: debug_simulated_data_processing_v2.m:
    176-182).  ``raw_iq_data`` is [prtNum, point_PRT, channel_num] of any shape, ``DBF_coeffs_data_C``
    [beam_num, channel_num]; returns complex128 [prtNum, point_PRT, beam_num].  'c128' computes in
    complex double like MATLAB, 'c64' in complex single (widened to double)."""
    cfg, cfar, cluster, W, ang, k = named_config('plumbing')   # the plan gives the device and the precision only
    p = _plan_for(cfg, cfar, cluster, precompute(cfg, W, ang, k, V8_FIR), device, precision)
    return p.dbf(raw_iq_data, DBF_coeffs_data_C, conj=conj)


def mtd_doppler(pc_results, MTD_win, nfft=None, device=0, precision='c128'):
    """``rdm(:, :, b) = fftshift(fft(pc_results(:, :, b) .* MTD_win, nfft, 1), 1)`` for every beam b
    (main_simulate_echoes_with_array_v7_7.m:501-503 with FFTnum_MTD = 512; fun_process_single_frame.m:
    134-135 with ``nfft=None``, MATLAB's ``[]``).  ``pc_results`` is [prtNum, gates] or [prtNum, gates,
    beam_num] of any shape, ``MTD_win`` prtNum reals (a column, as kaiser's; None: no window), ``nfft``
    any length from prtNum to 2048, a power of two or not.  Returns complex128 [nfft, gates(,
    beam_num)]."""
    cfg, cfar, cluster, W, ang, k = named_config('plumbing')   # the plan gives the device and the precision only
    p = _plan_for(cfg, cfar, cluster, precompute(cfg, W, ang, k, V8_FIR), device, precision)
    return p.mtd(pc_results, MTD_win, nfft=nfft)


def mix_filter_downsample(xt, f, fs, Num, D, device=0, precision='c128'):
    """The receiver front end of simulation_learn.m:79-102: ``xrt = xt .* sin(2*pi*f*t2)`` with
    ``t2 = (0:N-1)/fs``, ``firxrt = filter(Num, 1, xrt)`` and ``xrtdown = downsample(firxrt, D)``.  ``xt`` is
    the real IF line [N] (or lines [P, N], [P, N, C], the fast-time axis second), ``Num`` the FIR taps
    (FIR.mat's 12), ``D`` the decimation factor (4).  Returns the real baseband samples, float64 with
    ceil(N / D) along the fast-time axis.  The mixer is the library's 64-bit NCO at ``ddc_phase_word(f, fs)``
    (``Plan.ddc`` with ``nco='sin'``; include/rsp.h has the arithmetic)."""
    cfg, cfar, cluster, W, ang, k = named_config('plumbing')   # the plan gives the device and the precision only
    p = _plan_for(cfg, cfar, cluster, precompute(cfg, W, ang, k, V8_FIR), device, precision)
    return np.ascontiguousarray(p.ddc(xt, Num, D, f0=f, fs=fs, nco='sin').real)


def mtd_velocity_axis(v_max, nfft):
    """``linspace(-v_max/2, v_max/2, nfft)`` (main_simulate_echoes_with_array_v7_7.m:190): the velocity
    of every row of ``mtd_doppler``'s result as the reference labels them, v_max = wavelength / (2 prt)."""
    return np.linspace(-v_max / 2.0, v_max / 2.0, int(nfft))


def _plumbing_plan(device, precision, monopulse='amplitude'):
    """A plan that gives the device and the precision only (and, for S9, the monopulse form)."""
    cfg, cfar, cluster, W, ang, k = named_config('plumbing')
    if monopulse == 'amplitude':
        return _plan_for(cfg, cfar, cluster, precompute(cfg, W, ang, k, V8_FIR), device, precision)
    key = ('plumbing', monopulse, device, precision)
    p = _PLANS.pop(key, None)
    if p is None:
        p = Plan(cfg, cfar, cluster, precompute(cfg, W, ang, k, V8_FIR), device=device, precision=precision, monopulse=monopulse)
        while len(_PLANS) >= _MAX_PLANS:
            _PLANS.popitem(last=False)[1].close()
    _PLANS[key] = p
    return p


def detect_rdm(rdm_13beam, cfar_params, cluster_params, precomputed_data, monopulse='amplitude', device=0, precision='c128',
               want_cfar=False):
    """fun_process_single_frame.m S8-S11 on a given range-Doppler cube: ``fun_run_goca_cfar_8(rdm_13beam,
    cfar_params)``, ``fun_parameter_estimation_9``, ``fun_cluster_stage1_10`` and ``fun_cluster_stage2_11``
    (fsf:172-407).  ``rdm_13beam`` is complex [V, G, B] of any shape, B >= 2; ``precomputed_data`` gives
    ``range_axis`` (G), ``velocity_axis`` (V), ``deltaR``, ``deltaV``, ``beam_angles_deg`` (B) and
    ``k_slopes_LUT`` (B - 1).  ``monopulse`` 'complex': the angle from the complex ratio
    (main_plot_snr_vs_angle_error.m:455-462).  Returns a dict: ``final_targets``, ``detections`` (the
    parameterised detections in the reference's order) and, with ``want_cfar``, ``cfar_maps``
    (rdm_for_cfar_all, [V, G, B - 1])."""
    pre = precomputed_data
    p = _plumbing_plan(device, precision, monopulse)
    return p.detect(rdm_13beam, cfar_params, cluster_params, pre['range_axis'], pre['velocity_axis'], pre['deltaR'],
                    pre['deltaV'], pre['beam_angles_deg'], pre['k_slopes_LUT'], monopulse, want_cfar=want_cfar)


def mtd_detect(pc_results, MTD_win, nfft, cfar_params, cluster_params, precomputed_data, velocity_axis=None, v_max=None,
               monopulse='amplitude', device=0, precision='c128', want_rdm=False, want_cfar=False):
    """main_simulate_echoes_with_array_v7_7.m sections 7-10 from the pulse-compression results on:
    ``mtd_doppler(pc_results, MTD_win, nfft)`` and ``detect_rdm`` on its result, without the cube leaving
    the device.  ``velocity_axis`` (nfft entries) defaults to ``mtd_velocity_axis(v_max, nfft)`` when
    ``v_max`` is given (v7_7:190), else to ``precomputed_data['velocity_axis']``; the other axes and
    parameters as ``detect_rdm``.  ``want_rdm`` adds the cube ``rdm`` [nfft, G, B]."""
    pre = precomputed_data
    n = int(nfft) if nfft else np.asarray(pc_results).shape[0]
    if velocity_axis is None:
        velocity_axis = mtd_velocity_axis(v_max, n) if v_max is not None else pre['velocity_axis']
    p = _plumbing_plan(device, precision, monopulse)
    return p.mtd_detect(pc_results, MTD_win, n, cfar_params, cluster_params, pre['range_axis'], velocity_axis,
                        pre['deltaR'], pre['deltaV'], pre['beam_angles_deg'], pre['k_slopes_LUT'], monopulse,
                        want_rdm=want_rdm, want_cfar=want_cfar)


_PC_PLAN_PULSES = 16   # the pulse count of the plans behind pulse_compress / beams_detect / raw_detect


def _pc_plan(config, precomputed_data, device, precision):
    """The cached plan behind the three calls below: ``config``'s waveform, gate layout and filters with a
    pulse count every plan accepts, so that a ``config`` whose prtNum a plan refuses (odd, 333) works.
    The stage reads neither prtNum nor the per-pulse tables, which are cut or padded to that count."""
    n = _PC_PLAN_PULSES
    cfg = dict(config, Sig_Config=dict(config['Sig_Config'], prtNum=n))

    def fit(x):
        x = np.asarray(x, float).ravel()
        return np.concatenate([x[:n], np.zeros(max(n - x.size, 0))])

    pre = dict(precomputed_data, MTD_win=fit(precomputed_data['MTD_win']),
               velocity_axis=fit(precomputed_data['velocity_axis']))
    return _plan_for(cfg, default_cfar_params(), default_cluster_params(), pre, device, precision)


def pulse_compress(iq_data_13beam, config, precomputed_data, device=0, precision='c128'):
    """Section 6 of main_simulate_echoes_with_array_v7_7.m (:362-486; fun_process_single_frame.m:99-127):
    the three-segment pulse compression of every pulse of every beam.  ``iq_data_13beam`` is the DBF's
    result [prtNum, point_PRT, beam_num]; the pulse and beam counts are the array's, any number of either
    (odd, prime, one), whatever ``config`` says.  ``config`` and ``precomputed_data`` give the waveform, the
    gate layout and the matched filters.  Returns PC_results, complex128 [prtNum, N_total_gate, beam_num]."""
    return _pc_plan(config, precomputed_data, device, precision).pulse_compress(iq_data_13beam)


def _chain_velocity_axis(velocity_axis, v_max, n, pre):
    if velocity_axis is None:
        velocity_axis = mtd_velocity_axis(v_max, n) if v_max is not None else pre['velocity_axis']
    return velocity_axis


def beams_detect(iq_data_13beam, MTD_win, nfft, cfar_params, cluster_params, config, precomputed_data,
                 velocity_axis=None, v_max=None, monopulse='amplitude', device=0, precision='c128', want_rdm=False,
                 want_cfar=False):
    """main_simulate_echoes_with_array_v7_7.m sections 6-10 from the beams on: ``pulse_compress``,
    ``mtd_doppler(.., MTD_win, nfft)`` and ``detect_rdm`` without the cubes leaving the device.  The
    arguments after ``nfft`` are ``mtd_detect``'s, with ``config`` as ``pulse_compress`` takes it."""
    pre = precomputed_data
    n = int(nfft) if nfft else np.asarray(iq_data_13beam).shape[0]
    p = _pc_plan(config, pre, device, precision)
    return p.pc_mtd_detect(iq_data_13beam, MTD_win, n, cfar_params, cluster_params, pre['range_axis'],
                           _chain_velocity_axis(velocity_axis, v_max, n, pre), pre['deltaR'], pre['deltaV'],
                           pre['beam_angles_deg'], pre['k_slopes_LUT'], monopulse, want_rdm=want_rdm, want_cfar=want_cfar)


def raw_detect(raw_iq_data, DBF_coeffs_data_C, MTD_win, nfft, cfar_params, cluster_params, config, precomputed_data,
               conj=True, velocity_axis=None, v_max=None, monopulse='amplitude', device=0, precision='c128',
               want_rdm=False, want_cfar=False):
    """main_simulate_echoes_with_array_v7_7.m sections 5-10 from the raw frame on: ``dbf_beams(raw_iq_data,
    DBF_coeffs_data_C, conj)`` and ``beams_detect`` on its result without leaving the device.
    ``raw_iq_data`` is [prtNum, point_PRT, channel_num], ``DBF_coeffs_data_C`` [beam_num, channel_num]."""
    pre = precomputed_data
    n = int(nfft) if nfft else np.asarray(raw_iq_data).shape[0]
    p = _pc_plan(config, pre, device, precision)
    return p.raw_detect(raw_iq_data, DBF_coeffs_data_C, conj, MTD_win, n, cfar_params, cluster_params, pre['range_axis'],
                        _chain_velocity_axis(velocity_axis, v_max, n, pre), pre['deltaR'], pre['deltaV'],
                        pre['beam_angles_deg'], pre['k_slopes_LUT'], monopulse, want_rdm=want_rdm, want_cfar=want_cfar)


def process_frame_stage2(raw_iq_data, angle, config, DBF_coeffs_data_C, conj=True, gate_cols=None,
                         precomputed_data=None, device=0, precision='c128'):
    """The stage-2 scripts from the raw frame on: the DBF loop (``dbf_beams``) and
    ``process_stage2_mtd(iq_data_13beam, angle, config)`` in one call, without the beams leaving the
    device.  ``raw_iq_data[m, n, c]`` is the raw 16-channel frame (``load_frame``'s cube), full PRT or
    gated as ``process_stage2_mtd`` takes it (n = 3404: the v2 gating; others via ``gate_cols``);
    ``DBF_coeffs_data_C`` is [beam_num, channel_num]; ``conj`` as ``dbf_beams``.  Returns
    ``(MTD_results, PC_results)``, complex [P, G, B], equal to the two calls in a row to the bit."""
    raw = np.asarray(raw_iq_data)
    W = np.asarray(DBF_coeffs_data_C, np.complex128)
    if raw.ndim != 3 or W.ndim != 2 or W.shape[1] != raw.shape[2]:
        raise ValueError('raw_iq_data %r and DBF_coeffs_data_C %r: expected [P, n, C] and [B, C]' % (raw.shape, W.shape))
    config = stage2_config(config)
    config = dict(config, Sig_Config=dict(config['Sig_Config'], channel_num=int(raw.shape[2])))
    if W.shape[0] != config['Sig_Config']['beam_num']:
        raise ValueError('DBF_coeffs_data_C has %d rows, config has %d beams' % (W.shape[0], config['Sig_Config']['beam_num']))
    if precomputed_data is None:
        precomputed_data = _stage2_precompute(config)
    p = _plan_for(config, default_cfar_params(), default_cluster_params(), precomputed_data, device, precision)
    if raw.shape[1] == p.N:
        return p.process_raw_stage2(raw, W, conj=conj)
    return p.process_raw_stage2(raw, W, conj=conj, gate_cols=gate_cols if gate_cols is not None else REFERENCE_GATE_COLS)


def local_execute_cfar(mtd_amplitude_map, cfar_params, config, device=0, precision='c128'):
    """debug_simulated_data_processing_v2.m:419 -- ``[cfar_flag, threshold_matrix] =
    local_execute_cfar(mtd_amplitude_map, cfar_params, config)``: the stage-3 range CFAR the
    reference runs on ``abs(MTD_results)`` (:209-213), per pulse segment, with the zero-velocity
    notch, greatest-of / smallest-of selection, the opposite window at a segment's edges and the
    ``>=`` test (include/rsp.h restates it).

    ``mtd_amplitude_map`` is real [P, G] or [P, G, B]; ``cfar_params`` has the reference's fields
    refCells_R, saveCells_R, T_CFAR, CFARmethod_R, MTD_0v_num (None: ``config['cfar']``, which is
    what the reference's executeCFAR_2D reads; config.debug_v2_cfar_config builds the script's);
    the segment lengths are point_prt(2:3) of ``config`` (through config.stage2_config).  Returns
    float64 arrays of the input's shape, as MATLAB does.  'c128' computes in double like MATLAB,
    'c64' in single (thresholds widened to double)."""
    if cfar_params is None:
        cfar_params = config['cfar']
    config = stage2_config(config)
    segs = config['Sig_Config']['point_prt_segments']
    p = _plan_for(config, default_cfar_params(), default_cluster_params(), _stage2_precompute(config), device, precision)
    r = p.stage3_cfar(mtd_amplitude_map, cfar_params, segments=segs, want_hits=False)
    return r['flags'].astype(np.float64), r['threshold']


def local_cfar_detector(rdm_abs, params, device=0, precision='c128'):
    """main_simulate_echoes_with_array_v3.m:278 -- ``[detection_map, threshold_map] =
    local_cfar_detector(rdm_abs, params)``: the cell-averaging CFAR the reference slides along the
    velocity axis of ``abs(mtd_results)`` of one beam (:249-250), every range column on its own, with
    the guard and reference windows clipped where the map ends and the strict ``>`` test
    (include/rsp.h restates it).

    ``rdm_abs`` is real [P, G] (or [P, G, n]) of any shape; ``params`` has the reference's fields
    refCells_V, guardCells_V and T_CFAR (config.v3_cfar_params builds the script's).
    ``params['method']`` is ignored, as the reference's function ignores it: the noise level is always
    the cell average (``Plan.doppler_cfar`` has the greatest-of and smallest-of variants).  Returns
    (detection_map bool, threshold_map float64) of the input's shape.  'c128' computes in double like
    MATLAB, 'c64' in single (thresholds widened to double)."""
    cfg, cfar, cluster, W, ang, k = named_config('plumbing')   # the plan gives the device and the precision only
    p = _plan_for(cfg, cfar, cluster, precompute(cfg, W, ang, k, V8_FIR), device, precision)
    r = p.doppler_cfar(rdm_abs, params, method='ca', want_hits=False)
    return r['flags'].astype(bool), r['threshold']


def goca_cfar_maps(amp, cfar_params, device=0, precision='c128'):
    """fun_run_goca_cfar_8's cross GOCA-CFAR test (fun_process_single_frame.m:192-213) on any real
    amplitude map: ``[detection_map, threshold_map] = goca_cfar_maps(amp, cfar_params)``.  Every cell
    r = hR + 1 .. G - hR, v = hV + 1 .. P - hV (hR = refCells_R + guardCells_R, hV likewise) is tested
    against T_CFAR times the greatest of its four slice means, two along range and two along Doppler,
    with the strict ``>`` (include/rsp.h restates it); the cells the reference never tests have no
    detection and threshold +Inf.

    ``amp`` is real [P, G] (or [P, G, n]) of any shape; ``cfar_params`` has the reference's fields
    refCells_R, guardCells_R, refCells_V, guardCells_V and T_CFAR (``default_cfar_params``).  Returns
    (detection_map bool, threshold_map float64) of the input's shape.  'c128' computes in double like
    MATLAB, 'c64' in K3's single-precision form (thresholds widened to double)."""
    cfg, cfar, cluster, W, ang, k = named_config('plumbing')   # the plan gives the device and the precision only
    p = _plan_for(cfg, cfar, cluster, precompute(cfg, W, ang, k, V8_FIR), device, precision)
    r = p.cross_cfar(amp, cfar_params, want_hits=False)
    return r['flags'].astype(bool), r['threshold']
