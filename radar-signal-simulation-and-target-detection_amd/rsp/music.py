"""MUSIC direction finding on the device (MUSIC_1D.m:21-48, run_music_algorithm.m:22-69).

``MusicPlan`` binds the ``rsp_music_*`` C-ABI (include/rsp.h): the scripts' parameters
(N channels, K snapshots, M sources, element spacing / wavelength, scan grid phi_list) make the
plan; ``process`` runs a batch of snapshot matrices X [N x K] through

  R = X X^H / K -> eig, sort descend -> Q_n -> P(phi) = 1/sum|Q_n^H a(phi)|^2 -> P_dB -> findpeaks

and returns what the scripts compute: ``P_MUSIC_dB``, the sorted eigenvalues ``EVA``, the M
peak indices / angles ``phi_e`` (MUSIC_1D.m:48).  ``MUSIC_1D(X, ...)`` is the one-instance
form of MUSIC_1D.m.  ``precision``: 'c128' (complex double, MATLAB's arithmetic; default) or
'c64' (complex single).  All compute runs in librsp.so; there is no CPU path.

``MusicPlan2D`` / ``MUSIC_2D`` are the planar-array form (MUSIC_2D.m): an nx x ny uniform
rectangular array scanned over a theta x phi grid, peaks by imregionalmax; complex double only.
"""
import ctypes as ct

import numpy as np

from . import _abi


class MusicPlan:
    def __init__(self, channel_num, num_snapshots, num_sources, scan_rad, d_over_lambda=0.5, max_batch=1,
                 device=0, precision='c128'):
        if precision not in ('c128', 'c64'):
            raise ValueError("precision must be 'c128' or 'c64'")
        self._lib = _abi.lib()
        self.precision = precision
        self.cdtype = np.complex128 if precision == 'c128' else np.complex64   # device snapshots
        self.scan_rad = np.ascontiguousarray(scan_rad, np.float64)
        self.N, self.K, self.M, self.S = int(channel_num), int(num_snapshots), int(num_sources), len(self.scan_rad)
        self.max_batch = int(max_batch)
        cfg = _abi.MusicConfig(self.N, self.K, self.M, self.S, float(d_over_lambda),
                               self.scan_rad.ctypes.data_as(_abi._dp), self.max_batch,
                               _abi.RSP_C128 if precision == 'c128' else _abi.RSP_C64)
        h = ct.c_void_p()
        _abi.check(self._lib.rsp_music_create(ct.byref(cfg), int(device), ct.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, '_h', None):
            self._lib.rsp_music_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- outputs -------------------------------------------------------------------------
    def _out(self, n, want_cov, want_eig=True):
        o = {'spectrum_db': np.zeros((n, self.S), np.float64), 'peaks': np.zeros((n, self.M), np.int32),
             'n_peaks': np.zeros(n, np.int32)}
        if want_eig:
            o['eig'] = np.zeros((n, self.N), np.float64)
        if want_cov:
            o['R'] = np.zeros((n, self.N, self.N, 2), np.float64)   # per instance: [b][a] = R(a, b)
        st = _abi.MusicOut(o['spectrum_db'].ctypes.data_as(_abi._dp),
                           o['eig'].ctypes.data_as(_abi._dp) if want_eig else None,
                           o['peaks'].ctypes.data_as(ct.POINTER(ct.c_int32)),
                           o['n_peaks'].ctypes.data_as(ct.POINTER(ct.c_int32)),
                           o['R'].ctypes.data_as(_abi._dp) if want_cov else None)
        return o, st

    def _finish(self, o):
        if 'R' in o:
            r = o.pop('R')
            o['R'] = np.ascontiguousarray(np.transpose(r[..., 0] + 1j * r[..., 1], (0, 2, 1)))
        pk = o['peaks']
        o['angles_deg'] = np.where(pk > 0, self.scan_rad[np.maximum(pk - 1, 0)] * 180.0 / np.pi, np.nan)
        return o

    def process(self, X, want_cov=False, want_eig=True):
        """X: complex [n, N, K] (or [N, K]) host snapshots -> dict of per-instance outputs.
        ``want_eig=False``: the eigenvalues are not read (no 'eig' key), so complex double finds
        only the M signal eigenvalues (the spectrum is still the full eigensolver's)."""
        X = np.asarray(X)
        if X.ndim == 2:
            X = X[None]
        n = X.shape[0]
        if X.shape[1:] != (self.N, self.K):
            raise ValueError('X must be [n, %d, %d], got %s' % (self.N, self.K, X.shape))
        # MATLAB column-major N x K per instance == C-order [n][K][N]
        if X.dtype == np.complex64:
            buf, dt = np.ascontiguousarray(np.transpose(X, (0, 2, 1))), _abi.RSP_C64
        else:
            buf, dt = np.ascontiguousarray(np.transpose(X.astype(np.complex128), (0, 2, 1))), _abi.RSP_C128
        o, st = self._out(n, want_cov, want_eig)
        _abi.check(self._lib.rsp_music_process(self._h, buf.ctypes.data, dt, n, ct.byref(st)))
        return self._finish(o)

    def peaks(self, X):
        """rsp_music_process on host snapshots with only the peaks requested (the eigenvalues not
        read): (peak indices [n, M] 1-based, findpeaks counts [n])."""
        X = np.asarray(X)
        if X.ndim == 2:
            X = X[None]
        n = X.shape[0]
        buf = np.ascontiguousarray(np.transpose(X.astype(np.complex128 if self.cdtype == np.complex128 else np.complex64),
                                                (0, 2, 1)))
        pk = np.zeros((n, self.M), np.int32)
        npk = np.zeros(n, np.int32)
        st = _abi.MusicOut(None, None, pk.ctypes.data_as(ct.POINTER(ct.c_int32)),
                           npk.ctypes.data_as(ct.POINTER(ct.c_int32)), None)
        dt = _abi.RSP_C128 if buf.dtype == np.complex128 else _abi.RSP_C64
        _abi.check(self._lib.rsp_music_process(self._h, buf.ctypes.data, dt, n, ct.byref(st)))
        return pk, npk

    # ---- device-resident path (bench) ------------------------------------------------------
    def device_alloc(self, n_inst):
        p = ct.c_void_p()
        _abi.check(self._lib.rsp_music_device_alloc(self._h, n_inst * self.N * self.K * np.dtype(self.cdtype).itemsize,
                                                    ct.byref(p)))
        return p.value

    def device_free(self, p):
        _abi.check(self._lib.rsp_music_device_free(self._h, ct.c_void_p(p)))

    def download(self, d_X, n_inst):
        h = np.zeros((n_inst, self.K, self.N), self.cdtype)
        _abi.check(self._lib.rsp_music_device_download(self._h, h.ctypes.data, ct.c_void_p(d_X), h.nbytes))
        return np.ascontiguousarray(np.transpose(h, (0, 2, 1)))

    def synthesize_device(self, d_X, scene, n_inst, inst0=0, seed=20250101):
        ang = list(scene['angles_rad'])
        amp = list(scene.get('amplitudes', [1.0] * len(ang)))
        sc = _abi.MusicScene(len(ang), int(scene.get('complex_sources', 0)), int(scene.get('snr_measured', 1)), 0,
                             float(scene['snr_db']), (ct.c_double * 8)(*ang), (ct.c_double * 8)(*amp))
        _abi.check(self._lib.rsp_music_synthesize_device(self._h, ct.byref(sc), n_inst, inst0, ct.c_uint64(seed),
                                                         ct.c_void_p(d_X)))

    def process_device(self, d_X, n_inst, fetch=True, want_cov=False):
        if not fetch:
            _abi.check(self._lib.rsp_music_process_device(self._h, ct.c_void_p(d_X), n_inst, None))
            return None
        o, st = self._out(n_inst, want_cov)
        _abi.check(self._lib.rsp_music_process_device(self._h, ct.c_void_p(d_X), n_inst, ct.byref(st)))
        return self._finish(o)

    def _device_into(self, d_X, n_inst, peaks, n_peaks, spec=None, eig=None):
        """Device run into caller arrays; spec / eig None: not read."""
        st = _abi.MusicOut(None if spec is None else spec.ctypes.data_as(_abi._dp),
                           None if eig is None else eig.ctypes.data_as(_abi._dp),
                           peaks.ctypes.data_as(ct.POINTER(ct.c_int32)), n_peaks.ctypes.data_as(ct.POINTER(ct.c_int32)), None)
        _abi.check(self._lib.rsp_music_process_device(self._h, ct.c_void_p(d_X), n_inst, ct.byref(st)))

    def peaks_device(self, d_X, n_inst, peaks, n_peaks):
        """Device run returning only the peak indices (into caller arrays): the bench's step."""
        self._device_into(d_X, n_inst, peaks, n_peaks)

    def eig_device(self, d_X, n_inst, eig, peaks, n_peaks):
        """Device run returning all N eigenvalues (descending, MUSIC_1D.m:29-33) and the peak indices
        into caller arrays: the form of the 3-output rsp_mex('music') / music_1d_calllib.m call,
        which always runs the full eigensolver (bench.py --want-eig)."""
        self._device_into(d_X, n_inst, peaks, n_peaks, eig=eig)

    def spectrum_device(self, d_X, n_inst, spec, peaks, n_peaks):
        """Device run returning the pseudo-spectrum P_dB ([n_inst, n_scan], MUSIC_1D.m:41) and the peak
        indices into caller arrays, without the eigenvalues: the form of the 2-output rsp_mex('music')
        call and of MUSIC_1D.m's plot (bench.py --want-spectrum)."""
        self._device_into(d_X, n_inst, peaks, n_peaks, spec=spec)

    def fast_count(self):
        """Instances of the last call answered by the block-power fast path (rsp_music_fast_count)."""
        n = ct.c_int32()
        _abi.check(self._lib.rsp_music_fast_count(self._h, ct.byref(n)))
        return n.value

    # the forms of call the profile entries time (``what``)
    FORMS = {'peaks': _abi.RSP_MUSIC_PEAKS, 'spectrum': _abi.RSP_MUSIC_SPECTRUM, 'eigenvalues': _abi.RSP_MUSIC_EIGENVALUES}

    def profile(self, d_X, n_inst, iters=20, what='peaks'):
        """HIP-event times of the two stages for the form of call ``what``: 'peaks' (the bench's
        step), 'spectrum' (spectrum_db read) or 'eigenvalues' (all N eigenvalues read)."""
        ms = (ct.c_float * 2)()
        _abi.check(self._lib.rsp_music_profile_ex(self._h, ct.c_void_p(d_X), n_inst, iters, self.FORMS[what], ms))
        return {'cov_ms': ms[0], 'eig_ms': ms[1]}


class MusicPlan2D(MusicPlan):
    """MUSIC_2D.m:50-138 for an nx x ny uniform rectangular array (rsp_music_create_2d): element
    (ix, iy) is channel iy + ny*ix (MUSIC_2D.m:17-19), the scan runs over the theta x phi grid, the
    peaks are imregionalmax's.  Complex double only.  Outputs of ``process`` / ``process_device``:
    ``spectrum_db`` [n, n_theta, n_phi] (P_MUSIC_dB), ``peaks`` (1-based linear indices
    r + n_theta (c - 1), 0 = none), ``peak_rows`` / ``peak_cols`` (1-based), ``phi_e_deg`` /
    ``theta_e_deg`` (NaN where there is no peak), ``n_peaks`` (pixels of the imregionalmax mask),
    ``eig``, ``R``."""

    def __init__(self, nx, ny, num_snapshots, num_sources, phi_rad, theta_rad, dx_over_lambda=0.5,
                 dy_over_lambda=0.5, max_batch=1, device=0):
        self._lib = _abi.lib()
        self.precision = 'c128'
        self.cdtype = np.complex128
        self.phi_rad = np.ascontiguousarray(phi_rad, np.float64)
        self.theta_rad = np.ascontiguousarray(theta_rad, np.float64)
        self.nx, self.ny = int(nx), int(ny)
        self.n_phi, self.n_theta = len(self.phi_rad), len(self.theta_rad)
        self.N, self.K, self.M = self.nx * self.ny, int(num_snapshots), int(num_sources)
        self.S = self.n_phi * self.n_theta
        self.max_batch = int(max_batch)
        cfg = _abi.Music2DConfig(self.nx, self.ny, self.K, self.M, self.n_phi, self.n_theta, float(dx_over_lambda),
                                 float(dy_over_lambda), self.phi_rad.ctypes.data_as(_abi._dp),
                                 self.theta_rad.ctypes.data_as(_abi._dp), self.max_batch, _abi.RSP_C128)
        h = ct.c_void_p()
        _abi.check(self._lib.rsp_music_create_2d(ct.byref(cfg), int(device), ct.byref(h)))
        self._h = h

    def _finish(self, o):
        if 'R' in o:
            r = o.pop('R')
            o['R'] = np.ascontiguousarray(np.transpose(r[..., 0] + 1j * r[..., 1], (0, 2, 1)))
        n = o['spectrum_db'].shape[0]
        # device order: theta fastest (MATLAB's column-major n_theta x n_phi)
        o['spectrum_db'] = np.ascontiguousarray(
            np.transpose(o['spectrum_db'].reshape(n, self.n_phi, self.n_theta), (0, 2, 1)))
        o.update(self._peak_fields(o['peaks']))
        return o

    def _peak_fields(self, pk):
        z = np.maximum(pk - 1, 0)
        rows, cols = z % self.n_theta, z // self.n_theta
        return {'peak_rows': np.where(pk > 0, rows + 1, 0), 'peak_cols': np.where(pk > 0, cols + 1, 0),
                'phi_e_deg': np.where(pk > 0, np.rad2deg(self.phi_rad[cols]), np.nan),
                'theta_e_deg': np.where(pk > 0, np.rad2deg(self.theta_rad[rows]), np.nan)}

    def synthesize_device(self, d_X, scene, n_inst, inst0=0, seed=20250101):
        az, el = list(scene['azim_rad']), list(scene['elev_rad'])
        amp = list(scene.get('amplitudes', [1.0] * len(az)))
        sc = _abi.Music2DScene(len(az), int(scene.get('complex_sources', 1)), int(scene.get('snr_measured', 1)), 0,
                               float(scene['snr_db']), (ct.c_double * 8)(*az), (ct.c_double * 8)(*el),
                               (ct.c_double * 8)(*amp))
        _abi.check(self._lib.rsp_music_synthesize_device_2d(self._h, ct.byref(sc), n_inst, inst0, ct.c_uint64(seed),
                                                            ct.c_void_p(d_X)))

    def profile(self, d_X, n_inst, iters=20, what='peaks'):
        """HIP-event times of the four stages (covariance, signal subspace, scan, dB + peaks) for the
        form of call ``what``: 'peaks', 'spectrum' or 'eigenvalues'."""
        ms = (ct.c_float * 4)()
        _abi.check(self._lib.rsp_music_profile_2d(self._h, ct.c_void_p(d_X), n_inst, iters, self.FORMS[what], ms))
        return {'cov_ms': ms[0], 'subspace_ms': ms[1], 'scan_ms': ms[2], 'peaks_ms': ms[3]}


def music_2d_scene():
    """MUSIC_2D.m:4-30,61-62: 8 x 8 array at dx = dy = lambda/2, complex sources at (phi, theta) =
    (30, 20) and (-60, 45) deg, 1000 snapshots, awgn 10 dB 'measured', scan phi = linspace(-90, 90,
    181), theta = linspace(0, 90, 91) deg.  Returns (scene dict for MusicPlan2D.synthesize_device,
    phi grid [rad], theta grid [rad], dx/lambda, dy/lambda); nx = ny = 8, K = 1000, M = 2."""
    return ({'azim_rad': np.array([30.0, -60.0]) * np.pi / 180, 'elev_rad': np.array([20.0, 45.0]) * np.pi / 180,
             'amplitudes': np.ones(2), 'complex_sources': 1, 'snr_db': 10.0, 'snr_measured': 1},
            np.linspace(-90.0, 90.0, 181) * np.pi / 180, np.linspace(0.0, 90.0, 91) * np.pi / 180, 0.5, 0.5)


def MUSIC_2D(X1, M, nx, ny, phi_list=None, theta_list=None, dx_over_lambda=0.5, dy_over_lambda=0.5, device=0):
    """MUSIC_2D.m:50-138 on one snapshot matrix X1 [nx*ny x K]: returns (phi_e [deg], theta_e [deg],
    P_MUSIC_dB [n_theta x n_phi], EVA)."""
    X1 = np.asarray(X1)
    _, phi_d, theta_d, _, _ = music_2d_scene()
    phi_list = phi_d if phi_list is None else phi_list          # MUSIC_2D.m:61
    theta_list = theta_d if theta_list is None else theta_list  # MUSIC_2D.m:62
    plan = MusicPlan2D(nx, ny, X1.shape[1], M, phi_list, theta_list, dx_over_lambda, dy_over_lambda, max_batch=1,
                       device=device)
    try:
        o = plan.process(X1)
    finally:
        plan.close()
    return o['phi_e_deg'][0], o['theta_e_deg'][0], o['spectrum_db'][0], o['eig'][0]


def music_1d_scene():
    """MUSIC_1D.m:5-35 scene at BASELINE config #5 (64 channels, 1024 snapshots): d = lambda/2,
    real sources at (-10, -30, 60) deg, awgn 10 dB 'measured', 200-point scan over +-90 deg.
    Returns (scene dict for MusicPlan.synthesize_device, scan grid [rad], d/lambda)."""
    return ({'angles_rad': np.deg2rad([-10.0, -30.0, 60.0]), 'amplitudes': np.ones(3), 'complex_sources': 0,
             'snr_db': 10.0, 'snr_measured': 1},
            np.linspace(-np.pi / 2, np.pi / 2, 200), 0.5)


def run_music_scene():
    """run_music_algorithm.m:7-20,60: 16 channels at 13.8 mm, fc 9.45 GHz, complex sources at
    2.0 / -1.5 deg with amplitudes 1 / 0.7, SNR 15 dB (fixed noise power), scan -20:0.1:20 deg."""
    wl = 2.99792458e8 / 9450e6
    return ({'angles_rad': np.deg2rad([2.0, -1.5]), 'amplitudes': np.array([1.0, 0.7]), 'complex_sources': 1,
             'snr_db': 15.0, 'snr_measured': 0},
            np.deg2rad(np.round(np.arange(-200, 201) * 0.1, 10)), 0.0138 / wl)


def MUSIC_1D(X1, M, phi_list=None, d_over_lambda=0.5, device=0, precision='c128'):
    """MUSIC_1D.m:26-48 on one snapshot matrix X1 [N x K]: returns (phi_e [deg], P_MUSIC_dB, EVA)."""
    X1 = np.asarray(X1)
    if phi_list is None:
        phi_list = np.linspace(-np.pi / 2, np.pi / 2, 200)   # MUSIC_1D.m:35
    plan = MusicPlan(X1.shape[0], X1.shape[1], M, phi_list, d_over_lambda, max_batch=1, device=device,
                     precision=precision)
    try:
        o = plan.process(X1)
    finally:
        plan.close()
    return o['angles_deg'][0], o['spectrum_db'][0], o['eig'][0]
