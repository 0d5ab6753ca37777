"""2-D MUSIC (MUSIC_2D.m) without a device: the numpy restatement tests/_music2d_ref.py pinned by
known answers, and the new C-ABI surface (struct layouts, refusals, scene constants).

The GPU parity tests are tests/test_music2d.py.
"""
import ctypes as ct
import os
import subprocess
import tempfile

import numpy as np
import pytest

import _music2d_ref as ref
from rsp import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'rsp.h')
SEED = 20250101


# ------------------------------------------------------------------ imregionalmax semantics
def _mask(rows):
    return ref.regional_max(np.array(rows, np.float64)).astype(int).tolist()


def test_regional_max_isolated_maximum():
    assert _mask([[0, 0, 0, 0], [0, 5, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0]]) == \
        [[0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0]]


def test_regional_max_border_and_corner_qualify():
    assert _mask([[9, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 7, 0, 0]]) == \
        [[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 1, 0, 0]]


def test_regional_max_two_pixel_plateau_is_whole():
    assert _mask([[0, 0, 0, 0], [0, 4, 4, 0], [0, 0, 0, 0]]) == [[0, 0, 0, 0], [0, 1, 1, 0], [0, 0, 0, 0]]


def test_regional_max_plateau_touching_a_higher_pixel_is_out():
    # the 4-plateau reaches the 5 only through its last pixel: none of it is a regional maximum
    assert _mask([[0, 0, 0, 0, 0, 0], [0, 4, 4, 4, 5, 0], [0, 0, 0, 0, 0, 0]]) == \
        [[0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 1, 0], [0, 0, 0, 0, 0, 0]]


def test_regional_max_diagonal_connection():
    # 8-connectivity: the two 3s form one plateau through the corner; with the 6 next to one of
    # them neither qualifies, without it both do
    assert _mask([[3, 0, 0], [0, 3, 6], [0, 0, 0]]) == [[0, 0, 0], [0, 0, 1], [0, 0, 0]]
    assert _mask([[3, 0, 0], [0, 3, 0], [0, 0, 0]]) == [[1, 0, 0], [0, 1, 0], [0, 0, 0]]


def test_regional_max_constant_map():
    assert ref.regional_max(np.full((3, 5), 2.5)).all()


def test_top_peaks_order_is_find_order_then_stable_descend():
    img = np.array([[1.0, 0, 7], [0, 0, 0], [7, 0, 0], [0, 0, 3]])     # 4 x 3, two equal maxima
    m = ref.regional_max(img)
    assert int(m.sum()) == 4
    # linear r + 4 c: 7 at (2, 0) -> 2 and (0, 2) -> 8; ties keep find (column-major) order
    assert list(ref.top_peaks(img, m, 3)) == [2, 8, 11]


# ------------------------------------------------------------------ known answers
GRID_PHI = np.deg2rad(np.linspace(-80.0, 80.0, 33))
GRID_THETA = np.deg2rad(np.linspace(0.0, 80.0, 17))


def test_noise_free_peaks_sit_on_the_sources():
    """Sources on the grid and no noise: Q_n is orthogonal to their steering vectors, so the two
    highest regional maxima are exactly those grid points (MUSIC_2D.m:92,119-124)."""
    scene = {'azim_rad': np.deg2rad([30.0, -60.0]), 'elev_rad': np.deg2rad([20.0, 45.0]), 'complex_sources': 1,
             'snr_db': 300.0, 'snr_measured': 1}
    X = ref.synthesize_2d(scene, 4, 4, 64, 0.5, 0.5, 0, SEED)
    r = ref.music_2d(X, 2, 4, 4, GRID_PHI, GRID_THETA, 0.5, 0.5)
    got = sorted(zip(np.round(r['phi_e_deg'], 9), np.round(r['theta_e_deg'], 9)))
    assert got == [(-60.0, 45.0), (30.0, 20.0)]
    assert np.abs(r['eig'][2:]).max() < 1e-12 * r['eig'][0]      # rank-M covariance
    assert r['spectrum_db'].shape == (17, 33)
    rows, cols = (r['peaks'] - 1) % 17, (r['peaks'] - 1) // 17   # sub2ind, theta down the rows
    assert sorted(zip(np.rad2deg(GRID_PHI[cols]).round(9), np.rad2deg(GRID_THETA[rows]).round(9))) == got


def test_element_order_is_iy_plus_ny_ix():
    """MUSIC_2D.m:17-19: meshgrid(0:Nx-1, 0:Ny-1)(:) runs y fastest.  nx != ny: a transposed
    order fails."""
    nx, ny, dxl, dyl = 3, 5, 0.5, 0.37
    phi, theta = np.deg2rad([25.0, -70.0]), np.deg2rad([10.0, 55.0])
    S = ref.steering_ura(nx, ny, dxl, dyl, phi, theta)
    assert S.shape == (15, 2)
    for ix in range(nx):
        for iy in range(ny):
            want = np.exp(1j * 2 * np.pi * (dxl * ix * np.cos(theta) * np.cos(phi)
                                            + dyl * iy * np.cos(theta) * np.sin(phi)))
            assert np.abs(S[iy + 5 * ix] - want).max() < 1e-14, (ix, iy)
    assert np.abs(S[1] - S[5]).max() > 0.1      # the x and y steps differ in this scene


# ------------------------------------------------------------------ C ABI without a device
STRUCTS = {'rsp_music2d_config': _abi.Music2DConfig, 'rsp_music2d_scene': _abi.Music2DScene}


def test_struct_layouts_match_header():
    """gcc's sizeof / offsetof of the two new structs against their ctypes mirrors."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rsp.h"', 'int main(void) {']
    for cname, py in STRUCTS.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in py._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['return 0;', '}']
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, 'probe.c'), os.path.join(d, 'probe')
        open(src, 'w').write('\n'.join(lines))
        subprocess.run(['gcc', '-I', os.path.dirname(HEADER), src, '-o', exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split('\n')
    got = dict(l.split() for l in out if l)
    for cname, py in STRUCTS.items():
        assert int(got[cname]) == ct.sizeof(py), cname
        for fname, _ in py._fields_:
            assert int(got['%s.%s' % (cname, fname)]) == getattr(py, fname).offset, (cname, fname)


def _create(nx=4, ny=4, K=64, M=2, n_phi=33, n_theta=17, precision=_abi.RSP_C128, phi=True, theta=True):
    ph, th = np.zeros(max(n_phi, 1)), np.zeros(max(n_theta, 1))
    cfg = _abi.Music2DConfig(nx, ny, K, M, n_phi, n_theta, 0.5, 0.5,
                             ph.ctypes.data_as(_abi._dp) if phi else None,
                             th.ctypes.data_as(_abi._dp) if theta else None, 1, precision)
    h = ct.c_void_p()
    lib = _abi.lib()
    rc = lib.rsp_music_create_2d(ct.byref(cfg), 0, ct.byref(h))
    msg = lib.rsp_last_error().decode(errors='replace')
    if rc == _abi.RSP_OK:
        lib.rsp_music_destroy(h)
    return rc, msg


@pytest.mark.parametrize('kw, code', [
    (dict(nx=5, ny=13), _abi.RSP_ERR_UNSUPPORTED),              # nx*ny = 65
    (dict(nx=65, ny=1), _abi.RSP_ERR_UNSUPPORTED),
    (dict(nx=1, ny=1, M=1), _abi.RSP_ERR_UNSUPPORTED),          # N = 1
    (dict(M=16), _abi.RSP_ERR_UNSUPPORTED),                     # M = N: no noise subspace
    (dict(M=9, nx=8, ny=8), _abi.RSP_ERR_UNSUPPORTED),          # M > 8
    (dict(M=0), _abi.RSP_ERR_UNSUPPORTED),
    (dict(n_phi=1024, n_theta=65), _abi.RSP_ERR_UNSUPPORTED),   # 66 560 points
    (dict(n_phi=65537, n_theta=1), _abi.RSP_ERR_UNSUPPORTED),   # n_phi*n_theta = 65 537 (a prime: only 1 x 65 537)
    (dict(n_phi=331, n_theta=198), _abi.RSP_ERR_UNSUPPORTED),   # 65 538: the least product past the cap with both axes legal
    (dict(n_theta=2), _abi.RSP_ERR_UNSUPPORTED),
    (dict(n_phi=1025, n_theta=3), _abi.RSP_ERR_UNSUPPORTED),
    (dict(precision=_abi.RSP_C64), _abi.RSP_ERR_UNSUPPORTED),
    (dict(phi=False), _abi.RSP_ERR_INVALID),                    # a null grid
    (dict(theta=False), _abi.RSP_ERR_INVALID),
    (dict(K=0), _abi.RSP_ERR_INVALID),
], ids=['n65', 'nx65', 'n1', 'm-eq-n', 'm9', 'm0', 'grid66560', 'grid65537', 'grid65538', 'ntheta2', 'nphi1025', 'c64',
        'null-phi', 'null-theta', 'k0'])
def test_create_2d_refusals(kw, code):
    """Every refusal of rsp_music_create_2d comes before any device call, with its code."""
    rc, msg = _create(**kw)
    assert rc == code, msg
    assert msg
    if kw.get('precision') == _abi.RSP_C64:
        assert 'complex double only' in msg


def test_create_2d_null_arguments():
    lib = _abi.lib()
    assert lib.rsp_music_create_2d(None, 0, None) == _abi.RSP_ERR_INVALID
    assert lib.rsp_music_synthesize_device_2d(None, None, 1, 0, 0, None) == _abi.RSP_ERR_INVALID
    assert lib.rsp_music_profile_2d(None, None, 1, 1, 0, None) == _abi.RSP_ERR_INVALID


def test_valid_2d_config_gets_past_validation():
    """The largest allowed grid and N = 64 are not refused: the call reaches the device (and on a
    machine without one reports that, as rsp_music_create does)."""
    rc, msg = _create(nx=8, ny=8, M=8, n_phi=1024, n_theta=64)
    assert rc in (_abi.RSP_OK, _abi.RSP_ERR_DEVICE), msg


def test_product_scene_equals_reference_scene():
    from rsp import music as pm
    a, b = pm.music_2d_scene(), ref.music_2d_scene()
    assert len(a) == len(b) == 5
    assert a[3] == b[3] == 0.5 and a[4] == b[4] == 0.5
    assert np.array_equal(a[1], b[1]) and len(a[1]) == 181
    assert np.array_equal(a[2], b[2]) and len(a[2]) == 91
    assert set(a[0]) == set(b[0])
    for k in b[0]:
        assert np.array_equal(np.asarray(a[0][k]), np.asarray(b[0][k])), k


def test_abi_version_unchanged():
    assert _abi.lib().rsp_abi_version() == 4
