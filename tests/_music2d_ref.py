"""2-D MUSIC for a uniform rectangular array, restated in numpy -- TEST INFRASTRUCTURE ONLY.

Restates ``MUSIC_2D.m`` the way ``oracle/music.py`` restates the 1-D scripts:

* ``MUSIC_2D.m:10-19``  -- Nx x Ny elements, ``meshgrid(0:Nx-1, 0:Ny-1)`` flattened by ``(:)``: the
  element with x-index ix and y-index iy is channel ``iy + Ny*ix``;
* ``MUSIC_2D.m:33-48``  -- complex Gaussian sources, ``awgn(X, SNR, 'measured')``;
* ``MUSIC_2D.m:52-57``  -- R = X1 X1^H / K, ``eig``, descending sort, noise subspace Q_n;
* ``MUSIC_2D.m:82-98``  -- the scan over ``meshgrid(search_phi, search_theta)`` (theta down the rows),
  ``P = 1 ./ sum(abs(Q_n' * S1).^2)``, ``P_dB = 10 log10(P / max P)``;
* ``MUSIC_2D.m:119-124`` -- ``imregionalmax`` (8-connected), ``find`` order, stable descending sort.

MATLAB's ``randn`` cannot be reproduced: the snapshots use the Philox streams documented in
``oracle/music.py`` (source index m + M*k with ``TAG_SRC``, noise index c + N*k with ``TAG_NOISE``,
c = iy + Ny*ix, counter word 2 = instance), which the device synthesis draws as well.
"""
import numpy as np

from oracle.music import TAG_NOISE, TAG_SRC
from oracle.philox import unit_normal_complex


def steering_ura(nx, ny, dx_over_lambda, dy_over_lambda, phi_rad, theta_rad):
    """a(phi, theta) = exp(1j k (x cos(theta) cos(phi) + y cos(theta) sin(phi))) for paired angle
    lists (MUSIC_2D.m:35,41-42,87-89): [nx*ny x len(phi)], row iy + ny*ix (MUSIC_2D.m:17-19)."""
    x_idx, y_idx = np.meshgrid(np.arange(nx), np.arange(ny))           # :17
    x = x_idx.flatten(order='F').astype(np.float64)[:, None] * dx_over_lambda   # :18 (in wavelengths)
    y = y_idx.flatten(order='F').astype(np.float64)[:, None] * dy_over_lambda   # :19
    phi = np.asarray(phi_rad, np.float64).ravel()[None, :]
    theta = np.asarray(theta_rad, np.float64).ravel()[None, :]
    A = np.cos(theta) * np.cos(phi)                                    # :87
    B = np.cos(theta) * np.sin(phi)                                    # :88
    return np.exp(1j * 2.0 * np.pi * (x * A + y * B))                  # :89 (k = 2 pi / lambda)


def synthesize_2d(scene, nx, ny, K, dx_over_lambda, dy_over_lambda, inst, seed):
    """One snapshot matrix X1 [nx*ny x K] (MUSIC_2D.m:36-48).  scene: azim_rad, elev_rad,
    amplitudes, complex_sources, snr_db, snr_measured as oracle.music.synthesize's."""
    az = np.asarray(scene['azim_rad'], np.float64)
    M, N = len(az), nx * ny
    amp = np.asarray(scene.get('amplitudes', np.ones(M)), np.float64)
    S = steering_ura(nx, ny, dx_over_lambda, dy_over_lambda, az, scene['elev_rad'])    # :36-43
    z = unit_normal_complex(M * K, inst, seed, tag=TAG_SRC).reshape(K, M).T           # index m + M k
    if scene.get('complex_sources', 1):
        alpha = z / np.sqrt(2.0) * amp[:, None]                                        # :46
    else:
        alpha = z.real * amp[:, None]
    X = S @ alpha                                                                      # :47
    if scene.get('snr_measured', 1):
        p_noise = np.sum(np.abs(X) ** 2) / X.size / 10.0 ** (scene['snr_db'] / 10.0)  # :48 'measured'
    else:
        p_noise = 1.0 / 10.0 ** (scene['snr_db'] / 10.0)
    n = unit_normal_complex(N * K, inst, seed, tag=TAG_NOISE).reshape(K, N).T          # index c + N k
    return X + np.sqrt(p_noise / 2.0) * n


def regional_max(img):
    """``imregionalmax(img)`` with the default 8-connectivity (MUSIC_2D.m:119), by literal flood
    fill: a pixel is in the mask iff its plateau (the 8-connected component of equal values that
    holds it) has no in-bounds neighbour with a larger value.  Border pixels qualify."""
    img = np.asarray(img, np.float64)
    nr, nc = img.shape
    mask = np.zeros((nr, nc), bool)
    seen = np.zeros((nr, nc), bool)
    for r0 in range(nr):
        for c0 in range(nc):
            if seen[r0, c0]:
                continue
            v = img[r0, c0]
            comp, stack, is_max = [], [(r0, c0)], True
            seen[r0, c0] = True
            while stack:
                r, c = stack.pop()
                comp.append((r, c))
                for rr in range(max(r - 1, 0), min(r + 2, nr)):
                    for cc in range(max(c - 1, 0), min(c + 2, nc)):
                        u = img[rr, cc]
                        if u > v:
                            is_max = False
                        elif u == v and not seen[rr, cc]:
                            seen[rr, cc] = True
                            stack.append((rr, cc))
            if is_max:
                for r, c in comp:
                    mask[r, c] = True
    return mask


def top_peaks(PdB, mask, M):
    """MUSIC_2D.m:120-127: ``find`` order (column-major), stable sort 'descend', the first M as
    0-based linear indices r + n_theta*c."""
    lin = np.flatnonzero(mask.flatten(order='F'))
    vals = PdB.flatten(order='F')[lin]
    return lin[np.argsort(-vals, kind='stable')][:M]


def largest_neighbour(img):
    """Per pixel the largest in-bounds 8-neighbour value (the test's tie-margin precondition)."""
    img = np.asarray(img, np.float64)
    nr, nc = img.shape
    pad = np.full((nr + 2, nc + 2), -np.inf)
    pad[1:-1, 1:-1] = img
    out = np.full((nr, nc), -np.inf)
    for dr in (0, 1, 2):
        for dc in (0, 1, 2):
            if dr != 1 or dc != 1:
                out = np.maximum(out, pad[dr:dr + nr, dc:dc + nc])
    return out


def music_2d(X, M, nx, ny, phi_rad, theta_rad, dx_over_lambda, dy_over_lambda):
    """MUSIC_2D.m:52-127 on one snapshot matrix X [nx*ny x K] (complex128, like MATLAB)."""
    N, K = X.shape
    R = X @ X.conj().T / K                                   # :52
    R = 0.5 * (R + R.conj().T)                               # herk output is exactly Hermitian
    w, V = np.linalg.eigh(R)                                 # :53-54 (ascending)
    order = np.argsort(-w, kind='stable')                    # :55
    Qn = V[:, order][:, M:]                                  # :56-57
    phi = np.asarray(phi_rad, np.float64)
    theta = np.asarray(theta_rad, np.float64)
    Phi, Theta = np.meshgrid(phi, theta)                     # :82 ([n_theta x n_phi])
    S1 = steering_ura(nx, ny, dx_over_lambda, dy_over_lambda, Phi.flatten(order='F'),
                      Theta.flatten(order='F'))              # :83-89
    denom = np.sum(np.abs(Qn.conj().T @ S1) ** 2, axis=0)    # :92
    P = np.abs(1.0 / denom).reshape(len(theta), len(phi), order='F')   # :93,96
    PdB = 10.0 * np.log10(P / P.max())                       # :97-98
    mask = regional_max(PdB)                                 # :119
    top = top_peaks(PdB, mask, M)                            # :120-127
    return {'R': R, 'eig': w[order], 'spectrum_db': PdB, 'mask': mask, 'peaks': top + 1,
            'n_peaks': int(mask.sum()),
            'phi_e_deg': np.rad2deg(phi[top // len(theta)]), 'theta_e_deg': np.rad2deg(theta[top % len(theta)])}


def music_2d_scene():
    """MUSIC_2D.m:4-30,61-62: (scene, phi grid, theta grid, dx/lambda, dy/lambda); nx = ny = 8,
    K = 1000, M = 2."""
    return ({'azim_rad': np.array([30.0, -60.0]) * np.pi / 180,      # :24
             'elev_rad': np.array([20.0, 45.0]) * np.pi / 180,       # :25
             'amplitudes': np.ones(2), 'complex_sources': 1,         # :46
             'snr_db': 10.0, 'snr_measured': 1},                     # :29,48
            np.linspace(-90.0, 90.0, 181) * np.pi / 180,             # :61,82
            np.linspace(0.0, 90.0, 91) * np.pi / 180,                # :62,82
            0.5, 0.5)                                                # :13-14
