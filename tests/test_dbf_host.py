"""The device-free half of the stage-1 DBF (rsp_dbf_table, rsp_dbf_describe, the refusals of rsp_dbf).

A table is checked by reconstructing the DBF from it alone: row m of block mb holds, per channel, the
coefficients of Re x and Im x of one part (Re or Im) of one beam, so
``part = sum_c coefRe[c] Re x_c + coefIm[c] Im x_c`` over the table must give ``x @ conj(W).T`` (conj) or
``x @ W.T`` in float64, to 1e-15 of the largest output (each output is a sum of at most 64 products, the
reference's own error is of that order).  The table build_tables makes for K1 is compared bit for bit
with tests/golden/dbf_atab_parent.npz, written by the commit before the builder was taken out of
build_tables (rsp_plan_derive's PlanHost::atab for the `plumbing` waveform at each (C, B)).
"""
import ctypes as ct
import os
import shutil
import subprocess

import numpy as np
import pytest

from rsp import _abi
from rsp import config as C
from rsp.plan import dbf_table, describe_dbf, describe_dbf_table
from rsp.precompute import precompute as product_precompute
from _scen import plumbing_config, plumbing_weights

CB = [(1, 1), (3, 1), (5, 3), (12, 3), (16, 8), (16, 9), (16, 13), (32, 16)]
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, 'radar-signal-simulation-and-target-detection_amd', 'csrc')
GOLDEN = os.path.join(HERE, 'golden', 'dbf_atab_parent.npz')


def _weights(Cn, B, seed=7):
    rng = np.random.default_rng(seed + 100 * Cn + B)
    return rng.standard_normal((B, Cn)) + 1j * rng.standard_normal((B, Cn))


def _row_of(layout, b, part):
    """(block, MFMA row) of (beam, part) in a row layout, as include/rsp.h states it."""
    mb, bl = divmod(b, 8)
    return (mb, bl + 8 * part) if layout == 'split' else (mb, 2 * bl + part)


def _apply(tab, Cn, B, layout, x):
    """y [n, B] from the table alone, x [n, Cn]."""
    nj = tab.shape[0] // (1 if B <= 8 else 2)
    y = np.zeros((x.shape[0], B), complex)
    for b in range(B):
        for part in (0, 1):
            mb, m = _row_of(layout, b, part)
            acc = np.zeros(x.shape[0])
            for c in range(Cn):
                j, g = divmod(c, 4)
                lane = m + 16 * g
                acc += tab[mb * nj + j, 0, lane] * x[:, c].real + tab[mb * nj + j, 1, lane] * x[:, c].imag
            y[:, b] += acc if part == 0 else 1j * acc
    return y


@pytest.mark.parametrize('layout', ['split', 'pair'])
@pytest.mark.parametrize('conj', [True, False])
@pytest.mark.parametrize('Cn,B', CB)
def test_table_reconstructs_the_dbf(Cn, B, conj, layout):
    W = _weights(Cn, B)
    tab = dbf_table(W, conj=conj, row_layout=layout)
    cp = 8 if Cn <= 8 else 16 if Cn <= 16 else 32
    assert tab.shape == ((1 if B <= 8 else 2) * cp // 4, 2, 64)
    rng = np.random.default_rng(11)
    x = rng.standard_normal((9, Cn)) + 1j * rng.standard_normal((9, Cn))
    want = x @ (W.conj().T if conj else W.T)
    got = _apply(tab, Cn, B, layout, x)
    err = np.abs(got - want).max() / np.abs(want).max()
    print('C=%d B=%d conj=%d %s: rel err %.3g' % (Cn, B, conj, layout, err))
    assert err <= 1e-15
    assert np.abs(_apply(tab, Cn, B, layout, x) - x @ (W.T if conj else W.conj().T)).max() > 1e-3   # the flag matters
    # padded beams and channels carry zero weights: every entry the reconstruction did not read is 0
    used = np.zeros(tab.shape, bool)
    nj = cp // 4
    for b in range(B):
        for part in (0, 1):
            mb, m = _row_of(layout, b, part)
            for c in range(Cn):
                used[mb * nj + c // 4, :, m + 16 * (c % 4)] = True
    assert not tab[~used].any()


@pytest.mark.parametrize('Cn,B', [(3, 1), (5, 3), (12, 3), (16, 8), (16, 9), (16, 13), (32, 13)])
def test_k1_table_is_unchanged(Cn, B):
    """build_tables' table (what a plan uploads for K1) equals the parent commit's, bit for bit, and is
    what the builder returns for (conj, split)."""
    g = np.load(GOLDEN)
    cfg = plumbing_config(16, B, Cn)
    W, ang, k = plumbing_weights(cfg)
    assert np.array_equal(np.asarray(W, complex), g['w_c%d_b%d' % (Cn, B)])
    pre = product_precompute(cfg, W, ang, k, C.V8_FIR)
    tab = describe_dbf_table(cfg, C.default_cfar_params(), C.default_cluster_params(), pre)
    want = g['atab_c%d_b%d' % (Cn, B)]
    assert tab.size == want.size
    assert tab.ravel().tobytes() == want.tobytes()          # -0.0 of the padded entries included
    assert tab.tobytes() == dbf_table(W, conj=True, row_layout='split').tobytes()


def _wg(Cn, B, prec):
    return describe_dbf(1, 1, Cn, B, prec)['wg_positions']


@pytest.mark.parametrize('prec', ['c128', 'c64'])
@pytest.mark.parametrize('Cn,B', CB)
def test_describe_covers_every_position_once(Cn, B, prec):
    wg = _wg(Cn, B, prec)
    for S in (1, 15, 16, 17, 35, wg - 1, wg, wg + 1):
        for P, N in ((1, S), (S, 1)) + (((5, S // 5),) if S % 5 == 0 else ()):
            d = describe_dbf(P, N, Cn, B, prec)
            assert d['positions'] == S
            assert d['sub_tile'] == (16 if prec == 'c128' else 32) and d['waves'] == 4
            assert d['row_layout'] == ('split' if prec == 'c128' else 'pair')
            assert d['wg_positions'] == d['waves'] * d['rounds'] * d['tiles_per_wave'] * d['sub_tile'] == wg
            # workgroup w takes positions [w wg, (w + 1) wg): the last one starts inside S and reaches its end
            assert (d['workgroups'] - 1) * wg < S <= d['workgroups'] * wg
            assert d['tail_positions'] == S % d['sub_tile']
            assert d['pitch'] >= S and (prec == 'c128' or d['pitch'] % 2 == 0) and d['pitch'] - S <= 1
    # tiles_per_wave is K1's: 16 16-B registers of loads per lane
    d = describe_dbf(1, 1, Cn, B, prec)
    assert d['tiles_per_wave'] * (d['CP'] // 4) * (1 if d['BMAX'] <= 8 else 2) <= 16
    assert d['CP'] >= Cn and d['BMAX'] >= B


def _refused(rc, word):
    assert rc == _abi.RSP_ERR_INVALID
    assert word in _abi.lib().rsp_last_error().decode(), _abi.lib().rsp_last_error()


def test_refusals_without_a_device():
    lib = _abi.lib()
    x = np.zeros((2, 3, 4), np.complex128, order='F')
    W = np.zeros(2 * 2 * 4)
    out = np.zeros((2, 3, 2), np.complex128, order='F')
    xp, op = x.ctypes.data_as(ct.c_void_p), out.ctypes.data_as(ct.POINTER(ct.c_double))
    wp = W.ctypes.data_as(ct.POINTER(ct.c_double))
    _refused(lib.rsp_dbf(None, 2, 3, 0, 2, xp, _abi.RSP_C128, wp, 1, op), 'C=0')
    _refused(lib.rsp_dbf(None, 2, 3, 33, 2, xp, _abi.RSP_C128, wp, 1, op), 'C=33')
    _refused(lib.rsp_dbf(None, 2, 3, 4, 17, xp, _abi.RSP_C128, wp, 1, op), 'B=17')
    _refused(lib.rsp_dbf(None, 0, 3, 4, 2, xp, _abi.RSP_C128, wp, 1, op), 'P=0')
    _refused(lib.rsp_dbf(None, 2, 3, 4, 2, xp, _abi.RSP_C128, None, 1, op), 'W')
    _refused(lib.rsp_dbf(None, 2, 3, 4, 2, xp, 7, wp, 1, op), 'dtype 7')
    _refused(lib.rsp_dbf(None, 2, 3, 4, 2, xp, _abi.RSP_C128, wp, 1, op), 'null')          # the plan itself
    for bad in ((2, 3, 0, 2), (2, 3, 33, 2), (2, 3, 4, 17), (2, 0, 4, 2)):
        with pytest.raises(_abi.RspError) as e:
            describe_dbf(*bad)
        assert e.value.code == _abi.RSP_ERR_INVALID
    with pytest.raises(_abi.RspError) as e:
        describe_dbf(1 << 14, 1 << 14, 32, 16)      # 2^28 positions x 32 channels x 16 B
    assert e.value.code == _abi.RSP_ERR_UNSUPPORTED
    n = ct.c_int32()
    _refused(lib.rsp_dbf_table(None, 2, 4, 1, 0, None, 0, ct.byref(n)), 'null')
    _refused(lib.rsp_dbf_table(wp, 2, 4, 1, 2, None, 0, ct.byref(n)), 'layout')
    _refused(lib.rsp_dbf_table(wp, 17, 4, 1, 0, None, 0, ct.byref(n)), 'B=17')
    _refused(lib.rsp_profile_dbf(None, 2, 3, 4, 2, 1, None, None), 'bad argument')
    _refused(lib.rsp_process_raw_stage2(None, xp, _abi.RSP_C128, 0, None, wp, 1, None, None), 'null')


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_dbf_host_code_under_sanitizers(tmp_path):
    """The table builder, the checks, the tiling and the regating on C channels in a stand-alone
    program (native/dbf_host_check.cpp) under AddressSanitizer / UBSan, on the CPU."""
    exe = str(tmp_path / 'dbf_host_check')
    subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                    '-fno-omit-frame-pointer', '-I', os.path.join(ROOT, 'include'), '-I', CSRC,
                    os.path.join(CSRC, 'rsp_host.cpp'), os.path.join(CSRC, 'rsp_geometry.cpp'),
                    os.path.join(CSRC, 'rsp_frame_host.cpp'), os.path.join(HERE, 'native', 'dbf_host_check.cpp'),
                    '-o', exe, '-lpthread'], check=True)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and 'ERROR: AddressSanitizer' not in r.stderr and 'runtime error' not in r.stderr, \
        (r.stdout + r.stderr)[-3000:]
    assert '2048 tables' in r.stdout
