"""CPU tests of the stand-alone MTD's device-free half: the exported symbols and the ctypes mirrors
against the header, every refusal of rsp_mtd_describe (the checks of all the rsp_mtd calls) with its
code and message, the refusal of null pointers without a device, route / M / tiling per case, and the
host code in a stand-alone program under AddressSanitizer / UBSan (native/mtd_host_check.cpp)."""
import ctypes as ct
import os
import shutil
import subprocess
import tempfile

import pytest

from rsp import _abi
from rsp.plan import describe_mtd, mtd_table
from _mtd_cases import CASES, CASE_IDS, COLUMN_CASES, PRECS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INCLUDE = os.path.join(ROOT, 'include')
CSRC = os.path.join(ROOT, 'radar-signal-simulation-and-target-detection_amd', 'csrc')
SYMBOLS = {'rsp_mtd_describe': 5, 'rsp_mtd_table': 5, 'rsp_mtd': 10, 'rsp_mtd_device': 9, 'rsp_profile_mtd': 8}

PROBE = r'''
#include <stdio.h>
#include <stddef.h>
#include "rsp.h"
int32_t (*f_describe)(int32_t, int32_t, int32_t, int32_t, rsp_mtd_info*) = rsp_mtd_describe;
int32_t (*f_table)(int32_t, int32_t, double*, int32_t, int32_t*) = rsp_mtd_table;
int32_t (*f_mtd)(rsp_plan*, int32_t, int32_t, int32_t, int32_t, const void*, int32_t, const double*, int32_t, double*) = rsp_mtd;
int32_t (*f_dev)(rsp_plan*, int32_t, int32_t, int32_t, int32_t, const void*, const double*, int32_t, void*) = rsp_mtd_device;
int32_t (*f_prof)(rsp_plan*, int32_t, int32_t, int32_t, int32_t, int32_t, float*, int64_t*) = rsp_profile_mtd;
int main(void) {
    rsp_mtd_info i;
    if (f_describe(332, 3404, 0, RSP_C128, &i) != RSP_OK) return 2;
    if (f_mtd(0, 4, 1, 1, 4, 0, RSP_C128, 0, 1, 0) != RSP_ERR_INVALID) return 3;
    if (f_dev(0, 4, 1, 1, 4, 0, 0, 1, 0) != RSP_ERR_INVALID) return 4;
    if (f_prof(0, 4, 1, 1, 4, 1, 0, 0) != RSP_ERR_INVALID) return 5;
    printf("%zu %zu %zu %d %d %d %d %d\n", sizeof(rsp_mtd_info), offsetof(rsp_mtd_info, route), offsetof(rsp_mtd_info, table_elems),
           RSP_ABI_VERSION, RSP_MTD_MAX_NFFT, RSP_MTD_ROUTE_POW2, RSP_MTD_ROUTE_CHIRPZ, RSP_MTD_ROUTE_DIRECT);
    printf("%d %d %d %d %d %d %d\n", i.P, i.G, i.nfft, i.route, i.M, i.col_tiles * i.cols >= i.G, i.table_elems);
    return 0;
}
'''


def test_abi_version_and_symbols():
    lib = _abi.lib()
    assert lib.rsp_abi_version() == 4
    for n, nargs in SYMBOLS.items():
        assert hasattr(lib, n), 'librsp.so does not export %s' % n
        assert len(_abi.PROTOTYPES[n][1]) == nargs


def test_declared_signatures_and_layout_against_the_header():
    libdir = os.path.dirname(_abi.lib()._name)
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, 'probe.c'), os.path.join(d, 'probe')
        open(src, 'w').write(PROBE)
        subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-I', INCLUDE, src, '-o', exe, '-L', libdir, '-lrsp',
                        '-Wl,-rpath,' + libdir], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split('\n')
    assert [int(x) for x in out[0].split()] == [ct.sizeof(_abi.MtdInfo), _abi.MtdInfo.route.offset,
                                                _abi.MtdInfo.table_elems.offset, 4, _abi.RSP_MTD_MAX_NFFT,
                                                _abi.RSP_MTD_ROUTE_POW2, _abi.RSP_MTD_ROUTE_CHIRPZ, _abi.RSP_MTD_ROUTE_DIRECT]
    assert ct.sizeof(_abi.MtdInfo) == 36
    assert [int(x) for x in out[1].split()] == [332, 3404, 332, 1, 1024, 1, 332 + 1024]


@pytest.mark.parametrize('args, code, word', [
    ((0, 5, None), _abi.RSP_ERR_INVALID, 'bad sizes P=0 G=5 n_maps=1 nfft=0'),
    ((-3, 5, 8), _abi.RSP_ERR_INVALID, 'bad sizes P=-3 G=5 n_maps=1 nfft=8'),
    ((332, 5, 331), _abi.RSP_ERR_INVALID, 'bad sizes P=332 G=5 n_maps=1 nfft=331 (P, G, n_maps >= 1, nfft >= P or 0)'),
    ((332, 5, 2049), _abi.RSP_ERR_UNSUPPORTED, 'nfft=2049: a transform holds at most RSP_MTD_MAX_NFFT = 2048 points'),
    ((2049, 5, None), _abi.RSP_ERR_UNSUPPORTED, 'nfft=2049'),
    ((332, 0, 512), _abi.RSP_ERR_INVALID, 'bad sizes P=332 G=0 n_maps=1 nfft=512'),
    ((2048, 65536, 2048), _abi.RSP_ERR_UNSUPPORTED, '65536 x 1 columns of 2048 points: the kernel addresses a cube of less than 2 GB'),
])
def test_refusals_and_messages(args, code, word):
    with pytest.raises(_abi.RspError) as e:
        describe_mtd(*args, precision='c128')
    assert e.value.code == code
    assert word in str(e.value), str(e.value)


def test_two_gigabytes_is_by_the_precision():
    """2048 x 65536 columns are 2 GB in complex double and 1 GB in complex single."""
    assert describe_mtd(2048, 65536, 2048, 'c64')['col_tiles'] == 65536 // describe_mtd(2048, 1, 2048, 'c64')['cols']
    assert describe_mtd(2048, 65535, 2048, 'c128')['nfft'] == 2048


def test_bad_precision():
    lib = _abi.lib()
    assert lib.rsp_mtd_describe(8, 8, 8, 5, None) == _abi.RSP_ERR_INVALID
    assert b'precision must be RSP_C128 or RSP_C64, got 5' in lib.rsp_last_error()
    n = ct.c_int32()
    assert lib.rsp_mtd_table(8, 5, None, 0, ct.byref(n)) == _abi.RSP_ERR_INVALID
    with pytest.raises(ValueError):
        describe_mtd(8, 8, 8, 'c32')


def test_null_arguments_are_refused_without_a_device():
    """Sizes, dtype, null pointers, in that order, before any device work: with no plan at all."""
    lib = _abi.lib()
    x = (ct.c_double * 64)()
    xp = ct.cast(x, ct.c_void_p)
    xd = ct.cast(x, ct.POINTER(ct.c_double))
    assert lib.rsp_mtd(None, 4, 2, 1, 4, None, _abi.RSP_C128, None, 1, xd) == _abi.RSP_ERR_INVALID     # null pc
    assert b'null argument' in lib.rsp_last_error()
    assert lib.rsp_mtd(None, 4, 2, 1, 4, xp, _abi.RSP_C128, None, 1, None) == _abi.RSP_ERR_INVALID   # null out
    assert b'null argument' in lib.rsp_last_error()
    assert lib.rsp_mtd(None, 4, 2, 1, 4, xp, _abi.RSP_C128, None, 1, xd) == _abi.RSP_ERR_INVALID     # null plan
    assert lib.rsp_mtd(None, 4, 2, 1, 4, None, 99, None, 1, None) == _abi.RSP_ERR_INVALID            # dtype before pointers
    assert b'unknown dtype 99' in lib.rsp_last_error()
    assert lib.rsp_mtd(None, 4, 2, 1, 3, None, 99, None, 1, None) == _abi.RSP_ERR_INVALID            # sizes before dtype
    assert b'bad sizes' in lib.rsp_last_error()
    assert lib.rsp_mtd(None, 4, 2, 1, 4096, None, 99, None, 1, None) == _abi.RSP_ERR_UNSUPPORTED
    assert lib.rsp_mtd(None, 4, 2, 0, 4, xp, _abi.RSP_C128, None, 1, xd) == _abi.RSP_ERR_INVALID     # n_maps < 1
    assert lib.rsp_mtd_device(None, 4, 2, 1, 4, None, None, 1, None) == _abi.RSP_ERR_INVALID
    assert lib.rsp_mtd_device(None, 4, 2, 1, 2, xp, None, 1, xp) == _abi.RSP_ERR_INVALID
    assert b'bad sizes' in lib.rsp_last_error()
    assert lib.rsp_profile_mtd(None, 4, 2, 1, 4, 1, None, None) == _abi.RSP_ERR_INVALID
    assert lib.rsp_mtd_describe(4, 2, 4, _abi.RSP_C128, None) == _abi.RSP_OK                          # info may be NULL
    n = ct.c_int32()
    assert lib.rsp_mtd_table(5, _abi.RSP_C128, None, 3, ct.byref(n)) == _abi.RSP_ERR_INVALID
    assert lib.rsp_mtd_table(5, _abi.RSP_C128, None, 0, None) == _abi.RSP_ERR_INVALID


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('P, nfft', CASES, ids=CASE_IDS)
def test_describe_route_and_tiling(P, nfft, prec):
    esz = 16 if prec == 'c128' else 8
    one = describe_mtd(P, 1, nfft, prec)
    cols = one['cols']
    pow2 = nfft & (nfft - 1) == 0
    for G in sorted({1, cols - 1, cols, cols + 1, 2 * cols + 1, 3404} - {0}):
        d = describe_mtd(P, G, nfft, prec)
        assert (d['P'], d['G'], d['nfft']) == (P, G, nfft)
        assert d['route'] == ('pow2' if pow2 else 'chirpz')
        if pow2:
            assert d['M'] == nfft and d['table_elems'] == 0
        else:
            M = d['M']
            assert M & (M - 1) == 0 and M >= 2 * nfft - 1 and M // 2 < 2 * nfft - 1
            assert d['table_elems'] == nfft + M
        assert d['cols'] == cols and d['col_tiles'] == -(-G // cols)
        assert cols * d['M'] * esz <= d['lds_bytes'] <= 160 * 1024
    assert describe_mtd(P, 3, None if nfft == P else nfft, prec)['nfft'] == nfft
    w, Bf = mtd_table(nfft, prec)
    assert (len(w), len(Bf)) == ((0, 0) if pow2 else (nfft, one['M']))


def test_column_cases_cover_every_route_and_length():
    """The column sweep of tests/test_mtd.py runs one case per (route, M) of the table."""
    for prec in PRECS:
        seen = {(describe_mtd(P, 1, n, prec)['route'], describe_mtd(P, 1, n, prec)['M']) for P, n in CASES}
        assert seen == set(COLUMN_CASES)
        for (route, M), (P, n) in COLUMN_CASES.items():
            d = describe_mtd(P, 1, n, prec)
            assert (d['route'], d['M']) == (route, M) and (P, n) in CASES


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_mtd_host_code_under_sanitizers(tmp_path):
    """rsp_mtd_describe and rsp_mtd_table (cap = 0, a short cap, nfft = 1, 2, 3, 2047, 2048) in a
    stand-alone program (native/mtd_host_check.cpp) under AddressSanitizer / UBSan, on the CPU."""
    exe = str(tmp_path / 'mtd_host_check')
    subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                    '-fno-omit-frame-pointer', '-I', INCLUDE, '-I', CSRC, os.path.join(CSRC, 'rsp_host.cpp'),
                    os.path.join(CSRC, 'rsp_geometry.cpp'), os.path.join(HERE, 'native', 'mtd_host_check.cpp'),
                    '-o', exe, '-lpthread'], check=True)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and 'ERROR: AddressSanitizer' not in r.stderr and 'runtime error' not in r.stderr, \
        (r.stderr + r.stdout)[-3000:]
    assert 'accepted' in r.stdout
