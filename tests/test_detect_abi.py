"""CPU tests of the detect calls' C ABI: the exported symbols and their ctypes prototypes, the struct
layouts against a compiled C program (as test_xcfar_abi.py does), and the null-argument refusals that
need no device."""
import ctypes as ct
import os
import subprocess
import tempfile

from rsp import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
INCLUDE = os.path.join(os.path.dirname(HERE), 'include')
SYMBOLS = {'rsp_detect_describe': 6, 'rsp_detect': 8, 'rsp_detect_device': 7, 'rsp_mtd_detect': 10,
           'rsp_process_stage2_detect': 4, 'rsp_profile_detect': 8}

PROBE = r'''
#include <stdio.h>
#include <stddef.h>
#include "rsp.h"
int32_t (*f_describe)(int32_t, int32_t, int32_t, int32_t, const rsp_cfar_params*, rsp_detect_info*) = rsp_detect_describe;
int32_t (*f_detect)(rsp_plan*, int32_t, int32_t, int32_t, const void*, int32_t, const rsp_detect_params*, rsp_frame_out*) = rsp_detect;
int32_t (*f_device)(rsp_plan*, int32_t, int32_t, int32_t, const void*, const rsp_detect_params*, rsp_frame_out*) = rsp_detect_device;
int32_t (*f_mtd)(rsp_plan*, int32_t, int32_t, int32_t, int32_t, const void*, int32_t, const double*, const rsp_detect_params*,
                 rsp_frame_out*) = rsp_mtd_detect;
int32_t (*f_stage2)(rsp_plan*, const void*, int32_t, rsp_frame_out*) = rsp_process_stage2_detect;
int32_t (*f_prof)(rsp_plan*, int32_t, int32_t, int32_t, const rsp_cfar_params*, int32_t, float*, int64_t*) = rsp_profile_detect;
int main(void) {
    rsp_cfar_params p = {5, 10, 5, 10, 8.0};
    rsp_detect_params dp = {{5, 10, 5, 10, 8.0}, {1, 1, 1}, 0, 0, 1.0, 1.0, 0, 0, 0, 0};
    rsp_detect_info i;
    if (f_describe(512, 3404, 13, RSP_C128, &p, &i) != RSP_OK) return 2;
    if (f_detect(0, 64, 64, 3, 0, RSP_C128, &dp, 0) != RSP_ERR_INVALID) return 3;
    if (f_device(0, 64, 64, 3, 0, &dp, 0) != RSP_ERR_INVALID) return 4;
    if (f_mtd(0, 32, 64, 3, 64, 0, RSP_C128, 0, &dp, 0) != RSP_ERR_INVALID) return 5;
    if (f_stage2(0, 0, RSP_C128, 0) != RSP_ERR_INVALID) return 6;
    if (f_prof(0, 64, 64, 3, &p, 1, 0, 0) != RSP_ERR_INVALID) return 7;
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(rsp_detect_params), offsetof(rsp_detect_params, cluster),
           offsetof(rsp_detect_params, range_axis), offsetof(rsp_detect_params, monopulse), sizeof(rsp_detect_info),
           offsetof(rsp_detect_info, lds_bytes), offsetof(rsp_detect_info, cells_under_test), sizeof(rsp_frame_out),
           RSP_ABI_VERSION);
    printf("%d %d %d %d %d %d %d %d %d %lld %lld\n", i.n_pairs, i.rows, i.cols, i.row_tiles, i.col_tiles, i.r0, i.r1, i.v0, i.v1,
           (long long)i.cells_under_test, (long long)i.max_detections);
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
    P, I = _abi.DetectParams, _abi.DetectInfo
    assert [int(x) for x in out[0].split()] == [ct.sizeof(P), P.cluster.offset, P.range_axis.offset, P.monopulse.offset, ct.sizeof(I),
                                                I.lds_bytes.offset, I.cells_under_test.offset, ct.sizeof(_abi.FrameOut), 4]
    assert ct.sizeof(P) == 104 and ct.sizeof(I) == 72
    assert [int(x) for x in out[1].split()] == [12, 64, 64, 8, 54, 16, 3389, 16, 497, 482 * 3374, 12 * 482 * 3374]


def test_null_arguments_need_no_device():
    lib = _abi.lib()
    dp = _abi.DetectParams(cfar=_abi.CfarParams(refCells_V=5, guardCells_V=10, refCells_R=5, guardCells_R=10, T_CFAR=8.0))
    assert lib.rsp_detect(None, 64, 64, 3, None, _abi.RSP_C128, ct.byref(dp), None) == _abi.RSP_ERR_INVALID
    assert b'null' in lib.rsp_last_error()
    assert lib.rsp_detect(None, 64, 64, 3, None, 9, ct.byref(dp), None) == _abi.RSP_ERR_INVALID
    assert b'unknown dtype 9' in lib.rsp_last_error()          # sizes, then the dtype, then the pointers
    assert lib.rsp_detect(None, 64, 64, 1, None, 9, ct.byref(dp), None) == _abi.RSP_ERR_INVALID and b'B=1' in lib.rsp_last_error()
    assert lib.rsp_detect_device(None, 64, 64, 3, None, ct.byref(dp), None) == _abi.RSP_ERR_INVALID
    assert lib.rsp_mtd_detect(None, 64, 8, 3, 32, None, _abi.RSP_C128, None, ct.byref(dp), None) == _abi.RSP_ERR_INVALID
    assert b'nfft' in lib.rsp_last_error()
    assert lib.rsp_process_stage2_detect(None, None, _abi.RSP_C128, None) == _abi.RSP_ERR_INVALID
    assert lib.rsp_profile_detect(None, 64, 64, 3, ct.byref(dp.cfar), 1, None, None) == _abi.RSP_ERR_INVALID
