"""CPU tests of the digital down-converter's C ABI: the exported symbols and the ctypes mirrors against the
header (the layouts of rsp_ddc_params and rsp_ddc_info through a compiled C probe), the new dtype values, the
version, and the refusals that need no device, in their documented order."""
import ctypes as ct
import os
import subprocess
import tempfile

from rsp import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INCLUDE = os.path.join(ROOT, 'include')
SYMBOLS = {'rsp_ddc_describe': 8, 'rsp_ddc_phase_word': 3, 'rsp_ddc': 8, 'rsp_ddc_device': 7, 'rsp_ddc_raw_detect': 14,
           'rsp_profile_ddc': 10}

PROBE = r'''
#include <stdio.h>
#include <stddef.h>
#include "rsp.h"
int32_t (*f_describe)(int32_t, int32_t, int32_t, int32_t, int32_t, int32_t, int32_t, rsp_ddc_info*) = rsp_ddc_describe;
int32_t (*f_word)(double, double, uint64_t*) = rsp_ddc_phase_word;
int32_t (*f_ddc)(rsp_plan*, int32_t, int32_t, int32_t, const void*, int32_t, const rsp_ddc_params*, double*) = rsp_ddc;
int32_t (*f_dev)(rsp_plan*, int32_t, int32_t, int32_t, const void*, const rsp_ddc_params*, void*) = rsp_ddc_device;
int32_t (*f_chain)(rsp_plan*, int32_t, int32_t, int32_t, const void*, int32_t, const rsp_ddc_params*, int32_t, int32_t,
                   const double*, int32_t, const double*, const rsp_detect_params*, rsp_frame_out*) = rsp_ddc_raw_detect;
int32_t (*f_prof)(rsp_plan*, int32_t, int32_t, int32_t, int32_t, int32_t, int32_t, int32_t, float*, int64_t*) = rsp_profile_ddc;
int main(void) {
    rsp_ddc_info info;
    uint64_t w = 0;
    if (f_describe(332, 23276, 16, 12, 4, 0, RSP_C128, &info) != RSP_OK || info.No != 5819) return 2;
    if (f_word(10e6, 100e6, &w) != RSP_OK || w != 1844674407370955162ull) return 3;
    if (f_ddc(0, 4, 8, 1, 0, RSP_R64, 0, 0) != RSP_ERR_INVALID) return 4;
    if (f_dev(0, 4, 8, 1, 0, 0, 0) != RSP_ERR_INVALID) return 5;
    if (f_chain(0, 4, 8, 1, 0, RSP_R64, 0, 1, 4, 0, 1, 0, 0, 0) != RSP_ERR_INVALID) return 6;
    if (f_prof(0, 4, 8, 1, 12, 4, 0, 1, 0, 0) != RSP_ERR_INVALID) return 7;
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(rsp_ddc_params), offsetof(rsp_ddc_params, w), offsetof(rsp_ddc_params, w0),
           offsetof(rsp_ddc_params, mode), offsetof(rsp_ddc_params, D), offsetof(rsp_ddc_params, off), offsetof(rsp_ddc_params, L),
           offsetof(rsp_ddc_params, h));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(rsp_ddc_info), offsetof(rsp_ddc_info, No), offsetof(rsp_ddc_info, TP),
           offsetof(rsp_ddc_info, in_rows), offsetof(rsp_ddc_info, workgroups), offsetof(rsp_ddc_info, lds_bytes),
           offsetof(rsp_ddc_info, k_per_thread), offsetof(rsp_ddc_info, in_bytes), offsetof(rsp_ddc_info, out_bytes));
    printf("%d %d %d %d %d %d %d %d %d\n", RSP_C64, RSP_C128, RSP_R32, RSP_R64, RSP_DDC_MAX_TAPS, RSP_DDC_MAX_D, RSP_DDC_NCO_IQ,
           RSP_DDC_NCO_SIN, RSP_ABI_VERSION);
    return 0;
}
'''


def test_abi_version_and_symbols():
    lib = _abi.lib()
    assert lib.rsp_abi_version() == 4
    for n, nargs in SYMBOLS.items():
        assert hasattr(lib, n), 'librsp.so does not export %s' % n
        assert len(_abi.PROTOTYPES[n][1]) == nargs
    assert (_abi.RSP_C64, _abi.RSP_C128, _abi.RSP_R32, _abi.RSP_R64) == (1, 2, 3, 4)


def test_declared_signatures_and_layout_against_the_header():
    libdir = os.path.dirname(_abi.lib()._name)
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, 'probe.c'), os.path.join(d, 'probe')
        open(src, 'w').write(PROBE)
        subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-I', INCLUDE, src, '-o', exe, '-L', libdir, '-lrsp',
                        '-Wl,-rpath,' + libdir], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split('\n')
    Pm, I = _abi.DdcParams, _abi.DdcInfo
    assert [int(x) for x in out[0].split()] == [ct.sizeof(Pm), Pm.w.offset, Pm.w0.offset, Pm.mode.offset, Pm.D.offset,
                                                Pm.off.offset, Pm.L.offset, Pm.h.offset]
    assert ct.sizeof(Pm) == 40 and Pm.h.offset == 32
    assert [int(x) for x in out[1].split()] == [ct.sizeof(I), I.No.offset, I.TP.offset, I.in_rows.offset, I.workgroups.offset,
                                                I.lds_bytes.offset, I.k_per_thread.offset, I.in_bytes.offset, I.out_bytes.offset]
    assert ct.sizeof(I) == 88 and I.in_bytes.offset == 72
    assert [int(x) for x in out[2].split()] == [_abi.RSP_C64, _abi.RSP_C128, _abi.RSP_R32, _abi.RSP_R64, _abi.RSP_DDC_MAX_TAPS,
                                                _abi.RSP_DDC_MAX_D, _abi.RSP_DDC_NCO_IQ, _abi.RSP_DDC_NCO_SIN, 4]


def _params(L=12, D=4, off=0, mode=0, h=True):
    taps = (ct.c_double * 512)()
    return _abi.DdcParams(w=1, w0=0, mode=mode, D=D, off=off, L=L, h=ct.cast(taps, ct.POINTER(ct.c_double)) if h else None), taps


def test_refusals_without_a_device_come_in_order():
    """Sizes, dtype, null pointers and mode: every one of them before the plan is looked at."""
    lib = _abi.lib()
    x = (ct.c_double * 64)()
    xp, xd = ct.cast(x, ct.c_void_p), ct.cast(x, ct.POINTER(ct.c_double))
    prm, keep = _params()
    assert lib.rsp_ddc(None, 0, 8, 1, None, 99, None, None) == _abi.RSP_ERR_INVALID            # sizes before dtype
    assert b'bad sizes P=0 N=8 C=1' in lib.rsp_last_error()
    bad, keep2 = _params(L=513)
    assert lib.rsp_ddc(None, 4, 8, 1, xp, 99, ct.byref(bad), xd) == _abi.RSP_ERR_INVALID        # the filter's sizes too
    assert b'L=513 taps' in lib.rsp_last_error()
    assert lib.rsp_ddc(None, 4, 8, 1, xp, _abi.RSP_C128, ct.byref(prm), xd) == _abi.RSP_ERR_INVALID   # a complex dtype
    assert b'unknown dtype 2' in lib.rsp_last_error()
    assert lib.rsp_ddc(None, 4, 8, 1, xp, _abi.RSP_R64, ct.byref(prm), xd) == _abi.RSP_ERR_INVALID    # null plan
    assert b'null argument' in lib.rsp_last_error()
    assert lib.rsp_ddc(None, 4, 8, 1, xp, _abi.RSP_R32, None, xd) == _abi.RSP_ERR_INVALID
    assert b'null argument' in lib.rsp_last_error()
    assert lib.rsp_ddc_device(None, 4, -1, 1, xp, ct.byref(prm), xp) == _abi.RSP_ERR_INVALID
    assert b'bad sizes P=4 N=-1 C=1' in lib.rsp_last_error()
    off, keep3 = _params(D=4, off=4)
    assert lib.rsp_ddc_device(None, 4, 8, 1, xp, ct.byref(off), xp) == _abi.RSP_ERR_INVALID
    assert b'off=4' in lib.rsp_last_error()
    assert lib.rsp_ddc_raw_detect(None, 4, 8, 0, xp, _abi.RSP_R64, ct.byref(prm), 2, 4, None, 1, None, None, None) == _abi.RSP_ERR_INVALID
    assert b'bad sizes P=4 N=8 C=0' in lib.rsp_last_error()
    assert lib.rsp_ddc_raw_detect(None, 4, 8, 1, xp, 0, ct.byref(prm), 2, 4, None, 1, None, None, None) == _abi.RSP_ERR_INVALID
    assert b'unknown dtype 0' in lib.rsp_last_error()
    assert lib.rsp_profile_ddc(None, 4, 8, 1, 0, 4, 0, 1, None, None) == _abi.RSP_ERR_INVALID
    assert b'L=0 taps' in lib.rsp_last_error()
    assert lib.rsp_profile_ddc(None, 4, 8, 1, 12, 4, 0, 1, None, None) == _abi.RSP_ERR_INVALID
    assert b'bad argument' in lib.rsp_last_error()
