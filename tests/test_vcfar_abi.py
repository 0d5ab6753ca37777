"""CPU tests of the Doppler CA-CFAR's C-ABI: the symbols of include/rsp.h exist in librsp.so with the
declared signatures (a C program that assigns each to a pointer of the declared type compiles with
-Werror), and the ctypes mirrors of its structs have the C layout."""
import ctypes as ct
import os
import subprocess
import tempfile

from rsp import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, 'include')
SYMBOLS = ('rsp_vcfar_describe', 'rsp_vcfar', 'rsp_process_stage2_vcfar', 'rsp_process_stage2_gated_vcfar',
           'rsp_profile_vcfar')

PROBE = r'''
#include <stdio.h>
#include <stddef.h>
#include "rsp.h"
#define HIT_TAIL uint8_t*, double*, rsp_stage3_hit*, int64_t, int64_t*
int32_t (*f_describe)(int32_t, int32_t, const rsp_vcfar_params*, rsp_vcfar_info*) = rsp_vcfar_describe;
int32_t (*f_vcfar)(rsp_plan*, int32_t, int32_t, const double*, int32_t, const rsp_vcfar_params*, HIT_TAIL) = rsp_vcfar;
int32_t (*f_fused)(rsp_plan*, const void*, int32_t, const rsp_vcfar_params*, double*, double*, HIT_TAIL) =
    rsp_process_stage2_vcfar;
int32_t (*f_gated)(rsp_plan*, const void*, int32_t, int32_t, const int32_t*, const rsp_vcfar_params*, double*, double*,
                   HIT_TAIL) = rsp_process_stage2_gated_vcfar;
int32_t (*f_prof)(rsp_plan*, const rsp_vcfar_params*, int32_t, float*, int64_t*) = rsp_profile_vcfar;
int main(void) {
    rsp_vcfar_params p = {4, 6, 0, 0, 6.0};
    rsp_vcfar_info i;
    if (f_describe(332, 3404, &p, &i) != RSP_OK) return 2;
    if (f_vcfar(0, 1, 1, 0, 1, &p, 0, 0, 0, 0, 0) != RSP_ERR_INVALID) return 3;
    if (f_fused(0, 0, RSP_C128, &p, 0, 0, 0, 0, 0, 0, 0) != RSP_ERR_INVALID) return 4;
    if (f_gated(0, 0, RSP_C128, 0, 0, &p, 0, 0, 0, 0, 0, 0, 0) != RSP_ERR_INVALID) return 5;
    if (f_prof(0, &p, 1, 0, 0) != RSP_ERR_INVALID) return 6;
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(rsp_vcfar_params), offsetof(rsp_vcfar_params, method),
           offsetof(rsp_vcfar_params, T_CFAR), sizeof(rsp_vcfar_info), offsetof(rsp_vcfar_info, rows),
           offsetof(rsp_vcfar_info, col_tiles), sizeof(rsp_stage3_hit));
    printf("%d %d %d %d %d %d\n", i.P, i.G, i.halo, i.max_halo, i.row_tiles, i.col_tiles);
    return 0;
}
'''


def test_symbols_and_prototypes():
    lib = _abi.lib()
    for n in SYMBOLS:
        assert hasattr(lib, n), 'librsp.so does not export %s' % n
        assert n in _abi.PROTOTYPES
    assert len(_abi.PROTOTYPES['rsp_vcfar'][1]) == 11
    assert len(_abi.PROTOTYPES['rsp_process_stage2_vcfar'][1]) == 11
    assert len(_abi.PROTOTYPES['rsp_process_stage2_gated_vcfar'][1]) == 13
    assert len(_abi.PROTOTYPES['rsp_profile_vcfar'][1]) == 5 and len(_abi.PROTOTYPES['rsp_vcfar_describe'][1]) == 4


def test_struct_sizes():
    assert ct.sizeof(_abi.VcfarParams) == 24
    assert ct.sizeof(_abi.VcfarInfo) == 32


def test_declared_signatures_and_layout_against_the_header():
    libdir = os.path.dirname(_abi.lib()._name)
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, 'probe.c'), os.path.join(d, 'probe')
        open(src, 'w').write(PROBE)
        subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-I', INCLUDE, src, '-o', exe, '-L', libdir, '-lrsp',
                        '-Wl,-rpath,' + libdir], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split('\n')
    sizes = [int(x) for x in out[0].split()]
    assert sizes == [24, _abi.VcfarParams.method.offset, _abi.VcfarParams.T_CFAR.offset, ct.sizeof(_abi.VcfarInfo),
                     _abi.VcfarInfo.rows.offset, _abi.VcfarInfo.col_tiles.offset, ct.sizeof(_abi.Stage3Hit)]
    P, G, halo, max_halo, row_tiles, col_tiles = (int(x) for x in out[1].split())
    assert (P, G, halo) == (332, 3404, 7) and max_halo >= 32 and row_tiles >= 1 and col_tiles >= 1


def test_null_arguments_are_rejected():
    lib = _abi.lib()
    assert lib.rsp_vcfar_describe(16, 64, None, None) == _abi.RSP_ERR_INVALID
    assert b'null' in lib.rsp_last_error()
    p = _abi.VcfarParams(refCells_V=4, guardCells_V=6, method=0, T_CFAR=6.0)
    assert lib.rsp_vcfar_describe(16, 64, ct.byref(p), None) == _abi.RSP_OK      # info may be NULL
    assert lib.rsp_vcfar(None, 16, 64, None, 1, ct.byref(p), None, None, None, 0, None) == _abi.RSP_ERR_INVALID
    assert lib.rsp_profile_vcfar(None, ct.byref(p), 1, None, None) == _abi.RSP_ERR_INVALID
