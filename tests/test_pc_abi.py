"""CPU tests of the stand-alone pulse compression's C ABI: the exported symbols and the ctypes mirrors against
the header (rsp_pc_info's layout included), and the refusals that need no device, in their documented order."""
import ctypes as ct
import os
import subprocess
import tempfile

from rsp import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INCLUDE = os.path.join(ROOT, 'include')
SYMBOLS = {'rsp_query_pc': 4, 'rsp_plan_describe_pc': 9, 'rsp_pc': 6, 'rsp_pc_device': 5, 'rsp_pc_mtd_detect': 9,
           'rsp_raw_detect': 12, 'rsp_profile_pc': 6}

PROBE = r'''
#include <stdio.h>
#include <stddef.h>
#include "rsp.h"
int32_t (*f_query)(const rsp_plan*, int32_t, int32_t, rsp_pc_info*) = rsp_query_pc;
int32_t (*f_describe)(const rsp_sig_config*, const rsp_cfar_params*, const rsp_cluster_params*, const rsp_precomputed*,
                      const rsp_plan_options*, int32_t, int32_t, int32_t, rsp_pc_info*) = rsp_plan_describe_pc;
int32_t (*f_pc)(rsp_plan*, int32_t, int32_t, const void*, int32_t, double*) = rsp_pc;
int32_t (*f_dev)(rsp_plan*, int32_t, int32_t, const void*, void*) = rsp_pc_device;
int32_t (*f_chain)(rsp_plan*, int32_t, int32_t, int32_t, const void*, int32_t, const double*, const rsp_detect_params*,
                   rsp_frame_out*) = rsp_pc_mtd_detect;
int32_t (*f_raw)(rsp_plan*, int32_t, int32_t, int32_t, int32_t, const void*, int32_t, const double*, int32_t, const double*,
                 const rsp_detect_params*, rsp_frame_out*) = rsp_raw_detect;
int32_t (*f_prof)(rsp_plan*, int32_t, int32_t, int32_t, float*, int64_t*) = rsp_profile_pc;
int main(void) {
    if (f_query(0, 4, 1, 0) != RSP_ERR_INVALID) return 2;
    if (f_pc(0, 4, 1, 0, RSP_C128, 0) != RSP_ERR_INVALID) return 3;
    if (f_dev(0, 4, 1, 0, 0) != RSP_ERR_INVALID) return 4;
    if (f_chain(0, 4, 2, 4, 0, RSP_C128, 0, 0, 0) != RSP_ERR_INVALID) return 5;
    if (f_raw(0, 4, 8, 2, 4, 0, RSP_C128, 0, 1, 0, 0, 0) != RSP_ERR_INVALID) return 6;
    if (f_prof(0, 4, 1, 1, 0, 0) != RSP_ERR_INVALID) return 7;
    if (f_describe(0, 0, 0, 0, 0, 256, 4, 1, 0) != RSP_ERR_INVALID) return 8;
    printf("%zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(rsp_pc_info), offsetof(rsp_pc_info, nU), offsetof(rsp_pc_info, z_elems),
           offsetof(rsp_pc_info, pack_rows), offsetof(rsp_pc_info, unpack_lds_bytes), offsetof(rsp_pc_info, ivl_lo),
           offsetof(rsp_pc_info, ivl_start), RSP_ABI_VERSION);
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
    I = _abi.PcInfo
    assert [int(x) for x in out[0].split()] == [ct.sizeof(I), I.nU.offset, I.z_elems.offset, I.pack_rows.offset,
                                                I.unpack_lds_bytes.offset, I.ivl_lo.offset, I.ivl_start.offset, 4]
    assert ct.sizeof(I) == 112 and I.z_elems.offset == 32


def test_refusals_without_a_device_come_in_order():
    """Sizes, dtype, null pointers: with no plan at all only P, B < 1 can be judged of the sizes."""
    lib = _abi.lib()
    x = (ct.c_double * 64)()
    xp, xd = ct.cast(x, ct.c_void_p), ct.cast(x, ct.POINTER(ct.c_double))
    assert lib.rsp_pc(None, 0, 1, None, 99, None) == _abi.RSP_ERR_INVALID          # sizes before dtype
    assert b'bad sizes P=0 B=1' in lib.rsp_last_error()
    assert lib.rsp_pc(None, 4, 0, xp, _abi.RSP_C128, xd) == _abi.RSP_ERR_INVALID
    assert b'bad sizes P=4 B=0' in lib.rsp_last_error()
    assert lib.rsp_pc(None, 4, 1, xp, _abi.RSP_C128, xd) == _abi.RSP_ERR_INVALID   # null plan
    assert b'null argument' in lib.rsp_last_error()
    assert lib.rsp_pc_device(None, -1, 1, xp, xp) == _abi.RSP_ERR_INVALID
    assert b'bad sizes P=-1 B=1' in lib.rsp_last_error()
    assert lib.rsp_pc_mtd_detect(None, 4, 0, 4, xp, _abi.RSP_C128, None, None, None) == _abi.RSP_ERR_INVALID
    assert b'bad sizes P=4 B=0' in lib.rsp_last_error()
    assert lib.rsp_raw_detect(None, 0, 8, 2, 4, xp, _abi.RSP_C128, None, 1, None, None, None) == _abi.RSP_ERR_INVALID
    assert b'bad sizes P=0 B=2' in lib.rsp_last_error()
    assert lib.rsp_profile_pc(None, 4, 1, 1, None, None) == _abi.RSP_ERR_INVALID
    assert lib.rsp_query_pc(None, 4, 1, None) == _abi.RSP_ERR_INVALID
