"""CPU test of the CFAR call family's first refusal: every entry of the three detectors (map call, stage 2 on
beams, on gated beams, on a raw cube, profile), rsp_stage3_cfar and rsp_last_cfar_threshold refuse a null plan
with RSP_ERR_INVALID before they read anything else, with a parameter block and without one.  The map, stage-2
and threshold entries say "null argument"; the profile entries check the plan together with iters and say "bad
argument"."""
import ctypes as ct

from rsp import _abi

S3, VC, XC = _abi.Stage3CfarParams, _abi.VcfarParams, _abi.CfarParams
# entry -> (its parameter struct, or None; the word of its refusal)
ENTRIES = {
    'rsp_stage3_cfar_shape': (S3, 'null'), 'rsp_stage3_cfar': (S3, 'null'),
    'rsp_process_stage2_cfar': (S3, 'null'), 'rsp_process_stage2_gated_cfar': (S3, 'null'),
    'rsp_process_raw_stage2_cfar': (S3, 'null'), 'rsp_profile_stage3': (S3, 'bad argument'),
    'rsp_vcfar': (VC, 'null'), 'rsp_process_stage2_vcfar': (VC, 'null'), 'rsp_process_stage2_gated_vcfar': (VC, 'null'),
    'rsp_process_raw_stage2_vcfar': (VC, 'null'), 'rsp_profile_vcfar': (VC, 'bad argument'),
    'rsp_xcfar': (XC, 'null'), 'rsp_process_stage2_xcfar': (XC, 'null'), 'rsp_process_stage2_gated_xcfar': (XC, 'null'),
    'rsp_process_raw_stage2_xcfar': (XC, 'null'), 'rsp_profile_xcfar': (XC, 'bad argument'),
    'rsp_last_cfar_threshold': (None, 'null'),
}


def _args(name, prm):
    """The entry's arguments with a null plan: ``prm`` (or null) for its parameter block, null for every
    other pointer, 1 for every integer (a valid iters, n_maps, dtype-free count) and 0 for hits_cap."""
    args = []
    for t in _abi.PROTOTYPES[name][1][1:]:
        if prm is not None and t is ct.POINTER(type(prm)):
            args.append(ct.byref(prm))
        elif t is ct.c_int64:
            args.append(0)
        elif t is ct.c_int32:
            args.append(1)
        else:
            args.append(None)
    return [None] + args


def test_null_plan_is_refused_first():
    lib = _abi.lib()
    names = [n for n in _abi.PROTOTYPES if ('cfar' in n or n == 'rsp_profile_stage3') and not n.endswith('_describe')]
    assert sorted(names) == sorted(ENTRIES) and len(ENTRIES) == 17     # the table is the whole family
    ok = XC(5, 10, 5, 10, 8.0)
    for name, (cls, word) in sorted(ENTRIES.items()):
        for prm in ([cls(), None] if cls else [None]):
            # another refusal's message first, so that the one read below is this call's
            assert lib.rsp_xcfar_describe(0, 0, ct.byref(ok), None) == _abi.RSP_ERR_INVALID
            assert b'bad map shape' in lib.rsp_last_error()
            assert getattr(lib, name)(*_args(name, prm)) == _abi.RSP_ERR_INVALID, name
            assert word.encode() in lib.rsp_last_error(), (name, lib.rsp_last_error())
