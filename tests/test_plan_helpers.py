"""The argument helpers of rsp/plan.py, without the library (CPU): the complex input of the frame and
stage-2 calls, the gate columns of the gated calls, and the two-pass retrieval of the stage-3 hit list."""
import ctypes as ct

import numpy as np
import pytest

from rsp import _abi
from rsp.plan import HIT_DTYPE, _complex_arg, _gate_cols_arg, _with_hits


def _bytes_at(ptr, n):
    return ct.string_at(ptr, n)


def test_complex_arg_keeps_complex64_and_widens_the_rest():
    rng = np.random.default_rng(3)
    c64 = (rng.standard_normal((3, 4, 2)) + 1j * rng.standard_normal((3, 4, 2))).astype(np.complex64)   # C order
    a, p, dt = _complex_arg(c64)
    assert dt == _abi.RSP_C64 and a.dtype == np.complex64 and a.flags.f_contiguous and np.array_equal(a, c64)
    assert _bytes_at(p, a.nbytes) == c64.tobytes(order='F')
    f128 = np.asfortranarray(rng.standard_normal((3, 4, 2)) + 1j * rng.standard_normal((3, 4, 2)))
    a, p, dt = _complex_arg(f128)
    assert dt == _abi.RSP_C128 and a is f128 and p.value == f128.ctypes.data   # already as the library takes it: no copy
    ints = np.arange(24).reshape(3, 4, 2)
    a, p, dt = _complex_arg(ints)
    assert dt == _abi.RSP_C128 and a.dtype == np.complex128 and a.flags.f_contiguous and np.array_equal(a, ints)
    assert _bytes_at(p, a.nbytes) == ints.astype(np.complex128).tobytes(order='F')
    a, p, dt = _complex_arg([[1 + 2j, 3.0]])   # anything np.asarray takes
    assert dt == _abi.RSP_C128 and a.shape == (1, 2)


def test_gate_cols_arg_is_six_int32_in_segment_order():
    cols = _gate_cols_arg(((1, 300), (301, 700), (np.int64(701), 1024.0)))
    assert isinstance(cols, ct.c_int32 * 6) and list(cols) == [1, 300, 301, 700, 701, 1024]
    with pytest.raises((IndexError, TypeError)):
        _gate_cols_arg(((1, 2), (3, 4), (5, 6), (7, 8)))   # a fourth segment does not fit


class _FakeCall:
    """Stands for the C function: `total` hits, of which it writes min(cap, total) records."""

    def __init__(self, total):
        self.total, self.calls = total, []

    def __call__(self, cap, hp, maps):
        self.calls.append((cap, hp is not None, maps))
        if hp is not None:
            rec = np.ctypeslib.as_array(ct.cast(hp, ct.POINTER(ct.c_int32)), (max(cap, 1) * HIT_DTYPE.itemsize // 4,))
            for i in range(min(cap, self.total)):
                rec[i * HIT_DTYPE.itemsize // 4] = i + 1   # v_idx
        return self.total


def test_with_hits_fetches_the_whole_list_in_a_second_call_without_maps():
    assert HIT_DTYPE.itemsize == ct.sizeof(_abi.Stage3Hit)
    below = _FakeCall(5)
    total, hits = _with_hits(below, 8, None, True)
    assert below.calls == [(8, True, True)] and total == 5
    assert hits.dtype == HIT_DTYPE and list(hits['v_idx']) == [1, 2, 3, 4, 5]
    above = _FakeCall(11)
    total, hits = _with_hits(above, 8, None, True)
    # the second call: the list alone (every map pointer None), at the capacity the first reported
    assert above.calls == [(8, True, True), (11, True, False)] and total == 11
    assert list(hits['v_idx']) == list(range(1, 12))
    capped = _FakeCall(11)   # the caller's own capacity: one call, the first hits_cap records
    total, hits = _with_hits(capped, 8, 4, True)
    assert capped.calls == [(4, True, True)] and total == 11 and list(hits['v_idx']) == [1, 2, 3, 4]
    none = _FakeCall(11)     # no list wanted: capacity 0, a null list
    total, hits = _with_hits(none, 8, None, False)
    assert none.calls == [(0, False, True)] and total == 11 and len(hits) == 0
    zero = _FakeCall(11)     # a capacity of 0 asks for the count alone
    total, hits = _with_hits(zero, 8, 0, True)
    assert zero.calls == [(0, False, True)] and total == 11 and len(hits) == 0
