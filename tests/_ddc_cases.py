"""The cases of the digital down-converter (k_ddc): what tests/test_ddc.py runs on the device against
tests/_ddc_ref.py.  test_ddc_cases.py proves on the CPU, from describe_ddc, that every case hits the tile edge
it is there for.

A case gives P, C, the taps' length L (12: FIR.mat's Num, else Gaussian taps), D, off, the NCO (mode, w, w0),
the input dtype ('match': the plan's own reals) and how many outputs a pulse has, as a function of the tile's
TK in the precision at hand ('TK-1', 'TK', 'TK+1', '2TK+1', or a number); N follows from it.  `expect` holds
what describe_ddc must say of the resolved shape.
"""
import os

import numpy as np

import rsp
from rsp import matio

HERE = os.path.dirname(os.path.abspath(__file__))
PRECS = ('c128', 'c64')
RDT = {'c128': np.float64, 'c64': np.float32}   # the plan's reals
TENTH = 1844674407370955162                     # rsp_ddc_phase_word(10e6, 100e6)
NO = {'TK-1': lambda tk: tk - 1, 'TK': lambda tk: tk, 'TK+1': lambda tk: tk + 1, '2TK+1': lambda tk: 2 * tk + 1}


def fir_mat():
    return np.asarray(matio.load(os.path.join(HERE, 'golden', 'ref_mat', 'FIR.mat'))['Num'], np.float64).ravel()


def _c(P, no, C=1, L=12, D=4, off=0, mode='iq', w=TENTH, w0=0, dtype='match', N=None, **expect):
    return dict(P=P, no=no, C=C, L=L, D=D, off=off, mode=mode, w=w, w0=w0, dtype=dtype, N=N, expect=expect)


CASES = {
    # pulses: TP = 1, 2, 4 and 64; one, two and three pulse tiles; with them the four tile edges along k
    'p1': _c(1, 'TK+1', TP=1, p_tiles=1, k_tiles=2),
    'p2': _c(2, 'TK-1', TP=2, p_tiles=1, k_tiles=1),
    'p3': _c(3, 'TK', TP=4, p_tiles=1, k_tiles=1),
    'p63': _c(63, 'TK+1', TP=64, p_tiles=1, k_tiles=2),
    'p64': _c(64, '2TK+1', TP=64, p_tiles=1, k_tiles=3),
    'p65': _c(65, 'TK-1', TP=64, p_tiles=2, k_tiles=1),
    'p130': _c(130, 'TK', TP=64, p_tiles=3, k_tiles=1),
    # one output, one sample, fewer samples than taps, no output at all
    'no1': _c(3, 1, No=1, k_tiles=1),
    'n1': _c(5, None, N=1, No=1),
    'n-lt-l': _c(2, None, N=7, No=2),
    'n-le-off': _c(2, None, N=3, off=3, No=0, k_tiles=0, workgroups=0),
    # decimation, at phase 0 and D - 1
    'd1': _c(5, 'TK+1', D=1, k_tiles=2),
    'd2': _c(5, 'TK+1', D=2, k_tiles=2),
    'd2-o1': _c(64, 'TK+1', D=2, off=1, k_tiles=2),
    'd4-o3': _c(64, 'TK+1', D=4, off=3, k_tiles=2),
    'd7': _c(5, 'TK+1', D=7, k_tiles=2),
    'd7-o6': _c(64, 'TK+1', D=7, off=6, k_tiles=2),
    'd64': _c(5, 'TK+1', D=64, k_tiles=2),
    'd64-o63': _c(64, 'TK+1', D=64, off=63, k_tiles=2),
    'd64-p1': _c(1, 'TK+1', D=64, off=17, k_tiles=2, threads=64),   # fewer k lanes than a wave has lanes
    # taps: one, two, 13, 64 and 512; 512 in one staging pass (P = 1) and in several (P = 64)
    'l1': _c(3, 'TK+1', L=1, D=1, k_tiles=2),
    'l2': _c(3, 'TK+1', L=2, k_tiles=2),
    'l13': _c(64, 'TK+1', L=13, k_tiles=2),
    # (lines longer than the filter, so that every tap of every pass meets samples)
    'l64': _c(64, 30, L=64),
    'l100': _c(64, 40, L=100),   # two staging passes in complex double, one in complex single
    'l512-p1': _c(1, 'TK+1', L=512, tap_chunk=512, k_tiles=2),
    'l512-p64': _c(64, 200, L=512),
    # channels
    'c3': _c(3, 'TK+1', C=3, k_tiles=2),
    'c16': _c(65, 'TK+1', C=16, p_tiles=2, k_tiles=2),
    # the real mixer
    'sin-p1': _c(1, 'TK+1', mode='sin', k_tiles=2),
    'sin-p65': _c(65, 'TK+1', mode='sin', p_tiles=2, k_tiles=2),
    # NCO words: none, fs/4, fs/2, a start phase, and words whose n w wraps every other sample
    'w0': _c(3, 'TK+1', w=0),
    'w-quarter': _c(64, 'TK+1', w=2 ** 62),
    'w-half': _c(3, 'TK+1', w=2 ** 63),
    'w-tenth-w0': _c(64, 'TK+1', w0=0x123456789ABCDEF0),
    'w-wrap': _c(64, 'TK+1', w=2 ** 64 - 2 ** 62 - 12345, w0=2 ** 63 + 77),
    'w-wrap-p1': _c(1, 'TK+1', w=2 ** 63 + 2 ** 40 + 1),
    # an input of the other precision
    'r32-in': _c(65, 'TK+1', dtype='r32', C=2),
    'r64-in': _c(65, 'TK+1', dtype='r64', C=2),
}
# the cases whose tap loop takes more than one staging pass in that precision
CHUNKED = {'c128': ('l100', 'l512-p64'), 'c64': ('l512-p64',)}


def resolve(name, prec):
    """The case's shape in `prec`: dict(P, N, C, L, D, off, mode, w, w0, dtype) and describe_ddc of it."""
    c = CASES[name]
    N = c['N']
    if N is None:
        no = c['no']
        if not isinstance(no, int):
            no = NO[no](rsp.describe_ddc(c['P'], 1 << 16, c['C'], c['L'], c['D'], c['off'], prec)['TK'])   # TK of a long line
        N = (no - 1) * c['D'] + c['off'] + 1 + min(c['D'] - 1, 2)   # the least N of `no` outputs, and up to two more
    shape = {k: c[k] for k in ('P', 'C', 'L', 'D', 'off', 'mode', 'w', 'w0')}
    shape['N'] = N
    shape['dtype'] = RDT[prec] if c['dtype'] == 'match' else {'r32': np.float32, 'r64': np.float64}[c['dtype']]
    return shape, rsp.describe_ddc(c['P'], N, c['C'], c['L'], c['D'], c['off'], prec)


def check_preconditions(name, prec):
    """Every entry of the case's `expect`, and the relation of No to TK it is named for."""
    c = CASES[name]
    shape, d = resolve(name, prec)
    for k, v in c['expect'].items():
        assert d[k] == v, (name, prec, k, d[k], v, d)
    if isinstance(c['no'], str):
        assert d['No'] == NO[c['no']](d['TK']), (name, prec, d)
    elif isinstance(c['no'], int):
        assert d['No'] == c['no'], (name, prec, d)
    assert d['No'] == max(0, -(-(shape['N'] - shape['off']) // shape['D']))
    assert d['TP'] == min(64, 1 << max(shape['P'] - 1, 0).bit_length())
    assert d['in_rows'] == (d['TK'] - 1) * shape['D'] + d['tap_chunk'] and 1 <= d['tap_chunk'] <= shape['L']
    assert d['k_tiles'] == -(-d['No'] // d['TK']) and d['p_tiles'] == -(-shape['P'] // d['TP'])
    assert d['workgroups'] == d['k_tiles'] * d['p_tiles'] * shape['C']
    assert d['lds_bytes'] <= 40 * 1024
    assert (d['tap_chunk'] < shape['L']) == (name in CHUNKED[prec]), (name, prec, d)
    return shape, d


def inputs(name, prec, seed=None):
    """(x [P, N, C] Gaussian of the case's dtype, Fortran order; h): reproducible."""
    shape, _ = resolve(name, prec)
    rng = np.random.default_rng(sorted(CASES).index(name) + 1000 if seed is None else seed)
    x = np.asfortranarray(rng.standard_normal((shape['P'], shape['N'], shape['C'])).astype(shape['dtype']))
    h = fir_mat() if shape['L'] == 12 else rng.standard_normal(shape['L']) / np.sqrt(shape['L'])
    return shape, x, h
