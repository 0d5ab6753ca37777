"""The cases of the stand-alone pulse compression (k_pc_pack, k2_pc on a record table of its own,
k_pc_unpack): what tests/test_pc.py runs on the device, the derivation of rsp_pc_derive restated, and the
per-segment, per-block metric of test_k2_parity.py restated.  test_pc_cases.py proves on the CPU, from
describe_pc, that the table reaches the paths it is there for.

A case is (scenario name, P, B).  The scenario gives the waveform, the gate layout and the filters only: the
plan's own prtNum and beam_num play no part in the stage.
"""
import numpy as np

from rsp import config as C
from rsp.precompute import precompute as product_precompute
from oracle import precompute as oracle_precompute

from _scen import scenario, plumbing_weights, _route_cfar, k2_blocks

PRECS = ('c128', 'c64')
NZ = 8                                    # RSP_PC_NZ
PACK_COLS, UNPACK_ROWS = 256, 64          # RSP_PCK_COLS, RSP_PCU_ROWS: the tiles' extents along the pulse axis
UNPACK_GROUP = 8                          # RSP_PCU_GROUP: pulse tiles one unpack workgroup walks
UNPACK_COLS = {'c128': 32, 'c64': 64}     # pcu_cols: 512 bytes of gates
LDS = {'pack': {'c128': 8 * 260 * 16, 'c64': 8 * 260 * 8}, 'unpack': {'c128': 64 * 33 * 16, 'c64': 64 * 65 * 8}}

# to the bit against Plan.process_stage2 at the case's own P = 16, B = 3
BIT_CASES = ('no-medium', 'mb-pow2', 'w4-mb128', 'fir-wrap', 'lh-heavy', 'm64-mb')
# against the oracle at pulse counts no plan takes: a 1024-sample case with three sample intervals, the second
# starting at compacted index 47, and nU = 700 = 4 mod 8
ORACLE_CASE = 'm64-mb'
# 333 in complex double only; 511 .. 513: one below, on and one above the 512 pulses one unpack workgroup walks
ORACLE_P = (1, 2, 7, 63, 64, 65, 255, 256, 257, 333, 511, 512, 513)
ORACLE_B = (1, 3, 13)                                 # at P = 7
# G one below and one above a multiple of either unpack tile width (`no-medium`, G = 320, is on one): the
# plumbing waveform with 255 and 257 long gates
OWN_CASES = {
    'pc-g511': dict(point_PRT=1024, tao=(0.16e-6, 2e-6, 6e-6), gap_duration=(2.84e-6, 8e-6, 12e-6),
                    point_prt_segments=(64, 192, 255)),
    'pc-g513': dict(point_PRT=1024, tao=(0.16e-6, 2e-6, 6e-6), gap_duration=(2.84e-6, 8e-6, 12e-6),
                    point_prt_segments=(64, 192, 257)),
}
G_EDGE_CASES = ('pc-g511', 'no-medium', 'pc-g513')


def gpu_cases():
    """Every (scenario, P, B, precisions) the GPU tests launch."""
    out = [(n, 16, 3, PRECS) for n in BIT_CASES]
    out += [(ORACLE_CASE, P, 3, ('c128',) if P == 333 else PRECS) for P in ORACLE_P]
    out += [(ORACLE_CASE, 7, B, PRECS) for B in ORACLE_B]
    out += [(ORACLE_CASE, P, B, PRECS) for P, B in ((130, 3), (65, 3), (16, 1), (7, 1), (21, 3))]
    out += [(n, 21, 3, PRECS) for n in G_EDGE_CASES]
    return sorted(set(out))


def pc_scenario(name, P=16, B=3):
    """_scen.scenario for the names it knows, and this module's own cases built the same way."""
    if name not in OWN_CASES:
        return scenario(name)
    cfg = C.make_config(prtNum=P, channel_num=8, beam_num=B, **OWN_CASES[name])
    W, ang, k = plumbing_weights(cfg)
    return dict(name=name, cfg=cfg, cfar=_route_cfar(P, 'small'), clus=C.default_cluster_params(),
                pre_o=oracle_precompute.precompute(cfg, W, ang, k, C.V8_FIR),
                pre_p=product_precompute(cfg, W, ang, k, C.V8_FIR))


def with_prt_num(cfg, P):
    return dict(cfg, Sig_Config=dict(cfg['Sig_Config'], prtNum=P))


def intervals(L):
    """The used fast-time samples of a K2 layout (describe_k2) as merged intervals [lo, hi], 0-based: the
    union of the segments' sample windows, windows that touch merged (derive_segments)."""
    need = sorted((sg['lo'], sg['hi']) for sg in L['segments'] if sg is not None and sg['hi'] >= sg['lo'])
    U = []
    for lo, hi in need:
        if U and lo <= U[-1][1] + 1:
            U[-1][1] = max(U[-1][1], hi)
        else:
            U.append([lo, hi])
    return U


def expected_info(L, sizes, P, B, prec):
    """rsp_pc_info of P pulses x B beams restated from a plan's K2 layout and sizes (N, G)."""
    U = intervals(L)
    starts = [0]
    for lo, hi in U:
        starts.append(starts[-1] + hi - lo + 1)
    nU = starts.pop()
    nzc = -(-nU // NZ)
    rows = B * P
    k2_wg = sum((sg['nblocks'] if sg['type'] == 1 else 1) * -(-rows // sg['rows_per_wg'])
                for sg in L['segments'] if sg is not None)
    cols = UNPACK_COLS[prec]
    return dict(P=P, B=B, N=sizes.N, G=sizes.G, nU=nU, n_intervals=len(U), NZ=NZ, nzc=nzc, z_elems=B * nzc * P * NZ,
                pack_rows=NZ, pack_cols=PACK_COLS, unpack_rows=UNPACK_ROWS, unpack_cols=cols,
                pack_wg=nzc * -(-P // PACK_COLS) * B, k2_wg=k2_wg, unpack_wg=-(-sizes.G // cols) * -(-P // (UNPACK_ROWS * UNPACK_GROUP)) * B,
                k2_wg_per_cu=L['wg_per_cu'], pack_lds_bytes=LDS['pack'][prec], unpack_lds_bytes=LDS['unpack'][prec],
                ivl_lo=[lo for lo, _ in U], ivl_start=starts)


def beams(s, P, B, prec, seed=7):
    """A beam cube [P, N, B] of unit-variance complex noise with a few strong samples, reproducible; rounded
    to complex single for a c64 plan (what the upload would do), returned as complex128."""
    N = s['cfg']['Sig_Config']['point_PRT']
    rng = np.random.default_rng(seed)
    iq = (rng.standard_normal((P, N, B)) + 1j * rng.standard_normal((P, N, B))) / np.sqrt(2)
    for i, n in enumerate(range(37, N, 97)):
        iq[i % P, n, i % B] += 20.0
    iq = np.asfortranarray(iq)
    return iq.astype(np.complex64).astype(np.complex128) if prec == 'c64' else iq


# the compositions' detector: the reference's range window; a Doppler guard that clears the main lobe of a
# 21-pulse Kaiser window zero-padded to 32 rows
CHAIN_CFAR = dict(refCells_R=5, guardCells_R=10, refCells_V=2, guardCells_V=4, T_CFAR=8.0, method='GOCA')


def echo_cube(s, P, prec, seed=20250101):
    """(raw cube [P, N, C], W [B, C]) of the scenario's waveform at P pulses: three echoes near zero Doppler, in
    the middle of the narrow, medium and long gates, plus Philox noise; rounded to complex single for c64."""
    from oracle import chain
    cfg = with_prt_num(s['cfg'], P)
    W, ang, k = plumbing_weights(cfg)
    pre = oracle_precompute.precompute(cfg, W, ang, k, C.V8_FIR)
    sc = cfg['Sig_Config']
    vmax = sc['wavelength'] / (2 * sc['prt'])
    g1, g2, G = pre['N_gate_narrow'], pre['N_gate_medium'], pre['N_total_gate']
    tg = [dict(Range=float(pre['range_axis'][g]), Velocity=0.03 * vmax, ElevationAngle=float(ang[i % len(ang)]) + 0.5, SNR_dB=15.0)
          for i, g in enumerate((g1 // 2, g1 + g2 // 2, (g1 + g2 + G) // 2))]
    raw = chain.synthesize_echo(tg, cfg, pre) + chain.philox_noise(cfg, 1, seed)
    return (raw if prec == 'c128' else raw.astype(np.complex64)), np.asarray(W, np.complex128)


def blocks_close(got, ref, L, tol, what):
    """test_k2_parity.py's metric on maps [P, G, B]: for every block [g0, gend) of the layout, max |delta| per
    gate is at most tol of the reference's maximum over that block's segment; the first and last gate of every
    block, the worst one, and the last gate of the map when G is no multiple of 4 are checked on their own."""
    G = ref.shape[1]
    bad, worst = [], 0.0
    for slot, blk, g0, gend in k2_blocks(L):
        sg = L['segments'][slot]
        scale = np.abs(ref[:, sg['ga']:sg['gb'], :]).max()
        err = np.abs(got[:, g0:gend, :] - ref[:, g0:gend, :]).max(axis=(0, 2))   # per gate
        worst = max(worst, err.max() / scale)
        print('%s segment %d block %d, gates [%d, %d): max err / segment max %.3g (tol %g)'
              % (what, slot, blk, g0, gend, err.max() / scale, tol))
        for g in sorted({g0, gend - 1, g0 + int(np.argmax(err))} | ({G - 1} if G % 4 and gend == G else set())):
            if not err[g - g0] <= tol * scale:
                bad.append('gate %d (segment %d block %d, gates [%d, %d)): err %.3g = %.3g of the segment maximum'
                           % (g, slot, blk, g0, gend, err[g - g0], err[g - g0] / scale))
    print('%s worst block: %.3g of its segment maximum (tol %g)' % (what, worst, tol))
    assert not bad, '%s: %s' % (what, '; '.join(bad))
