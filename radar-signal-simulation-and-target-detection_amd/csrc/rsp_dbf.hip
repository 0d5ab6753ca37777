// rsp_dbf.hip -- the stand-alone DBF of the stage-2 scripts for CDNA4 (gfx950), and its launcher.
//
//   k_dbf : C channel planes x[c][i] (MATLAB [P x N x C], position i = p + P n fastest) -> B beam
//           planes y[b][i] = sum_c A[b][c] x[c][i] (MATLAB [P x N x B], iq_data_13beam), A = conj(W)
//           (debug_simulated_data_processing.m:166-175, `* DBF_coeffs_data_C'`) or A = W
//           (main_test_with_simulated_data.m:207-214, `* DBF_coeffs_data_C.'`).
//
// The arithmetic is K1's (Dbf<T>, rsp_dbf.h): channel groups in ascending order, the Re operand
// before the Im operand, so an output element is the same sequence of fused operations as in
// k1_dbf_mtd.  The kernel moves data -- 16 (C + B) bytes per position in complex double -- so what
// counts is the access pattern: a lane's 16-B load is its MFMA B operand and the 16 lanes of a
// quarter-wave read 256 consecutive bytes of one channel plane; every store is 16 B per lane, 256
// consecutive bytes of one beam plane per quarter-wave.  DESIGN.md section 3f.
#include "rsp_dbf.h"

namespace {

// Cache policy of the beam stores: the default.  Non-temporal stores (2) were slower at the reference
// frame (complex double 0.087 .. 0.098 ms against 0.078; profiles/dbf_variants_ab.txt)
#define RSP_DBF_AUX 0

// A workgroup of RSP_DBF_THREADS / 64 waves takes RSP_DBF_ROUNDS rounds of consecutive sub-tiles;
// in a round wave w takes sub-tiles (round * waves + w) * TPW .. + TPW - 1, all of their loads in
// flight together (TPW = K1Cfg::TPW: 16 16-B registers per lane).  The A operands are read once
// per wave and serve all its rounds.  Two rounds: with 4 or 8 a frame of x2's size in complex single
// is too few workgroups to cover the load latency (0.023 / 0.036 ms against 0.019), with 1 the A
// operands' reads cost more than they save in complex double (profiles/dbf_variants_ab.txt).
//
// Row layout of the A table (rsp_dbf_atab): double DBF_ROWS_SPLIT, K1's -- registers i and i + 2 of
// a lane are Re and Im of beam (grp + 4 i) & 7; float DBF_ROWS_PAIR -- the four consecutive rows
// 4 grp + i of a lane are (Re, Im) of beams 2 grp and 2 grp + 1, so that with the two column blocks
// (positions q, q + 1) a lane stores (Re, Im, Re, Im) of one beam: 16 B.  K1's assignment would
// leave a float lane with four Re (or four Im) parts of four beams: 4-B stores.
//
// Tail positions, padded channels and padded beams take no branch: a lane past S loads and stores
// at RSP_OOB (the buffer resource returns 0 / drops the store), a padded channel reads plane C - 1
// against zero weights, a padded beam's store goes to RSP_OOB.  Float: the load of the last
// position of an odd S also reads position S, and the store writes it; both lie inside the planes'
// pitch (even, dbf_pitch) and never in another plane's positions < S.
template <class T, int CP, int MB>
__global__ __launch_bounds__(RSP_DBF_THREADS) void k_dbf(DbfDesc d, const void* __restrict__ x,
                                                         const T* __restrict__ At, void* __restrict__ y) {
    typedef cx<T> V;
    typedef Dbf<T> D;
    constexpr int NJ = CP / 4, TPW = k1_cfg(CP, 8 * MB).TPW, WAVES = RSP_DBF_THREADS / 64;
    constexpr int PT = 16 * D::PPL;   // positions per sub-tile
    static_assert(k1_cfg(CP, 8 * MB).NJ == NJ && k1_cfg(CP, 8 * MB).MB == MB, "CP / MB are k1_cfg's own values");
    const int lane = threadIdx.x & 63, grp = lane >> 4, col = lane & 15;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    T are[MB][NJ], aim[MB][NJ];   // this lane's A operand: row lane&15, channel 4j + lane>>4
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            are[mb][j] = At[((mb * NJ + j) * 2 + 0) * 64 + lane];
            aim[mb][j] = At[((mb * NJ + j) * 2 + 1) * 64 + lane];
        }
    const __amdgpu_buffer_rsrc_t xr = buf_rsrc(x, d.in_bytes), yr = buf_rsrc(y, d.out_bytes);
    unsigned coff[NJ];   // byte offset of this lane's channel plane of group j
#pragma unroll
    for (int j = 0; j < NJ; ++j) coff[j] = (unsigned)min(4 * j + grp, d.C - 1) * (unsigned)d.pitch * (unsigned)sizeof(V);
    const int t0 = blockIdx.x * (WAVES * RSP_DBF_ROUNDS * TPW);
#pragma unroll 1
    for (int r = 0; r < RSP_DBF_ROUNDS; ++r) {
        const int tb = t0 + (r * WAVES + wv) * TPW;   // wave-uniform
        if (tb * PT >= d.S) break;
        typename D::Ld xv[TPW][NJ];
#pragma unroll
        for (int u = 0; u < TPW; ++u) {   // every load of TPW sub-tiles in flight together
            const int q = (tb + u) * PT + D::PPL * col;
            const unsigned po = q < d.S ? (unsigned)q * (unsigned)sizeof(V) : RSP_OOB;
#pragma unroll
            for (int j = 0; j < NJ; ++j)   // non-temporal: the cube is read exactly once
                xv[u][j] = D::bits(__builtin_amdgcn_raw_buffer_load_b128(xr, (int)(po + coff[j]), 0, 2));
        }
#pragma unroll
        for (int u = 0; u < TPW; ++u) {
            typename D::Acc acc[MB][D::NACC];
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
#pragma unroll
                for (int a = 0; a < D::NACC; ++a) acc[mb][a] = typename D::Acc{};
#pragma unroll
                for (int j = 0; j < NJ; ++j) D::mma(acc[mb], are[mb][j], aim[mb][j], xv[u][j]);
            }
            const int q = (tb + u) * PT + D::PPL * col;
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    if constexpr (sizeof(T) == 8) {
                        const int b = mb * 8 + grp + 4 * h;   // rows grp + 4 h (Re) and grp + 4 h + 8 (Im)
                        const unsigned off = (b < d.B && q < d.S) ? ((unsigned)b * (unsigned)d.opitch + (unsigned)q) * 16u : RSP_OOB;
                        buf_st<RSP_DBF_AUX>(yr, off, d2{acc[mb][0][h], acc[mb][0][h + 2]});
                    } else {
                        const int b = mb * 8 + 2 * grp + h;   // rows 4 grp + 2 h (Re) and 4 grp + 2 h + 1 (Im)
                        const unsigned off = (b < d.B && q < d.S) ? ((unsigned)b * (unsigned)d.opitch + (unsigned)q) * 8u : RSP_OOB;
                        const f32x4 o{acc[mb][0][2 * h], acc[mb][0][2 * h + 1], acc[mb][1][2 * h], acc[mb][1][2 * h + 1]};
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), yr, (int)off, 0, RSP_DBF_AUX);
                    }
                }
        }
    }
}

template <class T, int CP>
hipError_t launch_dbf_c(const DbfDesc& d, int mb, int grid, const void* x, const void* At, void* y, hipStream_t s) {
    if (mb == 1) return launch(k_dbf<T, CP, 1>, dim3(grid), dim3(RSP_DBF_THREADS), 0, s, d, x, static_cast<const T*>(At), y);
    return launch(k_dbf<T, CP, 2>, dim3(grid), dim3(RSP_DBF_THREADS), 0, s, d, x, static_cast<const T*>(At), y);
}

template <class T>
hipError_t launch_dbf_t(const DbfDesc& d, const void* x, const void* At, void* y, hipStream_t s) {
    const K1Cfg kc = k1_cfg(d.C, d.B);
    const int grid = dbf_workgroups(d.S, d.C, d.B, sizeof(T) == 8 ? RSP_PREC_F64 : RSP_PREC_F32);
    switch (kc.CP) {
        case 8: return launch_dbf_c<T, 8>(d, kc.MB, grid, x, At, y, s);
        case 16: return launch_dbf_c<T, 16>(d, kc.MB, grid, x, At, y, s);
        default: return launch_dbf_c<T, 32>(d, kc.MB, grid, x, At, y, s);
    }
}

}  // namespace

hipError_t launch_dbf(const DbfDesc& d, int prec, const void* x, const void* At, void* y, hipStream_t s) {
    return prec == RSP_PREC_F64 ? launch_dbf_t<double>(d, x, At, y, s) : launch_dbf_t<float>(d, x, At, y, s);
}
