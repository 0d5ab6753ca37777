// rsp_pc.hip -- the way into and out of k2_pc for a pulse and beam count that are not the plan's (gfx950):
// two tiled transposes through LDS around the pulse-compression kernel of rsp_k2.hip, which is launched
// unchanged (launch_k2_set) on a Geometry that carries the caller's P and B (PcDesc, rsp_geometry.h).
// Neither kernel does arithmetic: every value k2_pc reads is a beam sample as it was uploaded, every value
// of the result is k2_pc's.
//
// k_pc_pack<T, N>: beams x [P x N x B] in MATLAB's layout (pulse index fastest, beam planes `pitch` elements
// apart) -> z, k2_pc's input: element (b, chunk c, pulse m, slot s) at ((b nzc + c) P + m) NZ + s holds
// sample used_sample(c NZ + s) of pulse m of beam b (zaddr, rsp_device.h), NZ = RSP_PC_NZ = 8.  The corner
// turn K1 mode 0 does for the plan's own P.  A workgroup takes one chunk of RSP_PCK_COLS = 256 pulses of
// one beam: 8 source rows of up to 256 consecutive pulses in (each slot looks up its own sample, so a chunk
// that straddles two sample intervals takes its rows from two places), one run of 256 x 8 consecutive z
// elements out.  Both sides are 16 bytes per lane over consecutive addresses: a complex double, or two
// complex singles -- on the z side always (a slab starts on 64 bytes), on the beam side where the columns
// start on 16 bytes (N = 2: P and the plane pitch even, an aligned base; else N = 1, one element per lane,
// k_mtd_any's rule).  The load units of a tile are counted over its actual pulses, so the last tile of a
// row (P = 332: 76 pulses) issues 3 rounds of loads instead of 8 mostly idle ones.  Slots past nU in the
// last chunk are written as zeros.
//   LDS tile [8][256 + 4] elements, one row per sample.  Writes run along a row: consecutive 16-byte units,
// conflict-free.  Reads take lanes (m, s) = (l / 8, l % 8) in complex double and (l / 4, 2 (l % 4)) then
// s + 1 in complex single: element address s 260 + m.  260 = 4 mod 16 puts the 16 lanes of a ds_read_b128
// group -- (s, m) = (0..3, 0), (4..7, 1), (4..7, 2), (0..3, 3) and its mirror -- on the 16 distinct 16-byte
// slots 4 s + m mod 16; 260 = 4 mod 32 puts the 32 lanes of a ds_read_b64 half on the 32 distinct 8-byte
// slots 4 s + m.
//
// k_pc_unpack<T, N>: k2_pc's result r [B][P][G] (range fastest) -> pc [P x G x B] (pulse fastest).  A
// workgroup takes RSP_PCU_ROWS = 64 pulses of 512 bytes of gates (64 complex singles, 32 complex doubles) of
// one beam.  Loads run along g, a lane per gate; stores run along m, 16 bytes per lane (N = 2 complex
// singles where P is even and the base aligned, else one).  LDS tile [64][cols + 1]: k_pairsum's odd row
// stride.  Writes are consecutive elements of a row.  Reads hold one gate and rows m ascending: m (cols + 1)
// mod 16 is a bijection of m mod 16, so the 16 rows of a ds_read_b128 group take 16 distinct slots, and the
// 32 rows of a ds_read_b64 half 32 distinct ones; with N = 2 a half holds 32 even rows, two to a slot.
// A workgroup walks up to RSP_PCU_GROUP = 8 such tiles along the pulse axis, the next tile's loads issued before
// the current tile's stores: a tile's store to a column is a run of 512 bytes or 1 KB that, for most P, begins
// and ends inside a 128-byte line whose other part belongs to the next pulse tile; walked by one workgroup the
// two parts meet in one L2 instead of leaving two XCDs as partial lines (DESIGN.md section 3j has the figures).
// Tails along m and g are predicated; nothing outside the P G B output elements is written.
#include "rsp_device.h"

namespace {

constexpr int NZ = RSP_PC_NZ, TP = RSP_PCK_COLS, LS = TP + RSP_PCK_PAD;
constexpr int TM = RSP_PCU_ROWS;
static_assert(NZ == 8 && (NZ & (NZ - 1)) == 0 && TP == RSP_THREADS, "a z slab row per 8 slots, a lane per pulse and round");
static_assert(LS % 32 == 4, "the pack tile's read rule: row stride = 4 mod 16 (16-byte) and mod 32 (8-byte elements)");

template <class E, int N>
struct alignas(sizeof(E) * N) Pack {   // N consecutive elements: one load or store
    E e[N];
};

template <class T, int N>
__global__ __launch_bounds__(RSP_THREADS) void k_pc_pack(Geometry g, int pitch, const cx<T>* __restrict__ x,
                                                         cx<T>* __restrict__ z) {
    typedef cx<T> V;
    typedef Pack<V, N> U;
    constexpr int EPU = 16 / (int)sizeof(V);   // elements of a 16-byte z unit
    typedef Pack<V, EPU> ZU;
    V* tile = reinterpret_cast<V*>(rsp_lds);   // [NZ][LS]
    const int P = g.P, tid = threadIdx.x;
    const int tiles = (P + TP - 1) / TP;
    const int c = blockIdx.x % g.nzc, rest = blockIdx.x / g.nzc;
    const int pt = rest % tiles, b = rest / tiles;
    const int p0 = pt * TP, pe = min(TP, P - p0);   // the tile's pulses
    const int uv = (pe + N - 1) / N;                // load units of a sample row (N = 2: P, so pe, is even)
    const V* __restrict__ xb = x + (size_t)b * pitch + p0;
    U xin[NZ];
#pragma unroll
    for (int k = 0; k < NZ; ++k) {
        const int u = tid + k * RSP_THREADS;
        xin[k] = U{};
        if (u < NZ * uv) {
            const int s = u / uv, m = N * (u - s * uv), np = c * NZ + s;
            if (np < g.nU) xin[k] = *reinterpret_cast<const U*>(xb + (size_t)used_sample(g, np) * P + m);
        }
    }
#pragma unroll
    for (int k = 0; k < NZ; ++k) {
        const int u = tid + k * RSP_THREADS;
        if (u < NZ * uv) {
            const int s = u / uv, m = N * (u - s * uv);
#pragma unroll
            for (int e = 0; e < N; ++e) tile[s * LS + m + e] = xin[k].e[e];
        }
    }
    __syncthreads();
    // the slab's pe NZ consecutive elements, 16 bytes per lane
    ZU* __restrict__ zs = reinterpret_cast<ZU*>(z + ((size_t)(b * g.nzc + c) * P + p0) * NZ);
    const int nunits = pe * NZ / EPU;
#pragma unroll
    for (int k = 0; k < NZ / EPU; ++k) {
        const int q = tid + k * RSP_THREADS;
        if (q < nunits) {
            const int e0 = q * EPU, m = e0 / NZ, s = e0 % NZ;
            ZU o;
#pragma unroll
            for (int e = 0; e < EPU; ++e) o.e[e] = tile[(s + e) * LS + m];
            zs[q] = o;
        }
    }
}

template <class T, int N>
__global__ __launch_bounds__(RSP_THREADS) void k_pc_unpack(int P, int G, const cx<T>* __restrict__ r,
                                                           cx<T>* __restrict__ pc) {
    typedef cx<T> V;
    typedef Pack<V, N> U;
    constexpr int TG = pcu_cols(sizeof(T) == 8 ? RSP_PREC_F64 : RSP_PREC_F32), LW = TG + RSP_PCU_PAD;
    constexpr int RPP = RSP_THREADS / TG, NL = TM / RPP;   // rows per load pass, loads per thread
    constexpr int UV = TM / N, NS = TG * UV / RSP_THREADS; // store units of a column, stores per thread
    static_assert(LW % 2 == 1 && TM % RPP == 0 && (TG * UV) % RSP_THREADS == 0, "odd row stride; whole passes");
    V* tile = reinterpret_cast<V*>(rsp_lds);   // [TM][LW]
    const int tid = threadIdx.x;
    const int ct = (G + TG - 1) / TG, rt = (P + TM - 1) / TM, rg = (rt + RSP_PCU_GROUP - 1) / RSP_PCU_GROUP;
    const int gt = blockIdx.x % ct, rest = blockIdx.x / ct;
    const int grp = rest % rg, b = rest / rg;
    const int g0 = gt * TG, mt0 = grp * RSP_PCU_GROUP, nt = min(RSP_PCU_GROUP, rt - mt0);
    const int gl = tid % TG, rl = tid / TG;
    const V* __restrict__ src = r + (size_t)b * P * G + g0 + gl;
    V* __restrict__ dst = pc + ((size_t)b * G + g0) * P;
    V xin[NL];
    auto load = [&](int m0) {
#pragma unroll
        for (int k = 0; k < NL; ++k) {
            const int row = m0 + rl + k * RPP;
            xin[k] = V{};
            if (g0 + gl < G && row < P) xin[k] = src[(size_t)row * G];
        }
    };
    load(mt0 * TM);
    for (int t = 0; t < nt; ++t) {
        const int m0 = (mt0 + t) * TM;
#pragma unroll
        for (int k = 0; k < NL; ++k) tile[(rl + k * RPP) * LW + gl] = xin[k];
        __syncthreads();
        if (t + 1 < nt) load(m0 + TM);   // in flight across this tile's stores
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const int u = tid + k * RSP_THREADS, col = u / UV, m = N * (u % UV);
            if (g0 + col < G && m0 + m < P) {   // N = 2: P is even, so a unit lies inside the cube or outside it as a whole
                U o;
#pragma unroll
                for (int e = 0; e < N; ++e) o.e[e] = tile[(m + e) * LW + col];
                *reinterpret_cast<U*>(dst + (size_t)col * P + m0 + m) = o;
            }
        }
        __syncthreads();   // the tile is read before the next one replaces it
    }
}

template <class T>
hipError_t launch_pc_pack_t(const PcDesc& d, const void* beams, int pitch, void* z, hipStream_t s) {
    constexpr int EPU = 16 / (int)sizeof(cx<T>);
    const cx<T>* x = static_cast<const cx<T>*>(beams);
    cx<T>* zp = static_cast<cx<T>*>(z);
    const size_t lds = pck_lds_bytes(d.g.prec);
    const dim3 grid((unsigned)d.pack_wg), block(RSP_THREADS);
    if (EPU > 1 && d.g.P % EPU == 0 && pitch % EPU == 0 && (uintptr_t)beams % 16 == 0)
        return launch(k_pc_pack<T, EPU>, grid, block, lds, s, d.g, pitch, x, zp);
    return launch(k_pc_pack<T, 1>, grid, block, lds, s, d.g, pitch, x, zp);
}

template <class T>
hipError_t launch_pc_unpack_t(const PcDesc& d, const void* res, void* pc, hipStream_t s) {
    constexpr int EPU = 16 / (int)sizeof(cx<T>);
    const cx<T>* r = static_cast<const cx<T>*>(res);
    cx<T>* o = static_cast<cx<T>*>(pc);
    const size_t lds = pcu_lds_bytes(d.g.prec);
    const dim3 grid((unsigned)d.unpack_wg), block(RSP_THREADS);
    if (EPU > 1 && d.g.P % EPU == 0 && (uintptr_t)pc % 16 == 0)
        return launch(k_pc_unpack<T, EPU>, grid, block, lds, s, d.g.P, d.g.G, r, o);
    return launch(k_pc_unpack<T, 1>, grid, block, lds, s, d.g.P, d.g.G, r, o);
}

}  // namespace

hipError_t launch_pc_pack(const PcDesc& d, const void* beams, int pitch, void* z, hipStream_t s) {
    return d.g.prec == RSP_PREC_F64 ? launch_pc_pack_t<double>(d, beams, pitch, z, s)
                                    : launch_pc_pack_t<float>(d, beams, pitch, z, s);
}

hipError_t launch_pc_unpack(const PcDesc& d, const void* res, void* pc, hipStream_t s) {
    return d.g.prec == RSP_PREC_F64 ? launch_pc_unpack_t<double>(d, res, pc, s)
                                    : launch_pc_unpack_t<float>(d, res, pc, s);
}
