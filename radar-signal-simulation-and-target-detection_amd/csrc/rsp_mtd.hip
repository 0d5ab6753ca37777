// rsp_mtd.hip -- the MTD as a stand-alone stage for CDNA4 (gfx950): a slow-time transform of any
// length on a cube in MATLAB's own layout, and its launcher.
//
//   k_mtd_any : pc [P x G x n_maps] (pulse index fastest) -> out [nfft x G x n_maps],
//               out[:, g, map] = shift(DFT_nfft([pc[:, g, map] .* win ; zeros(nfft - P)]))
//               (main_simulate_echoes_with_array_v7_7.m:501-503, fun_process_single_frame.m:131-135).
//
// A workgroup takes `cols` consecutive columns of one map (MtdDesc, rsp_geometry.h): P cols contiguous
// elements in, nfft cols contiguous elements out, and rows of L points in LDS in between, L = nfft
// (a power of two) or the chirp-z length M.  Both routes are the Stockham passes of rsp_fft_passes.h
// over PlanPow2<log2 L>, 16 points per thread, twiddles from the compact tables in global memory (L1/L2):
//   power of two : rows zero-filled to nfft, the forward passes, the rows stored (shifted).
// Complex double loads the first pass's inputs and stores the last pass's outputs straight from and to
// global memory; complex single stages both in LDS for 16-byte accesses (k_mtd_any says why).
//   chirp-z      : Bluestein.  With w[m] = exp(-i pi m^2 / nfft), k m = (k^2 + m^2 - (k - m)^2) / 2 gives
//                  X[k] = w[k] sum_m (x[m] w[m]) conj(w)[k - m]: a[m] = x[m] win[m] w[m] zero-filled to M,
//                  the forward passes, the product with the filter spectrum Bf (the M-point DFT of
//                  conj(w) wrapped round M, 1 / M folded in; host-built, read from L2), the inverse passes
//                  over the reversed plan as K2 runs them, and w[k] on the way out.  M >= 2 nfft - 1, so
//                  the circular convolution's wrap-around never reaches the nfft outputs kept.
// No route's work grows as nfft^2.  DESIGN.md section 3h.
#include "rsp_device.h"
#include "rsp_fft_passes.h"

namespace {

// Store policies of the passes that do more than put a point back into its row.
// The forward transform's last pass on the chirp-z route: the product with the filter spectrum on the way
// into LDS (position o of the row is frequency o).
template <class V>
struct StoreLdsMul {
    V* buf;
    const V* __restrict__ Bf;
    __device__ __forceinline__ void put(int, int, int o, int loff, V x) const { buf[loff] = vmul(x, Bf[o]); }
};
// The last pass of all in complex double: frequency o of column `row` straight to its row of the result,
// (o + floor(nfft / 2)) mod nfft (shift) or o, times w[o] on the chirp-z route.  The lanes of a pass hold
// consecutive o, so a wave's store is runs of consecutive 16-byte elements.
template <class V, bool CZ>
struct StoreOut {
    V* __restrict__ dst;
    const V* __restrict__ w;
    int nfft, half, ncols;
    __device__ __forceinline__ void put(int, int row, int o, int, V x) const {
        if (row < ncols && o < nfft) {
            if constexpr (CZ) x = vmul(x, w[o]);
            const int v = o + half < nfft ? o + half : o + half - nfft;
            dst[(size_t)row * nfft + v] = x;
        }
    }
};

template <class V> struct StoresLds<StoreLdsMul<V>> { static constexpr bool value = true; };   // it writes the rows the pass reads

// Complex double (16-byte elements) takes its columns from global memory straight into the registers of
// the first pass and stores the last pass's registers straight to the result: the rows make two LDS round
// trips and two barriers fewer.  Complex single goes through LDS at both ends, so that its global
// accesses are 16-byte pairs of elements wherever a column starts on 16 bytes (MtdDesc::vec) and single
// elements where it does not (odd P or nfft, an unaligned base).
template <class T, int LG, bool CZ>
__global__ __launch_bounds__(mtd_threads(1 << LG, sizeof(T) == 8 ? RSP_PREC_F64 : RSP_PREC_F32)) void k_mtd_any(
    MtdDesc d, const cx<T>* __restrict__ pc, const T* __restrict__ win, const cx<T>* __restrict__ tab,
    const cx<T>* __restrict__ tw, cx<T>* __restrict__ out) {
    typedef cx<T> V;
    typedef PlanPow2<LG> Plan;
    typedef PlanRev<Plan> PlanI;
    constexpr int PREC = sizeof(T) == 8 ? RSP_PREC_F64 : RSP_PREC_F32;
    constexpr int L = 1 << LG, COLS = mtd_cols(L, PREC), NTHR = mtd_threads(L, PREC), RS = mtd_row_stride(L);
    constexpr int SH = RSP_K2_SH, PTS = (COLS * L + NTHR - 1) / NTHR, NP = Plan::p.np;
    constexpr int TWI = plan_tw_total(Plan::p, true);   // the reversed plan's tables follow the forward ones
    constexpr bool DIRECT_IO = sizeof(T) == 8;
    constexpr int HL = L >= 2 ? L / 2 : 1;   // element pairs of a row (complex single)
    V* Y = reinterpret_cast<V*>(rsp_lds);   // [COLS][RS]
    const int tix = threadIdx.x;
    const int map = blockIdx.x / d.col_tiles, g0 = (blockIdx.x - map * d.col_tiles) * COLS;
    const int ncols = min(COLS, d.G - g0), P = d.P, nfft = d.nfft;
    const size_t c0 = (size_t)map * d.G + g0;   // the workgroup's first column of the cube
    const V* __restrict__ src = pc + c0 * P;
    V* __restrict__ dst = out + c0 * nfft;
    const V* __restrict__ w = tab;
    const bool has_win = d.has_win != 0;
    const int half = d.shift ? nfft >> 1 : 0;   // row v holds frequency (v - floor(nfft / 2)) mod nfft
    auto prep = [=](V x, int m) {   // x[m] win[m] (w[m])
        if (has_win) x = x * win[m];
        if constexpr (CZ) x = vmul(x, w[m]);
        return x;
    };
    const StoreLds<V> st{Y};
    const StoreLdsMul<V> stmul{Y, tab + nfft};

    if constexpr (DIRECT_IO) {
        const StoreOut<V, CZ> outp{dst, w, nfft, half, ncols};
        if constexpr (NP == 0) {   // one point
            if (tix < ncols) dst[tix] = prep(src[tix], 0);
        } else {
            // the first pass from global memory: butterfly j of a column reads pulses j + r L / R, zeros past P
            constexpr int R0 = Plan::p.rad[0], NB0 = (PTS + R0 - 1) / R0, nb = L / R0;
            V v[NB0][R0];
#pragma unroll
            for (int t = 0; t < NB0; ++t) {
                const int beta = tix + t * NTHR;
                if (beta < nb * COLS) {
                    const int col = beta / nb, j = beta - col * nb;
#pragma unroll
                    for (int r = 0; r < R0; ++r) {
                        const int m = j + r * nb;
                        v[t][r] = (col < ncols && m < P) ? prep(src[(size_t)col * P + m], m) : V{};
                    }
                }
            }
            if constexpr (NP == 1) {
                if constexpr (CZ) {
                    sh_store<R0, false, NB0, SH, NTHR, L, 1>(v, RS, COLS, stmul);
                    __syncthreads();
                } else {
                    sh_store<R0, false, NB0, SH, NTHR, L, 1>(v, RS, COLS, outp);
                }
            } else {
                sh_store<R0, false, NB0, SH, NTHR, L, 1>(v, RS, COLS, st);
                __syncthreads();
                if constexpr (CZ)
                    fft_range<Plan, 1, NP, PTS, false, SH, NTHR, true>(Y, RS, COLS, tw, st, stmul);
                else
                    fft_range<Plan, 1, NP, PTS, false, SH, NTHR, true, 0, false>(Y, RS, COLS, tw, st, outp);
            }
            if constexpr (CZ) fft_range<PlanI, 0, NP, PTS, true, SH, NTHR, true, 0, false>(Y, RS, COLS, tw + TWI, st, outp);
        }
    } else {
        // the columns into LDS, zero-filled to L (and the columns past G: zeros)
        if (L >= 2 && (d.vec & 1)) {   // P even: 16-B loads of (m, m + 1)
            for (int e = tix; e < COLS * L / 2; e += NTHR) {
                const int col = e / HL, m = 2 * (e % HL);
                V x0 = V{}, x1 = V{};
                if (col < ncols && m < P) {
                    const f32x4 q = *reinterpret_cast<const f32x4*>(src + (size_t)col * P + m);
                    x0 = prep(V{q.x, q.y}, m);
                    x1 = prep(V{q.z, q.w}, m + 1);
                }
                Y[col * RS + lidx<SH>(m)] = x0;
                Y[col * RS + lidx<SH>(m + 1)] = x1;
            }
        } else {
            for (int e = tix; e < COLS * L; e += NTHR) {
                const int col = e >> LG, m = e & (L - 1);
                V x = V{};
                if (col < ncols && m < P) x = prep(src[(size_t)col * P + m], m);
                Y[col * RS + lidx<SH>(m)] = x;
            }
        }
        __syncthreads();
        if constexpr (CZ) {
            fft_range<Plan, 0, NP, PTS, false, SH, NTHR, true>(Y, RS, COLS, tw, st, stmul);
            fft_range<PlanI, 0, NP, PTS, true, SH, NTHR, true>(Y, RS, COLS, tw + TWI, st, st);
        } else {
            fft_range<Plan, 0, NP, PTS, false, SH, NTHR, true>(Y, RS, COLS, tw, st, st);
        }
        // rows v < nfft out
        auto bin = [=](int col, int k) {
            V y = Y[col * RS + lidx<SH>(k)];
            if constexpr (CZ) y = vmul(y, w[k]);
            return y;
        };
        if (L >= 2 && (d.vec & 2)) {   // nfft even: 16-B stores of (v, v + 1)
            for (int e = tix; e < COLS * L / 2; e += NTHR) {
                const int col = e / HL, v = 2 * (e % HL);
                if (col < ncols && v < nfft) {
                    int k0 = v - half;
                    if (k0 < 0) k0 += nfft;
                    const int k1 = k0 + 1 == nfft ? 0 : k0 + 1;
                    const V y0 = bin(col, k0), y1 = bin(col, k1);
                    *reinterpret_cast<f32x4*>(dst + (size_t)col * nfft + v) = f32x4{y0.x, y0.y, y1.x, y1.y};
                }
            }
        } else {
            for (int e = tix; e < COLS * L; e += NTHR) {
                const int col = e >> LG, v = e & (L - 1);
                if (col < ncols && v < nfft) {
                    int k = v - half;
                    if (k < 0) k += nfft;
                    dst[(size_t)col * nfft + v] = bin(col, k);
                }
            }
        }
    }
}

template <class T, int LG, bool CZ>
hipError_t launch_mtd_k(const MtdDesc& d, const void* pc, const void* win, const void* tab, const void* tw, void* out,
                        hipStream_t s) {
    constexpr int PREC = sizeof(T) == 8 ? RSP_PREC_F64 : RSP_PREC_F32, L = 1 << LG;
    return launch(k_mtd_any<T, LG, CZ>, dim3((unsigned)d.col_tiles * (unsigned)d.n_maps), dim3(mtd_threads(L, PREC)),
                  mtd_lds_bytes(L, PREC), s, d, static_cast<const cx<T>*>(pc), static_cast<const T*>(win),
                  static_cast<const cx<T>*>(tab), static_cast<const cx<T>*>(tw), static_cast<cx<T>*>(out));
}

// power of two: L = nfft = 1 .. 2048; chirp-z: M = 8 (nfft = 3) .. 4096 (nfft = 2047)
#define MTD_CASE(LG, CZ) \
    case LG: return launch_mtd_k<T, LG, CZ>(d, pc, win, tab, tw, out, s)
template <class T>
hipError_t launch_mtd_t(const MtdDesc& d, const void* pc, const void* win, const void* tab, const void* tw, void* out,
                        hipStream_t s) {
    if (!d.chirp) switch (d.lgL) {
            MTD_CASE(0, false); MTD_CASE(1, false); MTD_CASE(2, false); MTD_CASE(3, false);
            MTD_CASE(4, false); MTD_CASE(5, false); MTD_CASE(6, false); MTD_CASE(7, false);
            MTD_CASE(8, false); MTD_CASE(9, false); MTD_CASE(10, false); MTD_CASE(11, false);
            default: return hipErrorInvalidValue;
        }
    switch (d.lgL) {
        MTD_CASE(3, true); MTD_CASE(4, true); MTD_CASE(5, true); MTD_CASE(6, true); MTD_CASE(7, true);
        MTD_CASE(8, true); MTD_CASE(9, true); MTD_CASE(10, true); MTD_CASE(11, true); MTD_CASE(12, true);
        default: return hipErrorInvalidValue;
    }
}
#undef MTD_CASE

}  // namespace

hipError_t launch_mtd(const MtdDesc& d, int prec, const void* pc, const void* win, const void* tab, const void* tw,
                      void* out, hipStream_t s) {
    return prec == RSP_PREC_F64 ? launch_mtd_t<double>(d, pc, win, tab, tw, out, s)
                                : launch_mtd_t<float>(d, pc, win, tab, tw, out, s);
}
