// rsp_k1.hip -- K1 of the per-frame radar chain for CDNA4 (gfx950), and its launchers.
//
//   k1_dbf_mtd  : cube [C][N][P] (MATLAB [P x N x C], pulse fastest) -> for each used
//                 fast-time sample n: DBF over channels (fsf:93-97, y = x * W'),
//                 MTD window + P-point FFT + fftshift over pulses (fsf:131-136);
//                 writes Doppler-domain rows z[b][tile][v][NT] (NT samples per 64 B).
//   k1p_dbf_mtd, k1q_dbf_mtd : the persistent forms of it (power-of-two P; P = R Q).
//
// The pipeline and the reordering of its stages are in DESIGN.md; K2 (rsp_k2.hip) reads z.
#include "rsp_dbf.h"   // rsp_device.h, Dbf<T>
#include "rsp_fft_passes.h"

namespace {

// Diagnostic builds (-DRSP_DEBUG_KNOBS) only: K1 phase stamps (s_memrealtime, 100 MHz).  The
// shipped library has neither the variable nor the stamps.
#ifdef RSP_DEBUG_KNOBS
// persistent K1: workgroup x, loop iteration it < 64 writes [(x 64 + it) 4 + i] (tools/ab/k1_phases.py)
__device__ unsigned long long* rsp_k1_trace;
#define K1_STAMP(it, i)                                                                                 \
    do {                                                                                                \
        if (rsp_k1_trace && threadIdx.x == 0 && (it) < 64)                                              \
            rsp_k1_trace[((size_t)blockIdx.x * 64 + (it)) * 4 + (i)] = wall_clock64();                 \
    } while (0)
extern "C" int rsp_debug_set_k1_trace(unsigned long long* p) {
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(rsp_k1_trace), &p, sizeof(p));
}
#else
#define K1_STAMP(it, i) ((void)0)
#endif

// ======================================================================================
// K1: DBF + MTD window + slow-time FFT + fftshift -> compacted rows
// ======================================================================================
#define K1_SH 4   // LDS pad shift of the slow-time FFT rows (row stride P + P/16)

// The DBF on the matrix cores (Dbf<T>): rsp_dbf.h, shared with k_dbf.

// Flat tile index TT of a persistent launch -> (frame, tile).
struct FrameTile { int f, tile; };
__device__ __forceinline__ FrameTile frame_tile(const Geometry& g, int TT) {
    const int f = __builtin_amdgcn_readfirstlane(TT / g.ntiles);
    return FrameTile{f, TT - f * g.ntiles};
}

// D of one sub-tile (sample nl, pulses p .. p + PPL*... of this lane) x window -> padded LDS
// columns [b * NT + nl][Ppad] (Re / Im parts as two scalar stores).
// plim: pulses >= plim (the last sub-tile's lanes past P when P is not a multiple of 16) are not
// stored.
template <class T, int MB>
__device__ __forceinline__ void dbf_store(T* Yf, const typename Dbf<T>::Acc (&acc)[MB][Dbf<T>::NACC], int grp, int B,
                                          int NT, int Ppad, int nl, int p, const T (&w)[Dbf<T>::NACC], int sh,
                                          int plim) {
    if constexpr (sizeof(T) == 8) {
        // double: registers i and i + 2 hold Re and Im of the same beam (rows grp + 4 i and
        // grp + 4 i + 8), so each beam's complex value goes out as one 16-B store.  Two 8-B
        // stores of the parts at a 16-B lane stride put lanes l and l + 8 on the same banks of
        // the 32-bank write path (2-way); the 16-B stores of 8 consecutive lanes cover the 32
        // banks once.
        const int ip = sh ? p + (p >> K1_SH) : p;
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int b = mb * 8 + ((grp + 4 * i) & 7);
                if (b < B && p < plim)
                    reinterpret_cast<d2*>(Yf)[(b * NT + nl) * Ppad + ip] =
                        d2{acc[mb][0][i] * w[0], acc[mb][0][i + 2] * w[0]};
            }
        return;
    }
#pragma unroll
    for (int a = 0; a < Dbf<T>::NACC; ++a) {
        const int pa = p + a;
        const int ip = sh ? pa + (pa >> K1_SH) : pa;
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {   // D row m: beam mb*8 + (m & 7), part m >> 3
                const int m = Dbf<T>::row(grp, i);
                const int b = mb * 8 + (m & 7);
                if (b < B && pa < plim) Yf[2 * ((b * NT + nl) * Ppad + ip) + (m >> 3)] = acc[mb][a][i] * w[a];
            }
    }
}

// Last slow-time FFT pass straight from registers to z with fftshift (fsf:135): column
// row = b NT + nl, frequency o -> Doppler cell v = (o + P/2) mod P.  16 lanes of a butterfly
// group write consecutive v of one column (64 B apart) and the next 16 lanes the neighbouring
// column, so the lines fill within the workgroup.
// Byte offset in z of column col = b NT + nl of store s's tile at Doppler cell v (StoreZ, StoreZq).
template <class V, class St>
__device__ __forceinline__ unsigned z_off(const St& s, int col, int v) {
    const int b = col >> s.lgNT, nl = col & ((1 << s.lgNT) - 1);
    const int np = (s.tile << s.lgNT) + nl;   // compacted sample
    return (unsigned)((((b * s.nzc + (np >> s.lgNZ)) * s.P + v) << s.lgNZ) + (np & ((1 << s.lgNZ) - 1))) * (unsigned)sizeof(V);
}
template <class V>
struct StoreZ {
    __amdgpu_buffer_rsrc_t z; int lgNT, nzc, tile, P, half, lgNZ;
    __device__ __forceinline__ void put(int, int row, int o, int, V x) const {
        buf_st<RSP_Z_AUX>(z, z_off<V>(*this, row, (o + half) & (P - 1)), x);   // power-of-two P: the wrap is a mask
    }
};

// In-place decimation-in-frequency FFT of length P = 16 R1 over nrows LDS rows (stride rs, pads
// per 2^SH), two passes:
//   A: radix 16 over x[n1 R1 + n2] (n1 < 16), output k1 times W_P^(n2 k1), written back to the
//      slots it was read from (n1 -> k1): no thread writes a slot another reads, so the pass
//      needs no read/write barrier (a Stockham pass does);
//   B: radix R1 over the R1 contiguous y[k1 R1 + n2] -> X[k1 + 16 k2], stored through st with
//      the natural bin o = k1 + 16 k2 (the z store applies fftshift).
// twd = the compact pass-A table in LDS, [i][n2] = W_P^(n2 2^i) (load_tw).  Same arithmetic per
// output as the radix-16 x radix-R1 Stockham plan, with the twiddles on the other side.
// PTS = points per thread (nrows P <= PTS NTHR, k1_persistent_fits).
// Which K1 slow-time FFTs run k1_fft_dif: k1_dif (rsp_geometry.h)
#define K1_DIF k1_dif(LGP, CP)

template <int LGP, int PTS, int NTHR, int SH, class V, class St>
__device__ __forceinline__ void k1_fft_dif(V* buf, int rs, int nrows, const V* twd, const St& st) {
    constexpr int P = 1 << LGP, R1 = P / 16, LGR1 = LGP - 4;
    static_assert(R1 >= 4 && R1 <= 16, "P in 64..256");
    {
        const int total = R1 * nrows;
        constexpr int NB = (PTS + 15) / 16;
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            const int beta = threadIdx.x + t * NTHR;
            if (beta < total) {
                const int row = beta >> LGR1, n2 = beta & (R1 - 1);
                V* src = buf + row * rs;
                V x[16];
#pragma unroll
                for (int n1 = 0; n1 < 16; ++n1) x[n1] = src[lidx<SH>(n1 * R1 + n2)];
                V b[4];   // W^(n2 2^i)
#pragma unroll
                for (int i = 0; i < 4; ++i) b[i] = twd[i * R1 + n2];
                Dft<16, false, V>::run(x);
                // W^(n2 k1) for k1 = 1..15 as in load_tw (w[r] = w[2^hb] w[r - 2^hb]), each applied
                // as soon as it exists so that only w[1..8] stay live
                V w[16];
#pragma unroll
                for (int k1 = 1; k1 < 16; ++k1) {
                    const int hb = 1 << clog2(k1);
                    w[k1] = (hb == k1) ? b[clog2(k1)] : vmul(w[hb], w[k1 - hb]);
                    x[k1] = vmul(x[k1], w[k1]);
                }
#pragma unroll
                for (int k1 = 0; k1 < 16; ++k1) src[lidx<SH>(k1 * R1 + n2)] = x[k1];
            }
        }
    }
    __syncthreads();
    {
        const int total = 16 * nrows;
        constexpr int NB = (16 * PTS + P - 1) / P;
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            const int beta = threadIdx.x + t * NTHR;
            if (beta < total) {
                const int row = beta >> 4, k1 = beta & 15;
                const V* src = buf + row * rs;
                V y[R1];
#pragma unroll
                for (int n2 = 0; n2 < R1; ++n2) y[n2] = src[lidx<SH>(k1 * R1 + n2)];
                Dft<R1, false, V>::run(y);
#pragma unroll
                for (int k2 = 0; k2 < R1; ++k2) st.put(k2, row, k1 + 16 * k2, 0, y[k2]);
            }
        }
    }
}

// Slow-time FFT of every (beam, sample) column in LDS for the runtime log2(P); the last pass
// stores through `last`.
template <class V, class StLast>
__device__ __forceinline__ void k1_fft(int lgp, V* Y, int Ppad, int ncols, const V* twl, const StLast& last, bool dif8) {
    StoreLds<V> st{Y};
    switch (lgp) {
        case 4: fft_passes<4, 16, K1_SH, K1_THREADS>(Y, Ppad, ncols, twl, st, last); break;
        case 5: fft_passes<5, 16, K1_SH, K1_THREADS>(Y, Ppad, ncols, twl, st, last); break;
        case 6: k1_fft_dif<6, 16, K1_THREADS, K1_SH>(Y, Ppad, ncols, twl, last); break;   // twl = twD
        case 7: k1_fft_dif<7, 16, K1_THREADS, K1_SH>(Y, Ppad, ncols, twl, last); break;
        case 8:
            if (dif8) k1_fft_dif<8, 16, K1_THREADS, K1_SH>(Y, Ppad, ncols, twl, last);
            else fft_passes<8, 16, K1_SH, K1_THREADS>(Y, Ppad, ncols, twl, st, last);
            break;
        default: fft_passes<9, 16, K1_SH, K1_THREADS>(Y, Ppad, ncols, twl, st, last); break;
    }
}

// ---- factored slow-time DFT for P = R Q (R = 2 or 4, Q odd >= 3; the reference frame's
// P = 332 = 4 x 83, v8:57), decimation in frequency:
//   X[R k1 + k2] = sum_{n1 < Q} W_Q^(n1 k1) y_k2[n1],  y_k2[n1] = W_P^(n1 k2) sum_{n2 < R} x[n1 + Q n2] W_R^(n2 k2)
// Pass 1 (thread per column and n1 <= (Q - 1) / 2): the radix-R DFTs of x[n1 + Q n2] and of its
// mirror x[Q - n1 + Q n2], their twiddles, and the fold of the Q-point stage
//   s_k2[n] = y_k2[n] + y_k2[Q - n] -> slot n + Q k2,   d_k2[n] = y_k2[n] - y_k2[Q - n] -> slot Q - n + Q k2
// in place (a thread writes exactly the slots it read).  Pass 2: with theta = 2 pi k1 n / Q,
//   A = y[0] + sum_{n=1}^{(Q-1)/2} s_n cos(theta),  Bv = sum_n d_n sin(theta),
//   X[R k1 + k2] = A - i Bv,   X[R (Q - k1) + k2] = A + i Bv          (k1 = 0 .. (Q - 1) / 2)
// -- 4 real FMAs per (k1, n) for two outputs, a quarter of the direct sum.  One lane per
// subsequence (column, k2), a wave-uniform set of RQ_RK frequencies per wave: the (cos, sin)
// pair of a step is the same for every lane (an LDS broadcast read), the lane's s_n and d_n two
// 16-B reads shared by its RQ_RK frequencies.  twq = [fset][n - 1][r] (twQ, in LDS), twp =
// W_P^i, i < P (in LDS); st.put(col, o, x) stores output bin o of column col.
template <int R, int NTHR, class V, class St>
__device__ __forceinline__ void k1_dft_rq(V* buf, int rs, int ncols, int Q, const V* twq, const V* twp, const St& st) {
    const int Qh = (Q - 1) >> 1, KH = Qh + 1;
    {   // ---- pass 1
        const int items = ncols * KH;
        for (int it = threadIdx.x; it < items; it += NTHR) {
            const int c = it / KH, n1 = it - c * KH;
            V* col = buf + c * rs;
            V u[R];
#pragma unroll
            for (int n2 = 0; n2 < R; ++n2) u[n2] = col[n1 + Q * n2];
            Dft<R, false, V>::run(u);
            if (n1 == 0) {   // W_P^0 = 1; y[0] is its own mirror
#pragma unroll
                for (int k2 = 0; k2 < R; ++k2) col[Q * k2] = u[k2];
                continue;
            }
            V v[R];
            const int m = Q - n1;
#pragma unroll
            for (int n2 = 0; n2 < R; ++n2) v[n2] = col[m + Q * n2];
            Dft<R, false, V>::run(v);
            col[n1] = u[0] + v[0];
            col[m] = u[0] - v[0];
#pragma unroll
            for (int k2 = 1; k2 < R; ++k2) {   // n1 k2, m k2 < Q R = P: direct table entries
                const V a = vmul(u[k2], twp[n1 * k2]), b = vmul(v[k2], twp[m * k2]);
                col[n1 + Q * k2] = a + b;
                col[m + Q * k2] = a - b;
            }
        }
    }
    __syncthreads();
    {   // ---- pass 2
        const int NS = ncols * R, nfs = (KH + RQ_RK - 1) / RQ_RK, ngrp = (NS + 63) >> 6;
        const int lane = threadIdx.x & 63;
        const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        for (int item = wv; item < ngrp * nfs; item += NTHR / 64) {   // wave-uniform
            const int grp = item / nfs, fs = item - grp * nfs;
            const int sub = grp * 64 + lane;
            const int sc = min(sub, NS - 1);   // idle lanes read a real column, store nothing
            const int c = sc / R, k2 = sc - c * R;
            const V* col = buf + c * rs + Q * k2;   // s_n = col[n], d_n = col[Q - n]
            const V* tw = twq + fs * Qh * RQ_RK;
            V A[RQ_RK], Bv[RQ_RK];
            const V y0 = col[0];
#pragma unroll
            for (int r = 0; r < RQ_RK; ++r) {
                A[r] = y0;
                Bv[r] = V{};
            }
            // software-pipelined: step n + 1's operands are read while step n computes, so one LDS
            // latency is exposed per step instead of one per (cos, sin) pair.  The reads past the
            // last step are never used and stay inside the workgroup's LDS: s and d at most two
            // slots on (index Qh + 2 <= Q of the subsequence: at worst the first slot of the next
            // one, or of the tables after the last column); the table one row pair on, RQ_RK
            // (Qh even) or 2 RQ_RK (Qh odd) entries past the frequency set's rows, which for the
            // last set is the head of W_P^i -- the launchers request at least 2 RQ_RK entries
            // there (rq_table_elems: P = 6 has only 6).  Pointer steps keep every address a base
            // plus an immediate offset.
            // Two register sets alternate: the reads of the step after next go out before this
            // step's FMAs (the scheduling barriers keep that order), so a read has a whole step of
            // FMAs to land.  Steps are taken in pairs; the second step of the last pair exists only
            // when Qh is even (uniform).
            const V* ps = col + 1;
            const V* pd = col + Q - 1;
            const V* pt = tw;
            V s0 = ps[0], d0 = pd[0], t0[RQ_RK];
#pragma unroll
            for (int r = 0; r < RQ_RK; ++r) t0[r] = pt[r];   // (cos, sin): the same address in every lane
            auto fma_step = [&](const V& sv, const V& dv, const V (&tc)[RQ_RK]) {
#pragma unroll
                for (int r = 0; r < RQ_RK; ++r) {
                    A[r] += tc[r].x * sv;
                    Bv[r] += tc[r].y * dv;
                }
            };
            for (int n = 1; n <= Qh; n += 2) {
                const V s1 = ps[1], d1 = pd[-1];
                V t1[RQ_RK];
#pragma unroll
                for (int r = 0; r < RQ_RK; ++r) t1[r] = pt[RQ_RK + r];
                __builtin_amdgcn_sched_barrier(0);
                fma_step(s0, d0, t0);
                __builtin_amdgcn_sched_barrier(0);
                ps += 2;
                pd -= 2;
                pt += 2 * RQ_RK;
                s0 = ps[0];
                d0 = pd[0];
#pragma unroll
                for (int r = 0; r < RQ_RK; ++r) t0[r] = pt[r];
                __builtin_amdgcn_sched_barrier(0);
                if (n + 1 <= Qh) fma_step(s1, d1, t1);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (sub < NS) {
#pragma unroll
                for (int r = 0; r < RQ_RK; ++r) {
                    const int k1 = fs * RQ_RK + r;
                    if (k1 < KH) {
                        st.put(c, R * k1 + k2, V{A[r].x + Bv[r].y, A[r].y - Bv[r].x});   // A - i Bv
                        if (k1 > 0) st.put(c, R * (Q - k1) + k2, V{A[r].x - Bv[r].y, A[r].y + Bv[r].x});
                    }
                }
            }
        }
    }
}

// z store of the factored DFT's outputs: column col = b NT + nl, bin o -> Doppler cell
// v = (o + P/2) mod P (fftshift, fsf:135), compacted sample tile NT + nl.
template <class V>
struct StoreZq {
    __amdgpu_buffer_rsrc_t z; int lgNT, nzc, tile, P, half, lgNZ;
    __device__ __forceinline__ void put(int col, int o, V x) const {
        int v = o + half;
        v = v >= P ? v - P : v;
        // default cache policy, not non-temporal: one store instruction writes 4 consecutive bins
        // (64 B) of each column and the next one of the wave the other half of the 128-B line,
        // which then merge in L2 (non-temporal partial lines went to HBM unmerged: 1.8x the bytes)
        buf_st<0>(z, z_off<V>(*this, col, v), x);
    }
};

template <class V, class St>
__device__ __forceinline__ void k1_dft_rq_r(int R, V* buf, int rs, int ncols, int Q, const V* twq, const V* twp,
                                            const St& st) {
    if (R == 2) k1_dft_rq<2, K1_THREADS>(buf, rs, ncols, Q, twq, twp, st);
    else k1_dft_rq<4, K1_THREADS>(buf, rs, ncols, Q, twq, twp, st);
}

// BMAX = beams rounded up (4/8/16), CP = channels rounded up (8/16/32).  conj(W) enters as the
// per-lane MFMA A operands (Atab, zero for padded beams/channels), so the DBF has no
// data-dependent branches.  mode 3 = DBF + MTD; mode 0 = transpose only (stage-2 path: the
// input channels are the beams).  Non-power-of-two P = R Q takes the factored DFT (k1_dft_rq),
// any other the direct DFT (O(P^2) per column).
// RQ: the instantiation that runs the factored DFT (its registers stay out of the others).
// K3's state of frame f, zeroed by the workgroup that takes the frame's first tile: the detection
// counter, the deferred-cell and on-demand-row counters next to it and, on the band route, the
// frame's edge-row flags, so that no flag survives into the lane's next batch.
__device__ __forceinline__ void k1_zero_frame_state(const FramePtrs& fp, int f) {
    static_assert(K1_THREADS >= RSP_NEED_BYTES / 4 && RSP_NEED_BYTES % 4 == 0, "one flag word per thread");
    if (!fp.count[f]) return;
    if (threadIdx.x < 3) fp.count[f][threadIdx.x] = 0;
    if (fp.need[f] && threadIdx.x < RSP_NEED_BYTES / 4) reinterpret_cast<int*>(fp.need[f])[threadIdx.x] = 0;
}

template <class T, int BMAX, int CP, bool RQ>
__global__ __launch_bounds__(K1_THREADS, 2) void k1_dbf_mtd(Geometry g, DevConsts k, FramePtrs fp, int mode) {
    typedef cx<T> V;
    typedef Dbf<T> D;
    V* Y = reinterpret_cast<V*>(rsp_lds);   // [B][NT][Ppad] | twiddles
    const int f = blockIdx.y, tile = blockIdx.x;
    const int B = g.B, C = g.C, P = g.P, NT = g.NT, Ppad = g.Ppad;
    if (tile == 0) k1_zero_frame_state(fp, f);
    V* twl = Y + B * NT * Ppad;
    const bool fft = (mode & 2) && g.pow2P;
    const bool rq = RQ && (mode & 2);   // factored DFT: twl = twQ | W_P^i
    const int sh = fft ? K1_SH : 0;
    // P = 64 .. 256 run the in-place k1_fft_dif (as the persistent K1: the same bits), the other
    // powers of two the Stockham passes
    const bool dif = fft && k1_dif(g.logP, CP);
    const V* __restrict__ twPp = static_cast<const V*>(dif ? k.twD : k.twPp);
    const int ntw = dif ? (P >> 2) : g.twPp_elems;
    const T* __restrict__ win = static_cast<const T*>(k.win);
    // twiddles: global loads issued first, LDS stores after the cube loads are in flight (the
    // barrier before the FFT orders them), so no load waits behind a barrier at kernel start
    constexpr int TWPRE = 2;
    V twv[TWPRE];
#pragma unroll
    for (int u = 0; u < TWPRE; ++u) {
        const int i = threadIdx.x + u * K1_THREADS;
        if (fft && i < ntw) twv[u] = twPp[i];
    }
    const V* __restrict__ x = static_cast<const V*>(fp.in[f]);
    const size_t NP = (size_t)g.cpitch;   // channel stride
    if (mode & 1) {
        constexpr int NJ = CP / 4, MB = BMAX <= 8 ? 1 : 2, TPW = (16 / NJ) / MB > 0 ? (16 / NJ) / MB : 1;
        constexpr int PT = 16 * D::PPL;   // pulses per sub-tile
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, grp = lane >> 4, col = lane & 15;
        const T* At = static_cast<const T*>(k.Atab);
        T are[MB][NJ], aim[MB][NJ];   // this lane's A operand: row lane&15, channel 4j + lane>>4
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                are[mb][j] = At[((mb * NJ + j) * 2 + 0) * 64 + lane];
                aim[mb][j] = At[((mb * NJ + j) * 2 + 1) * 64 + lane];
            }
        const int ptiles = (P + PT - 1) / PT;
        const int ntp = NT * ptiles;
        T* Yf = reinterpret_cast<T*>(Y);
        // a wave takes TPW consecutive sub-tiles (pulse tiles of the same sample first), so the
        // pulse row of each (channel, sample) is fetched by one wave in one burst
        for (int t0 = wv * TPW; t0 < ntp; t0 += (K1_THREADS / 64) * TPW) {
            typename D::Ld xv[TPW][NJ];
            int nlv[TPW], pv[TPW];
#pragma unroll
            for (int u = 0; u < TPW; ++u) {      // every load of TPW sub-tiles in flight together
                const int t = t0 + u;
                const int nl = t / ptiles;
                const int p = (t - nl * ptiles) * PT + D::PPL * col;
                const int np = tile * NT + nl;
                int n = -1;
                if (t < ntp && np < g.nU && p < P) n = used_sample(g, np);
                nlv[u] = t < ntp ? nl : -1;
                pv[u] = p;
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int c = min(4 * j + grp, C - 1);   // padded channels carry zero weights
                    xv[u][j] = n >= 0 ? D::bits(*reinterpret_cast<const u32x4*>(x + (size_t)c * NP + (size_t)n * P + p))
                                      : typename D::Ld{};
                }
            }
#pragma unroll
            for (int u = 0; u < TPW; ++u) {
                if (nlv[u] < 0) continue;
                typename D::Acc acc[MB][D::NACC];
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) {
#pragma unroll
                    for (int a = 0; a < D::NACC; ++a) acc[mb][a] = typename D::Acc{};
#pragma unroll
                    for (int j = 0; j < NJ; ++j) D::mma(acc[mb], are[mb][j], aim[mb][j], xv[u][j]);
                }
                const int p = pv[u];
                if (p >= P) continue;
                T w[D::NACC];
#pragma unroll
                for (int a = 0; a < D::NACC; ++a) w[a] = (mode & 2) ? win[p + a] : (T)1;
                dbf_store<T, MB>(Yf, acc, grp, B, NT, Ppad, nlv[u], p, w, sh, P);
            }
        }
    } else {
        // ---- transpose only (stage-2 path: input channels are the beams)
        const int items = NT * P;
        for (int it = threadIdx.x; it < items; it += K1_THREADS) {
            const int nl = it / P, p = it - nl * P;
            const int np = tile * NT + nl;
            int n = -1;
            if (np < g.nU) n = used_sample(g, np);
            const int ip = sh ? p + (p >> K1_SH) : p;
#pragma unroll
            for (int b = 0; b < BMAX; ++b) {
                if (b < B) {
                    V val = n >= 0 ? x[(size_t)b * NP + (size_t)n * P + p] : V{};
                    if (mode & 2) val *= win[p];
                    Y[(b * NT + nl) * Ppad + ip] = val;
                }
            }
        }
    }
    if (fft) {
#pragma unroll
        for (int u = 0; u < TWPRE; ++u) {
            const int i = threadIdx.x + u * K1_THREADS;
            if (i < ntw) twl[i] = twv[u];
        }
        for (int i = threadIdx.x + TWPRE * K1_THREADS; i < ntw; i += K1_THREADS) twl[i] = twPp[i];
    }
    if (RQ && rq) {
        stage_lds<K1_THREADS>(twl, static_cast<const V*>(k.twQ), g.twq_elems);
        stage_lds<K1_THREADS>(twl + g.twq_elems, static_cast<const V*>(k.twP), P);
    }
    __syncthreads();
    V* __restrict__ z = static_cast<V*>(fp.z[f]);
    const int zslab = P * NT;   // contiguous [P][NT] slab per (b, tile)
    const int lgNT = ilog2(NT);
    if (!(mode & 2)) {
        for (int e = threadIdx.x; e < B * zslab; e += K1_THREADS) {
            const int b = e / zslab, rem = e - b * zslab;
            const int v = rem >> lgNT, nl = rem & (NT - 1);
            z[zaddr(g, b, v, tile * NT + nl)] = Y[(b * NT + nl) * Ppad + v];
        }
        return;
    }
    const int half = P >> 1;
    if (fft) {
        // ---- P-point FFT of every (b, nl) column (fsf:135); the last pass applies fftshift
        // and stores the [P][NT] slabs from registers
        const StoreZ<V> sz{buf_rsrc(z, (unsigned)(B * g.nzc * P * g.NZ * sizeof(V))), lgNT, g.nzc, tile, P, half, ilog2(g.NZ)};
        k1_fft(g.logP, Y, Ppad, B * NT, twl, sz, k1_dif(8, CP));
    } else if (RQ && rq) {
        const StoreZq<V> sz{buf_rsrc(z, (unsigned)(B * g.nzc * P * g.NZ * sizeof(V))), lgNT, g.nzc, tile, P, half, ilog2(g.NZ)};
        k1_dft_rq_r(g.rqR, Y, Ppad, B * NT, g.rqQ, twl, twl + g.twq_elems, sz);
    } else {
        // non power-of-two P: direct DFT straight to global (O(P^2) per column)
        const V* __restrict__ twP = static_cast<const V*>(k.twP);
        for (int e = threadIdx.x; e < B * zslab; e += K1_THREADS) {
            const int b = e / zslab, rem = e - b * zslab;
            const int v = rem >> lgNT, nl = rem & (NT - 1);
            z[zaddr(g, b, v, tile * NT + nl)] = dft_bin(Y + (b * NT + nl) * Ppad, twP, P, v);
        }
    }
}

// Points per thread of the persistent K1's slow-time FFT (B * NT * P <= K1_PTS * K1_THREADS):
// the plan halves NT for double so that two tile buffers still fit the 160 KB of LDS.
template <class T> constexpr int k1p_pts() { return sizeof(T) == 4 ? 16 : 8; }


// K1, persistent and software-pipelined (the default for power-of-two P when one load round
// covers a tile): one workgroup per CU walks the (frame, tile) list with two LDS tile buffers.
// While tile TT's slow-time FFT runs out of one buffer and its last pass streams z to HBM, the
// cube loads of the workgroup's next tile are already in flight in registers; the DBF of that
// tile then fills the other buffer.  HBM reads and writes overlap instead of alternating
// round by round.  Same arithmetic as k1_dbf_mtd (mode 3).
// TPWX: sub-tiles a wave loads per tile (>= the tiled K1's TPW): 2 TPW when a tile holds more
// sub-tiles than the 8 waves cover at TPW (config #4: 32 channels x 16 beams, NT = 1 sample x
// 256 pulses = 16 sub-tiles, TPW = 1), so that one load round still covers a tile.
template <class T, int BMAX, int CP, int LGP, int TPWX>
__global__ __launch_bounds__(K1_THREADS, 1) void k1p_dbf_mtd(Geometry g, DevConsts k, FramePtrs fp, int nf) {
    typedef cx<T> V;
    typedef Dbf<T> D;
    V* Y = reinterpret_cast<V*>(rsp_lds);   // tile [B][NT][Ppad] x 2 | twiddles
    const int B = g.B, C = g.C, P = g.P, NT = g.NT, Ppad = g.Ppad;
    const int bufsz = B * NT * Ppad;
    V* twl = Y + 2 * bufsz;
    const int total = nf * g.ntiles;
    int TT = blockIdx.x;
    if (TT >= total) return;
    static_assert(LGP >= 6 && LGP <= 8, "the persistent K1 runs P = 64 .. 256 (k1_persistent_fits)");
    if constexpr (K1_DIF) stage_lds<K1_THREADS>(twl, static_cast<const V*>(k.twD), P >> 2);   // k1_fft_dif's table, 4 x P/16
    else stage_lds<K1_THREADS>(twl, static_cast<const V*>(k.twPp), g.twPp_elems);
    constexpr int NJ = CP / 4, MB = BMAX <= 8 ? 1 : 2, TPW = TPWX;
    constexpr int PT = 16 * D::PPL;
    const int lane = threadIdx.x & 63, grp = lane >> 4, col = lane & 15;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: nlv[] and n are scalar
    const T* At = static_cast<const T*>(k.Atab);
    // the conj(W) operands of the MFMA row blocks: held in registers for the kernel's life with
    // one row block (<= 8 beams); with two (16 beams: x4's 32 channels are 64 VGPRs of them) read
    // from LDS (after the twiddles, k1p_lds) in each sub-tile's DBF, which keeps the kernel
    // within 256 VGPRs without scratch
    constexpr bool ALDS = MB == 2;
    T* Al = reinterpret_cast<T*>(twl + P);
    T are[MB][NJ], aim[MB][NJ];
    if constexpr (ALDS) {
        stage_lds<K1_THREADS>(Al, At, MB * NJ * 2 * 64);
    } else {
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                are[mb][j] = At[((mb * NJ + j) * 2 + 0) * 64 + lane];
                aim[mb][j] = At[((mb * NJ + j) * 2 + 1) * 64 + lane];
            }
    }
    __syncthreads();   // the first DBF reads LDS entries (Atab) other waves wrote
    // this lane's sub-tiles are the same for every tile: (sample nl, pulses p ..) and their
    // window values (k1_persistent_fits guarantees one round: NT * ptiles <= waves * TPWX)
    const int ptiles = P / PT, ntp = NT * ptiles;
    const T* __restrict__ win = static_cast<const T*>(k.win);
    int nlv[TPW], pv[TPW];
    T wv_[TPW][D::NACC];
#pragma unroll
    for (int u = 0; u < TPW; ++u) {
        const int t = wv * TPW + u;
        const int nl = t / ptiles;
        pv[u] = (t - nl * ptiles) * PT + D::PPL * col;
        nlv[u] = t < ntp ? nl : -1;   // pv < P: P >= 64 here; wave-uniform
#pragma unroll
        for (int a = 0; a < D::NACC; ++a) wv_[u][a] = nlv[u] >= 0 ? win[pv[u] + a] : (T)0;
    }
    const size_t NPc = (size_t)g.cpitch;
    // per-lane byte offsets of this lane's (channel, pulses) inside a cube: loop-invariant,
    // so a tile's load issue is scalar sample offsets + buffer loads and writes no VGPR but xv
    // (a VGPR temporary there could be a pending z store's data register: WAR = vmcnt wait)
    unsigned loff[TPW][NJ];
#pragma unroll
    for (int u = 0; u < TPW; ++u)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            loff[u][j] = (unsigned)(((size_t)min(4 * j + grp, C - 1) * NPc + pv[u]) * sizeof(V));
    const unsigned cube_bytes = (unsigned)((size_t)C * NPc * sizeof(V));
    typename D::Ld xv[TPW][NJ];
    bool vld[TPW];   // wave-uniform: sub-tile u of the tile in flight lies inside the used samples
    // (k1q_dbf_mtd's issue differs on purpose: it re-forms the lane offsets instead of keeping loff[][])
    auto issue_u = [&](int Tn, int u) {   // cube loads of sub-tile u of tile Tn (fsf:93 operands) into xv[u]
        const FrameTile ft = frame_tile(g, Tn);
        const __amdgpu_buffer_rsrc_t xr = buf_rsrc(fp.in[ft.f], cube_bytes);
        const int np = ft.tile * NT + nlv[u];
        vld[u] = nlv[u] >= 0 && np < g.nU;
        if (vld[u]) {   // no else: zeroing xv here would wait (vmcnt) on the pending z stores
            const int soff = used_sample(g, np) * P * (int)sizeof(V);
#pragma unroll
            for (int j = 0; j < NJ; ++j)   // non-temporal: the cube is read exactly once
                xv[u][j] = D::bits(__builtin_amdgcn_raw_buffer_load_b128(xr, (int)loff[u][j], soff, 2));
        }
    };
    auto issue = [&](int Tn) {
#pragma unroll
        for (int u = 0; u < TPW; ++u) issue_u(Tn, u);
    };
    // Tnext >= 0 (EARLY2 below): sub-tile u of tile Tnext is loaded into xv[u] as soon as the
    // DBF has read it
    auto dbf = [&](V* buf, int Tnext) {   // MFMA DBF + window of xv into buf (padded rows, K1_SH)
        T* Yf = reinterpret_cast<T*>(buf);
#pragma unroll
        for (int u = 0; u < TPW; ++u) {
            if (nlv[u] < 0) continue;
            typename D::Acc acc[MB][D::NACC];
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int a = 0; a < D::NACC; ++a) acc[mb][a] = typename D::Acc{};
            if (vld[u]) {   // samples past the used ones: zero columns, like k1_dbf_mtd's n = -1
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        if constexpr (ALDS)
                            D::mma(acc[mb], Al[((mb * NJ + j) * 2 + 0) * 64 + lane], Al[((mb * NJ + j) * 2 + 1) * 64 + lane],
                                   xv[u][j]);
                        else
                            D::mma(acc[mb], are[mb][j], aim[mb][j], xv[u][j]);
                    }
            }
            if (Tnext >= 0) issue_u(Tnext, u);
            dbf_store<T, MB>(Yf, acc, grp, B, NT, Ppad, nlv[u], pv[u], wv_[u], K1_SH, P);
        }
    };
    const int lgNT = ilog2(NT), half = P >> 1;
    // EARLY: the next tile's loads go out as soon as this wave's DBF has read xv, before the tile
    // barrier (x2: K1 -0.6 %, bench +0.6 %; x4, since P = 256 runs the in-place DIF FFT as well:
    // K1 2.13 -> 2.06 ms, profiles/r06zc_k1_p256_dif_ab.txt).  Behind the Stockham passes (P = 256
    // with 8 channels, K1_DIF) the xv registers stay live across them and it cost 36 %.
    constexpr bool EARLY = K1_DIF;
    // EARLY2 (complex single): each sub-tile's loads of the next tile go out inside the DBF, right
    // after the sub-tile's MFMAs have read xv[u] (c64 K1 158-163 -> 151 us; in complex double
    // 226-227 -> 236-238, so double issues after the DBF)
    constexpr bool EARLY2 = EARLY && sizeof(T) == 4;
    issue(TT);
    dbf(Y, EARLY2 && TT + (int)gridDim.x < total ? TT + (int)gridDim.x : -1);
    if (EARLY && !EARLY2 && TT + (int)gridDim.x < total) issue(TT + gridDim.x);
    __syncthreads();
    int cur = 0;
    int it = 0;   // diagnostic builds: the phase stamps' iteration index
    for (; TT < total; TT += gridDim.x, ++it) {
        const int Tn = TT + gridDim.x;
        K1_STAMP(it, 0);
        if (!EARLY && Tn < total) issue(Tn);   // next tile's loads fly during this tile's FFT + z stores
        const FrameTile ft = frame_tile(g, TT);
        const int f = ft.f, tile = ft.tile;
        if (tile == 0) k1_zero_frame_state(fp, f);
        V* __restrict__ z = static_cast<V*>(fp.z[f]);
        const StoreZ<V> sz{buf_rsrc(z, (unsigned)(B * g.nzc * P * g.NZ * sizeof(V))), lgNT, g.nzc, tile, P, half, ilog2(g.NZ)};
        // K1_DIF: in place, one barrier between its two passes (P = 256 as 16 x 16: K1 2.23 -> 2.13
        // ms at x4 against the Stockham passes, which 8-channel plans keep).  No barrier after the
        // last pass: its reads of buffer cur are ordered before the next writes of cur (the next
        // tile's dbf) by the barrier below, and dbf now writes cur ^ 1
        if constexpr (K1_DIF)
            k1_fft_dif<LGP, k1p_pts<T>(), K1_THREADS, K1_SH>(Y + cur * bufsz, Ppad, B * NT, twl, sz);
        else
            fft_passes<LGP, k1p_pts<T>(), K1_SH, K1_THREADS, false>(Y + cur * bufsz, Ppad, B * NT, twl,
                                                                     StoreLds<V>{Y + cur * bufsz}, sz);
        K1_STAMP(it, 1);
        if (Tn < total) {
            dbf(Y + (cur ^ 1) * bufsz, EARLY2 && Tn + (int)gridDim.x < total ? Tn + (int)gridDim.x : -1);
            if (EARLY && !EARLY2 && Tn + (int)gridDim.x < total) issue(Tn + gridDim.x);
        }
        K1_STAMP(it, 2);
        __syncthreads();
        K1_STAMP(it, 3);
        cur ^= 1;
    }
}

// K1 for the factored slow-time DFT (P = R Q, k1_dft_rq; the reference frame's P = 332),
// persistent: one 512-thread workgroup per CU walks the flattened (frame, tile) list of the launch
// with ONE tile buffer -- the tile and the DFT's tables fill the LDS (reference frame: 13 beams x
// 332 pulses x 16 B + 33 KB of tables).  Per tile: the DBF consumes the cube loads already in
// registers, the next tile's loads go out at once (non-temporal), and they land while pass 1 and
// pass 2 run; pass 2 stores z.  Same arithmetic per element as k1_dbf_mtd (mode 3, factored DFT):
// bit-identical outputs.  TPW sub-tiles per wave cover a tile in one load round (k1q_tpw); the
// last sub-tile of a column may run past P (lanes with p >= P load the next row's samples or
// zeros past the cube and store nothing).
template <class T, int BMAX, int CP, int TPW>
__global__ __launch_bounds__(K1_THREADS, 1) void k1q_dbf_mtd(Geometry g, DevConsts k, FramePtrs fp, int nf) {
    typedef cx<T> V;
    typedef Dbf<T> D;
    // LDS: tile [B][NT][Ppad] | twQ | W_P^i | the DBF's MFMA A operands (Atab) -- read from LDS
    // per sub-tile rather than held in registers, which pass 2 needs for its operands in flight
    constexpr int NJ = CP / 4, MB = BMAX <= 8 ? 1 : 2;
    V* Y = reinterpret_cast<V*>(rsp_lds);
    const int B = g.B, C = g.C, P = g.P, NT = g.NT, Ppad = g.Ppad;
    V* twq = Y + B * NT * Ppad;
    V* twp = twq + g.twq_elems;
    T* Al = reinterpret_cast<T*>(twp + P);   // [MB][NJ][Re, Im][64]
    const int total = nf * g.ntiles;
    int TT = blockIdx.x;
    if (TT >= total) return;
    stage_lds<K1_THREADS>(twq, static_cast<const V*>(k.twQ), g.twq_elems);
    stage_lds<K1_THREADS>(twp, static_cast<const V*>(k.twP), P);
    stage_lds<K1_THREADS>(Al, static_cast<const T*>(k.Atab), MB * NJ * 2 * 64);
    __syncthreads();   // the first DBF reads Atab entries other waves wrote
    constexpr int PT = 16 * D::PPL;
    const int lane = threadIdx.x & 63, grp = lane >> 4, col = lane & 15;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ptiles = (P + PT - 1) / PT, ntp = NT * ptiles;
    const T* __restrict__ win = static_cast<const T*>(k.win);
    int nlv[TPW], pv[TPW];
    T wv_[TPW][D::NACC];
#pragma unroll
    for (int u = 0; u < TPW; ++u) {
        // round-robin over the waves: a tile's ntp sub-tiles (21 at the reference frame) split
        // 3/3/3/3/3/2/2/2 rather than 4/4/4/4/4/1, so that the waves sharing a SIMD (w, w + 4)
        // carry 6 + 5 + 5 + 5 of the MFMA work instead of 8 + 5 + 4 + 4
        const int t = u * (K1_THREADS / 64) + wv;
        const int nl = t / ptiles;
        pv[u] = (t - nl * ptiles) * PT + D::PPL * col;
        nlv[u] = t < ntp ? nl : -1;   // wave-uniform
#pragma unroll
        for (int a = 0; a < D::NACC; ++a) wv_[u][a] = (nlv[u] >= 0 && pv[u] + a < P) ? win[pv[u] + a] : (T)0;
    }
    const unsigned NPc = (unsigned)g.cpitch;
    const unsigned cube_bytes = (unsigned)((size_t)C * g.cpitch * sizeof(V));
    typename D::Ld xv[TPW][NJ];
    bool vld[TPW];
    // (k1p_dbf_mtd's issue_u differs on purpose: it keeps the lane offsets in loff[][] for the kernel's life)
    auto issue = [&](int Tn) {   // cube loads of tile Tn (fsf:93 operands) into xv
        const FrameTile ft = frame_tile(g, Tn);
        const __amdgpu_buffer_rsrc_t xr = buf_rsrc(fp.in[ft.f], cube_bytes);
        int gq = grp;
        asm volatile("" : "+v"(gq));   // the lane offsets are formed here, not kept live across the DFT
#pragma unroll
        for (int u = 0; u < TPW; ++u) {
            const int np = ft.tile * NT + nlv[u];
            vld[u] = nlv[u] >= 0 && np < g.nU;
            if (vld[u]) {
                const int soff = used_sample(g, np) * P * (int)sizeof(V);
#pragma unroll
                for (int j = 0; j < NJ; ++j) {   // non-temporal: the cube is read exactly once
                    const unsigned lo = ((unsigned)min(4 * j + gq, C - 1) * NPc + (unsigned)pv[u]) * (unsigned)sizeof(V);
                    xv[u][j] = D::bits(__builtin_amdgcn_raw_buffer_load_b128(xr, (int)lo, soff, 2));
                }
            }
        }
    };
    const int lgNT = ilog2(NT), half = P >> 1;
    issue(TT);
    int it = 0;   // diagnostic builds: the phase stamps' iteration index
    for (; TT < total; TT += gridDim.x, ++it) {
        const int Tn = TT + gridDim.x;
        K1_STAMP(it, 0);
        {   // MFMA DBF + window of xv into Y
            T* Yf = reinterpret_cast<T*>(Y);
#pragma unroll
            for (int u = 0; u < TPW; ++u) {
                if (nlv[u] < 0) continue;
                typename D::Acc acc[MB][D::NACC];
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                    for (int a = 0; a < D::NACC; ++a) acc[mb][a] = typename D::Acc{};
                if (vld[u]) {   // samples past the used ones: zero columns
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                        for (int j = 0; j < NJ; ++j)
                            D::mma(acc[mb], Al[((mb * NJ + j) * 2 + 0) * 64 + lane], Al[((mb * NJ + j) * 2 + 1) * 64 + lane],
                                   xv[u][j]);
                }
                dbf_store<T, MB>(Yf, acc, grp, B, NT, Ppad, nlv[u], pv[u], wv_[u], 0, P);
            }
        }
        if (Tn < total) issue(Tn);   // the next tile's loads fly during this tile's DFT
        K1_STAMP(it, 1);
        const FrameTile ft = frame_tile(g, TT);
        const int f = ft.f, tile = ft.tile;
        if (tile == 0) k1_zero_frame_state(fp, f);
        __syncthreads();   // the tile (and, the first time, the tables) in LDS
        K1_STAMP(it, 2);
        V* __restrict__ z = static_cast<V*>(fp.z[f]);
        const StoreZq<V> sz{buf_rsrc(z, (unsigned)(B * g.nzc * P * g.NZ * sizeof(V))), lgNT, g.nzc, tile, P, half, ilog2(g.NZ)};
        k1_dft_rq_r(g.rqR, Y, Ppad, B * NT, g.rqQ, twq, twp, sz);
        K1_STAMP(it, 3);
        __syncthreads();   // pass 2's reads of Y before the next DBF writes it
    }
}

}  // namespace

// Every request below (LDS bytes, the K1 route, the K1 template arguments) is rsp_geometry.h's.
template <class T, int BMAX, int CP>
static hipError_t launch_k1_t(const Geometry& g, const DevConsts& k, const FramePtrs& fp, int nf, int mode,
                              hipStream_t s) {
    const K1Route rt = k1_route(g, mode);
    if (rt.kernel == K1K_PERSISTENT) {
        // one FFT size per instantiation keeps the prefetch registers + FFT under 256 VGPRs
        const size_t ldsp = k1p_lds(g);
        const int grid = std::min(g.ncu, nf * g.ntiles);
        constexpr K1Cfg KC = k1_cfg(CP, BMAX);
        static_assert(KC.CP == CP && KC.BMAX == BMAX, "CP / BMAX are k1_cfg's own values");
        constexpr int TPW = KC.TPW;
        const bool twice = rt.tpw == 2 * TPW;
        const auto go = [&](auto kernel) { return launch(kernel, dim3(grid), dim3(K1_THREADS), ldsp, s, g, k, fp, nf); };
        // the 2 TPW instantiations exist only where k1_route may choose them
        constexpr bool TWICE_OK = KC.twice_ok;
        if (twice && !TWICE_OK) return hipErrorInvalidValue;
        switch (g.logP) {
            case 6:
                if constexpr (TWICE_OK) { if (twice) return go(k1p_dbf_mtd<T, BMAX, CP, 6, 2 * TPW>); }
                return go(k1p_dbf_mtd<T, BMAX, CP, 6, TPW>);
            case 7:
                if constexpr (TWICE_OK) { if (twice) return go(k1p_dbf_mtd<T, BMAX, CP, 7, 2 * TPW>); }
                return go(k1p_dbf_mtd<T, BMAX, CP, 7, TPW>);
            case 8:
                if constexpr (TWICE_OK) { if (twice) return go(k1p_dbf_mtd<T, BMAX, CP, 8, 2 * TPW>); }
                return go(k1p_dbf_mtd<T, BMAX, CP, 8, TPW>);
            default: return hipErrorInvalidValue;
        }
    }
    if constexpr (CP <= 16) {
        constexpr int NJ = k1_cfg(CP, BMAX).NJ;
        if (rt.kernel == K1K_PERSISTENT_FACTORED) {
            const size_t ldsq = k1q_lds(g);
            const int grid = std::min(g.ncu, nf * g.ntiles);
            const auto go = [&](auto kernel) { return launch(kernel, dim3(grid), dim3(K1_THREADS), ldsq, s, g, k, fp, nf); };
            switch (rt.tpw) {
                case 1: return go(k1q_dbf_mtd<T, BMAX, CP, 1>);
                case 2: return go(k1q_dbf_mtd<T, BMAX, CP, 2>);
                case 3: return go(k1q_dbf_mtd<T, BMAX, CP, 3>);
                default:
                    if constexpr (NJ <= 4) return go(k1q_dbf_mtd<T, BMAX, CP, 4>);
                    return hipGetLastError();   // no such instantiation: nothing launched
            }
        }
    }
    if (rt.kernel != K1K_TILED) return hipErrorInvalidValue;
    const bool rq = (mode & 2) && rt.transform == K1X_FACTORED;
    return launch(rq ? k1_dbf_mtd<T, BMAX, CP, true> : k1_dbf_mtd<T, BMAX, CP, false>, dim3(g.ntiles, nf), dim3(K1_THREADS),
                  k1_tiled_lds(g, rq), s, g, k, fp, mode);
}

template <class T, int BMAX>
static hipError_t launch_k1_b(const Geometry& g, const DevConsts& k, const FramePtrs& fp, int nf, int mode,
                              hipStream_t s) {
    switch (k1_cfg(g.C, g.B).CP) {
        case 8: return launch_k1_t<T, BMAX, 8>(g, k, fp, nf, mode, s);
        case 16: return launch_k1_t<T, BMAX, 16>(g, k, fp, nf, mode, s);
        default: return launch_k1_t<T, BMAX, 32>(g, k, fp, nf, mode, s);
    }
}

template <class T>
static hipError_t launch_k1_p(const Geometry& g, const DevConsts& k, const FramePtrs& fp, int nf, int mode,
                              hipStream_t s) {
    switch (k1_cfg(g.C, g.B).BMAX) {
        case 4: return launch_k1_b<T, 4>(g, k, fp, nf, mode, s);
        case 8: return launch_k1_b<T, 8>(g, k, fp, nf, mode, s);
        default: return launch_k1_b<T, 16>(g, k, fp, nf, mode, s);
    }
}

hipError_t launch_k1(const Geometry& g, const DevConsts& k, const FramePtrs& fp, int nf, int mode, hipStream_t s) {
    return g.prec == RSP_PREC_F64 ? launch_k1_p<double>(g, k, fp, nf, mode, s)
                                  : launch_k1_p<float>(g, k, fp, nf, mode, s);
}
