// rsp_fft_passes.h -- the Stockham pass family of the frame chain: the radix-R DFTs in registers,
// one sh_load / sh_store / sh_pass over rows in LDS, and fft_range / fft_passes, which walk a radix
// plan of rsp_geometry.h.  K1's slow-time FFT (rsp_k1.hip), K2's overlap-save blocks (rsp_k2.hip) and
// the stage-2 MTD (rsp_frame_aux.hip) instantiate it; the direct DFT bin of the sizes that have no
// plan is here too.  No kernel.
#pragma once
#include "rsp_device.h"

namespace {

// ---- radix-R DFT kernels in registers -------------------------------------------------
// Radix-2 butterfly with a twiddle, (a, b) <- (a + w b, a - w b): four FMAs for a + w b and one
// per component for a - w b = 2a - (a + w b) -- 6 operations instead of a complex multiply (4)
// plus an add and a subtract (4).
template <class V>
__device__ __forceinline__ void bfly_tw(V& a, V& b, V w) {
    typedef scal<V> S;
    const V t = a + w.xx * b + w.yy * V{-b.y, b.x};
    b = a * (S)2 - t;
    a = t;
}
template <int R, bool INV, class V> struct Dft;
template <bool INV, class V> struct Dft<2, INV, V> {
    static __device__ __forceinline__ void run(V* a) {
        const V t = a[0];
        a[0] = t + a[1];
        a[1] = t - a[1];
    }
};
template <bool INV, class V> struct Dft<4, INV, V> {
    static __device__ __forceinline__ void run(V* a) {
        const V t0 = a[0] + a[2], t1 = a[0] - a[2];
        const V t2 = a[1] + a[3], t3 = vrot<INV>(a[1] - a[3]);
        a[0] = t0 + t2;
        a[2] = t0 - t2;
        a[1] = t1 + t3;
        a[3] = t1 - t3;
    }
};
template <bool INV, class V> struct Dft<8, INV, V> {
    static __device__ __forceinline__ void run(V* a) {
        V e[4] = {a[0], a[2], a[4], a[6]};
        V o[4] = {a[1], a[3], a[5], a[7]};
        Dft<4, INV, V>::run(e);
        Dft<4, INV, V>::run(o);
        constexpr double r = 0.70710678118654752440;
        o[2] = vrot<INV>(o[2]);
        bfly_tw(e[1], o[1], vtw<INV, V>(r, r));
        bfly_tw(e[3], o[3], vtw<INV, V>(-r, r));
        a[0] = e[0] + o[0];
        a[4] = e[0] - o[0];
        a[2] = e[2] + o[2];
        a[6] = e[2] - o[2];
        a[1] = e[1];
        a[5] = o[1];
        a[3] = e[3];
        a[7] = o[3];
    }
};
template <bool INV, class V> struct Dft<16, INV, V> {
    static __device__ __forceinline__ void run(V* a) {
        V e[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            e[k] = a[2 * k];
            o[k] = a[2 * k + 1];
        }
        Dft<8, INV, V>::run(e);
        Dft<8, INV, V>::run(o);
        constexpr double c1 = 0.92387953251128675613, s1 = 0.38268343236508977173, r = 0.70710678118654752440;
        o[4] = vrot<INV>(o[4]);
        bfly_tw(e[1], o[1], vtw<INV, V>(c1, s1));
        bfly_tw(e[2], o[2], vtw<INV, V>(r, r));
        bfly_tw(e[3], o[3], vtw<INV, V>(s1, c1));
        bfly_tw(e[5], o[5], vtw<INV, V>(-s1, c1));
        bfly_tw(e[6], o[6], vtw<INV, V>(-r, r));
        bfly_tw(e[7], o[7], vtw<INV, V>(-c1, s1));
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k == 0 || k == 4) {
                a[k] = e[k] + o[k];
                a[k + 8] = e[k] - o[k];
            } else {
                a[k] = e[k];
                a[k + 8] = o[k];
            }
        }
    }
};

// Odd radices of the mixed-radix overlap-save blocks (M = 5 * 2^k, 3 * 2^k).
template <bool INV, class V> struct Dft<3, INV, V> {
    static __device__ __forceinline__ void run(V* a) {
        typedef scal<V> S;
        constexpr double h = 0.86602540378443864676;   // sin(2 pi / 3)
        const V s = a[1] + a[2], d = a[1] - a[2];
        const V t = a[0] - s * (S)0.5;
        const V u = vrot<INV>(d) * (S)h;                // -+ i sin(2pi/3) (x1 - x2)
        a[0] = a[0] + s;
        a[1] = t + u;
        a[2] = t - u;
    }
};
template <bool INV, class V> struct Dft<5, INV, V> {
    static __device__ __forceinline__ void run(V* a) {
        typedef scal<V> S;
        constexpr double c1 = 0.30901699437494742410, c2 = -0.80901699437494742410;   // cos(2pi/5), cos(4pi/5)
        constexpr double s1 = 0.95105651629515357212, s2 = 0.58778525229247312917;    // sin(2pi/5), sin(4pi/5)
        const V a1 = a[1] + a[4], b1 = a[1] - a[4], a2 = a[2] + a[3], b2 = a[2] - a[3];
        const V r1 = a[0] + a1 * (S)c1 + a2 * (S)c2, r2 = a[0] + a1 * (S)c2 + a2 * (S)c1;
        const V u1 = vrot<INV>(b1 * (S)s1 + b2 * (S)s2), u2 = vrot<INV>(b1 * (S)s2 - b2 * (S)s1);
        a[0] = a[0] + a1 + a2;
        a[1] = r1 + u1;
        a[4] = r1 - u1;
        a[2] = r2 + u2;
        a[3] = r2 - u2;
    }
};
// Good-Thomas prime-factor DFT of N = N1 N2 (coprime), no internal twiddles: input n =
// (N2 n1 + N1 n2) mod N, output k = (N2 (N2^-1 mod N1) k1 + N1 (N1^-1 mod N2) k2) mod N.
constexpr int inv_mod(int a, int m) {
    for (int x = 1; x < m; ++x)
        if ((a * x) % m == 1) return x;
    return 1;
}
template <int N1, int N2, bool INV, class V>
__device__ __forceinline__ void dft_pfa(V* a) {
    constexpr int N = N1 * N2;
    V y[N1][N2];
#pragma unroll
    for (int n1 = 0; n1 < N1; ++n1) {
#pragma unroll
        for (int n2 = 0; n2 < N2; ++n2) y[n1][n2] = a[(N2 * n1 + N1 * n2) % N];
        Dft<N2, INV, V>::run(y[n1]);
    }
#pragma unroll
    for (int k2 = 0; k2 < N2; ++k2) {
        V c[N1];
#pragma unroll
        for (int n1 = 0; n1 < N1; ++n1) c[n1] = y[n1][k2];
        Dft<N1, INV, V>::run(c);
#pragma unroll
        for (int k1 = 0; k1 < N1; ++k1)
            a[(N2 * inv_mod(N2 % N1, N1) * k1 + N1 * inv_mod(N1 % N2, N2) * k2) % N] = c[k1];
    }
}
template <bool INV, class V> struct Dft<10, INV, V> {
    static __device__ __forceinline__ void run(V* a) { dft_pfa<2, 5, INV>(a); }
};
template <bool INV, class V> struct Dft<12, INV, V> {
    static __device__ __forceinline__ void run(V* a) { dft_pfa<4, 3, INV>(a); }
};

// LDS index inside a row: SH > 0 inserts one complex every 2^SH to break power-of-two
// strides (tools/ab/lds_conflicts.py models the gfx950 bank rules for each pass).
template <int SH>
__device__ __forceinline__ int lidx(int i) { return SH ? i + (i >> SH) : i; }

// Store policies for the Stockham pass output.  put(idx, row, o, loff, x): idx = t * R + r for
// butterfly t / element r of this thread (a constant after unrolling), row, natural position
// o, and the padded LDS offset loff of (row, o).
template <class V>
struct StoreLds {
    V* buf;
    __device__ __forceinline__ void put(int, int, int, int loff, V x) const { buf[loff] = x; }
};
// A pass whose output goes back into the LDS rows it reads needs the read/write barrier; one
// that stores to global memory (the FFT's last pass into z or the RDM) does not.
template <class St> struct StoresLds { static constexpr bool value = false; };
template <class V> struct StoresLds<StoreLds<V>> { static constexpr bool value = true; };

// Twiddles w[r] = W_{Ns R}^{k r}, r = 1..R-1, of one butterfly (conjugated for the inverse)
// from this pass's table: CMP = false: full rows [k][r-1] (R-1 loads, twk = row k); CMP = true:
// compact columns [i][k] = W^(k 2^i) (lgR loads, twk = table + k, column stride NS), the other
// powers formed as products of at most lgR - 1 of them.  Column-major so that the lanes of a
// pass (consecutive k) read consecutive 16-B entries: conflict-free, where [k][i] rows of 4
// entries put every 4th lane on the same banks (tools/ab/lds_conflicts_k2v2.py).
// The compact form in two steps, so that a pass's table entries can be fetched ahead of the pass
// (k2_fft_job_mix): tw_fetch loads the bases W^(k 2^i), 2^i < R, as the table holds them; tw_expand
// conjugates them for the inverse and forms the other powers.
template <int R, int NS, class V, class TW>
__device__ __forceinline__ void tw_fetch(const TW& twk, V (&b)[tw_row(R, true)]) {
#pragma unroll
    for (int i = 0; i < tw_row(R, true); ++i) b[i] = twk[i * NS];
}
template <int R, bool INV, class V>
__device__ __forceinline__ void tw_expand(const V (&b)[tw_row(R, true)], V (&w)[R]) {
#pragma unroll
    for (int r = 1; r < R; ++r) {
        const int hb = 1 << clog2(r);
        const V t = b[clog2(r)];
        w[r] = (hb == r) ? V{t.x, INV ? -t.y : t.y} : vmul(w[hb], w[r - hb]);
    }
}
template <int R, bool INV, bool CMP, int NS, class V, class TW>
__device__ __forceinline__ void load_tw(const TW& twk, V (&w)[R]) {
    if constexpr (!CMP) {
#pragma unroll
        for (int r = 1; r < R; ++r) {
            const V t = twk[r - 1];
            w[r] = V{t.x, INV ? -t.y : t.y};
        }
    } else {
        V b[tw_row(R, true)];   // lgR bases (= log2 R for powers of two)
        tw_fetch<R, NS>(twk, b);
        tw_expand<R, INV>(b, w);
    }
}

// When the padded LDS offset of element i + r D, r < R, of a row splits into the thread's base
// lidx(i) plus the compile-time lidx_off(r) (a ds_read/ds_write immediate offset), for a base with
// i mod (D R) < D.  sh_load's i = j < nb = D and sh_store's i = idxD = (j / Ns) Ns R + j mod Ns with
// D = Ns are such bases.  With p = 2^SH the pad period, lidx(i + r D) - lidx(i) = r D + ((i + r D) >> SH)
// - (i >> SH), and ((i + r D) >> SH) = (i >> SH) + ((r D) >> SH):
//  - SH = 0: no pads;
//  - p | D: r D is whole pad periods;
//  - D | p and p | D R: i mod p = (i mod D R) mod p < D, and r D mod p is a multiple of D, so at most
//    p - D: the sum does not carry past p;
//  - D | p and D R | p: i and i + r D lie in one aligned group of D R elements (i mod D R + r D < D R),
//    which no multiple of p splits, and r D < p.
// Powers of two D, R always meet one of them; of the 2560-point block's passes, all but the
// unpadded rows' (SH = 30), whose addresses go through lidx element by element.
template <int SH, int D, int R>
constexpr bool lidx_sep() {
    constexpr int p = 1 << SH;
    return SH == 0 || D % p == 0 || (p % D == 0 && ((D * R) % p == 0 || p % (D * R) == 0));
}
template <int SH, int D>
constexpr int lidx_off(int r) {
    return r * D + (SH ? (r * D) >> SH : 0);
}

// One Stockham radix-R pass (Govindaraju et al. formulation) over `nrows` rows of length L held
// in LDS (row stride rs).  Ns = product of the earlier radices.  Reads stride nb = L / R, twiddle
// W_{Ns R}^{(j mod Ns) r} (from this pass's table), radix-R DFT, writes positions
// expand(j, Ns, R) + r Ns.  In place: all reads, barrier, all writes, barrier.  L, R and Ns are
// compile-time constants that need not be powers of two (divisions by them become shifts or
// multiply-shifts), so a pass is straight-line code and no address math is carried across passes.
// tix = the thread's index in the workgroup.
template <int R, bool INV, int NB, int SH, int NTHR, int L, int NS, bool CMP = false, int XL = 0, class V, class TW>
__device__ __forceinline__ void sh_load(const V* buf, int rs, int nrows, const TW& tw, V (&v)[NB][R],
                                        int tix = threadIdx.x) {
    constexpr int nb = L / R;
    static_assert(!XL || nb % 128 == 0, "XOR-swizzled input needs r nb to keep the swizzle bits");
    constexpr bool SEP = lidx_sep<SH, nb, R>();
    const int total = nb * nrows;
#pragma unroll
    for (int t = 0; t < NB; ++t) {
        const int beta = tix + t * NTHR;
        if (beta < total) {
            const int row = beta / nb, j = beta - row * nb;
            const V* src = XL ? buf + row * L + (j ^ ((j >> 4) & 7)) : buf + row * rs + (SEP ? lidx<SH>(j) : 0);
            V w[R];
            if (NS > 1) load_tw<R, INV, CMP, NS>(tw + (CMP ? j % NS : (j % NS) * tw_row(R, CMP)), w);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                V x = XL ? src[r * nb] : (SEP ? src[lidx_off<SH, nb>(r)] : src[lidx<SH>(j + r * nb)]);
                if (r > 0 && NS > 1) x = vmul(x, w[r]);
                v[t][r] = x;
            }
        }
    }
}

// The same pass in two steps (compact tables): sh_tw_fetch loads the table entries of this thread's
// butterflies, sh_load_pf reads the rows and applies them.  The entries depend on the thread's index
// alone, so the fetch can go out a pass ahead and its L2 round trip is over when the pass's LDS
// reads return; NB x lgR complex registers stay live in between.
template <int R, int NB, int NTHR, int L, int NS, class V, class TW>
__device__ __forceinline__ void sh_tw_fetch(int nrows, const TW& tw, V (&b)[NB][tw_row(R, true)], int tix = threadIdx.x) {
    constexpr int nb = L / R;
    static_assert(NS > 1, "a pass with twiddles");
    const int total = nb * nrows;
#pragma unroll
    for (int t = 0; t < NB; ++t) {
        const int beta = tix + t * NTHR;
        if (beta < total) tw_fetch<R, NS>(tw + (beta % nb) % NS, b[t]);
    }
}
template <int R, bool INV, int NB, int SH, int NTHR, int L, int NS, int XL = 0, class V>
__device__ __forceinline__ void sh_load_pf(const V* buf, int rs, int nrows, const V (&b)[NB][tw_row(R, true)],
                                           V (&v)[NB][R], int tix = threadIdx.x) {
    constexpr int nb = L / R;
    static_assert(!XL || nb % 128 == 0, "XOR-swizzled input needs r nb to keep the swizzle bits");
    constexpr bool SEP = lidx_sep<SH, nb, R>();
    const int total = nb * nrows;
#pragma unroll
    for (int t = 0; t < NB; ++t) {
        const int beta = tix + t * NTHR;
        if (beta < total) {
            const int row = beta / nb, j = beta - row * nb;
            const V* src = XL ? buf + row * L + (j ^ ((j >> 4) & 7)) : buf + row * rs + (SEP ? lidx<SH>(j) : 0);
            V w[R];
            tw_expand<R, INV>(b[t], w);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                V x = XL ? src[r * nb] : (SEP ? src[lidx_off<SH, nb>(r)] : src[lidx<SH>(j + r * nb)]);
                if (r > 0) x = vmul(x, w[r]);
                v[t][r] = x;
            }
        }
    }
}

// Radix-R DFT of the loaded butterflies and the Stockham store (through policy st).
// XL = 1: the output is stored XOR-swizzled, element i at (i ^ ((i >> 4) & 7)) of a row of L
// (Ns = 1 radix-16 passes only).  Their stores write 16 j + r for lane j, which the pad layout
// puts 2-way on the banks of every group of 8 lanes; swizzled, the 8 lanes hit 8 distinct
// 16-B banks, and the next pass's reads (j + r nb, nb a multiple of 128) stay conflict-free.
template <int R, bool INV, int NB, int SH, int NTHR, int L, int NS, int XL = 0, class V, class St>
__device__ __forceinline__ void sh_store(V (&v)[NB][R], int rs, int nrows, const St& st, int tix = threadIdx.x) {
    constexpr int nb = L / R;
    static_assert(!XL || (NS == 1 && R == 16), "XOR-swizzled output: Ns = 1 radix-16 passes");
    const int total = nb * nrows;
#pragma unroll
    for (int t = 0; t < NB; ++t) {
        const int beta = tix + t * NTHR;
        if (beta < total) {
            const int row = beta / nb, j = beta - row * nb;
            Dft<R, INV, V>::run(v[t]);
            const int idxD = (j / NS) * (NS * R) + j % NS;
            if constexpr (XL) {
                const int wbase = row * L + idxD, c = j & 7;
#pragma unroll
                for (int r = 0; r < R; ++r) st.put(t * R + r, row, idxD + r, wbase + (r & 8) + ((r & 7) ^ c), v[t][r]);
            } else if constexpr (lidx_sep<SH, NS, R>()) {
                const int wbase = row * rs + lidx<SH>(idxD);
#pragma unroll
                for (int r = 0; r < R; ++r) st.put(t * R + r, row, idxD + r * NS, wbase + lidx_off<SH, NS>(r), v[t][r]);
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r)
                    st.put(t * R + r, row, idxD + r * NS, row * rs + lidx<SH>(idxD + r * NS), v[t][r]);
            }
        }
    }
}

// The read/write barrier only when the store policy writes the LDS rows the pass reads.
// TAIL = false: no barrier after the pass (the caller's next LDS writes go to other rows).
template <int R, bool INV, int NB, int SH, int NTHR, int L, int NS, bool CMP, int XL = 0, bool TAIL = true, class V,
          class TW, class St>
__device__ __forceinline__ void sh_pass(V* buf, int rs, int nrows, const TW& tw, const St& st) {
    V v[NB][R];
    sh_load<R, INV, NB, SH, NTHR, L, NS, CMP, XL>(buf, rs, nrows, tw, v);
    if constexpr (StoresLds<St>::value) __syncthreads();   // every read of the pass before any write
    sh_store<R, INV, NB, SH, NTHR, L, NS>(v, rs, nrows, st);
    if constexpr (TAIL) __syncthreads();
}

// Passes Q..QEND-1 of radix plan Plan (rsp_geometry.h) over `nrows` rows; the plan's last pass
// stores through `last` (TAIL: followed by a barrier), the others through `mid`.  tw = the plan's
// concatenated tables.  PTS = complex points per thread (nrows * L / NTHR).  XIN: the first of
// these passes reads XOR-swizzled rows.
template <class Plan, int Q, int QEND, int PTS, bool INV, int SH, int NTHR, bool CMP, int XIN = 0, bool TAIL = true,
          class V, class TW, class StMid, class StLast>
__device__ __forceinline__ void fft_range(V* buf, int rs, int nrows, const TW& tw, const StMid& mid, const StLast& last) {
    if constexpr (Q < QEND) {
        constexpr int R = Plan::p.rad[Q], L = plan_len(Plan::p), NS = plan_ns(Plan::p, Q);
        constexpr int NB = (PTS + R - 1) / R, TWQ = plan_tw_off(Plan::p, Q, CMP);
        const auto twq = tw + TWQ;
        if constexpr (Q == Plan::p.np - 1)
            sh_pass<R, INV, NB, SH, NTHR, L, NS, CMP, XIN, TAIL>(buf, rs, nrows, twq, last);
        else
            sh_pass<R, INV, NB, SH, NTHR, L, NS, CMP, XIN>(buf, rs, nrows, twq, mid);
        fft_range<Plan, Q + 1, QEND, PTS, INV, SH, NTHR, CMP, 0, TAIL>(buf, rs, nrows, tw, mid, last);
    }
}

// All passes of a 2^LG-point FFT over `nrows` rows.
template <int LG, int PTS, int SH, int NTHR, bool TAIL = true, class V, class StMid, class StLast>
__device__ __forceinline__ void fft_passes(V* buf, int rs, int nrows, const V* tw, const StMid& mid,
                                           const StLast& last) {
    fft_range<PlanPow2<LG>, 0, PlanPow2<LG>::p.np, PTS, false, SH, NTHR, false, 0, TAIL>(buf, rs, nrows, tw, mid, last);
}

// Bin v (after fftshift: frequency v - P/2 mod P) of the direct O(P^2) DFT of col[0 .. P), the
// index into twP = W_P^i walked mod P.
template <class V>
__device__ __forceinline__ V dft_bin(const V* col, const V* twP, int P, int v) {
    int kk = v - (P >> 1);
    if (kk < 0) kk += P;
    V acc = V{};
    int idx = 0;
    for (int p = 0; p < P; ++p) {
        acc += vmul(col[p], twP[idx]);
        idx += kk;
        if (idx >= P) idx -= P;
    }
    return acc;
}

}  // namespace
