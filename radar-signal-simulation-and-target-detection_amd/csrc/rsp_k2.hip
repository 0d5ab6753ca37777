// rsp_k2.hip -- K2 of the per-frame radar chain for CDNA4 (gfx950), and its launchers.
//
//   k2_pc       : pulse compression along fast time of every (beam, Doppler) row
//                 (fsf:101-126): direct FIR for the narrow segment, overlap-save FFT
//                 (Stockham radix-16/8/4/2 in LDS) for medium/long, gate stitching
//                 fused into the output store -> RDM [B][P][G] + |RDM|.
//
// Reads the z rows K1 wrote (rsp_k1.hip); K3 (rsp_k3.hip) reads the magnitude maps.
#include "rsp_device.h"
#include "rsp_fft_passes.h"
#include "rsp_cmag.h"

namespace {

// Diagnostic builds (-DRSP_DEBUG_KNOBS) only: K2 phase stamps.  Workgroup (f, x) of a k2_pc
// launch writes s_memrealtime (100 MHz) at its phase boundaries into rsp_k2_trace[(f G + x) 8 +
// i], i < 6, plus its job type [6] and hardware position (HW_ID | XCC_ID << 32) [7]
// (tools/ab/k2_phases.py).  The shipped library has neither the variable nor the stamps.
#ifdef RSP_DEBUG_KNOBS
__device__ unsigned long long* rsp_k2_trace;
#define K2_STAMP(i)                                                                                     \
    do {                                                                                                \
        if (rsp_k2_trace && threadIdx.x == 0)                                                           \
            rsp_k2_trace[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 8 + (i)] = wall_clock64();    \
    } while (0)
#define K2_TAG(v)                                                                                       \
    do {                                                                                                \
        if (rsp_k2_trace && threadIdx.x == 0) {                                                         \
            unsigned long long* t_ = rsp_k2_trace + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 8;  \
            t_[6] = (v);                                                                                \
            t_[7] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) |                     \
                    ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32);             \
        }                                                                                               \
    } while (0)
extern "C" int rsp_debug_set_k2_trace(unsigned long long* p) {
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(rsp_k2_trace), &p, sizeof(p));
}
#else
#define K2_STAMP(i) ((void)0)
#define K2_TAG(v) ((void)0)
#endif

// ======================================================================================
// K2: pulse compression of every row (fsf:101-126)
// ======================================================================================
template <class V>
struct StoreRdm {   // last inverse pass: keep outputs i in [Lh-1, Lh-1+V) that map to gates < gend;
                    // also writes |x| (the CFAR input, fsf:184-185) into the magnitude map.
                    // Branch-free: rejected outputs get an out-of-range buffer offset.
    __amdgpu_buffer_rsrc_t rdm, mag; int G; int Gp; int row0; K2Rows rw; int P; int Lh1; int g0; int gend; bool has_rdm;
    __device__ __forceinline__ void put(int, int row, int o, int, V x) const {
        const int gg = g0 + o - Lh1;
        const int rho = k2_rho(rw, P, row0 + row);
        const bool ok = o >= Lh1 && gg < gend && row0 + row < rw.total;
        if (has_rdm) buf_st<RSP_RDM_AUX>(rdm, ok ? (unsigned)(rho * G + gg) * (unsigned)sizeof(V) : RSP_OOB, x);
        buf_st1(mag, ok ? (unsigned)(rho * Gp + gg) * (unsigned)sizeof(scal<V>) : RSP_OOB, cmag(x));
    }
};
// The same for a pass whose output rows are uniform per wave (or per workgroup): the row's
// resources are built once, before the pass, by the caller; RDM (compile-time) says whether the
// complex map is stored.  The pass is the overlap-save block's last inverse pass with nb = NS
// butterflies per row: thread j's output r is o = j + r NS, so the outputs r < rskip =
// floor(Lh1 / NS) lie below Lh1 -- discarded overlap-save outputs -- for every thread, and their
// |x| and stores are skipped (a uniform branch; only checked for r < R / 2, where they can be).
template <class V, bool RDM, int NS, int R>
struct StoreRowK {
    typedef scal<V> S;
    __amdgpu_buffer_rsrc_t rr, mr;
    unsigned lh1v, lh1s;   // Lh1 in bytes of V / of S
    int rskip;
    // rho: the row's index in the maps (k2_rho); valid: the row exists (its set index < the set's total)
    __device__ __forceinline__ StoreRowK(V* rdm, S* mag, int G, int Gp, int rho, bool valid, int Lh1, int g0,
                                         int gend) {
        const unsigned n = valid ? (unsigned)(gend - g0) : 0u;
        if (RDM) rr = buf_rsrc(rdm + (size_t)rho * G + g0, n * (unsigned)sizeof(V));
        mr = buf_rsrc(mag + (size_t)rho * Gp + g0, n * (unsigned)sizeof(S));
        lh1v = (unsigned)Lh1 * (unsigned)sizeof(V);
        lh1s = (unsigned)Lh1 * (unsigned)sizeof(S);
        rskip = Lh1 / NS;
    }
    __device__ __forceinline__ void put(int idx, int, int o, int, V x) const {
        const int r = idx % R;
        if (r < R / 2 && r < rskip) return;
        // The masked outputs rely on the wrapped offset being past num_records.  Left visible,
        // (o - Lh1) size = j size - Lh1 size + r NS size is split by the compiler into a wrapped
        // VGPR offset plus an immediate r NS size, and the range check of that sum is not the
        // modular one: the first kept gate of a block was dropped (complex single, maps without
        // the RDM).  The opaque offset keeps the whole (wrapped) value in the VGPR.
        unsigned ov = (unsigned)o * (unsigned)sizeof(V) - lh1v, os = (unsigned)o * (unsigned)sizeof(S) - lh1s;
        asm volatile("" : "+v"(ov), "+v"(os));
        if (RDM) buf_st<RSP_RDM_AUX>(rr, ov, x);
        buf_st1(mr, os, cmag(x));
    }
};

// Samples [lo, hi] of row (b, v) of one segment as one buffer window: z's element index is
// increasing in the compacted sample n' (tile-major, slot-minor), so a resource based at
// n' = off (sample lo) that spans n' = off + hi - lo masks every sample outside [lo, hi] --
// below wraps past num_records, above is past it.  rel(n') = the byte offset of n' in the
// window (may wrap); zrow_window() returns the resource of row i of the launch's row set
// (num_records 0 for rows past rows_total, which are uniform per wave here).
struct ZWin {
    __amdgpu_buffer_rsrc_t r;
    int e_lo, PNT, lgNT, NT1;
    __device__ __forceinline__ int rel(int np) const { return (np >> lgNT) * PNT + (np & NT1) - e_lo; }
};
template <class V>
__device__ __forceinline__ ZWin zrow_window(const Geometry& g, const K2Rows& rw, const V* z, int i, int rows_total,
                                            int off, int lo, int hi) {
    ZWin w;
    const int rho = k2_rho(rw, g.P, i);
    const int b = rho / g.P, v = rho - b * g.P;
    w.lgNT = ilog2(g.NZ);
    w.NT1 = g.NZ - 1;
    w.PNT = g.P * g.NZ;
    const int nph = off + hi - lo;
    w.e_lo = (off >> w.lgNT) * w.PNT + (off & w.NT1);
    const int e_hi = (nph >> w.lgNT) * w.PNT + (nph & w.NT1);
    const V* base = z + ((size_t)b * g.nzc * g.P + v) * g.NZ + w.e_lo;
    w.r = buf_rsrc(base, i < rows_total ? (unsigned)(e_hi - w.e_lo + 1) * (unsigned)sizeof(V) : 0u);
    return w;
}
// The R0 samples n' = np0 + r NB0, r < R0, of one pass-0 butterfly through its row's window zw (a
// scalar buffer resource, uniform per wave: a load's offset needs no mask).
template <int NB0, int R0, class V>
__device__ __forceinline__ void k2_load_wrow(const Geometry& g, const ZWin& zw, int np0, V (&v)[R0]) {
    if ((NB0 & (g.NZ - 1)) == 0) {   // uniform: element r sits r (NB0 P) past element 0
        const unsigned e0 = (unsigned)zw.rel(np0) * (unsigned)sizeof(V), st = (unsigned)(NB0 * g.P) * (unsigned)sizeof(V);
#pragma unroll
        for (int r = 0; r < R0; ++r) v[r] = buf_ld<V>(zw.r, e0 + r * st);
    } else {
#pragma unroll
        for (int r = 0; r < R0; ++r) v[r] = buf_ld<V>(zw.r, (unsigned)zw.rel(np0 + r * NB0) * (unsigned)sizeof(V));
    }
}

// LDS pad of the overlap-save rows: one complex per 32.  For 16-B elements this keeps every
// ds_read_b128 of a pass conflict-free (a pad per 16 would shift lanes 20-27 of a lane group
// onto lane 12's bank), and the stride-16 stores of the two radix-16 Ns = 1 passes 2-way
// (tools/ab/lds_conflicts64.py)
template <class T> constexpr int k2_sh() { return RSP_K2_SH; }
// The 2560-point-sized workgroups (k2_pc<double, 4>): rows without pads and twiddles read from
// L1/L2, so that a workgroup's LDS is the 2560 complex doubles of its row alone (40 KB) and 4 fit a
// CU; SH = 30 makes every pad expression zero.  Measured against 3 per CU with pads and staged
// twiddles: k2_pc -3 % at x2 (profiles/r06zf_k2_w4_ab.txt)
constexpr int K2_NOPAD_SH = 30;
template <class T, bool NOPAD> constexpr int k2_sh_np() { return NOPAD ? K2_NOPAD_SH : k2_sh<T>(); }
// LDS complex slots of a workgroup's rows, pts points (Geometry::k2_pts) + their pads: k2_lds_data
// (rsp_geometry.h)

// The block's twiddle tables are staged in LDS next to the rows: a pass's twiddles then arrive
// with its LDS data reads instead of after an L2 round trip (-6% for k2_pc in complex double).
// When the radix plan is a palindrome the inverse plan's table equals the forward one (the
// conjugation happens in load_tw), so one copy serves both.
constexpr int k2_tw_lds(RadixPlan p) {
    return plan_tw_total(p, true) + (plan_is_palindrome(p) ? 0 : plan_tw_total(plan_rev(p), true));
}
constexpr int k2_tw_lds_max() {   // over the blocks whose tables are staged: 64 .. 2048 and 2560
    int m = k2_tw_lds(plan_os_2560());
    for (int lg = 6; lg <= 11; ++lg) m = k2_tw_lds(plan_os_pow2(lg)) > m ? k2_tw_lds(plan_os_pow2(lg)) : m;
    return m;
}

// The kept overlap-save outputs of `rows` rows from LDS (in natural order after the inverse FFT's
// last pass) to the maps: output o = Lh1 + e is stitched gate g0 + e (fsf:123-126); |x| into the
// magnitude map (the CFAR input, fsf:184-185) and, when the frame's RD map is requested, x into
// it.  Consecutive lanes take consecutive gates (coalesced, conflict-free LDS reads), and the
// square roots run a few at a time instead of 16 per thread at once at the end of the last pass:
// that pass was k2_pc's register peak (188 VGPRs; with this epilogue 3 workgroups fit per CU).
//
// A trip takes U gates per lane, K2_THREADS apart: its U LDS reads go out together, the U
// independent magnitude chains (v_rsq_f64 and its refinement, rsp_cmag.h) interleave, then the
// stores.  One gate per trip left every read and every chain of a lane waiting for the one before
// it: eight serial trips for the 2560-point block's 1 860 gates, now two.  Branch-free: a lane past
// the kept gates reads the last one (inside the row) and its stores fall outside the buffer
// resources' range.
template <class T, int SH, int U, bool RDM>
__device__ __forceinline__ void k2_epi_trip(const cx<T>* src, int pad0, int e0, int nkeep, __amdgpu_buffer_rsrc_t rr,
                                            __amdgpu_buffer_rsrc_t mr) {
    typedef cx<T> V;
    V x[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = min(e0 + u * K2_THREADS, nkeep - 1);
        x[u] = src[i + (SH ? ((pad0 + i) >> SH) : 0)];
    }
    T m[U];
#pragma unroll
    for (int u = 0; u < U; ++u) m[u] = cmag(x[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const unsigned e = (unsigned)(e0 + u * K2_THREADS);
        if (RDM) buf_st<RSP_RDM_AUX>(rr, e * (unsigned)sizeof(V), x[u]);
        buf_st1(mr, e * (unsigned)sizeof(T), m[u]);
    }
}
template <class T, int SH, bool RDM>
__device__ __forceinline__ void k2_epi_row(const cx<T>* src, int pad0, int nkeep, __amdgpu_buffer_rsrc_t rr,
                                           __amdgpu_buffer_rsrc_t mr) {
    constexpr int U = 4;
    int e0 = threadIdx.x, left = nkeep;   // left: uniform
    for (; left > (U - 1) * K2_THREADS; left -= U * K2_THREADS, e0 += U * K2_THREADS)
        k2_epi_trip<T, SH, U, RDM>(src, pad0, e0, nkeep, rr, mr);
    // the remainder in one trip of the fewest gates per lane that cover it
    if (left > 2 * K2_THREADS)
        k2_epi_trip<T, SH, 3, RDM>(src, pad0, e0, nkeep, rr, mr);
    else if (left > K2_THREADS)
        k2_epi_trip<T, SH, 2, RDM>(src, pad0, e0, nkeep, rr, mr);
    else if (left > 0)
        k2_epi_trip<T, SH, 1, RDM>(src, pad0, e0, nkeep, rr, mr);
}
template <class T, int SH>
__device__ __forceinline__ void k2_epilogue(const cx<T>* L, int rs, int rows, int row0, const K2Rows& rw, int P, int Lh1,
                                            int g0, int gend, cx<T>* __restrict__ rdm, T* __restrict__ mag, int G,
                                            int Gp) {
    typedef cx<T> V;
    const int nkeep = gend - g0;
    for (int r = 0; r < rows; ++r) {
        if (row0 + r >= rw.total) break;
        const int rho = k2_rho(rw, P, row0 + r);   // uniform
        const V* src = L + r * rs + Lh1;
        const int pad0 = SH ? Lh1 : 0;
        const __amdgpu_buffer_rsrc_t mr = buf_rsrc(mag + (size_t)rho * Gp + g0, (unsigned)nkeep * (unsigned)sizeof(T));
        if (rdm) {
            const __amdgpu_buffer_rsrc_t rr = buf_rsrc(rdm + (size_t)rho * G + g0, (unsigned)nkeep * (unsigned)sizeof(V));
            k2_epi_row<T, SH, true>(src, pad0, nkeep, rr, mr);
        } else {
            k2_epi_row<T, SH, false>(src, pad0, nkeep, mr, mr);
        }
    }
}

// x[r] *= H[j + r S] (the filter spectrum, 1/M folded in) for the fused pass's R outputs, loaded
// after the forward DFT that produces them: H then occupies registers only from here to the
// product (an empty asm keeps the loads below the DFT; loaded with the samples it held 64 VGPRs
// of complex double through the whole forward FFT)
template <int R, int S, class V>
__device__ __forceinline__ void k2_apply_h(V (&x)[R], __amdgpu_buffer_rsrc_t hr, int j) {
    asm volatile("" ::: "memory");
    V h[R];
#pragma unroll
    for (int r = 0; r < R; ++r) h[r] = buf_ld<V>(hr, (unsigned)(j + r * S) * (unsigned)sizeof(V));
#pragma unroll
    for (int r = 0; r < R; ++r) x[r] = vmul(x[r], h[r]);
}

// One overlap-save block of one FFT segment for PTS / 2^LGM adjacent rows (PTS = 4096, or 2048
// in a plan whose workgroups are sized for the 2560-point block, Geometry::k2_pts).
// LDS round trips: forward pass 0 runs on the samples as loaded from z; the forward FFT's
// last pass, the filter-spectrum product and the inverse FFT's first pass (radices in
// reverse order, so that pass has the same butterflies) run in registers back to back;
// the inverse FFT's last pass stores the kept gates to HBM.  2 (log2 M / 4) round trips
// instead of 2 (log2 M / 4) + 3.  Twiddles are compact rows, staged in LDS.
// The twiddle source of a K2 job: the LDS copy, or the plan's table in global memory through a
// buffer resource (TwG; x4 k2_pc 2.355 -> 2.347 ms against 64-bit addresses, r06zg)
template <bool LDS, class V>
__device__ __forceinline__ auto k2_tw_src(const V* lds, const V* glob) {
    if constexpr (LDS)
        return lds;
    else
        return TwG<V>{buf_rsrc(glob, RSP_OOB), 0u};
}
template <class T, int LGM, int PTS, bool EPI, bool NOPAD>
__device__ __forceinline__ void k2_fft_job(const Geometry& g, const DevConsts& k, const SegDesc& sd, const K2Job& job,
                                           const cx<T>* __restrict__ z, cx<T>* __restrict__ rdm, T* __restrict__ mag,
                                           int row0, const K2Rows& rw, cx<T>* L) {
    const int rows_total = rw.total;
    typedef cx<T> V;
    constexpr int SH = k2_sh_np<T, NOPAD>();
    constexpr int M = 1 << LGM;
    constexpr int rows = PTS / M > 0 ? PTS / M : 1;
    constexpr int rs = M + (M >> SH);
    typedef PlanOs<M> Plan;
    typedef PlanRev<Plan> PlanI;   // the inverse FFT's
    constexpr int NP = Plan::p.np;
    static_assert(NP >= 2, "overlap-save block needs >= 2 FFT passes");
    constexpr bool CMP = true;
    constexpr int R0 = Plan::p.rad[0], NB0 = 16 / R0, nb0 = M / R0;
    constexpr int RL = Plan::p.rad[NP - 1], NBL = 16 / RL;   // last forward pass
    constexpr int TWL = plan_tw_off(Plan::p, NP - 1, CMP), TWIL = plan_tw_off(PlanI::p, NP - 1, CMP);
    const int P = g.P, G = g.G;
    const int lo = sd.lo, hi = sd.hi, off = sd.off;
    const int tid = threadIdx.x;
    const int Lh1 = sd.Lh - 1;
    const int g0 = sd.ga + job.blk * sd.V;
    const int a = sd.seg_lo + g0 - Lh1;           // sample index of u[0]
    const V* twl = static_cast<const V*>(k.twM) + sd.tw_off;
    const V* __restrict__ H = static_cast<const V*>(k.H);
    // every global load of the workgroup in flight together: the 16 samples of this thread's
    // pass-0 butterflies and its 16 filter-spectrum values (for the fused middle pass)
    V v0[NB0][R0];
    const int lgNT = ilog2(g.NZ);
    // one row per wave (nb0 a multiple of 64, one butterfly per thread): the row's sample window
    // is a scalar buffer resource, and a load's offset needs no mask
    constexpr bool WROW = nb0 >= 64 && NB0 == 1;
    if constexpr (WROW) {
        const int rl = __builtin_amdgcn_readfirstlane(tid / nb0);
        // waves past the block's rows (fewer rows than 256 / nb0) load nothing
        const ZWin zw = zrow_window(g, rw, z, row0 + rl, rl < rows ? rows_total : 0, off, lo, hi);
        k2_load_wrow<nb0>(g, zw, a + (tid & (nb0 - 1)) - lo + off, v0[0]);
    }
    const __amdgpu_buffer_rsrc_t zr = buf_rsrc(z, (unsigned)(g.B * g.nzc * P * g.NZ * sizeof(V)));
#pragma unroll
    for (int t = 0; t < (WROW ? 0 : NB0); ++t) {
        const int beta = tid + t * K2_THREADS;
        const int rl = beta / nb0, j = beta & (nb0 - 1);
        const int ri = row0 + rl, rho = k2_rho(rw, P, ri);
        const int b = rho / P, v = rho - b * P;
        // z index of sample n0 + r nb0: when NT | nb0 the tile advances by nb0/NT per r and the
        // in-tile slot is fixed, so element r sits at zb + r (nb0 P) (one multiply per thread)
        const int np0 = a + j - lo + off;
        const int zb = ((b * g.nzc + (np0 >> lgNT)) * P + v) * g.NZ + (np0 & (g.NZ - 1));
        // branch-free: every lane loads (an out-of-range offset when masked)
        if ((nb0 & (g.NZ - 1)) == 0) {   // uniform
#pragma unroll
            for (int r = 0; r < R0; ++r) {
                const int n = a + j + r * nb0;
                const bool ok = ri < rows_total && n >= lo && n <= hi;
                v0[t][r] = buf_ld<V>(zr, ok ? (unsigned)(zb + r * nb0 * P) * (unsigned)sizeof(V) : RSP_OOB);
            }
        } else {
#pragma unroll
            for (int r = 0; r < R0; ++r) {
                const int n = a + j + r * nb0;
                const bool ok = ri < rows_total && n >= lo && n <= hi;
                v0[t][r] = buf_ld<V>(zr, ok ? (unsigned)zaddr(g, b, v, n - lo + off) * (unsigned)sizeof(V) : RSP_OOB);
            }
        }
    }
    const __amdgpu_buffer_rsrc_t hr = buf_rsrc(H + sd.H_off, (unsigned)(M * sizeof(V)));
    // !EPI: H for the last forward pass's outputs j + r M/RL loaded with the samples; butterflies t
    // and t + (M/RL)/NTHR of a thread have the same j (different rows), so only the distinct ones
    constexpr int NHT = !EPI ? ((M / RL) / K2_THREADS >= NBL ? NBL : ((M / RL) / K2_THREADS > 0 ? (M / RL) / K2_THREADS : 1)) : 1;
    V hreg[NHT * RL];
    if constexpr (!EPI) {
#pragma unroll
        for (int t = 0; t < NHT; ++t) {
            const int j = (tid + t * K2_THREADS) & (M / RL - 1);   // last pass: Ns = nb = M / RL, idxD = j
#pragma unroll
            for (int r = 0; r < RL; ++r) hreg[t * RL + r] = buf_ld<V>(hr, (unsigned)(j + r * (M / RL)) * (unsigned)sizeof(V));
        }
    }
    constexpr int NTWF = plan_tw_total(Plan::p, CMP), NTWL = k2_tw_lds(Plan::p);
    // twiddles staged in LDS next to the rows; a 4096-point block's (1 088 entries) do not fit the
    // 2-per-CU workgroup's LDS and are read from L1/L2 instead
    constexpr bool TW_LDS = LGM <= 11 && !NOPAD;
    V* twL = L + k2_lds_data(g.k2_pts, SH);
    if constexpr (TW_LDS) stage_lds<K2_THREADS>(twL, twl, NTWL);   // visible after the pass-0 barrier
    const auto twF = k2_tw_src<TW_LDS, V>(twL, twl);
    constexpr int TWI = plan_is_palindrome(Plan::p) ? 0 : NTWF;   // a palindrome: the forward tables
    const auto twI = twF + TWI;
    // forward pass 0 (Ns = 1, no twiddles) straight from the loaded samples
    // the Ns = 1 passes' outputs XOR-swizzled (sh_store) when a middle pass reads them (3 passes)
    constexpr int XZ = (NP == 3 && R0 == 16 && RL == 16) ? 1 : 0;
    sh_store<R0, false, NB0, SH, K2_THREADS, M, 1, XZ>(v0, rs, rows, StoreLds<V>{L});
    __syncthreads();
    K2_STAMP(1);
    // forward passes 1 .. NP-2
    fft_range<Plan, 1, NP - 1, 16, false, SH, K2_THREADS, CMP, XZ>(L, rs, rows, twF, StoreLds<V>{L}, StoreLds<V>{L});
    // fused: forward last pass, x H (1/M folded in), inverse pass 0 of the reversed plan
    {
        V v[NBL][RL];
        sh_load<RL, false, NBL, SH, K2_THREADS, M, M / RL, CMP>(L, rs, rows, twF + TWL, v);
        __syncthreads();   // every read of the pass before any write
#pragma unroll
        for (int t = 0; t < NBL; ++t) {
            Dft<RL, false, V>::run(v[t]);
            // last forward pass: Ns = nb = M / RL, thread j's outputs j + r M / RL
            if constexpr (EPI) {
                k2_apply_h<RL, M / RL>(v[t], hr, (tid + t * K2_THREADS) & (M / RL - 1));
            } else {
#pragma unroll
                for (int r = 0; r < RL; ++r) v[t][r] = vmul(v[t][r], hreg[(t % NHT) * RL + r]);
            }
        }
        sh_store<RL, true, NBL, SH, K2_THREADS, M, 1, XZ>(v, rs, rows, StoreLds<V>{L});
        __syncthreads();
    }
    K2_STAMP(3);
    const int gend = min(sd.gb, g0 + sd.V);
    if constexpr (EPI) {
        // inverse passes 1 .. NP-1 (reversed radices) into LDS; then the valid overlap-save outputs
        // = stitched gates go to the maps
        fft_range<PlanI, 1, NP, 16, true, SH, K2_THREADS, CMP, XZ>(L, rs, rows, twI, StoreLds<V>{L}, StoreLds<V>{L});
        k2_epilogue<T, SH>(L, rs, rows, row0, rw, P, Lh1, g0, gend, rdm, mag, G, g.Gp);
    } else if constexpr (WROW) {
        // inverse passes 1 .. NP-2 into LDS, then the last one (Ns = nb0, input not swizzled:
        // XZ applies to the pass after an Ns = 1 pass only) stores the kept gates straight into
        // this wave's row of the maps
        fft_range<PlanI, 1, NP - 1, 16, true, SH, K2_THREADS, CMP, XZ>(L, rs, rows, twI, StoreLds<V>{L}, StoreLds<V>{L});
        static_assert(NP >= 3 || XZ == 0, "last pass input is never swizzled");
        const auto twl_last = twI + TWIL;
        const int ri = row0 + __builtin_amdgcn_readfirstlane(tid / nb0), rho = k2_rho(rw, P, ri);
        const bool valid = ri < rows_total;
        if (rdm)
            sh_pass<R0, true, NB0, SH, K2_THREADS, M, nb0, CMP, 0, false>(
                L, rs, rows, twl_last, StoreRowK<V, true, nb0, R0>(rdm, mag, G, g.Gp, rho, valid, Lh1, g0, gend));
        else
            sh_pass<R0, true, NB0, SH, K2_THREADS, M, nb0, CMP, 0, false>(
                L, rs, rows, twl_last, StoreRowK<V, false, nb0, R0>(rdm, mag, G, g.Gp, rho, valid, Lh1, g0, gend));
    } else {
        fft_range<PlanI, 1, NP, 16, true, SH, K2_THREADS, CMP, XZ, false>(
            L, rs, rows, twI, StoreLds<V>{L},
            StoreRdm<V>{buf_rsrc(rdm, (unsigned)(g.B * P * G * sizeof(V))),
                        buf_rsrc(mag, (unsigned)(g.B * P * g.Gp * sizeof(T))), G, g.Gp, row0, rw, P, Lh1, g0, gend,
                        rdm != nullptr});
    }
}

// Mixed-radix overlap-save block M = R0 x R1 x R0, a palindrome: the inverse FFT runs the same
// radices, the fused middle pass (forward last pass, x H, inverse pass 0) has the same
// butterflies on both sides as in k2_fft_job, and the inverse twiddle table equals the forward
// one (conjugated in load_tw).  Two plans:
//  - 2560 = 16 x 10 x 16: one block covers x2's long segment (Lh = 700, 1860 gates), which takes
//    two 2048-point blocks in powers of two -- 37.5% fewer points.  One row per workgroup: the
//    radix-16 passes run 160 butterflies (waves 0-2, the fourth wave skips them), the radix-10
//    passes 256.
//  - 1024 = 8 x 16 x 8 in workgroups sized for 2048 points (the 3-per-CU plans): two rows, and
//    the three Ns = 1 / fused / last passes run 2 x 128 radix-8 butterflies on all 256 threads;
//    as 16 x 4 x 16 those passes ran 2 x 64 radix-16 butterflies on half of them.
template <class T, int M, int R0, int R1, bool EPI, bool NOPAD>
__device__ __forceinline__ void k2_fft_job_mix(const Geometry& g, const DevConsts& k, const SegDesc& sd, const K2Job& job,
                                               const cx<T>* __restrict__ z, cx<T>* __restrict__ rdm, T* __restrict__ mag,
                                               int row0, const K2Rows& rw, cx<T>* L) {
    const int rows_total = rw.total;
    typedef cx<T> V;
    constexpr int SH = k2_sh_np<T, NOPAD>();
    static_assert(M == R0 * R1 * R0, "palindromic 3-pass plan");
    constexpr int rows = M >= 2048 ? 1 : 2048 / M;
    constexpr int rs = M + (M >> SH);
    constexpr bool CMP = true;
    constexpr int nb0 = M / R0;                                          // radix-R0 butterflies per row
    constexpr int NB0 = (nb0 * rows + K2_THREADS - 1) / K2_THREADS;
    constexpr int NB1 = ((M / R1) * rows + K2_THREADS - 1) / K2_THREADS;
    constexpr int NS1 = R0, NS2 = R0 * R1;                               // Ns of passes 1 and 2
    constexpr int TW2 = NS1 * tw_row(R1, CMP);                           // offset of pass 2's table
    constexpr int NTWF = TW2 + NS2 * tw_row(R0, CMP);
    const int G = g.G;
    const int lo = sd.lo, hi = sd.hi, off = sd.off;
    const int tid = threadIdx.x;
    const int Lh1 = sd.Lh - 1;
    const int g0 = sd.ga + job.blk * sd.V;
    const int a = sd.seg_lo + g0 - Lh1;
    const V* twl = static_cast<const V*>(k.twM) + sd.tw_off;
    const V* __restrict__ H = static_cast<const V*>(k.H);
    static_assert(NB0 == 1, "one radix-R0 butterfly per thread");
    static_assert(rows == 1 || nb0 % 64 == 0, "a row per whole wave (its z window is a scalar resource)");
    static_assert(!NOPAD || rows * rs <= 2560, "the row alone fills the 4-per-CU workgroup's LDS");
    static_assert(NOPAD || rows * rs + NTWF <= k2_lds_data(RSP_K2_POINTS, SH) + k2_tw_lds_max(), "fits the 2-per-CU LDS");
    V v0[NB0][R0];
    V hreg[EPI ? 1 : NB0][R0];   // !EPI: the fused pass's H, loaded with the samples
    // threads past the rows' butterflies (waves past them) skip the loads; a row's samples are one
    // scalar buffer window (zrow_window), so the loads need no masks
    const int rl = rows == 1 ? 0 : __builtin_amdgcn_readfirstlane(tid / nb0);
    const int j = tid - rl * nb0;
    if (tid < nb0 * rows) {
        const ZWin zw = zrow_window(g, rw, z, row0 + rl, rows_total, off, lo, hi);
        k2_load_wrow<nb0>(g, zw, a + j - lo + off, v0[0]);
        if constexpr (!EPI) {
            const __amdgpu_buffer_rsrc_t hr = buf_rsrc(H + sd.H_off, (unsigned)(M * sizeof(V)));
#pragma unroll
            for (int r = 0; r < R0; ++r)   // fused pass outputs j + r M/R0
                hreg[0][r] = buf_ld<V>(hr, (unsigned)(j + r * nb0) * (unsigned)sizeof(V));
        }
    }
    V* twL = L + k2_lds_data(g.k2_pts, SH);
    if constexpr (!NOPAD) stage_lds<K2_THREADS>(twL, twl, NTWF);
    const auto twF = k2_tw_src<!NOPAD, V>(twL, twl);
    const auto twI = twF;   // palindrome: the reversed plan's table is the forward one
    constexpr int XZ = R0 == 16 ? 1 : 0;   // Ns = 1 outputs XOR-swizzled (see sh_store)
    // NOPAD (twiddles from L1/L2): a twiddled pass opened with the L2 round trip of its table entries
    // between its barrier and its first butterfly.  Where registers allow, the entries are fetched a
    // pass ahead (sh_tw_fetch): pass 1's go out with the z loads (pass 0 has no twiddles), the inverse
    // last pass's after the inverse radix-R1 pass's twiddle products (R1 < R0: register slack; an
    // empty asm keeps the fetch below that pass's own loads).  The other two -- the fused pass's
    // fetched in forward pass 1, the inverse pass 1's after the H product -- spill (+16 B and +152 B
    // of scratch per lane) and measured slower; they load their entries as they start.
    V b1[NOPAD ? NB1 : 1][tw_row(R1, true)], b2[NOPAD ? NB0 : 1][tw_row(R0, true)];
    if constexpr (NOPAD) sh_tw_fetch<R1, NB1, K2_THREADS, M, NS1>(rows, twF, b1, tid);
    sh_store<R0, false, NB0, SH, K2_THREADS, M, 1, XZ>(v0, rs, rows, StoreLds<V>{L}, tid);
    __syncthreads();
    K2_STAMP(1);
    if constexpr (NOPAD) {
        V v[NB1][R1];
        sh_load_pf<R1, false, NB1, SH, K2_THREADS, M, NS1, XZ>(L, rs, rows, b1, v, tid);
        __syncthreads();   // every read of the pass before any write
        sh_store<R1, false, NB1, SH, K2_THREADS, M, NS1>(v, rs, rows, StoreLds<V>{L}, tid);
        __syncthreads();
    } else {
        sh_pass<R1, false, NB1, SH, K2_THREADS, M, NS1, CMP, XZ>(L, rs, rows, twF, StoreLds<V>{L});
    }
    K2_STAMP(2);
    {
        V v[NB0][R0];
        sh_load<R0, false, NB0, SH, K2_THREADS, M, NS2, CMP>(L, rs, rows, twF + TW2, v, tid);
        __syncthreads();   // every read of the pass before any write
        const __amdgpu_buffer_rsrc_t hr = buf_rsrc(H + sd.H_off, (unsigned)(M * sizeof(V)));
#pragma unroll
        for (int t = 0; t < NB0; ++t) {
            Dft<R0, false, V>::run(v[t]);
            if constexpr (EPI) {
                k2_apply_h<R0, nb0>(v[t], hr, j);   // fused pass outputs j + r M/R0
            } else {
#pragma unroll
                for (int r = 0; r < R0; ++r) v[t][r] = vmul(v[t][r], hreg[t][r]);
            }
        }
        sh_store<R0, true, NB0, SH, K2_THREADS, M, 1, XZ>(v, rs, rows, StoreLds<V>{L}, tid);
        __syncthreads();
    }
    K2_STAMP(3);
    if constexpr (NOPAD) {
        V v[NB1][R1];
        sh_load<R1, true, NB1, SH, K2_THREADS, M, NS1, CMP, XZ>(L, rs, rows, twI, v, tid);
        asm volatile("" ::: "memory");
        sh_tw_fetch<R0, NB0, K2_THREADS, M, NS2>(rows, twI + TW2, b2, tid);
        __syncthreads();   // every read of the pass before any write
        sh_store<R1, true, NB1, SH, K2_THREADS, M, NS1>(v, rs, rows, StoreLds<V>{L}, tid);
        __syncthreads();
    } else {
        sh_pass<R1, true, NB1, SH, K2_THREADS, M, NS1, CMP, XZ>(L, rs, rows, twI, StoreLds<V>{L});
    }
    K2_STAMP(4);
    const int gend = min(sd.gb, g0 + sd.V);
    if constexpr (EPI && NOPAD) {
        V v[NB0][R0];
        sh_load_pf<R0, true, NB0, SH, K2_THREADS, M, NS2>(L, rs, rows, b2, v, tid);
        __syncthreads();   // every read of the pass before any write
        sh_store<R0, true, NB0, SH, K2_THREADS, M, NS2>(v, rs, rows, StoreLds<V>{L}, tid);
        __syncthreads();
        k2_epilogue<T, SH>(L, rs, rows, row0, rw, g.P, Lh1, g0, gend, rdm, mag, G, g.Gp);
    } else if constexpr (EPI) {
        sh_pass<R0, true, NB0, SH, K2_THREADS, M, NS2, CMP>(L, rs, rows, twI + TW2, StoreLds<V>{L});
        k2_epilogue<T, SH>(L, rs, rows, row0, rw, g.P, Lh1, g0, gend, rdm, mag, G, g.Gp);
    } else {
        static_assert(EPI || (rows == 1 && NS2 == nb0), "last pass: thread j's outputs are j + r NS2 of one row");
        V v[NB0][R0];
        sh_load<R0, true, NB0, SH, K2_THREADS, M, NS2, CMP>(L, rs, rows, twI + TW2, v, tid);
        const int rho = k2_rho(rw, g.P, row0);
        if (rdm)
            sh_store<R0, true, NB0, SH, K2_THREADS, M, NS2>(
                v, rs, rows, StoreRowK<V, true, NS2, R0>(rdm, mag, G, g.Gp, rho, row0 < rows_total, Lh1, g0, gend), tid);
        else
            sh_store<R0, true, NB0, SH, K2_THREADS, M, NS2>(
                v, rs, rows, StoreRowK<V, false, NS2, R0>(rdm, mag, G, g.Gp, rho, row0 < rows_total, Lh1, g0, gend), tid);
    }
}

// k2_pc<T, WGS>: sized for WGS workgroups per CU.  WGS = 4 (a complex-double plan with a
// 2560-point block, Geometry::k2_pts = 2560: the row's 40 KB of LDS alone -- no pads, twiddles
// from L1/L2 (NOPAD) -- and 128 VGPRs per lane) runs the blocks with EPI (the filter spectrum loaded
// after the forward DFT, the kept gates stored by k2_epilogue): without them the last pass peaks
// at 188 VGPRs.  (Round 5's 3 per CU with pads and staged twiddles, 53.5 KB: 3 % slower.)
// WGS = 2 (4096-point workgroups, 76 KB of LDS) keeps H in registers from the start and stores
// the gates from the last pass, which measured faster at that occupancy (x2 at 2 per CU: 225 vs
// 248 us per 8 frames).
template <class T, int WGS>
__global__ __launch_bounds__(K2_THREADS, WGS) void k2_pc(Geometry g, DevConsts k, FramePtrs fp, K2Rows rw,
                                                         const K2Rec* __restrict__ recs, int on_demand) {
    constexpr bool EPI = WGS >= 3;
    constexpr bool NOPAD = WGS == 4;
    typedef cx<T> V;
    V* L = reinterpret_cast<V*>(rsp_lds);   // overlap-save rows | narrow: staged rows + taps
    const int f = blockIdx.y;
    // the plan's dispatch order (job kinds interleaved) as one record per workgroup: a single scalar
    // load, where a dispatch-order entry and a search of g.jobs were 3 to 5 dependent ones
    const K2Rec rec = recs[blockIdx.x];
    const K2Job job{rec.seg, rec.blk, 0, 0};   // the block jobs read seg and blk
    const SegDesc& sd = g.segs[rec.seg];
    const int rows = sd.rows_per_wg;
    const int row0 = rec.row0;   // of the launch's row set rw
    const int rows_total = rw.total;
    if (on_demand) {
        // the edge set after K3's first phase: row i's flag is byte i of the frame's block (beam-major,
        // 2 hV per beam, as the set counts its rows).  A workgroup none of whose rows is asked for
        // returns; one with any computes them all, so a row's values never depend on its neighbours'
        // flags.  Uniform: scalar loads and a scalar branch.
        const unsigned char* __restrict__ need = fp.need[f];
        int any = 0;
        for (int r = 0; r < rows && row0 + r < rows_total; ++r) any |= need[row0 + r];
        if (!any) return;
        if (rec.seg == 0 && rec.blk == 0 && threadIdx.x == 0) atomicAdd(fp.count[f] + 2, min(rows, rows_total - row0));
    }
    const V* __restrict__ z = static_cast<const V*>(fp.z[f]);
    V* __restrict__ rdm = static_cast<V*>(fp.rdm[f]);
    T* __restrict__ mag = static_cast<T*>(fp.mag[f]);
    const int P = g.P, G = g.G;
    const int lo = sd.lo, hi = sd.hi, off = sd.off;
    const int tid = threadIdx.x;
    K2_STAMP(0);
    K2_TAG((unsigned long long)(sd.type * 16 + sd.logM));

    if (sd.type == 1 && sd.logM == 0) {   // mixed-radix block
        k2_fft_job_mix<T, 2560, 16, 10, EPI, NOPAD>(g, k, sd, job, z, rdm, mag, row0, rw, L);
    } else if (sd.type == 1) {
        // workgroups sized for the 2560-point block (WGS >= 3) run 2048 points of 2^k rows, up to
        // one 2048-point row; the others RSP_K2_POINTS, up to one 4096-point row
        constexpr int PTS = WGS >= 3 ? 2048 : RSP_K2_POINTS;
        constexpr int LGTOP = WGS >= 3 ? 11 : 12;   // the largest block: the default
        switch (sd.logM) {
            case 6: k2_fft_job<T, 6, PTS, EPI, NOPAD>(g, k, sd, job, z, rdm, mag, row0, rw, L); break;
            case 7: k2_fft_job<T, 7, PTS, EPI, NOPAD>(g, k, sd, job, z, rdm, mag, row0, rw, L); break;
            case 8: k2_fft_job<T, 8, PTS, EPI, NOPAD>(g, k, sd, job, z, rdm, mag, row0, rw, L); break;
            case 9: k2_fft_job<T, 9, PTS, EPI, NOPAD>(g, k, sd, job, z, rdm, mag, row0, rw, L); break;
            case 10: k2_fft_job<T, 10, PTS, EPI, NOPAD>(g, k, sd, job, z, rdm, mag, row0, rw, L); break;
            case 11:
                if constexpr (LGTOP > 11) {
                    k2_fft_job<T, 11, PTS, EPI, NOPAD>(g, k, sd, job, z, rdm, mag, row0, rw, L);
                    break;
                }
                [[fallthrough]];
            default: k2_fft_job<T, LGTOP, PTS, EPI, NOPAD>(g, k, sd, job, z, rdm, mag, row0, rw, L); break;
        }
    } else {
        // direct FIR (narrow segment): filter() + circshift(-fir_delay) (fsf:111-112).  Each
        // staged row carries ntaps - 1 leading zeros (filter()'s zero state / samples before lo),
        // so the tap loop is branch-free.
        const int W = hi - lo + 1;
        const int PADL = sd.ntaps - 1, WP = W + PADL;
        const int nw = rows * WP;
        for (int e0 = 0; e0 < nw; e0 += 16 * K2_THREADS) {
            V val[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int e = e0 + tid + u * K2_THREADS;
                val[u] = V{};
                if (e < nw) {
                    const int rl = e / WP, i = e - rl * WP - PADL;
                    if (row0 + rl < rows_total && i >= 0) {
                        const int rho = k2_rho(rw, P, row0 + rl);
                        const int b = rho / P, v = rho - b * P;
                        val[u] = z[zaddr(g, b, v, i + off)];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int e = e0 + tid + u * K2_THREADS;
                if (e < nw) L[e] = val[u];
            }
        }
        T* tp = reinterpret_cast<T*>(L + nw);   // taps: LDS broadcast reads
        const T* __restrict__ taps = static_cast<const T*>(k.taps);
        for (int e = tid; e < sd.ntaps; e += K2_THREADS) tp[e] = taps[sd.taps_off + e];
        __syncthreads();
        K2_STAMP(1);
        const int nout = sd.gb - sd.ga;
        // 4 consecutive gates per thread: the 4 outputs share a register window that slides one
        // sample per tap (1 LDS read + 4 FMAs per tap); a group whose circshift index wraps
        // mid-group takes the per-gate loop
        const int ngrp = (nout + 3) >> 2;
        for (int e = tid; e < rows * ngrp; e += K2_THREADS) {
            const int rl = e / ngrp, q0 = 4 * (e - rl * ngrp);
            if (row0 + rl >= rows_total) continue;
            const int rho = k2_rho(rw, P, row0 + rl);
            const int gg0 = sd.ga + q0;
            int kk0 = (gg0 + sd.delay) % sd.Ls;
            if (kk0 < 0) kk0 += sd.Ls;
            const V* row = L + rl * WP + PADL - lo + sd.seg_lo;   // row[kk] = x(seg_lo + kk)
            if (q0 + 4 <= nout && kk0 + 3 < sd.Ls) {
                const V* xr = row + kk0;
                V w0 = xr[0], w1 = xr[1], w2 = xr[2], w3 = xr[3];
                T t = tp[0];
                V a0 = t * w0, a1 = t * w1, a2 = t * w2, a3 = t * w3;
#pragma unroll 4
                for (int j = 1; j < sd.ntaps; ++j) {
                    w3 = w2; w2 = w1; w1 = w0;
                    w0 = xr[-j];
                    t = tp[j];
                    a0 += t * w0; a1 += t * w1; a2 += t * w2; a3 += t * w3;
                }
                if (rdm) {
                    V* ro = rdm + (size_t)rho * G + gg0;
                    ro[0] = a0; ro[1] = a1; ro[2] = a2; ro[3] = a3;
                }
                T* mo = mag + (size_t)rho * g.Gp + gg0;
                mo[0] = cmag(a0); mo[1] = cmag(a1); mo[2] = cmag(a2); mo[3] = cmag(a3);
            } else {
                for (int q = 0; q < 4 && q0 + q < nout; ++q) {
                    const int gg = gg0 + q;
                    int kk = (gg + sd.delay) % sd.Ls;
                    if (kk < 0) kk += sd.Ls;
                    const V* xr = row + kk;
                    V acc = V{};
                    for (int j = 0; j < sd.ntaps; ++j) acc += tp[j] * xr[-j];
                    if (rdm) rdm[(size_t)rho * G + gg] = acc;
                    mag[(size_t)rho * g.Gp + gg] = cmag(acc);
                }
            }
        }
    }
    K2_STAMP(5);
}

}  // namespace

template <class T>
static hipError_t launch_k2_p(const Geometry& g, const DevConsts& k, const FramePtrs& fp, int nf, const K2Rows& rows,
                              const K2Rec* recs, int nwg, bool on_demand, hipStream_t s) {
    // workgroups sized for the 2560-point block (complex double): 4 per CU, the row's LDS alone
    const bool w4 = k2_wg_per_cu(g) == 4;
    const size_t lds = w4 ? (size_t)g.k2_pts * sizeof(cx<T>)
                          : (size_t)(k2_lds_data(g.k2_pts, k2_sh<T>()) + k2_tw_lds_max()) * sizeof(cx<T>);
    const auto kernel = w4 ? k2_pc<T, 4> : k2_pc<T, 2>;
    if (nwg == 0) {   // nothing to launch; the LDS attribute is set all the same
        const hipError_t e = allow_lds(kernel, lds);
        return e != hipSuccess ? e : hipGetLastError();
    }
    return launch(kernel, dim3(nwg, nf), dim3(K2_THREADS), lds, s, g, k, fp, rows, recs, on_demand ? 1 : 0);
}

hipError_t launch_k2_set(const Geometry& g, const DevConsts& k, const FramePtrs& fp, int nf, const K2Rows& rows,
                         const K2Rec* recs, int nwg, bool on_demand, hipStream_t s) {
    return g.prec == RSP_PREC_F64 ? launch_k2_p<double>(g, k, fp, nf, rows, recs, nwg, on_demand, s)
                                  : launch_k2_p<float>(g, k, fp, nf, rows, recs, nwg, on_demand, s);
}

hipError_t launch_k2(const Geometry& g, const DevConsts& k, const FramePtrs& fp, int nf, hipStream_t s) {
    return launch_k2_set(g, k, fp, nf, k2_row_set(g, K2SET_ALL), k.k2rec, g.nwg_k2, false, s);
}
