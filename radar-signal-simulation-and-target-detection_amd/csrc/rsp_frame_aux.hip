// rsp_frame_aux.hip -- the frame chain's kernels beside K1, K2 and K3 (gfx950), and their launchers.
//
//   k_mtd_cols     : MTD over pulses of a pulse-compressed cube (stage-2 path).
//   k_synth        : S4 echo synthesis + S4.1 Philox noise (fsf:45-88) on the device.
//   k_dets_to_host : the queue's read-back of the detection lists into pinned host memory.
//   k_stream_copy  : the streaming copy of rsp_hbm_copy_probe.
#include "rsp_device.h"
#include "rsp_fft_passes.h"
#include "rsp_noise_math.h"

namespace {

// ======================================================================================
// MTD over pulses of a pulse-compressed cube pc[B][P][G] -> rdm[B][P][G] (fsf:131-136)
// ======================================================================================
template <class T, int LGP>
__global__ __launch_bounds__(RSP_THREADS, 2) void k_mtd_cols(Geometry g, DevConsts k, const cx<T>* __restrict__ pc,
                                                        cx<T>* __restrict__ rdm) {
    typedef cx<T> V;
    V* Y = reinterpret_cast<V*>(rsp_lds);   // [GT][Ppad] + W_P table
    constexpr int GT = 16;
    V* twl = Y + GT * g.Ppad;
    const T* __restrict__ win = static_cast<const T*>(k.win);
    constexpr int NTW = plan_tw_total(PlanPow2<LGP>::p, false);
    if constexpr (LGP > 0) stage_lds<RSP_THREADS>(twl, static_cast<const V*>(k.twPp), NTW);
    const int b = blockIdx.y, gt0 = blockIdx.x * GT;
    const int P = g.P, G = g.G, Ppad = g.Ppad;
    for (int e = threadIdx.x; e < P * GT; e += RSP_THREADS) {
        const int m = e / GT, gl = e - m * GT;
        const int gg = gt0 + gl;
        V val = V{};
        if (gg < G) val = pc[((size_t)b * P + m) * G + gg] * win[m];
        Y[gl * Ppad + m] = val;
    }
    __syncthreads();
    const int half = P >> 1;
    if constexpr (LGP > 0) {
        StoreLds<V> st{Y};
        fft_passes<LGP, (16 << LGP) / RSP_THREADS, 0, RSP_THREADS>(Y, Ppad, GT, twl, st, st);
        for (int e = threadIdx.x; e < P * GT; e += RSP_THREADS) {
            const int v = e / GT, gl = e - v * GT;
            const int gg = gt0 + gl;
            int src = v - half;
            if (src < 0) src += P;
            if (gg < G) rdm[((size_t)b * P + v) * G + gg] = Y[gl * Ppad + src];
        }
    } else {
        const V* __restrict__ twP = static_cast<const V*>(k.twP);
        for (int e = threadIdx.x; e < P * GT; e += RSP_THREADS) {
            const int v = e / GT, gl = e - v * GT;
            const int gg = gt0 + gl;
            const V acc = dft_bin(Y + gl * Ppad, twP, P, v);
            if (gg < G) rdm[((size_t)b * P + v) * G + gg] = acc;
        }
    }
}

// ======================================================================================
// S4 + S4.1 on the device: echo synthesis + Philox noise (fsf:45-88)
// ======================================================================================
// The per-target phasors of S4, once per (target, pulse) and (target, channel) instead of once per
// sample: tab[t][j] = e^{i 2 pi fd_prt j} for j < P (doppler_phase_shift, fsf:58), then
// e^{i c dphi} for c < C (the channel phasor, fsf:71-72) -- the same sincos arguments, so the
// cube is what the per-sample evaluation gave.
__global__ __launch_bounds__(RSP_THREADS) void k_synth_tab(Geometry g, SynthTargets tg, int nt, d2* __restrict__ tab) {
    const int per = g.P + g.C;
    const int i = blockIdx.x * RSP_THREADS + threadIdx.x;
    if (i >= nt * per) return;
    const int t = i / per, j = i - t * per;
    double s, c;
    if (j < g.P)
        sincos(2.0 * M_PI * tg.t[t].fd_prt * j, &s, &c);
    else
        sincos((double)(j - g.P) * tg.t[t].dphi, &s, &c);
    tab[i] = d2{c, s};
}

// S4 + S4.1 on the device, laid out so that everything shared is loaded once: a wave owns one
// fast-time strip of SYNTH_NS samples n of one channel c (both wave-uniform, so the tx_pulse
// samples and the channel phasors are scalar loads), a lane owns the pulse pair (m, m + 1), and
// each target's two Doppler phasors are read once per strip, not once per sample. The pair is one
// Philox4x32-10 block (P is even, so flat indices 2q, 2q + 1 of the [C][N][P] order): the first
// sample takes words 0-1, the second 2-3 (oracle/philox.py documents the stream). Per sample the
// targets are summed in order (fsf:51-78), then the Box-Muller noise is added (fsf:80-88).
#define SYNTH_NS 8   // 4: same time, 16: +10 % (profiles/r06q_synth_ab.txt)
template <class T>
__global__ __launch_bounds__(RSP_THREADS) void k_synth(Geometry g, const double* __restrict__ tx, SynthTargets tg,
                                                          int nt, const d2* __restrict__ tab, int frame_idx,
                                                          uint64_t seed, double nscale, cx<T>* __restrict__ cube) {
    const int lane = threadIdx.x & 63;
    const int n0 = __builtin_amdgcn_readfirstlane((int)(blockIdx.y * (RSP_THREADS / 64) + (threadIdx.x >> 6)) * SYNTH_NS);
    if (n0 >= g.N) return;   // the whole wave
    const int c = blockIdx.z;
    const int m = 2 * ((int)blockIdx.x * 64 + lane);
    const bool act = m < g.P;
    const int per = g.P + g.C;
    double re[SYNTH_NS][2], im[SYNTH_NS][2];
#pragma unroll
    for (int u = 0; u < SYNTH_NS; ++u) re[u][0] = re[u][1] = im[u][0] = im[u][1] = 0.0;
    for (int t = 0; t < nt; ++t) {
        const int ds = tg.t[t].delay;
        if (!(ds > 0 && ds < g.N) || n0 + SYNTH_NS - 1 < ds) continue;
        const d2 d0 = act ? tab[t * per + m] : d2{}, d1 = act ? tab[t * per + m + 1] : d2{};
        const d2 cp = tab[t * per + g.P + c];
        const double amp = tg.t[t].amp;
#pragma unroll
        for (int u = 0; u < SYNTH_NS; ++u) {
            const int n = n0 + u;
            if (n < g.N && n >= ds) {
                const double tr = tx[2 * (n - ds)], ti = tx[2 * (n - ds) + 1];
                double er = amp * (tr * d0.x - ti * d0.y);   // amplitude * base * doppler
                double ei = amp * (tr * d0.y + ti * d0.x);
                re[u][0] += er * cp.x - ei * cp.y;
                im[u][0] += er * cp.y + ei * cp.x;
                er = amp * (tr * d1.x - ti * d1.y);
                ei = amp * (tr * d1.y + ti * d1.x);
                re[u][1] += er * cp.x - ei * cp.y;
                im[u][1] += er * cp.y + ei * cp.x;
            }
        }
    }
    if (!act) return;
#pragma unroll
    for (int u = 0; u < SYNTH_NS; ++u) {
        const int n = n0 + u;
        if (n >= g.N) break;
        const uint64_t q = ((uint64_t)c * g.N + n) * (uint64_t)(g.P >> 1) + (uint64_t)(m >> 1);   // flat index / 2
        uint32_t ctr[4] = {(uint32_t)q, (uint32_t)(q >> 32), (uint32_t)frame_idx, 0x52535020u};
        rsp_philox10(ctr, (uint32_t)seed, (uint32_t)(seed >> 32));
        cx<T>* dst = cube + (size_t)c * g.cpitch + (size_t)n * g.P + m;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint32_t xa = h ? ctr[2] : ctr[0];
            const uint32_t xb = h ? ctr[3] : ctr[1];
            const double ua = ((double)xa + 0.5) * 2.3283064365386963e-10;
            const double ub = ((double)xb + 0.5) * 2.3283064365386963e-10;
            const double rr = sqrt(-2.0 * rsp_nm_log(ua));
            double sb, cb;
            rsp_nm_sincos2pi(ub, &sb, &cb);   // sincos(2 pi ub)
            dst[h] = cx<T>{(T)(re[u][h] + rr * cb * nscale), (T)(im[u][h] + rr * sb * nscale)};
        }
    }
}

// ======================================================================================
// Detection lists -> pinned host memory (the queue's read-back, after K3)
// ======================================================================================
// Frame f = blockIdx.x: record 0 (the count) and the first min(count, dcap, hcap) detections
// from the device list (stride dcap + 1 records) into the mapped host list (stride hcap + 1), so
// only the records that exist cross PCIe, whatever the count (a fixed-size async copy moved the
// first 512 and left the rest to a synchronous tail copy).
__global__ __launch_bounds__(RSP_THREADS) void k_dets_to_host(const DevDet* __restrict__ dets, int dcap,
                                                             DevDet* __restrict__ host, int hcap) {
    const int f = blockIdx.x;
    const u32x4* src = reinterpret_cast<const u32x4*>(dets + (size_t)f * (dcap + 1));
    u32x4* dst = reinterpret_cast<u32x4*>(host + (size_t)f * (hcap + 1));
    const int cnt = *reinterpret_cast<const int*>(src);
    const int n = 1 + min(cnt, min(dcap, hcap));   // records, the count record included
    constexpr int U = sizeof(DevDet) / 16;        // 16-B units per record
    for (int e = threadIdx.x; e < n * U; e += RSP_THREADS) dst[e] = src[e];
}

}  // namespace

hipError_t launch_dets_to_host(const void* dets, int dcap, void* host, int hcap, int nf, hipStream_t s) {
    static_assert(sizeof(DevDet) % 16 == 0, "16-B units");
    hipLaunchKernelGGL(k_dets_to_host, dim3(nf), dim3(RSP_THREADS), 0, s, static_cast<const DevDet*>(dets), dcap,
                       static_cast<DevDet*>(host), hcap);
    return hipGetLastError();
}

// Streaming copy (rsp_hbm_copy_probe): CU16 x 16 B per lane, all loads in flight before the
// stores, one chunk per workgroup.
#define RSP_COPY_U 4    // 16-B loads per lane in flight; non-temporal both ways (6.2-6.5 TB/s at 0.25-1 GiB, 5.7-5.9 plain)
__global__ __launch_bounds__(256) void k_stream_copy(const u32x4* __restrict__ in, u32x4* __restrict__ out, size_t n16) {
    const size_t base = (size_t)blockIdx.x * (256 * RSP_COPY_U) + threadIdx.x;
    u32x4 v[RSP_COPY_U];
#pragma unroll
    for (int u = 0; u < RSP_COPY_U; ++u)
        if (base + u * 256 < n16) v[u] = __builtin_nontemporal_load(in + base + u * 256);
#pragma unroll
    for (int u = 0; u < RSP_COPY_U; ++u)
        if (base + u * 256 < n16) __builtin_nontemporal_store(v[u], out + base + u * 256);
}

hipError_t launch_stream_copy(const void* in, void* out, size_t n16, int, hipStream_t s) {
    hipLaunchKernelGGL(k_stream_copy, dim3((unsigned)((n16 + 256 * RSP_COPY_U - 1) / (256 * RSP_COPY_U))), dim3(256), 0, s,
                       static_cast<const u32x4*>(in), static_cast<u32x4*>(out), n16);
    return hipGetLastError();
}

template <class T, int LGP>
static hipError_t launch_mtd_t(const Geometry& g, const DevConsts& k, const void* pc, void* rdm, hipStream_t s) {
    return launch(k_mtd_cols<T, LGP>, dim3((g.G + 15) / 16, g.B), dim3(RSP_THREADS), mtd_cols_lds(g), s, g, k,
                  static_cast<const cx<T>*>(pc), static_cast<cx<T>*>(rdm));
}

template <class T>
static hipError_t launch_mtd_p(const Geometry& g, const DevConsts& k, const void* pc, void* rdm, hipStream_t s) {
    switch (k1_route(g, 0).lgp2) {
        case 4: return launch_mtd_t<T, 4>(g, k, pc, rdm, s);
        case 5: return launch_mtd_t<T, 5>(g, k, pc, rdm, s);
        case 6: return launch_mtd_t<T, 6>(g, k, pc, rdm, s);
        case 7: return launch_mtd_t<T, 7>(g, k, pc, rdm, s);
        case 8: return launch_mtd_t<T, 8>(g, k, pc, rdm, s);
        case 9: return launch_mtd_t<T, 9>(g, k, pc, rdm, s);
        default: return launch_mtd_t<T, 0>(g, k, pc, rdm, s);
    }
}

hipError_t launch_mtd_cols(const Geometry& g, const DevConsts& k, const void* pc, void* rdm, hipStream_t s) {
    return g.prec == RSP_PREC_F64 ? launch_mtd_p<double>(g, k, pc, rdm, s) : launch_mtd_p<float>(g, k, pc, rdm, s);
}

hipError_t launch_synth(const Geometry& g, const double* tx, const SynthTargets& tg, int nt, void* tab, int frame_idx,
                        uint64_t seed, double nscale, void* cube, hipStream_t s) {
    if (g.P & 1) return hipErrorInvalidValue;   // pulse pairs are Philox pairs; plans reject odd P at creation
    if (nt > 0)
        hipLaunchKernelGGL(k_synth_tab, dim3((nt * (g.P + g.C) + RSP_THREADS - 1) / RSP_THREADS), dim3(RSP_THREADS), 0, s,
                           g, tg, nt, static_cast<d2*>(tab));
    constexpr int rows = SYNTH_NS * (RSP_THREADS / 64);   // fast-time samples per workgroup
    const dim3 grid((g.P / 2 + 63) / 64, (g.N + rows - 1) / rows, g.C);
    if (g.prec == RSP_PREC_F64)
        hipLaunchKernelGGL(k_synth<double>, grid, dim3(RSP_THREADS), 0, s, g, tx, tg, nt, static_cast<const d2*>(tab),
                           frame_idx, seed, nscale, static_cast<d2*>(cube));
    else
        hipLaunchKernelGGL(k_synth<float>, grid, dim3(RSP_THREADS), 0, s, g, tx, tg, nt, static_cast<const d2*>(tab),
                           frame_idx, seed, nscale, static_cast<f2*>(cube));
    return hipGetLastError();
}
