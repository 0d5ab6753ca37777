// rsp_plan.h -- what the units of the host runtime share (private: not installed): struct rsp_plan with
// its lanes, and the helpers more than one of rsp_plan.cpp (the plan, the queue, the synchronous frame
// paths), rsp_plan_cfar.cpp (stage 2 and the CFAR call family) and rsp_plan_calls.cpp (the stand-alone
// DBF, MTD, detection, pulse-compression and down-conversion calls) uses.
#pragma once
#include "rsp.h"
#include "rsp_frame_host.h"
#include "rsp_internal.h"

#include <algorithm>
#include <complex>
#include <deque>
#include <map>
#include <memory>
#include <vector>

#pragma GCC visibility push(hidden)

// Error sink (declared in rsp_frame_host.h) and host-only stages live in rsp_host.cpp (plain C++,
// built and sanitized without HIP); this is their hidden entry point.
void rsp_cluster_frame(const rsp_cluster_params& cp, std::vector<rsp_detection>& dets, std::vector<rsp_target>& final_targets);

template <class... A>
int fail(int code, const char* fmt, A... a) { return rsp_set_error(code, fmt, a...); }

#define HIPCHK(expr)                                                                            \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail(RSP_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                    \
    } while (0)

using cd = std::complex<double>;
using cf = std::complex<float>;

struct Lane {
    hipStream_t stream = nullptr;   // the lane's stream: its batches' kernels and detection read-back
    hipEvent_t tev[4] = {};         // live stage timing: before K1, after K1, K2, K3
    bool timed = false;
    hipEvent_t done = nullptr;
    void* z = nullptr;          // F frames
    void* rdm = nullptr;        // ONE frame: the synchronous paths' RDM (queue frames write the caller's maps)
    void* mag = nullptr;        // F frames
    DevDet* dets = nullptr;     // F x (1 + dcap): record 0 of each frame holds its count
    int dcap = 0;               // device detection-list capacity per frame (grows on demand)
    DevDet* h_dets = nullptr;   // mapped pinned F x (1 + hcap), same layout, written by k_dets_to_host
    DevDet* h_dets_dev = nullptr;
    int hcap = 0;               // host read-back capacity per frame (grows on demand)
    // band route: the frames' edge-row flags (F x RSP_NEED_BYTES) and deferred-cell lists (F x fcap
    // entries; grow on demand like the detection lists)
    unsigned char* need = nullptr;
    int2* defer = nullptr;
    int fcap = 0;
    bool band = false;          // the batch in flight took the band route
    FramePtrs fp{};             // the batch in flight (K3 runs again after a device-list growth)
    int nf = 0;
    int frame_ids[RSP_MAX_F];
    bool busy = false;
};

struct FrameResult {
    int frame_idx;
    int n_dets;
    std::vector<rsp_target> targets;
};

class ClusterPool;   // the queue's clustering workers (rsp_plan.cpp)

#pragma GCC visibility pop

struct rsp_plan {
    int device = 0;
    Geometry g{};
    DevConsts k{};
    rsp_cluster_params cl{};
    SynthConsts sc{};   // what S4 reads of the configuration
    int F = 1;
    int det_bound = 1;   // cells under test per frame: the most detections a frame can have
    size_t esz = 16;   // bytes of one complex element (16: complex128, 8: complex64)
    size_t rsz = 8;    // bytes of one real element
    size_t z_elems = 0, rdm_elems = 0, mag_elems = 0;
    std::vector<void*> dev_allocs;
    double* d_tx = nullptr;
    double* d_stab = nullptr;     // S4 phasor tables: RSP_MAX_SYNTH_TARGETS x (P + C) complex
    void* d_cube = nullptr;       // staging cube for the synchronous paths
    void* d_aux = nullptr;        // second map for the stage-2 path
    void* d_smap = nullptr;       // rdm_for_cfar_all of the synchronous path (allocated on first request)
    // stage-3 range CFAR (rsp_stage3_cfar, rsp_process_stage2_cfar): the segments' gate counts, whether
    // d_aux holds a stage-2 result, and device buffers that grow on demand (freed with the plan)
    int32_t gates[3] = {0, 0, 0};
    std::vector<K2Rec> k2rec;     // host copy of DevConsts::k2rec (rsp_query_k2_records)
    // band route (launch_batch): the three row sets, the band and edge record tables on the device
    // and on the host, whether the plan may take it at all, and what it did (rsp_band_counters_get)
    K2Rows k2rows[3] = {};
    std::vector<K2Rec> k2rec_band, k2rec_edge;
    const K2Rec* drec_band = nullptr;
    const K2Rec* drec_edge = nullptr;
    bool band_ok = false;
    rsp_band_counters ctr{};
    bool aux_valid = false;
    bool smap_valid = false;      // d_smap holds the pair-sum maps of the plan's last synchronous frame
    struct DevBuf {
        void* p = nullptr;
        size_t cap = 0;
    };
    DevBuf s3_in, s3_amp, s3_thr, s3_flags, s3_hits, s3_count;
    // stand-alone DBF (rsp_dbf, rsp_profile_dbf): channel planes, beam planes and the A operands of the call
    DevBuf dbf_in, dbf_out, dbf_tab;
    // stand-alone MTD (rsp_mtd, rsp_profile_mtd): the call's cube, result and window, and what a length
    // needs once: the chirp-z tables w | Bf by nfft and the Stockham twiddles by log2 of the LDS transform
    DevBuf mtd_in, mtd_out, mtd_win;
    std::map<int, void*> mtd_tab, mtd_tw;
    // detection on any RD cube (rsp_detect and its compositions): the call's cube, its pair-sum maps, the
    // S9 records of its hits, and the caller's axes, angles and K-LUT (doubles); the plan's own
    // cluster parameters are `cl`
    DevBuf det_in, det_smap, det_dets, det_axes;
    // pulse compression for any pulse and beam count (rsp_pc and its compositions): the call's beams, k2_pc's
    // z input, its [B][P][G] result and the magnitude map it always stores (scratch: nothing reads it), the
    // host forms' result in MATLAB's layout, and the record table of the (P, B) in pc_d, rebuilt only when
    // they change (pc_d.g.P = 0: none yet)
    DevBuf pc_in, pc_z, pc_res, pc_mag, pc_out, pc_rec;
    PcDesc pc_d{};
    // digital down-conversion (rsp_ddc and its composition): the call's real cube, its complex result and taps
    DevBuf ddc_in, ddc_out, ddc_h;
    // raw-cube stage 2 (rsp_process_raw_stage2*): the plan's own weights, and the A operands of the last
    // call whose W / conj were not the plan's (K1's layout; uploaded again only when they change)
    std::vector<double> h_W;
    DevBuf raw_tab;
    std::vector<double> raw_W;
    int raw_conj = 0;
    unsigned char* h_stage = nullptr;   // pinned staging for uploads
    size_t h_stage_bytes = 0;
    Lane lanes[RSP_LANES];
    int nlanes = RSP_NLANES;   // lanes (streams) of the throughput queue
    int next_lane = 0;
    // live stage timing of the queue (rsp_set_stage_timing): HIP events around K1/K2/K3 of
    // every batch, summed at harvest
    bool time_stages = false;
    double stage_ms[3] = {0, 0, 0};
    int64_t stage_launches = 0, stage_frames = 0;
    // pending batch of the queue
    const void* pend_in[RSP_MAX_F];
    void* pend_rdm[RSP_MAX_F];  // caller's device RD map of each pending frame (nullptr: kept on chip)
    int pend_ids[RSP_MAX_F];
    int pend_slot[RSP_MAX_F];   // producer-ring slot of each pending frame, -1 = caller's device cube
    int npend = 0;
    // producer ring of the queue (rsp_enqueue_host, rsp_process_targets_multi): device cubes
    // written on up_stream.  slot_ready[s] orders K1 after the write; slot_free[s], recorded after
    // the K1 that read slot s, orders the next write after it.  (nlanes + 1) x F slots: a slot
    // comes round again only after its frame's batch has been launched.
    hipStream_t up_stream = nullptr;
    std::vector<void*> ring;
    std::vector<hipEvent_t> slot_ready, slot_free;
    std::vector<char> slot_used;
    int ring_next = 0;
    std::deque<FrameResult> results;   // deque: push_back keeps the elements the pool writes in place
    std::vector<rsp_detection> last_dets;   // detections of the last synchronous frame (rsp_last_detections)
    std::vector<rsp_target> last_targets;   // its final targets (rsp_last_targets)
    // clustering workers of the queue (created with the first batch of F > 1 frames); every
    // reader of `results` calls results_ready() first.  Declared after `results`: destroyed first.
    // ClusterPool is rsp_plan.cpp's, and so are the three members that need all of it.
    std::unique_ptr<ClusterPool> pool;
    __attribute__((visibility("hidden"))) void results_ready() const;

    __attribute__((visibility("hidden"))) rsp_plan();
    ~rsp_plan();
    int dalloc_bytes(void** p, size_t bytes) {
        void* q = nullptr;
        if (hipMalloc(&q, bytes + 16) != hipSuccess) return fail(RSP_ERR_NOMEM, "hipMalloc(%zu bytes) failed", bytes);
        dev_allocs.push_back(q);
        *p = q;
        return RSP_OK;
    }
    template <class T>
    int dalloc(T** p, size_t n) {
        void* q = nullptr;
        int rc = dalloc_bytes(&q, n * sizeof(T));
        *p = (T*)q;
        return rc;
    }
    template <class T>
    int upload(T** p, const std::vector<T>& h) {
        int rc = dalloc(p, std::max<size_t>(h.size(), 1));
        if (rc) return rc;
        if (!h.empty()) HIPCHK(hipMemcpy(*p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
        return RSP_OK;
    }
    // n doubles into device memory as the plan's real type: narrowed for a complex-single plan
    int put_reals(void* d, const double* h, size_t n) {
        std::vector<float> v(g.prec == RSP_PREC_F64 ? 0 : n);
        if (g.prec != RSP_PREC_F64) rsp_convert_reals(h, RSP_C128, n, v.data());
        if (n) HIPCHK(hipMemcpy(d, g.prec == RSP_PREC_F64 ? (const void*)h : v.data(), n * rsz, hipMemcpyHostToDevice));
        return RSP_OK;
    }
    // complex / real tables in the plan's precision
    int upload_reals(const void** p, const double* h, size_t n) {
        void* q = nullptr;
        int rc = dalloc_bytes(&q, std::max<size_t>(n, 1) * rsz);
        *p = q;
        return rc ? rc : put_reals(q, h, n);
    }
    int upload_c(const void** p, const std::vector<cd>& h) {
        return upload_reals(p, reinterpret_cast<const double*>(h.data()), 2 * h.size());
    }
    int upload_r(const void** p, const std::vector<double>& h) { return upload_reals(p, h.data(), h.size()); }
};

#pragma GCC visibility push(hidden)

// The dtype code of the plan's precision; RSP_C128 without a plan, for the size checks before the null check
inline int plan_dtype(const rsp_plan* p) { return p && p->g.prec != RSP_PREC_F64 ? RSP_C64 : RSP_C128; }

// ---- rsp_plan.cpp ----
// Every queued batch launched, harvested and clustered; begin_sync: how a synchronous call starts, the
// plan's device current and the plan idle
int drain_all(rsp_plan* p);
int begin_sync(rsp_plan* p);
// The buffers of nf frames on lane L: the cubes `in`, the lane's own, and the RD maps rdm[f] (null: see launch_batch)
FramePtrs lane_ptrs(const rsp_plan* p, const Lane& L, const void* const* in, int nf, void* const* rdm);
// A device buffer that grows on demand (freed with the plan)
int dev_reserve(rsp_plan::DevBuf& b, size_t bytes);
// `elems` complex values of a host array (dtype RSP_C64 or RSP_C128, already checked) in the plan's precision:
// *src = h when the dtypes agree, else the plan's pinned staging buffer after rsp_convert_reals.  Either is
// borrowed until the caller has waited for its copy.
int host_in_plan_prec(rsp_plan* p, const void* h, int dtype, size_t elems, const void** src);
// The same for `reals` real values, doubles (f64) or floats
int host_reals_in_plan_prec(rsp_plan* p, const void* h, bool f64, size_t reals, const void** src);
// `elems` complex values of the plan's precision, device to host on stream s and waited for, widened to double
int download_widened(rsp_plan* p, const void* d_src, size_t elems, double* out, hipStream_t s);
// Copy a host cube (complex64 or complex128, nch channel slabs of N x P) into d_dst in the
// plan's precision (a converting copy only when the dtypes differ).
int upload_cube(rsp_plan* p, const void* cube, int dtype, int nch, void* d_dst, hipStream_t s);
// A device map [B][P][G] of the plan's shape and precision -> MATLAB's [P x G x B] complex double
int rdm_out(const rsp_plan* p, const void* d_map, double* out);
// The two capped lists of a synchronous frame into out (not null): both are copied before an overflow is
// reported (the return value); the targets first, so that with both lists short the message that stays is the detections'
int frame_lists_out(const std::vector<rsp_target>& targets, const std::vector<rsp_detection>& dets, rsp_frame_out* out);

// ---- rsp_plan_cfar.cpp ----
// Stage 2 of beams [P x N x B]: PC_results into lane 0's map, MTD_results into p->d_aux; returns with the stream idle
int stage2_device(rsp_plan* p, const void* iq, int dtype);
// A CFAR kernel (D: S3Desc, VcDesc or XcDesc) on lane 0's stream over the n_maps device maps d_in of d.P x d.G
// (cplx: complex values of the plan's precision, else real amplitudes), with the device outputs the caller
// asks for (amp / thr / flags: the plan's s3 buffers, already reserved) and, with `list`, the device hit list
// p->s3_hits: count, then grow -- a run that counts more hits than the list holds grows the list to the
// count and runs once more.  Returns with the stream idle, *total = the hits, all of them on the device
// when `list`.
template <class D>
int cfar_launch_grow(rsp_plan* p, const D& d, bool cplx, const void* d_in, int n_maps, bool amp, bool thr, bool flags,
                     bool list, int* total_out);

// n device maps [P][G] of element type S -> MATLAB column-major [P x G x n] of D (rsp_transpose_planes)
template <class S, class D>
int maps_to_matlab(const void* d_map, int P, int G, int n, D* out) {
    std::vector<S> m((size_t)n * P * G);
    HIPCHK(hipMemcpy(m.data(), d_map, m.size() * sizeof(S), hipMemcpyDeviceToHost));
    rsp_transpose_planes(m.data(), P, G, n, out);
    return RSP_OK;
}
// ... of the plan's precision, widened: complex maps (the RD maps) as W = cd and N = cf, real ones (the
// pair-sum maps) as double and float
template <class W, class N>
int plan_maps_to_matlab(const rsp_plan* p, const void* d_map, int P, int G, int n, double* out) {
    return p->g.prec == RSP_PREC_F64 ? maps_to_matlab<W>(d_map, P, G, n, (W*)out) : maps_to_matlab<N>(d_map, P, G, n, (W*)out);
}

// The profile entries' measurement: run() once to warm up, then iters times between two events on
// stream s; *ms_per_iter = elapsed / iters.  run returns a status; the first one that is not RSP_OK
// ends the measurement and is returned.  The events are destroyed on every way out.
template <class F>
int time_launches(hipStream_t s, int iters, F run, float* ms_per_iter) {
    struct Events {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() {
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
        }
    } ev;
    HIPCHK(hipEventCreate(&ev.e0));
    HIPCHK(hipEventCreate(&ev.e1));
    int rc = run();
    if (rc) return rc;
    HIPCHK(hipEventRecord(ev.e0, s));
    for (int i = 0; i < iters; ++i)
        if ((rc = run())) return rc;
    HIPCHK(hipEventRecord(ev.e1, s));
    HIPCHK(hipEventSynchronize(ev.e1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    *ms_per_iter = ms / iters;
    return RSP_OK;
}

#pragma GCC visibility pop
