// rsp_plan.cpp -- host runtime of librsp: plan construction (device checks, uploads and lanes;
// the geometry analysis of the reference's precomputed_data is rsp_geometry.cpp's), the C-ABI of
// include/rsp.h, the device-resident frame queue, and the host stages S10/S11 (two-level BFS
// clustering, fsf:302-407).
#include "rsp.h"
#include "rsp_frame_host.h"
#include "rsp_internal.h"

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

// Error sink (declared in rsp_frame_host.h) and host-only stages live in rsp_host.cpp (plain C++,
// built and sanitized without HIP); this is their hidden entry point.
__attribute__((visibility("hidden"))) void rsp_cluster_frame(const rsp_cluster_params& cp, std::vector<rsp_detection>& dets,
                                                             std::vector<rsp_target>& final_targets);

namespace {

template <class... A>
int fail(int code, const char* fmt, A... a) { return rsp_set_error(code, fmt, a...); }

}  // namespace

namespace {

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

// Host worker threads for S10/S11 (fsf:302-407) of the queue's frames: a harvested batch's
// frames are clustered in parallel while the host thread goes on launching batches, so the
// clustering neither delays the next launch nor serialises the end of a run (one x2 frame with
// ~250 detections takes ~60 us; eight in a row were ~0.5 ms of host time per batch).
class ClusterPool {
public:
    explicit ClusterPool(int n) {
        for (int i = 0; i < n; ++i) th_.emplace_back([this] { loop(); });
    }
    ~ClusterPool() {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
    void submit(std::function<void()> f) {
        {
            std::lock_guard<std::mutex> g(m_);
            q_.push_back(std::move(f));
            ++pending_;
        }
        cv_.notify_one();
    }
    void wait() {   // every submitted task has finished
        std::unique_lock<std::mutex> g(m_);
        done_.wait(g, [this] { return pending_ == 0; });
    }

private:
    void loop() {
        for (;;) {
            std::function<void()> f;
            {
                std::unique_lock<std::mutex> g(m_);
                cv_.wait(g, [this] { return stop_ || !q_.empty(); });
                if (q_.empty()) return;
                f = std::move(q_.front());
                q_.pop_front();
            }
            f();
            std::lock_guard<std::mutex> g(m_);
            if (--pending_ == 0) done_.notify_all();
        }
    }
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    std::deque<std::function<void()>> q_;
    int pending_ = 0;
    bool stop_ = false;
};

struct FrameResult {
    int frame_idx;
    int n_dets;
    std::vector<rsp_target> targets;
};

}  // namespace

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
    std::unique_ptr<ClusterPool> pool;
    void results_ready() const {
        if (pool) pool->wait();
    }

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

rsp_plan::~rsp_plan() {
    results_ready();
    (void)hipSetDevice(device);
    for (auto& L : lanes) {
        if (L.stream) (void)hipStreamSynchronize(L.stream);
        if (L.h_dets) (void)hipHostFree(L.h_dets);
        if (L.dets) (void)hipFree(L.dets);
        if (L.defer) (void)hipFree(L.defer);
        if (L.done) (void)hipEventDestroy(L.done);
        for (auto& e : L.tev)
            if (e) (void)hipEventDestroy(e);
        if (L.stream) (void)hipStreamDestroy(L.stream);
    }
    if (up_stream) (void)hipStreamSynchronize(up_stream);
    for (auto e : slot_ready) if (e) (void)hipEventDestroy(e);
    for (auto e : slot_free) if (e) (void)hipEventDestroy(e);
    if (up_stream) (void)hipStreamDestroy(up_stream);
    if (h_stage) (void)hipHostFree(h_stage);
    for (DevBuf* b : {&s3_in, &s3_amp, &s3_thr, &s3_flags, &s3_hits, &s3_count, &dbf_in, &dbf_out, &dbf_tab, &raw_tab, &mtd_in, &mtd_out,
                      &mtd_win, &det_in, &det_smap, &det_dets, &det_axes, &pc_in, &pc_z, &pc_res, &pc_mag, &pc_out, &pc_rec})
        if (b->p) (void)hipFree(b->p);
    for (auto* m : {&mtd_tab, &mtd_tw})
        for (auto& kv : *m) (void)hipFree(kv.second);
    for (void* p : dev_allocs) (void)hipFree(p);
}

namespace {

// Device detection lists of a lane: F x (1 + cap) records (record 0 of a frame = its count).
// The new lists are allocated first and swapped in only on success: a failed growth leaves the
// lane with its old lists and capacity (still consistent for the next launch).
int lane_dets_alloc(rsp_plan* p, Lane& L, int cap) {
    const int ncap = std::max(cap, 1);
    DevDet* nd = nullptr;
    if (hipMalloc((void**)&nd, sizeof(DevDet) * (size_t)(ncap + 1) * p->F) != hipSuccess)
        return fail(RSP_ERR_NOMEM, "hipMalloc of %d-detection lists failed", ncap);
    if (L.dets) HIPCHK(hipFree(L.dets));
    L.dets = nd;
    L.dcap = ncap;
    return RSP_OK;
}

// Mapped, coherent pinned read-back lists of a lane: F x (1 + cap) records, written by
// k_dets_to_host over PCIe after K3 (only the records that exist).
int lane_host_alloc(rsp_plan* p, Lane& L, int cap) {
    if (L.h_dets) HIPCHK(hipHostFree(L.h_dets));
    L.h_dets = L.h_dets_dev = nullptr;
    L.hcap = std::max(cap, 1);
    if (hipHostMalloc((void**)&L.h_dets, sizeof(DevDet) * (size_t)(L.hcap + 1) * p->F,
                      hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
        return fail(RSP_ERR_NOMEM, "pinned %d-detection read-back lists failed", L.hcap);
    HIPCHK(hipHostGetDevicePointer((void**)&L.h_dets_dev, L.h_dets, 0));
    return RSP_OK;
}

// Deferred-cell lists of a lane, F x cap entries; swapped in only on success, like the detection lists
int lane_defer_alloc(rsp_plan* p, Lane& L, int cap) {
    const int ncap = std::max(cap, 1);
    int2* nd = nullptr;
    if (hipMalloc((void**)&nd, sizeof(int2) * (size_t)ncap * p->F) != hipSuccess)
        return fail(RSP_ERR_NOMEM, "hipMalloc of %d-cell deferred lists failed", ncap);
    if (L.defer) HIPCHK(hipFree(L.defer));
    L.defer = nd;
    L.fcap = ncap;
    return RSP_OK;
}

int pow2_at_least(int x) {
    int c = 1;
    while (c < x && c < (1 << 30)) c <<= 1;
    return c;
}

int setup_lane(rsp_plan* p, Lane& L) {
    HIPCHK(hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&L.done, hipEventDisableTiming));
    for (auto& e : L.tev) HIPCHK(hipEventCreate(&e));
    int rc;
    if ((rc = p->dalloc_bytes(&L.z, p->z_elems * p->F * p->esz))) return rc;
    // one frame (sync paths); F frames when S9 reads the complex map (RSP_PLAN_MONOPULSE_COMPLEX)
    if ((rc = p->dalloc_bytes(&L.rdm, p->rdm_elems * p->esz * (p->g.mono_c ? p->F : 1)))) return rc;
    if ((rc = p->dalloc_bytes(&L.mag, p->mag_elems * p->F * p->rsz))) return rc;
    if ((rc = lane_dets_alloc(p, L, std::min(p->det_bound, 4096)))) return rc;
    if (p->band_ok) {
        void* q = nullptr;
        if ((rc = p->dalloc_bytes(&q, (size_t)RSP_NEED_BYTES * p->F))) return rc;
        L.need = static_cast<unsigned char*>(q);
        if ((rc = lane_defer_alloc(p, L, std::min(p->det_bound, 1024)))) return rc;
    }
    return lane_host_alloc(p, L, std::min(p->det_bound, 1024));
}

// rdm[f] = nullptr: K2 keeps frame f's complex RD map on chip and stores only its magnitudes,
// the one input of K3 and S9.  fun_process_single_frame returns final_targets (fsf:13); its
// rdm_13beam is an intermediate, so the throughput queue does not write it to HBM (-10% k2_pc)
// unless the caller hands a map for the frame (rsp_enqueue_device_rdm).  rdm == nullptr: no
// frame writes its map.  The synchronous paths (rsp_process_* with out->rdm, process_stage2)
// run one frame into the lane's own map L.rdm.  With RSP_PLAN_MONOPULSE_COMPLEX K3's S9 reads
// the complex map, so every frame writes one: the caller's, or the lane's own (F frames).
// Each frame's count (zeroed by K1, bumped by K3) and detections in the lane's device lists as they
// are now: again after a growth.
void lane_det_ptrs(const Lane& L, int nf, FramePtrs& fp) {
    for (int f = 0; f < nf; ++f) {
        DevDet* rec = L.dets + (size_t)(L.dcap + 1) * f;
        fp.count[f] = reinterpret_cast<int*>(rec);
        fp.dets[f] = rec + 1;
    }
}

FramePtrs lane_ptrs(const rsp_plan* p, const Lane& L, const void* const* in, int nf, void* const* rdm) {
    FramePtrs fp{};
    for (int f = 0; f < nf; ++f) {
        fp.in[f] = in[f];
        fp.z[f] = (char*)L.z + p->z_elems * p->esz * f;
        fp.rdm[f] = rdm && rdm[f] ? rdm[f] : (p->g.mono_c ? (char*)L.rdm + p->rdm_elems * p->esz * f : nullptr);
        fp.mag[f] = (char*)L.mag + p->mag_elems * p->rsz * f;
    }
    lane_det_ptrs(L, nf, fp);
    return fp;
}

// The band route's flag blocks and deferred lists of the lane as they are now (null off the route)
void lane_band_ptrs(const Lane& L, int nf, FramePtrs& fp) {
    for (int f = 0; f < nf; ++f) {
        fp.need[f] = L.band ? L.need + (size_t)RSP_NEED_BYTES * f : nullptr;
        fp.defer[f] = L.band ? L.defer + (size_t)L.fcap * f : nullptr;
    }
}

// Whether a batch takes the band route: K2 of the rows under test, K3 with the edge cells deferred,
// K2 of the flagged edge rows, K3's finish.  Only where nobody reads the other rows: no frame writes
// its RD map (fp.rdm: the caller's, or the complex-ratio monopulse's) and no CFAR map is asked for.
bool band_route(const rsp_plan* p, const FramePtrs& fp, int nf) {
    if (!p->band_ok) return false;
    for (int f = 0; f < nf; ++f)
        if (fp.rdm[f] || fp.smap[f]) return false;
    return true;
}

// K2 of nf frames on the lane's stream: the rows under test on the band route, else every row
hipError_t launch_k2_lane(const rsp_plan* p, const Lane& L, const FramePtrs& fp, int nf) {
    if (!L.band) return launch_k2(p->g, p->k, fp, nf, L.stream);
    return launch_k2_set(p->g, p->k, fp, nf, p->k2rows[K2SET_BAND], p->drec_band, (int)p->k2rec_band.size(), false, L.stream);
}

// K3 of nf frames on the lane's stream, its lists at the lane's present capacities; on the band
// route its two phases with the on-demand K2 of the edge rows between them
hipError_t launch_k3_lane(const rsp_plan* p, const Lane& L, const FramePtrs& fp, int nf) {
    Geometry g3 = p->g;
    g3.max_dets = L.dcap;
    if (!L.band) return launch_k3(g3, p->k, fp, nf, L.stream);
    hipError_t e = launch_k3(g3, p->k, fp, nf, L.stream, K3_DEFER, L.fcap);
    if (e == hipSuccess)
        e = launch_k2_set(p->g, p->k, fp, nf, p->k2rows[K2SET_EDGE], p->drec_edge, (int)p->k2rec_edge.size(), true, L.stream);
    return e != hipSuccess ? e : launch_k3(g3, p->k, fp, nf, L.stream, K3_FINISH, L.fcap);
}

// A frame's counters (record 0 of its list) and, on the band route, the flag blocks: what K1 zeroes
// in the pipeline, for the launches that run K3 without a K1 before it
hipError_t zero_k3_state(const Lane& L, int nf) {
    hipError_t e = hipMemset2DAsync(L.dets, sizeof(DevDet) * (L.dcap + 1), 0, 3 * sizeof(int), nf, L.stream);
    if (e == hipSuccess && L.band) e = hipMemsetAsync(L.need, 0, (size_t)RSP_NEED_BYTES * nf, L.stream);
    return e;
}

// Enqueue K1 -> K2 -> K3 for nf frames on lane L, plus the async detection read-back.
// smap (optional, one frame): K3 also writes rdm_for_cfar_all there.
// A lane's buffers are reused only after harvest has waited for the lane's previous batch.
int launch_batch(rsp_plan* p, Lane& L, const void* const* in, const int* ids, int nf, void* smap = nullptr,
                 const int* slots = nullptr, void* const* rdm = nullptr) {
    FramePtrs fp = lane_ptrs(p, L, in, nf, rdm);
    fp.smap[0] = smap;
    L.band = band_route(p, fp, nf);
    lane_band_ptrs(L, nf, fp);
    if (slots)   // producer-ring frames: K1 after their upload / synthesis
        for (int f = 0; f < nf; ++f)
            if (slots[f] >= 0) HIPCHK(hipStreamWaitEvent(L.stream, p->slot_ready[slots[f]], 0));
    L.timed = p->time_stages;
    if (L.timed) HIPCHK(hipEventRecord(L.tev[0], L.stream));
    HIPCHK(launch_k1(p->g, p->k, fp, nf, 3, L.stream));
    if (slots)   // K1 has read the cubes: their slots may be written again
        for (int f = 0; f < nf; ++f)
            if (slots[f] >= 0) HIPCHK(hipEventRecord(p->slot_free[slots[f]], L.stream));
    if (L.timed) HIPCHK(hipEventRecord(L.tev[1], L.stream));
    HIPCHK(launch_k2_lane(p, L, fp, nf));
    if (L.timed) HIPCHK(hipEventRecord(L.tev[2], L.stream));
    HIPCHK(launch_k3_lane(p, L, fp, nf));
    if (L.timed) HIPCHK(hipEventRecord(L.tev[3], L.stream));
    // every frame's count and detections into the lane's mapped pinned lists (only what exists)
    HIPCHK(launch_dets_to_host(L.dets, L.dcap, L.h_dets_dev, L.hcap, nf, L.stream));
    HIPCHK(hipEventRecord(L.done, L.stream));
    L.fp = fp;
    L.nf = nf;
    for (int f = 0; f < nf; ++f) L.frame_ids[f] = ids[f];
    L.busy = true;
    return RSP_OK;
}

// Wait for lane L, gather its detections and cluster.  The lists have no fixed capacity, like
// all_raw_detections(end+1, :) (fsf:215-221): a frame with more detections than the lane's device
// list grows the list and runs K3 again on the batch (its magnitude maps are still in the lane),
// and a frame with more than the host read-back holds is copied directly once and the read-back
// grown, so that later batches come back whole through k_dets_to_host.
int harvest(rsp_plan* p, Lane& L, std::vector<std::vector<rsp_detection>>* keep_dets = nullptr) {
    if (!L.busy) return RSP_OK;
    HIPCHK(hipEventSynchronize(L.done));
    L.busy = false;
    if (L.timed) {
        for (int i = 0; i < 3; ++i) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, L.tev[i], L.tev[i + 1]));
            p->stage_ms[i] += ms;
        }
        p->stage_launches += 1;
        p->stage_frames += L.nf;
    }
    // record 0 of a frame: detections, deferred cells, edge rows computed on demand
    int cnt[RSP_MAX_F], dfc[RSP_MAX_F], erows[RSP_MAX_F], maxc = 0, rc;
    for (int f = 0; f < L.nf; ++f) {
        const int* h = reinterpret_cast<const int*>(L.h_dets + (size_t)f * (L.hcap + 1));
        cnt[f] = h[0]; dfc[f] = h[1]; erows[f] = h[2];
    }
    bool regrow = false;
    for (;;) {
        // rare: grow the device lists, run K3 again with them, read back directly.  A deferred list
        // that was too short leaves the detection count short too, so the counts are read again and
        // the detection lists may grow in a second round.
        int maxf = 0;
        maxc = 0;
        for (int f = 0; f < L.nf; ++f) {
            maxc = std::max(maxc, cnt[f]);
            maxf = std::max(maxf, dfc[f]);
        }
        const bool more_d = maxc > L.dcap, more_f = L.band && maxf > L.fcap;
        if (!more_d && !more_f) break;
        regrow = true;
        if (more_d && (rc = lane_dets_alloc(p, L, std::min(p->det_bound, pow2_at_least(maxc))))) return rc;
        if (more_f && (rc = lane_defer_alloc(p, L, std::min(p->det_bound, pow2_at_least(maxf))))) return rc;
        FramePtrs fp = L.fp;
        lane_det_ptrs(L, L.nf, fp);
        lane_band_ptrs(L, L.nf, fp);
        HIPCHK(zero_k3_state(L, L.nf));
        HIPCHK(launch_k3_lane(p, L, fp, L.nf));
        HIPCHK(hipStreamSynchronize(L.stream));
        L.fp = fp;
        for (int f = 0; f < L.nf; ++f) {
            int h[3];
            HIPCHK(hipMemcpy(h, L.dets + (size_t)(L.dcap + 1) * f, sizeof h, hipMemcpyDeviceToHost));
            cnt[f] = h[0]; dfc[f] = h[1]; erows[f] = h[2];
        }
    }
    p->ctr.frames += L.nf;
    if (L.band) {
        p->ctr.band_frames += L.nf;
        for (int f = 0; f < L.nf; ++f) {
            p->ctr.edge_rows += erows[f];
            p->ctr.deferred_cells += dfc[f];
        }
    }
    if (keep_dets) keep_dets->assign(L.nf, {});
    for (int f = 0; f < L.nf; ++f) {
        const DevDet* hrec = L.h_dets + (size_t)f * (L.hcap + 1);
        const DevDet* drec = L.dets + (size_t)(L.dcap + 1) * f;
        FrameResult fr;
        fr.frame_idx = L.frame_ids[f];
        const int n = cnt[f];
        fr.n_dets = n;
        std::vector<rsp_detection> dets(n);
        static_assert(sizeof(DevDet) == sizeof(rsp_detection), "layout");
        const int na = regrow ? 0 : std::min(n, L.hcap);   // already in host memory
        if (na) memcpy(dets.data(), hrec + 1, sizeof(DevDet) * na);
        if (n > na) HIPCHK(hipMemcpy(dets.data() + na, drec + 1 + na, sizeof(DevDet) * (n - na), hipMemcpyDeviceToHost));
        if (keep_dets || L.nf == 1) {   // synchronous frame paths: cluster here
            rsp_cluster_frame(p->cl, dets, fr.targets);
            if (keep_dets) (*keep_dets)[f] = dets;
            p->results.push_back(std::move(fr));
        } else {
            if (!p->pool) p->pool.reset(new ClusterPool(std::max(1, std::min<int>(p->F, 8))));
            p->results.push_back(std::move(fr));
            FrameResult* slot = &p->results.back();
            const rsp_cluster_params cl = p->cl;
            p->pool->submit([cl, slot, d = std::move(dets)]() mutable { rsp_cluster_frame(cl, d, slot->targets); });
        }
    }
    if (maxc > L.hcap && (rc = lane_host_alloc(p, L, std::min(p->det_bound, pow2_at_least(maxc))))) return rc;
    return RSP_OK;
}

int flush_pending(rsp_plan* p) {
    if (!p->npend) return RSP_OK;
    Lane& L = p->lanes[p->next_lane];
    int rc = harvest(p, L);
    if (rc) return rc;
    rc = launch_batch(p, L, p->pend_in, p->pend_ids, p->npend, nullptr, p->pend_slot, p->pend_rdm);
    p->npend = 0;
    p->next_lane = (p->next_lane + 1) % p->nlanes;
    return rc;
}

int drain_all(rsp_plan* p) {
    int rc = flush_pending(p);
    if (rc) return rc;
    // harvest in launch order: the lane launched first is next_lane
    for (int q = 0; q < p->nlanes; ++q) {
        rc = harvest(p, p->lanes[(p->next_lane + q) % p->nlanes]);
        if (rc) return rc;
    }
    p->results_ready();
    return RSP_OK;
}

// Next slot of the producer ring (allocated on first use); up_stream waits until the K1 that
// last read it has run.
int ring_acquire(rsp_plan* p, int* slot) {
    if (p->ring.empty()) {
        const int n = (p->nlanes + 1) * p->F;
        HIPCHK(hipStreamCreateWithFlags(&p->up_stream, hipStreamNonBlocking));
        p->ring.assign(n, nullptr);
        p->slot_ready.assign(n, nullptr);
        p->slot_free.assign(n, nullptr);
        p->slot_used.assign(n, 0);
        for (int i = 0; i < n; ++i) {
            int rc = p->dalloc_bytes(&p->ring[i], (size_t)p->g.C * p->g.cpitch * p->esz);
            if (rc) return rc;
            HIPCHK(hipEventCreateWithFlags(&p->slot_ready[i], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&p->slot_free[i], hipEventDisableTiming));
        }
    }
    const int s = p->ring_next;
    p->ring_next = (s + 1) % (int)p->ring.size();
    if (p->slot_used[s]) HIPCHK(hipStreamWaitEvent(p->up_stream, p->slot_free[s], 0));
    *slot = s;
    return RSP_OK;
}

int enqueue_frame(rsp_plan* p, const void* d_cube, int slot, int frame_idx, void* d_rdm = nullptr) {
    if (slot >= 0) {
        HIPCHK(hipEventRecord(p->slot_ready[slot], p->up_stream));
        p->slot_used[slot] = 1;
    }
    p->pend_in[p->npend] = d_cube;
    p->pend_rdm[p->npend] = d_rdm;
    p->pend_ids[p->npend] = frame_idx;
    p->pend_slot[p->npend] = slot;
    if (++p->npend == p->F) return flush_pending(p);
    return RSP_OK;
}

int ensure_stage(rsp_plan* p, size_t bytes) {
    if (p->h_stage_bytes >= bytes) return RSP_OK;
    if (p->h_stage) (void)hipHostFree(p->h_stage);
    p->h_stage = nullptr;
    HIPCHK(hipHostMalloc((void**)&p->h_stage, bytes, hipHostMallocDefault));
    p->h_stage_bytes = bytes;
    return RSP_OK;
}

// Copy a host cube (complex64 or complex128, nch channel slabs of N x P) into d_dst in the
// plan's precision (a converting copy only when the dtypes differ).
int upload_cube(rsp_plan* p, const void* cube, int dtype, int nch, void* d_dst, hipStream_t s) {
    if (dtype != RSP_C64 && dtype != RSP_C128) return fail(RSP_ERR_INVALID, "unknown dtype %d", dtype);
    const size_t slab = (size_t)p->g.N * p->g.P, elems = slab * nch;
    const bool f64 = p->g.prec == RSP_PREC_F64;
    const void* src = cube;
    if ((dtype == RSP_C128) != f64) {
        int rc = ensure_stage(p, elems * p->esz);
        if (rc) return rc;
        rsp_convert_reals(cube, dtype, 2 * elems, p->h_stage);
        src = p->h_stage;
    }
    HIPCHK(hipMemcpy2DAsync(d_dst, (size_t)p->g.cpitch * p->esz, src, slab * p->esz, slab * p->esz, nch,
                            hipMemcpyHostToDevice, s));   // channel slabs at cpitch
    HIPCHK(hipStreamSynchronize(s));   // the caller's buffer (or the staging buffer) is borrowed for the call
    return RSP_OK;
}

// n device maps [P][G] of element type S -> MATLAB column-major [P x G x n] of D (rsp_transpose_planes)
template <class S, class D>
int maps_to_matlab(const void* d_map, int P, int G, int n, D* out) {
    std::vector<S> m((size_t)n * P * G);
    HIPCHK(hipMemcpy(m.data(), d_map, m.size() * sizeof(S), hipMemcpyDeviceToHost));
    rsp_transpose_planes(m.data(), P, G, n, out);
    return RSP_OK;
}

// ... of the plan's shape and precision, widened: complex maps (the RD maps, [B]) as W = cd and
// N = cf, real ones (K3's S, [B - 1]) as double and float
template <class W, class N>
int plan_maps_to_matlab(const rsp_plan* p, const void* d_map, int n, double* out) {
    return p->g.prec == RSP_PREC_F64 ? maps_to_matlab<W>(d_map, p->g.P, p->g.G, n, (W*)out)
                                     : maps_to_matlab<N>(d_map, p->g.P, p->g.G, n, (W*)out);
}
int rdm_out(const rsp_plan* p, const void* d_map, double* out) { return plan_maps_to_matlab<cd, cf>(p, d_map, p->g.B, out); }

int run_sync_frame(rsp_plan* p, const void* d_in, int frame_idx, rsp_frame_out* out) {
    int rc = drain_all(p);
    if (rc) return rc;
    const size_t nres = p->results.size();
    Lane& L = p->lanes[0];
    const void* in[1] = {d_in};
    int ids[1] = {frame_idx};
    std::vector<std::vector<rsp_detection>> dets;
    void* smap = nullptr;
    p->smap_valid = false;   // rsp_last_cfar_threshold reads the maps of the last synchronous frame, if it asked for them
    if (out && out->cfar_maps && p->g.B > 1) {
        if (!p->d_smap && (rc = p->dalloc_bytes(&p->d_smap, (size_t)(p->g.B - 1) * p->g.P * p->g.G * p->rsz))) return rc;
        smap = p->d_smap;
    }
    void* rdm[1] = {L.rdm};
    if ((rc = launch_batch(p, L, in, ids, 1, smap, nullptr, out && out->rdm ? rdm : nullptr))) return rc;
    if ((rc = harvest(p, L, &dets))) return rc;
    p->smap_valid = smap != nullptr;
    FrameResult fr = p->results.back();
    p->results.resize(nres);   // synchronous frames do not enter the queue's result list
    p->last_dets = std::move(dets[0]);
    p->last_targets = fr.targets;
    if (out) {
        // both lists are copied and the maps written before an overflow is reported; the targets
        // first, so that with both lists short the message that stays is the detections'
        const int nt = (int)fr.targets.size(), nd = (int)p->last_dets.size();
        const int rt = rsp_capped_copy(out->targets, fr.targets.data(), nt, out->targets_cap, &out->n_targets,
                                       "%d targets exceed targets_cap %d (all of them: rsp_last_targets)", nt, out->targets_cap);
        const int rd = rsp_capped_copy(out->dets, p->last_dets.data(), nd, out->dets_cap, &out->n_dets,
                                       "%d detections exceed dets_cap %d (all of them: rsp_last_detections)", nd, out->dets_cap);
        if (out->rdm && (rc = rdm_out(p, L.rdm, out->rdm))) return rc;
        if (smap && (rc = plan_maps_to_matlab<double, float>(p, smap, p->g.B - 1, out->cfar_maps))) return rc;   // device-produced (fsf:184-187)
        return rd ? rd : rt;
    }
    return RSP_OK;
}

// A device buffer that grows on demand (the stage-3 CFAR's, the DBF's; freed with the plan)
int s3_reserve(rsp_plan::DevBuf& b, size_t bytes) {
    if (b.cap >= bytes && b.p) return RSP_OK;
    if (b.p) HIPCHK(hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
    if (hipMalloc(&b.p, bytes) != hipSuccess) {
        b.p = nullptr;
        return fail(RSP_ERR_NOMEM, "hipMalloc(%zu bytes) failed", bytes);
    }
    b.cap = bytes;
    return RSP_OK;
}

// The input of a stage-2 call: beams [P x N x B] (raw = false), or the raw cube [P x N x C] with the
// weights of its DBF (W null: the plan's) -- the scripts' DBF loop fused into the corner turn
struct Stage2In {
    const void* data;
    int dtype;
    bool raw;
    const double* W;
    int conj;
};

// The DBF A operands (K1's layout) of a raw call on the device: the plan's own table for its own
// weights conjugated; else the call's, uploaded when W or conj differ from the last raw call's
int raw_atab(rsp_plan* p, const Stage2In& in, const void** atab) {
    if (!in.W && in.conj) {
        *atab = p->k.Atab;
        return RSP_OK;
    }
    const size_t nw = 2 * (size_t)p->g.B * p->g.C;
    const double* W = in.W ? in.W : p->h_W.data();
    const bool same = p->raw_tab.p && p->raw_conj == (in.conj != 0) && p->raw_W.size() == nw &&
                      memcmp(p->raw_W.data(), W, nw * sizeof(double)) == 0;
    if (!same) {
        std::vector<double> t;
        rsp_dbf_atab(W, p->g.B, p->g.C, in.conj, DBF_ROWS_SPLIT, t);
        p->raw_W.clear();   // no key while the table is being replaced
        int rc = s3_reserve(p->raw_tab, t.size() * p->rsz);
        if (rc || (rc = p->put_reals(p->raw_tab.p, t.data(), t.size()))) return rc;
        p->raw_W.assign(W, W + nw);
        p->raw_conj = in.conj != 0;
    }
    *atab = p->raw_tab.p;
    return RSP_OK;
}

// The device half of the stage-2 calls: PC_results into lane 0's map, MTD_results into p->d_aux
// (both [B][P][G] complex in the plan's precision); returns with the stream idle.  Beams: K1
// transposes only (its input channels are the beams); a raw cube: K1 runs its DBF as well (mode 1)
// on the plan's own geometry.  K2 and k_mtd_cols are the same launches for both.
int stage2_device(rsp_plan* p, const Stage2In& in) {
    HIPCHK(hipSetDevice(p->device));
    int rc = drain_all(p);
    if (rc) return rc;
    Lane& L = p->lanes[0];
    Geometry gs = p->g;
    DevConsts ks = p->k;
    if (!in.raw) gs.C = gs.B;   // input channels are the beams; no DBF, no MTD
    else if ((rc = raw_atab(p, in, &ks.Atab))) return rc;
    if ((rc = upload_cube(p, in.data, in.dtype, gs.C, p->d_cube, L.stream))) return rc;
    if (!p->d_aux && (rc = p->dalloc_bytes(&p->d_aux, p->rdm_elems * p->esz))) return rc;
    const void* cube[1] = {p->d_cube};
    void* rdm[1] = {L.rdm};
    const FramePtrs fp = lane_ptrs(p, L, cube, 1, rdm);
    HIPCHK(launch_k1(gs, ks, fp, 1, in.raw ? 1 : 0, L.stream));
    HIPCHK(launch_k2(gs, ks, fp, 1, L.stream));                  // PC rows (b, m) -> L.rdm
    HIPCHK(launch_mtd_cols(gs, ks, L.rdm, p->d_aux, L.stream));  // S7 over pulses
    HIPCHK(hipStreamSynchronize(L.stream));
    p->aux_valid = true;
    return RSP_OK;
}
int stage2_device(rsp_plan* p, const void* iq, int dtype) { return stage2_device(p, Stage2In{iq, dtype, false, nullptr, 1}); }

// ---- stage-3 range CFAR ----
struct S3Out {   // host outputs of one CFAR call, each optional
    double* amp;
    uint8_t* flags;
    double* thr;
    rsp_stage3_hit* hits;
    int64_t hits_cap;
    int64_t* n_hits;
};

// The argument checks every CFAR entry starts with (prm: its parameter struct)
int s3_args(const rsp_plan* p, const void* in, const void* prm, int64_t hits_cap) {
    if (!p || !in || !prm) return fail(RSP_ERR_INVALID, "null argument");
    if (hits_cap < 0) return fail(RSP_ERR_INVALID, "negative hits_cap");
    return RSP_OK;
}

// A CFAR kernel on lane 0's stream over `cells` cells in all, with the device outputs the caller asks for
// (amp / thr / flags: the plan's s3 buffers, already reserved) and, with `list`, the device hit list
// p->s3_hits: count, then grow -- a run that counts more hits than the list holds grows the list to the
// count and runs once more.  launch(amp, thr, flags, hits, count, cap, stream) starts the kernel with the
// device outputs of this run (launch_s3's / launch_vcfar's trailing arguments).  Returns with the stream
// idle, *total = the hits, all of them on the device when `list`.
template <class Launch>
int cfar_launch_grow(rsp_plan* p, size_t cells, bool amp, bool thr, bool flags, bool list, Launch launch, int* total_out) {
    Lane& L = p->lanes[0];
    int rc;
    if ((rc = s3_reserve(p->s3_count, 16))) return rc;
    if (list && (rc = s3_reserve(p->s3_hits, sizeof(rsp_stage3_hit) * std::min<size_t>(cells, 65536)))) return rc;
    int total = 0;
    for (int pass = 0;; ++pass) {
        const int cap = list ? (int)std::min<size_t>(p->s3_hits.cap / sizeof(rsp_stage3_hit), (size_t)INT32_MAX) : 0;
        HIPCHK(hipMemsetAsync(p->s3_count.p, 0, 4, L.stream));
        HIPCHK(launch(amp ? (double*)p->s3_amp.p : nullptr, thr ? (double*)p->s3_thr.p : nullptr,
                      flags ? (uint8_t*)p->s3_flags.p : nullptr, list ? (rsp_stage3_hit*)p->s3_hits.p : nullptr,
                      (int*)p->s3_count.p, cap, L.stream));
        HIPCHK(hipStreamSynchronize(L.stream));
        HIPCHK(hipMemcpy(&total, p->s3_count.p, 4, hipMemcpyDeviceToHost));
        if (!list || total <= cap) break;
        if (pass > 0) return fail(RSP_ERR_DEVICE, "CFAR hit count changed between two runs on the same map");
        if ((rc = s3_reserve(p->s3_hits, sizeof(rsp_stage3_hit) * (size_t)total))) return rc;   // every hit, then again
    }
    *total_out = total;
    return RSP_OK;
}

// A CFAR kernel over n_maps device maps of P x G on lane 0's stream (cfar_launch_grow), then the requested
// outputs to the host.
template <class Launch>
int cfar_run(rsp_plan* p, int P, int G, int n_maps, const S3Out& o, Launch launch) {
    const size_t cells = (size_t)n_maps * P * G;
    int rc;
    if (o.amp && (rc = s3_reserve(p->s3_amp, cells * 8))) return rc;
    if (o.thr && (rc = s3_reserve(p->s3_thr, cells * 8))) return rc;
    if (o.flags && (rc = s3_reserve(p->s3_flags, cells))) return rc;
    const bool list = o.hits && o.hits_cap > 0;
    int total = 0;
    if ((rc = cfar_launch_grow(p, cells, o.amp != nullptr, o.thr != nullptr, o.flags != nullptr, list, launch, &total))) return rc;
    if (o.n_hits) *o.n_hits = total;
    if (o.amp && (rc = maps_to_matlab<double>(p->s3_amp.p, P, G, n_maps, o.amp))) return rc;
    if (o.thr && (rc = maps_to_matlab<double>(p->s3_thr.p, P, G, n_maps, o.thr))) return rc;
    if (o.flags && (rc = maps_to_matlab<uint8_t>(p->s3_flags.p, P, G, n_maps, o.flags))) return rc;
    if (list && total > 0) {
        std::vector<rsp_stage3_hit> h((size_t)total);   // the device list is in no order
        HIPCHK(hipMemcpy(h.data(), p->s3_hits.p, sizeof(rsp_stage3_hit) * (size_t)total, hipMemcpyDeviceToHost));
        rsp_s3_sorted_hits(h.data(), total, o.hits, o.hits_cap);
    }
    return RSP_OK;
}

// k_s3_cfar over n_maps device maps d_in (complex: the stage-2 result; else real amplitudes of the
// plan's precision)
int s3_run(rsp_plan* p, const S3Desc& d, bool cplx, const void* d_in, int n_maps, const S3Out& o) {
    return cfar_run(p, d.P, d.G, n_maps, o,
                    [&](double* amp, double* thr, uint8_t* flags, rsp_stage3_hit* hits, int* count, int cap, hipStream_t s) {
                        return launch_s3(d, p->g.prec, cplx, d_in, n_maps, amp, thr, flags, hits, count, cap, s);
                    });
}
// ... and k_vcfar
int vc_run(rsp_plan* p, const VcDesc& d, bool cplx, const void* d_in, int n_maps, const S3Out& o) {
    return cfar_run(p, d.P, d.G, n_maps, o,
                    [&](double* amp, double* thr, uint8_t* flags, rsp_stage3_hit* hits, int* count, int cap, hipStream_t s) {
                        return launch_vcfar(d, p->g.prec, cplx, d_in, n_maps, amp, thr, flags, hits, count, cap, s);
                    });
}

// ... and k_xcfar
int xc_run(rsp_plan* p, const XcDesc& d, bool cplx, const void* d_in, int n_maps, const S3Out& o) {
    return cfar_run(p, d.P, d.G, n_maps, o,
                    [&](double* amp, double* thr, uint8_t* flags, rsp_stage3_hit* hits, int* count, int cap, hipStream_t s) {
                        return launch_xcfar(d, p->g.prec, cplx, d_in, n_maps, amp, thr, flags, hits, count, cap, s);
                    });
}

int s3_fused(rsp_plan* p, const Stage2In& in, const rsp_stage3_cfar_params* prm, double* mtd_out, const S3Out& o) {
    S3Desc d;
    int rc = rsp_stage3_derive(p->g.P, p->gates, prm, &d);   // refusals before any device work
    if (rc || (rc = rsp_s3_check_cells(d.P, d.G, p->g.B)) || (rc = stage2_device(p, in))) return rc;
    if (mtd_out && (rc = rdm_out(p, p->d_aux, mtd_out))) return rc;
    return s3_run(p, d, true, p->d_aux, p->g.B, o);
}

int vc_fused(rsp_plan* p, const Stage2In& in, const rsp_vcfar_params* prm, double* mtd_out, const S3Out& o) {
    VcDesc d;
    int rc = rsp_vcfar_derive(p->g.P, p->g.G, prm, &d);   // refusals before any device work
    if (rc || (rc = rsp_s3_check_cells(d.P, d.G, p->g.B)) || (rc = stage2_device(p, in))) return rc;
    if (mtd_out && (rc = rdm_out(p, p->d_aux, mtd_out))) return rc;
    return vc_run(p, d, true, p->d_aux, p->g.B, o);
}

int xc_fused(rsp_plan* p, const Stage2In& in, const rsp_cfar_params* prm, double* mtd_out, const S3Out& o) {
    XcDesc d;
    int rc = rsp_xcfar_derive(p->g.P, p->g.G, prm, &d);   // refusals before any device work
    if (rc || (rc = rsp_s3_check_cells(d.P, d.G, p->g.B)) || (rc = stage2_device(p, in))) return rc;
    if (mtd_out && (rc = rdm_out(p, p->d_aux, mtd_out))) return rc;
    return xc_run(p, d, true, p->d_aux, p->g.B, o);
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

// The three timed forms of a CFAR kernel over the B beams of the plan's last stage-2 result (what
// rsp_profile_stage3 documents).  launch(cplx, in, amp, thr, flags, hits, count, cap, stream) starts the kernel.
template <class Launch>
int cfar_profile(rsp_plan* p, int P, int G, int iters, float* ms_out, int64_t* bytes_out, Launch launch) {
    if (!p->aux_valid) return fail(RSP_ERR_INVALID, "no stage-2 result on the device: call rsp_process_stage2 first");
    HIPCHK(hipSetDevice(p->device));
    int rc;
    if ((rc = drain_all(p))) return rc;
    Lane& L = p->lanes[0];
    const int B = p->g.B;
    const size_t cells = (size_t)B * P * G, rs = p->rsz;
    if ((rc = s3_reserve(p->s3_amp, cells * 8)) || (rc = s3_reserve(p->s3_thr, cells * 8)) ||
        (rc = s3_reserve(p->s3_flags, cells)) || (rc = s3_reserve(p->s3_count, 16)) || (rc = s3_reserve(p->s3_in, cells * rs)) ||
        (rc = s3_reserve(p->s3_hits, sizeof(rsp_stage3_hit) * std::min<size_t>(cells, 65536))))
        return rc;
    double* amp = (double*)p->s3_amp.p;
    double* thr = (double*)p->s3_thr.p;
    uint8_t* fl = (uint8_t*)p->s3_flags.p;
    rsp_stage3_hit* hits = (rsp_stage3_hit*)p->s3_hits.p;
    int* cnt = (int*)p->s3_count.p;
    const int cap = (int)std::min<size_t>(p->s3_hits.cap / sizeof(rsp_stage3_hit), (size_t)INT32_MAX);
    {   // the real form's input: the magnitudes the complex form writes, in the plan's precision
        HIPCHK(hipMemsetAsync(cnt, 0, 4, L.stream));
        HIPCHK(launch(true, p->d_aux, amp, nullptr, nullptr, nullptr, cnt, 0, L.stream));
        HIPCHK(hipStreamSynchronize(L.stream));
        std::vector<double> a(cells);
        HIPCHK(hipMemcpy(a.data(), amp, cells * 8, hipMemcpyDeviceToHost));
        if ((rc = p->put_reals(p->s3_in.p, a.data(), cells))) return rc;
    }
    for (int s = 0; s < 3; ++s) {
        auto run = [&]() -> hipError_t {
            hipError_t e = hipMemsetAsync(cnt, 0, 4, L.stream);
            if (e != hipSuccess) return e;
            if (s == 0) return launch(false, p->s3_in.p, nullptr, thr, fl, nullptr, cnt, 0, L.stream);
            if (s == 1) return launch(true, p->d_aux, amp, thr, fl, nullptr, cnt, 0, L.stream);
            return launch(true, p->d_aux, nullptr, nullptr, nullptr, hits, cnt, cap, L.stream);
        };
        float ms = 0;
        if ((rc = time_launches(L.stream, iters, [&]() -> int { HIPCHK(run()); return RSP_OK; }, &ms))) return rc;
        if (ms_out) ms_out[s] = ms;
    }
    if (bytes_out) rsp_stage3_bytes((int64_t)cells, (int)p->esz, bytes_out);
    return RSP_OK;
}

const char* kStageNames[] = {"k1_dbf_mtd", "k2_pc", "k3_cfar"};

}  // namespace

// =========================================================================================
extern "C" {

const char* rsp_stage_name(int32_t s) { return (s >= 0 && s < 3) ? kStageNames[s] : "?"; }

int32_t rsp_plan_options_default(rsp_plan_options* o) {
    if (!o) return fail(RSP_ERR_INVALID, "null argument");
    o->device = 0;
    o->frames_per_launch = 1;
    o->precision = RSP_C128;
    o->flags = 0;
    return RSP_OK;
}

int32_t rsp_plan_create(const rsp_sig_config* cfg, const rsp_cfar_params* cfar, const rsp_cluster_params* cluster,
                        const rsp_precomputed* pre, int32_t device, int32_t frames_per_launch, rsp_plan** out) {
    rsp_plan_options o;
    rsp_plan_options_default(&o);
    o.device = device;
    o.frames_per_launch = frames_per_launch;
    return rsp_plan_create_ex(cfg, cfar, cluster, pre, &o, out);
}

int32_t rsp_plan_create_ex(const rsp_sig_config* cfg, const rsp_cfar_params* cfar, const rsp_cluster_params* cluster,
                           const rsp_precomputed* pre, const rsp_plan_options* opt, rsp_plan** out) {
    if (!cfg || !cfar || !cluster || !pre || !opt || !out) return fail(RSP_ERR_INVALID, "null argument");
    *out = nullptr;
    int rc = rsp_plan_check_args(cfg, cfar, cluster, pre, opt);
    if (rc) return rc;
    const int device = opt->device;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(RSP_ERR_DEVICE, "no HIP device available");
    if (device < 0 || device >= ndev) return fail(RSP_ERR_INVALID, "device %d out of range (%d devices)", device, ndev);
    HIPCHK(hipSetDevice(device));
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) ncu = 0;
    PlanHost h;   // every size, route input and table, derived without the device (rsp_geometry.cpp)
    if ((rc = rsp_plan_derive(cfg, cfar, cluster, pre, opt, ncu, &h))) return rc;

    rsp_plan* p = new rsp_plan();
    auto bail = [&](int rc) { delete p; return rc; };
    p->device = device;
    p->F = opt->frames_per_launch;
    p->cl = *cluster;
    p->sc = SynthConsts{cfg->c, cfg->fs, cfg->wavelength, cfg->element_spacing, cfg->prt, pre->P_signal_unscaled};
    p->esz = opt->precision == RSP_C128 ? 16 : 8;
    p->rsz = p->esz / 2;
    p->g = h.g;
    p->det_bound = h.det_bound;
    p->z_elems = h.z_elems; p->rdm_elems = h.rdm_elems; p->mag_elems = h.mag_elems;
    p->h_W.assign(pre->DBF_coeffs_data_C, pre->DBF_coeffs_data_C + 2 * (size_t)h.g.B * h.g.C);
    p->gates[0] = pre->N_gate_narrow; p->gates[1] = pre->N_gate_medium; p->gates[2] = pre->N_gate_long;

    // ---- constants to the device, in the plan's precision
    DevConsts& k = p->k;
    double *dra, *dva, *dang, *dkl;
    K2Rec* drec;
    if ((rc = p->upload_r(&k.Atab, h.atab)) || (rc = p->upload_c(&k.twP, h.twP)) || (rc = p->upload_c(&k.twPp, h.twPp)) ||
        (rc = p->upload_c(&k.twD, h.twD)) || (rc = p->upload_c(&k.twQ, h.twQ)) || (rc = p->upload_r(&k.win, h.win)) ||
        (rc = p->upload_r(&k.taps, h.taps)) || (rc = p->upload_c(&k.H, h.H)) || (rc = p->upload_c(&k.twM, h.twM)) ||
        (rc = p->upload(&dra, h.range_axis)) || (rc = p->upload(&dva, h.velocity_axis)) ||
        (rc = p->upload(&dang, h.beam_angles)) || (rc = p->upload(&dkl, h.klut)) || (rc = p->upload(&drec, h.k2rec)))
        return bail(rc);
    k.range_axis = dra; k.velocity_axis = dva; k.beam_angles = dang; k.klut = dkl;
    k.k2rec = drec;
    p->k2rec = std::move(h.k2rec);
    for (int w = 0; w < 3; ++w) p->k2rows[w] = h.k2rows[w];
    p->band_ok = !(opt->flags & RSP_PLAN_K2_ALL_ROWS) && h.k2rows[K2SET_BAND].n > 0 && !h.g.mono_c && h.g.B >= 2 &&
                 h.g.B <= RSP_NEED_BMAX;
    if (h.k2rows[K2SET_BAND].n > 0) {
        K2Rec *db, *de;
        if ((rc = p->upload(&db, h.k2rec_band)) || (rc = p->upload(&de, h.k2rec_edge))) return bail(rc);
        p->drec_band = db;
        p->drec_edge = de;
        p->k2rec_band = std::move(h.k2rec_band);
        p->k2rec_edge = std::move(h.k2rec_edge);
    }
    k.deltaR = pre->deltaR; k.deltaV = pre->deltaV;
    const Geometry& g = p->g;
    if (pre->tx_pulse) {
        std::vector<double> tx(pre->tx_pulse, pre->tx_pulse + 2 * (size_t)g.N);
        if ((rc = p->upload(&p->d_tx, tx))) return bail(rc);
    }
    if ((rc = p->dalloc(&p->d_stab, (size_t)2 * RSP_MAX_SYNTH_TARGETS * (g.P + g.C)))) return bail(rc);
    if ((rc = p->dalloc_bytes(&p->d_cube, (size_t)std::max(g.C, g.B) * g.cpitch * p->esz))) return bail(rc);
    for (auto& L : p->lanes)
        if ((rc = setup_lane(p, L))) return bail(rc);
    *out = p;
    return RSP_OK;
}

int32_t rsp_set_stage_timing(rsp_plan* p, int32_t on) {
    if (!p) return fail(RSP_ERR_INVALID, "null plan");
    p->time_stages = on != 0;
    for (double& v : p->stage_ms) v = 0;
    p->stage_launches = p->stage_frames = 0;
    return RSP_OK;
}

int32_t rsp_stage_times(const rsp_plan* p, double* ms_sum, int32_t cap, int64_t* launches, int64_t* frames) {
    if (!p || !ms_sum || cap < 0) return fail(RSP_ERR_INVALID, "bad argument");
    for (int i = 0; i < std::min(cap, 3); ++i) ms_sum[i] = p->stage_ms[i];
    if (launches) *launches = p->stage_launches;
    if (frames) *frames = p->stage_frames;
    return RSP_OK;
}

int32_t rsp_plan_destroy(rsp_plan* plan) {
    delete plan;
    return RSP_OK;
}

int32_t rsp_query_sizes(const rsp_plan* p, rsp_sizes* s) {
    if (!p || !s) return fail(RSP_ERR_INVALID, "null argument");
    rsp_fill_sizes(p->g, p->det_bound, s);
    return RSP_OK;
}

int32_t rsp_query_k1_route(const rsp_plan* p, rsp_k1_route* out) {
    if (!p || !out) return fail(RSP_ERR_INVALID, "null argument");
    rsp_fill_k1_route(p->g, out);
    return RSP_OK;
}

int32_t rsp_query_k3_tiling(const rsp_plan* p, rsp_k3_tiling* out) {
    if (!p || !out) return fail(RSP_ERR_INVALID, "null argument");
    rsp_fill_k3_tiling(p->g, out);
    return RSP_OK;
}

int32_t rsp_query_k2_layout(const rsp_plan* p, rsp_k2_layout* out) {
    if (!p || !out) return fail(RSP_ERR_INVALID, "null argument");
    rsp_fill_k2_layout(p->g, p->gates, out);
    return RSP_OK;
}

int32_t rsp_query_k2_records(const rsp_plan* p, rsp_k2_record* out, int32_t cap, int32_t* n) {
    if (!p) return fail(RSP_ERR_INVALID, "null argument");
    return rsp_fill_k2_records(p->k2rec, out, cap, n);
}

int32_t rsp_query_k2_row_set(const rsp_plan* p, int32_t which, rsp_k2_row_set* set, rsp_k2_record* out, int32_t cap,
                             int32_t* n) {
    if (!p) return fail(RSP_ERR_INVALID, "null argument");
    const std::vector<K2Rec>* const rec[3] = {&p->k2rec, &p->k2rec_band, &p->k2rec_edge};
    return rsp_fill_k2_row_set(p->k2rows, rec, which, set, out, cap, n);
}

int32_t rsp_band_counters_get(const rsp_plan* p, rsp_band_counters* out) {
    if (!p || !out) return fail(RSP_ERR_INVALID, "null argument");
    *out = p->ctr;
    return RSP_OK;
}

int32_t rsp_band_counters_reset(rsp_plan* p) {
    if (!p) return fail(RSP_ERR_INVALID, "null argument");
    p->ctr = rsp_band_counters{};
    return RSP_OK;
}

int32_t rsp_process_cube(rsp_plan* p, const void* cube, int32_t dtype, int32_t layout, int32_t frame_idx,
                         rsp_frame_out* out) {
    if (!p || !cube) return fail(RSP_ERR_INVALID, "null argument");
    if (layout != RSP_LAYOUT_PNC) return fail(RSP_ERR_UNSUPPORTED, "layout %d", layout);
    HIPCHK(hipSetDevice(p->device));
    int rc = drain_all(p);
    if (rc) return rc;
    if ((rc = upload_cube(p, cube, dtype, p->g.C, p->d_cube, p->lanes[0].stream))) return rc;
    return run_sync_frame(p, p->d_cube, frame_idx, out);
}

static int synth_into(rsp_plan* p, const rsp_target_in* t, int nt, int frame_idx, uint64_t seed, double p_noise,
                      void* d_cube, hipStream_t s, bool sync) {
    if (!p->d_tx) return fail(RSP_ERR_INVALID, "plan has no tx_pulse (synthesis path needs precomputed_data.tx_pulse)");
    if (nt < 0 || nt > RSP_MAX_SYNTH_TARGETS)
        return fail(RSP_ERR_INVALID, "0..%d targets supported, got %d", RSP_MAX_SYNTH_TARGETS, nt);
    SynthTargets tg;
    rsp_synth_targets(p->sc, t, nt, p_noise, &tg);
    // the targets travel in the kernel arguments; the phasor tables are rewritten in stream order
    HIPCHK(launch_synth(p->g, p->d_tx, tg, nt, p->d_stab, frame_idx, seed, std::sqrt(p_noise / 2.0), d_cube, s));
    if (sync) HIPCHK(hipStreamSynchronize(s));   // the caller may read the cube from another stream
    return RSP_OK;
}

int32_t rsp_synthesize_device(rsp_plan* p, const rsp_target_in* t, int32_t nt, int32_t frame_idx, uint64_t seed,
                              double p_noise, void* d_cube) {
    if (!p || (!t && nt) || !d_cube) return fail(RSP_ERR_INVALID, "null argument");
    HIPCHK(hipSetDevice(p->device));
    return synth_into(p, t, nt, frame_idx, seed, p_noise, d_cube, p->lanes[0].stream, true);
}

int32_t rsp_profile_synthesis(rsp_plan* p, const rsp_target_in* t, int32_t nt, int32_t iters, void* d_cube,
                              float* ms_out, int64_t* bytes_out) {
    if (!p || (!t && nt) || !d_cube || iters < 1 || !ms_out) return fail(RSP_ERR_INVALID, "bad argument");
    HIPCHK(hipSetDevice(p->device));
    int rc = drain_all(p);
    if (rc) return rc;
    hipStream_t s = p->lanes[0].stream;
    int k = 0;   // frame 1 warms up, then frames 1 .. iters
    auto run = [&] { return synth_into(p, t, nt, std::max(k++, 1), 20250101, 1.0, d_cube, s, false); };
    if ((rc = time_launches(s, iters, run, ms_out))) return rc;
    if (bytes_out) *bytes_out = (int64_t)p->g.C * p->g.N * p->g.P * (int64_t)p->esz;
    return RSP_OK;
}

int32_t rsp_process_targets(rsp_plan* p, const rsp_target_in* t, int32_t nt, int32_t frame_idx, uint64_t seed,
                            double p_noise, rsp_frame_out* out) {
    if (!p || (!t && nt)) return fail(RSP_ERR_INVALID, "null argument");
    HIPCHK(hipSetDevice(p->device));
    int rc = drain_all(p);
    if (rc) return rc;
    // the frame runs on the same stream: no host synchronisation in between
    if ((rc = synth_into(p, t, nt, frame_idx, seed, p_noise, p->d_cube, p->lanes[0].stream, false))) return rc;
    return run_sync_frame(p, p->d_cube, frame_idx, out);
}

int32_t rsp_enqueue_device(rsp_plan* p, const void* d_cube, int32_t frame_idx) {
    if (!p || !d_cube) return fail(RSP_ERR_INVALID, "null argument");
    HIPCHK(hipSetDevice(p->device));   // a host thread may drive plans on several devices
    return enqueue_frame(p, d_cube, -1, frame_idx);
}

int32_t rsp_enqueue_device_n(rsp_plan* p, const void* const* d_cubes, const int32_t* frame_idx, int32_t n) {
    if (!p || (n > 0 && (!d_cubes || !frame_idx)) || n < 0) return fail(RSP_ERR_INVALID, "bad argument");
    HIPCHK(hipSetDevice(p->device));
    for (int i = 0; i < n; ++i)   // all or nothing: no frame is queued when any pointer is bad
        if (!d_cubes[i]) return fail(RSP_ERR_INVALID, "cube %d is null", i);
    for (int i = 0; i < n; ++i) {
        int rc = enqueue_frame(p, d_cubes[i], -1, frame_idx[i]);
        if (rc) return rc;
    }
    return RSP_OK;
}

int32_t rsp_enqueue_device_rdm(rsp_plan* p, const void* d_cube, int32_t frame_idx, void* d_rdm) {
    if (!p || !d_cube || !d_rdm) return fail(RSP_ERR_INVALID, "null argument");
    HIPCHK(hipSetDevice(p->device));
    return enqueue_frame(p, d_cube, -1, frame_idx, d_rdm);
}

int32_t rsp_enqueue_device_rdm_n(rsp_plan* p, const void* const* d_cubes, const int32_t* frame_idx, void* const* d_rdms,
                                 int32_t n) {
    if (!p || (n > 0 && (!d_cubes || !frame_idx || !d_rdms)) || n < 0) return fail(RSP_ERR_INVALID, "bad argument");
    HIPCHK(hipSetDevice(p->device));
    for (int i = 0; i < n; ++i)   // all or nothing: no frame is queued when any pointer is bad
        if (!d_cubes[i] || !d_rdms[i]) return fail(RSP_ERR_INVALID, "cube or map %d is null", i);
    for (int i = 0; i < n; ++i) {
        int rc = enqueue_frame(p, d_cubes[i], -1, frame_idx[i], d_rdms[i]);
        if (rc) return rc;
    }
    return RSP_OK;
}

int32_t rsp_enqueue_host(rsp_plan* p, const void* h_cube, int32_t dtype, int32_t frame_idx) {
    if (!p || !h_cube) return fail(RSP_ERR_INVALID, "null argument");
    if (dtype != (p->g.prec == RSP_PREC_F64 ? RSP_C128 : RSP_C64))
        return fail(RSP_ERR_INVALID, "rsp_enqueue_host: dtype %d differs from the plan precision (rsp_process_cube converts)",
                    dtype);
    HIPCHK(hipSetDevice(p->device));
    int s, rc;
    if ((rc = ring_acquire(p, &s))) return rc;
    // only the fast-time samples the chain reads (Geometry::ivl_*): per interval, the channel
    // slabs' [lo, lo + len) x P block, pitch N P
    const Geometry& g = p->g;
    const size_t row = (size_t)g.P * p->esz;
    for (int q = 0; q < g.nivl; ++q) {
        const int len = (q + 1 < g.nivl ? g.ivl_start[q + 1] : g.nU) - g.ivl_start[q];
        const size_t off = (size_t)g.ivl_lo[q] * row;
        HIPCHK(hipMemcpy2DAsync((char*)p->ring[s] + off, (size_t)g.cpitch * p->esz, (const char*)h_cube + off,
                                (size_t)g.N * row, (size_t)len * row, g.C, hipMemcpyHostToDevice, p->up_stream));
    }
    return enqueue_frame(p, p->ring[s], s, frame_idx);
}

int32_t rsp_host_alloc(rsp_plan* p, int64_t bytes, void** h_ptr) {
    if (!p || !h_ptr || bytes <= 0) return fail(RSP_ERR_INVALID, "bad argument");
    HIPCHK(hipSetDevice(p->device));
    *h_ptr = nullptr;
    if (hipHostMalloc(h_ptr, (size_t)bytes, hipHostMallocDefault) != hipSuccess)
        return fail(RSP_ERR_NOMEM, "hipHostMalloc(%lld bytes) failed", (long long)bytes);
    return RSP_OK;
}

int32_t rsp_host_free(rsp_plan* p, void* h_ptr) {
    if (!p) return fail(RSP_ERR_INVALID, "null argument");
    if (h_ptr) HIPCHK(hipHostFree(h_ptr));
    return RSP_OK;
}

int32_t rsp_process_targets_multi(rsp_plan* const* plans, int32_t n_plans, const rsp_target_in* const* targets,
                                  const int32_t* n_targets, const int32_t* frame_idx, int32_t n_frames, uint64_t seed,
                                  double p_noise, rsp_target* out, int32_t cap, int32_t* n_out) {
    if (!plans || n_plans < 1 || !targets || !n_targets || !frame_idx || n_frames < 0 || !out || cap < 0 || !n_out)
        return fail(RSP_ERR_INVALID, "bad argument");
    for (int i = 0; i < n_plans; ++i) {
        if (!plans[i]) return fail(RSP_ERR_INVALID, "plan %d is null", i);
        for (int j = 0; j < i; ++j)
            if (plans[j] == plans[i]) return fail(RSP_ERR_INVALID, "plan %d listed twice (one host thread per plan)", i);
        plans[i]->results_ready();
        if (!plans[i]->results.empty() || plans[i]->npend)
            return fail(RSP_ERR_INVALID, "plan %d has queued frames or uncleared results", i);
    }
    struct Work { int rc = RSP_OK; std::string err; };
    std::vector<Work> work(n_plans);
    auto run = [&](int i) {
        rsp_plan* p = plans[i];
        const int f0 = (int)((int64_t)n_frames * i / n_plans), f1 = (int)((int64_t)n_frames * (i + 1) / n_plans);
        auto body = [&]() -> int {
            HIPCHK(hipSetDevice(p->device));
            int rc;
            for (int j = f0; j < f1; ++j) {
                int s;
                if ((rc = ring_acquire(p, &s))) return rc;
                if ((rc = synth_into(p, targets[j], n_targets[j], frame_idx[j], seed, p_noise, p->ring[s], p->up_stream,
                                  false)))   // slot_ready orders K1 after it
                    return rc;
                if ((rc = enqueue_frame(p, p->ring[s], s, frame_idx[j]))) return rc;
            }
            if ((rc = drain_all(p))) return rc;
            for (int j = f0; j < f1; ++j) {   // results come back in enqueue order
                const FrameResult& r = p->results[j - f0];
                const int nt = (int)r.targets.size();
                if ((rc = rsp_capped_copy(out + (size_t)j * cap, r.targets.data(), nt, cap, n_out + j,
                                          "frame %d: %d targets > cap %d", frame_idx[j], nt, cap)))
                    return rc;
            }
            p->results.clear();
            return RSP_OK;
        };
        work[i].rc = body();
        if (work[i].rc) {
            // leave the plan reusable: finish what was queued, then drop the partial share
            work[i].err = rsp_last_error();
            (void)drain_all(p);
            p->npend = 0;
            p->results.clear();
        }
    };
    std::vector<std::thread> th;
    for (int i = 1; i < n_plans; ++i) th.emplace_back(run, i);
    run(0);
    for (auto& t : th) t.join();
    for (int i = 0; i < n_plans; ++i)
        if (work[i].rc) return fail(work[i].rc, "plan %d (device %d): %s", i, plans[i]->device, work[i].err.c_str());
    return RSP_OK;
}

int32_t rsp_drain(rsp_plan* p) {
    if (!p) return fail(RSP_ERR_INVALID, "null argument");
    HIPCHK(hipSetDevice(p->device));
    return drain_all(p);
}

int32_t rsp_last_detections(const rsp_plan* p, rsp_detection* dets, int32_t cap, int32_t* n) {
    if (!p || !n || cap < 0 || (cap > 0 && !dets)) return fail(RSP_ERR_INVALID, "bad argument");
    const int m = (int)p->last_dets.size();
    return rsp_capped_copy(dets, p->last_dets.data(), m, cap, n, "%d detections > cap %d", m, cap);
}

int32_t rsp_last_targets(const rsp_plan* p, rsp_target* targets, int32_t cap, int32_t* n) {
    if (!p || !n || cap < 0 || (cap > 0 && !targets)) return fail(RSP_ERR_INVALID, "bad argument");
    const int m = (int)p->last_targets.size();
    return rsp_capped_copy(targets, p->last_targets.data(), m, cap, n, "%d targets > cap %d", m, cap);
}

int32_t rsp_results_count(const rsp_plan* p, int32_t* n_frames, int64_t* n_targets) {
    if (!p) return fail(RSP_ERR_INVALID, "null argument");
    p->results_ready();
    int64_t nt = 0;
    for (auto& r : p->results) nt += (int64_t)r.targets.size();
    if (n_frames) *n_frames = (int32_t)p->results.size();
    if (n_targets) *n_targets = nt;
    return RSP_OK;
}

int32_t rsp_results_get(const rsp_plan* p, int32_t i, int32_t* frame_idx, rsp_target* targets, int32_t cap,
                        int32_t* n_targets, int32_t* n_dets) {
    if (!p) return fail(RSP_ERR_INVALID, "null argument");
    p->results_ready();
    if (i < 0 || i >= (int)p->results.size()) return fail(RSP_ERR_INVALID, "result index out of range");
    const FrameResult& r = p->results[i];
    if (frame_idx) *frame_idx = r.frame_idx;
    if (n_dets) *n_dets = r.n_dets;
    return rsp_capped_copy(targets, r.targets.data(), (int64_t)r.targets.size(), cap, n_targets, "cap too small");
}

int32_t rsp_results_rows(const rsp_plan* p, double* rows, int64_t cap, int64_t* n_rows) {
    if (!p || !n_rows) return fail(RSP_ERR_INVALID, "bad argument");
    p->results_ready();
    int64_t n = 0;
    for (const FrameResult& r : p->results) rsp_result_rows(r.frame_idx, r.targets.data(), r.targets.size(), rows, cap, &n);
    *n_rows = n;
    if (rows && n > cap) return fail(RSP_ERR_OVERFLOW, "%lld rows > cap %lld", (long long)n, (long long)cap);
    return RSP_OK;   // rows == NULL: a size query
}

int32_t rsp_results_clear(rsp_plan* p) {
    if (!p) return fail(RSP_ERR_INVALID, "null argument");
    p->results_ready();
    p->results.clear();
    return RSP_OK;
}

int32_t rsp_process_stage2(rsp_plan* p, const void* iq, int32_t dtype, double* mtd_out, double* pc_out) {
    if (!p || !iq) return fail(RSP_ERR_INVALID, "null argument");
    int rc = stage2_device(p, iq, dtype);
    if (rc) return rc;
    if (pc_out && (rc = rdm_out(p, p->lanes[0].rdm, pc_out))) return rc;
    if (mtd_out && (rc = rdm_out(p, p->d_aux, mtd_out))) return rc;
    return RSP_OK;
}

int32_t rsp_process_stage2_gated(rsp_plan* p, const void* iq, int32_t dtype, int32_t n_gated, const int32_t* cols,
                                 double* mtd_out, double* pc_out) {
    if (!p || !iq) return fail(RSP_ERR_INVALID, "null argument");
    std::vector<unsigned char> full;
    int rc = rsp_stage2_regate(p->g.P, p->g.N, p->g.B, iq, dtype, n_gated, cols, full);
    if (rc) return rc;
    return rsp_process_stage2(p, full.data(), dtype, mtd_out, pc_out);
}

int32_t rsp_stage3_cfar_shape(rsp_plan* p, int32_t P, const int32_t* gates, const double* amp, int32_t n_maps,
                              const rsp_stage3_cfar_params* prm, uint8_t* flags, double* threshold, rsp_stage3_hit* hits,
                              int64_t hits_cap, int64_t* n_hits) {
    S3Desc d;
    int rc = s3_args(p, gates && amp ? amp : nullptr, prm, hits_cap);
    if (rc || (rc = rsp_stage3_derive(P, gates, prm, &d))) return rc;   // refusals before any device work
    if ((rc = rsp_s3_check_cells(d.P, d.G, n_maps))) return rc;
    HIPCHK(hipSetDevice(p->device));
    if ((rc = drain_all(p))) return rc;
    // MATLAB column-major [P x G x n] -> [n][P][G] in the plan's precision
    const size_t cells = (size_t)n_maps * d.P * d.G, rs = p->rsz;
    std::vector<unsigned char> host(cells * rs);
    if (rs == 8) rsp_transpose_planes(amp, d.G, d.P, n_maps, reinterpret_cast<double*>(host.data()));
    else rsp_transpose_planes(amp, d.G, d.P, n_maps, reinterpret_cast<float*>(host.data()));
    if ((rc = s3_reserve(p->s3_in, cells * rs))) return rc;
    HIPCHK(hipMemcpy(p->s3_in.p, host.data(), cells * rs, hipMemcpyHostToDevice));
    const S3Out o{nullptr, flags, threshold, hits, hits_cap, n_hits};
    return s3_run(p, d, false, p->s3_in.p, n_maps, o);
}

int32_t rsp_stage3_cfar(rsp_plan* p, const double* amp, int32_t n_maps, const rsp_stage3_cfar_params* prm, uint8_t* flags,
                        double* threshold, rsp_stage3_hit* hits, int64_t hits_cap, int64_t* n_hits) {
    if (!p) return fail(RSP_ERR_INVALID, "null argument");
    return rsp_stage3_cfar_shape(p, p->g.P, p->gates, amp, n_maps, prm, flags, threshold, hits, hits_cap, n_hits);
}

int32_t rsp_process_stage2_cfar(rsp_plan* p, const void* iq, int32_t dtype, const rsp_stage3_cfar_params* prm,
                                double* mtd_out, double* amp_out, uint8_t* flags, double* threshold, rsp_stage3_hit* hits,
                                int64_t hits_cap, int64_t* n_hits) {
    const int rc = s3_args(p, iq, prm, hits_cap);
    return rc ? rc : s3_fused(p, Stage2In{iq, dtype, false, nullptr, 1}, prm, mtd_out, S3Out{amp_out, flags, threshold, hits, hits_cap, n_hits});
}

int32_t rsp_process_stage2_gated_cfar(rsp_plan* p, const void* iq, int32_t dtype, int32_t n_gated, const int32_t* cols,
                                      const rsp_stage3_cfar_params* prm, double* mtd_out, double* amp_out, uint8_t* flags,
                                      double* threshold, rsp_stage3_hit* hits, int64_t hits_cap, int64_t* n_hits) {
    S3Desc d;
    int rc = s3_args(p, iq, prm, hits_cap);
    if (rc || (rc = rsp_stage3_derive(p->g.P, p->gates, prm, &d))) return rc;   // before the re-insertion's work too
    std::vector<unsigned char> full;
    if ((rc = rsp_stage2_regate(p->g.P, p->g.N, p->g.B, iq, dtype, n_gated, cols, full))) return rc;
    const S3Out o{amp_out, flags, threshold, hits, hits_cap, n_hits};
    return s3_fused(p, Stage2In{full.data(), dtype, false, nullptr, 1}, prm, mtd_out, o);
}

int32_t rsp_profile_stage3(rsp_plan* p, const rsp_stage3_cfar_params* prm, int32_t iters, float* ms_out, int64_t* bytes_out) {
    if (!p || !prm || iters < 1) return fail(RSP_ERR_INVALID, "bad argument");
    S3Desc d;
    int rc = rsp_stage3_derive(p->g.P, p->gates, prm, &d);
    if (rc || (rc = rsp_s3_check_cells(d.P, d.G, p->g.B))) return rc;
    const int B = p->g.B;
    return cfar_profile(p, d.P, d.G, iters, ms_out, bytes_out,
                        [&](bool cplx, const void* in, double* amp, double* thr, uint8_t* fl, rsp_stage3_hit* hits, int* cnt,
                            int cap, hipStream_t st) { return launch_s3(d, p->g.prec, cplx, in, B, amp, thr, fl, hits, cnt, cap, st); });
}

int32_t rsp_vcfar(rsp_plan* p, int32_t P, int32_t G, const double* amp, int32_t n_maps, const rsp_vcfar_params* prm,
                  uint8_t* flags, double* threshold, rsp_stage3_hit* hits, int64_t hits_cap, int64_t* n_hits) {
    VcDesc d;
    int rc = s3_args(p, amp, prm, hits_cap);
    if (rc || (rc = rsp_vcfar_derive(P, G, prm, &d))) return rc;   // refusals before any device work
    if ((rc = rsp_s3_check_cells(d.P, d.G, n_maps))) return rc;
    HIPCHK(hipSetDevice(p->device));
    if ((rc = drain_all(p))) return rc;
    // MATLAB column-major [P x G x n] -> [n][P][G] in the plan's precision
    const size_t cells = (size_t)n_maps * d.P * d.G, rs = p->rsz;
    std::vector<unsigned char> host(cells * rs);
    if (rs == 8) rsp_transpose_planes(amp, d.G, d.P, n_maps, reinterpret_cast<double*>(host.data()));
    else rsp_transpose_planes(amp, d.G, d.P, n_maps, reinterpret_cast<float*>(host.data()));
    if ((rc = s3_reserve(p->s3_in, cells * rs))) return rc;
    HIPCHK(hipMemcpy(p->s3_in.p, host.data(), cells * rs, hipMemcpyHostToDevice));
    const S3Out o{nullptr, flags, threshold, hits, hits_cap, n_hits};
    return vc_run(p, d, false, p->s3_in.p, n_maps, o);
}

int32_t rsp_process_stage2_vcfar(rsp_plan* p, const void* iq, int32_t dtype, const rsp_vcfar_params* prm, double* mtd_out,
                                 double* amp_out, uint8_t* flags, double* threshold, rsp_stage3_hit* hits, int64_t hits_cap,
                                 int64_t* n_hits) {
    const int rc = s3_args(p, iq, prm, hits_cap);
    return rc ? rc : vc_fused(p, Stage2In{iq, dtype, false, nullptr, 1}, prm, mtd_out, S3Out{amp_out, flags, threshold, hits, hits_cap, n_hits});
}

int32_t rsp_process_stage2_gated_vcfar(rsp_plan* p, const void* iq, int32_t dtype, int32_t n_gated, const int32_t* cols,
                                       const rsp_vcfar_params* prm, double* mtd_out, double* amp_out, uint8_t* flags,
                                       double* threshold, rsp_stage3_hit* hits, int64_t hits_cap, int64_t* n_hits) {
    VcDesc d;
    int rc = s3_args(p, iq, prm, hits_cap);
    if (rc || (rc = rsp_vcfar_derive(p->g.P, p->g.G, prm, &d))) return rc;   // before the re-insertion's work too
    std::vector<unsigned char> full;
    if ((rc = rsp_stage2_regate(p->g.P, p->g.N, p->g.B, iq, dtype, n_gated, cols, full))) return rc;
    const S3Out o{amp_out, flags, threshold, hits, hits_cap, n_hits};
    return vc_fused(p, Stage2In{full.data(), dtype, false, nullptr, 1}, prm, mtd_out, o);
}

int32_t rsp_profile_vcfar(rsp_plan* p, const rsp_vcfar_params* prm, int32_t iters, float* ms_out, int64_t* bytes_out) {
    if (!p || !prm || iters < 1) return fail(RSP_ERR_INVALID, "bad argument");
    VcDesc d;
    int rc = rsp_vcfar_derive(p->g.P, p->g.G, prm, &d);
    if (rc || (rc = rsp_s3_check_cells(d.P, d.G, p->g.B))) return rc;
    const int B = p->g.B;
    return cfar_profile(p, d.P, d.G, iters, ms_out, bytes_out,
                        [&](bool cplx, const void* in, double* amp, double* thr, uint8_t* fl, rsp_stage3_hit* hits, int* cnt,
                            int cap, hipStream_t st) { return launch_vcfar(d, p->g.prec, cplx, in, B, amp, thr, fl, hits, cnt, cap, st); });
}

// The raw cube of a raw-cube stage-2 call as the full-PRT [P x N x C] the device takes: the caller's, or
// (n_gated != 0) its gated columns put back at their PRT positions in `full`
static int raw_full_prt(const rsp_plan* p, const void* cube, int dtype, int n_gated, const int32_t* cols,
                        std::vector<unsigned char>& full, const void** out) {
    *out = cube;
    if (!n_gated) return dtype == RSP_C64 || dtype == RSP_C128 ? RSP_OK : fail(RSP_ERR_INVALID, "unknown dtype %d", dtype);
    const int rc = rsp_stage2_regate(p->g.P, p->g.N, p->g.C, cube, dtype, n_gated, cols, full);
    *out = full.data();
    return rc;
}

int32_t rsp_process_raw_stage2(rsp_plan* p, const void* cube, int32_t dtype, int32_t n_gated, const int32_t* cols,
                               const double* W, int32_t conj, double* mtd_out, double* pc_out) {
    if (!p || !cube) return fail(RSP_ERR_INVALID, "null argument");
    std::vector<unsigned char> full;
    const void* src;
    int rc = raw_full_prt(p, cube, dtype, n_gated, cols, full, &src);
    if (rc || (rc = stage2_device(p, Stage2In{src, dtype, true, W, conj}))) return rc;
    if (pc_out && (rc = rdm_out(p, p->lanes[0].rdm, pc_out))) return rc;
    if (mtd_out && (rc = rdm_out(p, p->d_aux, mtd_out))) return rc;
    return RSP_OK;
}

int32_t rsp_process_raw_stage2_cfar(rsp_plan* p, const void* cube, int32_t dtype, int32_t n_gated, const int32_t* cols,
                                    const double* W, int32_t conj, const rsp_stage3_cfar_params* prm, double* mtd_out,
                                    double* amp_out, uint8_t* flags, double* threshold, rsp_stage3_hit* hits,
                                    int64_t hits_cap, int64_t* n_hits) {
    S3Desc d;
    int rc = s3_args(p, cube, prm, hits_cap);
    if (rc || (rc = rsp_stage3_derive(p->g.P, p->gates, prm, &d))) return rc;   // before the re-insertion's work too
    std::vector<unsigned char> full;
    const void* src;
    if ((rc = raw_full_prt(p, cube, dtype, n_gated, cols, full, &src))) return rc;
    return s3_fused(p, Stage2In{src, dtype, true, W, conj}, prm, mtd_out, S3Out{amp_out, flags, threshold, hits, hits_cap, n_hits});
}

int32_t rsp_process_raw_stage2_vcfar(rsp_plan* p, const void* cube, int32_t dtype, int32_t n_gated, const int32_t* cols,
                                     const double* W, int32_t conj, const rsp_vcfar_params* prm, double* mtd_out,
                                     double* amp_out, uint8_t* flags, double* threshold, rsp_stage3_hit* hits,
                                     int64_t hits_cap, int64_t* n_hits) {
    VcDesc d;
    int rc = s3_args(p, cube, prm, hits_cap);
    if (rc || (rc = rsp_vcfar_derive(p->g.P, p->g.G, prm, &d))) return rc;   // before the re-insertion's work too
    std::vector<unsigned char> full;
    const void* src;
    if ((rc = raw_full_prt(p, cube, dtype, n_gated, cols, full, &src))) return rc;
    return vc_fused(p, Stage2In{src, dtype, true, W, conj}, prm, mtd_out, S3Out{amp_out, flags, threshold, hits, hits_cap, n_hits});
}

// ---- cross GOCA-CFAR as a map detector ----
int32_t rsp_xcfar(rsp_plan* p, int32_t P, int32_t G, const double* amp, int32_t n_maps, const rsp_cfar_params* prm,
                  uint8_t* flags, double* threshold, rsp_stage3_hit* hits, int64_t hits_cap, int64_t* n_hits) {
    XcDesc d;
    int rc = s3_args(p, amp, prm, hits_cap);
    if (rc || (rc = rsp_xcfar_derive(P, G, prm, &d))) return rc;   // refusals before any device work
    if ((rc = rsp_s3_check_cells(d.P, d.G, n_maps))) return rc;
    HIPCHK(hipSetDevice(p->device));
    if ((rc = drain_all(p))) return rc;
    // MATLAB column-major [P x G x n] -> [n][P][G] in the plan's precision
    const size_t cells = (size_t)n_maps * d.P * d.G, rs = p->rsz;
    std::vector<unsigned char> host(cells * rs);
    if (rs == 8) rsp_transpose_planes(amp, d.G, d.P, n_maps, reinterpret_cast<double*>(host.data()));
    else rsp_transpose_planes(amp, d.G, d.P, n_maps, reinterpret_cast<float*>(host.data()));
    if ((rc = s3_reserve(p->s3_in, cells * rs))) return rc;
    HIPCHK(hipMemcpy(p->s3_in.p, host.data(), cells * rs, hipMemcpyHostToDevice));
    const S3Out o{nullptr, flags, threshold, hits, hits_cap, n_hits};
    return xc_run(p, d, false, p->s3_in.p, n_maps, o);
}

int32_t rsp_process_stage2_xcfar(rsp_plan* p, const void* iq, int32_t dtype, const rsp_cfar_params* prm, double* mtd_out,
                                 double* amp_out, uint8_t* flags, double* threshold, rsp_stage3_hit* hits, int64_t hits_cap,
                                 int64_t* n_hits) {
    const int rc = s3_args(p, iq, prm, hits_cap);
    return rc ? rc : xc_fused(p, Stage2In{iq, dtype, false, nullptr, 1}, prm, mtd_out, S3Out{amp_out, flags, threshold, hits, hits_cap, n_hits});
}

int32_t rsp_process_stage2_gated_xcfar(rsp_plan* p, const void* iq, int32_t dtype, int32_t n_gated, const int32_t* cols,
                                       const rsp_cfar_params* prm, double* mtd_out, double* amp_out, uint8_t* flags,
                                       double* threshold, rsp_stage3_hit* hits, int64_t hits_cap, int64_t* n_hits) {
    XcDesc d;
    int rc = s3_args(p, iq, prm, hits_cap);
    if (rc || (rc = rsp_xcfar_derive(p->g.P, p->g.G, prm, &d))) return rc;   // before the re-insertion's work too
    std::vector<unsigned char> full;
    if ((rc = rsp_stage2_regate(p->g.P, p->g.N, p->g.B, iq, dtype, n_gated, cols, full))) return rc;
    const S3Out o{amp_out, flags, threshold, hits, hits_cap, n_hits};
    return xc_fused(p, Stage2In{full.data(), dtype, false, nullptr, 1}, prm, mtd_out, o);
}

int32_t rsp_process_raw_stage2_xcfar(rsp_plan* p, const void* cube, int32_t dtype, int32_t n_gated, const int32_t* cols,
                                     const double* W, int32_t conj, const rsp_cfar_params* prm, double* mtd_out,
                                     double* amp_out, uint8_t* flags, double* threshold, rsp_stage3_hit* hits,
                                     int64_t hits_cap, int64_t* n_hits) {
    XcDesc d;
    int rc = s3_args(p, cube, prm, hits_cap);
    if (rc || (rc = rsp_xcfar_derive(p->g.P, p->g.G, prm, &d))) return rc;   // before the re-insertion's work too
    std::vector<unsigned char> full;
    const void* src;
    if ((rc = raw_full_prt(p, cube, dtype, n_gated, cols, full, &src))) return rc;
    return xc_fused(p, Stage2In{src, dtype, true, W, conj}, prm, mtd_out, S3Out{amp_out, flags, threshold, hits, hits_cap, n_hits});
}

int32_t rsp_last_cfar_threshold(rsp_plan* p, uint8_t* flags, double* threshold, rsp_stage3_hit* hits, int64_t hits_cap,
                                int64_t* n_hits) {
    if (!p) return fail(RSP_ERR_INVALID, "null argument");
    if (hits_cap < 0) return fail(RSP_ERR_INVALID, "negative hits_cap");
    if (p->g.B < 2) return fail(RSP_ERR_INVALID, "a plan with one beam has no pair-sum maps");
    if (!p->smap_valid || !p->d_smap)
        return fail(RSP_ERR_INVALID, "no pair-sum maps on the device: the plan's last synchronous frame did not ask for cfar_maps");
    const rsp_cfar_params prm{p->g.refV, p->g.guardV, p->g.refR, p->g.guardR, p->g.T};
    XcDesc d;
    int rc = rsp_xcfar_derive(p->g.P, p->g.G, &prm, &d);
    if (rc || (rc = rsp_s3_check_cells(d.P, d.G, p->g.B - 1))) return rc;
    HIPCHK(hipSetDevice(p->device));
    if ((rc = drain_all(p))) return rc;
    return xc_run(p, d, false, p->d_smap, p->g.B - 1, S3Out{nullptr, flags, threshold, hits, hits_cap, n_hits});
}

int32_t rsp_profile_xcfar(rsp_plan* p, const rsp_cfar_params* prm, int32_t iters, float* ms_out, int64_t* bytes_out) {
    if (!p || !prm || iters < 1) return fail(RSP_ERR_INVALID, "bad argument");
    XcDesc d;
    int rc = rsp_xcfar_derive(p->g.P, p->g.G, prm, &d);
    if (rc || (rc = rsp_s3_check_cells(d.P, d.G, p->g.B))) return rc;
    const int B = p->g.B;
    return cfar_profile(p, d.P, d.G, iters, ms_out, bytes_out,
                        [&](bool cplx, const void* in, double* amp, double* thr, uint8_t* fl, rsp_stage3_hit* hits, int* cnt,
                            int cap, hipStream_t st) { return launch_xcfar(d, p->g.prec, cplx, in, B, amp, thr, fl, hits, cnt, cap, st); });
}

// The device buffers and the kernel argument of a k_dbf launch of these sizes (already checked)
static int dbf_reserve(rsp_plan* p, int S, int C, int B, DbfDesc* d) {
    const int pitch = dbf_pitch(S, p->g.prec);
    *d = dbf_desc(S, C, B, pitch, pitch, p->g.prec);
    const K1Cfg kc = k1_cfg(C, B);
    int rc;
    if ((rc = s3_reserve(p->dbf_in, d->in_bytes)) || (rc = s3_reserve(p->dbf_out, d->out_bytes))) return rc;
    return s3_reserve(p->dbf_tab, (size_t)kc.MB * kc.NJ * 2 * 64 * p->rsz);
}

int32_t rsp_dbf(rsp_plan* p, int32_t P, int32_t N, int32_t C, int32_t B, const void* cube, int32_t dtype, const double* W,
                int32_t conj, double* beams_out) {
    int rc = rsp_dbf_check_sizes(P, N, C, B, p ? (p->g.prec == RSP_PREC_F64 ? RSP_C128 : RSP_C64) : RSP_C128);
    if (rc || (rc = rsp_dbf_check_args(p, cube, dtype, W, beams_out))) return rc;   // refusals before any device work
    HIPCHK(hipSetDevice(p->device));
    if ((rc = drain_all(p))) return rc;
    const bool f64 = p->g.prec == RSP_PREC_F64;
    const size_t S = (size_t)P * N, esz = p->esz;
    DbfDesc d;
    if ((rc = dbf_reserve(p, (int)S, C, B, &d))) return rc;
    hipStream_t s = p->lanes[0].stream;
    std::vector<double> t;
    rsp_dbf_atab(W, B, C, conj, f64 ? DBF_ROWS_SPLIT : DBF_ROWS_PAIR, t);
    if ((rc = p->put_reals(p->dbf_tab.p, t.data(), t.size()))) return rc;
    const void* src = cube;
    if ((dtype == RSP_C128) != f64) {   // as upload_cube: a converting copy only when the dtypes differ
        if ((rc = ensure_stage(p, S * C * esz))) return rc;
        rsp_convert_reals(cube, dtype, 2 * S * C, p->h_stage);
        src = p->h_stage;
    }
    HIPCHK(hipMemcpy2DAsync(p->dbf_in.p, (size_t)d.pitch * esz, src, S * esz, S * esz, C, hipMemcpyHostToDevice, s));
    HIPCHK(launch_dbf(d, p->g.prec, p->dbf_in.p, p->dbf_tab.p, p->dbf_out.p, s));
    // the beam planes, widened to double for a complex-single plan
    std::vector<float> nar(f64 ? 0 : 2 * S * B);
    void* dst = f64 ? (void*)beams_out : (void*)nar.data();
    HIPCHK(hipMemcpy2DAsync(dst, S * esz, p->dbf_out.p, (size_t)d.opitch * esz, S * esz, B, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));   // the caller's cube (or the staging buffer) is borrowed for the call
    if (!f64) rsp_convert_reals(nar.data(), RSP_C64, 2 * S * B, beams_out);
    return RSP_OK;
}

int32_t rsp_profile_dbf(rsp_plan* p, int32_t P, int32_t N, int32_t C, int32_t B, int32_t iters, float* ms_out,
                        int64_t* bytes_out) {
    if (!p || iters < 1 || !ms_out) return fail(RSP_ERR_INVALID, "bad argument");
    int rc = rsp_dbf_check_sizes(P, N, C, B, p->g.prec == RSP_PREC_F64 ? RSP_C128 : RSP_C64);
    if (rc) return rc;
    HIPCHK(hipSetDevice(p->device));
    if ((rc = drain_all(p))) return rc;
    const int S = P * N;
    DbfDesc d;
    if ((rc = dbf_reserve(p, S, C, B, &d))) return rc;
    hipStream_t s = p->lanes[0].stream;
    HIPCHK(hipMemsetAsync(p->dbf_in.p, 0, d.in_bytes, s));   // zeros, and zero weights: the time does not depend on the values
    HIPCHK(hipMemsetAsync(p->dbf_tab.p, 0, p->dbf_tab.cap, s));
    auto run = [&]() -> int {
        HIPCHK(launch_dbf(d, p->g.prec, p->dbf_in.p, p->dbf_tab.p, p->dbf_out.p, s));
        return RSP_OK;
    };
    if ((rc = time_launches(s, iters, run, ms_out))) return rc;
    if (bytes_out) *bytes_out = (int64_t)p->esz * S * (C + B);
    return RSP_OK;
}

// The device tables of a k_mtd_any launch, built and uploaded the first time a length is seen
static int mtd_tables(rsp_plan* p, const MtdDesc& d, const void** tab, const void** tw) {
    typedef std::complex<double> cd;
    *tab = *tw = nullptr;
    auto put = [&](std::map<int, void*>& m, int key, const std::vector<cd>& h, const void** out) -> int {
        void* q = nullptr;
        if (hipMalloc(&q, h.size() * p->esz) != hipSuccess) return fail(RSP_ERR_NOMEM, "hipMalloc of the MTD tables failed");
        const int rc = p->put_reals(q, reinterpret_cast<const double*>(h.data()), 2 * h.size());
        if (rc) {
            (void)hipFree(q);
            return rc;
        }
        m[key] = q;
        *out = q;
        return RSP_OK;
    };
    int rc;
    std::vector<cd> h;
    if (d.chirp) {
        auto it = p->mtd_tab.find(d.nfft);
        if (it != p->mtd_tab.end())
            *tab = it->second;
        else {
            rsp_mtd_tables(d.nfft, p->g.prec, h);
            if ((rc = put(p->mtd_tab, d.nfft, h, tab))) return rc;
        }
    }
    if (d.lgL >= 5) {   // one pass (L <= 16): no twiddles
        auto it = p->mtd_tw.find(d.lgL);
        if (it != p->mtd_tw.end())
            *tw = it->second;
        else {
            rsp_mtd_twiddles(d.lgL, h);
            if ((rc = put(p->mtd_tw, d.lgL, h, tw))) return rc;
        }
    }
    return RSP_OK;
}

// One k_mtd_any launch on device memory of the plan's precision (sizes checked, queue drained)
static int mtd_run(rsp_plan* p, MtdDesc d, const void* d_pc, const double* win, void* d_out, hipStream_t s) {
    const void *tab, *tw;
    int rc = mtd_tables(p, d, &tab, &tw);
    if (rc) return rc;
    if (win) {
        if ((rc = s3_reserve(p->mtd_win, (size_t)d.P * p->rsz)) || (rc = p->put_reals(p->mtd_win.p, win, d.P))) return rc;
    }
    // complex single: element pairs where a column starts on 16 bytes (even length, aligned base)
    if (p->g.prec != RSP_PREC_F64)
        d.vec = ((d.P % 2 == 0 && (uintptr_t)d_pc % 16 == 0) ? 1 : 0) | ((d.nfft % 2 == 0 && (uintptr_t)d_out % 16 == 0) ? 2 : 0);
    HIPCHK(launch_mtd(d, p->g.prec, d_pc, win ? p->mtd_win.p : nullptr, tab, tw, d_out, s));
    return RSP_OK;
}

static int mtd_prec(const rsp_plan* p) { return p ? (p->g.prec == RSP_PREC_F64 ? RSP_C128 : RSP_C64) : RSP_C128; }

int32_t rsp_mtd(rsp_plan* p, int32_t P, int32_t G, int32_t n_maps, int32_t nfft, const void* pc, int32_t dtype,
                const double* win, int32_t shift, double* out) {
    int n = 0;
    int rc = rsp_mtd_check_sizes(P, G, n_maps, nfft, mtd_prec(p), &n);
    if (rc) return rc;   // refusals before any device work
    if (dtype != RSP_C64 && dtype != RSP_C128) return fail(RSP_ERR_INVALID, "unknown dtype %d", dtype);
    if (!p || !pc || !out) return fail(RSP_ERR_INVALID, "null argument");
    HIPCHK(hipSetDevice(p->device));
    if ((rc = drain_all(p))) return rc;
    const bool f64 = p->g.prec == RSP_PREC_F64;
    const size_t cols = (size_t)G * n_maps, nin = cols * P, nout = cols * n, esz = p->esz;
    if ((rc = s3_reserve(p->mtd_in, nin * esz)) || (rc = s3_reserve(p->mtd_out, nout * esz))) return rc;
    hipStream_t s = p->lanes[0].stream;
    const void* src = pc;
    if ((dtype == RSP_C128) != f64) {   // as upload_cube: a converting copy only when the dtypes differ
        if ((rc = ensure_stage(p, nin * esz))) return rc;
        rsp_convert_reals(pc, dtype, 2 * nin, p->h_stage);
        src = p->h_stage;
    }
    HIPCHK(hipMemcpyAsync(p->mtd_in.p, src, nin * esz, hipMemcpyHostToDevice, s));
    if ((rc = mtd_run(p, mtd_desc(P, G, n_maps, n, shift, win != nullptr, p->g.prec), p->mtd_in.p, win, p->mtd_out.p, s)))
        return rc;
    std::vector<float> nar(f64 ? 0 : 2 * nout);   // widened to double for a complex-single plan
    HIPCHK(hipMemcpyAsync(f64 ? (void*)out : (void*)nar.data(), p->mtd_out.p, nout * esz, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));   // the caller's cube (or the staging buffer) is borrowed for the call
    if (!f64) rsp_convert_reals(nar.data(), RSP_C64, 2 * nout, out);
    return RSP_OK;
}

int32_t rsp_mtd_device(rsp_plan* p, int32_t P, int32_t G, int32_t n_maps, int32_t nfft, const void* d_pc,
                       const double* win, int32_t shift, void* d_out) {
    int n = 0;
    int rc = rsp_mtd_check_sizes(P, G, n_maps, nfft, mtd_prec(p), &n);
    if (rc) return rc;
    if (!p || !d_pc || !d_out) return fail(RSP_ERR_INVALID, "null argument");
    const size_t cols = (size_t)G * n_maps;
    const char *a = static_cast<const char*>(d_pc), *b = static_cast<const char*>(d_out);
    if (a < b + cols * n * p->esz && b < a + cols * P * p->esz) return fail(RSP_ERR_INVALID, "d_pc and d_out overlap");
    if ((uintptr_t)d_pc % p->esz || (uintptr_t)d_out % p->esz)
        return fail(RSP_ERR_INVALID, "d_pc and d_out must be aligned to a complex element (%zu bytes)", p->esz);
    HIPCHK(hipSetDevice(p->device));
    if ((rc = drain_all(p))) return rc;
    hipStream_t s = p->lanes[0].stream;
    if ((rc = mtd_run(p, mtd_desc(P, G, n_maps, n, shift, win != nullptr, p->g.prec), d_pc, win, d_out, s))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    return RSP_OK;
}

int32_t rsp_profile_mtd(rsp_plan* p, int32_t P, int32_t G, int32_t n_maps, int32_t nfft, int32_t iters, float* ms_out,
                        int64_t* bytes_out) {
    if (!p || iters < 1 || !ms_out) return fail(RSP_ERR_INVALID, "bad argument");
    int n = 0;
    int rc = rsp_mtd_check_sizes(P, G, n_maps, nfft, mtd_prec(p), &n);
    if (rc) return rc;
    HIPCHK(hipSetDevice(p->device));
    if ((rc = drain_all(p))) return rc;
    const size_t cols = (size_t)G * n_maps;
    if ((rc = s3_reserve(p->mtd_in, cols * P * p->esz)) || (rc = s3_reserve(p->mtd_out, cols * n * p->esz))) return rc;
    hipStream_t s = p->lanes[0].stream;
    HIPCHK(hipMemsetAsync(p->mtd_in.p, 0, cols * P * p->esz, s));   // zeros: the time does not depend on the values
    const std::vector<double> win(P, 1.0);
    MtdDesc d = mtd_desc(P, G, n_maps, n, 1, true, p->g.prec);
    if ((rc = mtd_run(p, d, p->mtd_in.p, win.data(), p->mtd_out.p, s))) return rc;   // tables and window up, once
    const void *tab, *tw;
    if ((rc = mtd_tables(p, d, &tab, &tw))) return rc;
    if (p->g.prec != RSP_PREC_F64) d.vec = (P % 2 == 0 ? 1 : 0) | (n % 2 == 0 ? 2 : 0);
    auto run = [&]() -> int {
        HIPCHK(launch_mtd(d, p->g.prec, p->mtd_in.p, p->mtd_win.p, tab, tw, p->mtd_out.p, s));
        return RSP_OK;
    };
    if ((rc = time_launches(s, iters, run, ms_out))) return rc;
    if (bytes_out) *bytes_out = (int64_t)p->esz * (int64_t)cols * (P + n);
    return RSP_OK;
}

// ---- detection on any RD cube: k_pairsum -> k_xcfar -> k_s9 -> S10 / S11 ----
static int det_prec(const rsp_plan* p) { return p ? (p->g.prec == RSP_PREC_F64 ? RSP_C128 : RSP_C64) : RSP_C128; }

// The checks of the detect entries after the sizes: the parameter block and the outputs
static int det_args(const rsp_plan* p, const void* in, const rsp_detect_params* prm, const rsp_frame_out* out, bool rdm_ok) {
    if (!p || !in || !prm) return fail(RSP_ERR_INVALID, "null argument");
    if (!prm->range_axis || !prm->velocity_axis || !prm->beam_angles_deg || !prm->k_slopes_LUT)
        return fail(RSP_ERR_INVALID, "null argument: range_axis, velocity_axis, beam_angles_deg and k_slopes_LUT are needed");
    if (prm->monopulse != 0 && prm->monopulse != 1) return fail(RSP_ERR_INVALID, "monopulse must be 0 or 1, got %d", prm->monopulse);
    if (out && out->rdm && !rdm_ok) return fail(RSP_ERR_INVALID, "out->rdm must be NULL: the cube is the caller's");
    return RSP_OK;
}

// The caller's axes (G, V), angles (B) and K-LUT (B - 1) on the device, as the DevConsts fields S9 reads
static int det_consts(rsp_plan* p, int V, int G, int B, const rsp_detect_params* prm, DevConsts* k) {
    std::vector<double> h;
    h.reserve((size_t)G + V + 2 * B);
    h.insert(h.end(), prm->range_axis, prm->range_axis + G);
    h.insert(h.end(), prm->velocity_axis, prm->velocity_axis + V);
    h.insert(h.end(), prm->beam_angles_deg, prm->beam_angles_deg + B);
    h.insert(h.end(), prm->k_slopes_LUT, prm->k_slopes_LUT + (B - 1));
    int rc = s3_reserve(p->det_axes, h.size() * sizeof(double));
    if (rc) return rc;
    HIPCHK(hipMemcpy(p->det_axes.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    const double* d = static_cast<const double*>(p->det_axes.p);
    *k = DevConsts{};
    k->range_axis = d;
    k->velocity_axis = d + G;
    k->beam_angles = d + G + V;
    k->klut = d + G + V + B;
    k->deltaR = prm->deltaR;
    k->deltaV = prm->deltaV;
    return RSP_OK;
}

// The device half on a cube of xd.P x xd.G x B in `layout` on lane 0's stream: the pair-sum maps into
// p->det_smap, k_xcfar's hit list (cfar_launch_grow) in p->s3_hits, their S9 records in p->det_dets, in
// the list's order.  Returns with the stream idle and *n_hits set.
static int det_device(rsp_plan* p, const XcDesc& xd, int B, int layout, const void* d_x, const DevConsts& k, int cplx,
                      int* n_hits) {
    Lane& L = p->lanes[0];
    const int V = xd.P, G = xd.G, np = B - 1, prec = p->g.prec;
    const size_t cells = (size_t)np * V * G;
    int rc;
    if ((rc = s3_reserve(p->det_smap, cells * p->rsz))) return rc;
    const DetDesc dd{V, G, B, 0, cplx};
    HIPCHK(launch_pairsum(dd, prec, layout, d_x, p->det_smap.p, L.stream));
    const void* smap = p->det_smap.p;
    rc = cfar_launch_grow(p, cells, false, false, false, true,
                          [&](double* amp, double* thr, uint8_t* flags, rsp_stage3_hit* hits, int* count, int cap, hipStream_t s) {
                              return launch_xcfar(xd, prec, false, smap, np, amp, thr, flags, hits, count, cap, s);
                          }, n_hits);
    if (rc || *n_hits == 0) return rc;
    if ((rc = s3_reserve(p->det_dets, sizeof(DevDet) * (size_t)*n_hits))) return rc;
    HIPCHK(launch_s9(dd, prec, layout, k, d_x, smap, (const rsp_stage3_hit*)p->s3_hits.p, *n_hits, (DevDet*)p->det_dets.p, L.stream));
    HIPCHK(hipStreamSynchronize(L.stream));
    return RSP_OK;
}

// ... and the host half: the records in the reference's order, S10 / S11, the caller's outputs as
// run_sync_frame fills them (rdm excepted: the entry's)
static int det_run(rsp_plan* p, const XcDesc& xd, int B, int layout, const void* d_x, const DevConsts& k, int cplx,
                   const rsp_cluster_params& cl, rsp_frame_out* out) {
    int n = 0;
    int rc = det_device(p, xd, B, layout, d_x, k, cplx, &n);
    if (rc) return rc;
    static_assert(sizeof(DevDet) == sizeof(rsp_detection), "layout");
    std::vector<rsp_detection> dets((size_t)n);
    if (n) HIPCHK(hipMemcpy(dets.data(), p->det_dets.p, sizeof(DevDet) * (size_t)n, hipMemcpyDeviceToHost));
    std::vector<rsp_target> tg;
    rsp_cluster_frame(cl, dets, tg);   // sorts into fsf's find order (pair, r, v) first
    p->last_dets = std::move(dets);
    p->last_targets = tg;
    if (!out) return RSP_OK;
    const int nt = (int)tg.size(), nd = (int)p->last_dets.size();
    const int rt = rsp_capped_copy(out->targets, tg.data(), nt, out->targets_cap, &out->n_targets,
                                   "%d targets exceed targets_cap %d (all of them: rsp_last_targets)", nt, out->targets_cap);
    const int rd = rsp_capped_copy(out->dets, p->last_dets.data(), nd, out->dets_cap, &out->n_dets,
                                   "%d detections exceed dets_cap %d (all of them: rsp_last_detections)", nd, out->dets_cap);
    if (out->cfar_maps) {
        rc = p->g.prec == RSP_PREC_F64 ? maps_to_matlab<double>(p->det_smap.p, xd.P, xd.G, B - 1, out->cfar_maps)
                                       : maps_to_matlab<float>(p->det_smap.p, xd.P, xd.G, B - 1, out->cfar_maps);
        if (rc) return rc;
    }
    return rd ? rd : rt;
}

// A host cube of `elems` complex values into buf in the plan's precision, on stream s (borrowed until the sync)
static int det_upload(rsp_plan* p, rsp_plan::DevBuf& buf, const void* src, int dtype, size_t elems, hipStream_t s) {
    int rc = s3_reserve(buf, elems * p->esz);
    if (rc) return rc;
    if ((dtype == RSP_C128) != (p->g.prec == RSP_PREC_F64)) {   // as upload_cube: a converting copy only when the dtypes differ
        if ((rc = ensure_stage(p, elems * p->esz))) return rc;
        rsp_convert_reals(src, dtype, 2 * elems, p->h_stage);
        src = p->h_stage;
    }
    HIPCHK(hipMemcpyAsync(buf.p, src, elems * p->esz, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    return RSP_OK;
}

int32_t rsp_detect(rsp_plan* p, int32_t V, int32_t G, int32_t B, const void* rdm, int32_t dtype,
                   const rsp_detect_params* prm, rsp_frame_out* out) {
    XcDesc xd;
    int rc = rsp_detect_check_sizes(V, G, B, det_prec(p), prm ? &prm->cfar : nullptr, &xd);
    if (rc) return rc;   // refusals before any device work
    if (dtype != RSP_C64 && dtype != RSP_C128) return fail(RSP_ERR_INVALID, "unknown dtype %d", dtype);
    if ((rc = det_args(p, rdm, prm, out, false))) return rc;
    HIPCHK(hipSetDevice(p->device));
    if ((rc = drain_all(p))) return rc;
    DevConsts k;
    if ((rc = det_consts(p, V, G, B, prm, &k))) return rc;
    if ((rc = det_upload(p, p->det_in, rdm, dtype, (size_t)V * G * B, p->lanes[0].stream))) return rc;
    return det_run(p, xd, B, DET_LAYOUT_MATLAB, p->det_in.p, k, prm->monopulse, prm->cluster, out);
}

int32_t rsp_detect_device(rsp_plan* p, int32_t V, int32_t G, int32_t B, const void* d_rdm, const rsp_detect_params* prm,
                          rsp_frame_out* out) {
    XcDesc xd;
    int rc = rsp_detect_check_sizes(V, G, B, det_prec(p), prm ? &prm->cfar : nullptr, &xd);
    if (rc || (rc = det_args(p, d_rdm, prm, out, false))) return rc;
    if ((uintptr_t)d_rdm % p->esz) return fail(RSP_ERR_INVALID, "d_rdm must be aligned to a complex element (%zu bytes)", p->esz);
    HIPCHK(hipSetDevice(p->device));
    if ((rc = drain_all(p))) return rc;
    DevConsts k;
    if ((rc = det_consts(p, V, G, B, prm, &k))) return rc;
    return det_run(p, xd, B, DET_LAYOUT_MATLAB, d_rdm, k, prm->monopulse, prm->cluster, out);
}

int32_t rsp_mtd_detect(rsp_plan* p, int32_t P, int32_t G, int32_t B, int32_t nfft, const void* pc, int32_t dtype,
                       const double* win, const rsp_detect_params* prm, rsp_frame_out* out) {
    int n = 0;
    XcDesc xd;
    int rc = rsp_mtd_check_sizes(P, G, B, nfft, det_prec(p), &n);
    if (rc || (rc = rsp_detect_check_sizes(n, G, B, det_prec(p), prm ? &prm->cfar : nullptr, &xd))) return rc;
    if (dtype != RSP_C64 && dtype != RSP_C128) return fail(RSP_ERR_INVALID, "unknown dtype %d", dtype);
    if ((rc = det_args(p, pc, prm, out, true))) return rc;
    HIPCHK(hipSetDevice(p->device));
    if ((rc = drain_all(p))) return rc;
    hipStream_t s = p->lanes[0].stream;
    const size_t nout = (size_t)G * B * n;
    DevConsts k;
    if ((rc = det_consts(p, n, G, B, prm, &k)) || (rc = s3_reserve(p->mtd_out, nout * p->esz))) return rc;
    if ((rc = det_upload(p, p->mtd_in, pc, dtype, (size_t)G * B * P, s))) return rc;
    if ((rc = mtd_run(p, mtd_desc(P, G, B, n, 1, win != nullptr, p->g.prec), p->mtd_in.p, win, p->mtd_out.p, s))) return rc;
    const int rr = det_run(p, xd, B, DET_LAYOUT_MATLAB, p->mtd_out.p, k, prm->monopulse, prm->cluster, out);
    if (rr && rr != RSP_ERR_OVERFLOW) return rr;
    if (out && out->rdm) {   // the cube, widened to double for a complex-single plan
        const bool f64 = p->g.prec == RSP_PREC_F64;
        std::vector<float> nar(f64 ? 0 : 2 * nout);
        HIPCHK(hipMemcpy(f64 ? (void*)out->rdm : (void*)nar.data(), p->mtd_out.p, nout * p->esz, hipMemcpyDeviceToHost));
        if (!f64) rsp_convert_reals(nar.data(), RSP_C64, 2 * nout, out->rdm);
    }
    return rr;
}

int32_t rsp_process_stage2_detect(rsp_plan* p, const void* iq, int32_t dtype, rsp_frame_out* out) {
    if (!p || !iq) return fail(RSP_ERR_INVALID, "null argument");
    const rsp_cfar_params prm{p->g.refV, p->g.guardV, p->g.refR, p->g.guardR, p->g.T};
    XcDesc xd;
    int rc = rsp_detect_check_sizes(p->g.P, p->g.G, p->g.B, det_prec(p), &prm, &xd);   // refusals before any device work
    if (rc || (rc = stage2_device(p, iq, dtype))) return rc;
    const int rr = det_run(p, xd, p->g.B, DET_LAYOUT_DEVICE, p->d_aux, p->k, p->g.mono_c ? 1 : 0, p->cl, out);
    if (rr && rr != RSP_ERR_OVERFLOW) return rr;
    if (out && out->rdm && (rc = rdm_out(p, p->d_aux, out->rdm))) return rc;
    return rr;
}

int32_t rsp_profile_detect(rsp_plan* p, int32_t V, int32_t G, int32_t B, const rsp_cfar_params* prm, int32_t iters,
                           float* ms_out, int64_t* bytes_out) {
    if (!p || !prm || iters < 1 || !ms_out) return fail(RSP_ERR_INVALID, "bad argument");
    XcDesc xd;
    int rc = rsp_detect_check_sizes(V, G, B, det_prec(p), prm, &xd);
    if (rc) return rc;
    HIPCHK(hipSetDevice(p->device));
    if ((rc = drain_all(p))) return rc;
    Lane& L = p->lanes[0];
    const size_t elems = (size_t)V * G * B, cells = (size_t)V * G * (B - 1);
    {   // the test cube rsp.h describes, in the plan's precision
        std::vector<float> h(2 * elems);
        uint32_t st = 0x9E3779B9u;
        for (size_t i = 0; i < 2 * elems; ++i) {
            st = st * 1664525u + 1013904223u;   // Numerical Recipes' LCG
            h[i] = (float)(st >> 8) * (1.0f / 16777216.0f);
        }
        for (int b = 0; b < B; ++b)
            for (int g = 50; g < G; g += 101)
                for (int v = 18; v < V; v += 37) h[2 * ((size_t)v + (size_t)V * (g + (size_t)G * b))] = 100.0f;
        if ((rc = det_upload(p, p->det_in, h.data(), RSP_C64, elems, L.stream))) return rc;
    }
    const std::vector<double> ax((size_t)std::max(std::max(V, G), B), 0.0);
    rsp_detect_params dp{};
    dp.range_axis = dp.velocity_axis = dp.beam_angles_deg = dp.k_slopes_LUT = ax.data();
    DevConsts k;
    if ((rc = det_consts(p, V, G, B, &dp, &k))) return rc;
    int n = 0;
    if ((rc = det_device(p, xd, B, DET_LAYOUT_MATLAB, p->det_in.p, k, 0, &n))) return rc;   // buffers sized, hits on the device
    const DetDesc dd{V, G, B, 0, 0};
    const int prec = p->g.prec, cap = (int)std::min<size_t>(p->s3_hits.cap / sizeof(rsp_stage3_hit), (size_t)INT32_MAX);
    for (int s = 0; s < 3; ++s) {
        auto run = [&]() -> int {
            if (s == 0) HIPCHK(launch_pairsum(dd, prec, DET_LAYOUT_MATLAB, p->det_in.p, p->det_smap.p, L.stream));
            if (s == 1) {
                HIPCHK(hipMemsetAsync(p->s3_count.p, 0, 4, L.stream));
                HIPCHK(launch_xcfar(xd, prec, false, p->det_smap.p, B - 1, nullptr, nullptr, nullptr, (rsp_stage3_hit*)p->s3_hits.p,
                                    (int*)p->s3_count.p, cap, L.stream));
            }
            if (s == 2)
                HIPCHK(launch_s9(dd, prec, DET_LAYOUT_MATLAB, k, p->det_in.p, p->det_smap.p, (const rsp_stage3_hit*)p->s3_hits.p, n,
                                 (DevDet*)p->det_dets.p, L.stream));
            return RSP_OK;
        };
        if ((rc = time_launches(L.stream, iters, run, &ms_out[s]))) return rc;
    }
    if (bytes_out) {
        bytes_out[0] = (int64_t)(elems * p->esz + cells * p->rsz);
        bytes_out[1] = (int64_t)(cells * p->rsz);
        bytes_out[2] = (int64_t)sizeof(DevDet) * n;
    }
    return RSP_OK;
}

// ---- pulse compression for any pulse and beam count: k_pc_pack -> k2_pc -> k_pc_unpack ----
// The sizes of a call (checked), the plan's scratch for them and the record table of (P, B) on the device
static int pc_prepare(rsp_plan* p, int P, int B) {
    int rc;
    if (p->pc_d.g.P != P || p->pc_d.g.B != B || !p->pc_rec.p) {
        PcDesc d;
        std::vector<K2Rec> rec;
        if ((rc = rsp_pc_derive(p->g, P, B, &d, &rec))) return rc;
        p->pc_d.g.P = 0;   // no key while the table is being replaced
        if ((rc = s3_reserve(p->pc_rec, std::max<size_t>(rec.size(), 1) * sizeof(K2Rec)))) return rc;
        if (!rec.empty()) HIPCHK(hipMemcpy(p->pc_rec.p, rec.data(), rec.size() * sizeof(K2Rec), hipMemcpyHostToDevice));
        p->pc_d = d;
    }
    const PcDesc& d = p->pc_d;
    if ((rc = s3_reserve(p->pc_z, d.z_elems * p->esz)) || (rc = s3_reserve(p->pc_res, d.out_elems * p->esz))) return rc;
    return s3_reserve(p->pc_mag, d.mag_elems * p->rsz);
}

// The three launches on device memory of the plan's precision (pc_prepare done, queue drained): beams at
// `pitch` elements per plane -> d_pc [P x G x B].  k2_pc stores its magnitude map whatever is asked of it:
// it goes to the scratch p->pc_mag.
static int pc_launches(rsp_plan* p, const void* d_beams, int pitch, void* d_pc, hipStream_t s, int only = -1) {
    const PcDesc& d = p->pc_d;
    FramePtrs fp{};
    fp.z[0] = p->pc_z.p;
    fp.rdm[0] = p->pc_res.p;
    fp.mag[0] = p->pc_mag.p;
    if (only < 0 || only == 0) HIPCHK(launch_pc_pack(d, d_beams, pitch, p->pc_z.p, s));
    if (only < 0 || only == 1)
        HIPCHK(launch_k2_set(d.g, p->k, fp, 1, d.rows, static_cast<const K2Rec*>(p->pc_rec.p), d.g.nwg_k2, false, s));
    if (only < 0 || only == 2) HIPCHK(launch_pc_unpack(d, p->pc_res.p, d_pc, s));
    return RSP_OK;
}

static int pc_sizes(const rsp_plan* p, int64_t P, int64_t B, PcDesc* d) {
    // without a plan the sizes cannot be judged: only the refusals that need none (P, B < 1) come first
    if (!p) return (P < 1 || B < 1) ? fail(RSP_ERR_INVALID, "bad sizes P=%lld B=%lld (P, B >= 1)", (long long)P, (long long)B)
                                    : fail(RSP_ERR_INVALID, "null argument");
    if (P >= 1 && p->pc_d.g.P == P && p->pc_d.g.B == B) {   // the sizes of the last call: already derived
        if (d) *d = p->pc_d;
        return RSP_OK;
    }
    return rsp_pc_derive(p->g, P, B, d, nullptr);
}

int32_t rsp_query_pc(const rsp_plan* p, int32_t P, int32_t B, rsp_pc_info* info) {
    PcDesc d;
    int rc = pc_sizes(p, P, B, &d);
    if (rc || !info) return rc;
    rsp_fill_pc_info(d, info);
    return RSP_OK;
}

// A host beam cube into p->pc_in and the launches into d_pc
static int pc_from_host(rsp_plan* p, int P, int B, const void* iq, int dtype, void* d_pc, hipStream_t s) {
    int rc = pc_prepare(p, P, B);
    if (rc || (rc = det_upload(p, p->pc_in, iq, dtype, p->pc_d.in_elems, s))) return rc;
    return pc_launches(p, p->pc_in.p, p->g.N * P, d_pc, s);
}

int32_t rsp_pc(rsp_plan* p, int32_t P, int32_t B, const void* iq, int32_t dtype, double* pc_out) {
    int rc = pc_sizes(p, P, B, nullptr);
    if (rc) return rc;   // refusals before any device work
    if (dtype != RSP_C64 && dtype != RSP_C128) return fail(RSP_ERR_INVALID, "unknown dtype %d", dtype);
    if (!iq || !pc_out) return fail(RSP_ERR_INVALID, "null argument");
    HIPCHK(hipSetDevice(p->device));
    if ((rc = drain_all(p))) return rc;
    hipStream_t s = p->lanes[0].stream;
    const bool f64 = p->g.prec == RSP_PREC_F64;
    const size_t nout = (size_t)P * p->g.G * B;
    if ((rc = s3_reserve(p->pc_out, nout * p->esz)) || (rc = pc_from_host(p, P, B, iq, dtype, p->pc_out.p, s))) return rc;
    std::vector<float> nar(f64 ? 0 : 2 * nout);   // widened to double for a complex-single plan
    HIPCHK(hipMemcpyAsync(f64 ? (void*)pc_out : (void*)nar.data(), p->pc_out.p, nout * p->esz, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (!f64) rsp_convert_reals(nar.data(), RSP_C64, 2 * nout, pc_out);
    return RSP_OK;
}

int32_t rsp_pc_device(rsp_plan* p, int32_t P, int32_t B, const void* d_beams, void* d_pc) {
    int rc = pc_sizes(p, P, B, nullptr);
    if (rc) return rc;
    if (!d_beams || !d_pc) return fail(RSP_ERR_INVALID, "null argument");
    const size_t nin = (size_t)P * p->g.N * B, nout = (size_t)P * p->g.G * B;
    const char *a = static_cast<const char*>(d_beams), *b = static_cast<const char*>(d_pc);
    if (a < b + nout * p->esz && b < a + nin * p->esz) return fail(RSP_ERR_INVALID, "d_beams and d_pc overlap");
    if ((uintptr_t)d_beams % p->esz || (uintptr_t)d_pc % p->esz)
        return fail(RSP_ERR_INVALID, "d_beams and d_pc must be aligned to a complex element (%zu bytes)", p->esz);
    HIPCHK(hipSetDevice(p->device));
    if ((rc = drain_all(p))) return rc;
    hipStream_t s = p->lanes[0].stream;
    if ((rc = pc_prepare(p, P, B)) || (rc = pc_launches(p, d_beams, p->g.N * P, d_pc, s))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    return RSP_OK;
}

// MTD to n rows (shift = 1) of the pc cube in p->mtd_in into p->mtd_out, the detector on it, and out->rdm: the
// back half of rsp_mtd_detect, shared by the two compositions below (sizes checked, k and mtd_out set up)
static int pc_mtd_detect_tail(rsp_plan* p, int P, int B, int n, const XcDesc& xd, const DevConsts& k, const double* win,
                              const rsp_detect_params* prm, rsp_frame_out* out, hipStream_t s) {
    const int G = p->g.G;
    const size_t nout = (size_t)G * B * n;
    int rc = mtd_run(p, mtd_desc(P, G, B, n, 1, win != nullptr, p->g.prec), p->mtd_in.p, win, p->mtd_out.p, s);
    if (rc) return rc;
    const int rr = det_run(p, xd, B, DET_LAYOUT_MATLAB, p->mtd_out.p, k, prm->monopulse, prm->cluster, out);
    if (rr && rr != RSP_ERR_OVERFLOW) return rr;
    if (out && out->rdm) {   // the cube, widened to double for a complex-single plan
        const bool f64 = p->g.prec == RSP_PREC_F64;
        std::vector<float> nar(f64 ? 0 : 2 * nout);
        HIPCHK(hipMemcpy(f64 ? (void*)out->rdm : (void*)nar.data(), p->mtd_out.p, nout * p->esz, hipMemcpyDeviceToHost));
        if (!f64) rsp_convert_reals(nar.data(), RSP_C64, 2 * nout, out->rdm);
    }
    return rr;
}

// The size checks of the two compositions after the pulse compression's own: MTD and detector at G = the plan's
static int pc_chain_sizes(const rsp_plan* p, int P, int B, int nfft, const rsp_detect_params* prm, int* n, XcDesc* xd) {
    int rc = rsp_mtd_check_sizes(P, p->g.G, B, nfft, det_prec(p), n);
    return rc ? rc : rsp_detect_check_sizes(*n, p->g.G, B, det_prec(p), prm ? &prm->cfar : nullptr, xd);
}

int32_t rsp_pc_mtd_detect(rsp_plan* p, int32_t P, int32_t B, int32_t nfft, const void* iq, int32_t dtype, const double* win,
                          const rsp_detect_params* prm, rsp_frame_out* out) {
    int n = 0;
    XcDesc xd;
    int rc = pc_sizes(p, P, B, nullptr);
    if (rc || (rc = pc_chain_sizes(p, P, B, nfft, prm, &n, &xd))) return rc;
    if (dtype != RSP_C64 && dtype != RSP_C128) return fail(RSP_ERR_INVALID, "unknown dtype %d", dtype);
    if ((rc = det_args(p, iq, prm, out, true))) return rc;
    HIPCHK(hipSetDevice(p->device));
    if ((rc = drain_all(p))) return rc;
    hipStream_t s = p->lanes[0].stream;
    const int G = p->g.G;
    DevConsts k;
    if ((rc = det_consts(p, n, G, B, prm, &k)) || (rc = s3_reserve(p->mtd_out, (size_t)G * B * n * p->esz)) ||
        (rc = s3_reserve(p->mtd_in, (size_t)G * B * P * p->esz)))
        return rc;
    if ((rc = pc_from_host(p, P, B, iq, dtype, p->mtd_in.p, s))) return rc;
    return pc_mtd_detect_tail(p, P, B, n, xd, k, win, prm, out, s);
}

int32_t rsp_raw_detect(rsp_plan* p, int32_t P, int32_t C, int32_t B, int32_t nfft, const void* cube, int32_t dtype,
                       const double* W, int32_t conj, const double* win, const rsp_detect_params* prm, rsp_frame_out* out) {
    int n = 0;
    XcDesc xd;
    int rc = pc_sizes(p, P, B, nullptr);
    if (rc || (rc = rsp_dbf_check_sizes(P, p->g.N, C, B, det_prec(p))) || (rc = pc_chain_sizes(p, P, B, nfft, prm, &n, &xd)))
        return rc;
    if (dtype != RSP_C64 && dtype != RSP_C128) return fail(RSP_ERR_INVALID, "unknown dtype %d", dtype);
    if ((rc = det_args(p, cube, prm, out, true))) return rc;
    if (!W && (B != p->g.B || C != p->g.C))
        return fail(RSP_ERR_INVALID, "W = NULL takes the plan's weights, %d x %d; the call has B=%d C=%d", p->g.B, p->g.C, B, C);
    HIPCHK(hipSetDevice(p->device));
    if ((rc = drain_all(p))) return rc;
    hipStream_t s = p->lanes[0].stream;
    const bool f64 = p->g.prec == RSP_PREC_F64;
    const int G = p->g.G;
    const size_t S = (size_t)P * p->g.N, esz = p->esz;
    DevConsts k;
    DbfDesc dd;
    if ((rc = det_consts(p, n, G, B, prm, &k)) || (rc = s3_reserve(p->mtd_out, (size_t)G * B * n * esz)) ||
        (rc = s3_reserve(p->mtd_in, (size_t)G * B * P * esz)) || (rc = dbf_reserve(p, (int)S, C, B, &dd)) ||
        (rc = pc_prepare(p, P, B)))
        return rc;
    // rsp_dbf's device half: the A operands, the channel planes at the kernel's pitch, k_dbf
    std::vector<double> t;
    rsp_dbf_atab(W ? W : p->h_W.data(), B, C, conj, f64 ? DBF_ROWS_SPLIT : DBF_ROWS_PAIR, t);
    if ((rc = p->put_reals(p->dbf_tab.p, t.data(), t.size()))) return rc;
    const void* src = cube;
    if ((dtype == RSP_C128) != f64) {
        if ((rc = ensure_stage(p, S * C * esz))) return rc;
        rsp_convert_reals(cube, dtype, 2 * S * C, p->h_stage);
        src = p->h_stage;
    }
    HIPCHK(hipMemcpy2DAsync(p->dbf_in.p, (size_t)dd.pitch * esz, src, S * esz, S * esz, C, hipMemcpyHostToDevice, s));
    HIPCHK(launch_dbf(dd, p->g.prec, p->dbf_in.p, p->dbf_tab.p, p->dbf_out.p, s));
    HIPCHK(hipStreamSynchronize(s));   // the caller's cube (or the staging buffer) is borrowed until here
    if ((rc = pc_launches(p, p->dbf_out.p, dd.opitch, p->mtd_in.p, s))) return rc;
    return pc_mtd_detect_tail(p, P, B, n, xd, k, win, prm, out, s);
}

int32_t rsp_profile_pc(rsp_plan* p, int32_t P, int32_t B, int32_t iters, float* ms_out, int64_t* bytes_out) {
    int rc = pc_sizes(p, P, B, nullptr);   // sizes first, as the other calls of the section
    if (rc) return rc;
    if (iters < 1 || !ms_out) return fail(RSP_ERR_INVALID, "bad argument");
    HIPCHK(hipSetDevice(p->device));
    if ((rc = drain_all(p))) return rc;
    hipStream_t s = p->lanes[0].stream;
    if ((rc = pc_prepare(p, P, B))) return rc;
    const PcDesc& d = p->pc_d;
    if ((rc = s3_reserve(p->pc_in, d.in_elems * p->esz)) || (rc = s3_reserve(p->pc_out, d.out_elems * p->esz))) return rc;
    HIPCHK(hipMemsetAsync(p->pc_in.p, 0, d.in_elems * p->esz, s));   // zeros: the times do not depend on the values
    for (int st = 0; st < 3; ++st) {
        auto run = [&]() -> int { return pc_launches(p, p->pc_in.p, p->g.N * P, p->pc_out.p, s, st); };
        if ((rc = time_launches(s, iters, run, &ms_out[st]))) return rc;
    }
    if (bytes_out) {
        bytes_out[0] = (int64_t)p->esz * ((int64_t)P * d.g.nU * B + (int64_t)d.z_elems);
        bytes_out[1] = (int64_t)p->esz * (int64_t)(d.z_elems + d.out_elems) + (int64_t)p->rsz * (int64_t)d.mag_elems;
        bytes_out[2] = 2 * (int64_t)p->esz * (int64_t)d.out_elems;
    }
    return RSP_OK;
}

int32_t rsp_profile_stages(rsp_plan* p, const void* const* d_cubes, int32_t n_cubes, int32_t iters, float* ms_out,
                           int64_t* bytes_out, int32_t cap, int32_t* frames_out) {
    return rsp_profile_stages_rdm(p, d_cubes, n_cubes, nullptr, iters, ms_out, bytes_out, cap, frames_out);
}

int32_t rsp_profile_stages_rdm(rsp_plan* p, const void* const* d_cubes, int32_t n_cubes, void* const* d_rdms,
                               int32_t iters, float* ms_out, int64_t* bytes_out, int32_t cap, int32_t* frames_out) {
    if (!p || !d_cubes || n_cubes < 1 || iters < 1) return fail(RSP_ERR_INVALID, "bad argument");
    HIPCHK(hipSetDevice(p->device));
    int rc = drain_all(p);
    if (rc) return rc;
    Lane& L = p->lanes[0];
    const int nf = std::min(n_cubes, p->F);
    for (int f = 0; f < nf && d_rdms; ++f)   // d_rdms holds (at least) one map per frame of the batch
        if (!d_rdms[f]) return fail(RSP_ERR_INVALID, "map %d is null (d_rdms needs min(n_cubes, F) maps)", f);
    // batches rotate over all n_cubes cubes (cube (j nf + f) mod n_cubes in batch j), so that a
    // ring larger than the 256 MiB Infinity Cache makes K1 read its input from HBM as in the queue
    const int nsets = (n_cubes + nf - 1) / nf;
    std::vector<FramePtrs> fps(nsets);
    for (int j = 0; j < nsets; ++j) {
        const void* in[RSP_MAX_F];
        for (int f = 0; f < nf; ++f) in[f] = d_cubes[(j * nf + f) % n_cubes];
        fps[j] = lane_ptrs(p, L, in, nf, d_rdms);   // as the queue: complex RDM stores only into d_rdms
        // ... and the launches the queue makes: stage 1 the band launch, stage 2 K3's phases with the
        // on-demand K2 between them, where the queue takes the band route
        L.band = band_route(p, fps[j], nf);
        lane_band_ptrs(L, nf, fps[j]);
    }
    const Geometry& g = p->g;
    for (int s = 0; s < 3 && s < cap; ++s) {
        int it = 0;
        auto run = [&]() -> hipError_t {
            const FramePtrs& fj = fps[it++ % nsets];
            if (s == 0) return launch_k1(g, p->k, fj, nf, 3, L.stream);
            if (s == 1) return launch_k2_lane(p, L, fj, nf);
            // counts and flags are zeroed by K1 in the pipeline; here by tiny memsets per launch
            hipError_t e = zero_k3_state(L, nf);
            return e != hipSuccess ? e : launch_k3_lane(p, L, fj, nf);
        };
        float ms = 0;
        if ((rc = time_launches(L.stream, iters, [&]() -> int { HIPCHK(run()); return RSP_OK; }, &ms))) return rc;
        if (ms_out) ms_out[s] = ms;
    }
    if (frames_out) *frames_out = nf;
    if (bytes_out) rsp_stage_bytes(g, (int)p->esz, nf, d_rdms || g.mono_c, cap, bytes_out, L.band ? p->k2rows[K2SET_BAND].n : -1);
    return RSP_OK;
}

int32_t rsp_hbm_copy_probe(int32_t device, int64_t bytes, int32_t iters, double* gbps) {
    if (!gbps || bytes < (1 << 20) || iters < 1) return fail(RSP_ERR_INVALID, "bad argument");
    HIPCHK(hipSetDevice(device));
    int ncu = 0;
    HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device));
    const size_t n16 = (size_t)bytes / 16;
    void *a = nullptr, *b = nullptr;
    if (hipMalloc(&a, n16 * 16) != hipSuccess) return fail(RSP_ERR_NOMEM, "hipMalloc(%lld) failed", (long long)bytes);
    if (hipMalloc(&b, n16 * 16) != hipSuccess) {
        (void)hipFree(a);
        return fail(RSP_ERR_NOMEM, "hipMalloc(%lld) failed", (long long)bytes);
    }
    hipEvent_t e0, e1;
    hipError_t e = hipMemset(a, 0, n16 * 16);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    float ms = 0.f;
    if (e == hipSuccess) {
        for (int i = 0; i < 3 && e == hipSuccess; ++i) e = launch_stream_copy(a, b, n16, ncu, nullptr);
        if (e == hipSuccess) e = hipEventRecord(e0, nullptr);
        for (int i = 0; i < iters && e == hipSuccess; ++i) e = launch_stream_copy(a, b, n16, ncu, nullptr);
        if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    }
    (void)hipFree(a);
    (void)hipFree(b);
    if (e != hipSuccess) return fail(RSP_ERR_DEVICE, "copy probe: %s", hipGetErrorString(e));
    *gbps = 2.0 * (double)(n16 * 16) / (ms * 1e-3 / iters) / 1e9;
    return RSP_OK;
}

int32_t rsp_device_alloc(rsp_plan* p, int64_t bytes, void** d) {
    if (!p || !d || bytes <= 0) return fail(RSP_ERR_INVALID, "bad argument");
    HIPCHK(hipSetDevice(p->device));
    if (hipMalloc(d, bytes) != hipSuccess) return fail(RSP_ERR_NOMEM, "hipMalloc(%lld) failed", (long long)bytes);
    return RSP_OK;
}
int32_t rsp_device_free(rsp_plan* p, void* d) {
    if (!p) return fail(RSP_ERR_INVALID, "null plan");
    HIPCHK(hipFree(d));
    return RSP_OK;
}
int32_t rsp_device_upload(rsp_plan* p, void* d, const void* h, int64_t bytes) {
    if (!p || !d || !h) return fail(RSP_ERR_INVALID, "null argument");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice));
    return RSP_OK;
}
int32_t rsp_device_download(rsp_plan* p, void* h, const void* d, int64_t bytes) {
    if (!p || !d || !h) return fail(RSP_ERR_INVALID, "null argument");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost));
    return RSP_OK;
}
int32_t rsp_device_sync(rsp_plan* p) {
    if (!p) return fail(RSP_ERR_INVALID, "null plan");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipDeviceSynchronize());
    return RSP_OK;
}

}  // extern "C"
