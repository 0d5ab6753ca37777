// rsp_plan.cpp -- host runtime of librsp: plan construction (device checks, uploads and lanes;
// the geometry analysis of the reference's precomputed_data is rsp_geometry.cpp's), the C-ABI of
// include/rsp.h, the device-resident frame queue, and the host stages S10/S11 (two-level BFS
// clustering, fsf:302-407).
#include "rsp_plan.h"

#include <cmath>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>

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

rsp_plan::rsp_plan() = default;
void rsp_plan::results_ready() const {
    if (pool) pool->wait();
}

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
                      &mtd_win, &det_in, &det_smap, &det_dets, &det_axes, &pc_in, &pc_z, &pc_res, &pc_mag, &pc_out, &pc_rec,
                      &ddc_in, &ddc_out, &ddc_h})
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

}  // namespace

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

namespace {

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

}  // namespace

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

int begin_sync(rsp_plan* p) {
    HIPCHK(hipSetDevice(p->device));
    return drain_all(p);
}

namespace {

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

}  // namespace

int host_reals_in_plan_prec(rsp_plan* p, const void* h, bool f64, size_t reals, const void** src) {
    *src = h;
    if (f64 == (p->g.prec == RSP_PREC_F64)) return RSP_OK;
    int rc = ensure_stage(p, reals * p->rsz);
    if (rc) return rc;
    rsp_convert_reals(h, f64 ? RSP_C128 : RSP_C64, reals, p->h_stage);
    *src = p->h_stage;
    return RSP_OK;
}

int host_in_plan_prec(rsp_plan* p, const void* h, int dtype, size_t elems, const void** src) {
    return host_reals_in_plan_prec(p, h, dtype == RSP_C128, 2 * elems, src);
}

int download_widened(rsp_plan* p, const void* d_src, size_t elems, double* out, hipStream_t s) {
    const bool f64 = p->g.prec == RSP_PREC_F64;
    std::vector<float> nar(f64 ? 0 : 2 * elems);
    HIPCHK(hipMemcpyAsync(f64 ? (void*)out : (void*)nar.data(), d_src, elems * p->esz, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (!f64) rsp_convert_reals(nar.data(), RSP_C64, 2 * elems, out);
    return RSP_OK;
}

int upload_cube(rsp_plan* p, const void* cube, int dtype, int nch, void* d_dst, hipStream_t s) {
    if (dtype != RSP_C64 && dtype != RSP_C128) return fail(RSP_ERR_INVALID, "unknown dtype %d", dtype);
    const size_t slab = (size_t)p->g.N * p->g.P;
    const void* src;
    int rc = host_in_plan_prec(p, cube, dtype, slab * nch, &src);
    if (rc) return rc;
    HIPCHK(hipMemcpy2DAsync(d_dst, (size_t)p->g.cpitch * p->esz, src, slab * p->esz, slab * p->esz, nch,
                            hipMemcpyHostToDevice, s));   // channel slabs at cpitch
    HIPCHK(hipStreamSynchronize(s));   // the caller's buffer (or the staging buffer) is borrowed for the call
    return RSP_OK;
}

int rdm_out(const rsp_plan* p, const void* d_map, double* out) { return plan_maps_to_matlab<cd, cf>(p, d_map, p->g.P, p->g.G, p->g.B, out); }

int frame_lists_out(const std::vector<rsp_target>& targets, const std::vector<rsp_detection>& dets, rsp_frame_out* out) {
    const int nt = (int)targets.size(), nd = (int)dets.size();
    const int rt = rsp_capped_copy(out->targets, targets.data(), nt, out->targets_cap, &out->n_targets,
                                   "%d targets exceed targets_cap %d (all of them: rsp_last_targets)", nt, out->targets_cap);
    const int rd = rsp_capped_copy(out->dets, dets.data(), nd, out->dets_cap, &out->n_dets,
                                   "%d detections exceed dets_cap %d (all of them: rsp_last_detections)", nd, out->dets_cap);
    return rd ? rd : rt;
}

int dev_reserve(rsp_plan::DevBuf& b, size_t bytes) {
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

namespace {

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
        const int rl = frame_lists_out(fr.targets, p->last_dets, out);   // the maps are written before an overflow is reported
        if (out->rdm && (rc = rdm_out(p, L.rdm, out->rdm))) return rc;
        if (smap && (rc = plan_maps_to_matlab<double, float>(p, smap, p->g.P, p->g.G, p->g.B - 1, out->cfar_maps))) return rc;   // device-produced (fsf:184-187)
        return rl;
    }
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
    int rc = begin_sync(p);
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
    int rc = begin_sync(p);
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
    int rc = begin_sync(p);
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
    if (dtype != plan_dtype(p))
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
    return begin_sync(p);
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


int32_t rsp_profile_stages(rsp_plan* p, const void* const* d_cubes, int32_t n_cubes, int32_t iters, float* ms_out,
                           int64_t* bytes_out, int32_t cap, int32_t* frames_out) {
    return rsp_profile_stages_rdm(p, d_cubes, n_cubes, nullptr, iters, ms_out, bytes_out, cap, frames_out);
}

int32_t rsp_profile_stages_rdm(rsp_plan* p, const void* const* d_cubes, int32_t n_cubes, void* const* d_rdms,
                               int32_t iters, float* ms_out, int64_t* bytes_out, int32_t cap, int32_t* frames_out) {
    if (!p || !d_cubes || n_cubes < 1 || iters < 1) return fail(RSP_ERR_INVALID, "bad argument");
    int rc = begin_sync(p);
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
