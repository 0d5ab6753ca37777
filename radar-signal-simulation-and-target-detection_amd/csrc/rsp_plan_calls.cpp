// rsp_plan_calls.cpp -- the stand-alone calls of librsp's host runtime on arrays of any size within the plan's
// envelope, and their compositions: DBF (k_dbf), MTD of any length (k_mtd_any), detection on any RD cube
// (k_pairsum -> k_xcfar -> k_s9 -> S10 / S11), pulse compression for any pulse and beam count
// (k_pc_pack -> k2_pc -> k_pc_unpack) and the digital down-converter in front of them (k_ddc).
#include "rsp_plan.h"

extern "C" {

// The device buffers and the kernel argument of a k_dbf launch of these sizes (already checked)
static int dbf_reserve(rsp_plan* p, int S, int C, int B, DbfDesc* d) {
    const int pitch = dbf_pitch(S, p->g.prec);
    *d = dbf_desc(S, C, B, pitch, pitch, p->g.prec);
    const K1Cfg kc = k1_cfg(C, B);
    int rc;
    if ((rc = dev_reserve(p->dbf_in, d->in_bytes)) || (rc = dev_reserve(p->dbf_out, d->out_bytes))) return rc;
    return dev_reserve(p->dbf_tab, (size_t)kc.MB * kc.NJ * 2 * 64 * p->rsz);
}

// k_dbf on stream s from the channel planes in p->dbf_in into p->dbf_out (dbf_reserve done), after the A
// operands of W
static int dbf_launch_planes(rsp_plan* p, const DbfDesc& d, int C, int B, const double* W, int conj, hipStream_t s) {
    std::vector<double> t;
    rsp_dbf_atab(W, B, C, conj, p->g.prec == RSP_PREC_F64 ? DBF_ROWS_SPLIT : DBF_ROWS_PAIR, t);
    const int rc = p->put_reals(p->dbf_tab.p, t.data(), t.size());
    if (rc) return rc;
    HIPCHK(launch_dbf(d, p->g.prec, p->dbf_in.p, p->dbf_tab.p, p->dbf_out.p, s));
    return RSP_OK;
}

// The device half of a DBF call on stream s, into p->dbf_out (dbf_reserve done): the A operands of W, the
// host cube's S x C channel planes at the kernel's pitch, k_dbf.  No wait: the caller's cube (or the staging
// buffer) is borrowed until the caller has waited for s.
static int dbf_launch_host(rsp_plan* p, const DbfDesc& d, size_t S, int C, int B, const void* cube, int dtype,
                           const double* W, int conj, hipStream_t s) {
    const size_t esz = p->esz;
    const void* src;
    const int rc = host_in_plan_prec(p, cube, dtype, S * C, &src);
    if (rc) return rc;
    HIPCHK(hipMemcpy2DAsync(p->dbf_in.p, (size_t)d.pitch * esz, src, S * esz, S * esz, C, hipMemcpyHostToDevice, s));
    return dbf_launch_planes(p, d, C, B, W, conj, s);
}

int32_t rsp_dbf(rsp_plan* p, int32_t P, int32_t N, int32_t C, int32_t B, const void* cube, int32_t dtype, const double* W,
                int32_t conj, double* beams_out) {
    int rc = rsp_dbf_check_sizes(P, N, C, B, plan_dtype(p));
    if (rc || (rc = rsp_dbf_check_args(p, cube, dtype, W, beams_out))) return rc;   // refusals before any device work
    if ((rc = begin_sync(p))) return rc;
    const bool f64 = p->g.prec == RSP_PREC_F64;
    const size_t S = (size_t)P * N, esz = p->esz;
    DbfDesc d;
    hipStream_t s = p->lanes[0].stream;
    if ((rc = dbf_reserve(p, (int)S, C, B, &d)) || (rc = dbf_launch_host(p, d, S, C, B, cube, dtype, W, conj, s))) return rc;
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
    int rc = rsp_dbf_check_sizes(P, N, C, B, plan_dtype(p));
    if (rc) return rc;
    if ((rc = begin_sync(p))) return rc;
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
        if ((rc = dev_reserve(p->mtd_win, (size_t)d.P * p->rsz)) || (rc = p->put_reals(p->mtd_win.p, win, d.P))) return rc;
    }
    // complex single: element pairs where a column starts on 16 bytes (even length, aligned base)
    if (p->g.prec != RSP_PREC_F64)
        d.vec = ((d.P % 2 == 0 && (uintptr_t)d_pc % 16 == 0) ? 1 : 0) | ((d.nfft % 2 == 0 && (uintptr_t)d_out % 16 == 0) ? 2 : 0);
    HIPCHK(launch_mtd(d, p->g.prec, d_pc, win ? p->mtd_win.p : nullptr, tab, tw, d_out, s));
    return RSP_OK;
}

int32_t rsp_mtd(rsp_plan* p, int32_t P, int32_t G, int32_t n_maps, int32_t nfft, const void* pc, int32_t dtype,
                const double* win, int32_t shift, double* out) {
    int n = 0;
    int rc = rsp_mtd_check_sizes(P, G, n_maps, nfft, plan_dtype(p), &n);
    if (rc) return rc;   // refusals before any device work
    if (dtype != RSP_C64 && dtype != RSP_C128) return fail(RSP_ERR_INVALID, "unknown dtype %d", dtype);
    if (!p || !pc || !out) return fail(RSP_ERR_INVALID, "null argument");
    if ((rc = begin_sync(p))) return rc;
    const size_t cols = (size_t)G * n_maps, nin = cols * P, nout = cols * n, esz = p->esz;
    if ((rc = dev_reserve(p->mtd_in, nin * esz)) || (rc = dev_reserve(p->mtd_out, nout * esz))) return rc;
    hipStream_t s = p->lanes[0].stream;
    const void* src;
    if ((rc = host_in_plan_prec(p, pc, dtype, nin, &src))) return rc;
    HIPCHK(hipMemcpyAsync(p->mtd_in.p, src, nin * esz, hipMemcpyHostToDevice, s));
    if ((rc = mtd_run(p, mtd_desc(P, G, n_maps, n, shift, win != nullptr, p->g.prec), p->mtd_in.p, win, p->mtd_out.p, s)))
        return rc;
    return download_widened(p, p->mtd_out.p, nout, out, s);   // its wait: the caller's cube (or the staging buffer) is borrowed for the call
}

int32_t rsp_mtd_device(rsp_plan* p, int32_t P, int32_t G, int32_t n_maps, int32_t nfft, const void* d_pc,
                       const double* win, int32_t shift, void* d_out) {
    int n = 0;
    int rc = rsp_mtd_check_sizes(P, G, n_maps, nfft, plan_dtype(p), &n);
    if (rc) return rc;
    if (!p || !d_pc || !d_out) return fail(RSP_ERR_INVALID, "null argument");
    const size_t cols = (size_t)G * n_maps;
    const char *a = static_cast<const char*>(d_pc), *b = static_cast<const char*>(d_out);
    if (a < b + cols * n * p->esz && b < a + cols * P * p->esz) return fail(RSP_ERR_INVALID, "d_pc and d_out overlap");
    if ((uintptr_t)d_pc % p->esz || (uintptr_t)d_out % p->esz)
        return fail(RSP_ERR_INVALID, "d_pc and d_out must be aligned to a complex element (%zu bytes)", p->esz);
    if ((rc = begin_sync(p))) return rc;
    hipStream_t s = p->lanes[0].stream;
    if ((rc = mtd_run(p, mtd_desc(P, G, n_maps, n, shift, win != nullptr, p->g.prec), d_pc, win, d_out, s))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    return RSP_OK;
}

int32_t rsp_profile_mtd(rsp_plan* p, int32_t P, int32_t G, int32_t n_maps, int32_t nfft, int32_t iters, float* ms_out,
                        int64_t* bytes_out) {
    if (!p || iters < 1 || !ms_out) return fail(RSP_ERR_INVALID, "bad argument");
    int n = 0;
    int rc = rsp_mtd_check_sizes(P, G, n_maps, nfft, plan_dtype(p), &n);
    if (rc) return rc;
    if ((rc = begin_sync(p))) return rc;
    const size_t cols = (size_t)G * n_maps;
    if ((rc = dev_reserve(p->mtd_in, cols * P * p->esz)) || (rc = dev_reserve(p->mtd_out, cols * n * p->esz))) return rc;
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
    int rc = dev_reserve(p->det_axes, h.size() * sizeof(double));
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
    if ((rc = dev_reserve(p->det_smap, cells * p->rsz))) return rc;
    const DetDesc dd{V, G, B, 0, cplx};
    HIPCHK(launch_pairsum(dd, prec, layout, d_x, p->det_smap.p, L.stream));
    const void* smap = p->det_smap.p;
    rc = cfar_launch_grow(p, xd, false, smap, np, false, false, false, true, n_hits);
    if (rc || *n_hits == 0) return rc;
    if ((rc = dev_reserve(p->det_dets, sizeof(DevDet) * (size_t)*n_hits))) return rc;
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
    const int rl = frame_lists_out(tg, p->last_dets, out);
    if (out->cfar_maps && (rc = plan_maps_to_matlab<double, float>(p, p->det_smap.p, xd.P, xd.G, B - 1, out->cfar_maps))) return rc;
    return rl;
}

// A host cube of `elems` complex values into buf in the plan's precision, on stream s (borrowed until the sync)
static int det_upload(rsp_plan* p, rsp_plan::DevBuf& buf, const void* src, int dtype, size_t elems, hipStream_t s) {
    int rc = dev_reserve(buf, elems * p->esz);
    if (rc || (rc = host_in_plan_prec(p, src, dtype, elems, &src))) return rc;
    HIPCHK(hipMemcpyAsync(buf.p, src, elems * p->esz, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    return RSP_OK;
}

int32_t rsp_detect(rsp_plan* p, int32_t V, int32_t G, int32_t B, const void* rdm, int32_t dtype,
                   const rsp_detect_params* prm, rsp_frame_out* out) {
    XcDesc xd;
    int rc = rsp_detect_check_sizes(V, G, B, plan_dtype(p), prm ? &prm->cfar : nullptr, &xd);
    if (rc) return rc;   // refusals before any device work
    if (dtype != RSP_C64 && dtype != RSP_C128) return fail(RSP_ERR_INVALID, "unknown dtype %d", dtype);
    if ((rc = det_args(p, rdm, prm, out, false))) return rc;
    if ((rc = begin_sync(p))) return rc;
    DevConsts k;
    if ((rc = det_consts(p, V, G, B, prm, &k))) return rc;
    if ((rc = det_upload(p, p->det_in, rdm, dtype, (size_t)V * G * B, p->lanes[0].stream))) return rc;
    return det_run(p, xd, B, DET_LAYOUT_MATLAB, p->det_in.p, k, prm->monopulse, prm->cluster, out);
}

int32_t rsp_detect_device(rsp_plan* p, int32_t V, int32_t G, int32_t B, const void* d_rdm, const rsp_detect_params* prm,
                          rsp_frame_out* out) {
    XcDesc xd;
    int rc = rsp_detect_check_sizes(V, G, B, plan_dtype(p), prm ? &prm->cfar : nullptr, &xd);
    if (rc || (rc = det_args(p, d_rdm, prm, out, false))) return rc;
    if ((uintptr_t)d_rdm % p->esz) return fail(RSP_ERR_INVALID, "d_rdm must be aligned to a complex element (%zu bytes)", p->esz);
    if ((rc = begin_sync(p))) return rc;
    DevConsts k;
    if ((rc = det_consts(p, V, G, B, prm, &k))) return rc;
    return det_run(p, xd, B, DET_LAYOUT_MATLAB, d_rdm, k, prm->monopulse, prm->cluster, out);
}

// MTD to n rows (shift = 1) of the pc cube [P x G x B] in p->mtd_in into p->mtd_out, the detector on it, and
// out->rdm: the back half of rsp_mtd_detect and of the two compositions from the pulse compression on (sizes
// checked, k and mtd_out set up)
static int mtd_detect_tail(rsp_plan* p, int P, int G, int B, int n, const XcDesc& xd, const DevConsts& k, const double* win,
                           const rsp_detect_params* prm, rsp_frame_out* out, hipStream_t s) {
    int rc = mtd_run(p, mtd_desc(P, G, B, n, 1, win != nullptr, p->g.prec), p->mtd_in.p, win, p->mtd_out.p, s);
    if (rc) return rc;
    const int rr = det_run(p, xd, B, DET_LAYOUT_MATLAB, p->mtd_out.p, k, prm->monopulse, prm->cluster, out);
    if (rr && rr != RSP_ERR_OVERFLOW) return rr;
    // the cube; a blocking copy on the null stream (the lane's is idle: det_run waited for it)
    if (out && out->rdm && (rc = download_widened(p, p->mtd_out.p, (size_t)G * B * n, out->rdm, nullptr))) return rc;
    return rr;
}

int32_t rsp_mtd_detect(rsp_plan* p, int32_t P, int32_t G, int32_t B, int32_t nfft, const void* pc, int32_t dtype,
                       const double* win, const rsp_detect_params* prm, rsp_frame_out* out) {
    int n = 0;
    XcDesc xd;
    int rc = rsp_mtd_check_sizes(P, G, B, nfft, plan_dtype(p), &n);
    if (rc || (rc = rsp_detect_check_sizes(n, G, B, plan_dtype(p), prm ? &prm->cfar : nullptr, &xd))) return rc;
    if (dtype != RSP_C64 && dtype != RSP_C128) return fail(RSP_ERR_INVALID, "unknown dtype %d", dtype);
    if ((rc = det_args(p, pc, prm, out, true))) return rc;
    if ((rc = begin_sync(p))) return rc;
    hipStream_t s = p->lanes[0].stream;
    const size_t nout = (size_t)G * B * n;
    DevConsts k;
    if ((rc = det_consts(p, n, G, B, prm, &k)) || (rc = dev_reserve(p->mtd_out, nout * p->esz))) return rc;
    if ((rc = det_upload(p, p->mtd_in, pc, dtype, (size_t)G * B * P, s))) return rc;
    return mtd_detect_tail(p, P, G, B, n, xd, k, win, prm, out, s);
}

int32_t rsp_process_stage2_detect(rsp_plan* p, const void* iq, int32_t dtype, rsp_frame_out* out) {
    if (!p || !iq) return fail(RSP_ERR_INVALID, "null argument");
    const rsp_cfar_params prm{p->g.refV, p->g.guardV, p->g.refR, p->g.guardR, p->g.T};
    XcDesc xd;
    int rc = rsp_detect_check_sizes(p->g.P, p->g.G, p->g.B, plan_dtype(p), &prm, &xd);   // refusals before any device work
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
    int rc = rsp_detect_check_sizes(V, G, B, plan_dtype(p), prm, &xd);
    if (rc) return rc;
    if ((rc = begin_sync(p))) return rc;
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
        if ((rc = dev_reserve(p->pc_rec, std::max<size_t>(rec.size(), 1) * sizeof(K2Rec)))) return rc;
        if (!rec.empty()) HIPCHK(hipMemcpy(p->pc_rec.p, rec.data(), rec.size() * sizeof(K2Rec), hipMemcpyHostToDevice));
        p->pc_d = d;
    }
    const PcDesc& d = p->pc_d;
    if ((rc = dev_reserve(p->pc_z, d.z_elems * p->esz)) || (rc = dev_reserve(p->pc_res, d.out_elems * p->esz))) return rc;
    return dev_reserve(p->pc_mag, d.mag_elems * p->rsz);
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
    if ((rc = begin_sync(p))) return rc;
    hipStream_t s = p->lanes[0].stream;
    const size_t nout = (size_t)P * p->g.G * B;
    if ((rc = dev_reserve(p->pc_out, nout * p->esz)) || (rc = pc_from_host(p, P, B, iq, dtype, p->pc_out.p, s))) return rc;
    return download_widened(p, p->pc_out.p, nout, pc_out, s);
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
    if ((rc = begin_sync(p))) return rc;
    hipStream_t s = p->lanes[0].stream;
    if ((rc = pc_prepare(p, P, B)) || (rc = pc_launches(p, d_beams, p->g.N * P, d_pc, s))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    return RSP_OK;
}

// The size checks of the two compositions after the pulse compression's own: MTD and detector at G = the plan's
static int pc_chain_sizes(const rsp_plan* p, int P, int B, int nfft, const rsp_detect_params* prm, int* n, XcDesc* xd) {
    int rc = rsp_mtd_check_sizes(P, p->g.G, B, nfft, plan_dtype(p), n);
    return rc ? rc : rsp_detect_check_sizes(*n, p->g.G, B, plan_dtype(p), prm ? &prm->cfar : nullptr, xd);
}

int32_t rsp_pc_mtd_detect(rsp_plan* p, int32_t P, int32_t B, int32_t nfft, const void* iq, int32_t dtype, const double* win,
                          const rsp_detect_params* prm, rsp_frame_out* out) {
    int n = 0;
    XcDesc xd;
    int rc = pc_sizes(p, P, B, nullptr);
    if (rc || (rc = pc_chain_sizes(p, P, B, nfft, prm, &n, &xd))) return rc;
    if (dtype != RSP_C64 && dtype != RSP_C128) return fail(RSP_ERR_INVALID, "unknown dtype %d", dtype);
    if ((rc = det_args(p, iq, prm, out, true))) return rc;
    if ((rc = begin_sync(p))) return rc;
    hipStream_t s = p->lanes[0].stream;
    const int G = p->g.G;
    DevConsts k;
    if ((rc = det_consts(p, n, G, B, prm, &k)) || (rc = dev_reserve(p->mtd_out, (size_t)G * B * n * p->esz)) ||
        (rc = dev_reserve(p->mtd_in, (size_t)G * B * P * p->esz)))
        return rc;
    if ((rc = pc_from_host(p, P, B, iq, dtype, p->mtd_in.p, s))) return rc;
    return mtd_detect_tail(p, P, p->g.G, B, n, xd, k, win, prm, out, s);
}

// The checks of rsp_raw_detect for a cube `in` of P x the plan's N x C, in three steps (the entry's dtype check
// lies between the first two), and its buffers: the sizes of the three stages ...
static int raw_sizes(const rsp_plan* p, int P, int C, int B, int nfft, const rsp_detect_params* prm, int* n, XcDesc* xd) {
    int rc = pc_sizes(p, P, B, nullptr);
    if (rc || (rc = rsp_dbf_check_sizes(P, p->g.N, C, B, plan_dtype(p)))) return rc;
    return pc_chain_sizes(p, P, B, nfft, prm, n, xd);
}
// ... the pointers and the weights ...
static int raw_args(const rsp_plan* p, const void* in, int C, int B, const double* W, const rsp_detect_params* prm,
                    const rsp_frame_out* out) {
    const int rc = det_args(p, in, prm, out, true);
    if (rc) return rc;
    if (!W && (B != p->g.B || C != p->g.C))
        return fail(RSP_ERR_INVALID, "W = NULL takes the plan's weights, %d x %d; the call has B=%d C=%d", p->g.B, p->g.C, B, C);
    return RSP_OK;
}
// ... and, the queue drained, the detector's constants and the scratch of every stage
static int raw_reserve(rsp_plan* p, int P, int C, int B, int n, const rsp_detect_params* prm, DevConsts* k, DbfDesc* dd) {
    const int G = p->g.G;
    const size_t S = (size_t)P * p->g.N, esz = p->esz;
    int rc;
    if ((rc = det_consts(p, n, G, B, prm, k)) || (rc = dev_reserve(p->mtd_out, (size_t)G * B * n * esz)) ||
        (rc = dev_reserve(p->mtd_in, (size_t)G * B * P * esz)) || (rc = dbf_reserve(p, (int)S, C, B, dd)))
        return rc;
    return pc_prepare(p, P, B);
}

int32_t rsp_raw_detect(rsp_plan* p, int32_t P, int32_t C, int32_t B, int32_t nfft, const void* cube, int32_t dtype,
                       const double* W, int32_t conj, const double* win, const rsp_detect_params* prm, rsp_frame_out* out) {
    int n = 0;
    XcDesc xd;
    int rc = raw_sizes(p, P, C, B, nfft, prm, &n, &xd);
    if (rc) return rc;
    if (dtype != RSP_C64 && dtype != RSP_C128) return fail(RSP_ERR_INVALID, "unknown dtype %d", dtype);
    if ((rc = raw_args(p, cube, C, B, W, prm, out))) return rc;
    if ((rc = begin_sync(p))) return rc;
    hipStream_t s = p->lanes[0].stream;
    const size_t S = (size_t)P * p->g.N;
    DevConsts k;
    DbfDesc dd;
    if ((rc = raw_reserve(p, P, C, B, n, prm, &k, &dd))) return rc;
    if ((rc = dbf_launch_host(p, dd, S, C, B, cube, dtype, W ? W : p->h_W.data(), conj, s))) return rc;
    HIPCHK(hipStreamSynchronize(s));   // the caller's cube (or the staging buffer) is borrowed until here
    if ((rc = pc_launches(p, p->dbf_out.p, dd.opitch, p->mtd_in.p, s))) return rc;
    return mtd_detect_tail(p, P, p->g.G, B, n, xd, k, win, prm, out, s);
}

int32_t rsp_profile_pc(rsp_plan* p, int32_t P, int32_t B, int32_t iters, float* ms_out, int64_t* bytes_out) {
    int rc = pc_sizes(p, P, B, nullptr);   // sizes first, as the other calls of the section
    if (rc) return rc;
    if (iters < 1 || !ms_out) return fail(RSP_ERR_INVALID, "bad argument");
    if ((rc = begin_sync(p))) return rc;
    hipStream_t s = p->lanes[0].stream;
    if ((rc = pc_prepare(p, P, B))) return rc;
    const PcDesc& d = p->pc_d;
    if ((rc = dev_reserve(p->pc_in, d.in_elems * p->esz)) || (rc = dev_reserve(p->pc_out, d.out_elems * p->esz))) return rc;
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

// ---- digital down-conversion: k_ddc ----
// The size checks of a call and its kernel argument.  Without a parameter block the filter cannot be judged:
// only the refusals of P, N and C come first, the null check follows.
static int ddc_sizes(const rsp_plan* p, int64_t P, int64_t N, int64_t C, const rsp_ddc_params* prm, DdcDesc* d) {
    const int rc = prm ? rsp_ddc_derive(P, N, C, prm->L, prm->D, prm->off, plan_dtype(p), d)
                       : rsp_ddc_derive(P, N, C, 1, 1, 0, plan_dtype(p), d);
    if (rc || !prm) return rc;
    d->mode = prm->mode;
    d->w = prm->w;
    d->w0 = prm->w0;
    return RSP_OK;
}

// ... and of its pointers and mode
static int ddc_args(const rsp_plan* p, const void* x, const rsp_ddc_params* prm, const void* out) {
    if (!p || !x || !prm || !prm->h || !out) return fail(RSP_ERR_INVALID, "null argument");
    if (prm->mode != RSP_DDC_NCO_IQ && prm->mode != RSP_DDC_NCO_SIN)
        return fail(RSP_ERR_INVALID, "mode must be RSP_DDC_NCO_IQ or RSP_DDC_NCO_SIN, got %d", prm->mode);
    return RSP_OK;
}

// The taps in the plan's precision and one k_ddc launch on device memory (sizes checked, queue drained)
static int ddc_run(rsp_plan* p, const DdcDesc& d, const double* h, const void* d_x, void* d_y, hipStream_t s) {
    int rc = dev_reserve(p->ddc_h, (size_t)d.L * p->rsz);
    if (rc || (rc = p->put_reals(p->ddc_h.p, h, d.L))) return rc;
    HIPCHK(launch_ddc(d, p->g.prec, d_x, p->ddc_h.p, d_y, s));
    return RSP_OK;
}

// A host cube of reals into p->ddc_in in the plan's precision on stream s (borrowed until the sync)
static int ddc_upload(rsp_plan* p, const DdcDesc& d, const void* x, int dtype, hipStream_t s) {
    const size_t reals = (size_t)d.P * d.N * d.C;
    const void* src;
    int rc = dev_reserve(p->ddc_in, reals * p->rsz);
    if (rc || (rc = host_reals_in_plan_prec(p, x, dtype == RSP_R64, reals, &src))) return rc;
    HIPCHK(hipMemcpyAsync(p->ddc_in.p, src, reals * p->rsz, hipMemcpyHostToDevice, s));
    return RSP_OK;
}

int32_t rsp_ddc(rsp_plan* p, int32_t P, int32_t N, int32_t C, const void* x, int32_t dtype, const rsp_ddc_params* prm,
                double* out) {
    DdcDesc d;
    int rc = ddc_sizes(p, P, N, C, prm, &d);
    if (rc) return rc;   // refusals before any device work
    if (dtype != RSP_R32 && dtype != RSP_R64) return fail(RSP_ERR_INVALID, "unknown dtype %d (RSP_R32 or RSP_R64)", dtype);
    if ((rc = ddc_args(p, x, prm, out))) return rc;
    if ((rc = begin_sync(p))) return rc;
    hipStream_t s = p->lanes[0].stream;
    const size_t nout = (size_t)P * d.No * C;
    if ((rc = dev_reserve(p->ddc_out, std::max<size_t>(nout, 1) * p->esz)) || (rc = ddc_upload(p, d, x, dtype, s)) ||
        (rc = ddc_run(p, d, prm->h, p->ddc_in.p, p->ddc_out.p, s)))
        return rc;
    return download_widened(p, p->ddc_out.p, nout, out, s);   // its wait: the caller's cube (or the staging buffer) is borrowed for the call
}

int32_t rsp_ddc_device(rsp_plan* p, int32_t P, int32_t N, int32_t C, const void* d_x, const rsp_ddc_params* prm, void* d_out) {
    DdcDesc d;
    int rc = ddc_sizes(p, P, N, C, prm, &d);
    if (rc || (rc = ddc_args(p, d_x, prm, d_out))) return rc;
    const size_t nin = (size_t)P * N * C, nout = (size_t)P * d.No * C;
    const char *a = static_cast<const char*>(d_x), *b = static_cast<const char*>(d_out);
    if (a < b + nout * p->esz && b < a + nin * p->rsz) return fail(RSP_ERR_INVALID, "d_x and d_out overlap");
    if ((uintptr_t)d_x % p->rsz || (uintptr_t)d_out % p->esz)
        return fail(RSP_ERR_INVALID, "d_x must be aligned to a real (%zu bytes) and d_out to a complex element (%zu bytes)", p->rsz,
                    p->esz);
    if ((rc = begin_sync(p))) return rc;
    hipStream_t s = p->lanes[0].stream;
    if ((rc = ddc_run(p, d, prm->h, d_x, d_out, s))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    return RSP_OK;
}

int32_t rsp_ddc_raw_detect(rsp_plan* p, int32_t P, int32_t N, int32_t C, const void* x, int32_t dtype, const rsp_ddc_params* prm,
                           int32_t B, int32_t nfft, const double* W, int32_t conj, const double* win,
                           const rsp_detect_params* dprm, rsp_frame_out* out) {
    DdcDesc d;
    int n = 0;
    XcDesc xd;
    int rc = ddc_sizes(p, P, N, C, prm, &d);
    if (rc) return rc;
    if (dtype != RSP_R32 && dtype != RSP_R64) return fail(RSP_ERR_INVALID, "unknown dtype %d (RSP_R32 or RSP_R64)", dtype);
    if ((rc = ddc_args(p, x, prm, x))) return rc;
    if (d.No != p->g.N)
        return fail(RSP_ERR_INVALID, "the down-converter gives No = %d samples a pulse, the plan's point_PRT is %d", d.No, p->g.N);
    if ((rc = raw_sizes(p, P, C, B, nfft, dprm, &n, &xd)) || (rc = raw_args(p, x, C, B, W, dprm, out))) return rc;
    if ((rc = begin_sync(p))) return rc;
    hipStream_t s = p->lanes[0].stream;
    DevConsts k;
    DbfDesc dd;
    if ((rc = raw_reserve(p, P, C, B, n, dprm, &k, &dd)) || (rc = ddc_upload(p, d, x, dtype, s))) return rc;
    ddc_set_opitch(&d, (unsigned)dd.pitch, (unsigned)p->esz);   // the IQ cube straight into k_dbf's channel planes
    if ((rc = ddc_run(p, d, prm->h, p->ddc_in.p, p->dbf_in.p, s))) return rc;
    if ((rc = dbf_launch_planes(p, dd, C, B, W ? W : p->h_W.data(), conj, s))) return rc;
    HIPCHK(hipStreamSynchronize(s));   // the caller's cube (or the staging buffer) is borrowed until here
    if ((rc = pc_launches(p, p->dbf_out.p, dd.opitch, p->mtd_in.p, s))) return rc;
    return mtd_detect_tail(p, P, p->g.G, B, n, xd, k, win, dprm, out, s);
}

int32_t rsp_profile_ddc(rsp_plan* p, int32_t P, int32_t N, int32_t C, int32_t L, int32_t D, int32_t off, int32_t iters,
                        float* ms_out, int64_t* bytes_out) {
    DdcDesc d;
    int rc = rsp_ddc_derive(P, N, C, L, D, off, plan_dtype(p), &d);   // sizes first, as the other calls of the section
    if (rc) return rc;
    if (!p || iters < 1 || !ms_out) return fail(RSP_ERR_INVALID, "bad argument");
    if (d.No < 1) return fail(RSP_ERR_INVALID, "N=%d, off=%d: no output to time", N, off);
    if ((rc = begin_sync(p))) return rc;
    hipStream_t s = p->lanes[0].stream;
    d.mode = RSP_DDC_NCO_IQ;
    d.w = 0x199999999999999Aull;   // 2^64 / 10
    if ((rc = dev_reserve(p->ddc_in, d.in_bytes)) || (rc = dev_reserve(p->ddc_out, d.out_bytes)) ||
        (rc = dev_reserve(p->ddc_h, (size_t)L * p->rsz)))
        return rc;
    HIPCHK(hipMemsetAsync(p->ddc_in.p, 0, d.in_bytes, s));   // zeros, and zero taps: the time does not depend on the values
    HIPCHK(hipMemsetAsync(p->ddc_h.p, 0, (size_t)L * p->rsz, s));
    auto run = [&]() -> int {
        HIPCHK(launch_ddc(d, p->g.prec, p->ddc_in.p, p->ddc_h.p, p->ddc_out.p, s));
        return RSP_OK;
    };
    if ((rc = time_launches(s, iters, run, ms_out))) return rc;
    if (bytes_out) *bytes_out = (int64_t)d.in_bytes + (int64_t)d.out_bytes;
    return RSP_OK;
}
}  // extern "C"
