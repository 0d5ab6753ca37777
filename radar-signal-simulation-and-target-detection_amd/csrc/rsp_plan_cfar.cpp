// rsp_plan_cfar.cpp -- the stage-2 calls of librsp's host runtime (beams or a raw cube into PC_results
// and MTD_results) and the CFAR call family on their result or on a caller's amplitude maps: the stage-3
// range CFAR, the Doppler CA-CFAR and the cross GOCA-CFAR, each as map call, stage 2 on beams, on gated
// beams, on a raw cube, and profile.  The entry shapes are written once, over the detector's descriptor.
#include "rsp_plan.h"

#include <cstring>

namespace {

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
        int rc = dev_reserve(p->raw_tab, t.size() * p->rsz);
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
    int rc = begin_sync(p);
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

// PC_results and MTD_results of the last stage2_device to the host, each optional
int stage2_out(rsp_plan* p, double* mtd_out, double* pc_out) {
    int rc;
    if (pc_out && (rc = rdm_out(p, p->lanes[0].rdm, pc_out))) return rc;
    if (mtd_out && (rc = rdm_out(p, p->d_aux, mtd_out))) return rc;
    return RSP_OK;
}

// The raw cube of a raw-cube stage-2 call as the full-PRT [P x N x C] the device takes: the caller's, or
// (n_gated != 0) its gated columns put back at their PRT positions in `full`
int raw_full_prt(const rsp_plan* p, const void* cube, int dtype, int n_gated, const int32_t* cols,
                 std::vector<unsigned char>& full, const void** out) {
    *out = cube;
    if (!n_gated) return dtype == RSP_C64 || dtype == RSP_C128 ? RSP_OK : fail(RSP_ERR_INVALID, "unknown dtype %d", dtype);
    const int rc = rsp_stage2_regate(p->g.P, p->g.N, p->g.C, cube, dtype, n_gated, cols, full);
    *out = full.data();
    return rc;
}

// ---- the CFAR call family ----
// A detector is its descriptor type D (S3Desc: the stage-3 range CFAR, VcDesc: the Doppler CA-CFAR, XcDesc:
// the cross GOCA-CFAR), cfar_derive: the descriptor of the plan's shape from the detector's parameters, and
// cfar_launch: its launcher.  (The descriptor of a caller's shape is the map entry's own rsp_*_derive call.)
struct CfarDev {   // device outputs of one launch, each optional (launch_s3's trailing arguments)
    double *amp, *thr;
    uint8_t* flags;
    rsp_stage3_hit* hits;
    int* count;
    int cap;
};

int cfar_derive(const rsp_plan* p, const rsp_stage3_cfar_params* prm, S3Desc* d) { return rsp_stage3_derive(p->g.P, p->gates, prm, d); }
int cfar_derive(const rsp_plan* p, const rsp_vcfar_params* prm, VcDesc* d) { return rsp_vcfar_derive(p->g.P, p->g.G, prm, d); }
int cfar_derive(const rsp_plan* p, const rsp_cfar_params* prm, XcDesc* d) { return rsp_xcfar_derive(p->g.P, p->g.G, prm, d); }

hipError_t cfar_launch(const S3Desc& d, int prec, bool cplx, const void* in, int n_maps, const CfarDev& o, hipStream_t s) {
    return launch_s3(d, prec, cplx, in, n_maps, o.amp, o.thr, o.flags, o.hits, o.count, o.cap, s);
}
hipError_t cfar_launch(const VcDesc& d, int prec, bool cplx, const void* in, int n_maps, const CfarDev& o, hipStream_t s) {
    return launch_vcfar(d, prec, cplx, in, n_maps, o.amp, o.thr, o.flags, o.hits, o.count, o.cap, s);
}
hipError_t cfar_launch(const XcDesc& d, int prec, bool cplx, const void* in, int n_maps, const CfarDev& o, hipStream_t s) {
    return launch_xcfar(d, prec, cplx, in, n_maps, o.amp, o.thr, o.flags, o.hits, o.count, o.cap, s);
}

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

// The plan's device buffers of a run over `cells` cells: the maps asked for, and the counter with (list) a
// hit list to start from; cfar_list_cap: the records the list holds now
int cfar_reserve(rsp_plan* p, size_t cells, bool amp, bool thr, bool flags, bool list) {
    int rc;
    if (amp && (rc = dev_reserve(p->s3_amp, cells * 8))) return rc;
    if (thr && (rc = dev_reserve(p->s3_thr, cells * 8))) return rc;
    if (flags && (rc = dev_reserve(p->s3_flags, cells))) return rc;
    if ((rc = dev_reserve(p->s3_count, 16))) return rc;
    return list ? dev_reserve(p->s3_hits, sizeof(rsp_stage3_hit) * std::min<size_t>(cells, 65536)) : RSP_OK;
}
int cfar_list_cap(const rsp_plan* p) { return (int)std::min<size_t>(p->s3_hits.cap / sizeof(rsp_stage3_hit), (size_t)INT32_MAX); }

}  // namespace

int stage2_device(rsp_plan* p, const void* iq, int dtype) { return stage2_device(p, Stage2In{iq, dtype, false, nullptr, 1}); }

template <class D>
int cfar_launch_grow(rsp_plan* p, const D& d, bool cplx, const void* d_in, int n_maps, bool amp, bool thr, bool flags,
                     bool list, int* total_out) {
    Lane& L = p->lanes[0];
    const size_t cells = (size_t)n_maps * d.P * d.G;
    int rc = cfar_reserve(p, cells, false, false, false, list);
    if (rc) return rc;
    int total = 0;
    for (int pass = 0;; ++pass) {
        const int cap = list ? cfar_list_cap(p) : 0;
        HIPCHK(hipMemsetAsync(p->s3_count.p, 0, 4, L.stream));
        HIPCHK(cfar_launch(d, p->g.prec, cplx, d_in, n_maps,
                           CfarDev{amp ? (double*)p->s3_amp.p : nullptr, thr ? (double*)p->s3_thr.p : nullptr,
                                   flags ? (uint8_t*)p->s3_flags.p : nullptr, list ? (rsp_stage3_hit*)p->s3_hits.p : nullptr,
                                   (int*)p->s3_count.p, cap},
                           L.stream));
        HIPCHK(hipStreamSynchronize(L.stream));
        HIPCHK(hipMemcpy(&total, p->s3_count.p, 4, hipMemcpyDeviceToHost));
        if (!list || total <= cap) break;
        if (pass > 0) return fail(RSP_ERR_DEVICE, "CFAR hit count changed between two runs on the same map");
        if ((rc = dev_reserve(p->s3_hits, sizeof(rsp_stage3_hit) * (size_t)total))) return rc;   // every hit, then again
    }
    *total_out = total;
    return RSP_OK;
}
template int cfar_launch_grow<XcDesc>(rsp_plan*, const XcDesc&, bool, const void*, int, bool, bool, bool, bool, int*);   // rsp_plan_calls.cpp's

namespace {

// A CFAR kernel over the n_maps device maps d_in (complex: the stage-2 result; else real amplitudes of the
// plan's precision) on lane 0's stream (cfar_launch_grow), then the requested outputs to the host.
template <class D>
int cfar_run(rsp_plan* p, const D& d, bool cplx, const void* d_in, int n_maps, const S3Out& o) {
    const int P = d.P, G = d.G;
    const bool list = o.hits && o.hits_cap > 0;
    int total = 0;
    int rc = cfar_reserve(p, (size_t)n_maps * P * G, o.amp != nullptr, o.thr != nullptr, o.flags != nullptr, false);
    if (rc || (rc = cfar_launch_grow(p, d, cplx, d_in, n_maps, o.amp != nullptr, o.thr != nullptr, o.flags != nullptr, list, &total)))
        return rc;
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

// MATLAB column-major amplitude maps [P x G x n] -> p->s3_in as [n][P][G] in the plan's precision
int cfar_upload_maps(rsp_plan* p, const double* amp, int P, int G, int n_maps) {
    const size_t cells = (size_t)n_maps * P * G, rs = p->rsz;
    std::vector<unsigned char> host(cells * rs);
    if (rs == 8) rsp_transpose_planes(amp, G, P, n_maps, reinterpret_cast<double*>(host.data()));
    else rsp_transpose_planes(amp, G, P, n_maps, reinterpret_cast<float*>(host.data()));
    int rc = dev_reserve(p->s3_in, cells * rs);
    if (rc) return rc;
    HIPCHK(hipMemcpy(p->s3_in.p, host.data(), cells * rs, hipMemcpyHostToDevice));
    return RSP_OK;
}

// The map call: the detector of d (derived from the caller's shape, after s3_args) on the caller's maps
template <class D>
int cfar_map(rsp_plan* p, const D& d, const double* amp, int n_maps, const S3Out& o) {
    int rc = rsp_s3_check_cells(d.P, d.G, n_maps);   // refusals before any device work
    if (rc) return rc;
    if ((rc = begin_sync(p)) || (rc = cfar_upload_maps(p, amp, d.P, d.G, n_maps))) return rc;
    return cfar_run(p, d, false, p->s3_in.p, n_maps, o);
}

// Stage 2 of `in`, then the detector on its MTD_results (arguments checked)
template <class D, class Prm>
int cfar_fused(rsp_plan* p, const Stage2In& in, const Prm* prm, double* mtd_out, const S3Out& o) {
    D d;
    int rc = cfar_derive(p, prm, &d);   // refusals before any device work
    if (rc || (rc = rsp_s3_check_cells(d.P, d.G, p->g.B)) || (rc = stage2_device(p, in))) return rc;
    if (mtd_out && (rc = rdm_out(p, p->d_aux, mtd_out))) return rc;
    return cfar_run(p, d, true, p->d_aux, p->g.B, o);
}

// The entry on beams [P x N x B] ...
template <class D, class Prm>
int cfar_beams(rsp_plan* p, const void* iq, int dtype, const Prm* prm, double* mtd_out, const S3Out& o) {
    const int rc = s3_args(p, iq, prm, o.hits_cap);
    return rc ? rc : cfar_fused<D>(p, Stage2In{iq, dtype, false, nullptr, 1}, prm, mtd_out, o);
}

// ... on gated beams [P x n_gated x B] ...
template <class D, class Prm>
int cfar_gated(rsp_plan* p, const void* iq, int dtype, int n_gated, const int32_t* cols, const Prm* prm, double* mtd_out,
               const S3Out& o) {
    D d;
    int rc = s3_args(p, iq, prm, o.hits_cap);
    if (rc || (rc = cfar_derive(p, prm, &d))) return rc;   // before the re-insertion's work too
    std::vector<unsigned char> full;
    if ((rc = rsp_stage2_regate(p->g.P, p->g.N, p->g.B, iq, dtype, n_gated, cols, full))) return rc;
    return cfar_fused<D>(p, Stage2In{full.data(), dtype, false, nullptr, 1}, prm, mtd_out, o);
}

// ... and on a raw cube [P x N x C] (n_gated != 0: its gated columns) with the weights of its DBF
template <class D, class Prm>
int cfar_raw(rsp_plan* p, const void* cube, int dtype, int n_gated, const int32_t* cols, const double* W, int conj,
             const Prm* prm, double* mtd_out, const S3Out& o) {
    D d;
    int rc = s3_args(p, cube, prm, o.hits_cap);
    if (rc || (rc = cfar_derive(p, prm, &d))) return rc;   // before the re-insertion's work too
    std::vector<unsigned char> full;
    const void* src;
    if ((rc = raw_full_prt(p, cube, dtype, n_gated, cols, full, &src))) return rc;
    return cfar_fused<D>(p, Stage2In{src, dtype, true, W, conj}, prm, mtd_out, o);
}

// The three timed forms of a CFAR kernel over the B beams of the plan's last stage-2 result (what
// rsp_profile_stage3 documents)
template <class D, class Prm>
int cfar_profile(rsp_plan* p, const Prm* prm, int iters, float* ms_out, int64_t* bytes_out) {
    if (!p || !prm || iters < 1) return fail(RSP_ERR_INVALID, "bad argument");
    D d;
    int rc = cfar_derive(p, prm, &d);
    if (rc || (rc = rsp_s3_check_cells(d.P, d.G, p->g.B))) return rc;
    if (!p->aux_valid) return fail(RSP_ERR_INVALID, "no stage-2 result on the device: call rsp_process_stage2 first");
    if ((rc = begin_sync(p))) return rc;
    Lane& L = p->lanes[0];
    const int B = p->g.B, prec = p->g.prec;
    const size_t cells = (size_t)B * d.P * d.G;
    if ((rc = cfar_reserve(p, cells, true, true, true, true)) || (rc = dev_reserve(p->s3_in, cells * p->rsz))) return rc;
    double* amp = (double*)p->s3_amp.p;
    double* thr = (double*)p->s3_thr.p;
    uint8_t* fl = (uint8_t*)p->s3_flags.p;
    rsp_stage3_hit* hits = (rsp_stage3_hit*)p->s3_hits.p;
    int* cnt = (int*)p->s3_count.p;
    const int cap = cfar_list_cap(p);
    {   // the real form's input: the magnitudes the complex form writes, in the plan's precision
        HIPCHK(hipMemsetAsync(cnt, 0, 4, L.stream));
        HIPCHK(cfar_launch(d, prec, true, p->d_aux, B, CfarDev{amp, nullptr, nullptr, nullptr, cnt, 0}, L.stream));
        HIPCHK(hipStreamSynchronize(L.stream));
        std::vector<double> a(cells);
        HIPCHK(hipMemcpy(a.data(), amp, cells * 8, hipMemcpyDeviceToHost));
        if ((rc = p->put_reals(p->s3_in.p, a.data(), cells))) return rc;
    }
    for (int s = 0; s < 3; ++s) {
        auto run = [&]() -> hipError_t {
            hipError_t e = hipMemsetAsync(cnt, 0, 4, L.stream);
            if (e != hipSuccess) return e;
            if (s == 0) return cfar_launch(d, prec, false, p->s3_in.p, B, CfarDev{nullptr, thr, fl, nullptr, cnt, 0}, L.stream);
            if (s == 1) return cfar_launch(d, prec, true, p->d_aux, B, CfarDev{amp, thr, fl, nullptr, cnt, 0}, L.stream);
            return cfar_launch(d, prec, true, p->d_aux, B, CfarDev{nullptr, nullptr, nullptr, hits, cnt, cap}, L.stream);
        };
        float ms = 0;
        if ((rc = time_launches(L.stream, iters, [&]() -> int { HIPCHK(run()); return RSP_OK; }, &ms))) return rc;
        if (ms_out) ms_out[s] = ms;
    }
    if (bytes_out) rsp_stage3_bytes((int64_t)cells, (int)p->esz, bytes_out);
    return RSP_OK;
}

}  // namespace

// =========================================================================================
extern "C" {

int32_t rsp_process_stage2(rsp_plan* p, const void* iq, int32_t dtype, double* mtd_out, double* pc_out) {
    if (!p || !iq) return fail(RSP_ERR_INVALID, "null argument");
    const int rc = stage2_device(p, iq, dtype);
    return rc ? rc : stage2_out(p, mtd_out, pc_out);
}

int32_t rsp_process_stage2_gated(rsp_plan* p, const void* iq, int32_t dtype, int32_t n_gated, const int32_t* cols,
                                 double* mtd_out, double* pc_out) {
    if (!p || !iq) return fail(RSP_ERR_INVALID, "null argument");
    std::vector<unsigned char> full;
    int rc = rsp_stage2_regate(p->g.P, p->g.N, p->g.B, iq, dtype, n_gated, cols, full);
    if (rc) return rc;
    return rsp_process_stage2(p, full.data(), dtype, mtd_out, pc_out);
}

int32_t rsp_process_raw_stage2(rsp_plan* p, const void* cube, int32_t dtype, int32_t n_gated, const int32_t* cols,
                               const double* W, int32_t conj, double* mtd_out, double* pc_out) {
    if (!p || !cube) return fail(RSP_ERR_INVALID, "null argument");
    std::vector<unsigned char> full;
    const void* src;
    int rc = raw_full_prt(p, cube, dtype, n_gated, cols, full, &src);
    if (rc || (rc = stage2_device(p, Stage2In{src, dtype, true, W, conj}))) return rc;
    return stage2_out(p, mtd_out, pc_out);
}

// ---- stage-3 range CFAR ----
int32_t rsp_stage3_cfar_shape(rsp_plan* p, int32_t P, const int32_t* gates, const double* amp, int32_t n_maps,
                              const rsp_stage3_cfar_params* prm, uint8_t* flags, double* threshold, rsp_stage3_hit* hits,
                              int64_t hits_cap, int64_t* n_hits) {
    S3Desc d;
    int rc = s3_args(p, gates && amp ? amp : nullptr, prm, hits_cap);
    if (rc || (rc = rsp_stage3_derive(P, gates, prm, &d))) return rc;
    return cfar_map(p, d, amp, n_maps, S3Out{nullptr, flags, threshold, hits, hits_cap, n_hits});
}

int32_t rsp_stage3_cfar(rsp_plan* p, const double* amp, int32_t n_maps, const rsp_stage3_cfar_params* prm, uint8_t* flags,
                        double* threshold, rsp_stage3_hit* hits, int64_t hits_cap, int64_t* n_hits) {
    if (!p) return fail(RSP_ERR_INVALID, "null argument");
    return rsp_stage3_cfar_shape(p, p->g.P, p->gates, amp, n_maps, prm, flags, threshold, hits, hits_cap, n_hits);
}

int32_t rsp_process_stage2_cfar(rsp_plan* p, const void* iq, int32_t dtype, const rsp_stage3_cfar_params* prm,
                                double* mtd_out, double* amp_out, uint8_t* flags, double* threshold, rsp_stage3_hit* hits,
                                int64_t hits_cap, int64_t* n_hits) {
    return cfar_beams<S3Desc>(p, iq, dtype, prm, mtd_out, S3Out{amp_out, flags, threshold, hits, hits_cap, n_hits});
}

int32_t rsp_process_stage2_gated_cfar(rsp_plan* p, const void* iq, int32_t dtype, int32_t n_gated, const int32_t* cols,
                                      const rsp_stage3_cfar_params* prm, double* mtd_out, double* amp_out, uint8_t* flags,
                                      double* threshold, rsp_stage3_hit* hits, int64_t hits_cap, int64_t* n_hits) {
    return cfar_gated<S3Desc>(p, iq, dtype, n_gated, cols, prm, mtd_out, S3Out{amp_out, flags, threshold, hits, hits_cap, n_hits});
}

int32_t rsp_process_raw_stage2_cfar(rsp_plan* p, const void* cube, int32_t dtype, int32_t n_gated, const int32_t* cols,
                                    const double* W, int32_t conj, const rsp_stage3_cfar_params* prm, double* mtd_out,
                                    double* amp_out, uint8_t* flags, double* threshold, rsp_stage3_hit* hits,
                                    int64_t hits_cap, int64_t* n_hits) {
    return cfar_raw<S3Desc>(p, cube, dtype, n_gated, cols, W, conj, prm, mtd_out,
                            S3Out{amp_out, flags, threshold, hits, hits_cap, n_hits});
}

int32_t rsp_profile_stage3(rsp_plan* p, const rsp_stage3_cfar_params* prm, int32_t iters, float* ms_out, int64_t* bytes_out) {
    return cfar_profile<S3Desc>(p, prm, iters, ms_out, bytes_out);
}

// ---- Doppler CA-CFAR ----
int32_t rsp_vcfar(rsp_plan* p, int32_t P, int32_t G, const double* amp, int32_t n_maps, const rsp_vcfar_params* prm,
                  uint8_t* flags, double* threshold, rsp_stage3_hit* hits, int64_t hits_cap, int64_t* n_hits) {
    VcDesc d;
    int rc = s3_args(p, amp, prm, hits_cap);
    if (rc || (rc = rsp_vcfar_derive(P, G, prm, &d))) return rc;
    return cfar_map(p, d, amp, n_maps, S3Out{nullptr, flags, threshold, hits, hits_cap, n_hits});
}

int32_t rsp_process_stage2_vcfar(rsp_plan* p, const void* iq, int32_t dtype, const rsp_vcfar_params* prm, double* mtd_out,
                                 double* amp_out, uint8_t* flags, double* threshold, rsp_stage3_hit* hits, int64_t hits_cap,
                                 int64_t* n_hits) {
    return cfar_beams<VcDesc>(p, iq, dtype, prm, mtd_out, S3Out{amp_out, flags, threshold, hits, hits_cap, n_hits});
}

int32_t rsp_process_stage2_gated_vcfar(rsp_plan* p, const void* iq, int32_t dtype, int32_t n_gated, const int32_t* cols,
                                       const rsp_vcfar_params* prm, double* mtd_out, double* amp_out, uint8_t* flags,
                                       double* threshold, rsp_stage3_hit* hits, int64_t hits_cap, int64_t* n_hits) {
    return cfar_gated<VcDesc>(p, iq, dtype, n_gated, cols, prm, mtd_out, S3Out{amp_out, flags, threshold, hits, hits_cap, n_hits});
}

int32_t rsp_process_raw_stage2_vcfar(rsp_plan* p, const void* cube, int32_t dtype, int32_t n_gated, const int32_t* cols,
                                     const double* W, int32_t conj, const rsp_vcfar_params* prm, double* mtd_out,
                                     double* amp_out, uint8_t* flags, double* threshold, rsp_stage3_hit* hits,
                                     int64_t hits_cap, int64_t* n_hits) {
    return cfar_raw<VcDesc>(p, cube, dtype, n_gated, cols, W, conj, prm, mtd_out,
                            S3Out{amp_out, flags, threshold, hits, hits_cap, n_hits});
}

int32_t rsp_profile_vcfar(rsp_plan* p, const rsp_vcfar_params* prm, int32_t iters, float* ms_out, int64_t* bytes_out) {
    return cfar_profile<VcDesc>(p, prm, iters, ms_out, bytes_out);
}

// ---- cross GOCA-CFAR as a map detector ----
int32_t rsp_xcfar(rsp_plan* p, int32_t P, int32_t G, const double* amp, int32_t n_maps, const rsp_cfar_params* prm,
                  uint8_t* flags, double* threshold, rsp_stage3_hit* hits, int64_t hits_cap, int64_t* n_hits) {
    XcDesc d;
    int rc = s3_args(p, amp, prm, hits_cap);
    if (rc || (rc = rsp_xcfar_derive(P, G, prm, &d))) return rc;
    return cfar_map(p, d, amp, n_maps, S3Out{nullptr, flags, threshold, hits, hits_cap, n_hits});
}

int32_t rsp_process_stage2_xcfar(rsp_plan* p, const void* iq, int32_t dtype, const rsp_cfar_params* prm, double* mtd_out,
                                 double* amp_out, uint8_t* flags, double* threshold, rsp_stage3_hit* hits, int64_t hits_cap,
                                 int64_t* n_hits) {
    return cfar_beams<XcDesc>(p, iq, dtype, prm, mtd_out, S3Out{amp_out, flags, threshold, hits, hits_cap, n_hits});
}

int32_t rsp_process_stage2_gated_xcfar(rsp_plan* p, const void* iq, int32_t dtype, int32_t n_gated, const int32_t* cols,
                                       const rsp_cfar_params* prm, double* mtd_out, double* amp_out, uint8_t* flags,
                                       double* threshold, rsp_stage3_hit* hits, int64_t hits_cap, int64_t* n_hits) {
    return cfar_gated<XcDesc>(p, iq, dtype, n_gated, cols, prm, mtd_out, S3Out{amp_out, flags, threshold, hits, hits_cap, n_hits});
}

int32_t rsp_process_raw_stage2_xcfar(rsp_plan* p, const void* cube, int32_t dtype, int32_t n_gated, const int32_t* cols,
                                     const double* W, int32_t conj, const rsp_cfar_params* prm, double* mtd_out,
                                     double* amp_out, uint8_t* flags, double* threshold, rsp_stage3_hit* hits,
                                     int64_t hits_cap, int64_t* n_hits) {
    return cfar_raw<XcDesc>(p, cube, dtype, n_gated, cols, W, conj, prm, mtd_out,
                            S3Out{amp_out, flags, threshold, hits, hits_cap, n_hits});
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
    int rc = cfar_derive(p, &prm, &d);
    if (rc || (rc = rsp_s3_check_cells(d.P, d.G, p->g.B - 1))) return rc;
    if ((rc = begin_sync(p))) return rc;
    return cfar_run(p, d, false, p->d_smap, p->g.B - 1, S3Out{nullptr, flags, threshold, hits, hits_cap, n_hits});
}

int32_t rsp_profile_xcfar(rsp_plan* p, const rsp_cfar_params* prm, int32_t iters, float* ms_out, int64_t* bytes_out) {
    return cfar_profile<XcDesc>(p, prm, iters, ms_out, bytes_out);
}

}  // extern "C"
