// rsp_internal.h -- device-side descriptors and launchers of librsp (not part of the C-ABI).  The
// plan descriptors (Geometry, SegDesc, K2Job, K1Route) and every sizing decision are in
// rsp_geometry.h, which needs no HIP.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rsp_geometry.h"
#include "rsp_music_geometry.h"

#define RSP_LANES 4          // max streams of the throughput queue (batches in flight)
#define RSP_NLANES 3         // streams the throughput queue uses (<= RSP_LANES)
#define K2_THREADS 256       // threads per pulse-compression workgroup (16 points each)
#define RSP_THREADS 256
// The kernel variants measured and not kept (profiles/EXPERIMENTS.md) were removed in round 6;
// the library has one code path per configuration and no compile-time A/B switches.

// Philox4x32-10 (Salmon et al., SC'11) in place on counter c with key (k0, k1); the streams
// built on it are documented in oracle/philox.py (echo noise) and oracle/music.py (MUSIC).
__device__ __forceinline__ void rsp_philox10(uint32_t c[4], uint32_t k0, uint32_t k1) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)M0 * c[0];
        const uint64_t p1 = (uint64_t)M1 * c[2];
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// Device record of one CFAR detection + its S9 estimate; layout == rsp_detection.
struct DevDet {
    int32_t v_idx, r_idx, pair_idx, reserved;   // 1-based like fsf:220
    double amp, range, velocity, angle;
};

// Per-frame device buffers of one launch.  Element types follow Geometry::prec: complex
// values are (re, im) pairs of float or double, maps are float or double.
struct FramePtrs {
    const void* in[RSP_MAX_F];     // K1 input cube (PNC) or beam cube
    void* z[RSP_MAX_F];            // compacted Doppler-domain rows
    void* rdm[RSP_MAX_F];          // [B][P][G] complex
    void* mag[RSP_MAX_F];          // |rdm| [B][P][Gp] (K2 epilogue, read by K3)
    void* smap[RSP_MAX_F];         // optional: rdm_for_cfar_all [B-1][P][G] as K3 thresholds it (fsf:184-187)
    unsigned long long* trace;     // diagnostic builds (-DRSP_DEBUG_KNOBS): 4 stamps per workgroup
    DevDet* dets[RSP_MAX_F];
    // record 0 of a frame's detection list: [0] detections, [1] deferred cells, [2] edge rows
    // computed on demand; zeroed by K1 (in the pipeline) with the frame's flag block
    int* count[RSP_MAX_F];
    // band route (else null): RSP_NEED_BYTES flags of the frame's edge rows, byte b 2hV + e for edge
    // row e of beam b, and its deferred cells, (pair << 16 | v, r) each
    unsigned char* need[RSP_MAX_F];
    int2* defer[RSP_MAX_F];
};

struct DevConsts {
    const void* Atab;        // DBF MFMA A operands per lane: [MB][CP/4][Re,Im][64] (rsp_dbf_atab), real
    const void* win;         // MTD window [P], real
    const void* twP;         // W_P^i table (direct DFT path), complex
    const void* twPp;        // per-pass Stockham twiddles of the P-point FFT, complex
    const void* twD;         // persistent K1's in-place FFT: [i][n2] = W_P^(n2 2^i), i < 4, n2 < P/16, complex
    const void* twQ;         // factored DFT (P = R Q): [fset][n - 1][r] = (cos, sin)(2 pi k n / Q), k = RQ_RK fset + r
    const void* taps;        // narrow FIR taps, real
    const void* H;           // overlap-save spectra, 1/M scaled, complex
    const void* twM;         // per-pass Stockham twiddles of each overlap-save block size, complex
    const K2Rec* k2rec;      // pulse-compression workgroups in dispatch order (job kinds interleaved), a record each
    const double* range_axis;
    const double* velocity_axis;
    const double* beam_angles;
    const double* klut;
    double deltaR, deltaV;
};

// Launchers of the frame chain, each in its stage's unit: launch_k1 (rsp_k1.hip), launch_k2* (rsp_k2.hip),
// launch_k3 (rsp_k3.hip), launch_stream_copy / launch_mtd_cols / launch_synth / launch_dets_to_host
// (rsp_frame_aux.hip).  `mode` bits for K1: 1 = apply DBF, 2 = apply MTD.
hipError_t launch_k1(const Geometry& g, const DevConsts& k, const FramePtrs& fp, int nf, int mode, hipStream_t s);
hipError_t launch_stream_copy(const void* in, void* out, size_t n16, int ncu, hipStream_t s);
// K2 of every row (the plan's table k.k2rec), or of one row set with its record table; on_demand:
// the edge set, each workgroup only if fp.need flags one of its rows
hipError_t launch_k2(const Geometry& g, const DevConsts& k, const FramePtrs& fp, int nf, hipStream_t s);
hipError_t launch_k2_set(const Geometry& g, const DevConsts& k, const FramePtrs& fp, int nf, const K2Rows& rows,
                         const K2Rec* recs, int nwg, bool on_demand, hipStream_t s);
// K3: whole (K3_WHOLE), or the band route's two phases: K3_DEFER leaves the cells whose test reads an
// edge row on fp.defer and flags those rows in fp.need; K3_FINISH (after the on-demand K2) tests them.
// defer_cap: entries of each frame's deferred list.
enum { K3_WHOLE = 0, K3_DEFER = 1, K3_FINISH = 2 };
hipError_t launch_k3(const Geometry& g, const DevConsts& k, const FramePtrs& fp, int nf, hipStream_t s,
                     int phase = K3_WHOLE, int defer_cap = 0);
hipError_t launch_mtd_cols(const Geometry& g, const DevConsts& k, const void* pc, void* rdm, hipStream_t s);
// S4 + S4.1: tab holds RSP_MAX_SYNTH_TARGETS x (P + C) complex doubles (the per-target phasors)
hipError_t launch_synth(const Geometry& g, const double* tx, const SynthTargets& tg, int nt, void* tab, int frame_idx,
                        uint64_t seed, double noise_scale, void* cube, hipStream_t s);
// Stage-3 range CFAR (rsp_stage3.hip) of n_maps maps [n_maps][P][G], range fastest: `in` holds
// complex values of the precision (cplx: the stage-2 result, magnitudes by cmag) or real
// amplitudes.  Outputs, each optional: amp / thr as double, flags as bytes (same layout), hits
// (rsp_stage3_hit records, any order, the first hits_cap of them) counted in *count, which the
// caller zeroes.
hipError_t launch_s3(const S3Desc& d, int prec, bool cplx, const void* in, int n_maps, double* amp, double* thr,
                     uint8_t* flags, rsp_stage3_hit* hits, int* count, int hits_cap, hipStream_t s);
// Doppler CA-CFAR (rsp_vcfar.hip) of n_maps maps [n_maps][P][G]: inputs and outputs as launch_s3's.
hipError_t launch_vcfar(const VcDesc& d, int prec, bool cplx, const void* in, int n_maps, double* amp, double* thr,
                        uint8_t* flags, rsp_stage3_hit* hits, int* count, int hits_cap, hipStream_t s);
// Cross GOCA-CFAR (rsp_xcfar.hip) of n_maps maps [n_maps][P][G]: inputs and outputs as launch_s3's;
// `in` starts on a 16-byte boundary.
hipError_t launch_xcfar(const XcDesc& d, int prec, bool cplx, const void* in, int n_maps, double* amp, double* thr,
                        uint8_t* flags, rsp_stage3_hit* hits, int* count, int hits_cap, hipStream_t s);
// Stand-alone DBF (rsp_dbf.hip): d.C channel planes x at d.pitch -> d.B beam planes y at d.opitch, both
// complex of the precision, 16-B aligned; At = rsp_dbf_atab's table in the precision's row layout
// (double DBF_ROWS_SPLIT, float DBF_ROWS_PAIR) as reals of the precision.
hipError_t launch_dbf(const DbfDesc& d, int prec, const void* x, const void* At, void* y, hipStream_t s);
// Stand-alone MTD of any length (rsp_mtd.hip): pc [P x G x n_maps] -> out [nfft x G x n_maps], complex of
// the precision; win = P reals of the precision (d.has_win), tab = rsp_mtd_tables' w | Bf (chirp-z route)
// and tw = rsp_mtd_twiddles' tables of d.lgL, complex of the precision.  d.vec says which sides of a
// complex-single launch are 16-byte aligned.
hipError_t launch_mtd(const MtdDesc& d, int prec, const void* pc, const void* win, const void* tab, const void* tw,
                      void* out, hipStream_t s);
// Detection on any RD cube (rsp_detect.hip).  launch_pairsum: the complex cube x of d.V x d.G x d.B in
// `layout` (DET_LAYOUT_*) -> the pair-sum maps S [B - 1][V][G], reals of the precision; d.vec is set here from
// the pointers.  launch_s9: S9 of the n records `hits` of launch_xcfar on S (beam_idx = the pair) into dets[0 .. n),
// in the list's order; k gives the axes, angles, K-LUT and cell sizes (device pointers), d.cplx the monopulse form.
hipError_t launch_pairsum(DetDesc d, int prec, int layout, const void* x, void* S, hipStream_t s);
hipError_t launch_s9(const DetDesc& d, int prec, int layout, const DevConsts& k, const void* x, const void* S,
                     const rsp_stage3_hit* hits, int n, DevDet* dets, hipStream_t s);
// Pulse compression for any pulse and beam count (rsp_pc.hip), around launch_k2_set on d.g / d.rows.
// launch_pc_pack: beams [P x N x B] (pulse fastest, beam planes `pitch` elements apart) -> z of d.z_elems,
// 16-byte aligned; launch_pc_unpack: k2_pc's result [B][P][G] -> pc [P x G x B].  Complex of the precision;
// either launcher takes element pairs in complex single where the caller's side is aligned for them.
hipError_t launch_pc_pack(const PcDesc& d, const void* beams, int pitch, void* z, hipStream_t s);
hipError_t launch_pc_unpack(const PcDesc& d, const void* res, void* pc, hipStream_t s);
// Digital down-conversion (rsp_ddc.hip): x [P x N x C] reals of the precision -> y [P x No x C] complex of the
// precision, its channel planes d.opitch elements apart; h = d.L taps as reals of the precision (device memory);
// d.mode, d.w and d.w0 are the call's.  y is aligned to a complex element; x takes 16-byte loads where it is
// aligned for them.  d.No = 0: no launch.
hipError_t launch_ddc(const DdcDesc& d, int prec, const void* x, const void* h, void* y, hipStream_t s);
// Queue read-back: count record + the detections of nf frames (device stride dcap + 1 records) into
// mapped pinned host memory (stride hcap + 1), only the records that exist.
hipError_t launch_dets_to_host(const void* dets, int dcap, void* host, int hcap, int nf, hipStream_t s);
// MUSIC (rsp_music.hip): one stage (MusicStage) of a call's route over n_inst instances, and the
// snapshot synthesis.  buf: the plan's device buffers by MusicBuf; dX: snapshots in the plan's precision.
hipError_t launch_music_stage(int stage, const MusicDesc& d, const MusicRoute& r, void* const* buf, const void* dX,
                              int n_inst, hipStream_t s);
hipError_t launch_music_synth(const MusicDesc& d, const MusicSynth& sy, void* const* buf, int n_inst, int inst0,
                              uint64_t seed, void* dX, hipStream_t s);
