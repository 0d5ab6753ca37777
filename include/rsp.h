/*
 * rsp.h -- C-ABI of the MI355X radar signal-processing library (librsp.so).
 *
 * Drop-in boundary for the per-frame chain of the MATLAB reference
 * (XuZerui2023/Radar-Signal-Simulation-and-Target-Detection, Simulation/):
 *
 *   final_targets = fun_process_single_frame(targets, config, cfar_params,
 *                       cluster_params, precomputed_data, frame_idx)
 *                                              (fun_process_single_frame.m:13)
 *   [MTD_results, PC_results] = process_stage2_mtd(iq_data, angle, config)
 *                                              (process_stage2_mtd.m:1)
 *
 * The reference has no FFI; these entry points are what a MEX gateway or a
 * MATLAB `loadlibrary`/`calllib` binding of that path binds.
 * Plain C types only: pointers, sizes, int32 status codes.
 *
 * Conventions (mirroring MATLAB so a MEX gateway passes mxArray data as is):
 *   - complex arrays are interleaved (re, im) doubles (mxGetComplexDoubles,
 *     R2018a API) or interleaved floats (RSP_C64);
 *   - matrices are column-major; the echo cube is [P x N x C] (pulse fastest),
 *     range-Doppler maps [P x G x B], CFAR maps [P x G x (B-1)];
 *   - indices reported to the caller are 1-based (fun_process_single_frame.m:220);
 *   - segment starts in rsp_precomputed are 1-based (v8:116-117,130).
 * Arithmetic: a plan computes in complex double (RSP_C128, MATLAB's double as in
 * fun_process_single_frame.m:47,92,101,131 -- the default) or, on request, complex
 * single (RSP_C64); device-resident cubes and maps are in the plan's precision.
 * Errors: every function returns RSP_OK (0) or a negative rsp_status; the
 * message of the last failure on the calling thread is rsp_last_error().
 * Threading: a plan is not thread-safe; use one plan per host thread (MATLAB
 * parfor workers are processes, each with its own plan).
 */
#ifndef RSP_H
#define RSP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSP_ABI_VERSION 4

typedef enum rsp_status {
    RSP_OK = 0,
    RSP_ERR_INVALID = -1,      /* bad argument / inconsistent config            */
    RSP_ERR_UNSUPPORTED = -2,  /* config outside what the kernels implement      */
    RSP_ERR_DEVICE = -3,       /* HIP runtime failure                            */
    RSP_ERR_NOMEM = -4,        /* device or host allocation failed               */
    RSP_ERR_OVERFLOW = -5      /* a caller-sized output buffer is too small      */
} rsp_status;

typedef enum rsp_dtype {
    RSP_C64 = 1,   /* interleaved complex float  */
    RSP_C128 = 2,  /* interleaved complex double (MATLAB) */
    RSP_R32 = 3,   /* real float: rsp_ddc's input only   */
    RSP_R64 = 4    /* real double: rsp_ddc's input only  */
} rsp_dtype;

typedef enum rsp_layout {
    RSP_LAYOUT_PNC = 0   /* MATLAB column-major [P x N x C]: index m + P*(n + N*c) */
} rsp_layout;

/* config.Sig_Config + config.Array (main_simulate_echoes_with_array_v8.m:54-69). */
typedef struct rsp_sig_config {
    double c;                 /* Sig_Config.c                       */
    double fs;                /* Sig_Config.fs                      */
    double fc;                /* Sig_Config.fc                      */
    double prt;               /* Sig_Config.prt (s)                 */
    double wavelength;        /* Sig_Config.wavelength              */
    double element_spacing;   /* Array.element_spacing (m)          */
    int32_t prtNum;           /* P: pulses per frame                */
    int32_t point_PRT;        /* N: fast-time samples per pulse     */
    int32_t channel_num;      /* C                                  */
    int32_t beam_num;         /* B                                  */
} rsp_sig_config;

/* cfar_params (v8:45-47). Only 'GOCA' exists in fun_process_single_frame; the range CFAR of the
 * stage-2 path, with its greatest-of / smallest-of switch, is rsp_stage3_cfar_params below. */
typedef struct rsp_cfar_params {
    int32_t refCells_V, guardCells_V, refCells_R, guardCells_R;
    double T_CFAR;
} rsp_cfar_params;

/* cluster_params (v8:49-51). */
typedef struct rsp_cluster_params {
    double max_range_sep, max_vel_sep, max_angle_sep;
} rsp_cluster_params;

/* precomputed_data (v8:79-155).  Arrays are borrowed for rsp_plan_create only. */
typedef struct rsp_precomputed {
    const double* tx_pulse;            /* complex, point_PRT entries (synthesis; may be NULL) */
    double P_signal_unscaled;
    const double* DBF_coeffs_data_C;   /* complex, B x C column-major                        */
    const double* MF_narrow;           /* real FIR taps                                      */
    int32_t n_MF_narrow;
    int32_t fir_delay;
    const double* MF_medium_fft;       /* complex, N_fft_med entries                          */
    int32_t N_fft_med;
    const double* MF_long_fft;         /* complex, N_fft_long entries                         */
    int32_t N_fft_long;
    int32_t N_gate_narrow, N_gate_medium, N_gate_long, N_total_gate;
    int32_t seg_start_narrow, seg_start_medium, seg_start_long;   /* 1-based */
    const double* MTD_win;             /* prtNum                                              */
    const double* range_axis;          /* N_total_gate                                        */
    const double* velocity_axis;       /* prtNum                                              */
    double deltaR, deltaV;
    const double* beam_angles_deg;     /* beam_num                                            */
    const double* k_slopes_LUT;        /* beam_num - 1                                        */
} rsp_precomputed;

/* targets(k) of the driver (v8:29-37). */
typedef struct rsp_target_in {
    double Range, Velocity, ElevationAngle, SNR_dB;
} rsp_target_in;

/* One entry of final_targets / intra_beam_targets (fun_process_single_frame.m:393-406). */
typedef struct rsp_target {
    double Range, Velocity, Angle, Power;
} rsp_target;

/* One row of all_raw_detections (fsf:220, 1-based v/r/pair, the CFAR map value)
 * together with its S9 estimate (fsf:293-297). */
typedef struct rsp_detection {
    int32_t v_idx, r_idx, pair_idx, reserved;
    double amp;
    double Range, Velocity, Angle;
} rsp_detection;

/* Caller-owned outputs of one frame.  Any pointer may be NULL (not produced).
 * Sizes from rsp_query_sizes. */
typedef struct rsp_frame_out {
    double* rdm;              /* complex, [P x G x B] column-major (rdm_13beam, fsf:135)        */
    double* cfar_maps;        /* real, [P x G x (B-1)] (rdm_for_cfar_all, fsf:187)             */
    rsp_detection* dets;      /* parameterized detections in reference order                   */
    int32_t dets_cap;
    int32_t n_dets;           /* out                                                           */
    rsp_target* targets;      /* final_targets                                                 */
    int32_t targets_cap;
    int32_t n_targets;        /* out                                                           */
} rsp_frame_out;

typedef struct rsp_sizes {
    int64_t cube_elems;       /* P*N*C complex samples                      */
    int64_t rdm_elems;        /* P*G*B                                      */
    int64_t cfar_map_elems;   /* P*G*(B-1)                                  */
    int32_t P, N, C, B, G;
    int32_t used_samples;     /* fast-time samples the chain actually reads */
    int32_t max_detections;   /* most detections a frame can have (cells under
                                 test of every beam pair); the device lists
                                 start smaller and grow on demand           */
    int32_t n_stages;         /* device stages (for rsp_profile_stages)     */
    int32_t precision;        /* RSP_C128 or RSP_C64: device cube / map type */
    int32_t elem_bytes;       /* bytes of one device complex element (16/8) */
} rsp_sizes;

typedef struct rsp_plan rsp_plan;

int32_t rsp_abi_version(void);
const char* rsp_last_error(void);

/* Plan options (rsp_plan_options_default fills the defaults shown). */
#define RSP_PLAN_K1_TILED 1   /* force the one-tile-per-workgroup K1 instead of the persistent
                                 one (both compute the same operations; parity tests compare them) */
#define RSP_PLAN_MONOPULSE_COMPLEX 2   /* S9's angle from the complex ratio
                                 real((S_A - S_B) / (S_A + S_B + eps)) of the RD map, as the inline S9
                                 of main_plot_snr_vs_angle_error.m:455-462, instead of fsf:282-290's
                                 amplitude ratio (|S_A| - |S_B|) / (|S_A| + |S_B| + eps).  K2 then
                                 writes every frame's complex RD map (the caller's, or plan-owned) */
#define RSP_PLAN_K2_ALL_ROWS 4   /* the queue pulse-compresses every Doppler row of every frame.
                                 Without it a plan whose CFAR window is the compile-time 5/5/10/10
                                 one computes the rows under test, [hV, prtNum - hV) with hV = 15, and
                                 of the rows outside them only those a detection reads (rsp_k2_row_set);
                                 the results are the same bit for bit.  For tests and A/B timing */
typedef struct rsp_plan_options {
    int32_t device;              /* HIP device ordinal (0)                                   */
    int32_t frames_per_launch;   /* frames batched into each kernel launch by the queue (1)  */
    int32_t precision;           /* RSP_C128 (MATLAB double, default) or RSP_C64             */
    int32_t flags;               /* RSP_PLAN_* (0)                                           */
} rsp_plan_options;
int32_t rsp_plan_options_default(rsp_plan_options* opt);

/* Build a plan: uploads DBF weights, FIR taps, matched-filter spectra (re-blocked for
 * overlap-save), MTD window, axes, angles, K-LUT in the plan's precision.
 * `frames_per_launch` (1..8) frames are batched into each kernel launch by the
 * queue interface; rsp_process_* always run one frame.  rsp_plan_create = the defaults
 * with `device` and `frames_per_launch` (complex double). */
int32_t rsp_plan_create_ex(const rsp_sig_config* cfg, const rsp_cfar_params* cfar,
                           const rsp_cluster_params* cluster, const rsp_precomputed* pre,
                           const rsp_plan_options* opt, rsp_plan** out);
int32_t rsp_plan_create(const rsp_sig_config* cfg, const rsp_cfar_params* cfar,
                        const rsp_cluster_params* cluster, const rsp_precomputed* pre,
                        int32_t device, int32_t frames_per_launch, rsp_plan** out);
int32_t rsp_plan_destroy(rsp_plan* plan);
int32_t rsp_query_sizes(const rsp_plan* plan, rsp_sizes* out);

/* Which slow-time transform the plan runs (read-only; the decision is the one the launchers
 * take, for prtNum, beam_num, channel_num, the precision and RSP_PLAN_K1_TILED).  Tests assert
 * it, so that a change of the plan's heuristics cannot silently move a case off the kernel it
 * is there to cover. */
#define RSP_K1_KERNEL_TILED 0                 /* k1_dbf_mtd: one tile per workgroup            */
#define RSP_K1_KERNEL_PERSISTENT 1            /* k1p_dbf_mtd: power-of-two P, double-buffered  */
#define RSP_K1_KERNEL_PERSISTENT_FACTORED 2   /* k1q_dbf_mtd: P = R Q                          */
#define RSP_K1_TRANSFORM_STOCKHAM 0           /* out-of-place radix passes                     */
#define RSP_K1_TRANSFORM_DIF 1                /* in-place decimation in frequency              */
#define RSP_K1_TRANSFORM_FACTORED 2           /* P = R Q: radix-R stage + folded Q-point DFT   */
#define RSP_K1_TRANSFORM_DIRECT 3             /* O(P^2) DFT                                    */
typedef struct rsp_k1_route {
    int32_t kernel;           /* RSP_K1_KERNEL_*                                               */
    int32_t transform;        /* RSP_K1_TRANSFORM_*                                            */
    int32_t R, Q;             /* the factored transform's P = R Q; 0, 0 otherwise              */
    int32_t NT;               /* fast-time samples per tile                                    */
    int32_t Ppad;             /* LDS stride of a tile column (>= P)                            */
    int32_t tiles_per_wave;   /* MFMA sub-tiles a wave loads per tile in the persistent
                                 kernels; 0 for the tiled kernel                               */
    int32_t stage2_lgp;       /* rsp_process_stage2's column transform: log2 P for the FFT
                                 instantiations (P = 16 .. 512), 0 for the direct DFT          */
} rsp_k1_route;
int32_t rsp_query_k1_route(const rsp_plan* plan, rsp_k1_route* out);

/* How the plan tiles the CFAR/S9 kernel k3_cfar for its window, prtNum, gates and precision
 * (read-only; the fields the launcher and the kernel read).  Tests assert it, so that a case
 * runs the kernel path and the Doppler band count it is there to cover. */
typedef struct rsp_k3_tiling {
    int32_t fast;             /* 1: the compile-time 5/5/10/10 kernel, tiles without halo; 0: the
                                 generic kernel, tiles with the window halo                    */
    int32_t RT;               /* range cells under test per tile                               */
    int32_t hR;               /* range halo of the generic tile, cells on either side          */
    int32_t W;                /* LDS row stride of a tile, cells                               */
    int32_t n_tiles;          /* range tiles per Doppler band and beam pair (<= 0: the window
                                 leaves no range cell under test, K3 writes the maps only)     */
    int32_t n_bands;          /* Doppler bands                                                 */
    int32_t VB;               /* Doppler cells under test per band                             */
    int32_t rows;             /* Doppler rows of a tile in LDS                                 */
} rsp_k3_tiling;
int32_t rsp_query_k3_tiling(const rsp_plan* plan, rsp_k3_tiling* out);

/* How the plan lays out the pulse-compression kernel k2_pc (read-only; the fields the launcher
 * and the kernel read).  One slot per segment of the stitched row: 0 narrow (direct FIR), 1 medium,
 * 2 long (overlap-save).  Tests assert it, so that a case runs the instantiation, the block size
 * and the block count it is there to cover. */
typedef struct rsp_k2_segment {
    int32_t present;          /* 0: the segment has no gate; every other field is then 0        */
    int32_t type;             /* 0: direct FIR, 1: FFT overlap-save                             */
    int32_t ga, gb;           /* stitched gates [ga, gb), 0-based                               */
    int32_t seg_lo;           /* 0-based first fast-time sample of the segment                  */
    int32_t lo, hi;           /* 0-based sample window that reaches a kept gate, inclusive      */
    int32_t Ls, ntaps, delay; /* FIR: segment length (the circshift's modulus), taps, shift     */
    int32_t Lh, M, V;         /* overlap-save: filter length, block points, M - Lh + 1 gates
                                 per block                                                      */
    int32_t nblocks;          /* overlap-save blocks per row; block b holds the gates
                                 [ga + b V, min(gb, ga + (b + 1) V))                            */
    int32_t rows_per_wg;      /* rows of the [prtNum x beam_num] row set per workgroup          */
} rsp_k2_segment;
typedef struct rsp_k2_layout {
    int32_t k2_pts;           /* complex LDS points per workgroup: 4096 or 2560                 */
    int32_t wg_per_cu;        /* workgroups per CU the launched instantiation is sized for:
                                 4 (k2_pc<T, 4>, k2_pts = 2560) or 2 (k2_pc<T, 2>)              */
    int32_t NZ;               /* samples per slab of the K1 -> K2 buffer (K1's NT)              */
    int32_t nseg, njobs;      /* present segments; (segment, block) jobs                        */
    int32_t nwg;              /* workgroups per frame                                           */
    rsp_k2_segment seg[3];
} rsp_k2_layout;
int32_t rsp_query_k2_layout(const rsp_plan* plan, rsp_k2_layout* out);

/* The pulse-compression workgroups in dispatch order, one record each: what workgroup blockIdx.x of a
 * k2_pc launch reads to find its work.  rsp_k2_layout.nwg records; the first min(cap, nwg) go to
 * `out` (NULL allowed when cap is 0) and nwg to *n (NULL allowed). */
typedef struct rsp_k2_record {
    int32_t seg;              /* index among the present segments (narrow, medium, long order)   */
    int32_t blk;              /* overlap-save block of the segment (0 for the direct FIR)        */
    int32_t row0;             /* first row of the [beam_num x prtNum] row set; rows_per_wg rows  */
    int32_t wg;               /* the workgroup's index in job order: segment by segment, block by
                                 block, ceil(rows / rows_per_wg) workgroups per (segment, block)  */
} rsp_k2_record;
int32_t rsp_query_k2_records(const rsp_plan* plan, rsp_k2_record* out, int32_t cap, int32_t* n);

/* The rows of one pulse-compression launch and its record table.  Row i < total of a set is Doppler
 * row base + j + (j >= split ? gap : 0), j = i mod n, of beam i / n; a record's row0 counts rows of
 * the set.  RSP_K2_ROWS_ALL: every row, the table of rsp_query_k2_records.  RSP_K2_ROWS_BAND: the
 * rows the cross CFAR tests.  RSP_K2_ROWS_EDGE: the hV rows on either side of them, launched after
 * the CFAR for the rows a detection reads.  A plan without the band route (another CFAR window,
 * prtNum <= 2 hV) reports n = total = nwg = 0 and no records for the last two. */
#define RSP_K2_ROWS_ALL 0
#define RSP_K2_ROWS_BAND 1
#define RSP_K2_ROWS_EDGE 2
typedef struct rsp_k2_row_set {
    int32_t n, base, split, gap;
    int32_t total;            /* rows of the launch: beam_num * n                               */
    int32_t nwg;              /* workgroups = records of the table                              */
} rsp_k2_row_set;
int32_t rsp_query_k2_row_set(const rsp_plan* plan, int32_t which, rsp_k2_row_set* set, rsp_k2_record* out,
                             int32_t cap, int32_t* n);

/* What the queue's band route did since the last reset (or the plan's creation): frames that went
 * through launch batches, those of them on the band route, edge rows pulse-compressed on demand
 * (counted once per row, on the first segment's workgroups) and cells whose full CFAR test waited
 * for such rows. */
typedef struct rsp_band_counters {
    int64_t frames, band_frames, edge_rows, deferred_cells;
} rsp_band_counters;
int32_t rsp_band_counters_get(const rsp_plan* plan, rsp_band_counters* out);
int32_t rsp_band_counters_reset(rsp_plan* plan);

/* What rsp_plan_create_ex would build for these arguments on a device of `ncu` compute units,
 * without a device: the same checks (opt->device aside), refusals and messages, and the values
 * rsp_query_sizes and rsp_query_k1_route report for the created plan.  `sizes` / `route` may be
 * NULL.  No HIP call is made, so it runs on a machine without a GPU. */
int32_t rsp_plan_describe(const rsp_sig_config* cfg, const rsp_cfar_params* cfar,
                          const rsp_cluster_params* cluster, const rsp_precomputed* pre,
                          const rsp_plan_options* opt, int32_t ncu, rsp_sizes* sizes, rsp_k1_route* route);
/* The same for rsp_query_k3_tiling's values. */
int32_t rsp_plan_describe_k3(const rsp_sig_config* cfg, const rsp_cfar_params* cfar,
                             const rsp_cluster_params* cluster, const rsp_precomputed* pre,
                             const rsp_plan_options* opt, int32_t ncu, rsp_k3_tiling* tiling);
/* The same for rsp_query_k2_layout's values. */
int32_t rsp_plan_describe_k2(const rsp_sig_config* cfg, const rsp_cfar_params* cfar,
                             const rsp_cluster_params* cluster, const rsp_precomputed* pre,
                             const rsp_plan_options* opt, int32_t ncu, rsp_k2_layout* layout);
/* The same for rsp_query_k2_records' values. */
int32_t rsp_plan_describe_k2_records(const rsp_sig_config* cfg, const rsp_cfar_params* cfar,
                                     const rsp_cluster_params* cluster, const rsp_precomputed* pre,
                                     const rsp_plan_options* opt, int32_t ncu, rsp_k2_record* out, int32_t cap,
                                     int32_t* n);

/* rsp_query_k2_row_set without a device */
int32_t rsp_plan_describe_k2_row_set(const rsp_sig_config* cfg, const rsp_cfar_params* cfar,
                                     const rsp_cluster_params* cluster, const rsp_precomputed* pre,
                                     const rsp_plan_options* opt, int32_t ncu, int32_t which, rsp_k2_row_set* set,
                                     rsp_k2_record* out, int32_t cap, int32_t* n);

/* Cube-in path: S5..S11 of fun_process_single_frame on one host cube
 * (layout RSP_LAYOUT_PNC, dtype RSP_C64 or RSP_C128; converted to the plan's precision
 * only if they differ).  Synchronous.  out->cfar_maps, when requested, is the map K3
 * thresholds on the device (rdm_for_cfar_all, fsf:184-187). */
int32_t rsp_process_cube(rsp_plan* plan, const void* cube, int32_t dtype, int32_t layout,
                         int32_t frame_idx, rsp_frame_out* out);

/* Every detection of the last synchronous frame (rsp_process_cube / rsp_process_targets), in the
 * reference's order.  A frame's list has no fixed capacity (all_raw_detections(end+1,:),
 * fsf:215-221); a caller that passed out->dets == NULL or a dets_cap below out->n_dets reads the
 * whole list here.  *n = its length; RSP_ERR_OVERFLOW if cap < *n (the first cap are copied). */
int32_t rsp_last_detections(const rsp_plan* plan, rsp_detection* dets, int32_t cap, int32_t* n);
/* The final targets of the last synchronous frame, likewise (for out->targets == NULL or a
 * targets_cap below out->n_targets). */
int32_t rsp_last_targets(const rsp_plan* plan, rsp_target* targets, int32_t cap, int32_t* n);

/* Reference-signature path (fsf:13): S4 echo synthesis + S4.1 Philox noise
 * (seed, frame_idx) on the device, then S5..S11.  Needs tx_pulse in the plan. */
int32_t rsp_process_targets(rsp_plan* plan, const rsp_target_in* targets, int32_t n_targets,
                            int32_t frame_idx, uint64_t seed, double p_noise, rsp_frame_out* out);

/* Synthesise (S4 + S4.1) one cube on the device into `d_cube` (the plan's precision,
 * PNC layout, device pointer with cube_elems entries).  Synchronous. */
int32_t rsp_synthesize_device(rsp_plan* plan, const rsp_target_in* targets, int32_t n_targets,
                              int32_t frame_idx, uint64_t seed, double p_noise, void* d_cube);
/* Device time of that synthesis (its two kernels: per-target phasor tables, then the cube),
 * averaged over `iters` back-to-back launches into d_cube, by HIP events on the plan's stream.
 * *bytes_out (may be NULL) = the cube bytes one synthesis writes, C x N x P elements. */
int32_t rsp_profile_synthesis(rsp_plan* plan, const rsp_target_in* targets, int32_t n_targets, int32_t iters,
                              void* d_cube, float* ms_out, int64_t* bytes_out);

/* ---- device-resident queue (throughput path) ----
 * rsp_enqueue_device: process a PNC cube (the plan's precision) already resident in
 * device memory.  Frames are batched frames_per_launch at a time and alternate over the
 * plan's lanes (streams); detections come back asynchronously and are clustered
 * on the host.  rsp_drain waits for everything queued.  Results are kept in
 * enqueue order until rsp_results_clear. */
int32_t rsp_enqueue_device(rsp_plan* plan, const void* d_cube, int32_t frame_idx);
/* rsp_enqueue_device for n frames in one call (d_cubes[i], frame_idx[i]).  All or nothing: a null
 * d_cubes[i] (or d_rdms[i] in the _rdm_n form) is refused before any frame is queued. */
int32_t rsp_enqueue_device_n(rsp_plan* plan, const void* const* d_cubes, const int32_t* frame_idx, int32_t n);
/* rsp_enqueue_device that also produces the frame's complex range-Doppler map rdm_13beam
 * (fsf:131-136, the rsp_mex('cube') output): K2 writes it straight into the caller's device buffer
 * d_rdm (rsp_sizes.rdm_elems complex elements in the plan's precision, device layout [B][P][G],
 * range fastest).  d_rdm must stay allocated, and must not be handed to another frame, until
 * rsp_drain returns; the map is complete then.  Without it (rsp_enqueue_device) the map stays
 * on chip and only |RDM| reaches HBM. */
int32_t rsp_enqueue_device_rdm(rsp_plan* plan, const void* d_cube, int32_t frame_idx, void* d_rdm);
int32_t rsp_enqueue_device_rdm_n(rsp_plan* plan, const void* const* d_cubes, const int32_t* frame_idx,
                                 void* const* d_rdms, int32_t n);
/* End-to-end form of rsp_enqueue_device: a host PNC cube in the plan's precision (no conversion;
 * rsp_process_cube converts).  Only the fast-time samples the chain reads (rsp_sizes.used_samples)
 * are copied, asynchronously on the plan's upload stream into a plan-owned device ring, so
 * uploads overlap the kernels of earlier batches; with pinned memory (rsp_host_alloc) the copy
 * runs at full PCIe rate.  The host cube must stay unchanged until rsp_drain returns. */
int32_t rsp_enqueue_host(rsp_plan* plan, const void* h_cube, int32_t dtype, int32_t frame_idx);
int32_t rsp_host_alloc(rsp_plan* plan, int64_t bytes, void** h_ptr);   /* pinned host memory */
int32_t rsp_host_free(rsp_plan* plan, void* h_ptr);
int32_t rsp_drain(rsp_plan* plan);
int32_t rsp_results_count(const rsp_plan* plan, int32_t* n_frames, int64_t* n_targets);
int32_t rsp_results_get(const rsp_plan* plan, int32_t i, int32_t* frame_idx, rsp_target* targets,
                        int32_t cap, int32_t* n_targets, int32_t* n_dets);
int32_t rsp_results_clear(rsp_plan* plan);
/* Every queued result as rows of 5 doubles (frame_idx, Range, Velocity, Angle, Power), frames in
 * enqueue order, one NaN row for a frame without targets -- the detection-list payload of the
 * multi-GPU gather, in one call.  *n_rows = rows needed (rows == NULL: a size query);
 * RSP_ERR_OVERFLOW if more than cap. */
int32_t rsp_results_rows(const rsp_plan* plan, double* rows, int64_t cap, int64_t* n_rows);

/* ---- multi-GPU frame batch in one process (BASELINE config #3 for a MEX / loadlibrary host) ----
 * The reference's drivers loop over independent frames (main_simulate_echoes_with_array_v8.m:
 * 164-190, fsf:13 per frame).  Frames j = 0 .. n_frames-1 (targets[j], n_targets[j] targets,
 * frame_idx[j]) are split into contiguous shares over the plans -- plan i, typically one per
 * device, takes [i n / n_plans, (i+1) n / n_plans) -- each driven by its own host thread: S4/S4.1
 * synthesis into the plan's device ring, then the throughput queue.  The final targets of frame j
 * are gathered into out[j * cap ...], n_out[j] entries (the detection-list gather, in process
 * memory).  The plans must have no queued frames or uncleared results.  Synchronous. */
int32_t rsp_process_targets_multi(rsp_plan* const* plans, int32_t n_plans, const rsp_target_in* const* targets,
                                  const int32_t* n_targets, const int32_t* frame_idx, int32_t n_frames,
                                  uint64_t seed, double p_noise, rsp_target* out, int32_t cap, int32_t* n_out);

/* Stage-2 path (process_stage2_mtd.m:1): already-beamformed fast-time data
 * iq_data [P x N x B] (PNC layout with B beams) -> PC_results and MTD_results,
 * both complex [P x G x B] column-major (either may be NULL).  The reference's
 * fun_MTD_produce is un-vendored; this backs it with fsf S6 + S7. */
int32_t rsp_process_stage2(rsp_plan* plan, const void* iq_beams, int32_t dtype,
                           double* mtd_out, double* pc_out);
/* Gated stage-2 input, as the v2 `.mat` frames store it (main_simulate_echoes_with_array_v2.m:
 * 256-267): iq_gated [P x n_gated x B] holds, for segment k = narrow, medium, long, the PRT
 * columns cols[2k] .. cols[2k+1] (1-based, inclusive) side by side.  They are put back at
 * their PRT positions (zeros elsewhere) and processed like rsp_process_stage2.
 * cols = NULL: the reference gating 83:310, 311:1033, 1034:3486 (n_gated = 3404). */
int32_t rsp_process_stage2_gated(rsp_plan* plan, const void* iq_gated, int32_t dtype, int32_t n_gated,
                                 const int32_t* cols, double* mtd_out, double* pc_out);

/* ---- Value domain of the magnitudes and of the three map detectors ----
 * Holds for rsp_process_cube / rsp_process_targets (K2's magnitudes, K3), rsp_detect and its
 * compositions, rsp_stage3_cfar, rsp_vcfar, rsp_xcfar and their fused stage-2 forms.  Each statement
 * names the test that asserts it.
 *   Inputs are finite.  The result for a NaN anywhere in the input is unspecified.
 *   Magnitudes |x| of a complex value (x, y): q = RN(RN(x x) + RN(y y)), then the square root to one
 *     ulp.  While q is a normal, finite number -- |x| from about 2^-511 to 2^511 in complex double,
 *     2^-63 to 2^63 in complex single -- the result is within 3u of hypot(x, y), u = 2^-53 or 2^-24,
 *     and a pair sum RN(|a| + |b|) within 4u of |a| + |b|; 0 gives +0 whatever the signs.  Asserted
 *     per element at 2^-500 .. 2^500 (double) and 2^-60 .. 2^60 (single), on axis cells and on cells
 *     whose smaller square is lost, and on the device's own maps with a dynamic range above 1e3
 *     (tests/test_cmag.py).  Outside that interval q under- or overflows and nothing is promised.
 *   Every stage up to the magnitudes is linear and every detector homogeneous: an input scaled by a
 *     power of two inside the interval gives scaled maps and thresholds and the same flags, hits,
 *     detections, Range and Velocity, bit for bit (tests/test_scale_invariance.py: 2^+-300 in complex
 *     double, 2^+-24 in complex single).  Angle holds the reference's absolute eps.
 *   rsp_stage3_cfar and rsp_vcfar are defined to the bit over all finite amplitudes: subnormal cells,
 *     sums and thresholds, and window sums that overflow, whose threshold is +Inf (a cell is then
 *     flagged by >= only if it is +Inf itself, never by >).  A complex-single plan narrows the caller's
 *     doubles first: cells below the float subnormals are 0, cells above FLT_MAX are +Inf, and the
 *     definition applies to those.  T_CFAR is rounded to the plan's precision first
 *     (tests/test_cfar_value_range.py, cases tiny, sub, huge, narrowed, wide, const, zero, T-edge).
 *   rsp_xcfar, rsp_detect and K3: the same in complex single.  In complex double the quotient
 *     sum / n is k3_quot's FMA form, which equals RN(sum / n) wherever that quotient is a normal
 *     number, sum >= n 2^-1022.  Below, where the quotient is subnormal, an exact tie (n even and no
 *     power of two) may round to the other neighbour (tests/test_xcfar_ref.py::
 *     test_fma_quotient_domain, in exact rational arithmetic for n = 1 .. 64).  A window sum of +Inf
 *     gives a threshold of +Inf, as the division's, in the map detector k_xcfar (rsp_xcfar, rsp_detect,
 *     rsp_last_cfar_threshold and the fused forms).  K3, inside rsp_process_cube, forms no threshold
 *     output and does not saturate; its sums are sums of magnitudes inside the interval above and
 *     cannot overflow.  The map detector is asserted to the bit on maps from Rayleigh x 2^-900 upwards
 *     and on overflowing sums; the two cases below the bound are listed as not compared
 *     (tests/_cfar_value_cases.py LEFT_OUT). */

/* ---- stage-3 range CFAR of the stage-2 path ----
 * local_execute_cfar / executeCFAR_2D / Function_CFAR1D_sub of
 * debug_simulated_data_processing_v2.m:419-511, the detector every caller of process_stage2_mtd
 * feeds |MTD| into (:209-213).  Per real amplitude map A [P x G]:
 *   notch (:446-450): zc = round(P/2) + 1; rows max(1, zc - MTD_0v_num) .. min(P, zc + MTD_0v_num)
 *     (1-based) get flag 0 and threshold 0;
 *   segments (:423-439): columns 1..n1, n1+1..n1+n2, n1+n2+1..G (n1 = N_gate_narrow, n2 =
 *     N_gate_medium) are processed on their own, each with edges of its own;
 *   cell y of a segment of n columns (:481-505), r = refCells_R, s = saveCells_R:
 *     L = y-(s+r) .. y-s-1, R = y+s+1 .. y+s+r; mL = mean(L) if y-(s+r) >= 1 else mean(R);
 *     mR = mean(R) if y+s+r <= n else mean(L); u = max(mL, mR) (CFARmethod_R = 0) or min (1);
 *     threshold = u * T_CFAR; flag = A >= threshold.
 * mean = the r cells summed in ascending column order, divided by r.  Every operation is one
 * correctly rounded IEEE operation in the plan's precision (double for RSP_C128, float for
 * RSP_C64; T_CFAR and the amplitudes are rounded to it first), so the result is defined to the
 * bit; thresholds and amplitudes leave the device widened to double.  Not k3_cfar: range only,
 * per segment, >= instead of >, and the threshold matrix is an output. */
typedef struct rsp_stage3_cfar_params {
    int32_t refCells_R, saveCells_R, CFARmethod_R, MTD_0v_num;
    double T_CFAR;
} rsp_stage3_cfar_params;

/* One flagged cell: 1-based Doppler row, range column and map (beam); the amplitude tested and its
 * threshold.  Lists are ordered by beam, then as find() on [P x G]: r_idx outer, v_idx inner. */
typedef struct rsp_stage3_hit {
    int32_t v_idx, r_idx, beam_idx, reserved;
    double amp, threshold;
} rsp_stage3_hit;

/* What the CFAR does with a map of P rows and these segments (rsp_stage3_describe). */
typedef struct rsp_stage3_info {
    int32_t P, G;
    int32_t seg_first[3];     /* 1-based first column of the narrow / medium / long segment      */
    int32_t seg_len[3];       /* their lengths (an empty segment has no cells and no constraint) */
    int32_t notch_first, notch_last;   /* 1-based notched rows, clipped to 1..P (first > last: none) */
    int32_t halo;             /* s + r: cells a window reaches on either side of its cell        */
    int32_t max_halo;         /* the largest s + r the kernel's tile holds                       */
    int32_t chunk;            /* range cells one workgroup of k_s3_cfar resolves per Doppler row  */
    int32_t rows;             /* Doppler rows per workgroup                                      */
} rsp_stage3_info;

/* The checks of the calls below, with the same refusals and messages, and the layout they use,
 * for prtNum of `cfg` and the gate counts of `pre` (the other fields are not read).  RSP_ERR_INVALID:
 * refCells_R < 1, saveCells_R < 0, CFARmethod_R not 0 or 1, MTD_0v_num < 0, T_CFAR not finite or
 * <= 0, a non-empty segment shorter than 2 (s + r) (the reference indexes out of range there),
 * s + r beyond max_halo.  `info` may be NULL.  No HIP call is made. */
int32_t rsp_stage3_describe(const rsp_sig_config* cfg, const rsp_precomputed* pre,
                            const rsp_stage3_cfar_params* params, rsp_stage3_info* info);

/* local_execute_cfar on host maps: amp is real double [P x G x n_maps] column-major with the
 * plan's P and gate counts; flags (uint8) and threshold (double) have the same shape.  Any output
 * may be NULL.  *n_hits = flagged cells of all maps; min(*n_hits, hits_cap) entries of `hits` are
 * written, the first ones in order.  Synchronous; drains the queue first.  Refusals come before
 * any device work. */
int32_t rsp_stage3_cfar(rsp_plan* plan, const double* amp, int32_t n_maps, const rsp_stage3_cfar_params* params,
                        uint8_t* flags, double* threshold, rsp_stage3_hit* hits, int64_t hits_cap, int64_t* n_hits);
/* The same for maps of another shape: P rows and segments of gates[0], gates[1], gates[2] columns
 * (local_execute_cfar takes any map; odd P included).  The plan gives the device and the precision. */
int32_t rsp_stage3_cfar_shape(rsp_plan* plan, int32_t P, const int32_t* gates, const double* amp, int32_t n_maps,
                              const rsp_stage3_cfar_params* params, uint8_t* flags, double* threshold,
                              rsp_stage3_hit* hits, int64_t hits_cap, int64_t* n_hits);
/* rsp_process_stage2, then the CFAR on |MTD_results| of all B beams without leaving the device
 * (the magnitude routine of k2_pc's maps).  mtd_out complex [P x G x B]; amp_out (the map that
 * was tested), flags, threshold [P x G x B]; hits as above with beam_idx = the beam.  Every output
 * is optional: a call that asks for the hit list alone downloads nothing else. */
int32_t rsp_process_stage2_cfar(rsp_plan* plan, const void* iq_beams, int32_t dtype,
                                const rsp_stage3_cfar_params* params, double* mtd_out, double* amp_out,
                                uint8_t* flags, double* threshold, rsp_stage3_hit* hits, int64_t hits_cap,
                                int64_t* n_hits);
/* The same on a gated input (iq_gated, n_gated, cols as rsp_process_stage2_gated). */
int32_t rsp_process_stage2_gated_cfar(rsp_plan* plan, const void* iq_gated, int32_t dtype, int32_t n_gated,
                                      const int32_t* cols, const rsp_stage3_cfar_params* params, double* mtd_out,
                                      double* amp_out, uint8_t* flags, double* threshold, rsp_stage3_hit* hits,
                                      int64_t hits_cap, int64_t* n_hits);
/* Device time of k_s3_cfar over the plan's B beams of [P x G], by HIP events on the plan's stream,
 * averaged over `iters` launches each: ms_out[0] the real-amplitude form writing flags and
 * thresholds (rsp_stage3_cfar's launch), [1] the complex form writing amplitudes, flags and
 * thresholds, [2] the complex form with the hit list alone.  bytes_out[i] = algorithmic HBM bytes
 * of launch i (the hit records not counted).  The maps are the MTD result of the plan's last
 * stage-2 call and its magnitudes (RSP_ERR_INVALID when there has been none). */
int32_t rsp_profile_stage3(rsp_plan* plan, const rsp_stage3_cfar_params* params, int32_t iters, float* ms_out,
                           int64_t* bytes_out);

/* ---- Doppler cell-averaging CFAR of the stage-2 path ----
 * local_cfar_detector of main_simulate_echoes_with_array_v3.m:278-314, called at :249-250 on
 * abs(mtd_results) of one beam: the only CFAR of the reference that slides along the velocity
 * axis.  Per real amplitude map A [P x G] (P Doppler rows, 1-based row v, every range column on
 * its own), r = refCells_V >= 1, g = guardCells_V >= 0 and even, h = g / 2:
 *   gs = max(1, v - h);  lead  = rows max(1, gs - r) .. gs - 1          (empty when gs = 1)
 *   ge = min(P, v + h);  trail = rows ge + 1 .. min(P, ge + r)          (empty when ge = P)
 *   (:289-297; where the map ends the window is clipped, not replaced by the opposite one);
 *   method 0 (CA, the reference, :299-306): noise = sum / n, sum = one running sum over the lead
 *     rows in ascending order and then the trail rows in ascending order, starting from the first
 *     cell that exists, n = the number of cells; n = 0: noise = 0;
 *   method 1 (GOCA), 2 (SOCA): the two other values the script's `method` comment names (:35); the
 *     reference's function ignores the field, so they are defined here: mL = sum(lead) / nL,
 *     mT = sum(trail) / nT, each summed ascending with one division; noise = max(mL, mT) (GOCA) or
 *     min (SOCA); one side empty: the other; both empty: noise = 0;
 *   threshold = noise * T_CFAR; flag = A > threshold (strict, :309).  A cell with no reference
 *     cells has threshold 0 and is flagged exactly when A > 0.
 * No notch and no segments: the whole map is one piece.  Every operation is one correctly rounded
 * IEEE operation in the plan's precision, in the order above (double for RSP_C128, float for
 * RSP_C64; T_CFAR, the amplitudes and the count are rounded to it first), so the result is defined
 * to the bit; thresholds and amplitudes leave the device widened to double.  There are no
 * sliding-sum updates.  An odd guardCells_V makes the reference index with a non-integer and is
 * refused. */
typedef struct rsp_vcfar_params {
    int32_t refCells_V, guardCells_V, method, reserved;
    double T_CFAR;
} rsp_vcfar_params;

/* What the detector does with a map of P rows and G columns (rsp_vcfar_describe). */
typedef struct rsp_vcfar_info {
    int32_t P, G;
    int32_t halo;             /* r + h: rows a window reaches above and below its cell            */
    int32_t max_halo;         /* the largest r + h the kernel's tile holds                         */
    int32_t rows, cols;       /* Doppler rows and range columns one workgroup of k_vcfar resolves  */
    int32_t row_tiles, col_tiles;   /* workgroups per map along either axis                        */
} rsp_vcfar_info;

/* The checks of the calls below, with the same refusals and messages, and the tiling they use.
 * RSP_ERR_INVALID: refCells_V < 1, guardCells_V < 0 or odd, method not 0, 1 or 2, T_CFAR not
 * finite or <= 0, r + h beyond max_halo, P < 1 or G < 1.  `info` may be NULL.  No HIP call is made. */
int32_t rsp_vcfar_describe(int32_t P, int32_t G, const rsp_vcfar_params* params, rsp_vcfar_info* info);

/* local_cfar_detector on host maps of any shape: amp is real double [P x G x n_maps] column-major;
 * flags (uint8) and threshold (double) have the same shape.  The plan gives only the device and
 * the precision.  Any output may be NULL.  Hits are rsp_stage3_hit records ordered by map, then as
 * find() on [P x G]; *n_hits = flagged cells of all maps, min(*n_hits, hits_cap) entries of `hits`
 * are written, the first ones in order.  Synchronous; drains the queue first.  Refusals come
 * before any device work. */
int32_t rsp_vcfar(rsp_plan* plan, int32_t P, int32_t G, const double* amp, int32_t n_maps, const rsp_vcfar_params* params,
                  uint8_t* flags, double* threshold, rsp_stage3_hit* hits, int64_t hits_cap, int64_t* n_hits);
/* rsp_process_stage2, then the detector on |MTD_results| of all B beams without leaving the device
 * (outputs as rsp_process_stage2_cfar's, every one optional). */
int32_t rsp_process_stage2_vcfar(rsp_plan* plan, const void* iq_beams, int32_t dtype, const rsp_vcfar_params* params,
                                 double* mtd_out, double* amp_out, uint8_t* flags, double* threshold,
                                 rsp_stage3_hit* hits, int64_t hits_cap, int64_t* n_hits);
/* The same on a gated input (iq_gated, n_gated, cols as rsp_process_stage2_gated). */
int32_t rsp_process_stage2_gated_vcfar(rsp_plan* plan, const void* iq_gated, int32_t dtype, int32_t n_gated,
                                       const int32_t* cols, const rsp_vcfar_params* params, double* mtd_out,
                                       double* amp_out, uint8_t* flags, double* threshold, rsp_stage3_hit* hits,
                                       int64_t hits_cap, int64_t* n_hits);
/* Device time of k_vcfar over the plan's B beams of [P x G], in the three forms and with the
 * algorithmic bytes of rsp_profile_stage3 (the same maps, the same bytes per form). */
int32_t rsp_profile_vcfar(rsp_plan* plan, const rsp_vcfar_params* params, int32_t iters, float* ms_out,
                          int64_t* bytes_out);

/* ---- stage-1 DBF of the stage-2 path ----
 * Every stage-2 script of the reference beamforms the raw 16-channel frame (raw_iq_data of a
 * frame_sim_array_%d.mat, [prtNum x point_PRT x channel_num]) pulse by pulse before it calls
 * process_stage2_mtd: `single_pulse_16ch * DBF_coeffs_data_C'` (debug_simulated_data_processing.m:
 * 166-175, _v3.m:144-152; conj != 0 here, the form of fsf:95) or `iq_data_temp *
 * DBF_coeffs_data_C.'` (main_test_with_simulated_data.m:207-214, one beam of it in
 * debug_simulated_data_processing_v2.m:176-182; conj = 0).  For every position (p, n):
 *   beams[p, n, b] = sum_c a[b][c] cube[p, n, c],   a = conj(W) (conj != 0) or a = W,
 * W = DBF_coeffs_data_C, column-major B x C, interleaved (re, im) doubles.  The sum runs on the
 * matrix cores in the plan's precision (complex double for RSP_C128, complex single for RSP_C64)
 * exactly as K1's DBF: channels in groups of 4 in ascending order, per group the real parts of x
 * before the imaginary parts, every step a fused multiply-add into the running sum.  Not MATLAB's
 * summation order, so results agree with `x * W'` to rounding, not to the bit. */

/* How k_dbf covers a plane of P N positions (rsp_dbf_describe). */
typedef struct rsp_dbf_info {
    int32_t positions;        /* S = P N                                                          */
    int32_t CP, BMAX;         /* channels and beams rounded up to what the MFMA tiles hold (K1's)  */
    int32_t sub_tile;         /* positions per MFMA sub-tile: 16 (complex double), 32 (single)     */
    int32_t tiles_per_wave;   /* sub-tiles whose loads a wave keeps in flight together             */
    int32_t waves, rounds;    /* waves per workgroup; rounds of tiles_per_wave sub-tiles per wave  */
    int32_t wg_positions;     /* waves x rounds x tiles_per_wave x sub_tile                        */
    int32_t workgroups;       /* ceil(S / wg_positions)                                            */
    int32_t tail_positions;   /* S mod sub_tile: positions of the last, partly filled sub-tile     */
    int32_t row_layout;       /* RSP_DBF_ROWS_* of the A table the kernel reads                    */
    int32_t pitch;            /* elements between the planes of rsp_dbf's device buffers           */
} rsp_dbf_info;
#define RSP_DBF_ROWS_SPLIT 0   /* MFMA row m of an 8-beam block: beam m & 7, part m >> 3 (0 Re, 1 Im) */
#define RSP_DBF_ROWS_PAIR 1    /* beam m >> 1, part m & 1                                              */

/* The size checks of rsp_dbf, with the same refusals and messages, and the kernel's tiling, for a
 * plan of `precision` (RSP_C128 / RSP_C64).  RSP_ERR_INVALID: P < 1, N < 1, C outside 1..32, B
 * outside 1..16, unknown precision; RSP_ERR_UNSUPPORTED: 2 GB or more of input or output planes.
 * `info` may be NULL.  No HIP call is made. */
int32_t rsp_dbf_describe(int32_t P, int32_t N, int32_t C, int32_t B, int32_t precision, rsp_dbf_info* info);
/* The matrix-core A operands of the DBF for weights W (column-major B x C): [MB][CP/4][2][64]
 * doubles, MB = 1 (B <= 8) or 2; entry [mb][j][e][lane] is the coefficient of Re x_c (e = 0) or
 * Im x_c (e = 1), c = 4 j + lane / 16, in MFMA row lane % 16 of block mb -- which (beam, part)
 * that row is, row_layout says.  *n = the table's length; its first min(cap, *n) entries go to out.
 * No HIP call is made. */
int32_t rsp_dbf_table(const double* W, int32_t B, int32_t C, int32_t conj, int32_t row_layout, double* out, int32_t cap,
                      int32_t* n);
/* The table a plan of these arguments uploads for K1 (conj(W), RSP_DBF_ROWS_SPLIT), without a device. */
int32_t rsp_plan_describe_dbf_table(const rsp_sig_config* cfg, const rsp_cfar_params* cfar,
                                    const rsp_cluster_params* cluster, const rsp_precomputed* pre,
                                    const rsp_plan_options* opt, int32_t ncu, double* out, int32_t cap, int32_t* n);

/* The DBF of a raw cube of any shape: cube [P x N x C] (dtype RSP_C64 / RSP_C128, converted to the
 * plan's precision as rsp_process_cube does) -> beams_out complex double [P x N x B].  Any P, N >= 1
 * (odd too), 1 <= C <= 32, 1 <= B <= 16.  The plan gives only the device and the precision.
 * Synchronous; drains the queue first.  Refusals (sizes, dtype, null pointers, in that order) come
 * before any device work. */
int32_t rsp_dbf(rsp_plan* plan, int32_t P, int32_t N, int32_t C, int32_t B, const void* cube, int32_t dtype,
                const double* W, int32_t conj, double* beams_out);

/* The stage-2 calls on the raw cube: the scripts' DBF loop and process_stage2_mtd in one call.
 * cube is [P x n x C] with the plan's P and C.  n_gated = 0 (cols ignored): n is the plan's
 * point_PRT; otherwise cube holds n_gated gated columns per channel, put back at their PRT
 * positions as rsp_process_stage2_gated does with beams (cols NULL: the reference gating).
 * W: column-major B x C as above, NULL = the plan's DBF_coeffs_data_C; conj as rsp_dbf.  The DBF
 * runs inside the corner turn (K1 with its DBF stage and without the MTD), so the beams never
 * reach device memory in PRT order; the pulse compression, the MTD over pulses and the detectors
 * are those of the beams forms, and so are the outputs.  The result equals the beams form fed with
 * rsp_dbf's beams to the bit.  The A operands of a call are uploaded only when W or conj differ
 * from the previous raw call's. */
int32_t rsp_process_raw_stage2(rsp_plan* plan, const void* cube, int32_t dtype, int32_t n_gated, const int32_t* cols,
                               const double* W, int32_t conj, double* mtd_out, double* pc_out);
int32_t rsp_process_raw_stage2_cfar(rsp_plan* plan, const void* cube, int32_t dtype, int32_t n_gated, const int32_t* cols,
                                    const double* W, int32_t conj, const rsp_stage3_cfar_params* params, double* mtd_out,
                                    double* amp_out, uint8_t* flags, double* threshold, rsp_stage3_hit* hits,
                                    int64_t hits_cap, int64_t* n_hits);
int32_t rsp_process_raw_stage2_vcfar(rsp_plan* plan, const void* cube, int32_t dtype, int32_t n_gated, const int32_t* cols,
                                     const double* W, int32_t conj, const rsp_vcfar_params* params, double* mtd_out,
                                     double* amp_out, uint8_t* flags, double* threshold, rsp_stage3_hit* hits,
                                     int64_t hits_cap, int64_t* n_hits);
/* Device time of k_dbf alone on a cube of P x N x C (zeros) into B beams, by HIP events on the
 * plan's stream, averaged over `iters` launches; *bytes_out = algorithmic HBM bytes of a launch,
 * element bytes x P N x (C + B). */
int32_t rsp_profile_dbf(rsp_plan* plan, int32_t P, int32_t N, int32_t C, int32_t B, int32_t iters, float* ms_out,
                        int64_t* bytes_out);

/* ---- the MTD as a stand-alone stage: a slow-time transform of any length ----
 * `fftshift(fft(pc .* MTD_win, nfft, 1), 1)` (main_simulate_echoes_with_array_v7_7.m:501-503 with
 * FFTnum_MTD = 512 on 332 pulses; fun_process_single_frame.m:131-135 with nfft = prtNum) on a cube in
 * MATLAB's own layout.  For every column (g, map) of pc [P x G x n_maps], pulse index fastest:
 *   out[:, g, map] = shift( DFT_nfft( [pc[:, g, map] .* win ; zeros(nfft - P)] ) ),
 * shift = MATLAB's fftshift (output row v holds frequency (v - floor(nfft / 2)) mod nfft, odd nfft
 * included) or, shift = 0, natural order.  out is [nfft x G x n_maps].  Any 1 <= P <= nfft <=
 * RSP_MTD_MAX_NFFT, G, n_maps >= 1; nfft = 0 means P.  The work is O(nfft log nfft) per column at
 * every length: Stockham passes in LDS for nfft = 2^m, Bluestein's chirp-z transform over the least
 * power of two M >= 2 nfft - 1 for every other length. */
#define RSP_MTD_MAX_NFFT 2048
#define RSP_MTD_ROUTE_POW2 0     /* nfft = 2^m: zero fill, 2^m-point Stockham passes            */
#define RSP_MTD_ROUTE_CHIRPZ 1   /* chirp, M-point FFT, filter spectrum, inverse FFT, chirp     */
#define RSP_MTD_ROUTE_DIRECT 2   /* reserved: no length takes it                                */

/* How k_mtd_any covers a cube (rsp_mtd_describe). */
typedef struct rsp_mtd_info {
    int32_t P, G, nfft;      /* nfft as resolved (0 on input = P)                         */
    int32_t route;           /* RSP_MTD_ROUTE_*                                           */
    int32_t M;               /* points of the LDS transform: nfft (POW2), chirp-z M, 0    */
    int32_t cols;            /* columns one workgroup transforms                          */
    int32_t col_tiles;       /* workgroups per map                                        */
    int32_t lds_bytes;       /* dynamic LDS of a workgroup                                */
    int32_t table_elems;     /* complex entries of rsp_mtd_table: nfft + M, 0 if none     */
} rsp_mtd_info;
/* The size checks of rsp_mtd for one map, with the same refusals and messages, and the kernel's
 * route and tiling, for a plan of `precision`.  RSP_ERR_INVALID: unknown precision, P < 1, G < 1,
 * nfft < P (nfft = 0: P); RSP_ERR_UNSUPPORTED: nfft > RSP_MTD_MAX_NFFT, 2 GB or more of input or
 * output.  `info` may be NULL.  No HIP call is made. */
int32_t rsp_mtd_describe(int32_t P, int32_t G, int32_t nfft, int32_t precision, rsp_mtd_info* info);
/* The chirp-z tables of length nfft as the kernel reads them: w[0 .. nfft) = exp(-i pi (m^2 mod
 * 2 nfft) / nfft), then Bf[0 .. M), the M-point DFT of conj(w) wrapped round M (entry j and entry
 * M - j hold conj(w[j]), j < nfft) with 1 / M folded in -- interleaved (re, im) doubles that hold the
 * values rounded once to `precision` from a long double evaluation.  A power-of-two nfft has no
 * tables: *n = 0.  *n = the complex entries; the first min(cap, *n) go to out.  No HIP call is made. */
int32_t rsp_mtd_table(int32_t nfft, int32_t precision, double* out, int32_t cap, int32_t* n);
/* pc [P x G x n_maps] (dtype RSP_C64 / RSP_C128, converted to the plan's precision as rsp_process_cube
 * converts) -> out, complex double [nfft x G x n_maps].  win: P reals, NULL = none.  The plan gives
 * only the device, the stream and the precision; its tables of a length are built and uploaded once.
 * Synchronous; drains the queue first.  Refusals (sizes, dtype, null pointers, in that order) come
 * before any device work. */
int32_t rsp_mtd(rsp_plan* plan, int32_t P, int32_t G, int32_t n_maps, int32_t nfft, const void* pc, int32_t dtype,
                const double* win, int32_t shift, double* out);
/* The same on device memory in the plan's precision: d_pc [P x G x n_maps] -> d_out [nfft x G x
 * n_maps], which must not overlap and are aligned to a complex element of the precision.  Nothing outside
 * those nfft G n_maps elements is written. */
int32_t rsp_mtd_device(rsp_plan* plan, int32_t P, int32_t G, int32_t n_maps, int32_t nfft, const void* d_pc,
                       const double* win, int32_t shift, void* d_out);
/* Device time of k_mtd_any alone on a cube of zeros, by HIP events on the plan's stream, averaged
 * over `iters` launches; *bytes_out = element bytes x G n_maps (P + nfft). */
int32_t rsp_profile_mtd(rsp_plan* plan, int32_t P, int32_t G, int32_t n_maps, int32_t nfft, int32_t iters,
                        float* ms_out, int64_t* bytes_out);

/* ---- cross GOCA-CFAR as a map detector ----
 * fun_run_goca_cfar_8 (fun_process_single_frame.m:172-223) on any real amplitude map: the only CFAR
 * of the reference that tests along range and Doppler together, and the test K3 applies to the
 * frame chain's pair sums.  Here it returns a dense flag map and the threshold every cell was
 * tested against, like the two one-axis detectors above.  Per map A [P x G] (P Doppler rows,
 * 1-based row v; G range columns, 1-based column r) and rsp_cfar_params with
 *   rR = refCells_R >= 1, gR = guardCells_R >= 0, rV = refCells_V >= 1, gV = guardCells_V >= 0,
 *   T_CFAR finite and > 0, hR = rR + gR, hV = rV + gV:
 * the cells under test are r = hR + 1 .. G - hR, v = hV + 1 .. P - hV (:192-193).  For each:
 *   lr = A(v, r - hR) + .. + A(v, r - gR - 1)      tr = A(v, r + gR + 1) + .. + A(v, r + hR)
 *   lv = A(v - hV, r) + .. + A(v - gV - 1, r)      tv = A(v + gV + 1, r) + .. + A(v + hV, r)
 *   each sum one rounded add per cell in ascending index order starting from +0 (k3_map_sums); no
 *   sliding-sum updates;
 *   complex-double plans: nR = RN(max(lr, tr) / rR), nV = RN(max(lv, tv) / rV), the correctly
 *     rounded quotients (k3_quot's FMA form gives exactly that wherever the quotient is a normal
 *     number or +Inf: "Value domain" above);
 *   complex-single plans: nR = RN(max(lr, tr) RN(1 / rR)), nV likewise: K3's float form, part of the
 *     definition and not an approximation of the double one;
 *   noise = max(nR, nV); threshold = RN(T_CFAR noise); flag = A > threshold (strict, :209).
 * T_CFAR and the amplitudes are rounded to the plan's precision first; thresholds and amplitudes
 * leave the device widened to double.  Every other cell is never tested by the reference: its flag
 * is 0 and its threshold +Inf (a threshold of 0 would read as "everything detects").  A map with
 * no cell under test (G <= 2 hR or P <= 2 hV) gives all flags 0, all thresholds +Inf and no hits,
 * whatever the halos.  The arithmetic is k3_cfar's (rsp_k3_arith.h), so on the pair-sum maps of a
 * frame the flagged cells are the frame's detections. */

/* What the detector does with a map of P rows and G columns (rsp_xcfar_describe). */
typedef struct rsp_xcfar_info {
    int32_t P, G;
    int32_t hR, hV;           /* rR + gR, rV + gV: cells a window reaches along range / Doppler      */
    int32_t max_hR, max_hV;   /* the largest halos the kernel's tile holds                           */
    int32_t rows, cols;       /* Doppler rows and range columns one workgroup of k_xcfar resolves     */
    int32_t row_tiles, col_tiles;   /* workgroups per map along either axis                          */
    int32_t r0, r1, v0, v1;   /* 1-based cells under test r0..r1 x v0..v1; r0 > r1 and v0 > v1: none */
} rsp_xcfar_info;

/* The checks of the calls below, with the same refusals and messages, and the tiling they use.
 * RSP_ERR_INVALID: refCells_R or refCells_V < 1, a negative guard, T_CFAR not finite or <= 0, P < 1
 * or G < 1, hR beyond max_hR or hV beyond max_hV while the map has cells under test.  `info` may
 * be NULL.  No HIP call is made. */
int32_t rsp_xcfar_describe(int32_t P, int32_t G, const rsp_cfar_params* params, rsp_xcfar_info* info);

/* The detector on host maps of any shape, with the conventions of rsp_vcfar: amp real double
 * [P x G x n_maps] column-major, flags (uint8) and threshold (double) of the same shape, hits
 * ordered by map, then as find() on [P x G], beam_idx = the map; every output optional.
 * Synchronous; drains the queue first.  Refusals come before any device work. */
int32_t rsp_xcfar(rsp_plan* plan, int32_t P, int32_t G, const double* amp, int32_t n_maps, const rsp_cfar_params* params,
                  uint8_t* flags, double* threshold, rsp_stage3_hit* hits, int64_t hits_cap, int64_t* n_hits);
/* rsp_process_stage2 (or its gated / raw-cube form), then the detector on |MTD_results| of all B
 * beams without leaving the device (arguments and outputs as the _vcfar forms, every output optional). */
int32_t rsp_process_stage2_xcfar(rsp_plan* plan, const void* iq_beams, int32_t dtype, const rsp_cfar_params* params,
                                 double* mtd_out, double* amp_out, uint8_t* flags, double* threshold,
                                 rsp_stage3_hit* hits, int64_t hits_cap, int64_t* n_hits);
int32_t rsp_process_stage2_gated_xcfar(rsp_plan* plan, const void* iq_gated, int32_t dtype, int32_t n_gated,
                                       const int32_t* cols, const rsp_cfar_params* params, double* mtd_out,
                                       double* amp_out, uint8_t* flags, double* threshold, rsp_stage3_hit* hits,
                                       int64_t hits_cap, int64_t* n_hits);
int32_t rsp_process_raw_stage2_xcfar(rsp_plan* plan, const void* cube, int32_t dtype, int32_t n_gated, const int32_t* cols,
                                     const double* W, int32_t conj, const rsp_cfar_params* params, double* mtd_out,
                                     double* amp_out, uint8_t* flags, double* threshold, rsp_stage3_hit* hits,
                                     int64_t hits_cap, int64_t* n_hits);
/* The detector with the plan's own cfar_params on the pair-sum maps of the plan's last synchronous
 * frame that asked for rsp_frame_out.cfar_maps: the maps K3 thresholded, [P x G x (B - 1)], still
 * on the device.  flags / threshold [P x G x (B - 1)], beam_idx of a hit = the pair; every output
 * optional.  RSP_ERR_INVALID when the plan's last synchronous frame did not ask for the maps (or
 * there has been none), or when the plan has one beam. */
int32_t rsp_last_cfar_threshold(rsp_plan* plan, uint8_t* flags, double* threshold, rsp_stage3_hit* hits, int64_t hits_cap,
                                int64_t* n_hits);
/* Device time of k_xcfar over the plan's B beams of [P x G], in the three forms and with the
 * algorithmic bytes of rsp_profile_stage3 (the same maps, the same bytes per form). */
int32_t rsp_profile_xcfar(rsp_plan* plan, const rsp_cfar_params* params, int32_t iters, float* ms_out,
                          int64_t* bytes_out);

/* ---- detection on any range-Doppler cube ----
 * fun_run_goca_cfar_8 + fun_parameter_estimation_9 + fun_cluster_stage1_10 + fun_cluster_stage2_11
 * (fun_process_single_frame.m:172-407) as a call of their own on a complex RD cube x [V x G x B] of any
 * shape (V Doppler rows, 1-based row v; G range cells, 1-based r; B >= 2 beams) with the caller's axes:
 * the back end main_simulate_echoes_with_array_v7_7.m runs on its zero-padded 512-row cube (:509-...).
 *   1. pair sums (fsf:184-187): S(v, r, pair) = RN(|x(v, r, pair)| + |x(v, r, pair + 1)|), pair = 1 .. B - 1,
 *      magnitudes by the library's one routine (k2_pc's), one rounded add, in the plan's precision
 *      (k_pairsum): K3's bits on K3's maps;
 *   2. the cross GOCA-CFAR of the section above on every S(:, :, pair) with params->cfar (fsf:192-221;
 *      k_xcfar itself);
 *   3. S9 of every hit (fsf:237-297; k_s9, K3's arithmetic): the 5-cell windows r - 2 .. r + 2 and
 *      v - 2 .. v + 2 clipped to the map, the not-a-knot spline sampled at 1/8 (range) and 1/4 (velocity)
 *      cell, first maximum; Range = range_axis(r) + (rCellMax - r) deltaR, Velocity = velocity_axis(v) +
 *      (vCellMax - v) deltaV (fsf:262, :278), Angle = (beam_angles_deg(pair) + beam_angles_deg(pair + 1)) / 2
 *      + k_slopes_LUT(pair) ratio, ratio = (S_A - S_B) / (S_A + S_B + eps) of the two magnitudes at the
 *      integer cell (fsf:282-290), or with monopulse = 1 real((x_A - x_B) / (x_A + x_B + eps)) of the complex
 *      values, as RSP_PLAN_MONOPULSE_COMPLEX.  main_simulate_echoes_with_array_v7_7.m:677's variant
 *      velocity_axis(fix(vCellMax)) is not built;
 *   4. the detections in the reference's order (pair, then r, then v) and S10 / S11 on the host
 *      (fsf:302-407; rsp_cluster_detections' code) with params->cluster.
 * The plan gives only the device, the stream and the precision (rsp_process_stage2_detect excepted). */
typedef struct rsp_detect_params {
    rsp_cfar_params cfar;
    rsp_cluster_params cluster;
    const double* range_axis;      /* G                                                                */
    const double* velocity_axis;   /* V                                                                */
    double deltaR, deltaV;
    const double* beam_angles_deg; /* B                                                                */
    const double* k_slopes_LUT;    /* B - 1                                                            */
    int32_t monopulse;             /* 0: amplitude ratio (fsf:282-290); 1: complex ratio, as
                                      RSP_PLAN_MONOPULSE_COMPLEX                                       */
    int32_t reserved;
} rsp_detect_params;

/* What the detector does with a cube of V x G x B (rsp_detect_describe). */
typedef struct rsp_detect_info {
    int32_t V, G, B;
    int32_t n_pairs;                 /* B - 1 pair-sum maps of V x G                                    */
    int32_t rows, cols;              /* Doppler rows and range cells of k_pairsum's tile (cube in MATLAB's
                                        layout: the tile is transposed through LDS)                    */
    int32_t row_tiles, col_tiles;    /* workgroups along either axis; each walks all B beams           */
    int32_t lds_bytes;               /* LDS of a workgroup, padding included                           */
    int32_t r0, r1, v0, v1;          /* 1-based cells under test r0..r1 x v0..v1; r0 > r1, v0 > v1: none */
    int32_t reserved;
    int64_t cells_under_test;        /* per pair-sum map                                               */
    int64_t max_detections;          /* (B - 1) x cells_under_test                                     */
} rsp_detect_info;

/* The size checks of the calls below, with the same refusals and messages, for a plan of `precision`
 * (RSP_C128 / RSP_C64).  RSP_ERR_INVALID: unknown precision, B < 2, V < 1, G < 1, every refusal of
 * rsp_xcfar_describe for a V x G map with its message; RSP_ERR_UNSUPPORTED: 2 GB or more of cube or of
 * pair-sum maps.  `info` may be NULL.  No HIP call is made. */
int32_t rsp_detect_describe(int32_t V, int32_t G, int32_t B, int32_t precision, const rsp_cfar_params* params,
                            rsp_detect_info* info);
/* The detector on a host cube rdm [V x G x B] in MATLAB's layout (Doppler index fastest; dtype RSP_C64 /
 * RSP_C128, converted to the plan's precision as rsp_process_cube converts).  out->cfar_maps (optional) is
 * S, [V x G x (B - 1)]; out->dets / targets, their caps and counts behave as in rsp_process_cube, overflow
 * rule included (every detection and target: rsp_last_detections / rsp_last_targets); out->rdm must be NULL
 * (RSP_ERR_INVALID otherwise: the cube is the caller's).  Synchronous; drains the queue first.  Refusals
 * (sizes, dtype, null pointers, in that order) come before any device work. */
int32_t rsp_detect(rsp_plan* plan, int32_t V, int32_t G, int32_t B, const void* rdm, int32_t dtype,
                   const rsp_detect_params* params, rsp_frame_out* out);
/* The same on a device cube in the plan's precision and MATLAB's layout (rsp_mtd_device's output), aligned
 * to a complex element.  The cube is only read. */
int32_t rsp_detect_device(rsp_plan* plan, int32_t V, int32_t G, int32_t B, const void* d_rdm,
                          const rsp_detect_params* params, rsp_frame_out* out);
/* v7_7 sections 7-10: rsp_mtd (shift = 1) of pc [P x G x B] to nfft rows into a device cube, and the
 * detector on that cube in place (V = nfft; velocity_axis has nfft entries).  out->rdm (optional) is the
 * cube, complex double [nfft x G x B]; nothing but the requested outputs crosses to the host. */
int32_t rsp_mtd_detect(rsp_plan* plan, int32_t P, int32_t G, int32_t B, int32_t nfft, const void* pc, int32_t dtype,
                       const double* win, const rsp_detect_params* params, rsp_frame_out* out);
/* rsp_process_stage2, then the detector on MTD_results without leaving the device, with the plan's own
 * cfar_params, cluster_params, axes, angles, K-LUT and monopulse option, at nfft = P (the device's
 * range-contiguous layout [B][P][G], read in place).  out->rdm (optional) is MTD_results [P x G x B]. */
int32_t rsp_process_stage2_detect(rsp_plan* plan, const void* iq_beams, int32_t dtype, rsp_frame_out* out);
/* Device times of the three stages on a deterministic test cube of V x G x B (uniform noise in the unit
 * square, a peak of amplitude 100 in every beam at each 37th row and 101st range cell), by HIP events
 * on the plan's stream, averaged over `iters` launches: ms_out[0] k_pairsum (MATLAB layout), [1] k_xcfar
 * (hits only), [2] k_s9.  bytes_out[0] = cube + maps, [1] = maps, [2] = 48 x the cube's hits. */
int32_t rsp_profile_detect(rsp_plan* plan, int32_t V, int32_t G, int32_t B, const rsp_cfar_params* params, int32_t iters,
                           float* ms_out, int64_t* bytes_out);

/* ---- pulse compression as a stand-alone stage: any pulse count, any beam count ----
 * Section 6 of main_simulate_echoes_with_array_v7_7.m (:362-486; fun_process_single_frame.m:99-127): the
 * three-segment pulse compression of every (pulse, beam) row of a beam cube iq_beams [P x N x B] in MATLAB's
 * layout (pulse index fastest) into pc [P x G x B].  A row's arithmetic is k2_pc's, the kernel of
 * rsp_process_stage2, and depends on that row's samples alone; what is new is the way in and out of it:
 *   k_pc_pack    beams -> k2_pc's compacted sample rows (z) for the caller's P and B, no window, no transform;
 *   k2_pc        on a record table built for B P rows, with the plan's segments, taps, spectra and twiddles;
 *   k_pc_unpack  k2_pc's [B][P][G] result -> pc [P x G x B].
 * The plan gives the device, the stream, the precision, N = point_PRT, the gate layout and the filter
 * tables; its own prtNum and beam_num play no part, so P may be odd, prime or 1. */
typedef struct rsp_pc_info {
    int32_t P, B, N, G;
    int32_t nU, n_intervals;             /* used fast-time samples, and the intervals they form            */
    int32_t NZ, nzc;                     /* z: NZ compacted samples per (row, chunk) slab, nzc chunks       */
    int64_t z_elems;                     /* B nzc P NZ complex elements                                    */
    int32_t pack_rows, pack_cols;        /* k_pc_pack's tile: NZ samples x pulses                          */
    int32_t unpack_rows, unpack_cols;    /* k_pc_unpack's tile: pulses x gates; a workgroup walks up to 8
                                            such tiles along the pulse axis                                */
    int32_t pack_wg, k2_wg, unpack_wg;   /* workgroups of the three launches                               */
    int32_t k2_wg_per_cu;                /* the k2_pc instantiation (rsp_k2_layout.wg_per_cu)              */
    int32_t pack_lds_bytes, unpack_lds_bytes;   /* LDS of a workgroup, padding included                    */
    /* interval q < n_intervals: compacted samples ivl_start[q] .. are fast-time samples ivl_lo[q] .. (0-based) */
    int32_t ivl_lo[4], ivl_start[4];
} rsp_pc_info;
/* The size checks of the calls below, with the same refusals and messages, and how the three launches cover
 * P pulses of B beams.  RSP_ERR_INVALID: P < 1 or B < 1; RSP_ERR_UNSUPPORTED: 2 GB or more of beams, of z or
 * of result (the kernels address each with 32-bit byte offsets).  `info` may be NULL. */
int32_t rsp_query_pc(const rsp_plan* plan, int32_t P, int32_t B, rsp_pc_info* info);
/* The same from the arguments of rsp_plan_create_ex, whose prtNum and beam_num are not read (a
 * configuration that a plan refuses for its prtNum alone is accepted).  No HIP call is made. */
int32_t rsp_plan_describe_pc(const rsp_sig_config* cfg, const rsp_cfar_params* cfar, const rsp_cluster_params* cluster,
                             const rsp_precomputed* pre, const rsp_plan_options* opt, int32_t ncu, int32_t P, int32_t B,
                             rsp_pc_info* info);
/* iq_beams [P x N x B] (dtype RSP_C64 / RSP_C128, converted to the plan's precision as rsp_process_cube
 * converts) -> pc_out, complex double [P x G x B].  Synchronous; drains the queue first.  Refusals (sizes,
 * dtype, null pointers, in that order) come before any device work.  Scratch buffers are the plan's, grow on
 * demand and are kept; the record table is rebuilt only when (P, B) changes. */
int32_t rsp_pc(rsp_plan* plan, int32_t P, int32_t B, const void* iq_beams, int32_t dtype, double* pc_out);
/* The same on device memory in the plan's precision, MATLAB's layout on both sides: d_beams [P x N x B] ->
 * d_pc [P x G x B] (what rsp_mtd_device reads), which must not overlap and are aligned to a complex element.
 * Nothing outside those P G B elements is written. */
int32_t rsp_pc_device(rsp_plan* plan, int32_t P, int32_t B, const void* d_beams, void* d_pc);
/* v7_7 sections 6-10: rsp_pc_device, rsp_mtd_device (shift = 1, nfft rows; 0 = P) and rsp_detect_device on
 * the plan's scratch; the arguments and outputs are rsp_mtd_detect's, out->rdm the [nfft x G x B] cube. */
int32_t rsp_pc_mtd_detect(rsp_plan* plan, int32_t P, int32_t B, int32_t nfft, const void* iq_beams, int32_t dtype,
                          const double* win, const rsp_detect_params* params, rsp_frame_out* out);
/* v7_7 sections 5-10 from the raw cube [P x N x C]: k_dbf first, with rsp_dbf's W (B x C) and conj; W = NULL
 * takes the plan's own weights, whose shape B x C must then be the plan's. */
int32_t rsp_raw_detect(rsp_plan* plan, int32_t P, int32_t C, int32_t B, int32_t nfft, const void* cube, int32_t dtype,
                       const double* W, int32_t conj, const double* win, const rsp_detect_params* params,
                       rsp_frame_out* out);
/* Device times by HIP events on the plan's stream, averaged over `iters` launches each, on zeros: ms_out[0]
 * k_pc_pack, [1] the k2_pc launch, [2] k_pc_unpack.  bytes_out[0] = element bytes x (P nU B read + z written),
 * [1] = z + the result + the scratch magnitude map, [2] = 2 x element bytes x P G B. */
int32_t rsp_profile_pc(rsp_plan* plan, int32_t P, int32_t B, int32_t iters, float* ms_out, int64_t* bytes_out);

/* ---- digital down-conversion as a stand-alone stage: NCO mixer, FIR, decimator ----
 * simulation_learn.m:79-102 (xrt = xt .* sin(2*pi*f*t2); firxrt = filter(Num, 1, xrt); downsample(firxrt, 4)):
 * the receiver's front end, from sampled real IF data to the baseband cube every other call here starts from.
 * The plan gives only the device, the stream and the precision.
 *
 * Input x is real, [P x N x C] in MATLAB's layout (pulse index fastest), dtype RSP_R32 or RSP_R64, converted
 * to the plan's precision as rsp_process_cube converts.
 * NCO: a 64-bit phase accumulator.  With uint64 wrap-around phase(n) = w0 + n w; u_n = floor(phase(n) / 2^11)
 * 2^-53 and theta_n = 2 pi u_n; the phase restarts at w0 in every pulse and every channel.
 *   RSP_DDC_NCO_IQ    m[n] = cos theta_n - i sin theta_n
 *   RSP_DDC_NCO_SIN   m[n] = sin theta_n   (the reference's single real mixer, :79)
 * sin and cos are computed in double by the restricted-domain routine of the synthesis (2 pi u, u in [0, 1];
 * rsp_noise_math.h) and rounded once to the plan's precision.
 * Mixer: v[p,n,c] = x[p,n,c] m[n] for 0 <= n < N and 0 elsewhere; each part of v is one product, rounded once.
 * Filter and decimation: taps h[0..L) are real doubles, rounded once to the plan's precision, 1 <= L <=
 * RSP_DDC_MAX_TAPS;
 *   y[p,k,c] = sum_{j=0}^{L-1} h[j] v[p, off + k D - j, c],   k = 0 .. No - 1,  No = ceil((N - off) / D),
 * 1 <= D <= RSP_DDC_MAX_D, 0 <= off < D (MATLAB's downsample phase): filter(h, 1, .) with zero initial state
 * followed by downsample(., D, off).  The sum is a chain of fused multiply-adds in ascending j that starts from
 * 0, separately for the real and the imaginary part; that order is part of the contract and makes the result
 * independent of the kernel's tiling.
 * Output: complex [P x No x C] in the same layout (what rsp_dbf and rsp_raw_detect read); in SIN mode the
 * imaginary part is +0.
 * Out of scope: complex input, a per-pulse phase step, the FFT pulse compression of simulation_learn.m:112-130
 * (rsp_pc is the library's pulse compression). */
#define RSP_DDC_MAX_TAPS 512
#define RSP_DDC_MAX_D 64
#define RSP_DDC_NCO_IQ 0
#define RSP_DDC_NCO_SIN 1
typedef struct rsp_ddc_params {
    uint64_t w, w0;           /* phase step per sample and start phase, in 2^-64 turns (rsp_ddc_phase_word) */
    int32_t mode;             /* RSP_DDC_NCO_*                                                      */
    int32_t D, off;           /* decimation factor and phase                                        */
    int32_t L;                /* taps                                                               */
    const double* h;          /* L taps                                                             */
} rsp_ddc_params;
/* How k_ddc covers a cube (rsp_ddc_describe).  A workgroup takes TP pulses x TK outputs of one channel, threads
 * mapped pulse-fastest and then along k; it stages in_rows = (TK - 1) D + tap_chunk input rows (x as it is read,
 * and the row's NCO value, once) in LDS.  tap_chunk = L wherever the rows of all L taps fit the LDS budget of a
 * workgroup (40 KiB); a longer filter is staged tap_chunk taps at a time, the accumulators kept in registers. */
typedef struct rsp_ddc_info {
    int32_t P, N, C, L, D, off;
    int32_t No;               /* outputs per pulse: ceil((N - off) / D)                    */
    int32_t TP, TK;           /* the tile: TP = least power of two >= min(P, 64) pulses x TK outputs */
    int32_t in_rows;          /* input rows staged at a time: (TK - 1) D + tap_chunk       */
    int32_t k_tiles, p_tiles; /* tiles along k and along pulses                            */
    int32_t workgroups;       /* k_tiles x p_tiles x C                                     */
    int32_t lds_bytes;        /* dynamic LDS of a workgroup: rows, NCO values and the taps */
    int32_t tap_chunk;        /* taps whose rows are staged at a time                      */
    int32_t threads;          /* threads of a workgroup: TP x k lanes, at least one wave   */
    int32_t k_per_thread;     /* outputs a thread accumulates: TK / (k lanes)              */
    int64_t in_bytes, out_bytes;   /* the cube and the result in the plan's precision      */
} rsp_ddc_info;
/* The size checks of the calls below, with the same refusals and messages, and the kernel's tiling, for a plan
 * of `precision` (RSP_C128 / RSP_C64).  RSP_ERR_INVALID: P, N or C < 1, L outside 1..RSP_DDC_MAX_TAPS, D
 * outside 1..RSP_DDC_MAX_D, off outside 0..D-1, unknown precision; RSP_ERR_UNSUPPORTED: 2 GB or more of input
 * or output (the kernel addresses each with 32-bit byte offsets).  `info` may be NULL.  No HIP call is made. */
int32_t rsp_ddc_describe(int32_t P, int32_t N, int32_t C, int32_t L, int32_t D, int32_t off, int32_t precision,
                         rsp_ddc_info* info);
/* *w = round(f0 / fs 2^64) mod 2^64, computed in long double (a negative f0 wraps).  RSP_ERR_INVALID: f0 or fs
 * not finite, fs <= 0, w NULL.  No HIP call is made. */
int32_t rsp_ddc_phase_word(double f0, double fs, uint64_t* w);
/* x [P x N x C] real (dtype RSP_R32 / RSP_R64) -> out, complex double [P x No x C].  Synchronous; drains the
 * queue first.  Refusals (sizes, dtype, null pointers and mode, in that order) come before any device work.
 * Scratch buffers are the plan's, grow on demand and are kept. */
int32_t rsp_ddc(rsp_plan* plan, int32_t P, int32_t N, int32_t C, const void* x, int32_t dtype,
                const rsp_ddc_params* params, double* out);
/* The same on device memory in the plan's precision: d_x [P x N x C] reals -> d_out [P x No x C] complex, which
 * must not overlap and are aligned to a real and a complex element.  Nothing outside those P No C elements is
 * written. */
int32_t rsp_ddc_device(rsp_plan* plan, int32_t P, int32_t N, int32_t C, const void* d_x, const rsp_ddc_params* params,
                       void* d_out);
/* rsp_ddc_device into the plan's scratch and then the device chain of rsp_raw_detect on the result (k_dbf,
 * pulse compression, MTD, detection): the IQ cube never leaves the device.  No must be the plan's point_PRT
 * (RSP_ERR_INVALID otherwise, with the two numbers).  The arguments are rsp_ddc's followed by rsp_raw_detect's;
 * the outputs are rsp_raw_detect's. */
int32_t rsp_ddc_raw_detect(rsp_plan* plan, int32_t P, int32_t N, int32_t C, const void* x, int32_t dtype,
                           const rsp_ddc_params* params, int32_t B, int32_t nfft, const double* W, int32_t conj,
                           const double* win, const rsp_detect_params* dparams, rsp_frame_out* out);
/* Device time of k_ddc alone on a cube of zeros (taps of zero, IQ mode, w = 2^64 / 10), by HIP events on the
 * plan's stream, averaged over `iters` launches; *bytes_out = the input plus the output in the plan's precision. */
int32_t rsp_profile_ddc(rsp_plan* plan, int32_t P, int32_t N, int32_t C, int32_t L, int32_t D, int32_t off,
                        int32_t iters, float* ms_out, int64_t* bytes_out);

/* ---- measurement ----
 * Time each device stage `iters` times on the plan's stream with HIP events.  Each launch
 * batches nf = min(n_cubes, frames_per_launch) frames taken from the device-resident
 * cubes d_cubes[] (plan precision); launch j takes cubes (j nf + f) mod n_cubes, f < nf.  ms_out[i] = average ms per launch of stage i,
 * bytes_out[i] = algorithmic HBM bytes per launch (nf frames), *frames_out = nf.
 * Stage names via rsp_stage_name. */
int32_t rsp_profile_stages(rsp_plan* plan, const void* const* d_cubes, int32_t n_cubes, int32_t iters,
                           float* ms_out, int64_t* bytes_out, int32_t cap, int32_t* frames_out);
/* rsp_profile_stages with K2 writing every frame's complex RD map (d_rdms[f], f < nf, as
 * rsp_enqueue_device_rdm); bytes_out[1] then includes the map.  d_rdms = NULL: rsp_profile_stages.
 * d_rdms must hold nf = min(n_cubes, frames_per_launch) non-null maps (a null one is refused with
 * RSP_ERR_INVALID; the array's length cannot be checked here, so the caller sizes it).  A plan with
 * RSP_PLAN_MONOPULSE_COMPLEX writes the map into its own lane buffer on every launch, so its
 * bytes_out[1] includes the map whether or not d_rdms is given. */
int32_t rsp_profile_stages_rdm(rsp_plan* plan, const void* const* d_cubes, int32_t n_cubes, void* const* d_rdms,
                               int32_t iters, float* ms_out, int64_t* bytes_out, int32_t cap, int32_t* frames_out);
const char* rsp_stage_name(int32_t stage);

/* The box's streaming-copy bandwidth (SURVEY 8(d) "measured stream-copy peak"): a 16-B-per-lane
 * non-temporal copy kernel over two device buffers of `bytes` each, `iters` timed launches;
 * *gbps = 2 * bytes / average launch time (read + write).  Measurement only; no plan needed. */
int32_t rsp_hbm_copy_probe(int32_t device, int64_t bytes, int32_t iters, double* gbps);

/* Live stage timing of the throughput queue (rsp_enqueue_device): with timing on, every batch
 * records HIP events around K1, K2 and K3 on the stream the kernels run on, and harvest adds the
 * elapsed times.  rsp_set_stage_timing resets the sums.  rsp_stage_times: ms_sum[i] = total ms
 * of stage i over *launches batched launches holding *frames frames. */
int32_t rsp_set_stage_timing(rsp_plan* plan, int32_t on);
int32_t rsp_stage_times(const rsp_plan* plan, double* ms_sum, int32_t cap, int64_t* launches, int64_t* frames);

/* Host-only S10 + S11 (fun_cluster_stage1_10 / fun_cluster_stage2_11, fsf:302-407) on a
 * detection list (any order; sorted into the reference's find() order first).  No GPU. */
int32_t rsp_cluster_detections(const rsp_detection* dets, int32_t n, const rsp_cluster_params* cluster,
                               rsp_target* out, int32_t cap, int32_t* n_out);

/* ---- inter-frame track association (host only, no GPU) ----
 * main_simulate_echoes_with_array_v8_3.m:253-352: cumulative_final_log (final_targets of every
 * frame with iFrame and iAntAngle injected, :236-244) -> final_tracks_log.  Points are linked
 * when |dRange| <= Gate_R, |dVelocity| <= Gate_V, |d iAntAngle| <= Gate_Az, |dAngle| <= Gate_El
 * and |d iFrame| <= Max_Frame_Gap (config.inter_frame_cluster, v8_3:57-65); clusters are the
 * reference BFS's (connected components, numbered by first member).  Per cluster: the first
 * max-Power member gives Range / Velocity / Angle / Power, Azimuth is the power-weighted mean
 * of iAntAngle, FirstFrame / LastFrame / NumPoints over the members. */
typedef struct rsp_track_point {
    double Range, Velocity, Angle, Power;   /* one final_targets entry (fsf:393-406)     */
    double iAntAngle;                       /* servo azimuth of its frame (v8_3:238)     */
    int32_t iFrame, reserved;               /* frame index (v8_3:237)                    */
} rsp_track_point;

typedef struct rsp_inter_frame_params {
    double Gate_R, Gate_V, Gate_Az, Gate_El;
    int32_t Max_Frame_Gap, reserved;
} rsp_inter_frame_params;

typedef struct rsp_track {   /* one final_tracks_log entry (v8_3:318-335) */
    double Range, Velocity, Angle, Azimuth, Power;
    int32_t FirstFrame, LastFrame, NumPoints, reserved;
} rsp_track;

int32_t rsp_inter_frame_cluster(const rsp_track_point* log, int32_t n, const rsp_inter_frame_params* gates,
                                rsp_track* out, int32_t cap, int32_t* n_out);

/* Device memory helpers (so hosts without a GPU runtime binding can stage cubes). */
int32_t rsp_device_alloc(rsp_plan* plan, int64_t bytes, void** d_ptr);
int32_t rsp_device_free(rsp_plan* plan, void* d_ptr);
int32_t rsp_device_upload(rsp_plan* plan, void* d_dst, const void* h_src, int64_t bytes);
int32_t rsp_device_download(rsp_plan* plan, void* h_dst, const void* d_src, int64_t bytes);
int32_t rsp_device_sync(rsp_plan* plan);

/* ---- MAT-file frame I/O (host only, no GPU) ----
 * The reference moves frames as `frame_sim_array_%d.mat` written by MATLAB's default
 * `save` (-v7: Level-5 format, zlib-compressed elements):
 * main_simulate_echoes_with_array.m:226-229 (`raw_iq_data`),
 * main_simulate_echoes_with_array_v2.m:256-289 (`raw_iq_data_noise_sample`, `servo_angle`),
 * read back by `load` in debug_simulated_data_processing_v3.m:17-22 and
 * main_test_with_simulated_data.m:195,208,215.  These functions replace that MATLAB
 * `save`/`load` pair for hosts without MATLAB.  Level-5 files of either byte order,
 * compressed or not, are read; v7.3 (HDF5) returns RSP_ERR_UNSUPPORTED. */
#define RSP_MAT_MAXDIMS 8
typedef enum rsp_mat_class {    /* MATLAB mxClassID values */
    RSP_MAT_CHAR = 4, RSP_MAT_DOUBLE = 6, RSP_MAT_SINGLE = 7, RSP_MAT_INT8 = 8, RSP_MAT_UINT8 = 9,
    RSP_MAT_INT16 = 10, RSP_MAT_UINT16 = 11, RSP_MAT_INT32 = 12, RSP_MAT_UINT32 = 13,
    RSP_MAT_INT64 = 14, RSP_MAT_UINT64 = 15
} rsp_mat_class;
typedef enum rsp_mat_out {
    RSP_MAT_OUT_F64 = 1,   /* numeric -> double; complex interleaved (mxGetComplexDoubles) */
    RSP_MAT_OUT_F32 = 2,   /* numeric -> float;  complex interleaved                       */
    RSP_MAT_OUT_CHAR = 3   /* char array -> NUL-terminated UTF-8                           */
} rsp_mat_out;

/* One variable of a MAT file as `whos -file` lists it. */
typedef struct rsp_mat_var {
    char name[64];
    int32_t cls;           /* rsp_mat_class (1 cell, 2 struct, 5 sparse, ... listed, not read) */
    int32_t is_complex;
    int32_t ndims;
    int32_t reserved;
    int64_t dims[RSP_MAT_MAXDIMS];
    int64_t numel;
} rsp_mat_var;

/* A variable to write: column-major data, complex interleaved (re, im); cls is
 * RSP_MAT_DOUBLE (data = double*), RSP_MAT_SINGLE (float*) or RSP_MAT_CHAR (bytes). */
typedef struct rsp_mat_wvar {
    const char* name;
    int32_t cls;
    int32_t is_complex;
    int32_t ndims;
    const int64_t* dims;
    const void* data;
} rsp_mat_wvar;

/* List up to `cap` variables (*n_vars = how many the file holds). */
int32_t rsp_mat_list(const char* path, rsp_mat_var* vars, int32_t cap, int32_t* n_vars);
/* Read variable `name` into `out` (cap = entries of out; a complex value counts 2). */
int32_t rsp_mat_read(const char* path, const char* name, int32_t dtype, void* out, int64_t cap);
/* Write a MAT file (Level 5; compress != 0 -> zlib elements like MATLAB -v7). */
int32_t rsp_mat_write(const char* path, const rsp_mat_wvar* vars, int32_t n, int32_t compress);
/* load(frame_sim_array_%d.mat): the [P x N x C] cube (raw_iq_data_noise_sample, else
 * raw_iq_data) into `cube` as dtype RSP_C64/RSP_C128 (NULL: only dims_out), and
 * servo_angle (may be NULL; *n_angle = its length, 0 if absent).  One pass over the file. */
int32_t rsp_mat_load_frame(const char* path, int32_t dtype, void* cube, int64_t cap_elems, int32_t dims_out[3],
                           double* servo_angle, int32_t angle_cap, int32_t* n_angle);
/* save(frame_sim_array_%d.mat, ...): generation 1 -> `raw_iq_data`, 2 ->
 * `raw_iq_data_noise_sample`; complex double cube [P x N x C] interleaved; servo_angle
 * 1 x n_angle (omitted if NULL or n_angle == 0). */
int32_t rsp_mat_save_frame(const char* path, const double* cube, int32_t P, int32_t N, int32_t C,
                           const double* servo_angle, int32_t n_angle, int32_t generation, int32_t compress);

/* ---- MUSIC direction finding (BASELINE config #5) ----
 * MUSIC_1D.m:21-48 and run_music_algorithm.m:22-69: per instance X [N x K] (complex,
 * column-major, instances stacked as [N x K x I]):
 *   R = X*X'/K (MUSIC_1D.m:28); [EV, D] = eig(R), sort 'descend' (:29-32);
 *   Q_n = EV(:, M+1:N) (:33); P = 1./sum(abs(Q_n'*S1).^2) over the scan grid (:35-37);
 *   P_dB = 10*log10(P/max(P)) (:39-41); findpeaks(P_dB), the M largest (:43-47).
 * The reference scripts have no function signature; these entry points take the scripts'
 * variables (N, K, M, d/lambda, phi_list) as the plan and X as the data.  Arithmetic: complex
 * double by default, like MATLAB (f64 MFMA covariance, Householder + multisection + inverse
 * iteration in double); complex single on request (precision = RSP_C64).  Outputs are double
 * either way.  Tolerances vs the complex128 oracle: tests/test_music.py. */
typedef struct rsp_music_config {
    int32_t channel_num;      /* N, 2..64 (MUSIC_1D.m:10; BASELINE #5: 64)                 */
    int32_t num_snapshots;    /* K (MUSIC_1D.m:18; BASELINE #5: 1024)                      */
    int32_t num_sources;      /* M = signal subspace dimension, 1..min(8, N-1) (:15)       */
    int32_t n_scan;           /* scan grid length, 3..4096 (MUSIC_1D.m:35: 200)             */
    double d_over_lambda;     /* element spacing / wavelength (MUSIC_1D.m:11: 0.5)         */
    const double* scan_rad;   /* phi_list in radians, n_scan entries (borrowed for create) */
    int32_t max_batch;        /* instances per call (device buffers sized for it)          */
    int32_t precision;        /* RSP_C128 (complex double, MATLAB's; default) or RSP_C64:
                                 the device snapshots, covariance and eigensolver            */
} rsp_music_config;

/* Synthetic signal model of MUSIC_1D.m:14-24 / run_music_algorithm.m:14-39; MATLAB randn is
 * replaced by the Philox streams documented in oracle/music.py. */
typedef struct rsp_music_scene {
    int32_t n_src;            /* sources, 1..8                                              */
    int32_t complex_sources;  /* 0: Alpha = randn(M,K) (MUSIC_1D.m:22); 1: (randn+1j*randn)/sqrt(2)
                                 (run_music_algorithm.m:30-32); both scaled by amplitudes[m] */
    int32_t snr_measured;     /* 1: awgn(X, SNR, 'measured') (MUSIC_1D.m:24);
                                 0: noise power 1/10^(SNR/10) (run_music_algorithm.m:35)    */
    int32_t reserved;
    double snr_db;
    double angles_rad[8];     /* phi (MUSIC_1D.m:14)                                        */
    double amplitudes[8];     /* source_amplitudes (run_music_algorithm.m:15); 1 for MUSIC_1D */
} rsp_music_scene;

/* Caller-owned outputs for n_inst instances; any pointer may be NULL (not produced). */
typedef struct rsp_music_out {
    double* spectrum_db;      /* [n_scan x I] P_MUSIC_dB (MUSIC_1D.m:41)                      */
    double* eigenvalues;      /* [N x I] descending (MUSIC_1D.m:30-31); when NULL, complex double
                                 (M <= 4) first finds only the signal subspace (the block-power
                                 fast path with a proven 1e-12 subspace bound,
                                 rsp_music_fast_count); a peaks-only call keeps it whenever the
                                 bound is proven, a call that reads spectrum_db only where the
                                 bound also holds P_dB to 1e-8 dB; otherwise (and M > 4) the full
                                 eigensolver finds the M signal eigenvalues the spectrum needs */
    int32_t* peak_idx;        /* [M x I] 1-based scan indices of the M largest peaks (:43-47), 0 = none */
    int32_t* n_peaks;         /* [I] number of findpeaks peaks                                 */
    double* covariance;       /* complex [N x N x I] R (MUSIC_1D.m:28), column-major           */
} rsp_music_out;

typedef struct rsp_music_plan rsp_music_plan;

int32_t rsp_music_create(const rsp_music_config* cfg, int32_t device, rsp_music_plan** out);
int32_t rsp_music_destroy(rsp_music_plan* plan);
/* Host snapshots X [N x K x n_inst] (RSP_C64 or RSP_C128), synchronous. */
int32_t rsp_music_process(rsp_music_plan* plan, const void* X, int32_t dtype, int32_t n_inst, rsp_music_out* out);
/* Device-resident snapshots in the plan's precision ([N x K x n_inst], complex double or single);
 * results copied to `out` (NULL: results stay on the device). */
int32_t rsp_music_process_device(rsp_music_plan* plan, const void* d_X, int32_t n_inst, rsp_music_out* out);
/* Synthesise n_inst instances (instance ids inst0..) into device memory d_X [N x K x n_inst]. */
int32_t rsp_music_synthesize_device(rsp_music_plan* plan, const rsp_music_scene* scene, int32_t n_inst,
                                    int32_t inst0, uint64_t seed, void* d_X);
/* HIP-event timing of the two device stages (ms_out[0] covariance, ms_out[1] eig + spectrum)
 * averaged over `iters` launches on the plan's stream, in the peaks-only form of a call (the
 * eigenvalues not requested: complex double then finds only the M signal eigenvalues). */
int32_t rsp_music_profile(rsp_music_plan* plan, const void* d_X, int32_t n_inst, int32_t iters, float* ms_out);
/* The same timing for the form of call `what` names: RSP_MUSIC_PEAKS (= rsp_music_profile: only
 * peak_idx / n_peaks read; the block-power fast path may stand in for the eigensolver),
 * RSP_MUSIC_SPECTRUM (spectrum_db read too: the fast path only where it bounds P_dB to 1e-8 dB,
 * else the full eigensolver for the M signal eigenvalues) or
 * RSP_MUSIC_EIGENVALUES (eigenvalues read: the full eigensolver, all N eigenvalues -- the
 * 3-output rsp_mex('music') call and music_1d_calllib.m, MUSIC_1D.m:29-33). */
#define RSP_MUSIC_PEAKS 0
#define RSP_MUSIC_SPECTRUM 1
#define RSP_MUSIC_EIGENVALUES 2
int32_t rsp_music_profile_ex(rsp_music_plan* plan, const void* d_X, int32_t n_inst, int32_t iters, int32_t what,
                             float* ms_out);
/* Instances of the last call whose signal subspace came from the block-power fast path (complex
 * double, calls that do not read the eigenvalues, M <= 4: the iteration converged with a proven
 * 1e-12 subspace bound -- and, when spectrum_db is read, that bound holds P_dB to 1e-8 dB;
 * rsp_music.hip me_fast_subspace); the others ran the full tridiagonal eigensolver.  Diagnostic. */
int32_t rsp_music_fast_count(rsp_music_plan* plan, int32_t* n_fast);
int32_t rsp_music_device_alloc(rsp_music_plan* plan, int64_t bytes, void** d_ptr);
int32_t rsp_music_device_free(rsp_music_plan* plan, void* d_ptr);
int32_t rsp_music_device_download(rsp_music_plan* plan, void* h_dst, const void* d_src, int64_t bytes);

/* ---- 2-D MUSIC for a uniform rectangular array (MUSIC_2D.m) ----
 * MUSIC_2D.m:52-138 per instance X [N x K], N = nx*ny elements, element (ix, iy) is channel
 * iy + ny*ix (meshgrid(0:Nx-1, 0:Ny-1) flattened by (:), MUSIC_2D.m:17-19):
 *   R = X*X'/K, eig, sort 'descend', Q_n (:52-57);
 *   a(phi, theta) = exp(1j*2*pi*(dx/lambda*ix*cos(theta)*cos(phi) + dy/lambda*iy*cos(theta)*sin(phi)))
 *   (:35,87-89); P = 1./sum(abs(Q_n'*S1).^2) over the n_theta x n_phi grid (:92-93);
 *   P_dB = 10*log10(P/max(P(:))) (:96-98); imregionalmax (8-connected), the M largest (:119-124).
 * rsp_music_create_2d returns the same plan type as rsp_music_create, and rsp_music_process,
 * rsp_music_process_device, rsp_music_fast_count, rsp_music_device_alloc / _free / _download and
 * rsp_music_destroy take it with N = nx*ny and n_scan = n_theta*n_phi.  In rsp_music_out:
 *   spectrum_db [n_theta x n_phi x I], column-major with theta fastest (P_MUSIC_dB);
 *   peak_idx    [M x I] 1-based linear indices r + n_theta*(c - 1) (sub2ind, :123), 0 = none;
 *   n_peaks     [I] pixels of the imregionalmax mask (length(peak_vals), :123);
 *   eigenvalues, covariance as for a line-array plan.
 * A peaks-only call (M <= 4) may keep the block-power signal subspace (rsp_music_fast_count); a
 * call that reads spectrum_db or eigenvalues runs the full eigensolver.  Complex double only.
 * Device memory: the spectrum buffer is max_batch * n_theta*n_phi * 8 bytes (132 KB per instance
 * at MUSIC_2D.m's 91 x 181 grid), next to max_batch * 64 KB of covariance.
 * rsp_music_synthesize_device, rsp_music_profile and rsp_music_profile_ex refuse a 2-D plan, and
 * the _2d calls below refuse a line-array plan (RSP_ERR_INVALID).
 * Tolerances vs the complex128 restatement: tests/test_music2d.py. */
typedef struct rsp_music2d_config {
    int32_t nx, ny;            /* URA elements along x and y (MUSIC_2D.m:10-12); N = nx*ny in 2..64 */
    int32_t num_snapshots;     /* K (MUSIC_2D.m:30)                                             */
    int32_t num_sources;       /* M, 1..min(8, N-1)                                             */
    int32_t n_phi, n_theta;    /* each 3..1024, n_phi*n_theta <= 65536 (MUSIC_2D.m:61-62: 181, 91) */
    double dx_over_lambda, dy_over_lambda;   /* MUSIC_2D.m:13-14: 0.5, 0.5                      */
    const double* phi_rad;     /* azimuth grid, n_phi entries (borrowed for create)             */
    const double* theta_rad;   /* elevation grid, n_theta entries                               */
    int32_t max_batch;         /* instances per call (device buffers sized for it)              */
    int32_t precision;         /* RSP_C128 (RSP_C64: RSP_ERR_UNSUPPORTED)                        */
} rsp_music2d_config;

/* rsp_music_scene plus the elevations (MUSIC_2D.m:24-25,46-48: complex_sources = 1,
 * snr_measured = 1); the Philox streams are those of the line array (noise index c + N*k with
 * c = iy + ny*ix). */
typedef struct rsp_music2d_scene {
    int32_t n_src, complex_sources, snr_measured, reserved;
    double snr_db;
    double azim_rad[8];        /* phi   (MUSIC_2D.m:24) */
    double elev_rad[8];        /* theta (MUSIC_2D.m:25) */
    double amplitudes[8];
} rsp_music2d_scene;

int32_t rsp_music_create_2d(const rsp_music2d_config* cfg, int32_t device, rsp_music_plan** out);
int32_t rsp_music_synthesize_device_2d(rsp_music_plan* plan, const rsp_music2d_scene* scene, int32_t n_inst,
                                       int32_t inst0, uint64_t seed, void* d_X);
/* HIP-event timing of the four device stages, averaged over `iters` launches: ms_out[0]
 * covariance, [1] signal subspace, [2] scan, [3] dB + peaks; `what` as rsp_music_profile_ex. */
int32_t rsp_music_profile_2d(rsp_music_plan* plan, const void* d_X, int32_t n_inst, int32_t iters, int32_t what,
                             float* ms_out);

#ifdef __cplusplus
}
#endif
#endif /* RSP_H */
