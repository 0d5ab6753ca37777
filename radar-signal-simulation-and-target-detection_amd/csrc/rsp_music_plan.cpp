// rsp_music_plan.cpp -- the MUSIC plan and its C-ABI (include/rsp.h, MUSIC sections).  Every check,
// size, table, routing decision and host conversion is rsp_music_geometry.{h,cpp}'s; the kernels and
// their launchers are rsp_music.hip's.  This file owns the device objects and the order of calls.
#include "rsp.h"
#include "rsp_internal.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

__attribute__((visibility("hidden"))) int rsp_set_error(int code, const char* fmt, ...);   // rsp_host.cpp

struct rsp_music_plan {
    int device = 0;
    MusicDesc d;
    hipStream_t stream = nullptr;
    void* buf[MB_COUNT] = {};   // by MusicBuf
    hipEvent_t ev[5] = {};
    int last_inst = 0;          // instances of the last eig launch (rsp_music_fast_count)
};

namespace {

#define MUCHK(expr)                                                                                    \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return rsp_set_error(RSP_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                 __FILE__, __LINE__);                                                  \
    } while (0)

// rsp_music_create / _2d: the checks, then stream, events, the buffers of music_buffer_bytes and the
// steering table (narrowed for a complex-single plan)
template <class CFG>
int music_create(const CFG* cfg, int device, rsp_music_plan** out) {
    MusicDesc d;
    if (out) *out = nullptr;
    const int rc = music_describe(cfg, out ? &d : nullptr);
    if (rc) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return rsp_set_error(RSP_ERR_DEVICE, "HIP device %d not available (%d devices)", device, ndev);
    rsp_music_plan* p = new rsp_music_plan();
    p->device = device;
    p->d = d;
    auto bail = [&](int rc) { rsp_music_destroy(p); return rc; };
    if (hipSetDevice(device) != hipSuccess) return bail(rsp_set_error(RSP_ERR_DEVICE, "hipSetDevice(%d)", device));
    if (hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking) != hipSuccess)
        return bail(rsp_set_error(RSP_ERR_DEVICE, "hipStreamCreate failed"));
    for (auto& e : p->ev)
        if (hipEventCreate(&e) != hipSuccess) return bail(rsp_set_error(RSP_ERR_DEVICE, "hipEventCreate failed"));
    size_t bytes[MB_COUNT];
    music_buffer_bytes(d, bytes);
    bytes[MB_X] = 0;   // on first use (rsp_music_process)
#ifdef RSP_DEBUG_KNOBS   // diagnostic builds only: the shipped library reads no environment variable
    const char* tr = getenv("RSP_MUSIC_TRACE");
    if (!tr || !atoi(tr)) bytes[MB_TRACE] = 0;
#else
    bytes[MB_TRACE] = 0;
#endif
    for (int b = 0; b < MB_COUNT; ++b)
        if (bytes[b] && hipMalloc(&p->buf[b], bytes[b]) != hipSuccess)
            return bail(rsp_set_error(RSP_ERR_NOMEM, "hipMalloc(%zu bytes) failed", bytes[b]));
    const std::vector<double> tab = music_table(d, cfg);
    const int tb = d.planar ? MB_EXY : MB_S1T;
    std::vector<unsigned char> stage;
    if (hipMemcpy(p->buf[tb], music_in_precision(d, tab.data(), RSP_C128, tab.size(), stage), bytes[tb], hipMemcpyHostToDevice) != hipSuccess)
        return bail(rsp_set_error(RSP_ERR_DEVICE, "steering upload failed"));
    *out = p;
    return RSP_OK;
}

// The stages of the route of `want` (MusicWant) on the plan's stream; timed: ms[q] = stage q's time.
int music_run(rsp_music_plan* p, const void* dX, int n_inst, bool timed, float* ms, int want) {
    if (n_inst < 1 || n_inst > p->d.max_batch)
        return rsp_set_error(RSP_ERR_INVALID, "n_inst %d outside 1..max_batch %d", n_inst, p->d.max_batch);
    MUCHK(hipSetDevice(p->device));
    const MusicRoute r = music_route(p->d, want);
    p->last_inst = n_inst;
    for (int q = 0; q < r.n_stages; ++q) {   // MusicStage q
        if (timed) MUCHK(hipEventRecord(p->ev[q], p->stream));
        MUCHK(launch_music_stage(q, p->d, r, p->buf, dX, n_inst, p->stream));
    }
    if (timed) {
        MUCHK(hipEventRecord(p->ev[r.n_stages], p->stream));
        MUCHK(hipEventSynchronize(p->ev[r.n_stages]));
        for (int q = 0; q < r.n_stages; ++q) MUCHK(hipEventElapsedTime(&ms[q], p->ev[q], p->ev[q + 1]));
    }
    return RSP_OK;
}

// device results -> caller (music_fetch_plan says what goes where)
int music_fetch(rsp_music_plan* p, int n_inst, rsp_music_out* out) {
    MusicFetch f;
    music_fetch_plan(p->d, n_inst, out, &f);
    for (int c = 0; c < f.n; ++c)
        MUCHK(hipMemcpyAsync(f.copy[c].dst, p->buf[f.copy[c].buf], f.copy[c].bytes, hipMemcpyDeviceToHost, p->stream));
    MUCHK(hipStreamSynchronize(p->stream));
    music_unpack(p->d, n_inst, f, out);
    return RSP_OK;
}

// rsp_music_synthesize_device / _2d
template <class SC>
int music_synth(rsp_music_plan* p, const SC* sc, int n_inst, int inst0, uint64_t seed, void* d_X) {
    if (!p || !sc || !d_X) return rsp_set_error(RSP_ERR_INVALID, "null argument");
    MusicSynth sy;
    const int rc = music_scene(p->d, sc, n_inst, &sy);
    if (rc) return rc;
    MUCHK(hipSetDevice(p->device));
    MUCHK(hipMemcpyAsync(p->buf[MB_SRC], sy.src.data(), sy.src.size() * sizeof(double), hipMemcpyHostToDevice, p->stream));
    MUCHK(hipMemcpyAsync(p->buf[MB_AMP], sy.amp, sizeof sy.amp, hipMemcpyHostToDevice, p->stream));
    MUCHK(launch_music_synth(p->d, sy, p->buf, n_inst, inst0, seed, d_X, p->stream));
    MUCHK(hipStreamSynchronize(p->stream));   // the staging above is the caller's stack and heap
    return RSP_OK;
}

// rsp_music_profile_ex / _2d: the mean stage times of `iters` timed runs in the form `what`
int music_profile(rsp_music_plan* p, bool planar_entry, const void* d_X, int n_inst, int iters, int what, float* ms_out) {
    if (!p || !d_X || !ms_out || iters < 1) return rsp_set_error(RSP_ERR_INVALID, "bad argument");
    if (p->d.planar != planar_entry)
        return rsp_set_error(RSP_ERR_INVALID, planar_entry ? "rsp_music_profile_2d on a line-array plan"
                                                           : "planar-array plan: use rsp_music_profile_2d (four stages)");
    int want = MU_WANT_PEAKS;
    const int rc = music_want_of_form(what, &want);
    if (rc) return rc;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const int ns = music_route(p->d, want).n_stages;
    for (int it = 0; it < iters; ++it) {
        float ms[4];
        const int rr = music_run(p, d_X, n_inst, true, ms, want);
        if (rr) return rr;
        for (int q = 0; q < ns; ++q) acc[q] += ms[q];
    }
    for (int q = 0; q < ns; ++q) ms_out[q] = (float)(acc[q] / iters);
    return RSP_OK;
}

}  // namespace

extern "C" {

int32_t rsp_music_create(const rsp_music_config* cfg, int32_t device, rsp_music_plan** out) {
    return music_create(cfg, device, out);
}
int32_t rsp_music_create_2d(const rsp_music2d_config* cfg, int32_t device, rsp_music_plan** out) {
    return music_create(cfg, device, out);
}

int32_t rsp_music_destroy(rsp_music_plan* p) {
    if (!p) return RSP_OK;
    (void)hipSetDevice(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    for (void* b : p->buf)
        if (b) (void)hipFree(b);
    for (auto& e : p->ev)
        if (e) (void)hipEventDestroy(e);
    if (p->stream) (void)hipStreamDestroy(p->stream);
    delete p;
    return RSP_OK;
}

int32_t rsp_music_synthesize_device(rsp_music_plan* p, const rsp_music_scene* sc, int32_t n_inst, int32_t inst0,
                                    uint64_t seed, void* d_X) {
    return music_synth(p, sc, n_inst, inst0, seed, d_X);
}
int32_t rsp_music_synthesize_device_2d(rsp_music_plan* p, const rsp_music2d_scene* sc, int32_t n_inst, int32_t inst0,
                                       uint64_t seed, void* d_X) {
    return music_synth(p, sc, n_inst, inst0, seed, d_X);
}

int32_t rsp_music_process_device(rsp_music_plan* p, const void* d_X, int32_t n_inst, rsp_music_out* out) {
    if (!p || !d_X) return rsp_set_error(RSP_ERR_INVALID, "null argument");
    const int rc = music_run(p, d_X, n_inst, false, nullptr, music_want(out));
    if (rc) return rc;
    if (!out) {
        MUCHK(hipStreamSynchronize(p->stream));
        return RSP_OK;
    }
    return music_fetch(p, n_inst, out);
}

int32_t rsp_music_process(rsp_music_plan* p, const void* X, int32_t dtype, int32_t n_inst, rsp_music_out* out) {
    if (!p || !X) return rsp_set_error(RSP_ERR_INVALID, "null argument");
    const MusicDesc& d = p->d;
    if (n_inst < 1 || n_inst > d.max_batch)
        return rsp_set_error(RSP_ERR_INVALID, "n_inst %d outside 1..max_batch %d", n_inst, d.max_batch);
    if (dtype != RSP_C64 && dtype != RSP_C128) return rsp_set_error(RSP_ERR_INVALID, "unknown dtype %d", dtype);
    MUCHK(hipSetDevice(p->device));
    const size_t reals = (size_t)2 * n_inst * d.K * d.N;
    if (!p->buf[MB_X]) {
        size_t bytes[MB_COUNT];
        music_buffer_bytes(d, bytes);
        if (hipMalloc(&p->buf[MB_X], bytes[MB_X]) != hipSuccess)
            return rsp_set_error(RSP_ERR_NOMEM, "hipMalloc(%zu bytes) failed", bytes[MB_X]);
    }
    std::vector<unsigned char> stage;   // snapshots of the other precision: widened or narrowed
    MUCHK(hipMemcpy(p->buf[MB_X], music_in_precision(d, X, dtype, reals, stage), reals / 2 * d.xsz(), hipMemcpyHostToDevice));
    return rsp_music_process_device(p, p->buf[MB_X], n_inst, out);
}

int32_t rsp_music_profile(rsp_music_plan* p, const void* d_X, int32_t n_inst, int32_t iters, float* ms_out) {
    return rsp_music_profile_ex(p, d_X, n_inst, iters, RSP_MUSIC_PEAKS, ms_out);
}

int32_t rsp_music_profile_2d(rsp_music_plan* p, const void* d_X, int32_t n_inst, int32_t iters, int32_t what,
                             float* ms_out) {
    return music_profile(p, true, d_X, n_inst, iters, what, ms_out);
}

int32_t rsp_music_profile_ex(rsp_music_plan* p, const void* d_X, int32_t n_inst, int32_t iters, int32_t what,
                             float* ms_out) {
    const int rc = music_profile(p, false, d_X, n_inst, iters, what, ms_out);
    if (rc || !p->buf[MB_TRACE]) return rc;
    // mean phase durations of the last launch (s_memrealtime: 100 MHz)
    std::vector<unsigned long long> t((size_t)n_inst * 8);
    MUCHK(hipMemcpy(t.data(), p->buf[MB_TRACE], t.size() * sizeof(t[0]), hipMemcpyDeviceToHost));
    auto mean = [&](int a, int b) {   // us between stamps a and b
        double us = 0;
        for (int i = 0; i < n_inst; ++i) us += (double)(t[(size_t)i * 8 + b] - t[(size_t)i * 8 + a]) * 0.01 / n_inst;
        return us;
    };
    // stamp 7 (complex double): dlagtf's end, inside the inverse-iteration phase
    fprintf(stderr, "k_music_eig%s phases (us/instance): tridiag %.2f eigenvalues %.2f inviter %.2f (dlagtf %.2f) backxf %.2f spectrum %.2f peaks %.2f\n",
            p->d.f64 ? "64" : "", mean(0, 1), mean(1, 2), mean(2, 3), p->d.f64 ? mean(2, 7) : 0.0, mean(3, 4), mean(4, 5), mean(5, 6));
    return RSP_OK;
}

int32_t rsp_music_device_alloc(rsp_music_plan* p, int64_t bytes, void** d_ptr) {
    if (!p || !d_ptr || bytes <= 0) return rsp_set_error(RSP_ERR_INVALID, "bad argument");
    MUCHK(hipSetDevice(p->device));
    if (hipMalloc(d_ptr, (size_t)bytes) != hipSuccess)
        return rsp_set_error(RSP_ERR_NOMEM, "hipMalloc(%lld bytes) failed", (long long)bytes);
    return RSP_OK;
}

int32_t rsp_music_device_free(rsp_music_plan* p, void* d_ptr) {
    if (!p) return rsp_set_error(RSP_ERR_INVALID, "null plan");
    MUCHK(hipSetDevice(p->device));
    MUCHK(hipStreamSynchronize(p->stream));
    MUCHK(hipFree(d_ptr));
    return RSP_OK;
}

int32_t rsp_music_fast_count(rsp_music_plan* p, int32_t* n_fast) {
    if (!p || !n_fast) return rsp_set_error(RSP_ERR_INVALID, "bad argument");
    *n_fast = 0;
    // only the complex-double eigen kernels write the flag, and only a row with M < MU_MMAX has the slot
    if (!music_route(p->d, MU_WANT_PEAKS).fast_flag || p->last_inst < 1) return RSP_OK;
    MUCHK(hipSetDevice(p->device));
    MUCHK(hipStreamSynchronize(p->stream));
    std::vector<int> pk((size_t)p->last_inst * MU_PK_ROW);
    MUCHK(hipMemcpy(pk.data(), p->buf[MB_PEAKS], pk.size() * sizeof(int), hipMemcpyDeviceToHost));
    *n_fast = music_fast_count(pk.data(), p->last_inst);
    return RSP_OK;
}

int32_t rsp_music_device_download(rsp_music_plan* p, void* h_dst, const void* d_src, int64_t bytes) {
    if (!p || !h_dst || !d_src || bytes < 0) return rsp_set_error(RSP_ERR_INVALID, "bad argument");
    MUCHK(hipSetDevice(p->device));
    MUCHK(hipStreamSynchronize(p->stream));
    MUCHK(hipMemcpy(h_dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost));
    return RSP_OK;
}

}  // extern "C"
