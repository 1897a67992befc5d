// ctx.h -- the runtime units' private view of a context: nori_gpu_ctx and
// nori_gpu_comm, device buffers, HIP error handling, the kernel clock, the
// film target, and the few functions that cross units.  Included by upload.hip, render.hip, queries.hip,
// film_splat.hip, li.hip, adaptive.hip, dynamic.hip, materials.hip and sharded.hip only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "comm.h"
#include "kernels.h"
#include "render_plan.h"
#include "scene_plan.h"
#include "scene_prep.h"

#define HIP_TRY(x)                                                                                       \
    do {                                                                                                 \
        hipError_t e_ = (x);                                                                             \
        if (e_ != hipSuccess) throw NoriException(NORI_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
    } while (0)

namespace nori {

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    void ensure(size_t n) {
        if (n <= bytes && p) return;
        release();
        hipError_t e = hipMalloc(&p, n ? n : 16);
        if (e != hipSuccess) {
            p = nullptr;
            throw NoriException(NORI_ERR_OOM, std::string("hipMalloc(") + std::to_string(n) + "): " + hipGetErrorString(e));
        }
        bytes = n;
    }
    template <class T> void upload(const std::vector<T> &v) {
        ensure(v.size() * sizeof(T));
        if (!v.empty()) HIP_TRY(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

enum KernelKind { kKindExtend, kKindShadow, kKindShade, kKindSplat, kKindFinish, kKernelKinds };  // the ms_* of nori_gpu_stats

// The HIP-event times of a call's launches, summed per kind.  A local clock per
// timed render; the context's own (c.clock) for the queries, which collect after
// every chunk and so reuse the same three events.
struct KernelClock {
    struct Span {
        size_t a, b;  // indices into ev
        int kind;
    };
    bool on;
    double ms[kKernelKinds] = {};
    std::vector<hipEvent_t> ev;
    size_t used = 0;
    std::vector<Span> spans;  // not yet collected
    explicit KernelClock(bool enabled = true) : on(enabled) {}
    KernelClock(const KernelClock &) = delete;
    ~KernelClock() {
        for (auto e : ev) (void)hipEventDestroy(e);
    }
    void reset(bool enabled) {  // (the context's clock, at the start of a call)
        on = enabled;
        spans.clear();
        used = 0;
        std::memset(ms, 0, sizeof(ms));
    }
    size_t mark(hipStream_t st) {
        if (used == ev.size()) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e));
            ev.push_back(e);
        }
        HIP_TRY(hipEventRecord(ev[used], st));
        return used++;
    }
    // launch() on `st`, between two events when the clock is enabled.  chained: the
    // launch follows the last span's on the same stream with nothing between, and
    // that span's end event is this one's start.
    template <class Launch> void span(hipStream_t st, int kind, Launch &&launch, bool chained = false) {
        if (!on) {
            HIP_TRY(launch());
            return;
        }
        const size_t a = chained && !spans.empty() ? spans.back().b : mark(st);
        HIP_TRY(launch());
        spans.push_back(Span{a, mark(st), kind});
    }
    // after the caller has synchronised the spans' streams: their times into ms[], the events free again
    void collect() {
        for (const Span &s : spans) {
            float t = 0.0f;
            HIP_TRY(hipEventElapsedTime(&t, ev[s.a], ev[s.b]));
            ms[s.kind] += t;
        }
        spans.clear();
        used = 0;
    }
};

}  // namespace nori

using namespace nori;  // (the C ABI's opaque types are global and made of nori:: ones)

struct nori_gpu_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t side = nullptr;       // film splat, overlapped with the tail finisher
    hipEvent_t fork = nullptr, join = nullptr;
    hipStream_t parts[kMaxParts] = {};  // parts[0] unused (part 0 runs on `stream`)
    hipEvent_t joins[kMaxParts] = {};
    DevScene S{};
    ScanRtc rtc;         // scan-mode scenes: the scan kernels specialised for this scene (rtc.hip), or empty
    ShadeRtc shade_rtc;  // ... with the basic plugins: k_shade compiled for this scene (rtc.hip), or empty
    // an iteration's extension and shadow rays of a part in one launch
    // (launch_trace_both); set at upload_scene (NORI_TRACE_FUSE=0 / 1 forces it)
    bool fuse_trace = true;
    // the tail's finisher enqueued before the film splat beside it (NORI_FINISH_FIRST=0: after)
    bool finish_first = true;
    nori_camera_desc cam{};
    DevBuf nodes, prims, tri_vidx, pos, nrm, prim_shape, shapes, bsdfs, emitters, cdf, env, blob, plane_c, plane_f;
    DevBuf tex;          // ImageTexture / NormalMap texels (RGBX8), global memory
    uint32_t spp = 1;    // the scene's sampleCount (default pass count)
    uint32_t scene_spp = 0;  // ... as the scene gives it (0 stays 0: nori_gpu_film_splat_passes has no array to size by 1)
    int stack = 8;       // traversal of extend/shadow: 0 = wave-uniform scan, else LDS stack depth
    uint32_t bvh_depth = 0, bvh_nodes = 0, num_prims = 0;
    size_t scene_bytes = 0;
    std::atomic<int> cancel{0};
    std::atomic<float> progress{1.0f};
    // nori_gpu_render_adaptive runs render() once per round: inside it a
    // round's progress f is reported as prog_off + prog_scale * f, and the
    // rounds do not clear a cancel request (the adaptive call clears it once)
    double prog_off = 0.0, prog_scale = 1.0;
    bool in_rounds = false;
    void report(double f) { progress = (float)(prog_off + prog_scale * f); }
    DevBuf errbuf, errids;           // adaptive rounds: per-block error, the blocks to evaluate
    // render state
    DevBuf q[2][5], sq[3], seg[4], segstats, tailpre, rec, counters, pixels, blocks, film;
    DevBuf varbuf;                   // per-pixel sample statistics when variance_out is a host buffer
    // nori_gpu_query / nori_gpu_camera_rays: staging of host rays, hits and records (q_hits also
    // serves a device query without a hit output), reused across calls; the clock of their kernels
    // (and of nori_gpu_li's and the film splats')
    DevBuf q_rays, q_hits, q_surf;
    KernelClock clock;
    // the shading queries (nori_gpu_bsdf_eval ..): staging of up to three host input arrays and the output
    // (nori_gpu_film_splat*: sh_in[0] / sh_in[1] stage host positions and values)
    DevBuf sh_in[3], sh_out;
    // nori_gpu_li: its ray and invalid-row counters (rays, stream ids and values are staged in q_rays, sh_in[0], sh_out)
    DevBuf li_count;
    DevBuf ph, ph_rgbe, ph_tab, ph_start;             // photonmapper: photon map (photon_map.cpp) and its hash-grid buckets
    // nori_gpu_update_vertices: the refit schedule (host copy of its level bounds, device copy of
    // its slots), staging of host positions / normals, the non-finite counter, the shapes as
    // uploaded (area_norm and solitary change) and the meshes that carry an emitter
    RefitPlan refit;
    DevBuf refit_slots, upd_pos, upd_nrm, upd_count;
    hipEvent_t upd_ev[2] = {};
    uint32_t num_vertices = 0;
    // nori_gpu_rebuild_bvh: the stack NORI_BVH_STACK forced at creation (0: none), and the scratch
    // the new tree is built in -- rb_nodes, rb_prims and rb_slots are swapped with nodes, prims
    // and refit_slots on success, so a context that rebuilds holds two trees' worth of buffers
    int stack_forced = 0;
    DevBuf rb_box, rb_keys[2], rb_sort_tmp, rb_scan_tmp, rb_prims, rb_nodes, rb_refs, rb_ranges[2], rb_ends, rb_count,
        rb_scan, rb_inner, rb_leaf, rb_slots;
    hipEvent_t rb_ev[2] = {};
    // nori_gpu_update_materials / nori_gpu_bsdf_grad (materials.hip): the scene's BSDF count, the
    // successful updates so far, staging of host rows (also the host form's zeroed sums), the
    // table path's slabs of partial sums, staging of host gradient rows and of the terms
    uint32_t num_bsdfs = 0;
    uint64_t materials_version = 0;
    DevBuf mat_rows, bg_slabs, bg_gout, bg_terms;
    std::vector<DevShape> hshapes;
    std::vector<EmitterMesh> emitter_meshes;
    uint32_t pool_cap = 0;
    uint32_t *pinned = nullptr;      // host-mapped flags: [0] done, [1] exhausted segments
    uint32_t *pinned_dev = nullptr;  // device view of `pinned`
    // the render's blocks (spiral order, block_subset applied) and their
    // block-major pixel list, with device copies in `pixels` / `blocks`:
    // rebuilt and uploaded only when the block selection changes
    std::vector<uint32_t> work_order, hpixels;
    std::vector<int4> hblocks;
    bool work_valid = false;
    // pinned staging of the end-of-render read-back (Counters + per-segment stats)
    char *readback = nullptr;
    size_t readback_bytes = 0;
    std::vector<hipEvent_t> ring[kMaxParts];
    ~nori_gpu_ctx() {
        for (auto &r : ring)
            for (auto e : r) (void)hipEventDestroy(e);
        for (int h = 1; h < kMaxParts; ++h) {
            if (joins[h]) (void)hipEventDestroy(joins[h]);
            if (parts[h]) (void)hipStreamDestroy(parts[h]);
        }
        scan_rtc_release(rtc);
        shade_rtc_release(shade_rtc);
        for (auto e : upd_ev)
            if (e) (void)hipEventDestroy(e);
        for (auto e : rb_ev)
            if (e) (void)hipEventDestroy(e);
        if (pinned) (void)hipHostFree(pinned);
        if (readback) (void)hipHostFree(readback);
        if (fork) (void)hipEventDestroy(fork);
        if (join) (void)hipEventDestroy(join);
        if (side) (void)hipStreamDestroy(side);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

struct nori_gpu_comm {
    void *nccl = nullptr;  // ncclComm_t (comm.cpp)
    int nranks = 1, rank = 0, device = 0;
    bool aborted = false;   // ncclCommAbort ran: every later call fails
    int *status_dev = nullptr, *status_host = nullptr;  // the per-render status exchange word
    ~nori_gpu_comm() {
        if (!aborted) comm_destroy(nccl);
        if (status_dev) (void)hipFree(status_dev);
        if (status_host) (void)hipHostFree(status_host);
    }
};

namespace nori {

// Throws NORI_ERR_INVALID with `msg` unless the runtime knows p as device memory
// (a host pointer would fault in the first kernel that reads it).
inline void require_device_ptr(const void *p, const std::string &msg) {
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess || (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged)) {
        (void)hipGetLastError();
        throw NoriException(NORI_ERR_INVALID, msg);
    }
}

// The fields of nori_gpu_stats that follow from the context alone, and the
// call's wall time since t0; the caller zeroes `s` and sets its own counters.
inline void scene_stats(const nori_gpu_ctx &c, std::chrono::steady_clock::time_point t0, nori_gpu_stats *s) {
    s->scene_bytes = c.scene_bytes;
    s->bvh_nodes = c.bvh_nodes;
    s->bvh_depth = c.bvh_depth;
    s->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    s->scan_rtc = c.rtc.extend ? 1u : 0u;  // (held: k_direct, k_features and k_surface scan generically)
    s->scan_rtc_cached = c.rtc.cached ? 1u : 0u;
    s->ms_scan_rtc = c.rtc.compile_ms;
}

// The start of a call's statistics (stats may be null: false): zeroed, scene_stats, one stream.
inline bool begin_stats(const nori_gpu_ctx &c, std::chrono::steady_clock::time_point t0, nori_gpu_stats *s) {
    if (!s) return false;
    std::memset(s, 0, sizeof(*s));
    scene_stats(c, t0, s);
    s->stream_parts = 1;
    return true;
}

// Where a call's kernels add the film and the per-pixel sample statistics: the
// caller's own arrays when they are device memory, else zeroed context buffers
// (c.film, c.varbuf) that finish() adds into the caller's host arrays.
struct FilmOut {
    nori_gpu_ctx &c;
    const bool on_device;
    float *const rgbw, *const variance;  // the caller's (variance may be null)
    float *film = nullptr, *var = nullptr;  // the device pointers, set by begin()
    const size_t film_elems, var_elems;
    FilmOut(nori_gpu_ctx &ctx, bool dev, float *rgbw_, float *variance_ = nullptr)
        : c(ctx), on_device(dev), rgbw(rgbw_), variance(variance_),
          film_elems(4 * (size_t)(c.S.W + 2 * c.S.border) * (size_t)(c.S.H + 2 * c.S.border)),
          var_elems(8 * (size_t)c.S.W * (size_t)c.S.H) {}
    void begin() {
        film = rgbw;
        var = variance;
        if (on_device) return;
        c.film.ensure(film_elems * sizeof(float));
        film = c.film.as<float>();
        HIP_TRY(hipMemsetAsync(film, 0, film_elems * sizeof(float), c.stream));
        if (!variance) return;
        c.varbuf.ensure(var_elems * sizeof(float));
        var = c.varbuf.as<float>();
        HIP_TRY(hipMemsetAsync(var, 0, var_elems * sizeof(float), c.stream));
    }
    void finish(bool cancelled) {  // (a cancelled call leaves the host arrays as they were)
        if (on_device || cancelled) return;
        std::vector<float> h(variance ? std::max(film_elems, var_elems) : film_elems);
        HIP_TRY(hipMemcpy(h.data(), film, film_elems * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < film_elems; ++i) rgbw[i] += h[i];
        if (!variance) return;
        HIP_TRY(hipMemcpy(h.data(), var, var_elems * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < var_elems; ++i) variance[i] += h[i];
    }
};

void work_lists(nori_gpu_ctx &c, const nori_gpu_render_desc &rd);                                       // render.hip
int render(nori_gpu_ctx &c, const nori_gpu_render_desc &rd, float *rgbw_out, nori_gpu_stats *stats);   // render.hip

}  // namespace nori
