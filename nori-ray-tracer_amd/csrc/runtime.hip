// runtime.hip -- libnori_gpu host runtime and C ABI (include/nori_gpu.h).
//
// nori_gpu_render replaces RenderThread::renderScene's pass loop
// (render.cpp:173-250): instead of spp sequential passes of a
// tbb::parallel_for over 32x32 blocks, every (pass, pixel) sample of the
// requested blocks becomes a work id; a pool of paths stays resident in HBM
// and the shade kernel refills finished slots from a device work counter, so
// the GPU stays full until the last sample.  Radiance accumulates per sample
// record; after the pool drains, k_splat applies ImageBlock::put.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "bsdf_desc.h"
#include "comm.h"
#include "host_scene.h"
#include "kernels.h"
#include "rebuild.h"

namespace nori {

static thread_local std::string g_last_error;
constexpr uint32_t kScanMaxPrims = 64;  // wave-uniform scan instead of BVH at or below this
constexpr size_t kBlobMaxBytes = 48 << 10;  // small-scene blob staged into LDS

#define HIP_TRY(x)                                                                                       \
    do {                                                                                                 \
        hipError_t e_ = (x);                                                                             \
        if (e_ != hipSuccess) throw NoriException(NORI_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
    } while (0)

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

// rfilter.cpp -> tabulated filter (block.cpp:54-66)
static float filter_eval(const nori_camera_desc &c, float x) {
    switch (c.filter_type) {
    case NORI_FILTER_GAUSSIAN: {
        float alpha = -1.0f / (2.0f * c.filter_p0 * c.filter_p0);
        float v = std::exp(alpha * x * x) - std::exp(alpha * c.filter_radius * c.filter_radius);
        return 0.0f < v ? v : 0.0f;
    }
    case NORI_FILTER_MITCHELL: {
        float B = c.filter_p0, C = c.filter_p1;
        x = std::fabs(2.0f * x / c.filter_radius);
        float x2 = x * x, x3 = x2 * x;
        if (x < 1) return 1.0f / 6.0f * ((12 - 9 * B - 6 * C) * x3 + (-18 + 12 * B + 6 * C) * x2 + (6 - 2 * B));
        if (x < 2) return 1.0f / 6.0f * ((-B - 6 * C) * x3 + (6 * B + 30 * C) * x2 + (-12 * B - 48 * C) * x + (8 * B + 24 * C));
        return 0.0f;
    }
    case NORI_FILTER_TENT: {
        float v = 1.0f - std::fabs(x);
        return 0.0f < v ? v : 0.0f;
    }
    case NORI_FILTER_BOX: return 1.0f;
    case NORI_FILTER_WINDOWED: {
        x = std::fabs(x);
        const float pi = 3.14159265358979323846f;
        auto sinc = [&](float y) { return y < 1e-5f ? 1.0f : std::sin(pi * y) / (pi * y); };
        return sinc(x) * sinc(x / c.filter_p0);
    }
    }
    return 0.0f;
}
static int film_border(const nori_camera_desc &c) { return (int)std::ceil(c.filter_radius - 0.5f); }
// k_splat's weights from a jitter class (device_math.h jit_class) need every
// step of ImageBlock::put's index arithmetic exact: a power-of-two radius and
// lookup factor (radius * lookup = NORI_FILTER_RESOLUTION), lookup <= 64 so
// that a class fits 8 bits.  The reference's default radii (gaussian and
// Mitchell 2, tent 1, box 0.5) qualify; other filters keep the pcg32 jitter.
static bool pow2f(float v) {
    int e = 0;
    return v > 0.0f && std::frexp(v, &e) == 0.5f;
}
static int jit_code_lookup(float radius, float lookup) {
    if (const char *e = std::getenv("NORI_JIT_CODE"); e && e[0] == '0') return 0;  // A/B
    if (!pow2f(radius) || !pow2f(lookup) || lookup > 64.0f || radius * lookup != (float)NORI_FILTER_RESOLUTION)
        return 0;
    return (int)lookup;
}
static void filter_table(const nori_camera_desc &c, float *t) {
    for (int i = 0; i < NORI_FILTER_RESOLUTION; ++i) t[i] = filter_eval(c, (c.filter_radius * i) / NORI_FILTER_RESOLUTION);
    t[NORI_FILTER_RESOLUTION] = 0.0f;
}

// EnvironmentMap tables (envmap.cpp:13-58, 91-109), appended to `env`.
// precompute1D literally: res is the LAST value of `i + f(row, i)`, and the CDF
// accumulates pf(i - 1), a column-major linear index into the whole pf matrix
// (rows not yet computed read as 0, as from a fresh allocation).
static float env_precompute1D(int row, const float *f, int cols, float *pf, float *Pf, int pf_rows) {
    float res = 0;
    int i;
    for (i = 0; i < cols; i++) res = (float)i + f[(size_t)row * cols + i];
    if (res == 0) return res;
    for (int j = 0; j < cols; j++) pf[(size_t)row * cols + j] = f[(size_t)row * cols + j] / res;
    Pf[(size_t)row * (cols + 1)] = 0;
    for (i = 1; i < cols; i++) {
        const int k = i - 1;
        Pf[(size_t)row * (cols + 1) + i] =
            Pf[(size_t)row * (cols + 1) + i - 1] + pf[(size_t)(k % pf_rows) * cols + (k / pf_rows)];
    }
    Pf[(size_t)row * (cols + 1) + i] = 1;
    return res;
}
static void build_envmap(const nori_emitter_desc &e, DevEmitter &o, std::vector<float> &env) {
    const int R = e.env_rows, C = e.env_cols;
    if (R < 2 || C < 2 || !e.env_rgb) throw NoriException(NORI_ERR_INVALID, "EnvMap: the image needs at least 2x2 texels");
    o.weight = e.weight;
    o.R = R;
    o.C = C;
    auto grab = [&](size_t n) {
        const size_t off = env.size();
        env.resize(off + n, 0.0f);
        return (uint32_t)off;
    };
    o.rgb_off = grab(3 * (size_t)R * C);
    std::memcpy(&env[o.rgb_off], e.env_rgb, 12 * (size_t)R * C);
    o.pdf_off = grab((size_t)R * C);
    o.cdf_off = grab((size_t)R * (C + 1));
    o.pmarg_off = grab((size_t)R);
    o.cmarg_off = grab((size_t)R + 1);
    if (env.size() >= (1ull << 32)) throw NoriException(NORI_ERR_UNSUPPORTED, "EnvMap: tables above 4G floats");
    std::vector<float> lum((size_t)R * C), sum((size_t)R);
    for (int i = 0; i < R; i++)
        for (int j = 0; j < C; j++) {
            const float *c = e.env_rgb + 3 * ((size_t)i * C + j);
            lum[(size_t)i * C + j] =
                std::sqrt((e.lum_scale[0] * c[0] + e.lum_scale[1] * c[1]) + e.lum_scale[2] * c[2]) + kEps / 10000000;
        }
    for (int i = 0; i < R; ++i) sum[i] = env_precompute1D(i, lum.data(), C, &env[o.pdf_off], &env[o.cdf_off], R);
    env_precompute1D(0, sum.data(), R, &env[o.pmarg_off], &env[o.cmarg_off], 1);
}

// BlockGenerator spiral (block.cpp:140-188)
static std::vector<uint32_t> spiral_blocks(int W, int H) {
    int nx = (int)std::ceil(W / (float)NORI_BLOCK_SIZE), ny = (int)std::ceil(H / (float)NORI_BLOCK_SIZE);
    std::vector<uint32_t> out;
    int left = nx * ny, dir = 0, bx = nx / 2, by = ny / 2, steps = 1, numSteps = 1;
    while (left > 0) {
        out.push_back((uint32_t)(by * nx + bx));
        if (--left == 0) break;
        do {
            switch (dir) {
            case 0: ++bx; break;
            case 1: ++by; break;
            case 2: --bx; break;
            default: --by; break;
            }
            if (--steps == 0) {
                dir = (dir + 1) % 4;
                if (dir == 2 || dir == 0) ++numSteps;
                steps = numSteps;
            }
        } while (bx < 0 || by < 0 || bx >= nx || by >= ny);
    }
    return out;
}

}  // namespace nori

using namespace nori;

struct nori_scene {
    std::unique_ptr<HostScene> hs;
};

constexpr int kMaxParts = 4;  // pool parts on separate streams (GPU_MAX_HW_QUEUES is 4)

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
    // serves a device query without a hit output), reused across calls; events around the two kernels
    DevBuf q_rays, q_hits, q_surf;
    hipEvent_t q_ev[3] = {};
    // the shading queries (nori_gpu_bsdf_eval ..): staging of up to three host input arrays and the output
    DevBuf sh_in[3], sh_out;
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
    std::vector<DevShape> hshapes;
    struct EmitterMesh {
        uint32_t shape, cdf_offset, vtx_first, vtx_count;  // the vertex range its triangles use
        std::vector<uint32_t> tri;                          // 3 global vertex ids per triangle
    };
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
        for (auto e : q_ev)
            if (e) (void)hipEventDestroy(e);
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

namespace {

int fail(int code, const std::string &m) {
    g_last_error = m;
    return code;
}

template <class F> int guarded(F &&f) {
    try {
        g_last_error.clear();
        return f();
    } catch (const NoriException &e) {
        return fail(e.code, e.what());
    } catch (const std::bad_alloc &) {
        return fail(NORI_ERR_OOM, "host allocation failed");
    } catch (const std::exception &e) {
        return fail(NORI_ERR_INVALID, e.what());
    }
}

// The traversal stack of a 4-wide tree of `depth` levels (nori_gpu_create and
// nori_gpu_rebuild_bvh): at most 3 entries per level; the first `stack` live
// in LDS, up to kTraceSpill more in private memory (an 8-wide tree, 256-B
// nodes with a 19-comparator child order, was measured 15 % slower on C3 in
// round 5: DESIGN_LOG.md).  LDS budget 16 words: measured best on the 22.7k
// and 524k triangle scenes -- occupancy beats a deeper LDS part; 32 only when
// the spill area could not cover the rest.  forced: NORI_BVH_STACK's 8, 16 or
// 32 (tuning), or 0.  Throws for a tree too deep for the stack.
int bvh_stack_for(uint32_t depth, int forced) {
    const uint32_t need = 3 * depth + 1;
    int stack = 32;
    if (need <= (uint32_t)stack_lds_entries(8)) stack = 8;
    else if (need <= (uint32_t)stack_lds_entries(16) + kTraceSpill) stack = 16;
    if (forced) stack = forced;
    if (need > (uint32_t)stack_lds_entries(stack) + kTraceSpill) throw NoriException(NORI_ERR_UNSUPPORTED, "BVH too deep for the traversal stack");
    return stack;
}

// Scene box = BVH root box: every mesh vertex and every sphere's bounds.
void scene_root_box(const nori_scene_desc &d, float rmin[3], float rmax[3]) {
    for (int k = 0; k < 3; ++k) rmin[k] = __builtin_inff(), rmax[k] = -__builtin_inff();
    auto expand = [&](float x, float y, float z) {
        float p[3] = {x, y, z};
        for (int k = 0; k < 3; ++k) {
            rmin[k] = std::fmin(rmin[k], p[k]);
            rmax[k] = std::fmax(rmax[k], p[k]);
        }
    };
    for (uint32_t s = 0; s < d.num_shapes; ++s) {
        const nori_shape_desc &sd = d.shapes[s];
        if (sd.type == NORI_SHAPE_SPHERE) {
            expand(sd.center[0] - sd.radius, sd.center[1] - sd.radius, sd.center[2] - sd.radius);
            expand(sd.center[0] + sd.radius, sd.center[1] + sd.radius, sd.center[2] + sd.radius);
        } else {
            for (uint32_t v = 0; v < sd.vtx_count; ++v) {
                const float *p = d.positions + 3 * (size_t)(sd.vtx_offset + v);
                expand(p[0], p[1], p[2]);
            }
        }
    }
}

// DevShape::solitary for every sphere: no other primitive comes within a
// margin of its closed ball and the ball lies inside the scene box (rmin,
// rmax) by that margin.  Closest point of a triangle to the centre: Ericson,
// Real-Time Collision Detection 5.1.5, in double precision.
double point_triangle_dist2(const double p[3], const float *a, const float *b, const float *c) {
    double ab[3], ac[3], ap[3];
    for (int k = 0; k < 3; ++k) ab[k] = (double)b[k] - a[k], ac[k] = (double)c[k] - a[k], ap[k] = p[k] - a[k];
    auto dot = [](const double *x, const double *y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; };
    auto dist2 = [&](const double q[3]) {
        double s = 0;
        for (int k = 0; k < 3; ++k) s += (p[k] - q[k]) * (p[k] - q[k]);
        return s;
    };
    double q[3];
    const double d1 = dot(ab, ap), d2 = dot(ac, ap);
    if (d1 <= 0 && d2 <= 0) { for (int k = 0; k < 3; ++k) q[k] = a[k]; return dist2(q); }
    double bp[3];
    for (int k = 0; k < 3; ++k) bp[k] = p[k] - b[k];
    const double d3 = dot(ab, bp), d4 = dot(ac, bp);
    if (d3 >= 0 && d4 <= d3) { for (int k = 0; k < 3; ++k) q[k] = b[k]; return dist2(q); }
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0 && d1 >= 0 && d3 <= 0) {
        const double v = d1 / (d1 - d3);
        for (int k = 0; k < 3; ++k) q[k] = a[k] + v * ab[k];
        return dist2(q);
    }
    double cp[3];
    for (int k = 0; k < 3; ++k) cp[k] = p[k] - c[k];
    const double d5 = dot(ab, cp), d6 = dot(ac, cp);
    if (d6 >= 0 && d5 <= d6) { for (int k = 0; k < 3; ++k) q[k] = c[k]; return dist2(q); }
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0 && d2 >= 0 && d6 <= 0) {
        const double w = d2 / (d2 - d6);
        for (int k = 0; k < 3; ++k) q[k] = a[k] + w * ac[k];
        return dist2(q);
    }
    const double va = d3 * d6 - d5 * d4;
    if (va <= 0 && (d4 - d3) >= 0 && (d5 - d6) >= 0) {
        const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        for (int k = 0; k < 3; ++k) q[k] = b[k] + w * ((double)c[k] - b[k]);
        return dist2(q);
    }
    const double den = 1.0 / (va + vb + vc), v = vb * den, w = vc * den;
    for (int k = 0; k < 3; ++k) q[k] = a[k] + ab[k] * v + ac[k] * w;
    return dist2(q);
}

void mark_solitary_spheres(const nori_scene_desc &d, const float rmin[3], const float rmax[3],
                           std::vector<DevShape> &shapes) {
    if (const char *e = std::getenv("NORI_CHORD"); e && e[0] == '0') return;  // A/B: full scans only
    for (uint32_t s = 0; s < d.num_shapes; ++s) {
        const nori_shape_desc &sp = d.shapes[s];
        if (sp.type != NORI_SHAPE_SPHERE || !(sp.radius > 0.0f)) continue;
        const double r = sp.radius, c[3] = {sp.center[0], sp.center[1], sp.center[2]};
        const double margin = 1e-4 * (std::max({std::fabs(c[0]), std::fabs(c[1]), std::fabs(c[2])}) + r);
        bool ok = true;
        for (int k = 0; k < 3 && ok; ++k) ok = c[k] - r > (double)rmin[k] + margin && c[k] + r < (double)rmax[k] - margin;
        const double reach = r + margin;
        for (uint32_t o = 0; o < d.num_shapes && ok; ++o) {
            if (o == s) continue;
            const nori_shape_desc &od = d.shapes[o];
            if (od.type == NORI_SHAPE_SPHERE) {
                double dd = 0;
                for (int k = 0; k < 3; ++k) dd += (c[k] - od.center[k]) * (c[k] - od.center[k]);
                ok = std::sqrt(dd) > reach + od.radius;
                continue;
            }
            for (uint32_t t = 0; t < od.tri_count && ok; ++t) {
                const uint32_t *f = d.indices + 3 * (size_t)(od.tri_offset + t);
                const float *p0 = d.positions + 3 * (size_t)f[0], *p1 = d.positions + 3 * (size_t)f[1],
                            *p2 = d.positions + 3 * (size_t)f[2];
                bool far = false;  // quick reject: the triangle's box misses the ball's box
                for (int k = 0; k < 3; ++k)
                    far = far || std::min({p0[k], p1[k], p2[k]}) > c[k] + reach || std::max({p0[k], p1[k], p2[k]}) < c[k] - reach;
                if (!far) ok = point_triangle_dist2(c, p0, p1, p2) > reach * reach;
            }
        }
        shapes[s].solitary = ok ? 1 : 0;
        if (std::getenv("NORI_DEBUG")) std::fprintf(stderr, "[nori] sphere shape %u: solitary %d\n", s, (int)ok);
    }
}

// The scan list of scan-mode scenes (scan.h scan_core).  Triangles that
// lie in an axis plane -- both edges with an exactly zero component on the
// same axis a, so every vertex has x_a = c -- come first, paired by plane:
// the kernels skip such a pair for a whole wave when no ray of the wave can
// hit it, a test that is exact only under the conditions checked here (no
// cancellation in the one remaining product difference of det and of t's
// numerator, scan.h plane_may_hit).  Pairs are ordered by axis (the
// kernels loop over each axis separately); a plane holding an odd number of
// triangles pads its last pair with a record no ray hits.  The remaining
// triangles follow, padded to kScanGroup, then the spheres.  Every record
// carries its leaf-order position in e2.w: among equal t the scan keeps the
// hit of the later leaf position, the reference's traversal order.
bool debug_log();
struct ScanList {
    std::vector<float> prims;   // 12 floats per record
    std::vector<float> plane_c; // per pair: the plane coordinate c
    std::vector<float> plane_f; // per pair: the in-plane filter of k_extend_bin (8 floats, plane_filters)
    uint32_t plane_end[3] = {0, 0, 0};  // pairs with axis <= a
    uint32_t tris = 0;          // triangle records (pairs + the rest, padded)
    uint32_t real = 0;          // ... of which the last real one ends here (the padding after it never hits)
};

// The in-plane filter of the binned extension kernel (scan.h
// pair_candidate): a ray can be accepted by the Moller-Trumbore test of a
// triangle of pair g only if its crossing with the pair's plane x_A = c lies
// within the pair's in-plane bounding rectangle widened by a margin M that
// covers every rounding error of the test.  Derivation (A the plane axis, B
// and C the other two, u = 2^-24, gamma_k = k u / (1 - k u)): with e1_A =
// e2_A = 0, the reference's u numerator tvec . (d x e2) divided by the exact
// det = -d_A n (n = e1_B e2_C - e1_C e2_B) is a sum of terms bounded by
// E (|o_B - v0_B| + |o_C - v0_C| + |t*| (|d_B| + |d_C|)) / |n| = E L / |n|
// (E the largest in-plane edge component, t* = (c - o_A) / d_A the exact
// crossing), each computed with at most 6 roundings, and det carries
// (2 kappa + 1) u (kappa <= 32, axis_plane); so the computed u and v differ
// from the exact barycentrics of the crossing by at most
// gamma_8 E L / |n| + gamma_(2 kappa + 6) each.  An accepted (u, v) lies in
// the triangle (u + v <= 1 up to one rounding), hence the exact crossing lies
// within 2 E (gamma_8 E L / |n| + gamma_(2 kappa + 6)) + 2^-23 E of the
// triangle's bounding box in B and C.  The kernel computes the crossing as
// t_f = (c - o_A) * (1 / d_A) (3 roundings of t*) and d_B = o_B + t_f d_B -
// mid_B, whose own error is below gamma_8 S + 2^-22 |mid_B| with
// S = |o_B| + |o_C| + |t_f| (|d_B| + |d_C|) >= L - V, V = |v0_B| + |v0_C|.
// Hence the test  |d_B| <= half_B + Ka S + Kb  (and the same in C) with
//     Ka = (2 gamma_8 E^2 / n_min + gamma_8) * 1.05
//     Kb = (2 gamma_8 E^2 / n_min * V + 2 E gamma_70 + 2^-23 E + 2^-22 |mid|) * 1.05
// never rejects an accepted ray (the factor 1.05 covers the roundings of the
// filter's own products).  Per pair: (mid_B, half_B + Kb, mid_C, half_C + Kb),
// (Ka, c, 0, 0).  A padding record (zero edges) never hits and is left out.
void plane_filters(ScanList &L) {
    const uint32_t npairs = (uint32_t)L.plane_c.size();
    L.plane_f.assign(8 * (size_t)npairs, 0.0f);
    const double u = std::ldexp(1.0, -24);
    auto gam = [&](double k) { return k * u / (1.0 - k * u); };
    auto up = [](double x) {  // the float >= x
        float f = (float)x;
        return (double)f < x ? std::nextafter(f, INFINITY) : f;
    };
    for (uint32_t g = 0; g < npairs; ++g) {
        const int A = g < L.plane_end[0] ? 0 : g < L.plane_end[1] ? 1 : 2, B = (A + 1) % 3, C = (A + 2) % 3;
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        double E = 0.0, nmin = INFINITY, V = 0.0;
        for (int k = 0; k < 2; ++k) {
            const float *r = &L.prims[12 * (size_t)(2 * g + k)];
            const float *v0 = r, *e1 = r + 4, *e2 = r + 8;
            const double n = std::fabs((double)e1[B] * e2[C] - (double)e1[C] * e2[B]);
            if (n == 0.0) continue;  // padding record
            for (int a : {B, C}) {
                for (double x : {(double)v0[a], (double)v0[a] + e1[a], (double)v0[a] + e2[a]}) {
                    lo[a] = std::min(lo[a], x);
                    hi[a] = std::max(hi[a], x);
                }
                E = std::max({E, std::fabs((double)e1[a]), std::fabs((double)e2[a])});
            }
            nmin = std::min(nmin, n);
            V = std::max(V, std::fabs((double)v0[B]) + std::fabs((double)v0[C]));
        }
        float *f = &L.plane_f[8 * (size_t)g];
        if (!(nmin < INFINITY)) {  // two padding records: an empty rectangle no ray passes
            f[0] = f[2] = 0.0f;
            f[1] = f[3] = -1.0f;
            f[5] = L.plane_c[g];
            continue;
        }
        const double K1 = 2.0 * gam(8) * E * E / nmin;
        const double Ka = (K1 + gam(8)) * 1.05;
        for (int k = 0; k < 2; ++k) {
            const int a = k ? C : B;
            const float mid = (float)(0.5 * (lo[a] + hi[a]));
            const double half = std::max(hi[a] - mid, mid - lo[a]);
            const double Kb = (K1 * V + 2.0 * E * gam(70) + std::ldexp(E, -23) + std::ldexp(std::fabs(mid), -22)) * 1.05;
            f[2 * k] = mid;
            f[2 * k + 1] = (float)up(up(half) + Kb);
        }
        f[4] = (float)up(Ka);
        f[5] = L.plane_c[g];
    }
}
bool axis_plane(const float *r, int a) {
    const float *e1 = r + 4, *e2 = r + 8;
    if (e1[a] != 0.0f || e2[a] != 0.0f) return false;
    const int b = (a + 1) % 3, c = (a + 2) % 3;
    for (int k : {b, c}) {  // products of normal range: nonzero components in [2^-60, 2^60]
        for (float x : {e1[k], e2[k]})
            if (x != 0.0f && !(std::fabs(x) >= 0x1p-60f && std::fabs(x) <= 0x1p60f)) return false;
    }
    // det and t's numerator are (ray component) x (P - Q) with P, Q the two
    // products below: kappa = (|P| + |Q|) / |P - Q| bounds their rounding
    const double P = (double)e1[b] * e2[c], Q = (double)e1[c] * e2[b];
    const double diff = std::fabs(P - Q);
    return diff > 0.0 && (std::fabs(P) + std::fabs(Q)) <= 32.0 * diff;
}
ScanList build_scan_list(const DeviceBvh &bvh, uint32_t n) {
    ScanList L;
    auto rec = [&](uint32_t i) { return &bvh.prims[12 * (size_t)i]; };
    auto sphere = [&](uint32_t i) {
        uint32_t f;
        std::memcpy(&f, rec(i) + 7, 4);
        return f != 0u;
    };
    auto add = [&](uint32_t i) {
        const float *r = rec(i);
        L.prims.insert(L.prims.end(), r, r + 12);
        std::memcpy(&L.prims[L.prims.size() - 1], &i, 4);  // e2.w = leaf-order position
    };
    auto add_null = [&] {
        float null_prim[12] = {0};  // zero edges: det = 0, never hit
        const uint32_t none = 0xFFFFFFFFu;
        std::memcpy(&null_prim[3], &none, 4);
        L.prims.insert(L.prims.end(), null_prim, null_prim + 12);
    };
    std::vector<int> axis(n, -1);
    for (uint32_t i = 0; i < n; ++i)
        if (!sphere(i))
            for (int a = 0; a < 3 && axis[i] < 0; ++a)
                if (axis_plane(rec(i), a)) axis[i] = a;
    for (int a = 0; a < 3; ++a) {
        // this axis's planes in order of first appearance (leaf order)
        std::vector<float> planes;
        for (uint32_t i = 0; i < n; ++i)
            if (axis[i] == a && std::find(planes.begin(), planes.end(), rec(i)[a]) == planes.end())
                planes.push_back(rec(i)[a]);
        for (float c : planes) {
            uint32_t in_pair = 0;
            for (uint32_t i = 0; i < n; ++i)
                if (axis[i] == a && rec(i)[a] == c) {
                    add(i);
                    if (++in_pair == 2) {
                        L.plane_c.push_back(c);
                        in_pair = 0;
                    }
                }
            if (in_pair) {
                add_null();
                L.plane_c.push_back(c);
            }
        }
        L.plane_end[a] = (uint32_t)L.plane_c.size();
    }
    L.tris = 2 * (uint32_t)L.plane_c.size();
    uint32_t rest = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (!sphere(i) && axis[i] < 0) add(i), ++rest;
    L.real = L.tris + rest;
    for (; rest % kScanGroup; ++rest) add_null();
    L.tris += rest;
    for (uint32_t i = 0; i < n; ++i)
        if (sphere(i)) add(i);
    plane_filters(L);
    if (const char *e = std::getenv("NORI_PLANE_CULL"); e && e[0] == '0') {  // A/B: no plane pairs
        ScanList F;
        for (uint32_t i = 0; i < n; ++i)
            if (!sphere(i)) {
                const float *r = rec(i);
                F.prims.insert(F.prims.end(), r, r + 12);
                std::memcpy(&F.prims[F.prims.size() - 1], &i, 4);
                ++F.tris;
            }
        F.real = F.tris;
        for (; F.tris % kScanGroup; ++F.tris) {
            float null_prim[12] = {0};
            const uint32_t none = 0xFFFFFFFFu;
            std::memcpy(&null_prim[3], &none, 4);
            F.prims.insert(F.prims.end(), null_prim, null_prim + 12);
        }
        for (uint32_t i = 0; i < n; ++i)
            if (sphere(i)) {
                const float *r = rec(i);
                F.prims.insert(F.prims.end(), r, r + 12);
                std::memcpy(&F.prims[F.prims.size() - 1], &i, 4);
            }
        return F;
    }
    if (debug_log())
        std::fprintf(stderr, "[nori] scan list: %zu axis-plane pairs (x %u, y %u, z %u), %u other triangle records\n",
                     L.plane_c.size(), L.plane_end[0], L.plane_end[1] - L.plane_end[0],
                     L.plane_end[2] - L.plane_end[1], rest);
    return L;
}

// The path kernels' lite variants (FULL = false) serve scenes made of the
// basic plugins only: constant-albedo diffuse, mirror and dielectric BSDFs,
// area lights, the perspective camera, no normal maps.  NORI_BASIC=0 forces
// the full variants (A/B).
bool basic_scene(const nori_scene_desc &d) {
    if (const char *e = std::getenv("NORI_BASIC"); e && e[0] == '0') return false;
    for (uint32_t i = 0; i < d.num_bsdfs; ++i) {
        const nori_bsdf_desc &b = d.bsdfs[i];
        if (b.type != NORI_BSDF_DIFFUSE && b.type != NORI_BSDF_MIRROR && b.type != NORI_BSDF_DIELECTRIC) return false;
        if (b.type == NORI_BSDF_DIFFUSE && b.albedo_texture != NORI_TEXTURE_CONSTANT) return false;
    }
    for (uint32_t i = 0; i < d.num_emitters; ++i)
        if (d.emitters[i].type != NORI_EMITTER_AREA) return false;
    for (uint32_t i = 0; i < d.num_shapes; ++i)
        if (d.shapes[i].normal_map >= 0) return false;
    return d.camera.camera_type == NORI_CAMERA_PERSPECTIVE;
}

// Mesh::activate's area DiscretePDF (mesh.cpp:30-38, dpdf.h:58-91) of a mesh
// whose triangle t has the vertices tri[3t .. 3t+2] of vtx(id): the serial
// fp32 running sum of the areas, times 1 / sum, last entry 1, in cdf (count + 1
// entries).  Returns DiscretePDF::getNormalization = 1 / sum, 0 for a mesh
// without area (its CDF stays unnormalised).  The one statement of both
// nori_gpu_create and nori_gpu_update_vertices.
template <class Vtx> float mesh_area_cdf(const uint32_t *tri, uint32_t count, Vtx vtx, std::vector<float> &cdf) {
    cdf.assign((size_t)count + 1, 0.0f);
    for (uint32_t t = 0; t < count; ++t) {
        const uint32_t *f = tri + 3 * (size_t)t;
        const float *p0 = vtx(f[0]), *p1 = vtx(f[1]), *p2 = vtx(f[2]);
        float e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
        float cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
        float area = 0.5f * std::sqrt((cx * cx + cy * cy) + cz * cz);
        cdf[t + 1] = cdf[t] + area;
    }
    const float sum = cdf[count];
    if (!(sum > 0)) return 0.0f;
    const float norm = 1.0f / sum;
    for (uint32_t t = 1; t <= count; ++t) cdf[t] *= norm;
    cdf[count] = 1.0f;
    return norm;
}

// The size of the small-scene blob upload_scene builds (its ten tables, each
// 16-byte aligned), from the description alone: nori_scene_shade_rtc chooses
// the shade kernel's LDS variant with it, without a device.
size_t scene_blob_bytes(const nori_scene_desc &d, size_t prim_floats, size_t node_floats) {
    size_t prims = 0, cdf = 0;
    for (uint32_t s = 0; s < d.num_shapes; ++s) {
        const bool mesh = d.shapes[s].type == NORI_SHAPE_MESH;
        prims += mesh ? d.shapes[s].tri_count : 1u;
        cdf += mesh ? (size_t)d.shapes[s].tri_count + 1 : 0u;
    }
    const size_t vtx = d.num_vertices ? d.num_vertices : 1u;
    const size_t parts[10] = {prim_floats * 4, prims * 12, vtx * 16, vtx * 16, prims * 4, d.num_shapes * sizeof(DevShape),
                              d.num_bsdfs * sizeof(DevBsdf), d.num_emitters * sizeof(DevEmitter), (cdf ? cdf : 1u) * 4,
                              node_floats * 4};
    size_t n = 0;
    for (size_t b : parts) n = (n + 15) / 16 * 16 + b;
    return (n + 15) / 16 * 16;
}
// Scenes whose k_shade can hold a scan, and so get a compilation of their own
// (rtc.hip): scan mode with a scan list the scan program takes, the basic
// plugin set, an integrator of the wavefront loop.
bool shade_rtc_scene(const nori_scene_desc &d, bool scan, size_t records) {
    return scan && records <= 2 * kScanMaxPrims && basic_scene(d) && d.integrator < NORI_INTEGRATOR_NORMALS;
}

void upload_scene(nori_gpu_ctx &c, const nori_scene_desc &d) {
    float rmin[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float rmax[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    auto expand = [&](float x, float y, float z) {
        float p[3] = {x, y, z};
        for (int k = 0; k < 3; ++k) {
            rmin[k] = std::fmin(rmin[k], p[k]);
            rmax[k] = std::fmax(rmax[k], p[k]);
        }
    };
    // image textures and normal maps: 8-bit RGB -> one RGBX word per texel, so
    // a lookup is one 4-byte load; DevBsdf/DevShape hold pointers into it
    std::vector<size_t> img_off(d.num_images);
    {
        std::vector<uint32_t> tex;
        for (uint32_t i = 0; i < d.num_images; ++i) {
            const nori_image_desc &im = d.images[i];
            if (!im.rgb || im.width <= 0 || im.height <= 0 || (im.wrap != NORI_WRAP_REPEAT && im.wrap != NORI_WRAP_CLAMP))
                throw NoriException(NORI_ERR_INVALID, "bad image description");
            img_off[i] = tex.size();
            const size_t n = (size_t)im.width * im.height;
            for (size_t t = 0; t < n; ++t)
                tex.push_back((uint32_t)im.rgb[3 * t] | ((uint32_t)im.rgb[3 * t + 1] << 8) | ((uint32_t)im.rgb[3 * t + 2] << 16));
        }
        if (tex.empty()) tex.assign(1, 0u);
        c.tex.upload(tex);
    }
    auto image_ptr = [&](int32_t i) -> const uint32_t * {
        if (i < 0) return nullptr;
        if ((uint32_t)i >= d.num_images) throw NoriException(NORI_ERR_INVALID, "image index out of range");
        return c.tex.as<uint32_t>() + img_off[i];
    };
    std::vector<DevShape> shapes(d.num_shapes);
    std::vector<uint32_t> prim_shape, tri_vidx;
    std::vector<float> cdf;
    std::vector<nori_gpu_ctx::EmitterMesh> emitter_meshes;
    uint32_t off = 0;
    for (uint32_t s = 0; s < d.num_shapes; ++s) {
        const nori_shape_desc &sd = d.shapes[s];
        DevShape &ds = shapes[s];
        std::memset(&ds, 0, sizeof(ds));
        ds.nmap = image_ptr(sd.normal_map);
        if (ds.nmap) {
            ds.nm_w = d.images[sd.normal_map].width;
            ds.nm_h = d.images[sd.normal_map].height;
            ds.nm_wrap = d.images[sd.normal_map].wrap;
        }
        ds.type = sd.type;
        ds.bsdf = sd.bsdf;
        ds.emitter = sd.emitter;
        ds.has_normals = sd.has_normals;
        ds.has_uvs = sd.has_uvs && d.uvs ? 1u : 0u;
        ds.prim_offset = off;
        for (int k = 0; k < 3; ++k) ds.center[k] = sd.center[k];
        ds.radius = sd.radius;
        if (sd.bsdf < 0 || (uint32_t)sd.bsdf >= d.num_bsdfs) throw NoriException(NORI_ERR_INVALID, "shape without a valid bsdf");
        if (sd.type == NORI_SHAPE_SPHERE) {
            ds.prim_count = 1;
            float inv = 1.f / sd.radius;  // sphere.cpp:99-104: pow(1/r, 2) * 1/(4 pi)
            ds.area_norm = (float)((double)inv * (double)inv * (double)(0.25f * 0.31830988618379067154f));
            prim_shape.push_back(s);
            tri_vidx.insert(tri_vidx.end(), {0u, 0u, 0u});
            expand(sd.center[0] - sd.radius, sd.center[1] - sd.radius, sd.center[2] - sd.radius);
            expand(sd.center[0] + sd.radius, sd.center[1] + sd.radius, sd.center[2] + sd.radius);
        } else if (sd.type == NORI_SHAPE_MESH) {
            if ((uint64_t)sd.tri_offset + sd.tri_count > d.num_triangles || (uint64_t)sd.vtx_offset + sd.vtx_count > d.num_vertices)
                throw NoriException(NORI_ERR_INVALID, "mesh range outside the scene arrays");
            ds.prim_count = sd.tri_count;
            ds.cdf_offset = (uint32_t)cdf.size();
            for (uint32_t t = 0; t < sd.tri_count; ++t) {
                const uint32_t *f = d.indices + 3 * (size_t)(sd.tri_offset + t);
                for (int k = 0; k < 3; ++k)
                    if (f[k] >= d.num_vertices) throw NoriException(NORI_ERR_INVALID, "vertex index out of range");
                prim_shape.push_back(s);
                tri_vidx.insert(tri_vidx.end(), {f[0], f[1], f[2]});
            }
            std::vector<float> mc;
            const uint32_t *tri = d.indices + 3 * (size_t)sd.tri_offset;
            ds.area_norm = mesh_area_cdf(tri, sd.tri_count, [&](uint32_t i) { return d.positions + 3 * (size_t)i; }, mc);
            cdf.insert(cdf.end(), mc.begin(), mc.end());
            if (sd.emitter >= 0 && sd.tri_count) {  // nori_gpu_update_vertices recomputes this mesh's CDF
                nori_gpu_ctx::EmitterMesh em;
                em.shape = s;
                em.cdf_offset = ds.cdf_offset;
                em.tri.assign(tri, tri + 3 * (size_t)sd.tri_count);
                const auto mm = std::minmax_element(em.tri.begin(), em.tri.end());
                em.vtx_first = *mm.first;
                em.vtx_count = *mm.second - *mm.first + 1;
                emitter_meshes.push_back(std::move(em));
            }
            for (uint32_t v = 0; v < sd.vtx_count; ++v) {
                const float *p = d.positions + 3 * (size_t)(sd.vtx_offset + v);
                expand(p[0], p[1], p[2]);
            }
        } else {
            throw NoriException(NORI_ERR_INVALID, "unknown shape type");
        }
        off += ds.prim_count;
    }
    c.num_prims = off;
    mark_solitary_spheres(d, rmin, rmax, shapes);
    std::vector<DevBsdf> bsdfs(d.num_bsdfs);
    for (uint32_t i = 0; i < d.num_bsdfs; ++i) {
        const nori_bsdf_desc &b = d.bsdfs[i];
        DevBsdf &o = bsdfs[i];
        dev_bsdf_from_desc(b, o);  // desc values and derived constants (bsdf_desc.h)
        if (b.albedo_texture == NORI_TEXTURE_IMAGE) {
            o.img = image_ptr(b.albedo_image);
            if (!o.img) throw NoriException(NORI_ERR_INVALID, "ImageTexture albedo without an image");
            o.img_w = d.images[b.albedo_image].width;
            o.img_h = d.images[b.albedo_image].height;
            o.img_wrap = d.images[b.albedo_image].wrap;
        } else if (b.albedo_texture != NORI_TEXTURE_CONSTANT && b.albedo_texture != NORI_TEXTURE_CHECKERBOARD) {
            throw NoriException(NORI_ERR_INVALID, "unknown albedo texture");
        }
        if (b.type < NORI_BSDF_DIFFUSE || b.type > NORI_BSDF_DISNEY) throw NoriException(NORI_ERR_INVALID, "unknown bsdf type");
    }
    std::vector<DevEmitter> emitters(d.num_emitters);
    std::vector<float> env;  // envmap tables of every envmap emitter
    for (uint32_t i = 0; i < d.num_emitters; ++i) {
        const nori_emitter_desc &e = d.emitters[i];
        if (e.type != NORI_EMITTER_AREA && e.type != NORI_EMITTER_ENVMAP && e.type != NORI_EMITTER_POINT &&
            e.type != NORI_EMITTER_SPOT)
            throw NoriException(NORI_ERR_UNSUPPORTED, "unknown emitter type");
        const bool free_standing = e.type == NORI_EMITTER_POINT || e.type == NORI_EMITTER_SPOT;
        if (!free_standing && (e.shape < 0 || (uint32_t)e.shape >= d.num_shapes))
            throw NoriException(NORI_ERR_INVALID, "emitter without a shape");
        std::memset(&emitters[i], 0, sizeof(DevEmitter));
        emitters[i].type = e.type;
        emitters[i].shape = free_standing ? -1 : e.shape;
        for (int k = 0; k < 3; ++k) {
            emitters[i].radiance[k] = e.radiance[k];
            emitters[i].position[k] = e.position[k];
            emitters[i].power[k] = e.power[k];
            emitters[i].direction[k] = e.direction[k];
        }
        emitters[i].cos_fs = e.cos_falloff_start;
        emitters[i].cos_tw = e.cos_total_width;
        if (e.type == NORI_EMITTER_ENVMAP) build_envmap(e, emitters[i], env);
    }
    if (d.integrator < NORI_INTEGRATOR_PATH_MATS || d.integrator > NORI_INTEGRATOR_PHOTONMAPPER)
        throw NoriException(NORI_ERR_UNSUPPORTED, "unknown integrator");
    if (d.num_emitters == 0 && d.integrator != NORI_INTEGRATOR_NORMALS && d.integrator != NORI_INTEGRATOR_AV)
        throw NoriException(NORI_ERR_INVALID, "the scene has no emitter");
    if (d.integrator == NORI_INTEGRATOR_PHOTONMAPPER) {
        if (d.photon_count == 0 || !(d.photon_radius > 0.0f) || !std::isfinite(d.photon_radius))
            throw NoriException(NORI_ERR_INVALID, "photonmapper: photon_count and photon_radius must be positive");
        for (uint32_t i = 0; i < d.num_emitters; ++i)  // Emitter::samplePhoton (emitter.h) throws for the others
            if (d.emitters[i].type != NORI_EMITTER_AREA)
                throw NoriException(NORI_ERR_UNSUPPORTED, "photonmapper: photons from area lights only");
    }
    if (d.camera.camera_type < NORI_CAMERA_PERSPECTIVE || d.camera.camera_type > NORI_CAMERA_ADVANCED)
        throw NoriException(NORI_ERR_UNSUPPORTED, "unknown camera type");
    // the reference leaves Scene::m_medium uninitialised without a <medium>
    // (scene.h:141): rejected here, as in the oracle
    if (d.integrator == NORI_INTEGRATOR_VOLUMETRIC && !d.medium.present)
        throw NoriException(NORI_ERR_INVALID, "the volumetric integrator needs a <medium>");

    // Traversal strategy: scenes of at most kScanMaxPrims primitives are
    // intersected by a wave-uniform scan (scalar loads, no divergence), larger
    // ones by per-lane BVH traversal.  NORI_TRAVERSAL=bvh|scan overrides.
    const char *mode = std::getenv("NORI_TRAVERSAL");
    bool scan = off <= kScanMaxPrims;
    if (mode && std::string(mode) == "bvh") scan = false;
    if (mode && std::string(mode) == "scan") scan = true;
    DeviceBvh bvh;
    build_device_bvh(d, rmin, rmax, bvh);
    c.bvh_depth = bvh.depth;
    c.bvh_nodes = bvh.num_nodes;
    // traversal stack (bvh_stack_for); NORI_BVH_STACK = 8, 16 or 32 forces it (tuning)
    if (const char *e = std::getenv("NORI_BVH_STACK")) {
        const int v = std::atoi(e);
        if (v == 8 || v == 16 || v == 32) c.stack_forced = v;
    }
    c.stack = bvh_stack_for(bvh.depth, c.stack_forced);
    if (scan) c.stack = 0;
    ScanList scan_list;
    if (scan) scan_list = build_scan_list(bvh, off);
    const std::vector<float> &prim_list = scan ? scan_list.prims : bvh.prims;

    std::vector<float> pos(4 * (size_t)d.num_vertices), nrm(4 * (size_t)d.num_vertices);
    for (uint32_t v = 0; v < d.num_vertices; ++v) {
        for (int k = 0; k < 3; ++k) {
            pos[4 * (size_t)v + k] = d.positions[3 * (size_t)v + k];
            nrm[4 * (size_t)v + k] = d.normals ? d.normals[3 * (size_t)v + k] : 0.0f;
        }
        // texture coordinates ride in the w lanes (u with the position, v with the normal)
        pos[4 * (size_t)v + 3] = d.uvs ? d.uvs[2 * (size_t)v] : 0.0f;
        nrm[4 * (size_t)v + 3] = d.uvs ? d.uvs[2 * (size_t)v + 1] : 0.0f;
    }
    if (pos.empty()) pos.assign(4, 0.0f), nrm.assign(4, 0.0f);
    if (cdf.empty()) cdf.assign(1, 0.0f);
    c.nodes.upload(bvh.nodes);
    c.prims.upload(prim_list);
    if (!scan_list.plane_c.empty()) c.plane_c.upload(scan_list.plane_c);
    if (!scan_list.plane_f.empty()) c.plane_f.upload(scan_list.plane_f);
    c.tri_vidx.upload(tri_vidx);
    c.pos.upload(pos);
    c.nrm.upload(nrm);
    c.prim_shape.upload(prim_shape);
    c.shapes.upload(shapes);
    c.bsdfs.upload(bsdfs);
    c.emitters.upload(emitters);
    c.cdf.upload(cdf);
    if (env.empty()) env.assign(4, 0.0f);
    c.env.upload(env);
    c.scene_bytes = c.nodes.bytes + c.prims.bytes;
    // nori_gpu_update_vertices (BVH contexts): the order in which a refit recomputes the boxes
    c.hshapes = shapes;
    c.emitter_meshes = std::move(emitter_meshes);
    c.num_vertices = d.num_vertices;
    if (!scan) {
        c.refit = build_refit_plan(bvh);
        c.refit_slots.upload(c.refit.slots);
    }
    // small-scene blob (staged into LDS by the tail finisher)
    std::vector<char> blob;
    uint32_t offs[10] = {0};
    auto put = [&](int k, const void *p, size_t n) {
        while (blob.size() % 16) blob.push_back(0);
        offs[k] = (uint32_t)blob.size();
        const char *b = static_cast<const char *>(p);
        blob.insert(blob.end(), b, b + n);
    };
    put(0, prim_list.data(), prim_list.size() * 4);
    put(1, tri_vidx.data(), tri_vidx.size() * 4);
    put(2, pos.data(), pos.size() * 4);
    put(3, nrm.data(), nrm.size() * 4);
    put(4, prim_shape.data(), prim_shape.size() * 4);
    put(5, shapes.data(), shapes.size() * sizeof(DevShape));
    put(6, bsdfs.data(), bsdfs.size() * sizeof(DevBsdf));
    put(7, emitters.data(), emitters.size() * sizeof(DevEmitter));
    put(8, cdf.data(), cdf.size() * 4);
    put(9, bvh.nodes.data(), bvh.nodes.size() * 4);
    while (blob.size() % 16) blob.push_back(0);
    const bool use_blob = c.stack == 0 && blob.size() <= kBlobMaxBytes;
    if (use_blob) c.blob.upload(blob);

    DevScene &S = c.S;
    S.nodes = c.nodes.as<float4>();
    S.prims = c.prims.as<float4>();
    S.tri_vidx = c.tri_vidx.as<uint32_t>();
    S.pos = c.pos.as<float4>();
    S.nrm = c.nrm.as<float4>();
    S.prim_shape = c.prim_shape.as<uint32_t>();
    S.shapes = c.shapes.as<DevShape>();
    S.bsdfs = c.bsdfs.as<DevBsdf>();
    S.emitters = c.emitters.as<DevEmitter>();
    S.cdf = c.cdf.as<float>();
    S.env = c.env.as<float>();
    S.num_emitters = d.num_emitters;
    S.num_nodes = bvh.num_nodes;
    S.num_prims = (uint32_t)(prim_list.size() / 12);
    S.num_scan_tris = scan_list.tris;
    S.num_scan_real = scan_list.real;
    S.plane_c = scan_list.plane_c.empty() ? nullptr : c.plane_c.as<float>();
    S.plane_f = scan_list.plane_f.empty() ? nullptr : c.plane_f.as<float4>();
    for (int a = 0; a < 3; ++a) S.plane_end[a] = scan_list.plane_end[a];
    {
        const char *e = std::getenv("NORI_CAMERA_CULL");  // A/B and verification: 0 = no in-plane filter
        S.camera_cull = !(e && e[0] == '0');
        const char *t = std::getenv("NORI_TRACE_CULL");  // trace API: 0, 1 (default) or 2 (needs plane pairs)
        S.trace_cull = t ? std::atoi(t) : 1;
        if (S.trace_cull < 0 || S.trace_cull > 2 || (S.trace_cull == 2 && !S.plane_f)) S.trace_cull = 1;
    }
    if (scan && scan_list.prims.size() / 12 <= 2 * kScanMaxPrims) {  // the scan kernels compiled for this scene's scan list (rtc.hip); else the generic ones
        ScanRtcScene sc{scan_list.prims.data(), (uint32_t)(scan_list.prims.size() / 12), scan_list.plane_c.data(),
                        scan_list.plane_f.data(), (uint32_t)scan_list.plane_c.size(),
                        {scan_list.plane_end[0], scan_list.plane_end[1], scan_list.plane_end[2]}, scan_list.tris,
                        scan_list.real};
        std::string why;
        if (!scan_rtc_build(sc, c.device, S.trace_cull, c.rtc, why) && debug_log())
            std::fprintf(stderr, "[nori] generic scan kernels: %s\n", why.c_str());
    }
    for (int k = 0; k < 3; ++k) S.root_min[k] = rmin[k], S.root_max[k] = rmax[k];
    S.blob = use_blob ? c.blob.as<float4>() : nullptr;
    S.blob_bytes = use_blob ? (uint32_t)blob.size() : 0u;
    S.off_prims = offs[0];
    S.off_vidx = offs[1];
    S.off_pos = offs[2];
    S.off_nrm = offs[3];
    S.off_pshape = offs[4];
    S.off_shapes = offs[5];
    S.off_bsdfs = offs[6];
    S.off_emitters = offs[7];
    S.off_cdf = offs[8];
    S.off_nodes = offs[9];
    const nori_camera_desc &cam = d.camera;
    c.cam = cam;
    if (cam.width <= 0 || cam.height <= 0) throw NoriException(NORI_ERR_INVALID, "bad output size");
    S.W = cam.width;
    S.H = cam.height;
    S.invW = 1.0f / (float)cam.width;
    S.invH = 1.0f / (float)cam.height;
    std::memcpy(S.s2c, cam.sample_to_camera, sizeof(S.s2c));
    std::memcpy(S.c2w, cam.camera_to_world, sizeof(S.c2w));
    {  // perspective.cpp:104: Eigen's (c2w * (0,0,0,1)).hnormalized(), column order
        const float *c = S.c2w;
        const float w = ((c[12] * 0.0f + c[13] * 0.0f) + c[14] * 0.0f) + c[15];
        S.cam_o[0] = (((c[0] * 0.0f + c[1] * 0.0f) + c[2] * 0.0f) + c[3]) / w;
        S.cam_o[1] = (((c[4] * 0.0f + c[5] * 0.0f) + c[6] * 0.0f) + c[7]) / w;
        S.cam_o[2] = (((c[8] * 0.0f + c[9] * 0.0f) + c[10] * 0.0f) + c[11]) / w;
    }
    S.near_clip = cam.near_clip;
    S.far_clip = cam.far_clip;
    S.cam_type = cam.camera_type;
    S.lens_radius = cam.lens_radius;
    S.focal = cam.focal_distance;
    S.distortion[0] = cam.distortion[0];
    S.distortion[1] = cam.distortion[1];
    for (int k = 0; k < 3; ++k) S.chromatic[k] = cam.camera_type == NORI_CAMERA_ADVANCED ? cam.chromatic[k] : 0.0f;
    S.chroma = S.chromatic[0] != 0.0f || S.chromatic[1] != 0.0f || S.chromatic[2] != 0.0f;
    S.basic = basic_scene(d) ? 1 : 0;
    {
        // shadow rays traced inside k_shade (scan-mode scenes): on by default
        // for the basic-plugin kernels (C2 +3-7 %, its 64-spp share +3 %), off
        // for the full ones (C4 -5.7 %, C5 -4.3 %: the full k_shade holds 90-96
        // VGPRs, and the queue's shadow kernel is the scene-specialised one).
        // NORI_NEE_INLINE=0 / 1 forces it off / on for scan-mode scenes whose
        // shade kernel carries it (the basic ones; kernels.h kNeeFull).
        const char *n = std::getenv("NORI_NEE_INLINE");
        S.nee_inline = c.stack == 0 && (n ? n[0] == '1' : S.basic != 0) && (S.basic != 0 || kNeeFull);
        // ... and each vertex's extension ray (k_shade's closest-hit scan in
        // place of the extension launch and the hit's round trip through
        // memory): scan-mode scenes with the basic plugins and the inline
        // shadow rays.  NORI_EXT_INLINE=0 / 1 forces it off / on there.
        const char *x = std::getenv("NORI_EXT_INLINE");
        S.ext_inline = c.stack == 0 && S.basic != 0 && S.nee_inline != 0 && (x ? x[0] == '1' : true);
    }
    {
        // one launch for an iteration's extension and shadow queues: on for
        // the BVH walks (C3 +10 %) and the basic scan kernels that keep the
        // queue; the full-plugin scan scenes run faster with two launches
        // (C4 3942 -> 3957, C5 4217 -> 4288 Msamples/s, 3 interleaved reps,
        // tools/gpu_fuse_ab.sh).  NORI_TRACE_FUSE=0 / 1 forces it.
        const char *f = std::getenv("NORI_TRACE_FUSE");
        c.fuse_trace = f ? f[0] != '0' : !(c.stack == 0 && S.basic == 0);
    }
    S.W_max = cam.width > cam.height ? cam.width : cam.height;
    S.av_length = d.av_length;
    filter_table(cam, S.filter);
    S.filter_radius = cam.filter_radius;
    S.lookup = NORI_FILTER_RESOLUTION / cam.filter_radius;
    S.border = film_border(cam);
    if (S.border > 4) throw NoriException(NORI_ERR_UNSUPPORTED, "filter radius above 4.5 pixels");
    S.jit_lk = jit_code_lookup(S.filter_radius, S.lookup);
    S.integrator = d.integrator;
    if (shade_rtc_scene(d, scan, scan_list.prims.size() / 12)) {  // k_shade compiled for this scene (after the scan program)
        ScanRtcScene sc{scan_list.prims.data(), (uint32_t)(scan_list.prims.size() / 12), scan_list.plane_c.data(),
                        scan_list.plane_f.data(), (uint32_t)scan_list.plane_c.size(),
                        {scan_list.plane_end[0], scan_list.plane_end[1], scan_list.plane_end[2]}, scan_list.tris,
                        scan_list.real};
        std::string why;
        if (!shade_rtc_build(sc, c.device, shade_integrator(S.integrator), shade_lds_bytes(S.blob_bytes) != 0,
                             c.shade_rtc, why) && debug_log())
            std::fprintf(stderr, "[nori] ahead-of-time shade kernel: %s\n", why.c_str());
        if (debug_log() && scene_blob_bytes(d, prim_list.size(), bvh.nodes.size()) != blob.size())
            std::fprintf(stderr, "[nori] scene_blob_bytes %zu != blob %zu\n",
                         scene_blob_bytes(d, prim_list.size(), bvh.nodes.size()), blob.size());
    }
    {  // deviation D10 (shading.h skip_nee); NORI_DISCRETE_NEE=1 keeps the full NEE everywhere
        bool env = false;
        for (uint32_t i = 0; i < d.num_emitters; ++i) env = env || d.emitters[i].type == NORI_EMITTER_ENVMAP;
        const char *e = std::getenv("NORI_DISCRETE_NEE");
        S.skip_discrete_nee = !env && !(e && e[0] == '1');
    }
    S.has_medium = d.medium.present;
    if (S.has_medium) {  // medium.cpp:10-20
        const nori_medium_desc &m = d.medium;
        for (int k = 0; k < 3; ++k) {
            S.mbox_min[k] = m.box_min[k];
            S.mbox_max[k] = m.box_max[k];
            S.sigma_t[k] = m.sigma_a[k] + m.sigma_s[k];
            S.albedo[k] = m.sigma_s[k] / S.sigma_t[k];
        }
    }
}

void ensure_pool(nori_gpu_ctx &c, uint32_t pool) {
    if (pool <= c.pool_cap) return;
    for (int b = 0; b < 2; ++b) {
        c.q[b][0].ensure(16 * (size_t)pool);
        c.q[b][1].ensure(16 * (size_t)pool);
        c.q[b][2].ensure(16 * (size_t)pool);
        c.q[b][3].ensure(16 * (size_t)pool);
        c.q[b][4].ensure(4 * (size_t)pool);
    }
    for (int k = 0; k < 3; ++k) c.sq[k].ensure(16 * (size_t)pool);
    for (int k = 0; k < 4; ++k) c.seg[k].ensure(4 * (size_t)(pool / kSeg));
    c.segstats.ensure(16 * (size_t)(pool / kSeg));
    c.tailpre.ensure(4 * (size_t)(pool / kSeg + 1));
    c.pool_cap = pool;
}

PathQueue queue_of(nori_gpu_ctx &c, int b) {
    PathQueue q;
    q.ray_o = c.q[b][0].as<float4>();
    q.ray_d = c.q[b][1].as<float4>();
    q.hit = c.q[b][2].as<float4>();
    q.thr = c.q[b][3].as<float4>();
    q.rng = c.q[b][4].as<uint32_t>();
    return q;
}

constexpr int kRing = 16;     // readback ring entries
constexpr int kLookahead = 6;    // iterations queued ahead of the termination check
constexpr int kLookaheadEnd = 2; // ... once work streams run dry
// NORI_LOOKAHEAD=n (0 .. 8) replaces kLookahead.  The termination check reads
// the done flag as the device has set it by now, which may be up to `lag`
// iterations further than the event just waited for: how many iterations a
// render launches past the one that handed out the last work id (and so how
// its rays divide between the loop and the finisher) depends on how far the
// host runs ahead of the device.  With 0 the host waits for every iteration
// before it reads the flag, and the counts are the same in every run (the
// tests that compare two renders' statistics exactly use it).
int lookahead() {
    const char *e = std::getenv("NORI_LOOKAHEAD");
    const int v = e ? std::atoi(e) : kLookahead;
    return v < 0 ? 0 : v > 8 ? 8 : v;
}

struct Timers {
    std::vector<hipEvent_t> ev;
    size_t used = 0;
    hipEvent_t get() {
        if (used == ev.size()) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e));
            ev.push_back(e);
        }
        return ev[used++];
    }
    ~Timers() {
        for (auto e : ev) (void)hipEventDestroy(e);
    }
};

bool debug_log() {
    const char *e = std::getenv("NORI_DEBUG");
    return e && e[0] == '1';
}
// NORI_POOL_PARTS: independent pool parts on their own streams (1..kMaxParts).
// Default 3: each part's launches wait for their own slowest walks / longest
// lanes, and three streams keep the chip busy in between (C3: 2 parts 619,
// 3 parts 651, 4 parts 499 Msamples/s -- 4 streams exceed the hardware
// queues; table scene 517 -> 555; C2 4563 -> 4658; 64-spp share 3026 ->
// 3089; C4 and C5 within 1 %).
// Renders whose shade kernel traces its own extension rays (ext_loop): 2.
// An iteration is one launch there, so no part's scan is left to slip under
// another part's shade launch (C2, 1M pool: 2 parts 6529-6637 Msamples/s;
// 2M pool: 1 part 5579-5615, 2 parts 6404-6460, 3 parts 6311-6410).
uint32_t pool_parts(bool ext_loop) {
    const uint32_t def = ext_loop ? 2u : 3u;
    const char *e = std::getenv("NORI_POOL_PARTS");
    const long v = e ? std::atol(e) : (long)def;
    return (uint32_t)(v >= 1 && v <= kMaxParts ? v : def);
}
// Sample passes folded by one splat work-group.  Default: about one
// work-group per CU over the whole launch (passes x blocks / 256), so the
// splat leaves most of the chip to the tail finisher it overlaps with
// (cbox 512x512@512: 256 blocks x 512 passes per work-group, splat 3.0 ms and
// finisher 3.6 ms vs 4.7 / 5.2 ms at 32 passes).  NORI_SPLAT_PASSES overrides.
// The one-bounce integrators' splat has no finisher beside it: it targets
// 4096 work-groups instead.
uint32_t splat_passes(uint32_t np, size_t nblocks, uint32_t target_wgs = 256) {
    const char *e = std::getenv("NORI_SPLAT_PASSES");
    long v = e ? std::atol(e) : (long)(((uint64_t)np * nblocks + target_wgs - 1) / target_wgs);
    if (v < 1) v = 1;
    return (uint32_t)std::min<long>(v, np);
}
// Per-pixel sample statistics (render_desc.variance_out): the device buffer
// the kernels add into -- the caller's own when it is device memory, else a
// zeroed scratch buffer that var_finish adds into the host array.
float *var_begin(nori_gpu_ctx &c, const nori_gpu_render_desc &rd) {
    if (!rd.variance_out) return nullptr;
    if (rd.output_on_device) return rd.variance_out;
    const size_t n = 8 * (size_t)c.S.W * (size_t)c.S.H;
    c.varbuf.ensure(n * sizeof(float));
    HIP_TRY(hipMemsetAsync(c.varbuf.p, 0, n * sizeof(float), c.stream));
    return c.varbuf.as<float>();
}
void var_finish(nori_gpu_ctx &c, const nori_gpu_render_desc &rd, bool cancelled) {
    if (!rd.variance_out || rd.output_on_device || cancelled) return;
    const size_t n = 8 * (size_t)c.S.W * (size_t)c.S.H;
    std::vector<float> h(n);
    HIP_TRY(hipMemcpy(h.data(), c.varbuf.p, n * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) rd.variance_out[i] += h[i];
}

// PhotonMapper::preprocess (photonmapper.cpp:41-117): photons are traced on
// the device in emission order batches (k_photons count pass) until the
// stored count reaches photonCount, then the emitted photons that contribute
// are traced again writing their photons (store pass), and the host stores
// them as the reference's PhotonData and builds the hash grid.
void photon_preprocess(nori_gpu_ctx &c, const nori_scene_desc &d) {
    const uint64_t N = d.photon_count;
    const uint32_t batch = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(N, 1u << 20), 1u << 24);
    DevBuf cnt;
    cnt.ensure(4 * (size_t)batch);
    std::vector<uint32_t> hc(batch);
    std::vector<uint64_t> pre;  // photons stored before each emitted photon
    uint64_t total = 0, e0 = 0;
    while (total < N) {
        if (e0 >= 64 * N + batch)  // the reference would loop forever
            throw NoriException(NORI_ERR_INVALID, "photonmapper: photons do not reach a diffuse surface");
        HIP_TRY(launch_photons(c.S, e0, batch, cnt.as<uint32_t>(), nullptr, 0, nullptr, c.stack, c.stream));
        HIP_TRY(hipMemcpyAsync(hc.data(), cnt.p, 4 * (size_t)batch, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
        for (uint32_t i = 0; i < batch && total < N; ++i) {
            pre.push_back(total);
            total += hc[i];
        }
        e0 += batch;
    }
    DevBuf dpre, out;
    dpre.upload(pre);
    out.ensure(48 * (size_t)N);
    // all-ones (NaN) first: a slot the store pass leaves unwritten keeps a NaN
    // in its zero pad word and is caught below instead of entering the map
    HIP_TRY(hipMemsetAsync(out.p, 0xFF, 48 * (size_t)N, c.stream));
    HIP_TRY(launch_photons(c.S, 0, (uint32_t)pre.size(), nullptr, dpre.as<uint64_t>(), N, out.as<float4>(), c.stack,
                           c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    std::vector<float> raw(12 * (size_t)N), ph, tab;
    HIP_TRY(hipMemcpy(raw.data(), out.p, 48 * (size_t)N, hipMemcpyDeviceToHost));
    // the store pass must reproduce the count pass photon for photon
    // (position, 0, direction, 0, power, 0 per slot)
    for (size_t i = 0; i < (size_t)N; ++i)
        if (!(raw[12 * i + 3] == 0.0f && raw[12 * i + 7] == 0.0f && raw[12 * i + 11] == 0.0f))
            throw NoriException(NORI_ERR_INVALID, "photonmapper: the store pass left photon slot " + std::to_string(i) +
                                                      " unwritten (count and store passes disagree)");
    std::vector<uint32_t> start, rgbe;
    uint32_t mask = 0;
    build_photon_map(raw, (uint32_t)N, d.photon_radius, ph, rgbe, tab, start, mask);
    c.ph.upload(ph);
    c.ph_rgbe.upload(rgbe);
    c.ph_tab.upload(tab);
    c.ph_start.upload(start);
    c.S.ph_rgbe = c.ph_rgbe.as<uint32_t>();
    c.S.ph_tab = c.ph_tab.as<float>();
    const float r = d.photon_radius;
    c.S.ph = c.ph.as<float4>();
    c.S.ph_start = c.ph_start.as<uint32_t>();
    c.S.ph_mask = mask;
    c.S.ph_inv_cell = 1.0f / r;
    c.S.ph_r2 = r * r;                                 // kdtree.h:266
    c.S.ph_norm = (r * r) * (float)d.photon_count;     // photonmapper.cpp:177
}

// normals / av / direct*: no path pool -- per chunk of passes, k_direct runs
// every sample start to end and writes its record, then k_splat filters them.
int render_one_bounce(nori_gpu_ctx &c, const nori_gpu_render_desc &rd, const std::vector<uint32_t> &pixels,
                      const std::vector<int4> &blocks, float *rgbw_out, nori_gpu_stats *stats,
                      std::chrono::steady_clock::time_point t0) {
    const DevScene &S = c.S;
    const int W = S.W, H = S.H, B = S.border;
    const uint32_t M = (uint32_t)pixels.size(), passes = rd.pass_count;
    const size_t rec_budget = (size_t)4 << 30;
    uint32_t chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(passes, rec_budget / (16 * (size_t)M)));
    // work ids (record indices) < 2^29: the path queue keeps a chromatic
    // sample's colour channel in bits 29-30 of the same word (kWorkMask)
    chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(chunk, ((uint64_t)1 << kChanShift) / M));
    c.rec.ensure(16 * (size_t)chunk * M);
    c.counters.ensure(sizeof(Counters));
    const size_t film_elems = 4 * (size_t)(W + 2 * B) * (H + 2 * B);
    float *film = nullptr;
    if (rd.output_on_device) {
        film = rgbw_out;
    } else {
        c.film.ensure(film_elems * sizeof(float));
        film = c.film.as<float>();
        HIP_TRY(hipMemsetAsync(film, 0, film_elems * sizeof(float), c.stream));
    }
    Counters *C = c.counters.as<Counters>();
    HIP_TRY(hipMemsetAsync(C, 0, sizeof(Counters), c.stream));
    if (!c.in_rounds) c.cancel = 0;
    c.report(0.0);
    Timers tm;
    const bool timing = rd.timing != 0;
    double kms[2] = {0, 0};
    std::vector<std::array<hipEvent_t, 3>> spans;
    uint64_t done = 0;
    bool cancelled = false;
    float *var = var_begin(c, rd);
    for (uint32_t p0 = 0; p0 < passes; p0 += chunk) {
        if (c.cancel.load()) {
            cancelled = true;
            break;
        }
        const uint32_t np = std::min(chunk, passes - p0);
        WorkDesc wd{(uint64_t)np * M, M, rd.pass_begin + p0, c.pixels.as<uint32_t>(), rd.seed, 0, nullptr, 1, 0, var};
        SplatDesc sd{M, np, rd.pass_begin + p0, std::max<uint32_t>(1, splat_passes(np, blocks.size(), 4096)), c.blocks.as<int4>(),
                     rd.seed, var};
        std::array<hipEvent_t, 3> ev{};
        if (timing) {
            for (auto &e : ev) e = tm.get();
            HIP_TRY(hipEventRecord(ev[0], c.stream));
        }
        HIP_TRY(launch_direct(S, wd, c.rec.as<float4>(), C, c.stack, c.stream));
        if (timing) HIP_TRY(hipEventRecord(ev[1], c.stream));
        HIP_TRY(launch_splat(S, c.rec.as<float4>(), sd, (uint32_t)blocks.size(), film, C, c.stream));
        if (timing) {
            HIP_TRY(hipEventRecord(ev[2], c.stream));
            spans.push_back(ev);
        }
        HIP_TRY(hipStreamSynchronize(c.stream));
        done += wd.total;
        c.report((double)(p0 + np) / passes);
    }
    Counters hc;
    HIP_TRY(hipMemcpyAsync(&hc, C, sizeof(Counters), hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    for (const auto &e : spans) {
        float a = 0, b = 0;
        HIP_TRY(hipEventElapsedTime(&a, e[0], e[1]));
        HIP_TRY(hipEventElapsedTime(&b, e[1], e[2]));
        kms[0] += a;
        kms[1] += b;
    }
    if (!rd.output_on_device && !cancelled) {
        std::vector<float> hf(film_elems);
        HIP_TRY(hipMemcpy(hf.data(), film, film_elems * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < film_elems; ++i) rgbw_out[i] += hf[i];
    }
    var_finish(c, rd, cancelled);
    c.report(1.0);
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->samples = done;
        stats->invalid_samples = hc.invalid;
        stats->rays_closest = hc.direct_rays[0];
        stats->rays_shadow = hc.direct_rays[1];
        stats->iterations = 0;
        stats->scene_bytes = c.scene_bytes;
        stats->bvh_nodes = c.bvh_nodes;
        stats->bvh_depth = c.bvh_depth;
        stats->stream_parts = 1;
        stats->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        stats->ms_shade = kms[0];  // k_direct: the whole integrator
        stats->ms_splat = kms[1];
        stats->scan_rtc = c.rtc.extend ? 1u : 0u;  // (held for the trace API; k_direct scans generically)
        stats->scan_rtc_cached = c.rtc.cached ? 1u : 0u;
        stats->ms_scan_rtc = c.rtc.compile_ms;
    }
    if (cancelled) return fail(NORI_ERR_CANCELLED, "rendering was cancelled");
    return NORI_OK;
}

// The render's blocks in BlockGenerator order (block.cpp:140-188) with the
// block_subset applied, and the block-major pixel list (camera samples of one
// block are adjacent work ids); cached on the context with their device
// copies, so a render of the same selection neither rebuilds nor uploads them.
static void work_lists(nori_gpu_ctx &c, const nori_gpu_render_desc &rd) {
    const int W = c.S.W, H = c.S.H;
    const int nbx = (int)std::ceil(W / (float)NORI_BLOCK_SIZE), nby = (int)std::ceil(H / (float)NORI_BLOCK_SIZE);
    std::vector<uint32_t> order = spiral_blocks(W, H);
    if (rd.num_blocks) {
        std::vector<char> want((size_t)nbx * nby, 0);
        for (uint32_t i = 0; i < rd.num_blocks; ++i) {
            if (rd.block_ids[i] >= (uint32_t)(nbx * nby)) throw NoriException(NORI_ERR_INVALID, "block id out of range");
            want[rd.block_ids[i]] = 1;
        }
        std::vector<uint32_t> sel;
        for (uint32_t b : order)
            if (want[b]) sel.push_back(b);
        order.swap(sel);
    }
    if (c.work_valid && order == c.work_order) return;
    c.work_valid = false;
    c.hpixels.clear();
    c.hblocks.clear();
    for (uint32_t b : order) {
        int bx = (int)(b % (uint32_t)nbx), by = (int)(b / (uint32_t)nbx);
        int ox = bx * NORI_BLOCK_SIZE, oy = by * NORI_BLOCK_SIZE;
        int bw = std::min(NORI_BLOCK_SIZE, W - ox), bh = std::min(NORI_BLOCK_SIZE, H - oy);
        c.hblocks.push_back(make_int4(ox, oy, bw | (bh << 16), (int)c.hpixels.size()));
        for (int y = 0; y < bh; ++y)
            for (int x = 0; x < bw; ++x) c.hpixels.push_back((uint32_t)((oy + y) * W + (ox + x)));
    }
    c.pixels.upload(c.hpixels);
    c.blocks.upload(c.hblocks);
    c.work_order.swap(order);
    c.work_valid = true;
}

int render(nori_gpu_ctx &c, const nori_gpu_render_desc &rd, float *rgbw_out, nori_gpu_stats *stats) {
    auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(c.device));
    const DevScene &S = c.S;
    const int W = S.W, H = S.H, B = S.border;
    work_lists(c, rd);
    const std::vector<uint32_t> &pixels = c.hpixels;
    const std::vector<int4> &blocks = c.hblocks;
    const uint32_t M = (uint32_t)pixels.size();
    const uint32_t passes = rd.pass_count ? rd.pass_count : 0;
    if (passes == 0 || M == 0) throw NoriException(NORI_ERR_INVALID, "nothing to render (pass_count or blocks empty)");
    const bool one_bounce = S.integrator >= NORI_INTEGRATOR_NORMALS;
    // default pool: about 1/16 of the render's samples in flight, between
    // 1M and 4M paths (~0.9 GB of queues at 4M).  Large pools hide the shade
    // kernel's memory latency (4M measured best among 256K..4M on cbox at 512
    // spp); small renders -- the per-GPU share of a strong-scaled frame --
    // spend less time draining a smaller pool (round 2, two parts, cbox 64
    // spp: 4M 2190, 2M 2320, 1M 2400 Msamples/s; 512 spp: 4M and 2M within
    // 1 %).  With three parts (round 3) the 64-spp share peaks at 1.25-1.5M
    // (512K 2560, 1M 3030-3160, 1.25M 3320, 1.5M 3275-3296, 2M 3192, 3M 2952)
    // and the 128-spp share at 2M (3989 against 3875 at 2.5M, 3773 at 3M).
    // Since k_shade traces the shadow rays itself (round 6, nee_inline) the
    // 64-spp share peaks at 1M again (4875 against 4702 at 1.5M, 4734 at
    // 1.25M, 4555 at 768K; 3 reps), so the floor is 1M.  The BVH walks
    // (C3) want about 1/8 in flight: 4M 846-851 against 807-812 at 2M
    // (3M 796-798, 6M 796-798, 8M 839-846; 3 interleaved reps).
    // Renders whose shade kernel traces its own extension rays (ext_loop)
    // keep the 1M floor at every size: with one launch per iteration the
    // smaller pool wins (C2 at 512 spp, two parts: 1M 6529-6637, 1.5M
    // 6501-6511, 2M 6404-6460, 3M 6103-6210, 4M 6172-6180 Msamples/s; the
    // 64-spp share: 768K 4926-4981, 1M 5054-5131, 1.5M 4884-4998).
    if (one_bounce) return render_one_bounce(c, rd, pixels, blocks, rgbw_out, stats, t0);
    if (M > kWorkMask) throw NoriException(NORI_ERR_INVALID, "frame too large: more than 2^29 pixels per pass");
    const bool timing = rd.timing != 0;
    // S.ext_inline: an iteration is the shade launch alone.  A timing render
    // keeps the two launches (one event span per kernel), so its shade kernel
    // reads the hits as without the flag, and it keeps the pool and the parts
    // of the two-launch loop.
    const bool ext_loop = S.ext_inline != 0 && !timing;
    uint32_t pool = rd.path_pool;
    if (!pool) {  // NORI_PATH_POOL: default pool size override (tuning)
        const char *e = std::getenv("NORI_PATH_POOL");
        if (e && std::atol(e) > 0) {
            pool = (uint32_t)std::min<long>(std::atol(e), 1L << 26);
        } else {
            const uint64_t want = (uint64_t)passes * M / (c.stack ? 8 : 16);
            pool = 1u << 20;
            while (!ext_loop && pool < (1u << 22) && pool < want) pool <<= 1;
        }
    }
    pool = std::max<uint32_t>(kSeg, (pool + kSeg - 1) / kSeg * kSeg);
    ensure_pool(c, pool);
    // sample-record budget: chunks of passes, each < 2^31 records
    const size_t rec_budget = (size_t)6 << 30;
    uint32_t chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(passes, rec_budget / (16 * (size_t)M)));
    // work ids (record indices) < 2^29: the path queue keeps a chromatic
    // sample's colour channel in bits 29-30 of the same word (kWorkMask)
    chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(chunk, ((uint64_t)1 << kChanShift) / M));
    c.rec.ensure(16 * (size_t)chunk * M);
    c.counters.ensure(sizeof(Counters));
    const size_t film_elems = 4 * (size_t)(W + 2 * B) * (H + 2 * B);
    float *film = nullptr;
    if (rd.output_on_device) {
        film = rgbw_out;
    } else {
        c.film.ensure(film_elems * sizeof(float));
        film = c.film.as<float>();
        HIP_TRY(hipMemsetAsync(film, 0, film_elems * sizeof(float), c.stream));
    }
    if (!c.pinned) {
        // host-mapped, coherent: the shade kernel stores the completion flag here
        HIP_TRY(hipHostMalloc((void **)&c.pinned, 256, hipHostMallocMapped | hipHostMallocCoherent));
        HIP_TRY(hipHostGetDevicePointer((void **)&c.pinned_dev, c.pinned, 0));
        for (auto &r : c.ring) {
            r.resize(kRing);
            for (auto &e : r) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
    }
    Counters *C = c.counters.as<Counters>();
    ShadowQueue sq{c.sq[0].as<float4>(), c.sq[1].as<float4>(), c.sq[2].as<float4>()};
    PathQueue Q[2] = {queue_of(c, 0), queue_of(c, 1)};
    if (!c.in_rounds) c.cancel = 0;
    c.report(0.0);
    const uint64_t total_all = (uint64_t)passes * M;
    uint64_t done_before = 0, rays_c = 0, rays_s = 0, invalid = 0, iters = 0;
    Timers tm;
    struct Span {
        hipEvent_t a, b;
        int kind;
    };
    std::vector<Span> spans;
    DevScene Sk = S;
    if (!ext_loop) Sk.ext_inline = 0;
    auto timed_on = [&](hipStream_t st, int kind, auto &&launch) {
        if (!timing) {
            HIP_TRY(launch());
            return;
        }
        Span s{tm.get(), tm.get(), kind};
        HIP_TRY(hipEventRecord(s.a, st));
        HIP_TRY(launch());
        HIP_TRY(hipEventRecord(s.b, st));
        spans.push_back(s);
    };
    auto timed = [&](int kind, auto &&launch) { timed_on(c.stream, kind, launch); };
    bool cancelled = false;
    const uint32_t parts = std::max<uint32_t>(1, std::min<uint32_t>(pool_parts(ext_loop), pool / kSeg));
    const uint32_t G = pool / kSeg;
    SegState seg{{c.seg[0].as<uint32_t>(), c.seg[1].as<uint32_t>()}, c.seg[2].as<uint32_t>(), c.seg[3].as<uint32_t>(),
                 c.segstats.as<uint4>()};
    std::vector<uint4> hstats(G);
    uint64_t finish_rays = 0, samples_started = 0;
    float *var = var_begin(c, rd);
    for (uint32_t p0 = 0; p0 < passes && !cancelled; p0 += chunk) {
        uint32_t np = std::min(chunk, passes - p0);
        WorkDesc wd{(uint64_t)np * M, M, rd.pass_begin + p0, c.pixels.as<uint32_t>(), rd.seed, G, c.pinned_dev, 1, 0,
                    var};
        wd.rot = stream_rotation(wd.total, M, G);
        __atomic_store_n(&c.pinned[0], 0u, __ATOMIC_RELEASE);
        __atomic_store_n(&c.pinned[1], 0u, __ATOMIC_RELEASE);
        // segments whose stream is empty from the start count as exhausted
        uint32_t empty = 0;
        for (uint32_t b = 0; b < G; ++b) empty += stream_work(wd, b, 0) >= wd.total;
        HIP_TRY(launch_reset(C, empty, seg, G, c.stream));
        int last_out = 0;
        // The pool is split into `parts` independent parts (segments never
        // interact), each driven on its own stream: the memory-bound shade
        // launch of one part overlaps the VALU-bound traversal of another.
        std::vector<uint32_t> Gp(parts), base(parts);
        for (uint32_t h = 0; h < parts; ++h) {
            base[h] = (uint32_t)((uint64_t)G * h / parts);
            Gp[h] = (uint32_t)((uint64_t)G * (h + 1) / parts) - base[h];
        }
        auto q_view = [&](const PathQueue &q, uint32_t b0) {
            const size_t e = (size_t)b0 * kSeg;
            return PathQueue{q.ray_o + e, q.ray_d + e, q.hit + e, q.thr + e, q.rng + e};
        };
        std::vector<std::array<PathQueue, 2>> Qh(parts);
        std::vector<ShadowQueue> sqh(parts);
        std::vector<SegState> segh(parts);
        std::vector<WorkDesc> wdh(parts);
        for (uint32_t h = 0; h < parts; ++h) {
            Qh[h][0] = q_view(Q[0], base[h]);
            Qh[h][1] = q_view(Q[1], base[h]);
            const size_t e = (size_t)base[h] * kSeg;
            sqh[h] = ShadowQueue{sq.ray_o + e, sq.ray_d + e, sq.payload + e};
            segh[h] = SegState{{seg.cnt[0] + base[h], seg.cnt[1] + base[h]}, seg.shcnt + base[h],
                               seg.cursor + base[h], seg.stats + base[h]};
            wdh[h] = wd;
            wdh[h].b0 = base[h];
        }
        HIP_TRY(hipEventRecord(c.fork, c.stream));  // the part streams start after the resets above
        for (uint32_t h = 1; h < parts; ++h) HIP_TRY(hipStreamWaitEvent(c.parts[h], c.fork, 0));
        uint64_t lag = (uint64_t)lookahead();
        // NORI_DEBUG: host time spent enqueuing vs waiting on the ring events
        // (a wait that returns at once means the device ran dry of work)
        const bool dbg = debug_log();
        double t_enq = 0.0, t_wait = 0.0;
        uint32_t idle_waits = 0;
        auto now_us = [] {
            return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
        };
        for (uint64_t it = 0;; ++it) {
            const double te0 = dbg ? now_us() : 0.0;
            int in = (int)(it & 1), out = in ^ 1;
            last_out = out;
            for (uint32_t h = 0; h < parts; ++h) {
                hipStream_t st = h ? c.parts[h] : c.stream;
                const SegState &sg = segh[h];
                timed_on(st, 2, [&] {
                    return launch_shade(Sk, Qh[h][in], Qh[h][out], sqh[h], sg, in, wdh[h], c.rec.as<float4>(), C,
                                        Gp[h], st, &c.shade_rtc);
                });
                hipError_t both_err = hipSuccess;
                if (S.nee_inline) {  // the shadow rays were traced by k_shade itself
                    if (ext_loop) continue;  // ... and so will the next vertex's extension ray be
                    timed_on(st, 0, [&] { return launch_extend(S, Qh[h][out], sg.cnt[out], Gp[h], c.stack, st, &c.rtc); });
                    continue;
                }
                if (!timing && c.fuse_trace &&
                    launch_trace_both(S, Qh[h][out], sg.cnt[out], sqh[h], sg.shcnt, c.rec.as<float4>(), Gp[h], c.stack,
                                      &c.rtc, st, both_err)) {
                    HIP_TRY(both_err);  // (the timed renders keep two launches: one event span per kernel)
                    continue;
                }
                timed_on(st, 0, [&] { return launch_extend(S, Qh[h][out], sg.cnt[out], Gp[h], c.stack, st, &c.rtc); });
                timed_on(st, 1, [&] {
                    return launch_shadow(S, sqh[h], sg.shcnt, c.rec.as<float4>(), Gp[h], c.stack, st, &c.rtc);
                });
            }
            ++iters;
            // an event per iteration; the host waits on the one from `lag`
            // iterations back
            const uint64_t ev = it;
            for (uint32_t h = 0; h < parts; ++h)
                HIP_TRY(hipEventRecord(c.ring[h][ev % kRing], h ? c.parts[h] : c.stream));
            const double te1 = dbg ? now_us() : 0.0;
            t_enq += te1 - te0;
            if (ev >= lag) {
                for (uint32_t h = 0; h < parts; ++h) HIP_TRY(hipEventSynchronize(c.ring[h][(ev - lag) % kRing]));
                if (dbg) {
                    const double w = now_us() - te1;
                    t_wait += w;
                    idle_waits += w < 5.0 ? 1u : 0u;
                }
                uint32_t exhausted = __atomic_load_n(&c.pinned[1], __ATOMIC_ACQUIRE);
                // the streams are running dry: queue fewer iterations ahead,
                // so that few drain iterations (full-grid launches over a
                // thinning pool) are already queued when the last one does
                if (exhausted) lag = std::min<uint64_t>(lag, kLookaheadEnd);
                c.report(std::min(1.0, (double)done_before / (double)total_all +
                                           (double)np / passes * exhausted / G));
                // every work id has been handed out: finish the remaining paths in one launch
                if (__atomic_load_n(&c.pinned[0], __ATOMIC_ACQUIRE)) break;
                if (c.cancel.load()) {
                    cancelled = true;
                    break;
                }
            }
        }
        // ext_loop: the last iteration's survivors and new samples have no hits
        // yet; the finisher below reads them, so they are traced once here
        for (uint32_t h = 0; ext_loop && !cancelled && h < parts; ++h)
            HIP_TRY(launch_extend(S, Qh[h][last_out], segh[h].cnt[last_out], Gp[h], c.stack, h ? c.parts[h] : c.stream,
                                  &c.rtc));
        for (uint32_t h = 1; h < parts; ++h) {  // join: the tail below runs on the whole pool
            HIP_TRY(hipEventRecord(c.joins[h], c.parts[h]));
            HIP_TRY(hipStreamWaitEvent(c.stream, c.joins[h], 0));
        }
        if (cancelled) break;
        // The samples still in flight are marked pending; the film splat of all
        // the others runs on the side stream while the finisher completes the
        // pending ones and splats each itself.
        hipStream_t splat_st = c.side;
        HIP_TRY(launch_mark(Q[last_out], seg, last_out, c.rec.as<float4>(), G, c.stream));
        HIP_TRY(launch_tail_prefix(seg, last_out, G, c.tailpre.as<uint32_t>(), c.stream));
        HIP_TRY(hipEventRecord(c.fork, c.stream));
        HIP_TRY(hipStreamWaitEvent(c.side, c.fork, 0));
        SplatDesc sd{M, np, rd.pass_begin + p0, std::max<uint32_t>(1, splat_passes(np, blocks.size())),
                     c.blocks.as<int4>(), rd.seed, var};
        auto splat = [&] {
            timed_on(splat_st, 3, [&] { return launch_splat(S, c.rec.as<float4>(), sd, (uint32_t)blocks.size(), film, C, splat_st); });
        };
        auto finish = [&] {
            timed(4, [&] {
                return launch_finish(S, Q[last_out], seg, last_out, c.rec.as<float4>(), wd, film, C, G, c.stack,
                                     c.tailpre.as<uint32_t>(), c.stream);
            });
        };
        // both wait for the same fork; the finisher's waves are enqueued first
        // (c.finish_first) so that they are resident before the splat fills the CUs
        if (c.finish_first) {
            finish();
            splat();
        } else {
            splat();
            finish();
        }
        HIP_TRY(hipEventRecord(c.join, c.side));
        HIP_TRY(hipStreamWaitEvent(c.stream, c.join, 0));
        // read-back through pinned staging: both copies queue behind the
        // finisher without a host round trip each (pageable copies stage twice)
        const size_t rb = sizeof(Counters) + 16 * (size_t)G;
        if (c.readback_bytes < rb) {
            if (c.readback) HIP_TRY(hipHostFree(c.readback));
            c.readback = nullptr;
            c.readback_bytes = 0;
            HIP_TRY(hipHostMalloc((void **)&c.readback, rb, hipHostMallocDefault));
            c.readback_bytes = rb;
        }
        HIP_TRY(hipMemcpyAsync(c.readback, C, sizeof(Counters), hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipMemcpyAsync(c.readback + sizeof(Counters), seg.stats, 16 * (size_t)G, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
        Counters hc;
        std::memcpy(&hc, c.readback, sizeof(Counters));
        std::memcpy(hstats.data(), c.readback + sizeof(Counters), 16 * (size_t)G);
        for (const uint4 &st : hstats) {
            rays_c += st.x;
            rays_s += st.y;
            samples_started += st.z;
            finish_rays += st.w;
        }
        invalid += hc.invalid;
        if (debug_log())
        {
            std::fprintf(stderr, "[nori] chunk %u: %lu iterations, finisher %u paths, longest %u rays\n", p0,
                         (unsigned long)iters, hc.finish_paths, hc.finish_max_rays);
            std::fprintf(stderr, "[nori] host loop: %.0f us enqueuing, %.0f us waiting; %u of the waits returned at once\n",
                         t_enq, t_wait, idle_waits);
            if (hc.prof[6])  // NORI_PROF_SHADE builds
                std::fprintf(stderr, "[nori] shade clocks per wave: loads %.0f shade %.0f compact %.0f store %.0f regen %.0f drain %.0f (%llu waves)\n",
                             (double)hc.prof[0] / hc.prof[6], (double)hc.prof[1] / hc.prof[6],
                             (double)hc.prof[2] / hc.prof[6], (double)hc.prof[3] / hc.prof[6],
                             (double)hc.prof[4] / hc.prof[6], (double)hc.prof[5] / hc.prof[6], hc.prof[6]);
            else if (hc.prof[4])  // NORI_PROF_FINISH builds
                std::fprintf(stderr, "[nori] finisher clocks per wave-iteration: shade %.0f shadow %.0f splat %.0f extend %.0f (%llu); "
                             "longest wave %.3f ms over %llu iterations\n",
                             (double)hc.prof[0] / hc.prof[4], (double)hc.prof[1] / hc.prof[4],
                             (double)hc.prof[2] / hc.prof[4], (double)hc.prof[3] / hc.prof[4], hc.prof[4],
                             (double)(hc.prof[5] >> 20) * 1e-5, hc.prof[5] & 0xFFFFFull);
            if (hc.prof[14])  // NORI_PROF_GLASS builds
                std::fprintf(stderr, "[nori] lone-lane glass chains: %llu chord bounces, %.0f ns each\n", hc.prof[14],
                             10.0 * hc.prof[13] / hc.prof[14]);
            if (hc.prof[12])
                std::fprintf(stderr, "[nori] finisher late iterations (lone lanes): shade %.0f shadow %.0f splat %.0f extend %.0f ns (%llu)\n",
                             10.0 * hc.prof[8] / hc.prof[12], 10.0 * hc.prof[9] / hc.prof[12],
                             10.0 * hc.prof[10] / hc.prof[12], 10.0 * hc.prof[11] / hc.prof[12], hc.prof[12]);
        }
        done_before += wd.total;
    }
    if (samples_started != done_before && !cancelled)
        throw NoriException(NORI_ERR_INVALID, "internal: started " + std::to_string(samples_started) + " of " +
                                                  std::to_string(done_before) + " samples");
    double kms[5] = {0, 0, 0, 0, 0};
    if (timing) {
        HIP_TRY(hipStreamSynchronize(c.stream));
        for (const Span &s : spans) {
            float ms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&ms, s.a, s.b));
            kms[s.kind] += ms;
        }
    }
    if (!rd.output_on_device && !cancelled) {
        std::vector<float> hf(film_elems);
        HIP_TRY(hipMemcpy(hf.data(), film, film_elems * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < film_elems; ++i) rgbw_out[i] += hf[i];
    }
    var_finish(c, rd, cancelled);
    HIP_TRY(hipStreamSynchronize(c.stream));
    HIP_TRY(hipStreamSynchronize(c.side));
    for (int h = 1; h < kMaxParts; ++h) HIP_TRY(hipStreamSynchronize(c.parts[h]));
    c.report(1.0);
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->samples = done_before;
        stats->invalid_samples = invalid;
        stats->rays_closest = rays_c;
        stats->rays_shadow = rays_s;
        stats->iterations = iters;
        stats->scene_bytes = c.scene_bytes;
        stats->bvh_nodes = c.bvh_nodes;
        stats->bvh_depth = c.bvh_depth;
        stats->stream_parts = parts;
        stats->path_pool = pool;
        stats->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        stats->ms_extend = kms[0];
        stats->ms_shadow = kms[1];
        stats->ms_shade = kms[2];
        stats->ms_splat = kms[3];
        stats->ms_finish = kms[4];
        stats->rays_finish = finish_rays;
        stats->scan_rtc = c.rtc.extend ? 1u : 0u;
        stats->scan_rtc_cached = c.rtc.cached ? 1u : 0u;
        stats->ms_scan_rtc = c.rtc.compile_ms;
        stats->nee_inline = S.nee_inline ? 1u : 0u;
        stats->ext_inline = S.ext_inline ? 1u : 0u;
    }
    if (cancelled) return fail(NORI_ERR_CANCELLED, "rendering was cancelled");
    return NORI_OK;
}

// nori_gpu_render_features: k_features over the selected blocks' pixels, in
// chunks of passes (about 16M samples per launch) between which a cancel
// request is honoured.  The kernel continues each pixel's sums from the values
// in the buffer, so a host buffer is uploaded first and copied back after the
// last chunk: host and device buffers receive the same bits.
int render_features(nori_gpu_ctx &c, const nori_gpu_render_desc &rd, float *features, nori_gpu_stats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(c.device));
    if (rd.variance_out) throw NoriException(NORI_ERR_INVALID, "nori_gpu_render_features: variance_out must be NULL");
    work_lists(c, rd);
    const uint32_t M = (uint32_t)c.hpixels.size(), passes = rd.pass_count ? rd.pass_count : c.spp;
    if (passes == 0 || M == 0) throw NoriException(NORI_ERR_INVALID, "nothing to render (pass_count or blocks empty)");
    const size_t n = 8 * (size_t)c.S.W * (size_t)c.S.H;
    float *dev = features;
    if (rd.output_on_device) {
        if ((uintptr_t)features % 16) throw NoriException(NORI_ERR_INVALID, "device features must be 16-byte aligned");
    } else {
        c.varbuf.ensure(n * sizeof(float));
        dev = c.varbuf.as<float>();
        HIP_TRY(hipMemcpyAsync(dev, features, n * sizeof(float), hipMemcpyHostToDevice, c.stream));
    }
    c.cancel = 0;
    c.report(0.0);
    const uint32_t chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(passes, ((uint64_t)1 << 24) / M));
    Timers tm;
    std::vector<std::array<hipEvent_t, 2>> spans;
    uint64_t done = 0;
    bool cancelled = false;
    for (uint32_t p0 = 0; p0 < passes; p0 += chunk) {
        if (c.cancel.load()) {
            cancelled = true;
            break;
        }
        const uint32_t np = std::min(chunk, passes - p0);
        std::array<hipEvent_t, 2> ev{};
        if (rd.timing) {
            for (auto &e : ev) e = tm.get();
            HIP_TRY(hipEventRecord(ev[0], c.stream));
        }
        HIP_TRY(launch_features(c.S, c.pixels.as<uint32_t>(), M, rd.pass_begin + p0, np, rd.seed, dev, c.stack,
                                c.stream));
        if (rd.timing) {
            HIP_TRY(hipEventRecord(ev[1], c.stream));
            spans.push_back(ev);
        }
        HIP_TRY(hipStreamSynchronize(c.stream));
        done += (uint64_t)np * M;
        c.report((double)(p0 + np) / passes);
    }
    double kms = 0.0;
    for (const auto &e : spans) {
        float a = 0;
        HIP_TRY(hipEventElapsedTime(&a, e[0], e[1]));
        kms += a;
    }
    if (!rd.output_on_device && !cancelled)
        HIP_TRY(hipMemcpy(features, dev, n * sizeof(float), hipMemcpyDeviceToHost));
    c.report(1.0);
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->samples = done;
        stats->rays_closest = done;  // one primary ray per sample
        stats->scene_bytes = c.scene_bytes;
        stats->bvh_nodes = c.bvh_nodes;
        stats->bvh_depth = c.bvh_depth;
        stats->stream_parts = 1;
        stats->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        stats->ms_shade = kms;  // k_features
        stats->scan_rtc = c.rtc.extend ? 1u : 0u;  // (k_features scans generically, like k_direct)
        stats->scan_rtc_cached = c.rtc.cached ? 1u : 0u;
        stats->ms_scan_rtc = c.rtc.compile_ms;
    }
    if (cancelled) return fail(NORI_ERR_CANCELLED, "rendering was cancelled");
    return NORI_OK;
}

// nori_gpu_query: launch_trace (the kernels of nori_gpu_trace), then k_surface
// on its hits.  Device buffers are used in place; host arrays pass through the
// context's staging buffers in chunks of at most NORI_QUERY_CHUNK rays.
uint32_t query_chunk() {
    if (const char *e = std::getenv("NORI_QUERY_CHUNK")) {
        const long long v = std::atoll(e);
        if (v > 0) return (uint32_t)std::min<long long>(v, 0xFFFFFFFFll);
    }
    return 1u << 22;
}
int query(nori_gpu_ctx &c, const nori_gpu_query_desc &qd, const float *rays, nori_gpu_hit *hits,
          nori_gpu_surface *surf, nori_gpu_stats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(c.device));
    const uint32_t n = qd.n;
    if (stats)
        for (auto &e : c.q_ev)
            if (!e) HIP_TRY(hipEventCreate(&e));
    double ms_trace = 0.0, ms_surf = 0.0;
    // one chunk on the device: rays r -> hits h (-> records s)
    auto run = [&](const float4 *r, uint32_t m, float4 *h, float4 *s) {
        if (stats) HIP_TRY(hipEventRecord(c.q_ev[0], c.stream));
        HIP_TRY(launch_trace(c.S, r, m, qd.any_hit, h, c.stack, c.stream, &c.rtc));
        if (stats) HIP_TRY(hipEventRecord(c.q_ev[1], c.stream));
        if (s) HIP_TRY(launch_surface(c.S, r, h, m, s, c.stream));
        if (stats) HIP_TRY(hipEventRecord(c.q_ev[2], c.stream));
    };
    auto elapsed = [&] {  // (after the stream has been synchronised)
        if (!stats) return;
        float a = 0.0f, b = 0.0f;
        HIP_TRY(hipEventElapsedTime(&a, c.q_ev[0], c.q_ev[1]));
        HIP_TRY(hipEventElapsedTime(&b, c.q_ev[1], c.q_ev[2]));
        ms_trace += a;
        ms_surf += b;
    };
    if (qd.on_device) {
        float4 *h = reinterpret_cast<float4 *>(hits);
        if (!h) {
            c.q_hits.ensure(16 * (size_t)n);
            h = c.q_hits.as<float4>();
        }
        run(reinterpret_cast<const float4 *>(rays), n, h, reinterpret_cast<float4 *>(surf));
        HIP_TRY(hipStreamSynchronize(c.stream));
        elapsed();
    } else {
        const uint32_t chunk = std::min(n, query_chunk());
        c.q_rays.ensure(32 * (size_t)chunk);
        c.q_hits.ensure(16 * (size_t)chunk);
        if (surf) c.q_surf.ensure(64 * (size_t)chunk);
        for (uint64_t i0 = 0; i0 < n; i0 += chunk) {
            const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, n - i0);
            HIP_TRY(hipMemcpyAsync(c.q_rays.p, rays + 8 * i0, 32 * (size_t)m, hipMemcpyHostToDevice, c.stream));
            run(c.q_rays.as<float4>(), m, c.q_hits.as<float4>(), surf ? c.q_surf.as<float4>() : nullptr);
            if (hits) HIP_TRY(hipMemcpyAsync(hits + i0, c.q_hits.p, 16 * (size_t)m, hipMemcpyDeviceToHost, c.stream));
            if (surf) HIP_TRY(hipMemcpyAsync(surf + i0, c.q_surf.p, 64 * (size_t)m, hipMemcpyDeviceToHost, c.stream));
            HIP_TRY(hipStreamSynchronize(c.stream));
            elapsed();
        }
    }
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        (qd.any_hit ? stats->rays_shadow : stats->rays_closest) = n;
        stats->scene_bytes = c.scene_bytes;
        stats->bvh_nodes = c.bvh_nodes;
        stats->bvh_depth = c.bvh_depth;
        stats->stream_parts = 1;
        stats->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        stats->ms_extend = ms_trace;
        stats->ms_shade = ms_surf;  // k_surface
        stats->scan_rtc = c.rtc.extend ? 1u : 0u;
        stats->scan_rtc_cached = c.rtc.cached ? 1u : 0u;
        stats->ms_scan_rtc = c.rtc.compile_ms;
    }
    return NORI_OK;
}

// nori_gpu_camera_rays: k_camera_rays over the selected blocks' pixels, in
// chunks of passes (about 16M rays per launch).  Only the selected pixels are
// written, so a host buffer is uploaded first and copied back afterwards: the
// other entries keep the caller's values, as in a device buffer.
int camera_rays(nori_gpu_ctx &c, const nori_gpu_render_desc &rd, float *rays) {
    HIP_TRY(hipSetDevice(c.device));
    if (rd.variance_out) throw NoriException(NORI_ERR_INVALID, "nori_gpu_camera_rays: variance_out must be NULL");
    work_lists(c, rd);
    const uint32_t M = (uint32_t)c.hpixels.size(), passes = rd.pass_count ? rd.pass_count : c.spp;
    if (passes == 0 || M == 0) throw NoriException(NORI_ERR_INVALID, "nothing to do (pass_count or blocks empty)");
    const size_t bytes = 32 * (size_t)passes * (size_t)c.S.W * (size_t)c.S.H;
    float *dev = rays;
    if (rd.output_on_device) {
        if ((uintptr_t)rays % 16) throw NoriException(NORI_ERR_INVALID, "device rays must be 16-byte aligned");
    } else {
        c.q_rays.ensure(bytes);
        dev = c.q_rays.as<float>();
        HIP_TRY(hipMemcpyAsync(dev, rays, bytes, hipMemcpyHostToDevice, c.stream));
    }
    const uint32_t chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(passes, ((uint64_t)1 << 24) / M));
    for (uint32_t k0 = 0; k0 < passes; k0 += chunk)
        HIP_TRY(launch_camera_rays(c.S, c.pixels.as<uint32_t>(), M, rd.pass_begin, k0, std::min(chunk, passes - k0),
                                   rd.seed, dev, c.stream));
    if (!rd.output_on_device) HIP_TRY(hipMemcpyAsync(rays, dev, bytes, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    return NORI_OK;
}

// The shading queries (nori_gpu_bsdf_eval .. nori_gpu_emitter_eval, stated in
// nori_gpu.h): one element-wise kernel over up to three input arrays and one
// output array.  Device arrays are checked (alignment, and that the runtime
// knows them as device memory: update_vertices' check) and used in place;
// host arrays pass through the context's sh_in / sh_out buffers in chunks of
// at most NORI_QUERY_CHUNK elements.
struct ShadeArr {
    const void *p;   // may be null only where the call allows it (ids)
    size_t stride;   // bytes per element
    size_t align;    // of a device pointer
};
template <class Launch>
int shading_call(nori_gpu_ctx &c, const char *name, const nori_gpu_shading_desc &sd, const ShadeArr (&in)[3], void *out,
                 size_t out_stride, Launch &&launch) {
    HIP_TRY(hipSetDevice(c.device));
    const uint32_t n = sd.n;
    if (sd.on_device) {
        const ShadeArr all[4] = {in[0], in[1], in[2], ShadeArr{out, out_stride, 16}};
        for (const ShadeArr &a : all) {
            if (!a.p) continue;
            if ((uintptr_t)a.p % a.align)
                throw NoriException(NORI_ERR_INVALID, std::string(name) + ": a device pointer is not " +
                                                          std::to_string(a.align) + "-byte aligned");
            hipPointerAttribute_t at{};
            if (hipPointerGetAttributes(&at, a.p) != hipSuccess ||
                (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged)) {
                (void)hipGetLastError();
                throw NoriException(NORI_ERR_INVALID, std::string(name) + ": on_device with a pointer that is not device memory");
            }
        }
        const void *d[3] = {in[0].p, in[1].p, in[2].p};
        HIP_TRY(launch(d, out, n));
        HIP_TRY(hipStreamSynchronize(c.stream));
        return NORI_OK;
    }
    const uint32_t chunk = std::min(n, query_chunk());
    for (int k = 0; k < 3; ++k)
        if (in[k].p) c.sh_in[k].ensure(in[k].stride * (size_t)chunk);
    c.sh_out.ensure(out_stride * (size_t)chunk);
    for (uint64_t i0 = 0; i0 < n; i0 += chunk) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, n - i0);
        const void *d[3] = {nullptr, nullptr, nullptr};
        for (int k = 0; k < 3; ++k) {
            if (!in[k].p) continue;
            HIP_TRY(hipMemcpyAsync(c.sh_in[k].p, (const char *)in[k].p + in[k].stride * i0, in[k].stride * (size_t)m,
                                   hipMemcpyHostToDevice, c.stream));
            d[k] = c.sh_in[k].p;
        }
        HIP_TRY(launch(d, c.sh_out.p, m));
        HIP_TRY(hipMemcpyAsync((char *)out + out_stride * i0, c.sh_out.p, out_stride * (size_t)m, hipMemcpyDeviceToHost,
                               c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
    }
    return NORI_OK;
}
// Host records: the shape index must be the miss's -1 or a shape of the scene.
void check_host_records(const nori_gpu_ctx &c, const char *name, const nori_gpu_surface *surf, uint32_t n) {
    const int32_t ns = (int32_t)c.hshapes.size();
    for (uint32_t i = 0; i < n; ++i)
        if (surf[i].shape < -1 || surf[i].shape >= ns)
            throw NoriException(NORI_ERR_INVALID, std::string(name) + ": record " + std::to_string(i) + " names shape " +
                                                      std::to_string(surf[i].shape) + " of " + std::to_string(ns));
}

// nori_gpu_sample_uniforms: k_sample_uniforms over the selected blocks'
// pixels, in chunks of passes like camera_rays (and with its handling of a
// host buffer: uploaded first, so that unselected entries keep their values).
int sample_uniforms(nori_gpu_ctx &c, const nori_gpu_render_desc &rd, uint32_t first, uint32_t count, float *out) {
    HIP_TRY(hipSetDevice(c.device));
    if (rd.variance_out) throw NoriException(NORI_ERR_INVALID, "nori_gpu_sample_uniforms: variance_out must be NULL");
    if (count == 0 || first + count < first)
        throw NoriException(NORI_ERR_INVALID, "nori_gpu_sample_uniforms: count is 0 or first + count overflows");
    work_lists(c, rd);
    const uint32_t M = (uint32_t)c.hpixels.size(), passes = rd.pass_count ? rd.pass_count : c.spp;
    if (passes == 0 || M == 0) throw NoriException(NORI_ERR_INVALID, "nothing to do (pass_count or blocks empty)");
    const size_t bytes = 4 * (size_t)count * (size_t)passes * (size_t)c.S.W * (size_t)c.S.H;
    float *dev = out;
    if (rd.output_on_device) {
        if ((uintptr_t)out % 4) throw NoriException(NORI_ERR_INVALID, "nori_gpu_sample_uniforms: the device buffer must be 4-byte aligned");
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, out) != hipSuccess ||
            (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged)) {
            (void)hipGetLastError();
            throw NoriException(NORI_ERR_INVALID, "nori_gpu_sample_uniforms: output_on_device with a pointer that is not device memory");
        }
    } else {
        c.sh_out.ensure(bytes);
        dev = c.sh_out.as<float>();
        HIP_TRY(hipMemcpyAsync(dev, out, bytes, hipMemcpyHostToDevice, c.stream));
    }
    const uint32_t chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(passes, ((uint64_t)1 << 24) / M));
    for (uint32_t k0 = 0; k0 < passes; k0 += chunk)
        HIP_TRY(launch_sample_uniforms(c.S, c.pixels.as<uint32_t>(), M, rd.pass_begin, k0, std::min(chunk, passes - k0),
                                       rd.seed, first, count, dev, c.stream));
    if (!rd.output_on_device) HIP_TRY(hipMemcpyAsync(out, dev, bytes, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    return NORI_OK;
}

// nori_gpu_update_vertices (stated in nori_gpu.h): validate, then on the
// context's stream count the non-finite inputs (nothing is modified before
// that count is back), set the vertices, rebuild the records, refit the boxes
// one launch per level of c.refit, and bring the lights and the scene box up
// to date.
int update_vertices(nori_gpu_ctx &c, const nori_gpu_update_desc &ud, nori_gpu_update_stats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    if (c.stack == 0)
        throw NoriException(NORI_ERR_UNSUPPORTED,
                            "nori_gpu_update_vertices: a scan-mode context (its scan list and specialised kernels "
                            "are functions of the geometry); create the context with NORI_TRAVERSAL=bvh");
    if (c.S.integrator == NORI_INTEGRATOR_PHOTONMAPPER)
        throw NoriException(NORI_ERR_UNSUPPORTED,
                            "nori_gpu_update_vertices: a photonmapper context (its photon map was traced at creation)");
    if (ud.num_vertices != c.num_vertices)
        throw NoriException(NORI_ERR_INVALID, "nori_gpu_update_vertices: num_vertices " + std::to_string(ud.num_vertices) +
                                                  " is not the scene's " + std::to_string(c.num_vertices));
    for (uint32_t r : ud.reserved)
        if (r != 0) throw NoriException(NORI_ERR_INVALID, "nori_gpu_update_vertices: reserved must be 0");
    if (ud.on_device && ((uintptr_t)ud.positions % 4 || (uintptr_t)ud.normals % 4))
        throw NoriException(NORI_ERR_INVALID, "nori_gpu_update_vertices: device pointers must be 4-byte aligned");
    HIP_TRY(hipSetDevice(c.device));
    if (ud.on_device)  // a host pointer here would fault in the first kernel: ask the runtime what it is
        for (const float *p : {ud.positions, ud.normals}) {
            hipPointerAttribute_t at{};
            if (!p) continue;
            if (hipPointerGetAttributes(&at, p) != hipSuccess ||
                (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged)) {
                (void)hipGetLastError();
                throw NoriException(NORI_ERR_INVALID, "nori_gpu_update_vertices: on_device with a pointer that is not device memory");
            }
        }
    for (auto &e : c.upd_ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    const uint32_t V = c.num_vertices;
    const size_t nfl = 3 * (size_t)V;
    const float *dp = ud.positions, *dn = ud.normals;
    if (!ud.on_device) {
        c.upd_pos.ensure(nfl * 4);
        HIP_TRY(hipMemcpyAsync(c.upd_pos.p, ud.positions, nfl * 4, hipMemcpyHostToDevice, c.stream));
        dp = c.upd_pos.as<float>();
        if (ud.normals) {
            c.upd_nrm.ensure(nfl * 4);
            HIP_TRY(hipMemcpyAsync(c.upd_nrm.p, ud.normals, nfl * 4, hipMemcpyHostToDevice, c.stream));
            dn = c.upd_nrm.as<float>();
        }
    }
    uint32_t launches = 0;
    // ---- a pass of its own: nothing is modified before its count is back
    c.upd_count.ensure(4);
    HIP_TRY(hipMemsetAsync(c.upd_count.p, 0, 4, c.stream));
    HIP_TRY(launch_refit_count_nonfinite(dp, dn, nfl, c.upd_count.as<uint32_t>(), c.stream));
    ++launches;
    uint32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, c.upd_count.p, 4, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    if (bad)
        throw NoriException(NORI_ERR_INVALID, "nori_gpu_update_vertices: " + std::to_string(bad) +
                                                  " non-finite position or normal values; nothing was changed");
    // ---- vertices, records, boxes
    float4 *pos = c.pos.as<float4>();
    HIP_TRY(hipEventRecord(c.upd_ev[0], c.stream));
    HIP_TRY(launch_refit_set_vertices(pos, c.nrm.as<float4>(), dp, dn, V, c.stream));
    HIP_TRY(launch_refit_records(c.prims.as<float4>(), c.S.tri_vidx, pos, c.S.num_prims, c.stream));
    launches += 2;
    for (uint32_t l = 0; l < c.refit.levels(); ++l) {
        const uint32_t b = c.refit.level_begin[l], n = c.refit.level_begin[l + 1] - b;
        HIP_TRY(launch_refit_level(c.nodes.as<float4>(), c.S.prims, c.S.tri_vidx, pos, c.refit_slots.as<uint32_t>() + b, n,
                                   c.stream));
        launches += n ? 1u : 0u;
    }
    HIP_TRY(hipEventRecord(c.upd_ev[1], c.stream));
    // ---- the scene box: the root node's used slots (128 bytes back)
    float root[32], box[6];
    HIP_TRY(hipMemcpyAsync(root, c.nodes.p, sizeof(root), hipMemcpyDeviceToHost, c.stream));
    // ---- the lights: area CDF and normalisation of every mesh with an emitter, in nori_gpu_create's
    // own order on the host (mesh_area_cdf) from a read-back of that mesh's vertices; emitter meshes are small
    std::vector<std::vector<float>> verts(c.emitter_meshes.size());
    for (size_t m = 0; m < c.emitter_meshes.size(); ++m) {
        const auto &em = c.emitter_meshes[m];
        verts[m].resize(4 * (size_t)em.vtx_count);
        HIP_TRY(hipMemcpyAsync(verts[m].data(), pos + em.vtx_first, 16 * (size_t)em.vtx_count, hipMemcpyDeviceToHost,
                               c.stream));
    }
    HIP_TRY(hipStreamSynchronize(c.stream));
    refit_root_box(root, box);
    for (size_t m = 0; m < c.emitter_meshes.size(); ++m) {
        const auto &em = c.emitter_meshes[m];
        std::vector<float> cdf;
        const float *v = verts[m].data();
        c.hshapes[em.shape].area_norm = mesh_area_cdf(em.tri.data(), (uint32_t)(em.tri.size() / 3),
                                                      [&](uint32_t i) { return v + 4 * (size_t)(i - em.vtx_first); }, cdf);
        HIP_TRY(hipMemcpyAsync(c.cdf.as<float>() + em.cdf_offset, cdf.data(), cdf.size() * 4, hipMemcpyHostToDevice,
                               c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));  // (cdf is a local)
    }
    // the solitary shortcut's precondition was checked against the geometry as loaded: off for good
    for (DevShape &sh : c.hshapes)
        if (sh.type == NORI_SHAPE_SPHERE) sh.solitary = 0;
    HIP_TRY(hipMemcpyAsync(c.shapes.p, c.hshapes.data(), c.hshapes.size() * sizeof(DevShape), hipMemcpyHostToDevice,
                           c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    for (int k = 0; k < 3; ++k) c.S.root_min[k] = box[k], c.S.root_max[k] = box[3 + k];
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        HIP_TRY(hipEventElapsedTime(&stats->ms_device, c.upd_ev[0], c.upd_ev[1]));
        for (int k = 0; k < 3; ++k) stats->root_min[k] = box[k], stats->root_max[k] = box[3 + k];
        stats->nodes = c.bvh_nodes;
        stats->levels = c.refit.levels();
        stats->launches = launches;
        stats->ms = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return NORI_OK;
}

// nori_gpu_rebuild_bvh (stated in nori_gpu.h): a linear BVH for the positions
// the context holds, built in the rb_* scratch buffers on the context's
// stream and swapped in at the end; until then nothing the context renders
// with is written, so every refusal and every failure leaves it as it was.
int rebuild_bvh(nori_gpu_ctx &c, const nori_gpu_rebuild_desc &rd, nori_gpu_rebuild_stats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    if (c.stack == 0)
        throw NoriException(NORI_ERR_UNSUPPORTED,
                            "nori_gpu_rebuild_bvh: a scan-mode context; create the context with NORI_TRAVERSAL=bvh");
    if (c.S.integrator == NORI_INTEGRATOR_PHOTONMAPPER)
        throw NoriException(NORI_ERR_UNSUPPORTED,
                            "nori_gpu_rebuild_bvh: a photonmapper context (its photon map was traced at creation)");
    if (rd.leaf_max > kRebuildLeafMax) throw NoriException(NORI_ERR_INVALID, "nori_gpu_rebuild_bvh: leaf_max above 64");
    for (uint32_t r : rd.reserved)
        if (r != 0) throw NoriException(NORI_ERR_INVALID, "nori_gpu_rebuild_bvh: reserved must be 0");
    const uint32_t L = rd.leaf_max ? rd.leaf_max : kRebuildLeafDefault;
    const uint32_t n = c.S.num_prims;  // (a BVH context: one record per primitive, 1 <= n < 2^25)
    if (n == 0 || n >= kRebuildMaxPrims) throw NoriException(NORI_ERR_UNSUPPORTED, "nori_gpu_rebuild_bvh: primitive count");
    HIP_TRY(hipSetDevice(c.device));
    for (auto &e : c.rb_ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    hipStream_t st = c.stream;
    auto internal = [](const char *what) {
        return NoriException(NORI_ERR_HIP, std::string("nori_gpu_rebuild_bvh: ") + what + " (nothing was changed)");
    };
    // ---- scratch, sized from n alone: a level has at most n / 2 nodes, the tree fewer than n
    size_t sort_bytes = 0, scan_bytes = 0;
    HIP_TRY(rebuild_sort_keys(nullptr, sort_bytes, nullptr, nullptr, n, st));
    HIP_TRY(rebuild_scan_counts(nullptr, scan_bytes, nullptr, nullptr, n + 1, st));
    c.rb_sort_tmp.ensure(sort_bytes);
    c.rb_scan_tmp.ensure(scan_bytes);
    c.rb_box.ensure(24);
    for (auto &b : c.rb_keys) b.ensure(8 * (size_t)n);
    for (auto &b : c.rb_ranges) b.ensure(8 * (size_t)n);
    c.rb_ends.ensure(16 * (size_t)n);
    c.rb_count.ensure(8 * ((size_t)n + 1));
    c.rb_scan.ensure(8 * ((size_t)n + 1));
    c.rb_refs.ensure(16 * (size_t)n);
    c.rb_inner.ensure(4 * (size_t)n);
    c.rb_leaf.ensure(4 * (size_t)n);
    c.rb_prims.ensure(48 * (size_t)n);
    uint32_t launches = 0;
    // ---- the scene box, then the grid on the host (one division per axis)
    HIP_TRY(hipEventRecord(c.rb_ev[0], st));
    HIP_TRY(launch_rebuild_scene_box(c.S, n, c.rb_box.as<uint32_t>(), st));
    uint32_t boxk[6];
    HIP_TRY(hipMemcpyAsync(boxk, c.rb_box.p, sizeof(boxk), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    float lo[3], scale[3];
    for (int k = 0; k < 3; ++k) {
        lo[k] = rebuild_order_value(boxk[k]);
        scale[k] = rebuild_scale(lo[k], rebuild_order_value(boxk[3 + k]));
    }
    // ---- keys, sort, records
    uint64_t *keys = c.rb_keys[0].as<uint64_t>(), *sorted = c.rb_keys[1].as<uint64_t>();
    HIP_TRY(launch_rebuild_keys(c.S, n, lo, scale, keys, st));
    HIP_TRY(rebuild_sort_keys(c.rb_sort_tmp.p, sort_bytes, keys, sorted, n, st));
    HIP_TRY(launch_rebuild_records(c.S, sorted, n, c.rb_prims.as<float4>(), st));
    launches += 3;
    // ---- topology, one breadth-first level per round
    std::vector<uint32_t> node_begin{0};  // first node of every level, then the node count
    uint32_t leaves = 0, depth = 0;
    int stack = c.stack;
    const uint32_t root_ref[4] = {kRefitLeafBit | ((n - 1) << 25), 0xffffffffu, 0xffffffffu, 0xffffffffu};
    const uint32_t zero = 0, root_range[2] = {0, n - 1};
    if (n <= L) {  // one node, one leaf slot
        HIP_TRY(hipMemcpyAsync(c.rb_refs.p, root_ref, 16, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(c.rb_leaf.p, &zero, 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        node_begin.push_back(1);
        leaves = depth = 1;
        stack = bvh_stack_for(depth, c.stack_forced);
    } else {
        HIP_TRY(hipMemcpyAsync(c.rb_ranges[0].p, root_range, 8, hipMemcpyHostToDevice, st));
        uint32_t m = 1, level_off = 0;
        int cur = 0;
        while (m) {  // (bvh_stack_for throws at the depth limit: at most 26 rounds)
            stack = bvh_stack_for(++depth, c.stack_forced);
            const uint2 *ranges = c.rb_ranges[cur].as<uint2>();
            HIP_TRY(launch_rebuild_split(sorted, ranges, m, L, c.rb_ends.as<uint4>(), c.rb_count.as<uint64_t>(), st));
            HIP_TRY(rebuild_scan_counts(c.rb_scan_tmp.p, scan_bytes, c.rb_count.as<uint64_t>(), c.rb_scan.as<uint64_t>(),
                                        m + 1, st));
            uint64_t total = 0;
            HIP_TRY(hipMemcpyAsync(&total, c.rb_scan.as<uint64_t>() + m, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            const uint64_t inner = total & 0xffffffffull, leaf = total >> 32;
            // the counts size the next launches and index the lists: checked against their bounds first
            if (inner + leaf < 2 * (uint64_t)m || inner + leaf > 4 * (uint64_t)m || (uint64_t)level_off + m + inner > n ||
                (uint64_t)leaves + leaf > n)
                throw internal("a level's slot counts are out of bounds");
            HIP_TRY(launch_rebuild_emit(ranges, c.rb_ends.as<uint4>(), c.rb_scan.as<uint64_t>(), m, level_off, leaves, L,
                                        c.rb_refs.as<uint4>(), c.rb_ranges[cur ^ 1].as<uint2>(),
                                        c.rb_inner.as<uint32_t>(), c.rb_leaf.as<uint32_t>(), st));
            launches += 2;
            level_off += m;
            node_begin.push_back(level_off);
            leaves += (uint32_t)leaf;
            m = (uint32_t)inner;
            cur ^= 1;
        }
    }
    const uint32_t N = node_begin.back();
    // ---- the nodes, and the refit schedule: level 0 = every leaf slot, then the inner slots
    // deepest level first (the inner slot of child node c is entry c - 1 of rb_inner)
    c.rb_nodes.ensure(128 * (size_t)N);
    HIP_TRY(launch_rebuild_nodes(c.rb_refs.as<uint4>(), N, c.rb_nodes.as<float4>(), st));
    ++launches;
    RefitPlan plan;  // (its host `slots` stay empty: the schedule is made on the device)
    plan.level_begin = {0, leaves};
    c.rb_slots.ensure(4 * ((size_t)leaves + N - 1));
    uint32_t *slots = c.rb_slots.as<uint32_t>();
    HIP_TRY(hipMemcpyAsync(slots, c.rb_leaf.p, 4 * (size_t)leaves, hipMemcpyDeviceToDevice, st));
    for (uint32_t d = depth - 1; d-- > 0;) {  // node level d's inner slots = the nodes of level d + 1
        const uint32_t b = node_begin[d + 1] - 1, cnt = node_begin[d + 2] - node_begin[d + 1];
        HIP_TRY(hipMemcpyAsync(slots + plan.level_begin.back(), c.rb_inner.as<uint32_t>() + b, 4 * (size_t)cnt,
                               hipMemcpyDeviceToDevice, st));
        plan.level_begin.push_back(plan.level_begin.back() + cnt);
    }
    // ---- the boxes: the refit's kernel over the new schedule
    for (uint32_t l = 0; l < plan.levels(); ++l) {
        const uint32_t b = plan.level_begin[l], cnt = plan.level_begin[l + 1] - b;
        HIP_TRY(launch_refit_level(c.rb_nodes.as<float4>(), c.rb_prims.as<float4>(), c.S.tri_vidx, c.pos.as<float4>(),
                                   slots + b, cnt, st));
        launches += cnt ? 1u : 0u;
    }
    HIP_TRY(hipEventRecord(c.rb_ev[1], st));
    float root[32], box[6];
    HIP_TRY(hipMemcpyAsync(root, c.rb_nodes.p, sizeof(root), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    refit_root_box(root, box);
    // ---- success: the new tree replaces the old one
    auto swap_buf = [](DevBuf &a, DevBuf &b) {
        std::swap(a.p, b.p);
        std::swap(a.bytes, b.bytes);
    };
    swap_buf(c.nodes, c.rb_nodes);
    swap_buf(c.prims, c.rb_prims);
    swap_buf(c.refit_slots, c.rb_slots);
    c.refit = std::move(plan);
    c.S.nodes = c.nodes.as<float4>();
    c.S.prims = c.prims.as<float4>();
    c.S.num_nodes = N;
    c.bvh_nodes = N;
    c.bvh_depth = depth;
    c.stack = stack;
    c.scene_bytes = 128 * (size_t)N + 48 * (size_t)n;
    for (int k = 0; k < 3; ++k) c.S.root_min[k] = box[k], c.S.root_max[k] = box[3 + k];
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        HIP_TRY(hipEventElapsedTime(&stats->ms_device, c.rb_ev[0], c.rb_ev[1]));
        stats->nodes = N;
        stats->depth = depth;
        stats->stack = (uint32_t)stack;
        stats->levels = c.refit.levels();
        stats->launches = launches;
        stats->ms = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return NORI_OK;
}

int bvh_read(nori_gpu_ctx &c, float *nodes, float *prims, uint32_t *counts) {
    HIP_TRY(hipSetDevice(c.device));
    if (counts) counts[0] = c.S.num_nodes, counts[1] = c.S.num_prims;
    HIP_TRY(hipStreamSynchronize(c.stream));
    if (nodes) HIP_TRY(hipMemcpy(nodes, c.nodes.p, 128 * (size_t)c.S.num_nodes, hipMemcpyDeviceToHost));
    if (prims) HIP_TRY(hipMemcpy(prims, c.prims.p, 48 * (size_t)c.S.num_prims, hipMemcpyDeviceToHost));
    return NORI_OK;
}

int frame_blocks(const nori_gpu_ctx &c, int *nbx_out = nullptr) {
    const int nbx = (c.S.W + NORI_BLOCK_SIZE - 1) / NORI_BLOCK_SIZE, nby = (c.S.H + NORI_BLOCK_SIZE - 1) / NORI_BLOCK_SIZE;
    if (nbx_out) *nbx_out = nbx;
    return nbx * nby;
}

// nori_gpu_block_error: the metric of `stats` for every block of the frame.
int block_error(nori_gpu_ctx &c, const float *stats, bool on_device, float *errors) {
    HIP_TRY(hipSetDevice(c.device));
    int nbx = 0;
    const int nb = frame_blocks(c, &nbx);
    const size_t n = 8 * (size_t)c.S.W * (size_t)c.S.H;
    const float *dev = stats;
    if (on_device) {
        if ((uintptr_t)stats % 16) throw NoriException(NORI_ERR_INVALID, "device statistics must be 16-byte aligned");
    } else {
        c.varbuf.ensure(n * sizeof(float));
        HIP_TRY(hipMemcpyAsync(c.varbuf.p, stats, n * sizeof(float), hipMemcpyHostToDevice, c.stream));
        dev = c.varbuf.as<float>();
    }
    c.errbuf.ensure((size_t)nb * sizeof(float));
    HIP_TRY(launch_block_error(dev, c.S.W, c.S.H, nbx, nullptr, (uint32_t)nb, c.errbuf.as<float>(), c.stream));
    HIP_TRY(hipMemcpyAsync(errors, c.errbuf.p, (size_t)nb * sizeof(float), hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    return NORI_OK;
}

// nori_gpu_render_adaptive (nori_gpu.h has the schedule): one render() per
// round on the blocks still active, film and statistics resident on the
// device throughout; per round only the block errors come back.
int render_adaptive(nori_gpu_ctx &c, const nori_gpu_render_desc &rd0, const nori_gpu_adaptive_desc &ad, float *rgbw_out,
                    nori_gpu_stats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(c.device));
    const uint32_t cap = ad.max_passes ? ad.max_passes : c.spp;
    if (ad.min_passes < 2) throw NoriException(NORI_ERR_INVALID, "adaptive: min_passes must be at least 2");
    if (cap < ad.min_passes) throw NoriException(NORI_ERR_INVALID, "adaptive: the pass cap is below min_passes");
    if (!(ad.threshold >= 0.0f)) throw NoriException(NORI_ERR_INVALID, "adaptive: threshold is negative or NaN");
    if (ad.reserved != 0) throw NoriException(NORI_ERR_INVALID, "adaptive: reserved must be 0");
    if ((uint64_t)rd0.pass_begin + cap > 0xFFFFFFFFull) throw NoriException(NORI_ERR_INVALID, "adaptive: pass range overflows");
    const int W = c.S.W, H = c.S.H, B = c.S.border;
    int nbx = 0;
    const uint32_t nb = (uint32_t)frame_blocks(c, &nbx);
    // the selected blocks, ascending, duplicates dropped
    std::vector<uint32_t> active;
    if (rd0.num_blocks) {
        std::vector<char> want(nb, 0);
        for (uint32_t i = 0; i < rd0.num_blocks; ++i) {
            if (rd0.block_ids[i] >= nb) throw NoriException(NORI_ERR_INVALID, "block id out of range");
            want[rd0.block_ids[i]] = 1;
        }
        for (uint32_t b = 0; b < nb; ++b)
            if (want[b]) active.push_back(b);
    } else {
        active.resize(nb);
        for (uint32_t b = 0; b < nb; ++b) active[b] = b;
    }
    auto block_pixels = [&](uint32_t b) {
        const int ox = (int)(b % (uint32_t)nbx) * NORI_BLOCK_SIZE, oy = (int)(b / (uint32_t)nbx) * NORI_BLOCK_SIZE;
        return (uint64_t)std::min(NORI_BLOCK_SIZE, W - ox) * (uint64_t)std::min(NORI_BLOCK_SIZE, H - oy);
    };
    auto pixels_of = [&](const std::vector<uint32_t> &ids) {
        uint64_t m = 0;
        for (uint32_t b : ids) m += block_pixels(b);
        return m;
    };
    const double bound = (double)cap * (double)pixels_of(active);  // samples if no block stops early

    const size_t film_elems = 4 * (size_t)(W + 2 * B) * (H + 2 * B), var_elems = 8 * (size_t)W * (size_t)H;
    float *film = rgbw_out;
    if (!rd0.output_on_device) {
        c.film.ensure(film_elems * sizeof(float));
        film = c.film.as<float>();
        HIP_TRY(hipMemsetAsync(film, 0, film_elems * sizeof(float), c.stream));
    }
    c.varbuf.ensure(var_elems * sizeof(float));
    c.errbuf.ensure((size_t)nb * sizeof(float));
    c.errids.ensure((size_t)nb * sizeof(uint32_t));
    HIP_TRY(hipMemsetAsync(c.varbuf.p, 0, var_elems * sizeof(float), c.stream));
    HIP_TRY(hipMemsetAsync(c.errbuf.p, 0, (size_t)nb * sizeof(float), c.stream));

    struct Rounds {  // the context reports plain renders as before once the call is over
        nori_gpu_ctx &c;
        explicit Rounds(nori_gpu_ctx &ctx) : c(ctx) {
            c.in_rounds = true;
            c.prog_off = c.prog_scale = 0.0;
        }
        ~Rounds() {
            c.progress = 1.0f;
            c.in_rounds = false;
            c.prog_off = 0.0;
            c.prog_scale = 1.0;
        }
    } rounds(c);
    c.cancel = 0;
    c.progress = 0.0f;

    std::vector<uint32_t> passes(nb, 0);
    std::vector<float> herr(nb, 0.0f);
    nori_gpu_stats sum{}, rs{};
    uint32_t have = 0, np = ad.min_passes;
    while (!active.empty()) {
        if (c.cancel.load()) return fail(NORI_ERR_CANCELLED, "rendering was cancelled");
        const double round_samples = (double)np * (double)pixels_of(active);
        c.prog_off += c.prog_scale;  // where the last round ended, to the bit: the progress never steps back
        c.prog_scale = round_samples / bound;
        nori_gpu_render_desc rd = rd0;
        rd.pass_begin = rd0.pass_begin + have;
        rd.pass_count = np;
        rd.num_blocks = (uint32_t)active.size();
        rd.block_ids = active.data();
        rd.output_on_device = 1;
        rd.variance_out = c.varbuf.as<float>();
        const int rc = render(c, rd, film, &rs);
        if (rc != NORI_OK) return rc;
        sum.samples += rs.samples;
        sum.invalid_samples += rs.invalid_samples;
        sum.rays_closest += rs.rays_closest;
        sum.rays_shadow += rs.rays_shadow;
        sum.rays_finish += rs.rays_finish;
        sum.iterations += rs.iterations;
        sum.ms_extend += rs.ms_extend;
        sum.ms_shadow += rs.ms_shadow;
        sum.ms_shade += rs.ms_shade;
        sum.ms_splat += rs.ms_splat;
        sum.ms_finish += rs.ms_finish;
        have += np;
        for (uint32_t b : active) passes[b] = have;
        // E_b of the blocks just rendered (the others' statistics did not change)
        HIP_TRY(hipMemcpyAsync(c.errids.p, active.data(), active.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
        HIP_TRY(launch_block_error(c.varbuf.as<float>(), W, H, nbx, c.errids.as<uint32_t>(), (uint32_t)active.size(),
                                   c.errbuf.as<float>(), c.stream));
        HIP_TRY(hipMemcpyAsync(herr.data(), c.errbuf.p, (size_t)nb * sizeof(float), hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));  // (also orders the pageable upload of `active` before it changes)
        if (have >= cap) break;
        std::vector<uint32_t> next;
        for (uint32_t b : active)
            if (herr[b] > ad.threshold) next.push_back(b);
        active.swap(next);
        np = std::min(have, cap - have);
    }
    if (c.cancel.load()) return fail(NORI_ERR_CANCELLED, "rendering was cancelled");

    if (!rd0.output_on_device) {
        std::vector<float> hf(std::max(film_elems, var_elems));
        HIP_TRY(hipMemcpy(hf.data(), film, film_elems * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < film_elems; ++i) rgbw_out[i] += hf[i];
        if (rd0.variance_out) {
            HIP_TRY(hipMemcpy(hf.data(), c.varbuf.p, var_elems * sizeof(float), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < var_elems; ++i) rd0.variance_out[i] += hf[i];
        }
    } else if (rd0.variance_out) {
        HIP_TRY(launch_add_into(rd0.variance_out, c.varbuf.as<float>(), var_elems, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
    }
    if (ad.passes_out) std::copy(passes.begin(), passes.end(), ad.passes_out);
    if (ad.error_out) std::copy(herr.begin(), herr.end(), ad.error_out);
    c.progress = 1.0f;
    if (stats) {
        *stats = rs;  // the scene and pool fields of the last round
        stats->samples = sum.samples;
        stats->invalid_samples = sum.invalid_samples;
        stats->rays_closest = sum.rays_closest;
        stats->rays_shadow = sum.rays_shadow;
        stats->rays_finish = sum.rays_finish;
        stats->iterations = sum.iterations;
        stats->ms_extend = sum.ms_extend;
        stats->ms_shadow = sum.ms_shadow;
        stats->ms_shade = sum.ms_shade;
        stats->ms_splat = sum.ms_splat;
        stats->ms_finish = sum.ms_finish;
        stats->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return NORI_OK;
}

}  // namespace

// ------------------------------------------------------------------ C ABI
namespace {

// This rank's share of a whole-frame render (nori_gpu_shard_desc).  The pass
// count defaults to the scene's sampleCount (0 -> 1) in both entry points, and
// a block list is checked (range) and de-duplicated in both modes, so the
// share always fits the caller's block_buf (capacity = the frame's blocks).
nori_gpu_render_desc shard_of(int W, int H, uint32_t spp, const nori_gpu_render_desc &whole, int mode, int nranks,
                              int rank, std::vector<uint32_t> &blocks) {
    if (nranks < 1 || rank < 0 || rank >= nranks) throw NoriException(NORI_ERR_INVALID, "shard: rank out of range");
    if (mode != NORI_SHARD_PASSES && mode != NORI_SHARD_BLOCKS) throw NoriException(NORI_ERR_INVALID, "shard: unknown mode");
    nori_gpu_render_desc out = whole;
    const uint32_t P = whole.pass_count ? whole.pass_count : std::max<uint32_t>(spp, 1u);
    const uint32_t nb = (uint32_t)(((W + NORI_BLOCK_SIZE - 1) / NORI_BLOCK_SIZE) * ((H + NORI_BLOCK_SIZE - 1) / NORI_BLOCK_SIZE));
    std::vector<char> want(nb, whole.num_blocks ? 0 : 1);
    for (uint32_t i = 0; i < whole.num_blocks; ++i) {
        if (whole.block_ids[i] >= nb) throw NoriException(NORI_ERR_INVALID, "block id out of range");
        want[whole.block_ids[i]] = 1;
    }
    blocks.clear();
    if (mode == NORI_SHARD_PASSES) {
        const uint64_t a = (uint64_t)P * rank / nranks, b = (uint64_t)P * (rank + 1) / nranks;
        out.pass_begin = whole.pass_begin + (uint32_t)a;
        out.pass_count = (uint32_t)(b - a);
        if (whole.num_blocks)  // the restricted frame, each block once, in the caller's order
            for (uint32_t i = 0; i < whole.num_blocks; ++i)
                if (want[whole.block_ids[i]]) {
                    blocks.push_back(whole.block_ids[i]);
                    want[whole.block_ids[i]] = 0;
                }
    } else {
        uint32_t k = 0;  // round-robin over the spiral order (block.cpp:140-188)
        for (uint32_t b : spiral_blocks(W, H))
            if (want[b] && (k++ % (uint32_t)nranks) == (uint32_t)rank) blocks.push_back(b);
        out.pass_count = blocks.empty() ? 0 : P;  // no block of this rank: an empty share
    }
    out.num_blocks = (uint32_t)blocks.size();
    out.block_ids = blocks.empty() ? nullptr : blocks.data();
    return out;
}

// Samples of a share (pass count x pixels of its blocks, or of the image).
double share_samples(int W, int H, const nori_gpu_render_desc &s) {
    if (!s.num_blocks) return (double)s.pass_count * W * H;
    const int nx = (W + NORI_BLOCK_SIZE - 1) / NORI_BLOCK_SIZE;
    double px = 0;
    for (uint32_t i = 0; i < s.num_blocks; ++i) {
        const int bx = (int)(s.block_ids[i] % (uint32_t)nx), by = (int)(s.block_ids[i] / (uint32_t)nx);
        px += (double)std::min(NORI_BLOCK_SIZE, W - bx * NORI_BLOCK_SIZE) * std::min(NORI_BLOCK_SIZE, H - by * NORI_BLOCK_SIZE);
    }
    return px * s.pass_count;
}

// Watchdog of the collectives of a sharded render: how long a rank waits in
// the status exchange or the film sum for its peers before it aborts the
// communicator.  Only a peer that cannot join at all (its device faulted,
// its process died) is waited for: every other failure reaches the peers
// through the status exchange.  NORI_COMM_TIMEOUT_S fixes the bound;
// otherwise, for a rank that rendered its share (status NORI_OK), it scales
// with the frame: max(30 s, 20 x this rank's own render time x largest share
// / own share), since every peer renders a share of about the same size with
// the same code.  A rank whose own render failed or was cancelled, or that
// has no share, has no render time that says how long its peers need: it
// waits up to 600 s.
double comm_timeout_s(int status, double own_s, double own_samples, double max_samples) {
    if (const char *e = std::getenv("NORI_COMM_TIMEOUT_S")) {
        const double v = std::atof(e);
        if (v > 0.0) return v;
    }
    if (status != NORI_OK || !(own_samples > 0.0)) return 600.0;
    return std::max(30.0, 20.0 * own_s * std::max(1.0, max_samples / own_samples));
}

// Status word of the exchange: severity << 16 | rank, reduced by max over the
// ranks, so the worst outcome wins and names its rank (the highest of equals).
// Severity 0 rendered, 1 cancelled, 2 failed.
int comm_status_word(int rc, int rank) {
    const int sev = rc == NORI_OK ? 0 : (rc == NORI_ERR_CANCELLED ? 1 : 2);
    return (sev << 16) | (rank & 0xFFFF);
}

}  // namespace

extern "C" {

const char *nori_gpu_last_error(void) { return g_last_error.c_str(); }

// denoiser/denoiser.py (NL-means over a rendered image and its per-pixel
// variance) on device `device`: host buffers in, host buffer out.
int nori_denoise(int device, const float *rgb, const float *variance, int width, int height, int radius, int patch,
                 float k, int mode, float *out) {
    return guarded([&] {
        if (!rgb || !variance || !out || width <= 0 || height <= 0 || radius < 0 || radius > 8 || patch < 1 ||
            patch > 5 || mode < 0 || mode > 1 || !(k > 0.0f))
            return fail(NORI_ERR_INVALID, "nori_denoise: invalid arguments");
        HIP_TRY(hipSetDevice(device));
        {  // the tile + halo staging must fit one work-group's LDS
            int lds_max = 0;
            HIP_TRY(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
            const size_t need = denoise_lds_bytes(radius, patch - 1);
            if (need > (size_t)lds_max)
                return fail(NORI_ERR_INVALID, "nori_denoise: radius " + std::to_string(radius) + " / patch " +
                                                  std::to_string(patch) + " need " + std::to_string(need) +
                                                  " bytes of LDS per work-group, the device has " +
                                                  std::to_string(lds_max));
        }
        const size_t n = (size_t)width * (size_t)height;
        DevBuf di, dv, dout;
        di.ensure(12 * n);
        dv.ensure(4 * n);
        dout.ensure(12 * n);
        HIP_TRY(hipMemcpy(di.p, rgb, 12 * n, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dv.p, variance, 4 * n, hipMemcpyHostToDevice));
        HIP_TRY(launch_denoise((const float *)di.p, (const float *)dv.p, width, height, radius, patch - 1, k, mode,
                               (float *)dout.p, nullptr));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(out, dout.p, 12 * n, hipMemcpyDeviceToHost));
        return (int)NORI_OK;
    });
}
// The feature-guided denoiser (nori_film_denoise_guided states it) on device
// `device`: host buffers in, host buffer out.
int nori_denoise_guided(int device, const float *rgb, const float *variance, const float *feat7, int width, int height,
                        const nori_guided_desc *d, float *out) {
    return guarded([&] {
        if (!rgb || !variance || !feat7 || !out || width <= 0 || height <= 0 || !guided_desc_valid(d))
            return fail(NORI_ERR_INVALID, "nori_denoise_guided: invalid arguments");
        HIP_TRY(hipSetDevice(device));
        {  // the tile + halo staging must fit one work-group's LDS
            int lds_max = 0;
            HIP_TRY(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
            const size_t need = guided_lds_bytes(d->radius, d->patch);
            if (need > (size_t)lds_max)
                return fail(NORI_ERR_INVALID, "nori_denoise_guided: radius " + std::to_string(d->radius) + " / patch " +
                                                  std::to_string(d->patch) + " need " + std::to_string(need) +
                                                  " bytes of LDS per work-group, the device has " +
                                                  std::to_string(lds_max));
        }
        const size_t n = (size_t)width * (size_t)height;
        DevBuf di, dv, df, dout;
        di.ensure(12 * n);
        dv.ensure(4 * n);
        df.ensure(28 * n);
        dout.ensure(12 * n);
        HIP_TRY(hipMemcpy(di.p, rgb, 12 * n, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dv.p, variance, 4 * n, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(df.p, feat7, 28 * n, hipMemcpyHostToDevice));
        HIP_TRY(launch_guided((const float *)di.p, (const float *)dv.p, (const float *)df.p, width, height, d->radius,
                              d->patch, d->k, d->eps, d->sigma_albedo, d->sigma_normal, d->sigma_depth,
                              (float *)dout.p, nullptr));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(out, dout.p, 12 * n, hipMemcpyDeviceToHost));
        return (int)NORI_OK;
    });
}
int nori_gpu_abi_version(void) { return NORI_GPU_ABI_VERSION; }

int nori_read_image(const char *path, int *width, int *height, uint8_t *rgb) {
    return guarded([&] {
        if (!path || !width || !height) return fail(NORI_ERR_INVALID, "null argument");
        int w = 0, h = 0;
        std::vector<uint8_t> img;
        decode_image_rgb8(path, w, h, img);
        *width = w;
        *height = h;
        if (rgb) std::memcpy(rgb, img.data(), img.size());
        return NORI_OK;
    });
}

int nori_scene_load_xml(const char *path, int width, int height, int spp, nori_scene **out) {
    return guarded([&] {
        if (!path || !out) return fail(NORI_ERR_INVALID, "null argument");
        auto *s = new nori_scene;
        s->hs.reset(load_scene_xml(path, width, height, spp));
        *out = s;
        return NORI_OK;
    });
}
const nori_scene_desc *nori_scene_get_desc(const nori_scene *s) { return s ? &s->hs->desc : nullptr; }

int nori_scene_bvh_info(const nori_scene_desc *d, nori_bvh_info *out) {
    return guarded([&] {
        if (!d || !out) return fail(NORI_ERR_INVALID, "null argument");
        if (d->abi_version != NORI_GPU_ABI_VERSION) return fail(NORI_ERR_INVALID, "ABI version mismatch");
        float rmin[3], rmax[3];
        scene_root_box(*d, rmin, rmax);
        DeviceBvh bvh;
        build_device_bvh(*d, rmin, rmax, bvh);
        std::memset(out, 0, sizeof(*out));
        out->ref_nodes = bvh.ref_nodes;
        out->device_nodes = bvh.num_nodes;
        out->depth = bvh.depth;
        out->num_prims = (uint32_t)(bvh.prims.size() / 12);
        out->sah_cost = bvh.sah_cost;
        uint64_t h = 1469598103934665603ull;
        for (size_t i = 0; i < bvh.prims.size(); i += 12) {
            uint32_t id;
            std::memcpy(&id, &bvh.prims[i + 3], 4);
            for (int k = 0; k < 4; ++k) h = (h ^ ((id >> (8 * k)) & 0xFFu)) * 1099511628211ull;
        }
        out->order_hash = h;
        return NORI_OK;
    });
}
int nori_scene_scan_rtc(const nori_scene_desc *d, const char *arch, size_t *code_bytes, double *ms) {
    return guarded([&] {
        if (!d || !arch || !code_bytes || !ms) return fail(NORI_ERR_INVALID, "null argument");
        if (d->abi_version != NORI_GPU_ABI_VERSION) return fail(NORI_ERR_INVALID, "ABI version mismatch");
        float rmin[3], rmax[3];
        scene_root_box(*d, rmin, rmax);
        DeviceBvh bvh;
        build_device_bvh(*d, rmin, rmax, bvh);
        const uint32_t n = (uint32_t)(bvh.prims.size() / 12);
        *code_bytes = 0;
        *ms = 0.0;
        if (n > kScanMaxPrims) return NORI_OK;  // a BVH scene: nothing to specialise
        const ScanList L = build_scan_list(bvh, n);
        ScanRtcScene sc{L.prims.data(), (uint32_t)(L.prims.size() / 12), L.plane_c.data(), L.plane_f.data(),
                        (uint32_t)L.plane_c.size(), {L.plane_end[0], L.plane_end[1], L.plane_end[2]}, L.tris, L.real};
        std::vector<char> code;
        bool cached = false;
        std::string why;
        if (!rtc_compile(sc, arch, 1, code, *ms, cached, why)) return fail(NORI_ERR_UNSUPPORTED, why);
        *code_bytes = code.size();
        return NORI_OK;
    });
}
int nori_scene_shade_rtc(const nori_scene_desc *d, const char *arch, size_t *code_bytes, double *ms) {
    return guarded([&] {
        if (!d || !arch || !code_bytes || !ms) return fail(NORI_ERR_INVALID, "null argument");
        if (d->abi_version != NORI_GPU_ABI_VERSION) return fail(NORI_ERR_INVALID, "ABI version mismatch");
        float rmin[3], rmax[3];
        scene_root_box(*d, rmin, rmax);
        DeviceBvh bvh;
        build_device_bvh(*d, rmin, rmax, bvh);
        const uint32_t n = (uint32_t)(bvh.prims.size() / 12);
        *code_bytes = 0;
        *ms = 0.0;
        // (the traversal as nori_gpu_create chooses it, NORI_TRAVERSAL included)
        const char *mode = std::getenv("NORI_TRAVERSAL");
        bool scan = n <= kScanMaxPrims;
        if (mode && std::string(mode) == "bvh") scan = false;
        if (mode && std::string(mode) == "scan") scan = true;
        if (!scan) return NORI_OK;
        const ScanList L = build_scan_list(bvh, n);
        if (!shade_rtc_scene(*d, scan, L.prims.size() / 12)) return NORI_OK;  // the ahead-of-time kernel serves it
        ScanRtcScene sc{L.prims.data(), (uint32_t)(L.prims.size() / 12), L.plane_c.data(), L.plane_f.data(),
                        (uint32_t)L.plane_c.size(), {L.plane_end[0], L.plane_end[1], L.plane_end[2]}, L.tris, L.real};
        const size_t blob = scene_blob_bytes(*d, L.prims.size(), bvh.nodes.size());
        const bool lds = blob <= kBlobMaxBytes && shade_lds_bytes((uint32_t)blob) != 0;
        std::vector<char> code;
        bool cached = false;
        std::string why;
        if (!rtc_compile_shade(sc, arch, shade_integrator(d->integrator), lds, code, *ms, cached, why))
            return fail(NORI_ERR_UNSUPPORTED, why);
        *code_bytes = code.size();
        return NORI_OK;
    });
}
int nori_gpu_shade_rtc_info(nori_gpu_ctx *c, int *active, int *cached, double *ms, size_t *code_bytes) {
    return guarded([&] {
        if (!c) return fail(NORI_ERR_INVALID, "null argument");
        if (active) *active = c->shade_rtc.shade ? 1 : 0;
        if (cached) *cached = c->shade_rtc.cached ? 1 : 0;
        if (ms) *ms = c->shade_rtc.compile_ms;
        if (code_bytes) *code_bytes = c->shade_rtc.code_bytes;
        return NORI_OK;
    });
}
int nori_scene_scan_list(const nori_scene_desc *d, nori_scan_info *info, float *records, float *plane_c,
                         float *plane_f) {
    return guarded([&] {
        if (!d || !info) return fail(NORI_ERR_INVALID, "null argument");
        if (d->abi_version != NORI_GPU_ABI_VERSION) return fail(NORI_ERR_INVALID, "ABI version mismatch");
        float rmin[3], rmax[3];
        scene_root_box(*d, rmin, rmax);
        DeviceBvh bvh;
        build_device_bvh(*d, rmin, rmax, bvh);
        const uint32_t n = (uint32_t)(bvh.prims.size() / 12);
        std::memset(info, 0, sizeof(*info));
        if (n > kScanMaxPrims) return NORI_OK;  // a BVH scene: no scan list
        const ScanList L = build_scan_list(bvh, n);
        info->records = (uint32_t)(L.prims.size() / 12);
        info->pairs = (uint32_t)L.plane_c.size();
        for (int a = 0; a < 3; ++a) info->plane_end[a] = L.plane_end[a];
        info->tris = L.tris;
        if (records) std::memcpy(records, L.prims.data(), L.prims.size() * 4);
        if (plane_c && !L.plane_c.empty()) std::memcpy(plane_c, L.plane_c.data(), L.plane_c.size() * 4);
        if (plane_f && !L.plane_f.empty()) std::memcpy(plane_f, L.plane_f.data(), L.plane_f.size() * 4);
        return NORI_OK;
    });
}
void nori_scene_free(nori_scene *s) { delete s; }

int nori_film_border(const nori_scene_desc *d) { return d ? film_border(d->camera) : NORI_ERR_INVALID; }
int nori_filter_table(const nori_scene_desc *d, float *table) {
    if (!d || !table) return fail(NORI_ERR_INVALID, "null argument");
    filter_table(d->camera, table);
    return NORI_OK;
}
int nori_film_develop(const nori_scene_desc *d, const float *rgbw, float *rgb) {
    if (!d || !rgbw || !rgb) return fail(NORI_ERR_INVALID, "null argument");
    int W = d->camera.width, H = d->camera.height, B = film_border(d->camera), FW = W + 2 * B;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const float *c = rgbw + 4 * ((size_t)(y + B) * FW + (x + B));
            float *o = rgb + 3 * ((size_t)y * W + x);
            for (int k = 0; k < 3; ++k) o[k] = c[3] != 0 ? c[k] / c[3] : 0.0f;  // color.h:113-118
        }
    return NORI_OK;
}

int nori_gpu_device_count(int *count) {
    return guarded([&] {
        if (!count) return fail(NORI_ERR_INVALID, "null argument");
        int n = 0;
        hipError_t e = hipGetDeviceCount(&n);
        *count = e == hipSuccess ? n : 0;
        return NORI_OK;
    });
}

int nori_gpu_create(const nori_scene_desc *d, int device, nori_gpu_ctx **out) {
    return guarded([&] {
        if (!d || !out) return fail(NORI_ERR_INVALID, "null argument");
        if (d->abi_version != NORI_GPU_ABI_VERSION) return fail(NORI_ERR_INVALID, "scene desc ABI version mismatch");
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(NORI_ERR_HIP, "no HIP device available");
        if (device < 0 || device >= n) return fail(NORI_ERR_INVALID, "device index out of range");
        HIP_TRY(hipSetDevice(device));
        std::unique_ptr<nori_gpu_ctx> c(new nori_gpu_ctx);
        c->device = device;
        c->spp = d->sample_count ? d->sample_count : 1;
        if (const char *e = std::getenv("NORI_FINISH_FIRST"); e && e[0] == '0') c->finish_first = false;
        HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
        for (int h = 1; h < kMaxParts; ++h) {
            HIP_TRY(hipStreamCreateWithFlags(&c->parts[h], hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&c->joins[h], hipEventDisableTiming));
        }
        HIP_TRY(hipEventCreateWithFlags(&c->fork, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&c->join, hipEventDisableTiming));
        upload_scene(*c, *d);
        if (d->integrator == NORI_INTEGRATOR_PHOTONMAPPER) photon_preprocess(*c, *d);
        *out = c.release();
        return NORI_OK;
    });
}

int nori_gpu_render(nori_gpu_ctx *c, const nori_gpu_render_desc *rd, float *rgbw_out, nori_gpu_stats *stats) {
    return guarded([&] {
        if (!c || !rd || !rgbw_out) return fail(NORI_ERR_INVALID, "null argument");
        if (rd->num_blocks && !rd->block_ids) return fail(NORI_ERR_INVALID, "block_ids is null");
        return render(*c, *rd, rgbw_out, stats);
    });
}

int nori_gpu_render_features(nori_gpu_ctx *c, const nori_gpu_render_desc *rd, float *features, nori_gpu_stats *stats) {
    return guarded([&] {
        if (!c || !rd || !features) return fail(NORI_ERR_INVALID, "null argument");
        if (rd->num_blocks && !rd->block_ids) return fail(NORI_ERR_INVALID, "block_ids is null");
        return render_features(*c, *rd, features, stats);
    });
}

int nori_gpu_block_error(nori_gpu_ctx *c, const float *stats, int stats_on_device, float *errors) {
    return guarded([&] {
        if (!c || !stats || !errors) return fail(NORI_ERR_INVALID, "null argument");
        return block_error(*c, stats, stats_on_device != 0, errors);
    });
}

int nori_gpu_render_adaptive(nori_gpu_ctx *c, const nori_gpu_render_desc *rd, const nori_gpu_adaptive_desc *ad,
                             float *rgbw_out, nori_gpu_stats *stats) {
    return guarded([&] {
        if (!c || !rd || !ad || !rgbw_out) return fail(NORI_ERR_INVALID, "null argument");
        if (rd->num_blocks && !rd->block_ids) return fail(NORI_ERR_INVALID, "block_ids is null");
        return render_adaptive(*c, *rd, *ad, rgbw_out, stats);
    });
}

int nori_gpu_trace(nori_gpu_ctx *c, const float *rays, uint32_t n, int any_hit, nori_gpu_hit *hits) {
    return guarded([&] {
        if (!c || !rays || !hits) return fail(NORI_ERR_INVALID, "null argument");
        if (n == 0) return NORI_OK;
        HIP_TRY(hipSetDevice(c->device));
        DevBuf r, h;
        r.ensure(32 * (size_t)n);
        h.ensure(16 * (size_t)n);
        HIP_TRY(hipMemcpy(r.p, rays, 32 * (size_t)n, hipMemcpyHostToDevice));
        HIP_TRY(launch_trace(c->S, r.as<float4>(), n, any_hit, h.as<float4>(), c->stack, c->stream, &c->rtc));
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(hits, h.p, 16 * (size_t)n, hipMemcpyDeviceToHost));
        return NORI_OK;
    });
}

int nori_gpu_query(nori_gpu_ctx *c, const nori_gpu_query_desc *qd, const float *rays, nori_gpu_hit *hits,
                   nori_gpu_surface *surf, nori_gpu_stats *stats) {
    return guarded([&] {
        if (!c || !qd || !rays) return fail(NORI_ERR_INVALID, "null argument");
        if (!hits && !surf) return fail(NORI_ERR_INVALID, "nori_gpu_query: hits and surf are both null");
        if (qd->any_hit && surf) return fail(NORI_ERR_INVALID, "nori_gpu_query: an any-hit query has no hit record (surf must be NULL)");
        if (qd->reserved != 0) return fail(NORI_ERR_INVALID, "nori_gpu_query: reserved must be 0");
        if (qd->on_device && ((uintptr_t)rays % 16 || (uintptr_t)hits % 16 || (uintptr_t)surf % 16))
            return fail(NORI_ERR_INVALID, "nori_gpu_query: device pointers must be 16-byte aligned");
        if (qd->n == 0) return NORI_OK;
        return query(*c, *qd, rays, hits, surf, stats);
    });
}

int nori_gpu_camera_rays(nori_gpu_ctx *c, const nori_gpu_render_desc *rd, float *rays) {
    return guarded([&] {
        if (!c || !rd || !rays) return fail(NORI_ERR_INVALID, "null argument");
        if (rd->num_blocks && !rd->block_ids) return fail(NORI_ERR_INVALID, "block_ids is null");
        return camera_rays(*c, *rd, rays);
    });
}

int nori_gpu_bsdf_eval(nori_gpu_ctx *c, const nori_gpu_shading_desc *sd, const nori_gpu_surface *surf, const float *wi,
                       const float *wo, float *out) {
    return guarded([&] {
        if (!c || !sd || !surf || !wi || !wo || !out) return fail(NORI_ERR_INVALID, "null argument");
        if (sd->reserved != 0) return fail(NORI_ERR_INVALID, "nori_gpu_bsdf_eval: reserved must be 0");
        if (sd->n == 0) return NORI_OK;
        if (!sd->on_device) check_host_records(*c, "nori_gpu_bsdf_eval", surf, sd->n);
        const uint32_t shapes = (uint32_t)c->hshapes.size();
        return shading_call(*c, "nori_gpu_bsdf_eval", *sd, {{surf, 64, 16}, {wi, 12, 4}, {wo, 12, 4}}, out, 32,
                            [&](const void *const *d, void *o, uint32_t m) {
                                return launch_bsdf_eval(c->S, shapes, (const float4 *)d[0], (const float *)d[1],
                                                        (const float *)d[2], m, (float4 *)o, c->stream);
                            });
    });
}

int nori_gpu_bsdf_sample(nori_gpu_ctx *c, const nori_gpu_shading_desc *sd, const nori_gpu_surface *surf, const float *wi,
                         const float *u, float *out) {
    return guarded([&] {
        if (!c || !sd || !surf || !wi || !u || !out) return fail(NORI_ERR_INVALID, "null argument");
        if (sd->reserved != 0) return fail(NORI_ERR_INVALID, "nori_gpu_bsdf_sample: reserved must be 0");
        if (sd->n == 0) return NORI_OK;
        if (!sd->on_device) check_host_records(*c, "nori_gpu_bsdf_sample", surf, sd->n);
        const uint32_t shapes = (uint32_t)c->hshapes.size();
        return shading_call(*c, "nori_gpu_bsdf_sample", *sd, {{surf, 64, 16}, {wi, 12, 4}, {u, 8, 4}}, out, 32,
                            [&](const void *const *d, void *o, uint32_t m) {
                                return launch_bsdf_sample(c->S, shapes, (const float4 *)d[0], (const float *)d[1],
                                                          (const float *)d[2], m, (float4 *)o, c->stream);
                            });
    });
}

int nori_gpu_emitter_sample(nori_gpu_ctx *c, const nori_gpu_shading_desc *sd, const int32_t *ids, const float *x,
                            const float *u, float *out) {
    return guarded([&] {
        if (!c || !sd || !x || !u || !out) return fail(NORI_ERR_INVALID, "null argument");
        if (sd->reserved != 0) return fail(NORI_ERR_INVALID, "nori_gpu_emitter_sample: reserved must be 0");
        if (sd->n == 0) return NORI_OK;
        const int32_t ne = (int32_t)c->S.num_emitters;
        // host arrays: the host can look at every id (device arrays: the kernel's guard gives zeros)
        if (!sd->on_device && !ids && (sd->emitter < 0 || sd->emitter >= ne))
            return fail(NORI_ERR_INVALID, "nori_gpu_emitter_sample: desc->emitter " + std::to_string(sd->emitter) +
                                              " is outside the scene's " + std::to_string(ne) + " emitters");
        if (!sd->on_device && ids)
            for (uint32_t i = 0; i < sd->n; ++i)
                if (ids[i] < 0 || ids[i] >= ne)
                    return fail(NORI_ERR_INVALID, "nori_gpu_emitter_sample: ids[" + std::to_string(i) + "] = " +
                                                      std::to_string(ids[i]) + " is outside the scene's " +
                                                      std::to_string(ne) + " emitters");
        return shading_call(*c, "nori_gpu_emitter_sample", *sd, {{ids, 4, 4}, {x, 12, 4}, {u, 8, 4}}, out, 48,
                            [&](const void *const *d, void *o, uint32_t m) {
                                return launch_emitter_sample(c->S, (const int32_t *)d[0], sd->emitter, (const float *)d[1],
                                                             (const float *)d[2], m, (float4 *)o, c->stream);
                            });
    });
}

int nori_gpu_emitter_eval(nori_gpu_ctx *c, const nori_gpu_shading_desc *sd, const nori_gpu_surface *surf,
                          const float *from, float *out) {
    return guarded([&] {
        if (!c || !sd || !surf || !from || !out) return fail(NORI_ERR_INVALID, "null argument");
        if (sd->reserved != 0) return fail(NORI_ERR_INVALID, "nori_gpu_emitter_eval: reserved must be 0");
        if (sd->n == 0) return NORI_OK;
        if (!sd->on_device) check_host_records(*c, "nori_gpu_emitter_eval", surf, sd->n);
        const uint32_t shapes = (uint32_t)c->hshapes.size();
        return shading_call(*c, "nori_gpu_emitter_eval", *sd, {{surf, 64, 16}, {from, 12, 4}, {nullptr, 0, 4}}, out, 16,
                            [&](const void *const *d, void *o, uint32_t m) {
                                return launch_emitter_eval(c->S, shapes, (const float4 *)d[0], (const float *)d[1], m,
                                                           (float4 *)o, c->stream);
                            });
    });
}

int nori_gpu_sample_uniforms(nori_gpu_ctx *c, const nori_gpu_render_desc *rd, uint32_t first, uint32_t count, float *out) {
    return guarded([&] {
        if (!c || !rd || !out) return fail(NORI_ERR_INVALID, "null argument");
        if (rd->num_blocks && !rd->block_ids) return fail(NORI_ERR_INVALID, "block_ids is null");
        return sample_uniforms(*c, *rd, first, count, out);
    });
}

int nori_gpu_update_vertices(nori_gpu_ctx *c, const nori_gpu_update_desc *ud, nori_gpu_update_stats *stats) {
    return guarded([&] {
        if (!c || !ud || !ud->positions) return fail(NORI_ERR_INVALID, "null argument");
        return update_vertices(*c, *ud, stats);
    });
}

int nori_gpu_bvh_read(nori_gpu_ctx *c, float *nodes, float *prims, uint32_t *counts) {
    return guarded([&] {
        if (!c) return fail(NORI_ERR_INVALID, "null argument");
        return bvh_read(*c, nodes, prims, counts);
    });
}

int nori_scene_bvh_refit(const nori_scene_desc *d, const float *positions, float *nodes, float *prims, float *root_box) {
    return guarded([&] {
        if (!d) return fail(NORI_ERR_INVALID, "null argument");
        if (d->abi_version != NORI_GPU_ABI_VERSION) return fail(NORI_ERR_INVALID, "ABI version mismatch");
        if (positions)
            for (size_t i = 0; i < 3 * (size_t)d->num_vertices; ++i)
                if (!std::isfinite(positions[i])) return fail(NORI_ERR_INVALID, "nori_scene_bvh_refit: a non-finite position");
        float rmin[3], rmax[3];
        scene_root_box(*d, rmin, rmax);
        DeviceBvh bvh;
        build_device_bvh(*d, rmin, rmax, bvh);
        if (positions) refit_host(bvh, build_refit_plan(bvh), prim_vertex_ids(*d), positions, nullptr);
        if (nodes) std::memcpy(nodes, bvh.nodes.data(), bvh.nodes.size() * 4);
        if (prims) std::memcpy(prims, bvh.prims.data(), bvh.prims.size() * 4);
        if (root_box) refit_root_box(bvh.nodes.data(), root_box);
        return NORI_OK;
    });
}

int nori_gpu_rebuild_bvh(nori_gpu_ctx *c, const nori_gpu_rebuild_desc *rd, nori_gpu_rebuild_stats *stats) {
    return guarded([&] {
        if (!c || !rd) return fail(NORI_ERR_INVALID, "null argument");
        return rebuild_bvh(*c, *rd, stats);
    });
}

int nori_scene_bvh_rebuild(const nori_scene_desc *d, const float *positions, uint32_t leaf_max,
                           const float *refit_positions, nori_bvh_rebuild_info *info, float *nodes, float *prims,
                           float *root_box) {
    return guarded([&] {
        if (!d) return fail(NORI_ERR_INVALID, "null argument");
        if (d->abi_version != NORI_GPU_ABI_VERSION) return fail(NORI_ERR_INVALID, "ABI version mismatch");
        if (leaf_max > kRebuildLeafMax) return fail(NORI_ERR_INVALID, "nori_scene_bvh_rebuild: leaf_max above 64");
        for (const float *p : {positions, refit_positions})
            if (p)
                for (size_t i = 0; i < 3 * (size_t)d->num_vertices; ++i)
                    if (!std::isfinite(p[i])) return fail(NORI_ERR_INVALID, "nori_scene_bvh_rebuild: a non-finite position");
        DeviceBvh bvh;
        rebuild_host(*d, positions, leaf_max, bvh);
        if (refit_positions) refit_host(bvh, build_refit_plan(bvh), prim_vertex_ids(*d), refit_positions, nullptr);
        if (info) {
            std::memset(info, 0, sizeof(*info));
            info->device_nodes = bvh.num_nodes;
            info->depth = bvh.depth;
            info->num_prims = (uint32_t)(bvh.prims.size() / 12);
            info->leaf_max = leaf_max ? leaf_max : kRebuildLeafDefault;
        }
        if (nodes) std::memcpy(nodes, bvh.nodes.data(), bvh.nodes.size() * 4);
        if (prims) std::memcpy(prims, bvh.prims.data(), bvh.prims.size() * 4);
        if (root_box) refit_root_box(bvh.nodes.data(), root_box);
        return NORI_OK;
    });
}

// The hit record's statement (nori_gpu.h): fp32, the operation order of
// k_surface (kernels_query.hip surface_record), which it is tested against bit for bit.
int nori_scene_surface(const nori_scene_desc *d, uint32_t n, const float *rays, const nori_gpu_hit *hits,
                       nori_gpu_surface *out) {
    return guarded([&] {
        if (!d || !rays || !hits || !out) return fail(NORI_ERR_INVALID, "null argument");
        std::vector<uint32_t> first(d->num_shapes + 1, 0u);  // first global primitive id of each shape
        for (uint32_t s = 0; s < d->num_shapes; ++s)
            first[s + 1] = first[s] + (d->shapes[s].type == NORI_SHAPE_SPHERE ? 1u : d->shapes[s].tri_count);
        auto put3 = [](float *o, V3 v) { o[0] = v.x, o[1] = v.y, o[2] = v.z; };
        auto at3 = [](const float *a, uint32_t i) { return V3{a[3 * (size_t)i], a[3 * (size_t)i + 1], a[3 * (size_t)i + 2]}; };
        for (uint32_t i = 0; i < n; ++i) {
            const nori_gpu_hit &h = hits[i];
            nori_gpu_surface &r = out[i];
            std::memset(&r, 0, sizeof(r));
            if (h.prim < 0) {
                r.t = __builtin_inff();
                r.prim = r.shape = -1;
                continue;
            }
            if ((uint32_t)h.prim >= first[d->num_shapes]) return fail(NORI_ERR_INVALID, "primitive id outside the scene");
            const uint32_t s = (uint32_t)(std::upper_bound(first.begin(), first.end(), (uint32_t)h.prim) - first.begin()) - 1;
            const nori_shape_desc &sd = d->shapes[s];
            const float *ray = rays + 8 * (size_t)i;
            const float t = h.t, u = h.u, v = h.v;
            V3 p, ng, ns;
            V2 uv{u, v};
            if (sd.type == NORI_SHAPE_SPHERE) {
                p = V3{ray[0], ray[1], ray[2]} + V3{ray[4], ray[5], ray[6]} * t;
                ng = ns = normalize(p - V3{sd.center[0], sd.center[1], sd.center[2]});
                float phi = atan2f(ng.y, ng.x);  // sphericalCoordinates (common.cpp:264-272)
                if (phi < 0) phi += 2 * kPi;
                uv.x = (float)(0.5 + (double)(acosf(ng.z) / (2 * kPi)));
                uv.y = phi / kPi;
            } else {
                const uint64_t tri = (uint64_t)sd.tri_offset + ((uint32_t)h.prim - first[s]);
                if (tri >= d->num_triangles || !d->indices || !d->positions) return fail(NORI_ERR_INVALID, "mesh range outside the scene arrays");
                const uint32_t *f = d->indices + 3 * tri;
                if (f[0] >= d->num_vertices || f[1] >= d->num_vertices || f[2] >= d->num_vertices)
                    return fail(NORI_ERR_INVALID, "vertex index out of range");
                const V3 p0 = at3(d->positions, f[0]), p1 = at3(d->positions, f[1]), p2 = at3(d->positions, f[2]);
                const float bx = 1 - (u + v);
                p = (p0 * bx + p1 * u) + p2 * v;
                ng = normalize(cross(p1 - p0, p2 - p0));
                ns = ng;
                if (sd.has_uvs && d->uvs) {
                    const float *a = d->uvs + 2 * (size_t)f[0], *b = d->uvs + 2 * (size_t)f[1], *c = d->uvs + 2 * (size_t)f[2];
                    uv = V2{(bx * a[0] + u * b[0]) + v * c[0], (bx * a[1] + u * b[1]) + v * c[1]};
                }
                if (sd.has_normals) {
                    if (!d->normals) return fail(NORI_ERR_INVALID, "a mesh with normals in a scene without a normal array");
                    ns = normalize((at3(d->normals, f[0]) * bx + at3(d->normals, f[1]) * u) + at3(d->normals, f[2]) * v);
                    if (sd.normal_map >= 0) {  // NormalMap::eval (normalmap.cpp:95-134)
                        if ((uint32_t)sd.normal_map >= d->num_images) return fail(NORI_ERR_INVALID, "image index out of range");
                        const nori_image_desc &im = d->images[sd.normal_map];
                        if (!im.rgb || im.width <= 0 || im.height <= 0) return fail(NORI_ERR_INVALID, "bad image description");
                        const int W = im.width, H = im.height;
                        const float x = uv.x * (float)W, y = uv.y * (float)H;
                        int ix, iy;
                        if (im.wrap == NORI_WRAP_REPEAT) {
                            ix = (int)x % W;
                            iy = (int)y % H;
                            ix += ix < 0 ? W : 0;
                            iy += iy < 0 ? H : 0;
                        } else {
                            ix = std::min(std::max((int)x, 0), W - 1);
                            iy = std::min(std::max((int)y, 0), H - 1);
                        }
                        const uint8_t *tx = im.rgb + 3 * ((size_t)iy * W + ix);
                        const V3 c = V3{(float)tx[0] / 255.0f, (float)tx[1] / 255.0f, (float)tx[2] / 255.0f};
                        const V3 m = V3{2.0f * c.x - 1.0f, 2.0f * c.y - 1.0f, 2.0f * c.z - 1.0f};
                        ns = to_world(frame_from(ns), normalize(m));
                    }
                }
            }
            put3(r.p, p);
            r.t = t;
            put3(r.ng, ng);
            r.prim = h.prim;
            put3(r.ns, ns);
            r.shape = (int32_t)s;
            r.uv[0] = uv.x, r.uv[1] = uv.y;
            r.bary[0] = u, r.bary[1] = v;
        }
        return NORI_OK;
    });
}

int nori_gpu_cancel(nori_gpu_ctx *c) {
    if (!c) return fail(NORI_ERR_INVALID, "null argument");
    c->cancel = 1;
    return NORI_OK;
}
float nori_gpu_progress(const nori_gpu_ctx *c) { return c ? c->progress.load() : 0.0f; }

int nori_gpu_comm_id(unsigned char *id) {
    return guarded([&] {
        if (!id) return fail(NORI_ERR_INVALID, "null argument");
        comm_unique_id(id);
        return (int)NORI_OK;
    });
}
int nori_gpu_comm_create(const unsigned char *id, int nranks, int rank, int device, nori_gpu_comm **out) {
    return guarded([&] {
        if (!id || !out) return fail(NORI_ERR_INVALID, "null argument");
        if (nranks < 1 || nranks > 0xFFFF || rank < 0 || rank >= nranks) return fail(NORI_ERR_INVALID, "rank out of range");
        std::unique_ptr<nori_gpu_comm> c(new nori_gpu_comm);
        // the status exchange's words, allocated here so that no allocation
        // stands between a failed share and the exchange
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipMalloc((void **)&c->status_dev, sizeof(int)));
        HIP_TRY(hipHostMalloc((void **)&c->status_host, sizeof(int), hipHostMallocDefault));
        c->nccl = comm_create(id, nranks, rank, device);
        c->nranks = nranks;
        c->rank = rank;
        c->device = device;
        *out = c.release();
        return (int)NORI_OK;
    });
}
int nori_gpu_comm_rank(const nori_gpu_comm *c, int *nranks, int *rank) {
    if (!c || !nranks || !rank) return fail(NORI_ERR_INVALID, "null argument");
    *nranks = c->nranks;
    *rank = c->rank;
    return NORI_OK;
}
void nori_gpu_comm_destroy(nori_gpu_comm *c) { delete c; }
const char *nori_gpu_comm_library(void) { return comm_library_path(); }

int nori_gpu_shard_desc(const nori_scene_desc *d, const nori_gpu_render_desc *rd, int mode, int nranks, int rank,
                        nori_gpu_render_desc *out, uint32_t *block_buf) {
    return guarded([&] {
        if (!d || !rd || !out || (rd->num_blocks && !rd->block_ids)) return fail(NORI_ERR_INVALID, "null argument");
        std::vector<uint32_t> blocks;
        nori_gpu_render_desc s =
            shard_of(d->camera.width, d->camera.height, d->sample_count, *rd, mode, nranks, rank, blocks);
        if (!blocks.empty()) {
            if (!block_buf) return fail(NORI_ERR_INVALID, "block_buf is null");
            std::memcpy(block_buf, blocks.data(), 4 * blocks.size());
            s.block_ids = block_buf;
        } else {
            s.block_ids = nullptr;
        }
        *out = s;
        return (int)NORI_OK;
    });
}

int nori_gpu_render_sharded(nori_gpu_ctx *c, nori_gpu_comm *comm, const nori_gpu_render_desc *rd, int mode, int root,
                            float *film, nori_gpu_stats *stats) {
    return guarded([&] {
        if (!c || !comm) return fail(NORI_ERR_INVALID, "null argument");
        if (comm->aborted) return fail(NORI_ERR_HIP, "communicator was aborted by an earlier failure");
        // This rank's share.  A failure or a cancel (nori_gpu_cancel) must not
        // leave the peers blocked in the film sum: every rank joins a status
        // exchange first (max over ranks of severity << 16 | rank), and the
        // film sum runs only if every rank rendered its share.  Everything
        // fallible of the share -- argument checks, the film clear, the
        // render -- reports through the exchange.
        int rc = NORI_OK;
        std::string err;
        double own_s = 0.0, own_samples = 0.0, max_samples = 0.0;
        size_t n = 0;
        try {
            if (!rd || !film) throw NoriException(NORI_ERR_INVALID, "null argument");
            if (rd->num_blocks && !rd->block_ids) throw NoriException(NORI_ERR_INVALID, "block_ids is null");
            if (rd->variance_out)  // per-pixel statistics are not summed across ranks
                throw NoriException(NORI_ERR_INVALID, "nori_gpu_render_sharded: variance_out must be NULL");
            if (root >= comm->nranks) throw NoriException(NORI_ERR_INVALID, "root out of range");
            if (comm->device != c->device)
                throw NoriException(NORI_ERR_INVALID, "communicator and context on different devices");
            HIP_TRY(hipSetDevice(c->device));
            std::vector<uint32_t> blocks, other;
            nori_gpu_render_desc s = shard_of(c->S.W, c->S.H, c->spp, *rd, mode, comm->nranks, comm->rank, blocks);
            own_samples = share_samples(c->S.W, c->S.H, s);
            for (int r = 0; r < comm->nranks; ++r)
                max_samples = std::max(max_samples, share_samples(c->S.W, c->S.H,
                                                                  shard_of(c->S.W, c->S.H, c->spp, *rd, mode,
                                                                           comm->nranks, r, other)));
            s.output_on_device = 1;
            s.variance_out = nullptr;
            n = 4 * (size_t)(c->S.W + 2 * c->S.border) * (size_t)(c->S.H + 2 * c->S.border);
            HIP_TRY(hipMemsetAsync(film, 0, n * sizeof(float), c->stream));
            const auto t0 = std::chrono::steady_clock::now();
            if (s.pass_count) rc = render(*c, s, film, stats);
            else if (stats) std::memset(stats, 0, sizeof(*stats));
            own_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        } catch (const NoriException &e) {
            rc = e.code;
            err = e.what();
        } catch (const std::bad_alloc &) {
            rc = NORI_ERR_OOM;
            err = "out of memory";
        } catch (const std::exception &e) {
            rc = NORI_ERR_INVALID;
            err = e.what();
        }
        if (rc != NORI_OK && err.empty()) err = g_last_error;
        if (rc == NORI_ERR_HIP) {
            // A sticky error (a device fault) fails every later call on the
            // device, so this rank cannot join the exchange: abort, and the
            // peers' watchdog ends their wait.  Any other HIP error leaves
            // the stream usable and goes through the exchange.
            (void)hipGetLastError();
            if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
                comm_abort(comm->nccl);
                comm->aborted = true;
                return fail(rc, err);
            }
        }
        const double timeout = comm_timeout_s(rc, own_s, own_samples, max_samples);
        const int all = comm_max_int(comm->nccl, comm->status_dev, comm->status_host,
                                     comm_status_word(rc, comm->rank), c->stream, timeout, comm->aborted);
        if (rc != NORI_OK) return fail(rc, err);
        if ((all >> 16) != 0)
            return fail((all >> 16) == 1 ? NORI_ERR_CANCELLED : NORI_ERR_INVALID,
                        "the frame is incomplete: rank " + std::to_string(all & 0xFFFF) +
                            ((all >> 16) == 1 ? " was cancelled" : " failed to render its share"));
        comm_sum(comm->nccl, film, n, root, c->stream);
        comm_wait(comm->nccl, c->stream, timeout, comm->aborted);
        return (int)NORI_OK;
    });
}
int nori_gpu_comm_status_word(int rc, int rank) { return comm_status_word(rc, rank); }
double nori_gpu_comm_timeout(int status, double own_seconds, double own_samples, double max_samples) {
    return comm_timeout_s(status, own_seconds, own_samples, max_samples);
}
void nori_gpu_destroy(nori_gpu_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;
}

}  // extern "C"
