// kernels.hip -- kernels of the CDNA4 (gfx950) wavefront path tracer: the
// trace kernels (k_trace, k_extend, k_shadow, k_trace_both, their scan-mode
// variants) and k_reset; one sample per thread (k_direct, k_photons); the
// film splat (k_splat).
//
// One iteration of the state machine (render.hip drives it):
//   k_shade   : per path: surface hit -> emission, next-event estimation
//               (light sample + shadow ray), Russian roulette, BSDF sample,
//               or regeneration of a finished path slot with a new camera
//               sample.  Work-group b owns queue segment b; survivors and
//               shadow rays are compacted inside the segment with 64-lane
//               ballots + an LDS prefix over the 4 waves (no global atomics).
//               (kernels_shade.hip)
//   k_extend  : closest-hit BVH traversal of the compacted path queue.
//   k_shadow  : any-hit traversal; unoccluded rays add their payload to the
//               sample record (the reference's `color +=`, path_mis.cpp:48-60).
// Once every segment's work stream is used up, k_finish (kernels_finish.hip)
// runs the remaining paths to completion one thread per path (no per-bounce
// launches for the Russian-roulette tail), then k_splat filters every sample
// into the film.
//
// Together the kernel units replace render.cpp:194-233 (pass loop +
// tbb::parallel_for), renderBlock (render.cpp:80-133), PathMisIntegrator::Li
// (path_mis.cpp:17-101), PathMatsIntegrator::Li (path_mats.cpp:17-60),
// BVH::rayIntersect (bvh.cpp:404-462) and ImageBlock::put (block.cpp:93-133).
//
// Where the rest lives: traverse.h (the BVH walk, shared), shading.h (the path
// vertex, shared), onebounce.h (OneBounce), kernels_features.hip
// (k_features), kernels_query.hip (k_surface, k_camera_rays).  A template
// kernel is defined in the unit that launches it; each non-template kernel
// and launcher in exactly one unit.
#include <algorithm>
#include <cstddef>
#include <cstdlib>

#include "onebounce.h"

namespace nori {

// ------------------------------------------------------------------ trace kernels
template <int STACK, bool ANY>
__global__ __launch_bounds__(kTraceBlock) void k_trace(DevScene S, const float4 *rays, uint32_t n, float4 *hits) {
    if constexpr (STACK == 0) {  // the caller's rays: mint may be <= 0 (scan_core ZMINT)
        trace_scan_body<ANY>(S, rays, n, hits);
        return;
    }
    __shared__ uint32_t stk[stack_words(STACK) * kTraceBlock];
    uint32_t q = blockIdx.x * kTraceBlock + threadIdx.x;
    if (q >= n) return;
    float4 a = rays[2 * (size_t)q], b = rays[2 * (size_t)q + 1];
    TRay r;
    r.o = ld3(a);
    r.d = ld3(b);
    r.mint = a.w;
    r.maxt = b.w;
    float t, u, v;
    uint32_t p;
    const bool h = traverse<STACK, ANY>(S, r, stk + threadIdx.x, t, p, u, v);
    if (ANY) hits[q] = make_float4(h ? 0.0f : INF_F, __uint_as_float(h ? 0u : 0xFFFFFFFFu), 0.0f, 0.0f);
    else hits[q] = make_float4(t, __uint_as_float(p), u, v);
}

// Entry numbering of the trace launches: seg_index.h.
constexpr uint32_t kTraceSlices = kTraceGroup * kSeg / kTraceBlock;  // BVH-walk work-groups per group
ND SegRange seg_range(const uint32_t *cnt, uint32_t G, uint32_t bid) { return seg_group(cnt, G, bid, kTraceSlices); }

// Extension rays: closest hit of every queued path (work-group `bid` of the
// launch's extension part).
template <int STACK>
ND void extend_body(const DevScene &S, const PathQueue &pq, const uint32_t *cnt, uint32_t G, uint32_t bid,
                    uint32_t *stk) {
    const SegRange sr = seg_range(cnt, G, bid);
    const uint32_t i = seg_first(bid, kTraceSlices, kTraceBlock, 1, threadIdx.x);
    if (i < sr.pre[kTraceGroup]) {
        const uint32_t q = seg_entry(sr, i);
        TRay r;
        path_ray(S, pq.ray_o[q], pq.ray_d[q], r);
        float t, u, v;
        uint32_t p;
        traverse<STACK, false>(S, r, stk + threadIdx.x, t, p, u, v);
        pq.hit[q] = make_float4(t, __uint_as_float(p), u, v);
    }
}

// Shadow rays: any hit; unoccluded -> record += payload.
template <int STACK>
ND void shadow_body(const DevScene &S, const ShadowQueue &sq, const uint32_t *shcnt, float4 *rec, uint32_t G,
                    uint32_t bid, uint32_t *stk) {
    const SegRange sr = seg_range(shcnt, G, bid);
    const uint32_t i = seg_first(bid, kTraceSlices, kTraceBlock, 1, threadIdx.x);
    if (i < sr.pre[kTraceGroup]) {
        const uint32_t q = seg_entry(sr, i);
        float4 a = sq.ray_o[q], b = sq.ray_d[q];
        TRay r;
        r.o = ld3(a);
        r.d = ld3(b);
        r.mint = a.w;
        r.maxt = b.w;
        float t, u, v;
        uint32_t p;
        if (!traverse<STACK, true>(S, r, stk + threadIdx.x, t, p, u, v)) shadow_add(rec, sq.payload[q]);
    }
}

#ifdef NORI_TRACE_WAVES
#define NORI_TRACE_ATTR __attribute__((amdgpu_waves_per_eu(NORI_TRACE_WAVES)))
#else
#define NORI_TRACE_ATTR
#endif

template <int STACK>
__global__ __launch_bounds__(kTraceBlock) NORI_TRACE_ATTR void k_extend(DevScene S, PathQueue pq, const uint32_t *cnt, uint32_t G) {
    __shared__ uint32_t stk[stack_words(STACK) * kTraceBlock];
    extend_body<STACK>(S, pq, cnt, G, STACK ? xcd_block(blockIdx.x, gridDim.x) : blockIdx.x, stk);
}
template <int STACK>
__global__ __launch_bounds__(kTraceBlock) NORI_TRACE_ATTR void k_shadow(DevScene S, ShadowQueue sq, const uint32_t *shcnt,
                                                        float4 *rec, uint32_t G) {
    __shared__ uint32_t stk[stack_words(STACK) * kTraceBlock];
    shadow_body<STACK>(S, sq, shcnt, rec, G, STACK ? xcd_block(blockIdx.x, gridDim.x) : blockIdx.x, stk);
}
// An iteration's extension and shadow walks in one launch (launch_trace_both):
// work-groups [0, nb_ext) walk the extension rays, the rest the shadow rays
// (independent queues); nb_ext is a multiple of the 8 XCDs, so both ranges
// keep their XCD-aware order.
template <int STACK>
__global__ __launch_bounds__(kTraceBlock) NORI_TRACE_ATTR void k_trace_both(DevScene S, PathQueue pq, const uint32_t *cnt,
                                                                            ShadowQueue sq, const uint32_t *shcnt,
                                                                            float4 *rec, uint32_t G, uint32_t nb_ext) {
    __shared__ uint32_t stk[stack_words(STACK) * kTraceBlock];
    if (blockIdx.x < nb_ext) extend_body<STACK>(S, pq, cnt, G, xcd_block(blockIdx.x, nb_ext), stk);
    else shadow_body<STACK>(S, sq, shcnt, rec, G, xcd_block(blockIdx.x - nb_ext, gridDim.x - nb_ext), stk);
}
template <int K>
__global__ __launch_bounds__(NORI_EXTEND_BLOCK) void k_extend_scan(DevScene S, PathQueue pq, const uint32_t *cnt,
                                                                   uint32_t G) {
    extend_scan_body<K>(S, pq, cnt, G, blockIdx.x);
}
template <int K>
__global__ __launch_bounds__(NORI_SHADOW_BLOCK) void k_shadow_scan(DevScene S, ShadowQueue sq, const uint32_t *shcnt,
                                                                   float4 *rec, uint32_t G) {
    shadow_scan_body<K>(S, sq, shcnt, rec, G, blockIdx.x);
}

// ------------------------------------------------------------------ launchers of the trace kernels
template <bool ANY>
static hipError_t trace_dispatch(const DevScene &S, const float4 *rays, uint32_t n, float4 *hits, int stack,
                                 hipStream_t st) {
    dim3 g((n + kTraceBlock - 1) / kTraceBlock), b(kTraceBlock);
    with_stack<0, 64>(stack, [&](auto N) { hipLaunchKernelGGL((k_trace<N(), ANY>), g, b, 0, st, S, rays, n, hits); });
    return hipGetLastError();
}
hipError_t launch_trace(const DevScene &S, const float4 *rays, uint32_t n, int any_hit, float4 *hits, int stack,
                        hipStream_t st, const ScanRtc *rtc) {
    if (n == 0) return hipSuccess;
    if (stack == 0 && rtc && rtc->trace[any_hit ? 1 : 0]) {
        void *args[] = {(void *)&S, (void *)&rays, (void *)&n, (void *)&hits};
        return hipModuleLaunchKernel(rtc->trace[any_hit ? 1 : 0], (n + kTraceBlock - 1) / kTraceBlock, 1, 1, kTraceBlock,
                                     1, 1, 0, st, args, nullptr);
    }
    return any_hit ? trace_dispatch<true>(S, rays, n, hits, stack, st)
                   : trace_dispatch<false>(S, rays, n, hits, stack, st);
}

hipError_t launch_extend(const DevScene &S, const PathQueue &q, const uint32_t *cnt, uint32_t G, int stack,
                         hipStream_t st, const ScanRtc *rtc) {
    dim3 g(seg_grid(G, kTraceSlices)), b(kTraceBlock);
    if (stack == 0) {
        const dim3 gk(seg_grid(G, scan_per<kScanRays, NORI_EXTEND_BLOCK>())), bk(NORI_EXTEND_BLOCK);
        if (rtc && rtc->extend) {
            void *args[] = {(void *)&S, (void *)&q, (void *)&cnt, (void *)&G};
            const uint32_t per = kTraceGroup * kSeg / (NORI_EXTEND_BLOCK * (uint32_t)rtc->k_extend);
            return hipModuleLaunchKernel(rtc->extend, seg_grid(G, per), 1, 1, bk.x, 1, 1, 0, st, args, nullptr);
        }
        hipLaunchKernelGGL(k_extend_scan<kScanRays>, gk, bk, 0, st, S, q, cnt, G);
        return hipGetLastError();
    }
    with_stack<8, 64>(stack, [&](auto N) { hipLaunchKernelGGL(k_extend<N()>, g, b, 0, st, S, q, cnt, G); });
    return hipGetLastError();
}

bool launch_trace_both(const DevScene &S, const PathQueue &q, const uint32_t *cnt, const ShadowQueue &sq,
                       const uint32_t *shcnt, float4 *rec, uint32_t G, int stack, const ScanRtc *rtc, hipStream_t st,
                       hipError_t &err) {
    static_assert(NORI_EXTEND_BLOCK == NORI_SHADOW_BLOCK, "one work-group size for both roles");
    if (stack != 0) {  // BVH walks
        static_assert(kTraceSlices % kXcds == 0, "the shadow range starts on an XCD boundary");
        const uint32_t nbe = seg_grid(G, kTraceSlices), nbt = 2 * nbe;
        with_stack<8, 64>(stack, [&](auto N) {
            hipLaunchKernelGGL(k_trace_both<N()>, dim3(nbt), dim3(kTraceBlock), 0, st, S, q, cnt, sq, shcnt, rec, G, nbe);
        });
        err = hipGetLastError();
        return true;
    }
    if (!rtc || !rtc->both) return false;
    uint32_t nb_ext = seg_grid(G, kTraceGroup * kSeg / (NORI_EXTEND_BLOCK * (uint32_t)rtc->k_extend));
    const uint32_t nb = nb_ext + seg_grid(G, scan_per<kScanRaysShadow, NORI_SHADOW_BLOCK>());
    void *args[] = {(void *)&S, (void *)&q, (void *)&cnt, (void *)&sq, (void *)&shcnt, (void *)&rec, (void *)&G, (void *)&nb_ext};
    err = hipModuleLaunchKernel(rtc->both, nb, 1, 1, NORI_EXTEND_BLOCK, 1, 1, 0, st, args, nullptr);
    return true;
}
hipError_t launch_shadow(const DevScene &S, const ShadowQueue &sq, const uint32_t *shcnt, float4 *rec, uint32_t G,
                         int stack, hipStream_t st, const ScanRtc *rtc) {
    dim3 g(seg_grid(G, kTraceSlices)), b(kTraceBlock);
    if (stack == 0) {
        const dim3 gk(seg_grid(G, scan_per<kScanRaysShadow, NORI_SHADOW_BLOCK>())), bk(NORI_SHADOW_BLOCK);
        if (rtc && rtc->shadow) {
            void *args[] = {(void *)&S, (void *)&sq, (void *)&shcnt, (void *)&rec, (void *)&G};
            return hipModuleLaunchKernel(rtc->shadow, gk.x, 1, 1, bk.x, 1, 1, 0, st, args, nullptr);
        }
        hipLaunchKernelGGL(k_shadow_scan<kScanRaysShadow>, gk, bk, 0, st, S, sq, shcnt, rec, G);
        return hipGetLastError();
    }
    with_stack<8, 64>(stack, [&](auto N) { hipLaunchKernelGGL(k_shadow<N()>, g, b, 0, st, S, sq, shcnt, rec, G); });
    return hipGetLastError();
}

// Start of a chunk of passes: zero the counters, the segments' path counts,
// work cursors and statistics, and preset the count of segments whose work
// stream is empty from the start (one launch instead of five copies/fills).
__global__ __launch_bounds__(256) void k_reset(Counters *C, uint32_t empty, SegState seg, uint32_t G) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    constexpr uint32_t nw = sizeof(Counters) / 4;
    if (i < nw) reinterpret_cast<uint32_t *>(C)[i] = i == 0 ? empty : 0u;  // word 0: exhausted
    if (i < G) {
        seg.cnt[0][i] = 0u;
        seg.cursor[i] = 0u;
        seg.stats[i] = make_uint4(0u, 0u, 0u, 0u);
    }
}
hipError_t launch_reset(Counters *C, uint32_t empty, const SegState &seg, uint32_t G, hipStream_t st) {
    static_assert(offsetof(Counters, exhausted) == 0, "Counters layout");
    const uint32_t n = std::max<uint32_t>(G, sizeof(Counters) / 4);
    hipLaunchKernelGGL(k_reset, dim3((n + 255) / 256), dim3(256), 0, st, C, empty, seg, G);
    return hipGetLastError();
}

// ------------------------------------------------------------------ one sample per thread (OneBounce, onebounce.h)
#ifndef NORI_DIRECT_XCD
#define NORI_DIRECT_XCD 1
#endif
template <int STACK, int INTEG>
__global__ __launch_bounds__(kTraceBlock) void k_direct(DevScene S, WorkDesc wd, float4 *rec, Counters *C) {
    __shared__ uint32_t stk[stack_words(STACK) * kTraceBlock];
    // XCD-aware order (NORI_DIRECT_XCD): each XCD sweeps its own contiguous
    // eighth of the work ids, so at any moment it shades one band of image
    // rows and its L2 holds the photons / tree nodes of that band
    const uint32_t bid = NORI_DIRECT_XCD ? xcd_block(blockIdx.x, gridDim.x) : blockIdx.x;
    const uint64_t w = (uint64_t)bid * kTraceBlock + threadIdx.x;
    OneBounce<STACK> ob{S, stk + threadIdx.x};
    if (w < wd.total) {
        const uint32_t pass = (uint32_t)(w / wd.M), e = (uint32_t)(w - (uint64_t)pass * wd.M), pix = wd.pixels[e];
        const uint32_t y = pix / (uint32_t)S.W, x = pix - y * (uint32_t)S.W;
        Pcg rng;
        wave_seed(rng, wd.seed, (uint64_t)(wd.pass_begin + pass) * ((uint64_t)S.W * (uint64_t)S.H) + pix);
        const V2 jit = next2D(rng);
        const V2 ap = next2D(rng);  // apertureSample (render.cpp:99)
        const float px = (float)x + jit.x, py = (float)y + jit.y;
        V3 L;
        if (S.chromatic[0] != 0.0f || S.chromatic[1] != 0.0f || S.chromatic[2] != 0.0f) {
            // render.cpp:106-121: one ray per colour channel, Li calls in turn,
            // each weighted by its channel's unit colour
            V3 o[3], d[3];
            float mn[3], mx[3];
            for (int ch = 0; ch < 3; ++ch) camera_sample(S, px, py, ap, ch, o[ch], d[ch], mn[ch], mx[ch]);
            V3 v[3];
            for (int ch = 0; ch < 3; ++ch) {
                const V3 l = ob.template Li<INTEG>(rng, o[ch], d[ch], mn[ch], mx[ch]);
                v[ch] = V3{ch == 0 ? 1.f : 0.f, ch == 1 ? 1.f : 0.f, ch == 2 ? 1.f : 0.f} * l;
            }
            L = (v[0] + v[1]) + v[2];
        } else {
            V3 o, d;
            float mn, mx;
            camera_sample(S, px, py, ap, -1, o, d, mn, mx);
            L = V3{1, 1, 1} * ob.template Li<INTEG>(rng, o, d, mn, mx);
        }
        rec[w] = make_float4(L.x, L.y, L.z, rec_code(S.jit_lk, S.border, x, y, jit));
    }
    // ray counts: one atomic per wave
    uint32_t rc = ob.rc, rs = ob.rs;
    for (int off = 32; off > 0; off >>= 1) {
        rc += __shfl_xor(rc, off);
        rs += __shfl_xor(rs, off);
    }
    if (lane_id() == 0 && (rc | rs)) {
        atomicAdd(&C->direct_rays[0], (unsigned long long)rc);
        atomicAdd(&C->direct_rays[1], (unsigned long long)rs);
    }
}

// ------------------------------------------------------------------ photon tracing
// PhotonMapper::preprocess (photonmapper.cpp:41-117), one thread per emitted
// photon e (pcg32 stream wave_seed(kPhotonSeed, e), deviation D8): a light
// chosen uniformly, AreaEmitter::samplePhoton (arealight.cpp:78-95: surface
// point, cosine-weighted direction, power = Le * pi / pdf * lights), then
// bounces with a stored photon at every diffuse hit, Russian roulette on the
// red channel and BSDF sampling.  COUNT pass: photons stored per emitted
// photon.  STORE pass (photons e < n): they go to pre[e].. in emission order,
// and the map ends after `total` photons -- the reference's "return if the
// map is full" (photonmapper.cpp:92-94) over the emission order.
template <int STACK, bool STORE>
__global__ __launch_bounds__(kTraceBlock) void k_photons(DevScene S, uint64_t e0, uint32_t n, uint32_t *count,
                                                         const uint64_t *pre, uint64_t total, float4 *out) {
    __shared__ uint32_t stk[stack_words(STACK) * kTraceBlock];
    const uint32_t i = blockIdx.x * kTraceBlock + threadIdx.x;
    if (i >= n) return;
    Pcg rng;
    wave_seed(rng, kPhotonSeed, e0 + i);
    const uint32_t ne = S.num_emitters;
    uint32_t li = (uint32_t)floorf((float)ne * next1D(rng));  // Scene::getRandomEmitter (scene.h:68-74)
    if (li > ne - 1) li = ne - 1;
    const DevEmitter &E = S.emitters[li];
    const V2 s1 = next2D(rng), s2 = next2D(rng);
    const DevShape &esh = S.shapes[E.shape];
    V3 p, nrm;
    sample_surface(S, esh, s1, p, nrm);
    const float pdf = esh.area_norm;
    uint64_t stored = 0;
    const uint64_t base = STORE ? pre[i] : 0;
    const uint64_t limit = STORE ? (total > base ? total - base : 0) : ~0ull;
    if (pdf > 0) {  // (a light of zero area: no photon)
        const V3 cs = to_world(frame_from(nrm), sq_cosine_hemisphere(s2));
        const V3 ref = p + cs;  // EmitterQueryRecord(sRec.p + cosine_sample, sRec.p, sRec.n)
        V3 power = ((emitter_eval(S, E, nrm, normalize(p - ref)) * kPi) / pdf) * (float)ne;
        V3 o = p, d = cs;
        uint32_t *lstk = stk + threadIdx.x;
        for (;;) {
            TRay r{o, d, V3{0, 0, 0}, kEps, INF_F};
            float t, u, v;
            uint32_t prim;
            if (!traverse<STACK, false>(S, r, lstk, t, prim, u, v)) break;
            const SurfHit hs = surface(S, prim, t, u, v, o, d);
            const DevBsdf &B = S.bsdfs[S.shapes[hs.shape].bsdf];
            if (B.type == NORI_BSDF_DIFFUSE) {
                if (STORE) {
                    if (stored >= limit) break;
                    float4 *q = out + 3 * (size_t)(base + stored);
                    q[0] = make_float4(hs.p.x, hs.p.y, hs.p.z, 0.0f);
                    q[1] = make_float4(-d.x, -d.y, -d.z, 0.0f);
                    q[2] = make_float4(power.x, power.y, power.z, 0.0f);
                }
                ++stored;
            }
            const float q = smin(power.x, 0.99f);
            if (next1D(rng) > q) break;
            power = power / q;
            BRec br;
            br.wi = to_local(hs.sh, -d);
            br.wo = V3{0, 0, 1};
            br.measure = kMeasureUnknown;
            br.uv = hs.uv;
            const V3 w = bsdf_sample(B, br, next2D(rng));
            if (is_zero(w)) break;  // deviation D1
            power = power * w;
            o = hs.p;
            d = to_world(hs.sh, br.wo);
        }
    }
    if (!STORE) count[i] = (uint32_t)(stored < 0xFFFFFFFFull ? stored : 0xFFFFFFFFull);
}

template <int INTEG>
static void direct_dispatch(const DevScene &S, const WorkDesc &wd, float4 *rec, Counters *C, int stack,
                            hipStream_t st) {
    const dim3 g((uint32_t)((wd.total + kTraceBlock - 1) / kTraceBlock)), b(kTraceBlock);
    with_stack<0, 32>(stack, [&](auto N) { hipLaunchKernelGGL((k_direct<N(), INTEG>), g, b, 0, st, S, wd, rec, C); });
}
hipError_t launch_direct(const DevScene &S, const WorkDesc &wd, float4 *rec, Counters *C, int stack, hipStream_t st) {
    if (wd.total == 0) return hipSuccess;
    switch (S.integrator) {
    case NORI_INTEGRATOR_NORMALS: direct_dispatch<NORI_INTEGRATOR_NORMALS>(S, wd, rec, C, stack, st); break;
    case NORI_INTEGRATOR_AV: direct_dispatch<NORI_INTEGRATOR_AV>(S, wd, rec, C, stack, st); break;
    case NORI_INTEGRATOR_DIRECT: direct_dispatch<NORI_INTEGRATOR_DIRECT>(S, wd, rec, C, stack, st); break;
    case NORI_INTEGRATOR_DIRECT_EMS: direct_dispatch<NORI_INTEGRATOR_DIRECT_EMS>(S, wd, rec, C, stack, st); break;
    case NORI_INTEGRATOR_DIRECT_MATS: direct_dispatch<NORI_INTEGRATOR_DIRECT_MATS>(S, wd, rec, C, stack, st); break;
    case NORI_INTEGRATOR_DIRECT_MIS: direct_dispatch<NORI_INTEGRATOR_DIRECT_MIS>(S, wd, rec, C, stack, st); break;
    case NORI_INTEGRATOR_PHOTONMAPPER: direct_dispatch<NORI_INTEGRATOR_PHOTONMAPPER>(S, wd, rec, C, stack, st); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <bool STORE>
static void photons_dispatch(const DevScene &S, uint64_t e0, uint32_t n, uint32_t *count, const uint64_t *pre,
                             uint64_t total, float4 *out, int stack, hipStream_t st) {
    const dim3 g((n + kTraceBlock - 1) / kTraceBlock), b(kTraceBlock);
    with_stack<0, 32>(stack, [&](auto N) {
        hipLaunchKernelGGL((k_photons<N(), STORE>), g, b, 0, st, S, e0, n, count, pre, total, out);
    });
}
hipError_t launch_photons(const DevScene &S, uint64_t e0, uint32_t n, uint32_t *count, const uint64_t *pre,
                          uint64_t total, float4 *out, int stack, hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (out) photons_dispatch<true>(S, e0, n, count, pre, total, out, stack, st);
    else photons_dispatch<false>(S, e0, n, count, pre, total, out, stack, st);
    return hipGetLastError();
}

// ------------------------------------------------------------------ film splat
#ifndef NORI_SPLAT_DEPTH
#define NORI_SPLAT_DEPTH 1  // sample records in flight per thread (prefetch depth)
#endif
// ImageBlock::put(pos, val) (block.cpp:93-122) for every sample of one 32x32
// block and a range of passes, then ImageBlock::put(block) (block.cpp:124-133)
// into the film.  A thread owns one pixel: all samples of that pixel fall in
// the same (2B+1)^2 window around it, so the thread sums the filtered samples
// of all its passes in registers and touches the LDS tile once per window
// cell instead of once per sample and cell.
// CODED (S.jit_lk != 0): the sample's window weights come from the jitter
// class its record carries (device_math.h jit_class), one row of a class
// table built per work-group -- the same weights as re-deriving the jitter
// from the sample's pcg32 stream (CODED = false), without the stream.
// SPLIT: two lanes per pixel (adjacent lanes, the same record), the first
// summing the R, G and the second the B, W windows -- half the registers per
// lane (more waves per SIMD hide the record loads), each lane redoing only the
// record's decode and weight reads (CODED).
// 768 threads (3 waves per SIMD) with 4 records in flight per lane: 108
// VGPRs, so that a 144-VGPR finisher wave still fits beside three splat
// waves on a SIMD (3 x 112 + 144 <= 512).  Measured (C2): splat 1.14-1.18 ms
// and finisher 1.15-1.17 ms against 1.26-1.33 / 1.10-1.15 ms for 512 threads
// with 8 records; 768 threads with 8 records (136 VGPRs) splat in 0.83 ms
// but starve the finisher (1.75 ms), DESIGN_LOG.md (round 5).
#ifndef NORI_SPLAT_SPLIT_BLOCK
#define NORI_SPLAT_SPLIT_BLOCK 768
#endif
#ifndef NORI_SPLAT_SPLIT_DEPTH
#define NORI_SPLAT_SPLIT_DEPTH 4
#endif
#ifndef NORI_SPLAT_NB
#define NORI_SPLAT_NB 0
#endif
constexpr int kSplatSplitBlock = NORI_SPLAT_SPLIT_BLOCK;
template <int B, bool CODED, bool SPLIT = false>
__global__ __launch_bounds__(SPLIT ? kSplatSplitBlock : kSplatBlock) void k_splat(DevScene S, const float4 *rec,
                                                                                  SplatDesc sd, float *film,
                                                                                  Counters *C) {
    constexpr int NT = SPLIT ? kSplatSplitBlock : kSplatBlock, NH = SPLIT ? 1 : 2;  // threads; pairs per lane
    constexpr int D = SPLIT ? NORI_SPLAT_SPLIT_DEPTH : NORI_SPLAT_DEPTH;           // records in flight per lane
    constexpr bool NB = CODED && NORI_SPLAT_NB;  // per-sample checks as selects, not branches
    constexpr int TS = NORI_BLOCK_SIZE + 2 * B, K = 2 * B + 1, KP = (K + 3) / 4;  // float4s per weight row
    __shared__ float tile[TS * TS * 4];
    __shared__ float ftab[NORI_FILTER_RESOLUTION + 1];
    __shared__ float4 wtab[CODED ? 256 * KP : 1];  // CODED: the window weights of every jitter class
    int4 bi = sd.blocks[blockIdx.x];
    const int ox = bi.x, oy = bi.y, bw = bi.z & 0xFFFF, bh = bi.z >> 16;
    const uint32_t off = (uint32_t)bi.w;
    const uint32_t p0 = blockIdx.y * sd.passes_per_wg, p1 = min(sd.passes, p0 + sd.passes_per_wg);
    for (int i = threadIdx.x; i < TS * TS * 4; i += NT) tile[i] = 0.0f;
    if (threadIdx.x <= NORI_FILTER_RESOLUTION) ftab[threadIdx.x] = S.filter[threadIdx.x];
    __syncthreads();
    const int npix = bw * bh;
    const float rad = S.filter_radius, lk = S.lookup;
    if constexpr (CODED) {
        // class (floor(P) - lx - B + 1, [f lk integer], q) -> the K weights of the window
        // cells d = 0..K-1 (tile column lx + d), computed by the formula of
        // the direct path below on a representative sub-pixel offset f of the
        // class (q / lk or (q + 1/2) / lk: the same indices and box ends,
        // device_math.h jit_class); P = lx + m + f with m = B + n - 1
        float *wt = reinterpret_cast<float *>(wtab);
        for (int i = threadIdx.x; i < 16 * S.jit_lk * KP; i += NT) {
            const int c = i / (4 * KP), d = i - c * (4 * KP);
            const int m = B + (c & 1) - 1, q = c >> 2;
            const float f = (c & 2) ? (float)q / lk : ((float)q + 0.5f) / lk;
            float wv = 0.0f;
            if (d < K) {
                const int lo = m + (int)ceilf(f - rad), hi = m + (int)floorf(f + rad);
                const int k = min((int)(fabsf((float)(d - m) - f) * lk), NORI_FILTER_RESOLUTION);
                wv = (d >= lo && d <= hi) ? ftab[k] : 0.0f;
            }
            wt[i] = wv;
        }
        __syncthreads();
    }
    const uint64_t WH = (uint64_t)S.W * (uint64_t)S.H;
    uint32_t inval = 0;
    for (int jj = threadIdx.x; jj < (SPLIT ? 2 : 1) * npix; jj += NT) {
        const int j = SPLIT ? jj >> 1 : jj, h = SPLIT ? jj & 1 : 0;  // h: the lane's channel pair (SPLIT)
        const int ly = j / bw, lx = j - ly * bw, x = ox + lx, y = oy + ly;
        // the window's RGBW sums as two packed pairs per cell (RG, BW; SPLIT:
        // the lane's pair): each half of a v_pk_mul_f32 / v_pk_add_f32 rounds
        // as the scalar op does
        typedef float f2 __attribute__((ext_vector_type(2)));
        f2 acc[K][K][NH];
#pragma unroll
        for (int a = 0; a < K; ++a)
#pragma unroll
            for (int c = 0; c < K; ++c)
#pragma unroll
                for (int e = 0; e < NH; ++e) acc[a][c][e] = f2{0.0f, 0.0f};
        bool any = false;
        float vs[7] = {0, 0, 0, 0, 0, 0, 0};  // sample statistics of the pixel (sd.var)
        auto put = [&](const float4 &L0, uint32_t p) {
            const uint32_t code = __float_as_uint(L0.w);
            // pending: the finisher splats this sample; Color3f::isValid
            // (common.cpp:224-231): invalid samples are dropped
            const bool pend = (code & kRecPending) != 0u;
            const bool valid = !(L0.x < 0 || !isfinite(L0.x) || L0.y < 0 || !isfinite(L0.y) || L0.z < 0 || !isfinite(L0.z));
            const bool ok = !pend && valid;
            if constexpr (!NB) {
                if (!ok) {
                    inval += (!pend && h == 0) ? 1u : 0u;
                    return;
                }
            } else {
                inval += (!pend && !valid && h == 0) ? 1u : 0u;
            }
            // NB: a skipped sample adds exact zeros -- radiance 0 and weights
            // 0 -- so the window sums keep their values bit for bit
            const float4 L = make_float4(ok ? L0.x : 0.0f, ok ? L0.y : 0.0f, ok ? L0.z : 0.0f, 0.0f);
            any = any || ok;
            vs[0] += L.x;
            vs[1] += L.y;
            vs[2] += L.z;
            vs[3] += L.x * L.x;
            vs[4] += L.y * L.y;
            vs[5] += L.z * L.z;
            vs[6] += ok ? 1.0f : 0.0f;
            float wx[K], wy[K];
            if constexpr (CODED) {
                const float4 *tx = wtab + (code & 255u) * KP, *ty = wtab + ((code >> 8) & 255u) * KP;
#pragma unroll
                for (int e = 0; e < KP; ++e) {
                    const float4 a = tx[e], b = ty[e];
                    const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
                    for (int c4 = 0; c4 < 4; ++c4)
                        if (4 * e + c4 < K) {
                            wx[4 * e + c4] = av[c4];
                            wy[4 * e + c4] = ok ? bv[c4] : 0.0f;
                        }
                }
            } else {
                uint64_t sid = (uint64_t)(sd.pass_begin + p) * WH + (uint64_t)y * S.W + x;
                Pcg r;
                wave_seed(r, sd.seed, sid);
                V2 jit = next2D(r);
                float px = ((float)x + jit.x) - 0.5f - (float)(ox - B), py = ((float)y + jit.y) - 0.5f - (float)(oy - B);
                int x0 = max((int)ceilf(px - rad), 0), y0 = max((int)ceilf(py - rad), 0);
                int x1 = min((int)floorf(px + rad), TS - 1), y1 = min((int)floorf(py + rad), TS - 1);
#pragma unroll
                for (int d = 0; d < K; ++d) {
                    int cx = lx + d, cy = ly + d;  // tile column / row of window cell d
                    int kx = min((int)(fabsf((float)cx - px) * lk), NORI_FILTER_RESOLUTION);
                    int ky = min((int)(fabsf((float)cy - py) * lk), NORI_FILTER_RESOLUTION);
                    const float fx = ftab[kx], fy = ftab[ky];  // unconditional: no branch per cell
                    wx[d] = (cx >= x0 && cx <= x1) ? fx : 0.0f;
                    wy[d] = (cy >= y0 && cy <= y1) ? fy : 0.0f;
                }
            }
            // Color4f(value) * wx (the row factor is shared by all rows); (1 * wx) = wx exactly
            f2 lp[NH][K];
            const f2 rg{L.x, L.y}, bw1{L.z, 1.0f};
#pragma unroll
            for (int c = 0; c < K; ++c)
#pragma unroll
                for (int e = 0; e < NH; ++e) lp[e][c] = (SPLIT ? (h ? bw1 : rg) : (e ? bw1 : rg)) * wx[c];
#pragma unroll
            for (int a = 0; a < K; ++a)
#pragma unroll
                for (int c = 0; c < K; ++c)
#pragma unroll
                    for (int e = 0; e < NH; ++e) acc[a][c][e] += lp[e][c] * wy[a];
        };
        // the records of the next D passes are in flight while one is splatted
        // (a ring of D registers, the pass loop unrolled by D: no moves)
        float4 Lq[D];
#pragma unroll
        for (int d = 0; d < D; ++d)
            Lq[d] = p0 + d < p1 ? rec[(size_t)(p0 + d) * sd.M + off + j] : make_float4(0, 0, 0, __uint_as_float(kRecPending));
        for (uint32_t p = p0; p < p1; p += D) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const float4 L = Lq[d];
                if (p + D + d < p1) Lq[d] = rec[(size_t)(p + D + d) * sd.M + off + j];
                if (p + d < p1) put(L, p + d);
            }
        }
        if (any && sd.var && h == 0) {
            float *v = sd.var + 8 * ((size_t)y * S.W + x);
            for (int k = 0; k < 7; ++k) atomicAdd(v + k, vs[k]);
        }
        if (any) {
#pragma unroll
            for (int a = 0; a < K; ++a)
#pragma unroll
                for (int c = 0; c < K; ++c) {
                    float *t = tile + 4 * ((ly + a) * TS + (lx + c)) + 2 * h;
                    const f2 u = acc[a][c][0], v = acc[a][c][NH - 1];
                    if (SPLIT ? (u.x != 0.0f || u.y != 0.0f) : (v.y != 0.0f || u.x != 0.0f || u.y != 0.0f || v.x != 0.0f)) {
                        atomicAdd(t + 0, u.x);
                        atomicAdd(t + 1, u.y);
                        if (!SPLIT) {
                            atomicAdd(t + 2, v.x);
                            atomicAdd(t + 3, v.y);
                        }
                    }
                }
        }
    }
    if (inval) atomicAdd(&C->invalid, (unsigned long long)inval);
    __syncthreads();
    const int rows = bh + 2 * B, cols = bw + 2 * B, FW = S.W + 2 * B;
    for (int i = threadIdx.x; i < rows * cols; i += NT) {
        int yy = i / cols, xx = i - yy * cols;
        const float *c = tile + 4 * (yy * TS + xx);
        float *f = film + 4 * ((size_t)(oy + yy) * FW + (ox + xx));
        if (c[3] != 0.0f || c[0] != 0.0f || c[1] != 0.0f || c[2] != 0.0f) {
            atomicAdd(f + 0, c[0]);
            atomicAdd(f + 1, c[1]);
            atomicAdd(f + 2, c[2]);
            atomicAdd(f + 3, c[3]);
        }
    }
}

// NORI_SPLAT_SPLIT=0: one lane per pixel in the coded splat too.
#ifndef NORI_SPLAT_SPLIT
#define NORI_SPLAT_SPLIT 1
#endif
static bool splat_split() {
    static const bool on = [] {
        const char *e = std::getenv("NORI_SPLAT_SPLIT");
        return e ? e[0] != '0' : NORI_SPLAT_SPLIT != 0;
    }();
    return on;
}
hipError_t launch_splat(const DevScene &S, const float4 *rec, const SplatDesc &sd, uint32_t nblocks, float *film,
                        Counters *C, hipStream_t st) {
    if (nblocks == 0 || sd.passes == 0) return hipSuccess;
    dim3 g(nblocks, (sd.passes + sd.passes_per_wg - 1) / sd.passes_per_wg), b(kSplatBlock);
    const bool coded = S.jit_lk != 0, split = coded && splat_split();
    const dim3 b2(kSplatSplitBlock);
#define NORI_SPLAT_CASE(b_)                                                                          \
    case b_:                                                                                         \
        if (split) hipLaunchKernelGGL((k_splat<b_, true, true>), g, b2, 0, st, S, rec, sd, film, C); \
        else if (coded) hipLaunchKernelGGL((k_splat<b_, true>), g, b, 0, st, S, rec, sd, film, C);  \
        else hipLaunchKernelGGL((k_splat<b_, false>), g, b, 0, st, S, rec, sd, film, C);            \
        break;
    switch (S.border) {
    NORI_SPLAT_CASE(0)
    NORI_SPLAT_CASE(1)
    NORI_SPLAT_CASE(2)
    NORI_SPLAT_CASE(3)
    NORI_SPLAT_CASE(4)
    default: return hipErrorInvalidValue;
    }
#undef NORI_SPLAT_CASE
    return hipGetLastError();
}

}  // namespace nori
