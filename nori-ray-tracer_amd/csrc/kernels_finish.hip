// kernels_finish.hip -- the tail of a chunk: k_mark, k_tail_prefix and
// k_finish, which runs every path still queued to completion and splats its
// sample itself; their launchers.  The cooperative scan only the finisher
// uses and the prefix's body are in coop_scan.h, the numbering of the queued
// paths in tail_index.h.
#include <algorithm>

#include "coop_scan.h"
#include "shading.h"
#include "tail_index.h"
#include "traverse.h"

namespace nori {

// k_mark and the finisher's grid run two work-groups of kTraceBlock threads
// per segment, in whole waves.
static_assert(kSeg == 2 * kTraceBlock, "k_mark and the 2 * G grid of k_finish: two work-groups per segment");
static_assert(kTraceBlock % 64 == 0, "k_finish numbers its paths per wave");

// Pending marker for the samples the finisher will splat itself.
__global__ __launch_bounds__(kTraceBlock) void k_mark(PathQueue Q, SegState seg, int sel, float4 *rec) {
    const uint32_t sg = blockIdx.x >> 1, idx = (blockIdx.x & 1) * kTraceBlock + threadIdx.x;
    if (idx >= seg.cnt[sel][sg]) return;
    rec[__float_as_uint(Q.ray_d[sg * kSeg + idx].w) & kWorkMask].w = __uint_as_float(kRecPending);
}

// Exclusive prefix of the queued-path counts of the G segments (pre[G] = total).
__global__ __launch_bounds__(1024) void k_tail_prefix(const uint32_t *cnt, uint32_t G, uint32_t *pre) {
    tail_prefix(cnt, G, pre);
}

// Runs every path still queued to completion, one thread per path: the
// Russian-roulette tail (a glass-sphere path survives with q = 0.99 per
// bounce) would otherwise cost three launches per bounce.  Waves loop while
// any lane's path is alive so that the lanes can trace cooperatively.
#ifndef NORI_FINISH_PRIO
#define NORI_FINISH_PRIO 1
#endif
#ifndef NORI_FINISH_GLASS  // 0: the tail finisher shades glass-sphere vertices generically
#define NORI_FINISH_GLASS 1
#endif
constexpr bool kFinishGlass = NORI_FINISH_GLASS;
template <int STACK, int INTEG, bool LDS, int VAR>  // LDS: the scene blob is staged (scan-mode scenes); VAR: see k_shade
__global__ __launch_bounds__(kTraceBlock) void k_finish(DevScene Sg, PathQueue Q, SegState seg, int sel,
                                                        float4 *rec, WorkDesc wd, float *film, Counters *C,
                                                        const uint32_t *pre, uint32_t G) {
    __shared__ uint32_t stk[stack_words(STACK) * kTraceBlock];
    extern __shared__ __attribute__((aligned(16))) float4 blob_lds[];
    // the queued paths of all segments, numbered through the prefix `pre`
    // (k_tail_prefix), K consecutive ones per wave: K = n / kFinishWaves
    // rounded up, so the tail spreads over about kFinishWaves waves.  The
    // render waits for the longest path, and a lane's bounce costs the sum of
    // the branches its wave-mates take: few paths per wave keep that chain
    // close to the lone-lane latency from its first bounce on.
    constexpr bool FULL = VAR != 0, CHROMA = VAR == 2;
    const uint32_t n = pre[G];
    const uint32_t K = tail_paths_per_wave(n);
    if (tail_block_first(blockIdx.x, kTraceBlock / 64, K) >= n) return;  // whole block idle
    // Each bounce of a tail path is a chain of dependent reads of small
    // tables; for small scenes they are staged into LDS first so the chain
    // runs at LDS latency instead of L2 latency.
    DevScene S = Sg;
    if constexpr (LDS) {  // the BVH path reads global memory (gld)
        for (uint32_t i = threadIdx.x; i < Sg.blob_bytes / 16; i += kTraceBlock) blob_lds[i] = Sg.blob[i];
        __syncthreads();
        S = scene_in_lds(Sg, reinterpret_cast<const char *>(blob_lds));
    }
    const uint32_t first = tail_first(blockIdx.x * kTraceBlock + threadIdx.x, K), gid = first + lane_id();
    if (first >= n) return;  // whole wave idle
#if NORI_FINISH_PRIO
    // the film splat runs beside the finisher: its waves must not take the
    // issue slots of these few latency-bound ones
    __builtin_amdgcn_s_setprio(3);
#endif
    bool active = lane_id() < K && gid < n;
    uint32_t sg = 0;
    if (active) sg = tail_segment(pre, G, gid);  // last s with pre[s] <= gid
    const uint32_t q = active ? tail_slot(pre, sg, gid) : 0u;  // (sg = 0 for an idle lane)
    PathState ps;
    float4 h = make_float4(0, 0, 0, 0);
    if (active) {
        load_path(Sg, wd, Q, q, ps);
        h = Q.hit[q];
        ps.L = ld3(rec[ps.work]);
    }
    uint32_t rays = 0;
    const bool coop = STACK == 0 && S.num_prims <= 64;
    CoopPrim cp;
    if (coop) cp = coop_load(S);
    auto trace = [&](const TRay &r, bool want, bool any_hit, float &t, uint32_t &p, float &u, float &v) -> bool {
        if (coop && __popcll(__ballot(want)) <= kCoopMax)
            return any_hit ? coop_scan<true>(S, cp, r, want, t, p, u, v) : coop_scan<false>(S, cp, r, want, t, p, u, v);
        if (!want) return false;
        return any_hit ? traverse<STACK, true>(S, r, stk + threadIdx.x, t, p, u, v)
                       : traverse<STACK, false>(S, r, stk + threadIdx.x, t, p, u, v);
    };
#ifdef NORI_PROF_FINISH  // profiling build: clocks of the loop's phases, summed over waves
    // pt: shader clocks (s_memtime) of every iteration; p1: wall time (s_memrealtime,
    // 100 MHz) of the late iterations (index >= NORI_PROF_LATE) of long-running
    // waves, when the device runs little else: the lone-lane bounce
#ifndef NORI_PROF_LATE
#define NORI_PROF_LATE 200
#endif
    uint64_t pt[4] = {0, 0, 0, 0}, pc = __builtin_amdgcn_s_memtime(), rt0 = __builtin_amdgcn_s_memrealtime(), wit = 0;
    uint64_t p1[4] = {0, 0, 0, 0}, n1 = 0, rc = rt0;
    bool solo = false;
#define NORI_PHASE(i)                                        \
    {                                                        \
        const uint64_t now = __builtin_amdgcn_s_memtime();   \
        pt[i] += now - pc;                                   \
        pc = now;                                            \
        const uint64_t rnow = __builtin_amdgcn_s_memrealtime(); \
        if (solo) p1[i] += rnow - rc;                        \
        rc = rnow;                                           \
    }
#else
#define NORI_PHASE(i)
#endif
    while (__ballot(active)) {
#ifdef NORI_PROF_FINISH
        solo = wit >= NORI_PROF_LATE;
        n1 += solo ? 1 : 0;
        rc = __builtin_amdgcn_s_memrealtime();
#endif
        ShadowOut so;
        so.emit = false;
        bool alive = false;
        // the shape of the vertex being shaded, if it is a solitary sphere (its
        // table reads issued before the shading, off the dependency chain)
        int sol = -1;  // (volumetric: a scattering event moves the origin off the surface)
        if (INTEG != NORI_INTEGRATOR_VOLUMETRIC && active && __float_as_uint(h.y) != 0xFFFFFFFFu) {
            const int s0 = (int)S.prim_shape[__float_as_uint(h.y)];
            sol = S.shapes[s0].solitary ? s0 : -1;
        }
        // a vertex on a solitary glass sphere: the chain of its chord bounces
        // runs here (glass_bounce, chord_hit) until the path leaves the
        // sphere or ends, or its NEE could no longer be skipped
        bool shaded = false;  // this iteration's vertex is shaded, ps holds the next ray
        if (INTEG != NORI_INTEGRATOR_VOLUMETRIC && kFinishGlass && active && sol >= 0) {
            // copies: the chain's constants are read from LDS once, before
            // the loop, and kept in registers (not re-read per bounce)
            const DevShape gs = S.shapes[sol];
            const DevBsdf gb = S.bsdfs[gs.bsdf];
            if (gb.type == NORI_BSDF_DIELECTRIC && gs.emitter < 0) {
#ifdef NORI_PROF_GLASS  // diagnostic build: wall time of lone-lane chains per chord bounce
                const bool lone = __popcll(__ballot(active)) == 1;
                const uint64_t g0 = __builtin_amdgcn_s_memrealtime();
                const uint32_t r0 = rays;
#endif
                while (INTEG != NORI_INTEGRATOR_PATH_MIS || skip_nee(S, gb, ps.beta)) {
                    if (kGlassStep)  // reflected into the next chord, as long as it lasts
                        while (glass_step<INTEG>(gs, gb, ps, h.x)) ++rays;
                    alive = glass_bounce<INTEG>(gs, gb, ps, h.x);
                    shaded = true;
                    if (!alive) break;
                    float tc;
                    if (!chord_hit<kGlassFast>(gs, ps, tc)) {
                        sol = -1;  // it leaves the sphere: traced below
                        break;
                    }
                    h = make_float4(tc, __uint_as_float(gs.prim_offset), 0.0f, 0.0f);
                    ++rays;
                    shaded = false;
                }
#ifdef NORI_PROF_GLASS
                if (lone && rays - r0 >= 8) {
                    atomicAdd(&C->prof[13], (unsigned long long)(__builtin_amdgcn_s_memrealtime() - g0));
                    atomicAdd(&C->prof[14], (unsigned long long)(rays - r0));
                }
#endif
            }
        }
        if (active && !shaded) alive = shade_vertex<INTEG, false, FULL>(S, ps, h, rec, so);
        NORI_PHASE(0)
        {
            TRay r{so.o, so.d, V3{0, 0, 0}, kEps, so.maxt};
            float t, u, v;
            uint32_t p;
            rays += so.emit ? 1u : 0u;
            bool occluded = trace(r, so.emit, true, t, p, u, v);
            if (so.emit && !occluded) ps.L = ps.L + so.contrib;  // so.work == ps.work
        }
        NORI_PHASE(1)
        if (CHROMA && active && !alive && ps.chan < 2) {  // the sample's next colour channel
            next_channel<FULL>(Sg, wd, ps);
            alive = true;
            sol = -1;  // a camera ray
        }
        if (active && !alive) {
            active = false;
            // the sample is complete: splat it (k_splat skipped it as pending)
            const uint32_t w = ps.work, pass = w / wd.M, e = w - pass * wd.M, pix = wd.pixels[e];
            const uint32_t y = pix / (uint32_t)S.W, x = pix - y * (uint32_t)S.W;
            Pcg rg;
            wave_seed(rg, wd.seed, (uint64_t)(wd.pass_begin + pass) * ((uint64_t)S.W * (uint64_t)S.H) + pix);
            V2 jit = next2D(rg);
            // Sg: kernarg filter table (no local copy)
            splat_sample(Sg, film, C, x, y, jit, make_float4(ps.L.x, ps.L.y, ps.L.z, 0.0f), wd.var);
            atomicAdd(&seg.stats[sg].w, rays);
            atomicAdd(&C->finish_paths, 1u);
            atomicMax(&C->finish_max_rays, rays);
        }
        TRay r{ps.o, ps.d, V3{0, 0, 0}, ps.mint, ps.maxt};
        float t, u, v;
        uint32_t p;
        rays += active ? 1u : 0u;
        NORI_PHASE(2)
        // a path leaving a solitary sphere: its chord, if it has one, is the
        // closest hit (the glass-sphere paths of the tail bounce inside)
        bool want = active;
        if (active && sol >= 0) {
            float tc;
            if (chord_hit(S.shapes[sol], ps, tc)) {
                h = make_float4(tc, __uint_as_float(S.shapes[sol].prim_offset), 0.0f, 0.0f);
                want = false;
            }
        }
        trace(r, want, false, t, p, u, v);
        if (want) h = make_float4(t, __uint_as_float(p), u, v);
        NORI_PHASE(3)
#ifdef NORI_PROF_FINISH
        if (lane_id() == 0) atomicAdd(&C->prof[4], 1ull);
        ++wit;
#endif
    }
#ifdef NORI_PROF_FINISH
    if (lane_id() == 0) {
        for (int i = 0; i < 4; ++i) atomicAdd(&C->prof[i], (unsigned long long)pt[i]);
        for (int i = 0; i < 4; ++i) atomicAdd(&C->prof[8 + i], (unsigned long long)p1[i]);
        atomicAdd(&C->prof[12], (unsigned long long)n1);
        // the longest-running wave: its span in 100 MHz ticks (high bits) and loop iterations
        const uint64_t span = __builtin_amdgcn_s_memrealtime() - rt0;
        atomicMax(&C->prof[5], (unsigned long long)((span << 20) | (wit & 0xFFFFFu)));
    }
#endif
#undef NORI_PHASE
}

template <int INTEG, int VAR>
static void finish_dispatch(const DevScene &S, const PathQueue &Q, const SegState &seg, int sel, float4 *rec,
                            const WorkDesc &wd, float *film, Counters *C, uint32_t G, int stack, uint32_t *pre,
                            hipStream_t st) {
    // enough waves for any path count n <= 256 G (kFinishWaves, or n / 64 <= 4 G when
    // K = 64); the idle blocks exit at once
    constexpr uint32_t wpb = kTraceBlock / 64;  // waves per block
    dim3 g(tail_grid(G, wpb)), b(kTraceBlock);
    with_stack<0, 64>(stack, [&](auto N) {
        if constexpr (N() == 0) {  // LDS-staged when the scene has a blob
            if (S.blob_bytes) {
                hipLaunchKernelGGL((k_finish<0, INTEG, true, VAR>), g, b, S.blob_bytes, st, S, Q, seg, sel, rec, wd, film, C, pre, G);
                return;
            }
        }
        hipLaunchKernelGGL((k_finish<N(), INTEG, false, VAR>), g, b, 0, st, S, Q, seg, sel, rec, wd, film, C, pre, G);
    });
}
template <int INTEG>
static void finish_dispatch(const DevScene &S, const PathQueue &Q, const SegState &seg, int sel, float4 *rec,
                            const WorkDesc &wd, float *film, Counters *C, uint32_t G, int stack, uint32_t *pre,
                            hipStream_t st) {
    if (S.basic) finish_dispatch<INTEG, 0>(S, Q, seg, sel, rec, wd, film, C, G, stack, pre, st);
    else if (S.chroma) finish_dispatch<INTEG, 2>(S, Q, seg, sel, rec, wd, film, C, G, stack, pre, st);
    else finish_dispatch<INTEG, 1>(S, Q, seg, sel, rec, wd, film, C, G, stack, pre, st);
}
hipError_t launch_mark(const PathQueue &Q, const SegState &seg, int sel, float4 *rec, uint32_t G, hipStream_t st) {
    hipLaunchKernelGGL(k_mark, dim3(2 * G), dim3(kTraceBlock), 0, st, Q, seg, sel, rec);
    return hipGetLastError();
}
hipError_t launch_tail_prefix(const SegState &seg, int sel, uint32_t G, uint32_t *pre, hipStream_t st) {
    hipLaunchKernelGGL(k_tail_prefix, dim3(1), dim3(1024), 0, st, seg.cnt[sel], G, pre);
    return hipGetLastError();
}
hipError_t launch_finish(const DevScene &S, const PathQueue &Q, const SegState &seg, int sel, float4 *rec,
                         const WorkDesc &wd, float *film, Counters *C, uint32_t G, int stack, uint32_t *pre,
                         hipStream_t st) {
    if (S.integrator == NORI_INTEGRATOR_PATH_MATS)
        finish_dispatch<NORI_INTEGRATOR_PATH_MATS>(S, Q, seg, sel, rec, wd, film, C, G, stack, pre, st);
    else if (S.integrator == NORI_INTEGRATOR_VOLUMETRIC)
        finish_dispatch<NORI_INTEGRATOR_VOLUMETRIC>(S, Q, seg, sel, rec, wd, film, C, G, stack, pre, st);
    else
        finish_dispatch<NORI_INTEGRATOR_PATH_MIS>(S, Q, seg, sel, rec, wd, film, C, G, stack, pre, st);
    return hipGetLastError();
}

}  // namespace nori
