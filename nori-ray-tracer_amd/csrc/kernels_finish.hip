// kernels_finish.hip -- the tail of a chunk: k_mark, k_tail_prefix and
// k_finish, which runs every path still queued to completion and splats its
// sample itself; the cooperative scan only the finisher uses; their launchers.
#include <algorithm>

#include "shading.h"
#include "traverse.h"

namespace nori {

// Pending marker for the samples the finisher will splat itself.
__global__ __launch_bounds__(kTraceBlock) void k_mark(PathQueue Q, SegState seg, int sel, float4 *rec) {
    const uint32_t sg = blockIdx.x >> 1, idx = (blockIdx.x & 1) * kTraceBlock + threadIdx.x;
    if (idx >= seg.cnt[sel][sg]) return;
    rec[__float_as_uint(Q.ray_d[sg * kSeg + idx].w) & kWorkMask].w = __uint_as_float(kRecPending);
}

// Cooperative scan (scan-mode scenes, n <= 64 primitives): the rays of the
// lanes in `want` are traced one after another by the whole wave, lane l
// testing primitive l against the broadcast ray.  The result is exactly that
// of traverse<0, ANY> for the ray: every candidate passes the test against the
// ray's own maxt, the closest wins, and among equal t the last primitive in
// scan order wins (the `t <= maxt` update).  A lone tail path then pays one
// primitive test per ray instead of n.
struct CoopPrim {  // lane l's primitive, loaded once per finisher wave
    float4 p0, p1, p2;  // p2.w: leaf-order position (the tie rule of scan_core)
    bool has, tri;
};
ND CoopPrim coop_load(const DevScene &S) {
    CoopPrim c;
    const uint32_t lane = lane_id();
    c.has = lane < S.num_prims;
    c.p0 = c.p1 = c.p2 = make_float4(0, 0, 0, 0);
    if (c.has) {
        const float4 *pp = S.prims + 3 * (size_t)lane;
        c.p0 = pp[0];
        c.p1 = pp[1];
        c.p2 = pp[2];
    }
    c.tri = __float_as_uint(c.p1.w) == 0u;
    return c;
}
template <bool ANY>
ND bool coop_scan(const DevScene &S, const CoopPrim &cp, const TRay &mine, bool want, float &t, uint32_t &p, float &u,
                  float &v) {
    const uint32_t lane = lane_id();
    const float4 rmn = make_float4(S.root_min[0], S.root_min[1], S.root_min[2], 0.f);
    const float4 rmx = make_float4(S.root_max[0], S.root_max[1], S.root_max[2], 0.f);
    bool res = false;
    t = INF_F;
    p = 0xFFFFFFFFu;
    u = v = 0.0f;
    auto bcast = [](float x, int j) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), j)); };
    uint64_t m = __ballot(want);
    while (m) {
        const int j = __builtin_ctzll(m);
        m &= m - 1;
        TRay r;
        r.o = V3{bcast(mine.o.x, j), bcast(mine.o.y, j), bcast(mine.o.z, j)};
        r.d = V3{bcast(mine.d.x, j), bcast(mine.d.y, j), bcast(mine.d.z, j)};
        r.mint = bcast(mine.mint, j);
        r.maxt = bcast(mine.maxt, j);
        if (r.mint == kEps) r.mint = smax(r.mint, r.mint * smax(smax(fabsf(r.o.x), fabsf(r.o.y)), fabsf(r.o.z)));
        r.rcp = V3{rcp_full(r.d.x), rcp_full(r.d.y), rcp_full(r.d.z)};
        float tn;
        const bool live = !(r.maxt < r.mint) && box_test(rmn, rmx, r, tn);
        float tl = 0, ul = 0, vl = 0;
        bool hl = false;
        if (cp.has) hl = cp.tri ? tri_hit_nb(cp.p0, cp.p1, cp.p2, r, tl, ul, vl) : sphere_hit_nb(cp.p0, cp.p1, r, tl);
        uint64_t hm = __ballot(hl && live);
        if (ANY) {
            if ((int)lane == j) res = hm != 0ull;
            continue;
        }
        if (!hm) continue;
        // closest hit over the (few) hitting lanes, the later leaf-order
        // position among equal t (scan_core's rule); t > 0, so its bits order
        // like the value and the comparison stays scalar
        uint32_t best = 0xFFFFFFFFu, best_pos = 0;
        int w = 0;
        do {
            const int l = __builtin_ctzll(hm);
            hm &= hm - 1;
            const uint32_t tb = (uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(tl + 0.0f), l);
            const uint32_t pos = (uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(cp.p2.w), l);
            if (tb < best || (tb == best && pos >= best_pos)) {
                best = tb;
                best_pos = pos;
                w = l;
            }
        } while (hm);
        const float tw = __uint_as_float(best), uw = bcast(cp.tri ? ul : 0.0f, w), vw = bcast(cp.tri ? vl : 0.0f, w);
        const uint32_t pw = (uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(cp.p0.w), w);
        if ((int)lane == j) {
            res = true;
            t = tw;
            p = pw;
            u = uw;
            v = vw;
        }
    }
    return res;
}

// At most this many tracing lanes use the cooperative scan (each costs one
// primitive test per lane and a reduction; the per-lane scan costs n tests).
#ifndef NORI_COOP_MAX
#define NORI_COOP_MAX 4
#endif
constexpr int kCoopMax = NORI_COOP_MAX;

// Exclusive prefix of the queued-path counts of the G segments (pre[G] = total).
__global__ __launch_bounds__(1024) void k_tail_prefix(const uint32_t *cnt, uint32_t G, uint32_t *pre) {
    __shared__ uint32_t part[1024];
    const uint32_t t = threadIdx.x, per = (G + 1023) / 1024, b = t * per, e = min(G, b + per);
    uint32_t sum = 0;
    for (uint32_t i = b; i < e; ++i) sum += cnt[i];
    part[t] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) {  // inclusive scan (Hillis-Steele)
        const uint32_t v = t >= off ? part[t - off] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = t ? part[t - 1] : 0u;
    for (uint32_t i = b; i < e; ++i) {
        pre[i] = run;
        run += cnt[i];
    }
    if (t == 1023) pre[G] = part[1023];
}

// Runs every path still queued to completion, one thread per path: the
// Russian-roulette tail (a glass-sphere path survives with q = 0.99 per
// bounce) would otherwise cost three launches per bounce.  Waves loop while
// any lane's path is alive so that the lanes can trace cooperatively.
#ifndef NORI_FINISH_PRIO
#define NORI_FINISH_PRIO 1
#endif
#ifndef NORI_FINISH_WAVES  // 0: 64 paths per wave
// 2048 since the glass-sphere chain (round 3): fewer finisher waves leave the
// film splat beside it more of the chip; 64-spp share 3446 -> 3550 (4096) ->
// 3652 (2048) Msamples/s, 512 spp 4737 -> 4753 / 4744 (one box, interleaved).
// 1024 since round 6's shorter glass chain: 64-spp share 4677 -> 4725 (4
// reps, every 1024 run above every 2048 run), 512 spp 5843 / 5834 (noise)
#define NORI_FINISH_WAVES 1024
#endif
constexpr uint32_t kFinishWaves = NORI_FINISH_WAVES;
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
    const uint32_t K = kFinishWaves ? min(64u, max(1u, (n + kFinishWaves - 1) / kFinishWaves)) : 64u;
    if (blockIdx.x * (kTraceBlock / 64) * K >= n) return;  // whole block idle
    // Each bounce of a tail path is a chain of dependent reads of small
    // tables; for small scenes they are staged into LDS first so the chain
    // runs at LDS latency instead of L2 latency.
    DevScene S = Sg;
    if constexpr (LDS) {  // the BVH path reads global memory (gld)
        for (uint32_t i = threadIdx.x; i < Sg.blob_bytes / 16; i += kTraceBlock) blob_lds[i] = Sg.blob[i];
        __syncthreads();
        S = scene_in_lds(Sg, reinterpret_cast<const char *>(blob_lds));
    }
    const uint32_t first = (blockIdx.x * kTraceBlock + threadIdx.x) / 64 * K, gid = first + lane_id();
    if (first >= n) return;  // whole wave idle
#if NORI_FINISH_PRIO
    // the film splat runs beside the finisher: its waves must not take the
    // issue slots of these few latency-bound ones
    __builtin_amdgcn_s_setprio(3);
#endif
    bool active = lane_id() < K && gid < n;
    uint32_t sg = 0;
    if (active) {  // segment of path gid: last s with pre[s] <= gid
        uint32_t lo = 0, hi = G;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (pre[mid] <= gid) lo = mid;
            else hi = mid;
        }
        sg = lo;
    }
    const uint32_t q = sg * kSeg + (active ? gid - pre[sg] : 0u);
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
    dim3 g(std::max<uint32_t>(2 * G, (kFinishWaves + wpb - 1) / wpb)), b(kTraceBlock);
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
