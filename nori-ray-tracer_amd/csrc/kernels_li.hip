// kernels_li.hip -- k_li: Integrator::Li for the caller's rays, one path per
// lane from its first segment to its end (nori_gpu_li, stated in nori_gpu.h),
// and its launcher.  The path integrators run the per-lane loop of the tail
// finisher (kernels_finish.hip) on shading.h's generic vertex routine, the
// one-bounce integrators OneBounce::Li as k_direct calls it; tracing is the
// generic traverse<STACK>.  Nothing here knows a camera: the per-channel
// masking of a chromatic sample (chan_only) is switched off by the launcher.
#include <algorithm>

#include "onebounce.h"

namespace nori {

namespace {

// The ray of row i, or false when the row is not traced (three zeros): a
// component of o or d, or mint, not finite; maxt NaN; d zero.
ND bool li_load(const LiArgs &a, uint32_t i, V3 &o, V3 &d, float &mint, float &maxt) {
    const float4 ro = a.rays[2 * (size_t)i], rd = a.rays[2 * (size_t)i + 1];
    o = ld3(ro);
    d = ld3(rd);
    mint = ro.w;
    maxt = rd.w;
    const bool fin = isfinite(o.x) && isfinite(o.y) && isfinite(o.z) && isfinite(d.x) && isfinite(d.y) &&
                     isfinite(d.z) && isfinite(mint);
    return fin && !(maxt != maxt) && !(d.x == 0.0f && d.y == 0.0f && d.z == 0.0f);
}
// Row i's sampler: its stream after first_draw calls of next1D.
ND void li_seed(const LiArgs &a, uint32_t i, Pcg &rng) {
    wave_seed(rng, a.seed, a.ids ? a.ids[i] : a.stream_base + i);
    pcg_skip(rng, (int)a.first_draw);
}
// Writes row i; returns 1 if the value fails Color3f::isValid (it is written as computed).
ND uint32_t li_store(const LiArgs &a, uint32_t i, const V3 &L) {
    float *o = a.out + 3 * (size_t)i;
    o[0] = L.x;
    o[1] = L.y;
    o[2] = L.z;
    return (L.x < 0 || !isfinite(L.x) || L.y < 0 || !isfinite(L.y) || L.z < 0 || !isfinite(L.z)) ? 1u : 0u;
}

}  // namespace

// Wave w owns rows [w range, (w + 1) range).  One-bounce integrators: lane l
// takes rows l, l + 64, ... of the range.  Path integrators: a lane whose path
// has ended takes the next unstarted row of the range -- the free lanes'
// ballot, the lane's rank in it and a wave-uniform cursor, no atomics, and the
// lanes that load are consecutive in row index -- so a wave does not wait for
// its longest path with idle lanes (a path trapped in a glass sphere survives
// each bounce with probability 0.99).  refill = 0: rows are taken once, at the
// start (the launcher then gives every wave 64 rows).  Every row has its
// own stream and output, and traverse is exact per ray: the result does not
// depend on which wave, lane or iteration computes a row.
template <int STACK, int INTEG, bool LDS, bool FULL>
__global__ __launch_bounds__(kTraceBlock) void k_li(DevScene Sg, LiArgs a) {
    __shared__ uint32_t stk[stack_words(STACK) * kTraceBlock];
    extern __shared__ __attribute__((aligned(16))) float4 blob_lds[];
    DevScene S = Sg;
    if constexpr (LDS) {  // small scenes: the tables at LDS latency (k_finish does the same)
        for (uint32_t i = threadIdx.x; i < Sg.blob_bytes / 16; i += kTraceBlock) blob_lds[i] = Sg.blob[i];
        __syncthreads();
        S = scene_in_lds(Sg, reinterpret_cast<const char *>(blob_lds));
    }
    // each XCD sweeps a contiguous part of the rows (k_direct's order): neighbouring rays share tree nodes
    const uint32_t bid = STACK ? xcd_block(blockIdx.x, gridDim.x) : blockIdx.x;
    const uint32_t wave = bid * (kTraceBlock / 64) + threadIdx.x / 64;
    const uint64_t b64 = (uint64_t)wave * a.range;
    if (b64 >= a.n) return;  // whole wave idle
    const uint32_t begin = (uint32_t)b64, end = b64 + a.range < a.n ? (uint32_t)(b64 + a.range) : a.n;
    uint32_t *const lstk = stk + threadIdx.x;
    uint32_t rc = 0, rs = 0, bad = 0;  // closest-hit rays, shadow rays, invalid rows
    constexpr bool PATH = INTEG == NORI_INTEGRATOR_PATH_MATS || INTEG == NORI_INTEGRATOR_PATH_MIS ||
                          INTEG == NORI_INTEGRATOR_VOLUMETRIC;
    if constexpr (!PATH) {
        OneBounce<STACK> ob{S, lstk};
        for (uint32_t i = begin + lane_id(); i < end; i += 64) {
            V3 o, d;
            float mint, maxt;
            V3 L{0, 0, 0};
            if (li_load(a, i, o, d, mint, maxt)) {
                Pcg rng;
                li_seed(a, i, rng);
                L = ob.template Li<INTEG>(rng, o, d, mint, maxt);
            }
            bad += li_store(a, i, L);
        }
        rc = ob.rc;
        rs = ob.rs;
    } else {
        uint32_t cursor = begin;  // wave-uniform: the next unstarted row
        bool active = false, fresh = false, started = false;
        PathState ps;
        ps.L = V3{0, 0, 0};
        ps.work = 0;
        float4 h = make_float4(0, 0, 0, 0);
        for (;;) {
            const uint64_t fm = __ballot(!active);
            const uint32_t nfree = (uint32_t)__popcll(fm);
            if (cursor < end && nfree && (a.refill || !started)) {
                const uint32_t i = cursor + rank_in(fm);
                if (!active && i < end) {
                    if (li_load(a, i, ps.o, ps.d, ps.mint, ps.maxt)) {
                        li_seed(a, i, ps.rng);
                        ps.beta = V3{1, 1, 1};
                        ps.prev = -1.0f;
                        ps.cam = false;
                        ps.chan = 0;
                        ps.invz = 0.0f;
                        ps.L = V3{0, 0, 0};
                        ps.work = i;
                        active = fresh = true;
                    } else {
                        li_store(a, i, V3{0, 0, 0});
                    }
                }
                cursor += min(nfree, end - cursor);
                started = true;
            }
            if (!__ballot(active)) {
                if (cursor >= end || !a.refill) break;
                continue;  // every row taken was a row that is not traced
            }
            // the vertex at the hit of the lane's segment (a fresh lane has no hit yet)
            ShadowOut so;
            so.emit = false;
            bool alive = active;
            if (active && !fresh) alive = shade_vertex<INTEG, false, FULL>(S, ps, h, nullptr, so);
            if (so.emit) {  // next-event estimation: added after the vertex's emission, if unoccluded
                ++rs;
                const TRay r{so.o, so.d, V3{0, 0, 0}, kEps, so.maxt};
                float t, u, v;
                uint32_t p;
                if (!traverse<STACK, true>(S, r, lstk, t, p, u, v)) ps.L = ps.L + so.contrib;
            }
            if (active && !alive) {
                active = false;
                bad += li_store(a, ps.work, ps.L);
            }
            if (active) {  // the next segment (the first one carries the caller's interval)
                ++rc;
                const TRay r{ps.o, ps.d, V3{0, 0, 0}, ps.mint, ps.maxt};
                float t, u, v;
                uint32_t p;
                traverse<STACK, false>(S, r, lstk, t, p, u, v);
                h = make_float4(t, __uint_as_float(p), u, v);
            }
            fresh = false;
        }
    }
    // counters: one reduction and one atomic each per wave
    for (int off = 32; off > 0; off >>= 1) {
        rc += __shfl_xor(rc, off);
        rs += __shfl_xor(rs, off);
        bad += __shfl_xor(bad, off);
    }
    if (lane_id() == 0) {
        if (rc) atomicAdd(&a.counters[0], (unsigned long long)rc);
        if (rs) atomicAdd(&a.counters[1], (unsigned long long)rs);
        if (bad) atomicAdd(&a.counters[2], (unsigned long long)bad);
    }
}

namespace {

template <int INTEG, bool FULL>
void li_dispatch(const DevScene &S, const LiArgs &a, int stack, hipStream_t st) {
    const uint32_t waves = (uint32_t)(((uint64_t)a.n + a.range - 1) / a.range), wpb = kTraceBlock / 64;
    const dim3 g((waves + wpb - 1) / wpb), b(kTraceBlock);
    constexpr bool PATH = INTEG == NORI_INTEGRATOR_PATH_MATS || INTEG == NORI_INTEGRATOR_PATH_MIS ||
                          INTEG == NORI_INTEGRATOR_VOLUMETRIC;
    with_stack<0, PATH ? 64 : 32>(stack, [&](auto N) {
        if constexpr (N() == 0 && PATH) {
            if (S.blob_bytes) {  // LDS-staged when the scene has a blob (11 % on the Cornell box, DESIGN_LOG.md)
                hipLaunchKernelGGL((k_li<0, INTEG, true, FULL>), g, b, S.blob_bytes, st, S, a);
                return;
            }
        }
        hipLaunchKernelGGL((k_li<N(), INTEG, false, FULL>), g, b, 0, st, S, a);
    });
}
template <int INTEG>
void li_path(const DevScene &S, const LiArgs &a, int stack, hipStream_t st) {
    if (S.basic) li_dispatch<INTEG, false>(S, a, stack, st);
    else li_dispatch<INTEG, true>(S, a, stack, st);
}

}  // namespace

hipError_t launch_li(const DevScene &Sc, const LiArgs &args, int stack, hipStream_t st) {
    if (args.n == 0) return hipSuccess;
    if (args.range < 64 || !args.rays || !args.out || !args.counters) return hipErrorInvalidValue;
    DevScene S = Sc;
    S.chroma = 0;  // Li knows no camera: all three channels of every term (chan_only)
    LiArgs a = args;
    if (!a.refill) a.range = 64;  // one row per lane
    switch (S.integrator) {
    case NORI_INTEGRATOR_PATH_MATS: li_path<NORI_INTEGRATOR_PATH_MATS>(S, a, stack, st); break;
    case NORI_INTEGRATOR_PATH_MIS: li_path<NORI_INTEGRATOR_PATH_MIS>(S, a, stack, st); break;
    case NORI_INTEGRATOR_VOLUMETRIC: li_path<NORI_INTEGRATOR_VOLUMETRIC>(S, a, stack, st); break;
    case NORI_INTEGRATOR_NORMALS: li_dispatch<NORI_INTEGRATOR_NORMALS, true>(S, a, stack, st); break;
    case NORI_INTEGRATOR_AV: li_dispatch<NORI_INTEGRATOR_AV, true>(S, a, stack, st); break;
    case NORI_INTEGRATOR_DIRECT: li_dispatch<NORI_INTEGRATOR_DIRECT, true>(S, a, stack, st); break;
    case NORI_INTEGRATOR_DIRECT_EMS: li_dispatch<NORI_INTEGRATOR_DIRECT_EMS, true>(S, a, stack, st); break;
    case NORI_INTEGRATOR_DIRECT_MATS: li_dispatch<NORI_INTEGRATOR_DIRECT_MATS, true>(S, a, stack, st); break;
    case NORI_INTEGRATOR_DIRECT_MIS: li_dispatch<NORI_INTEGRATOR_DIRECT_MIS, true>(S, a, stack, st); break;
    case NORI_INTEGRATOR_PHOTONMAPPER: li_dispatch<NORI_INTEGRATOR_PHOTONMAPPER, true>(S, a, stack, st); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace nori
