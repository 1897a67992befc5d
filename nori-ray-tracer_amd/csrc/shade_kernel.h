// shade_kernel.h -- k_shade: one vertex of every queued path (shading.h),
// the compaction of survivors and shadow rays inside the segment, and the
// regeneration of the free slots with new camera samples.
//
// Compiled twice from this one text: ahead of time into libnori_gpu.so
// (kernels_shade.hip, the 18 instantiations and launch_shade), and at context
// creation through hipRTC (rtc.hip) with NORI_CONST_SCENE and the scene's
// const_scene.h, as the single kernel nori_rtc_shade (the second head at the
// kernel below) whose two scans read the scene's records as literal operands.  Host headers stay out of it and
// of what it includes.
#pragma once
#include "kernel_config.h"
#include "shading.h"

namespace nori {

#ifndef NORI_SHADE_WAVES
#define NORI_SHADE_WAVES 5
#endif
// S.nee_inline: one LDS slot per vertex that adds to its record (a shadow ray
// and/or emission), over the blob: (o, maxt), (d, work | flags),
// (contrib, the owner thread, whose emission is in nee_em_lds)
constexpr uint32_t kNeeSlotBytes = kSeg * 3 * 16;
constexpr uint32_t kSlotEmit = 1u << 31, kSlotEm = 1u << 30;  // above kWorkMask
#ifndef NORI_SORT_OCTANT
#define NORI_SORT_OCTANT 1
#endif
// S.ext_inline (basic-plugin kernels, VAR == 0): the closest hit of the
// thread's queued ray through the wave-uniform scan, as extend_scan_body finds
// it -- the ray of path_ray (load_path computes the same mint, maxt), a wave
// whose live lanes are all camera rays through the in-plane filter, every
// other wave unchecked; both scans are exact per ray, so the hit does not
// depend on the wave's composition.  live: the lane holds a path; the others
// run the arithmetic on their stale entry and touch no memory (the records
// arrive through scalar loads).
// The scan stands after the blob is staged and the barrier taken: against
// the blob's loads held in registers across the scan, and against the scan
// before those loads are issued, that order measured fastest (DESIGN.md
// section 5).
ND float4 ext_scan(const DevScene &Sg, const PathState &ps, bool is_live) {
    TRay r[1];
    r[0].o = ps.o;
    r[0].d = ps.d;
    r[0].mint = ps.mint;
    r[0].maxt = ps.maxt;
    bool live[1] = {is_live}, f[1];
    float t[1], u[1], v[1];
    uint32_t p[1];
    if (Sg.camera_cull && Sg.plane_f && __all(!is_live || ps.cam)) scan_rays<1, false, 2>(Sg, r, live, t, p, u, v, f);
    else scan_rays<1, false, 0>(Sg, r, live, t, p, u, v, f);
    return make_float4(t[0], __uint_as_float(p[0]), u[0], v[0]);
}
// lds_bytes != 0: the scene blob is staged into LDS first, so the chains of
// dependent table reads of a vertex (shape -> bsdf -> vertices -> light CDF)
// run at LDS instead of L2 latency.
// LDS is a template parameter, not a run-time choice: with the scene pointers
// known to point into LDS the compiler emits ds_read for the table reads; a
// run-time select between the LDS and the global tables leaves generic
// pointers, i.e. flat loads (vector-memory latency, both wait counters).
// k_shade's arguments as one struct, its only parameter.  As ten parameters
// the compiler read nearly all of them from the kernel-argument segment at the
// kernel's top (C2's kernel: 34 of 36 scalar loads before the first barrier)
// and held them to their uses: 106 SGPRs, the limit, in 10 of the 18
// instantiations, and up to 76 SGPRs spilled to VGPR lanes (C2's kernel: 41
// spilled, 41 v_writelane and 68 v_readlane instructions).  As fields of
// one struct they are read where they are used: 65-102 SGPRs, none spilled,
// in every instantiation.
struct ShadeArgs {
    DevScene S;
    PathQueue in, out;
    ShadowQueue sq;
    SegState seg;
    int in_sel;
    WorkDesc wd;
    float4 *rec;
    Counters *C;
    uint32_t lds_bytes;
};
// One body under two heads: the template the library instantiates ahead of
// time, and, in the hipRTC program (rtc.hip defines NORI_RTC_INTEG and
// NORI_RTC_LDS), the one kernel nori_rtc_shade = k_shade<NORI_RTC_INTEG,
// NORI_RTC_LDS, 0> of the scene.  (The body as a function inlined into both
// kept every resource figure but changed the ahead-of-time code by a few
// instructions per kernel; this way it is the parent's, bit for bit.)
#define NORI_SHADE_KERNEL __global__ __launch_bounds__(kShadeBlock) __attribute__((amdgpu_waves_per_eu(NORI_SHADE_WAVES)))
#ifdef NORI_RTC_INTEG
extern "C" NORI_SHADE_KERNEL void nori_rtc_shade(ShadeArgs args) {
    constexpr int INTEG = NORI_RTC_INTEG, VAR = 0;
    constexpr bool LDS = NORI_RTC_LDS != 0;
#else
template <int INTEG, bool LDS, int VAR>
NORI_SHADE_KERNEL void k_shade(ShadeArgs args) {
#endif
    const auto &[Sg, in, out, sq, seg, in_sel, wd, rec, C, lds_bytes] = args;
    static_assert(kShadeBlock == kSeg, "one shade thread per segment slot");
    // VAR: 0 basic plugins only (FULL = false), 1 full, 2 full + chromatic
    // aberration (the per-channel continuation is compiled in only then)
    constexpr bool FULL = VAR != 0, CHROMA = VAR == 2;
    __shared__ uint32_t s_sh[kShadeBlock / 64], s_al[kShadeBlock / 64], s_em[kShadeBlock / 64], s_w[kSeg], s_pix[kSeg];
#if NORI_SORT_OCTANT
    __shared__ uint32_t s_oc[8 * (kShadeBlock / 64)];
    const bool sort_octant = Sg.num_nodes > 0 && Sg.blob_bytes == 0;  // BVH-traversed scenes only
#endif
    extern __shared__ __attribute__((aligned(16))) float4 blob_lds[];
    const uint32_t b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, q = b * kSeg + tid;
#ifdef NORI_PROF_SHADE  // profiling build: clocks of the kernel's phases, summed over waves
    uint64_t pt[6] = {0, 0, 0, 0, 0, 0}, pc = __builtin_amdgcn_s_memtime();
#define NORI_SPHASE(i)                                       \
    {                                                        \
        const uint64_t now = __builtin_amdgcn_s_memtime();   \
        pt[i] += now - pc;                                   \
        pc = now;                                            \
    }
#else
#define NORI_SPHASE(i)
#endif
    // every load the work-group needs is issued up front, so their latencies
    // overlap instead of adding up: the segment's bookkeeping (scalar), and
    // the path entries whether or not they hold a path (a queue slot beyond
    // the count is stale but allocated; nothing reads its values)
    const uint32_t n_in = seg.cnt[in_sel][b];
    const uint32_t cursor = seg.cursor[b];
    const uint4 st0 = seg.stats[b];
    PathState ps;
    load_path(Sg, wd, in, q, ps);
    const bool ext_in = VAR == 0 && Sg.ext_inline != 0;
    float4 hit = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!ext_in) hit = in.hit[q];
    // (a wave without a live lane scans nothing; the wave index made scalar)
    const bool ext_wave = ext_in && (uint32_t)__builtin_amdgcn_readfirstlane((int)wave) * 64u < n_in;
    // The next kSeg positions of the segment's work stream and their pixels:
    // slot j of the free slots regenerates position cursor + j.  Looked up
    // here, beside the path loads, and parked in LDS; a lookup after the
    // compaction would wait for every store and atomic issued before it
    // (vmcnt counts in issue order).  Work ids < 2^31 (runtime chunking).
    const uint64_t wspec = stream_work(wd, wd.b0 + b, cursor + tid);
    const uint32_t pspec = wspec < wd.total ? wd.pixels[(uint32_t)wspec % wd.M] : 0u;
    DevScene S = Sg;
    if constexpr (LDS) {
        for (uint32_t i = tid; i < lds_bytes / 16; i += kShadeBlock) blob_lds[i] = Sg.blob[i];
        __syncthreads();
        S = scene_in_lds(Sg, reinterpret_cast<const char *>(blob_lds));
    }
    if constexpr (VAR == 0)
        if (ext_wave) hit = ext_scan(Sg, ps, tid < n_in);
    NORI_SPHASE(0)
    ShadowOut so;
    so.emit = false;
    so.has_em = false;
    bool alive = false;
#ifdef NORI_PROF_SHADE
    __builtin_amdgcn_s_waitcnt(0);  // path loads landed: phase 1 is the shading proper
    NORI_SPHASE(0)
#endif
    if (tid < n_in) {
        alive = shade_vertex<INTEG, true, FULL>(S, ps, hit, rec, so);
        ps.cam = false;  // a survivor carries its BSDF-sampled ray (Epsilon, inf)
        if (CHROMA && !alive && ps.chan < 2) {  // the sample's next colour channel
            next_channel<FULL>(Sg, wd, ps);
            alive = true;
        }
    }
    NORI_SPHASE(1)
    s_w[tid] = wspec < wd.total ? (uint32_t)wspec : ~0u;
    s_pix[tid] = pspec;
    // ---- compaction: survivors first (in lane order), shadow rays likewise
    // (S.nee_inline: the vertices that add to their record -- a shadow ray
    // and/or emission -- into the LDS slots)
    const bool nee_in = (!FULL || kNeeFull) && Sg.nee_inline != 0;
    const bool key = so.emit || so.has_em;  // (has_em only with nee_in)
    const uint64_t mal = __ballot(alive), msh = __ballot(key), mem = __ballot(so.emit);
    if (lane_id() == 0) {
        s_al[wave] = (uint32_t)__popcll(mal);
        s_sh[wave] = (uint32_t)__popcll(msh);
        s_em[wave] = (uint32_t)__popcll(mem);
    }
    __syncthreads();
    NORI_SPHASE(2)
    uint32_t al_off = rank_in(mal), sh_off = rank_in(msh), al_tot = 0, sh_tot = 0, em_tot = 0;
    for (uint32_t w = 0; w < kShadeBlock / 64; ++w) {
        al_off += w < wave ? s_al[w] : 0u;
        sh_off += w < wave ? s_sh[w] : 0u;
        al_tot += s_al[w];
        sh_tot += s_sh[w];
        em_tot += s_em[w];
    }
#if NORI_SORT_OCTANT
    // survivors grouped by the octant of their new direction (then lane
    // order), so the waves of the BVH extension kernel get rays that visit
    // a node's children in the same order
    if (sort_octant) {
        const uint32_t oct = (ps.d.x < 0.0f ? 1u : 0u) | (ps.d.y < 0.0f ? 2u : 0u) | (ps.d.z < 0.0f ? 4u : 0u);
        uint32_t mine = 0;
        for (uint32_t o = 0; o < 8; ++o) {
            const uint64_t m = __ballot(alive && oct == o);
            if (lane_id() == 0) s_oc[o * (kShadeBlock / 64) + wave] = (uint32_t)__popcll(m);
            if (alive && oct == o) mine = rank_in(m);
        }
        __syncthreads();
        if (alive) {
            uint32_t off = mine;
            for (uint32_t o = 0; o < 8; ++o)
                for (uint32_t w = 0; w < kShadeBlock / 64; ++w)
                    off += (o < oct || (o == oct && w < wave)) ? s_oc[o * (kShadeBlock / 64) + w] : 0u;
            al_off = off;
        }
    }
#endif
    const uint32_t need_tot = kSeg - al_tot;
    // (the slots overlay the blob: the compaction's barrier above ends every
    // read of it -- regeneration and the scan below read the global tables)
    float4 *const s_sa = blob_lds, *const s_sb = s_sa + kSeg, *const s_sc = s_sb + kSeg;
    if (nee_in && key) {
        s_sa[sh_off] = make_float4(so.o.x, so.o.y, so.o.z, so.maxt);
        s_sb[sh_off] = make_float4(so.d.x, so.d.y, so.d.z,
                                   __uint_as_float(ps.work | (so.emit ? kSlotEmit : 0u) | (so.has_em ? kSlotEm : 0u)));
        s_sc[sh_off] = make_float4(so.contrib.x, so.contrib.y, so.contrib.z, __uint_as_float(tid));
    } else if (so.emit) {
        uint32_t i = b * kSeg + sh_off;
        sq.ray_o[i] = make_float4(so.o.x, so.o.y, so.o.z, kEps);
        sq.ray_d[i] = make_float4(so.d.x, so.d.y, so.d.z, so.maxt);
        sq.payload[i] = make_float4(so.contrib.x, so.contrib.y, so.contrib.z, __uint_as_float(so.work));
    }
    if (alive) store_path(out, b * kSeg + al_off, ps);
    NORI_SPHASE(3)
    // ---- regeneration: the free slots [al_tot, kSeg) take the next work ids of
    // the segment's stream, so only the tail waves run the camera-ray code and
    // a wave's new samples are adjacent pixels (stream_work increases with p)
    if (tid >= al_tot) {
        const uint32_t wn = s_w[tid - al_tot];
        if (wn != ~0u) {
            PathState np;
            regen_path<FULL>(Sg, wd, wn, s_pix[tid - al_tot], np, rec);
            store_path(out, q, np);
        }
    }
    if (nee_in) {
        // slot j = thread j (dense waves): the record is read first, so its
        // latency hides behind the scan; the shadow ray's any hit through the
        // wave-uniform scan, as k_shadow_scan; then the record += emission,
        // += the unoccluded NEE term, in the order of the separate kernels
        __syncthreads();
        if (wave * 64u < sh_tot) {
            const bool mine = tid < sh_tot;
            const uint32_t j = mine ? tid : 0u;
            const float4 a = s_sa[j], d = s_sb[j], c = s_sc[j];
            const uint32_t bits = __float_as_uint(d.w), work = bits & kWorkMask;
            const bool emit = mine && (bits & kSlotEmit) != 0u, hem = mine && (bits & kSlotEm) != 0u;
            float4 L = make_float4(0.f, 0.f, 0.f, 0.f);
            if (mine) L = rec[work];
            bool f[1] = {false};
            if (__any(emit)) {
                TRay r[1];
                r[0].o = ld3(a);
                r[0].d = ld3(d);
                r[0].mint = kEps;
                r[0].maxt = a.w;
                bool live[1] = {emit};
                float t[1], u[1], v[1];
                uint32_t p[1];
                scan_rays<1, true>(Sg, r, live, t, p, u, v, f);
            }
            bool add = false;
            if (hem) {
                const float *e = nee_em_lds() + 3 * __float_as_uint(c.w);
                L.x += e[0];
                L.y += e[1];
                L.z += e[2];
                add = true;
            }
            if (emit && !f[0]) {
                L.x += c.x;
                L.y += c.y;
                L.z += c.z;
                add = true;
            }
            if (add) rec[work] = L;
        }
    }
    NORI_SPHASE(4)
#ifdef NORI_PROF_SHADE
    __builtin_amdgcn_s_waitcnt(0);
    NORI_SPHASE(5)
    if (lane_id() == 0 && (b & 15) == 0) {  // a sample of the waves (atomics on one line)
        for (int i = 0; i < 6; ++i) atomicAdd(&C->prof[i], (unsigned long long)pt[i]);
        atomicAdd(&C->prof[6], 1ull);
    }
#endif
#undef NORI_SPHASE
    if (tid == 0) {
        // new samples = the prefix of [cursor, cursor + need_tot) still inside the stream
        uint32_t lo = 0, hi = need_tot;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (stream_work(wd, wd.b0 + b, cursor + mid) < wd.total) lo = mid + 1;
            else hi = mid;
        }
        const uint32_t fresh_tot = lo;
        seg.cnt[in_sel ^ 1][b] = al_tot + fresh_tot;
        seg.shcnt[b] = nee_in ? 0u : sh_tot;  // (inline: traced above)
        seg.cursor[b] = cursor + need_tot;
        seg.stats[b] = make_uint4(st0.x + al_tot + fresh_tot, st0.y + em_tot, st0.z + fresh_tot, st0.w);
        if (stream_work(wd, wd.b0 + b, cursor) < wd.total && stream_work(wd, wd.b0 + b, cursor + need_tot) >= wd.total) {
            // the last segment to run dry tells the host (system-scope store to
            // host-mapped memory) -- no per-iteration readback is needed
            uint32_t n = atomicAdd(&C->exhausted, 1u) + 1u;
            // progress hint: plain system-scope store (no PCIe atomics needed),
            // every 64th exhausted segment only (a store to host memory per
            // segment slowed the last iterations measurably)
            if ((n & 63u) == 0u) __hip_atomic_store(wd.done_flag + 1, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if (n == wd.G) __hip_atomic_store(wd.done_flag, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

}  // namespace nori
