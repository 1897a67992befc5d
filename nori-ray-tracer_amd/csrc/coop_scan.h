// coop_scan.h -- the device routines only the tail finisher (k_finish,
// kernels_finish.hip) uses: the cooperative scan of its few tracing lanes and
// the body of the prefix over the segment counts.  A header of their own so
// that libnori_devtest.so (devtest.hip) can run them under a unit test
// (tests/test_gpu_finish_tail.py).  Not part of the hipRTC sources.
#pragma once
#include "kernel_config.h"
#include "scan.h"
#include "tail_index.h"

namespace nori {

// Cooperative scan (scan-mode scenes, n <= 64 primitives): the rays of the
// lanes in `want` are traced one after another by the whole wave, lane l
// testing primitive l against the broadcast ray.  The result is exactly that
// of traverse<0, ANY> for the ray: every candidate passes the test against the
// ray's own maxt, the closest wins, and among equal t the last primitive in
// scan order wins (the `t <= maxt` update).  A lone tail path then pays one
// primitive test per ray instead of n.
// Precondition: all 64 lanes of the wave call coop_load and coop_scan
// converged, wanting or not -- the scan reads rays, hits and records from
// any lane (readlane), and an inactive lane's registers are not its own.
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

// Exclusive prefix of the queued-path counts of the G segments (pre[G] =
// total): the body of k_tail_prefix, for one work-group of exactly 1024
// threads (thread t sums and then writes its `per` consecutive segments).
ND void tail_prefix(const uint32_t *cnt, uint32_t G, uint32_t *pre) {
    __shared__ uint32_t part[1024];
    const uint32_t t = threadIdx.x, per = tail_prefix_per(G), b = t * per, e = min(G, b + per);
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

}  // namespace nori
