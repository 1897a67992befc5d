// traverse.h -- what every kernel that walks the BVH shares: the wave helpers,
// the LDS-stack traversal (traverse<STACK, ANY>), the XCD-aware block order
// and the launchers' stack-depth dispatch.  Device code for the .hip units.
#pragma once
#include <type_traits>

#include "kernels.h"
#include "scan.h"

namespace nori {

// (the wave helpers lane_id and rank_in: kernel_config.h)

// ------------------------------------------------------------------ traversal
// Load through the global address space: the scene tables sit in a struct
// of generic pointers, which would otherwise compile to FLAT loads (they also
// count against lgkmcnt, which the LDS traversal stack waits on).  BVH
// traversal always reads global memory (only scan-mode scenes are staged in LDS).
typedef float gfloat4 __attribute__((ext_vector_type(4)));
ND float4 gld(const float4 *p) {
    const gfloat4 v = *(const __attribute__((address_space(1))) gfloat4 *)p;
    return make_float4(v.x, v.y, v.z, v.w);
}

// One 4-wide BVH node: the child boxes in SoA form (mnx.x = child 0's min.x,
// ...) and the four child references (exact 128-byte nodes; quantized
// 64-byte nodes measured 9-12 % slower on C3 and the table scene, DESIGN_LOG.md).
ND void load_node(const DevScene &S, uint32_t ref, float4 &mnx, float4 &mny, float4 &mnz, float4 &mxx, float4 &mxy,
                  float4 &mxz, float4 &rf) {
    const float4 *nd = S.nodes + 8 * (size_t)ref;
    mnx = gld(nd), mny = gld(nd + 1), mnz = gld(nd + 2), mxx = gld(nd + 3), mxy = gld(nd + 4), mxz = gld(nd + 5);
    rf = gld(nd + 6);
}

// Primitive records fetched per memory round trip in a BVH leaf.
#ifndef NORI_LEAF_BATCH
#define NORI_LEAF_BATCH 1
#endif
constexpr int kLeafBatch = NORI_LEAF_BATCH;

// LDS words per lane of a traversal stack of depth STACK: child refs and entry distances.
// (stack_lds_entries(STACK) entries: the LDS budget stays STACK words, so the
// occupancy does not change; deeper entries spill to private memory)
constexpr int stack_words(int STACK) { return STACK ? STACK : 1; }

// BVH::rayIntersect (bvh.cpp:404-462): adaptive epsilon, closest or any hit.
// Near child first; the short stack lives in LDS, one column per lane.
template <int STACK, bool ANY>
ND bool traverse(const DevScene &S, TRay r, uint32_t *stk, float &tb, uint32_t &pb, float &ub, float &vb) {
    if constexpr (STACK == 0) {
        TRay rr[1] = {r};
        bool live[1] = {true}, found[1];
        float t1[1], u1[1], v1[1];
        uint32_t p1[1];
        scan_rays<1, ANY>(S, rr, live, t1, p1, u1, v1, found);
        tb = t1[0];
        pb = p1[0];
        ub = u1[0];
        vb = v1[0];
        return found[0];
    }
    if (r.mint == kEps) r.mint = smax(r.mint, r.mint * smax(smax(fabsf(r.o.x), fabsf(r.o.y)), fabsf(r.o.z)));
    tb = INF_F;
    pb = 0xFFFFFFFFu;
    ub = vb = 0.0f;
    r.rcp = V3{rcp_full(r.d.x), rcp_full(r.d.y), rcp_full(r.d.z)};
    if (r.maxt < r.mint) return false;
    // 4-wide nodes: test the four child boxes, enter the nearest hit child and
    // push the others farthest first.  Box tests are monotone (a child box lies
    // inside its parent's and rounding keeps the slab test monotone), so the
    // candidate primitives are exactly those of the reference's binary tree.
    // Stack entries carry the child's entry distance: a popped entry whose box
    // starts beyond the current closest hit is dropped unvisited -- exactly
    // the nearT <= maxt clause of its box test re-run at pop time (same ray,
    // same box, maxt only shrinks), without fetching the node.
    uint32_t spill[kTraceSpill];  // stack entries beyond the LDS part (rare)
    float spillk[kTraceSpill];
    constexpr int L = stack_lds_entries(STACK);
    auto push = [&](int &sp, uint32_t v, float k) {
        if (sp < L) {
            stk[sp * kTraceBlock] = v;
            if (NORI_STACK_KEYS) stk[(L + sp) * kTraceBlock] = __float_as_uint(k);
        } else {
            spill[sp - L] = v;
            if (NORI_STACK_KEYS) spillk[sp - L] = k;
        }
        ++sp;
    };
    uint32_t ref = 0;
    int sp = 0;
    bool found = false;
    for (;;) {
        if (!(ref & 0x80000000u)) {
            float4 mnx, mny, mnz, mxx, mxy, mxz, rf;
            load_node(S, ref, mnx, mny, mnz, mxx, mxy, mxz, rf);
            float k0, k1, k2, k3;
            bool h;
            h = box_test(make_float4(mnx.x, mny.x, mnz.x, 0), make_float4(mxx.x, mxy.x, mxz.x, 0), r, k0);
            k0 = h ? k0 : INF_F;
            const bool h0 = h;
            h = box_test(make_float4(mnx.y, mny.y, mnz.y, 0), make_float4(mxx.y, mxy.y, mxz.y, 0), r, k1);
            k1 = h ? k1 : INF_F;
            const bool h1 = h;
            h = box_test(make_float4(mnx.z, mny.z, mnz.z, 0), make_float4(mxx.z, mxy.z, mxz.z, 0), r, k2);
            k2 = h ? k2 : INF_F;
            const bool h2 = h;
            h = box_test(make_float4(mnx.w, mny.w, mnz.w, 0), make_float4(mxx.w, mxy.w, mxz.w, 0), r, k3);
            k3 = h ? k3 : INF_F;
            const bool h3 = h;
            const int nh = (int)h0 + (int)h1 + (int)h2 + (int)h3;
            if (nh > 0) {
                // order (key, ref) by entry distance; misses (key inf, hit false) sort last
                uint32_t c0 = __float_as_uint(rf.x), c1 = __float_as_uint(rf.y), c2 = __float_as_uint(rf.z),
                         c3 = __float_as_uint(rf.w);
                bool m0 = !h0, m1 = !h1, m2 = !h2, m3 = !h3;
                auto cs = [](float &ka, uint32_t &ca, bool &ma, float &kb, uint32_t &cb, bool &mb) {
                    const bool sw = ma > mb || (ma == mb && kb < ka);
                    const float tk = ka;
                    const uint32_t tc = ca;
                    const bool tm = ma;
                    ka = sw ? kb : ka;
                    kb = sw ? tk : kb;
                    ca = sw ? cb : ca;
                    cb = sw ? tc : cb;
                    ma = sw ? mb : ma;
                    mb = sw ? tm : mb;
                };
                cs(k0, c0, m0, k1, c1, m1);
                cs(k2, c2, m2, k3, c3, m3);
                cs(k0, c0, m0, k2, c2, m2);
                cs(k1, c1, m1, k3, c3, m3);
                cs(k1, c1, m1, k2, c2, m2);
                if (nh > 3) push(sp, c3, k3);
                if (nh > 2) push(sp, c2, k2);
                if (nh > 1) push(sp, c1, k1);
                ref = c0;
                continue;
            }
        } else {
            // leaf: the records of NORI_LEAF_BATCH primitives are fetched
            // together (every record is 48 B, so the third vector is loaded
            // unconditionally; lanes past the leaf end re-read its last
            // record) -- one memory round trip per batch instead of one or
            // two per primitive.  Tested in leaf order, as bvh.cpp:440-452.
            const uint32_t start = ref & 0x1FFFFFFu, end = start + ((ref >> 25) & 63u) + 1u;
            for (uint32_t i0 = start; i0 < end; i0 += kLeafBatch) {
                float4 q[kLeafBatch][3];
#pragma unroll
                for (int k = 0; k < kLeafBatch; ++k) {
                    const float4 *p = S.prims + 3 * (size_t)min(i0 + (uint32_t)k, end - 1u);
                    q[k][0] = gld(p);
                    q[k][1] = gld(p + 1);
                    q[k][2] = gld(p + 2);
                }
#pragma unroll
                for (int k = 0; k < kLeafBatch; ++k) {
                    if (i0 + (uint32_t)k >= end) break;
                    float t = 0, u = 0, v = 0;
                    bool h;
                    if (__float_as_uint(q[k][1].w) == 0u) {
                        h = tri_hit(q[k][0], q[k][1], q[k][2], r, t, u, v);
                    } else {
                        h = sphere_hit(q[k][0], q[k][1], r, t);
                        u = v = 0.0f;
                    }
                    if (h) {
                        if (ANY) return true;
                        found = true;
                        r.maxt = tb = t;
                        ub = u;
                        vb = v;
                        pb = __float_as_uint(q[k][0].w);
                    }
                }
            }
        }
        bool next = false;
        while (sp > 0) {
            --sp;
            ref = sp < L ? stk[sp * kTraceBlock] : spill[sp - L];
            if (!NORI_STACK_KEYS) {
                next = true;
                break;
            }
            const float key = sp < L ? __uint_as_float(stk[(L + sp) * kTraceBlock]) : spillk[sp - L];
            if (!(key > r.maxt)) {
                next = true;
                break;
            }
        }
        if (!next) break;
    }
    (void)STACK;
    return found;
}

// XCD-aware block order for the BVH walks (NORI_XCD_REMAP): the dispatcher
// sends work-group b to XCD b % 8, each XCD with its own 4 MB L2.  Giving XCD
// x a contiguous range of queue segments (neighbouring image chunks, so
// nearby ray origins) lets each L2 hold the part of the tree its rays visit.
// A bijection of [0, nb): XCD x takes ranks [x q + min(x, r), ... + count).
#ifndef NORI_XCD_REMAP
#define NORI_XCD_REMAP 1
#endif
constexpr uint32_t kXcds = 8;
ND uint32_t xcd_block(uint32_t b, uint32_t nb) {
    if (!NORI_XCD_REMAP) return b;
    const uint32_t x = b % kXcds, k = b / kXcds, q = nb / kXcds, r = nb % kXcds;
    return x * q + min(x, r) + k;
}

// ------------------------------------------------------------------ stack dispatch (host)
// The launchers' choice of a kernel's STACK instantiation: calls
// fn(std::integral_constant<int, N>{}) for the depth N of {0, 8, 16, 32, 64}
// within [Lo, Hi] that equals `stack`; any other request runs the Hi form.
// Only the depths in [Lo, Hi] are instantiated.
template <int Lo, int Hi, int N = 0, class F>
void with_stack(int stack, F &&fn) {
    constexpr int next = N ? 2 * N : 8;
    if constexpr (N < Lo) with_stack<Lo, Hi, next>(stack, fn);
    else if constexpr (N >= Hi) fn(std::integral_constant<int, Hi>{});
    else if (stack == N) fn(std::integral_constant<int, N>{});
    else with_stack<Lo, Hi, next>(stack, fn);
}

}  // namespace nori
