// refit.hip -- dynamic geometry on the device (nori_gpu_update_vertices).
//
// New vertex positions replace the old ones in place, the triangle records
// are rewritten from them and the 4-wide BVH is refitted bottom-up: the tree's
// topology, child refs, leaf ranges and leaf order stay, only the boxes
// change.  The refit is stated once, at nori_scene_bvh_refit in
// include/nori_gpu.h (bvh_refit.cpp computes it on the host); the kernels give
// the same bytes: the records are differences of two fp32 values (contraction
// is off, nothing to fuse), the boxes are min / max with ordered zeros
// (refit.h), which do not round.
//
// Every kernel is one thread per item with plain vector loads and stores, no
// atomics on the data and no waiting between work-groups: the order the
// boxes need (children before parents) is the order of the LAUNCHES, one per
// level of the schedule the host made at nori_gpu_create (RefitPlan,
// host_scene.h).  Two threads never write the same word: a (node, slot)
// thread writes lane `slot` of the node's six box rows.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "refit.h"

namespace nori {

namespace {

constexpr int kRefitBlock = 256;

// Non-finite values among the n floats of a (and of b, if given), added to *count.
__global__ __launch_bounds__(kRefitBlock) void k_refit_count_nonfinite(const float *__restrict__ a,
                                                                       const float *__restrict__ b, size_t n,
                                                                       uint32_t *__restrict__ count) {
    const size_t i = (size_t)blockIdx.x * kRefitBlock + threadIdx.x;
    bool bad = false;
    if (i < n) {
        bad = refit_nonfinite(a[i]);
        if (b) bad = bad || refit_nonfinite(b[i]);
    }
    const unsigned long long m = __ballot(bad);
    if (m != 0ull && (threadIdx.x & 63) == 0) atomicAdd(count, (uint32_t)__popcll(m));
}

// pos[v].xyz = p[3v ..], nrm[v].xyz = n[3v ..] (n may be null); the w lanes (texture u, v) are kept.
__global__ __launch_bounds__(kRefitBlock) void k_refit_set_vertices(float4 *__restrict__ pos, float4 *__restrict__ nrm,
                                                                    const float *__restrict__ p,
                                                                    const float *__restrict__ n, uint32_t V) {
    const uint32_t v = blockIdx.x * kRefitBlock + threadIdx.x;
    if (v >= V) return;
    const size_t s = 3 * (size_t)v;
    float4 o = pos[v];
    o.x = p[s], o.y = p[s + 1], o.z = p[s + 2];
    pos[v] = o;
    if (n) {
        float4 q = nrm[v];
        q.x = n[s], q.y = n[s + 1], q.z = n[s + 2];
        nrm[v] = q;
    }
}

// Leaf-order record i of a triangle: (p0 | id), (p1 - p0 | w kept), (p2 - p0 | w kept).
// A sphere's record (p1.w == 1) is left alone.
__global__ __launch_bounds__(kRefitBlock) void k_refit_records(float4 *__restrict__ prims,
                                                               const uint32_t *__restrict__ vidx,
                                                               const float4 *__restrict__ pos, uint32_t P) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i >= P) return;
    float4 *r = prims + 3 * (size_t)i;
    float4 r0 = r[0], r1 = r[1], r2 = r[2];
    if (__float_as_uint(r1.w) == 1u) return;
    const uint32_t *f = vidx + 3 * (size_t)__float_as_uint(r0.w);
    const float4 p0 = pos[f[0]], p1 = pos[f[1]], p2 = pos[f[2]];
    r0.x = p0.x, r0.y = p0.y, r0.z = p0.z;
    r1.x = p1.x - p0.x, r1.y = p1.y - p0.y, r1.z = p1.z - p0.z;
    r2.x = p2.x - p0.x, r2.y = p2.y - p0.y, r2.z = p2.z - p0.z;
    r[0] = r0, r[1] = r1, r[2] = r2;
}

struct Box {
    float mn[3], mx[3];
    bool any;
    __device__ void add(float lx, float ly, float lz, float hx, float hy, float hz) {
        mn[0] = any ? box_min(mn[0], lx) : lx, mn[1] = any ? box_min(mn[1], ly) : ly, mn[2] = any ? box_min(mn[2], lz) : lz;
        mx[0] = any ? box_max(mx[0], hx) : hx, mx[1] = any ? box_max(mx[1], hy) : hy, mx[2] = any ? box_max(mx[2], hz) : hz;
        any = true;
    }
};

// One thread per (node, child slot) of a level of the schedule.  A leaf slot
// takes the min / max of its (<= 64) primitives' vertex positions, read from
// pos (not v0 + e1, which can differ by an ulp), or centre -/+ radius for a
// sphere; an inner slot the min / max over the used slots of its child node,
// which an earlier launch wrote.
__global__ __launch_bounds__(kRefitBlock) void k_refit_level(float *__restrict__ nodes,
                                                             const float4 *__restrict__ prims,
                                                             const uint32_t *__restrict__ vidx,
                                                             const float4 *__restrict__ pos,
                                                             const uint32_t *__restrict__ slots, uint32_t n) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = slots[i], k = s & 3u;
    float *nd = nodes + 32 * (size_t)(s >> 2);
    const uint32_t ref = __float_as_uint(nd[24 + k]);
    Box b;
    b.any = false;
    if (ref & kRefitLeafBit) {
        const uint32_t first = refit_leaf_first(ref), last = first + refit_leaf_count(ref);
        for (uint32_t j = first; j < last; ++j) {
            const float4 r0 = prims[3 * (size_t)j], r1 = prims[3 * (size_t)j + 1];
            if (__float_as_uint(r1.w) == 1u) {
                b.add(r0.x - r1.x, r0.y - r1.x, r0.z - r1.x, r0.x + r1.x, r0.y + r1.x, r0.z + r1.x);
            } else {
                const uint32_t *f = vidx + 3 * (size_t)__float_as_uint(r0.w);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float4 p = pos[f[c]];
                    b.add(p.x, p.y, p.z, p.x, p.y, p.z);
                }
            }
        }
    } else {
        const float4 *ch = reinterpret_cast<const float4 *>(nodes + 32 * (size_t)ref);
        const float4 lx = ch[0], ly = ch[1], lz = ch[2], hx = ch[3], hy = ch[4], hz = ch[5];
        if (!refit_unused(lx.x)) b.add(lx.x, ly.x, lz.x, hx.x, hy.x, hz.x);
        if (!refit_unused(lx.y)) b.add(lx.y, ly.y, lz.y, hx.y, hy.y, hz.y);
        if (!refit_unused(lx.z)) b.add(lx.z, ly.z, lz.z, hx.z, hy.z, hz.z);
        if (!refit_unused(lx.w)) b.add(lx.w, ly.w, lz.w, hx.w, hy.w, hz.w);
    }
    if (!b.any) return;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        nd[4 * a + k] = b.mn[a];
        nd[4 * (3 + a) + k] = b.mx[a];
    }
}

inline unsigned blocks_for(size_t n) { return (unsigned)((n + kRefitBlock - 1) / kRefitBlock); }

}  // namespace

hipError_t launch_refit_count_nonfinite(const float *a, const float *b, size_t n, uint32_t *count, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_refit_count_nonfinite, dim3(blocks_for(n)), dim3(kRefitBlock), 0, st, a, b, n, count);
    return hipGetLastError();
}

hipError_t launch_refit_set_vertices(float4 *pos, float4 *nrm, const float *p, const float *n, uint32_t V,
                                     hipStream_t st) {
    if (V == 0) return hipSuccess;
    hipLaunchKernelGGL(k_refit_set_vertices, dim3(blocks_for(V)), dim3(kRefitBlock), 0, st, pos, nrm, p, n, V);
    return hipGetLastError();
}

hipError_t launch_refit_records(float4 *prims, const uint32_t *vidx, const float4 *pos, uint32_t P, hipStream_t st) {
    if (P == 0) return hipSuccess;
    hipLaunchKernelGGL(k_refit_records, dim3(blocks_for(P)), dim3(kRefitBlock), 0, st, prims, vidx, pos, P);
    return hipGetLastError();
}

hipError_t launch_refit_level(float4 *nodes, const float4 *prims, const uint32_t *vidx, const float4 *pos,
                              const uint32_t *slots, uint32_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_refit_level, dim3(blocks_for(n)), dim3(kRefitBlock), 0, st, reinterpret_cast<float *>(nodes),
                       prims, vidx, pos, slots, n);
    return hipGetLastError();
}

}  // namespace nori
