// rebuild.hip -- the BVH rebuilt on the device (nori_gpu_rebuild_bvh).
//
// A linear BVH for the vertex positions the context holds now: the scene box,
// Morton keys of the primitive boxes' centres, a radix sort of the unique
// 64-bit keys (rocprim), the records in the new leaf order, Karras's radix
// tree over the sorted keys emitted 4-wide one breadth-first level at a time,
// and the refit's own kernel (launch_refit_level) for the boxes.  The tree is
// stated once, at nori_scene_bvh_rebuild in include/nori_gpu.h
// (bvh_rebuild.cpp computes it on the host); the kernels give the same bytes:
// the arithmetic is rebuild.h's on both sides, integer work or single fp32
// operations with contraction off.
//
// As in refit.hip every kernel is one thread per item with plain vector loads
// and stores and no waiting between work-groups: the order between the levels
// is the order of the LAUNCHES.  The only atomics are the integer min / max of
// the scene box (on an order-preserving key of a float; no float atomics).
// Two threads never write the same word: a node's thread writes that node's
// refs and split record, the words of the next level's ranges and of the two
// slot lists that the scan assigned to it.  Every loop has a stated bound: the
// split search runs at most kRebuildSearchSteps steps, a node has 4 slots.
// Sizes and grids come from n and from level counts that the host has checked
// against n before it passes them in.
#include <hip/hip_runtime.h>

#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "kernels.h"
#include "rebuild.h"

namespace nori {

namespace {

constexpr int kRebuildBlock = 256;
constexpr uint32_t kRebuildUnusedRef = 0xffffffffu;  // in the compact refs only: no leaf of < 2^25 records has it

// Box of primitive `id` (global id, shape order): box_min / box_max over a
// triangle's three vertex positions, centre -/+ radius of a sphere.
__device__ inline void prim_box(uint32_t id, const uint32_t *__restrict__ vidx, const float4 *__restrict__ pos,
                                const uint32_t *__restrict__ prim_shape, const DevShape *__restrict__ shapes,
                                float lo[3], float hi[3]) {
    const DevShape &sh = shapes[prim_shape[id]];
    if (sh.type == NORI_SHAPE_SPHERE) {
        const float r = sh.radius;
#pragma unroll
        for (int k = 0; k < 3; ++k) lo[k] = sh.center[k] - r, hi[k] = sh.center[k] + r;
        return;
    }
    const uint32_t *f = vidx + 3 * (size_t)id;
    const float4 p0 = pos[f[0]], p1 = pos[f[1]], p2 = pos[f[2]];
    lo[0] = box_min(box_min(p0.x, p1.x), p2.x), hi[0] = box_max(box_max(p0.x, p1.x), p2.x);
    lo[1] = box_min(box_min(p0.y, p1.y), p2.y), hi[1] = box_max(box_max(p0.y, p1.y), p2.y);
    lo[2] = box_min(box_min(p0.z, p1.z), p2.z), hi[2] = box_max(box_max(p0.z, p1.z), p2.z);
}

// box[0..2] = min, box[3..5] = max over all primitive boxes, as order keys
// (rebuild_order_key); the caller set box to (~0, ~0, ~0, 0, 0, 0).  A wave
// reduces its 64 boxes with shuffles, its first lane issues the six atomics.
__global__ __launch_bounds__(kRebuildBlock) void k_rebuild_scene_box(const uint32_t *__restrict__ vidx,
                                                                     const float4 *__restrict__ pos,
                                                                     const uint32_t *__restrict__ prim_shape,
                                                                     const DevShape *__restrict__ shapes, uint32_t n,
                                                                     uint32_t *__restrict__ box) {
    const uint32_t id = blockIdx.x * kRebuildBlock + threadIdx.x;
    uint32_t mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
    if (id < n) {
        float lo[3], hi[3];
        prim_box(id, vidx, pos, prim_shape, shapes, lo, hi);
#pragma unroll
        for (int k = 0; k < 3; ++k) mn[k] = rebuild_order_key(lo[k]), mx[k] = rebuild_order_key(hi[k]);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            mn[k] = min(mn[k], (uint32_t)__shfl_xor((int)mn[k], d, 64));
            mx[k] = max(mx[k], (uint32_t)__shfl_xor((int)mx[k], d, 64));
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            atomicMin(box + k, mn[k]);
            atomicMax(box + 3 + k, mx[k]);
        }
    }
}

struct RebuildGrid {
    float lo[3], scale[3];
};

// keys[id] = Morton code << 32 | id
__global__ __launch_bounds__(kRebuildBlock) void k_rebuild_keys(const uint32_t *__restrict__ vidx,
                                                                const float4 *__restrict__ pos,
                                                                const uint32_t *__restrict__ prim_shape,
                                                                const DevShape *__restrict__ shapes, uint32_t n,
                                                                RebuildGrid g, uint64_t *__restrict__ keys) {
    const uint32_t id = blockIdx.x * kRebuildBlock + threadIdx.x;
    if (id >= n) return;
    float lo[3], hi[3];
    prim_box(id, vidx, pos, prim_shape, shapes, lo, hi);
    const uint32_t qx = rebuild_cell(lo[0], hi[0], g.lo[0], g.scale[0]);
    const uint32_t qy = rebuild_cell(lo[1], hi[1], g.lo[1], g.scale[1]);
    const uint32_t qz = rebuild_cell(lo[2], hi[2], g.lo[2], g.scale[2]);
    keys[id] = ((uint64_t)rebuild_morton(qx, qy, qz) << 32) | id;
}

// Record i of the new leaf order: the primitive the i-th sorted key names.
__global__ __launch_bounds__(kRebuildBlock) void k_rebuild_records(const uint64_t *__restrict__ sorted,
                                                                   const uint32_t *__restrict__ vidx,
                                                                   const float4 *__restrict__ pos,
                                                                   const uint32_t *__restrict__ prim_shape,
                                                                   const DevShape *__restrict__ shapes, uint32_t n,
                                                                   float4 *__restrict__ prims) {
    const uint32_t i = blockIdx.x * kRebuildBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t id = (uint32_t)sorted[i];
    if (id >= n) return;  // (keys carry ids < n: a guard, not a case)
    float4 r0, r1, r2;
    const DevShape &sh = shapes[prim_shape[id]];
    if (sh.type == NORI_SHAPE_SPHERE) {
        r0 = make_float4(sh.center[0], sh.center[1], sh.center[2], 0.0f);
        r1 = make_float4(sh.radius, 0.0f, 0.0f, __uint_as_float(1u));
        r2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    } else {
        const uint32_t *f = vidx + 3 * (size_t)id;
        const float4 p0 = pos[f[0]], p1 = pos[f[1]], p2 = pos[f[2]];
        r0 = make_float4(p0.x, p0.y, p0.z, 0.0f);
        r1 = make_float4(p1.x - p0.x, p1.y - p0.y, p1.z - p0.z, 0.0f);
        r2 = make_float4(p2.x - p0.x, p2.y - p0.y, p2.z - p0.z, 0.0f);
    }
    r0.w = __uint_as_float(id);
    float4 *r = prims + 3 * (size_t)i;
    r[0] = r0, r[1] = r1, r[2] = r2;
}

// One thread per node of a level: its used slots (rebuild_node_slots) as the
// last record of each (unused: ~0) and the count of its inner and leaf slots,
// inner | leaf << 32.  count[m] = 0 closes the array for the exclusive scan,
// whose entry m is then the level's totals.
__global__ __launch_bounds__(kRebuildBlock) void k_rebuild_split(const uint64_t *__restrict__ sorted,
                                                                 const uint2 *__restrict__ ranges, uint32_t m,
                                                                 uint32_t leaf_max, uint4 *__restrict__ ends,
                                                                 uint64_t *__restrict__ count) {
    const uint32_t j = blockIdx.x * kRebuildBlock + threadIdx.x;
    if (j > m) return;
    if (j == m) {
        count[m] = 0ull;
        return;
    }
    const uint2 r = ranges[j];
    uint32_t end[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
    const int used = rebuild_node_slots(sorted, r.x, r.y, leaf_max, end);
    uint32_t inner = 0, leaf = 0, first = r.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < used) {
            if (end[k] - first + 1 > leaf_max) ++inner;
            else ++leaf;
            first = end[k] + 1;
        }
    }
    ends[j] = make_uint4(end[0], end[1], end[2], end[3]);
    count[j] = (uint64_t)inner | ((uint64_t)leaf << 32);
}

// One thread per node of a level, after the scan: the node's refs, the next
// level's ranges and the two slot lists.  Node level_off + j; its inner slots
// become the nodes next_off + (scan[j] & mask) ..., in slot order, and the
// inner slot of child node c is entry c - 1 of inner_slots (children are
// numbered by (parent, slot)); its leaf slots go to leaf_slots from
// leaf_base + (scan[j] >> 32).
__global__ __launch_bounds__(kRebuildBlock) void k_rebuild_emit(const uint2 *__restrict__ ranges,
                                                                const uint4 *__restrict__ ends,
                                                                const uint64_t *__restrict__ scan, uint32_t m,
                                                                uint32_t level_off, uint32_t leaf_base,
                                                                uint32_t leaf_max, uint4 *__restrict__ refs,
                                                                uint2 *__restrict__ next,
                                                                uint32_t *__restrict__ inner_slots,
                                                                uint32_t *__restrict__ leaf_slots) {
    const uint32_t j = blockIdx.x * kRebuildBlock + threadIdx.x;
    if (j >= m) return;
    const uint32_t node = level_off + j, next_off = level_off + m;
    const uint4 e4 = ends[j];
    const uint32_t end[4] = {e4.x, e4.y, e4.z, e4.w};
    const uint64_t s = scan[j];
    uint32_t in = (uint32_t)s, lf = leaf_base + (uint32_t)(s >> 32), first = ranges[j].x;
    uint32_t ref[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        ref[k] = kRebuildUnusedRef;
        if (end[k] == 0xffffffffu) continue;
        const uint32_t cnt = end[k] - first + 1;
        if (cnt > leaf_max) {
            const uint32_t child = next_off + in;
            ref[k] = child;
            next[in] = make_uint2(first, end[k]);
            inner_slots[child - 1] = 4u * node + (uint32_t)k;
            ++in;
        } else {
            ref[k] = kRefitLeafBit | ((cnt - 1u) << 25) | first;
            leaf_slots[lf++] = 4u * node + (uint32_t)k;
        }
        first = end[k] + 1;
    }
    refs[node] = make_uint4(ref[0], ref[1], ref[2], ref[3]);
}

// The N nodes from their compact refs: a used slot gets a zero box (the refit
// launches that follow write every used slot), an unused one NaN and the ref
// `leaf bit`; the last row is zero.
__global__ __launch_bounds__(kRebuildBlock) void k_rebuild_nodes(const uint4 *__restrict__ refs, uint32_t N,
                                                                 float4 *__restrict__ nodes) {
    const uint32_t i = blockIdx.x * kRebuildBlock + threadIdx.x;
    if (i >= N) return;
    uint4 r = refs[i];
    const float nan = __uint_as_float(0x7fc00000u);
    const float4 b = make_float4(r.x == kRebuildUnusedRef ? nan : 0.0f, r.y == kRebuildUnusedRef ? nan : 0.0f,
                                 r.z == kRebuildUnusedRef ? nan : 0.0f, r.w == kRebuildUnusedRef ? nan : 0.0f);
    if (r.x == kRebuildUnusedRef) r.x = kRefitLeafBit;
    if (r.y == kRebuildUnusedRef) r.y = kRefitLeafBit;
    if (r.z == kRebuildUnusedRef) r.z = kRefitLeafBit;
    if (r.w == kRebuildUnusedRef) r.w = kRefitLeafBit;
    float4 *nd = nodes + 8 * (size_t)i;
#pragma unroll
    for (int a = 0; a < 6; ++a) nd[a] = b;
    nd[6] = make_float4(__uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z), __uint_as_float(r.w));
    nd[7] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

inline unsigned blocks_for(size_t n) { return (unsigned)((n + kRebuildBlock - 1) / kRebuildBlock); }

// One block up to 1,024 keys, Onesweep above: the merge-sort path that
// rocprim's default would take between the two is configured away, so the
// sort has two paths and the tests take both.
using RebuildSortConfig = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                                                     rocprim::default_config, 1024>;
constexpr unsigned kRebuildKeyBits = 62;  // 32 id bits + 30 code bits

}  // namespace

hipError_t launch_rebuild_scene_box(const DevScene &S, uint32_t n, uint32_t *box, hipStream_t st) {
    hipError_t e = hipMemsetAsync(box, 0xff, 12, st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(box + 3, 0, 12, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rebuild_scene_box, dim3(blocks_for(n)), dim3(kRebuildBlock), 0, st, S.tri_vidx, S.pos,
                       S.prim_shape, S.shapes, n, box);
    return hipGetLastError();
}

hipError_t launch_rebuild_keys(const DevScene &S, uint32_t n, const float lo[3], const float scale[3], uint64_t *keys,
                               hipStream_t st) {
    RebuildGrid g;
    for (int k = 0; k < 3; ++k) g.lo[k] = lo[k], g.scale[k] = scale[k];
    hipLaunchKernelGGL(k_rebuild_keys, dim3(blocks_for(n)), dim3(kRebuildBlock), 0, st, S.tri_vidx, S.pos, S.prim_shape,
                       S.shapes, n, g, keys);
    return hipGetLastError();
}

hipError_t rebuild_sort_keys(void *temp, size_t &temp_bytes, const uint64_t *in, uint64_t *out, uint32_t n,
                             hipStream_t st) {
    return rocprim::radix_sort_keys<RebuildSortConfig>(temp, temp_bytes, in, out, n, 0u, kRebuildKeyBits, st);
}

hipError_t rebuild_scan_counts(void *temp, size_t &temp_bytes, const uint64_t *in, uint64_t *out, uint32_t n,
                               hipStream_t st) {
    return rocprim::exclusive_scan(temp, temp_bytes, in, out, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>(), st);
}

hipError_t launch_rebuild_records(const DevScene &S, const uint64_t *sorted, uint32_t n, float4 *prims, hipStream_t st) {
    hipLaunchKernelGGL(k_rebuild_records, dim3(blocks_for(n)), dim3(kRebuildBlock), 0, st, sorted, S.tri_vidx, S.pos,
                       S.prim_shape, S.shapes, n, prims);
    return hipGetLastError();
}

hipError_t launch_rebuild_split(const uint64_t *sorted, const uint2 *ranges, uint32_t m, uint32_t leaf_max, uint4 *ends,
                                uint64_t *count, hipStream_t st) {
    hipLaunchKernelGGL(k_rebuild_split, dim3(blocks_for((size_t)m + 1)), dim3(kRebuildBlock), 0, st, sorted, ranges, m,
                       leaf_max, ends, count);
    return hipGetLastError();
}

hipError_t launch_rebuild_emit(const uint2 *ranges, const uint4 *ends, const uint64_t *scan, uint32_t m,
                               uint32_t level_off, uint32_t leaf_base, uint32_t leaf_max, uint4 *refs, uint2 *next,
                               uint32_t *inner_slots, uint32_t *leaf_slots, hipStream_t st) {
    hipLaunchKernelGGL(k_rebuild_emit, dim3(blocks_for(m)), dim3(kRebuildBlock), 0, st, ranges, ends, scan, m, level_off,
                       leaf_base, leaf_max, refs, next, inner_slots, leaf_slots);
    return hipGetLastError();
}

hipError_t launch_rebuild_nodes(const uint4 *refs, uint32_t N, float4 *nodes, hipStream_t st) {
    hipLaunchKernelGGL(k_rebuild_nodes, dim3(blocks_for(N)), dim3(kRebuildBlock), 0, st, refs, N, nodes);
    return hipGetLastError();
}

}  // namespace nori
