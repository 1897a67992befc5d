// bvh_rebuild.cpp -- the linear-BVH rebuild on the host: the one statement
// (nori_scene_bvh_rebuild in include/nori_gpu.h) that the kernels of
// nori_gpu_rebuild_bvh (rebuild.hip) are tested against byte for byte.
//
// Morton keys of the primitive boxes' centres, a sort of the unique 64-bit
// keys, Karras's radix tree over the sorted keys emitted 4-wide and numbered
// breadth-first, and the refit's own box routine (refit_host) on that
// topology.  The arithmetic is in rebuild.h, shared with the kernels.
#include <algorithm>
#include <cstring>

#include "host_scene.h"
#include "rebuild.h"

namespace nori {

void rebuild_host(const nori_scene_desc &d, const float *positions, uint32_t leaf_max, DeviceBvh &out) {
    if (leaf_max == 0) leaf_max = kRebuildLeafDefault;
    if (leaf_max > kRebuildLeafMax) throw NoriException(NORI_ERR_INVALID, "nori_scene_bvh_rebuild: leaf_max above 64");
    if (!positions) positions = d.positions;
    const std::vector<uint32_t> vidx = prim_vertex_ids(d);  // (checks the indices)
    const uint32_t n = (uint32_t)(vidx.size() / 3);
    out = DeviceBvh();
    if (n == 0) throw NoriException(NORI_ERR_INVALID, "scene has no primitives");
    if (n >= kRebuildMaxPrims) throw NoriException(NORI_ERR_UNSUPPORTED, "more than 2^25 primitives");
    // ---- primitive boxes by global id (shape order), the scene box
    std::vector<const nori_shape_desc *> sphere(n, nullptr);
    {
        uint32_t p = 0;
        for (uint32_t s = 0; s < d.num_shapes; ++s) {
            const nori_shape_desc &sh = d.shapes[s];
            if (sh.type == NORI_SHAPE_SPHERE) sphere[p++] = &sh;
            else p += sh.tri_count;
        }
    }
    std::vector<float> lo(3 * (size_t)n), hi(3 * (size_t)n);
    float Lo[3], Hi[3];
    for (uint32_t p = 0; p < n; ++p) {
        float *l = &lo[3 * (size_t)p], *h = &hi[3 * (size_t)p];
        if (sphere[p]) {
            for (int k = 0; k < 3; ++k) l[k] = sphere[p]->center[k] - sphere[p]->radius, h[k] = sphere[p]->center[k] + sphere[p]->radius;
        } else {
            const uint32_t *f = &vidx[3 * (size_t)p];
            const float *p0 = positions + 3 * (size_t)f[0], *p1 = positions + 3 * (size_t)f[1], *p2 = positions + 3 * (size_t)f[2];
            for (int k = 0; k < 3; ++k) {
                l[k] = box_min(box_min(p0[k], p1[k]), p2[k]);
                h[k] = box_max(box_max(p0[k], p1[k]), p2[k]);
            }
        }
        for (int k = 0; k < 3; ++k) {
            Lo[k] = p ? box_min(Lo[k], l[k]) : l[k];
            Hi[k] = p ? box_max(Hi[k], h[k]) : h[k];
        }
    }
    // ---- keys: code << 32 | id, sorted (unique, so any sort gives this order)
    float scale[3];
    for (int k = 0; k < 3; ++k) scale[k] = rebuild_scale(Lo[k], Hi[k]);
    std::vector<uint64_t> keys(n);
    for (uint32_t p = 0; p < n; ++p) {
        uint32_t q[3];
        for (int k = 0; k < 3; ++k) q[k] = rebuild_cell(lo[3 * (size_t)p + k], hi[3 * (size_t)p + k], Lo[k], scale[k]);
        keys[p] = ((uint64_t)rebuild_morton(q[0], q[1], q[2]) << 32) | p;
    }
    std::sort(keys.begin(), keys.end());
    // ---- records in leaf order, as build_device_bvh writes them
    out.prims.assign(12 * (size_t)n, 0.0f);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t id = (uint32_t)keys[i];
        float *r = &out.prims[12 * (size_t)i];
        if (sphere[id]) {
            const uint32_t one = 1;
            for (int k = 0; k < 3; ++k) r[k] = sphere[id]->center[k];
            r[4] = sphere[id]->radius;
            std::memcpy(&r[7], &one, 4);
        } else {
            const uint32_t *f = &vidx[3 * (size_t)id];
            const float *p0 = positions + 3 * (size_t)f[0], *p1 = positions + 3 * (size_t)f[1], *p2 = positions + 3 * (size_t)f[2];
            for (int k = 0; k < 3; ++k) {
                r[k] = p0[k];
                r[4 + k] = p1[k] - p0[k];
                r[8 + k] = p2[k] - p0[k];
            }
        }
        std::memcpy(&r[3], &id, 4);
    }
    // ---- topology, breadth-first: the nodes of a level in (parent, slot) order
    struct Range {
        uint32_t a, b;
    };
    const float nan = __builtin_nanf("");
    auto new_node = [&](std::vector<float> &nodes) {
        nodes.resize(nodes.size() + 32, 0.0f);
        float *nd = &nodes[nodes.size() - 32];
        const uint32_t unused = kRefitLeafBit;
        for (int k = 0; k < 4; ++k) {
            for (int a = 0; a < 6; ++a) nd[4 * a + k] = nan;
            std::memcpy(&nd[24 + k], &unused, 4);
        }
        return nd;
    };
    auto set_slot = [&](float *nd, int k, uint32_t ref) {
        for (int a = 0; a < 6; ++a) nd[4 * a + k] = 0.0f;  // used: the refit below writes its box
        std::memcpy(&nd[24 + k], &ref, 4);
    };
    auto leaf_ref = [](uint32_t first, uint32_t count) { return kRefitLeafBit | ((count - 1) << 25) | first; };
    std::vector<Range> level, next;
    if (n <= leaf_max) {
        set_slot(new_node(out.nodes), 0, leaf_ref(0, n));
        out.depth = 1;
    } else {
        level.push_back({0, n - 1});
    }
    uint32_t level_off = 0;
    while (!level.empty()) {
        ++out.depth;
        const uint32_t next_off = level_off + (uint32_t)level.size();
        next.clear();
        for (const Range &r : level) {
            float *nd = new_node(out.nodes);
            uint32_t end[4];
            const int used = rebuild_node_slots(keys.data(), r.a, r.b, leaf_max, end);
            uint32_t first = r.a;
            for (int k = 0; k < used; ++k) {
                const uint32_t count = end[k] - first + 1;
                if (count > leaf_max) {
                    set_slot(nd, k, next_off + (uint32_t)next.size());
                    next.push_back({first, end[k]});
                } else {
                    set_slot(nd, k, leaf_ref(first, count));
                }
                first = end[k] + 1;
            }
        }
        level_off = next_off;
        level.swap(next);
    }
    out.num_nodes = (uint32_t)(out.nodes.size() / 32);
    // ---- boxes: the refit's statement on this topology
    refit_host(out, build_refit_plan(out), vidx, positions, nullptr);
}

}  // namespace nori
