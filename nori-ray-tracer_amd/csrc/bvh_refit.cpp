// bvh_refit.cpp -- the BVH refit on the host: the schedule the device kernels
// follow (nori_gpu_update_vertices, refit.hip) and the refit's one statement
// (nori_scene_bvh_refit in include/nori_gpu.h), which they are tested against
// byte for byte.
#include <cstring>

#include "host_scene.h"
#include "refit.h"

namespace nori {

// The 4-wide tree is in DFS preorder (bvh_builder.cpp collapse): a child's
// index is larger than its parent's, so one backward sweep gives every node's
// height (the longest way down to a node without inner children).
RefitPlan build_refit_plan(const DeviceBvh &bvh) {
    const uint32_t N = bvh.num_nodes;
    std::vector<uint32_t> height(N, 0);
    uint32_t top = 0;
    size_t leaf_slots = 0;
    for (uint32_t n = N; n-- > 0;) {
        const float *nd = &bvh.nodes[32 * (size_t)n];
        for (int k = 0; k < 4; ++k) {
            if (refit_unused(nd[k])) continue;  // unused slot: its box is NaN (its ref is not a mark)
            const uint32_t ref = refit_bits(nd[24 + k]);
            if (ref & kRefitLeafBit) {
                ++leaf_slots;
                continue;
            }
            if (ref <= n || ref >= N) throw NoriException(NORI_ERR_INVALID, "BVH nodes are not in preorder");
            if (height[ref] + 1 > height[n]) height[n] = height[ref] + 1;
        }
        if (height[n] > top) top = height[n];
    }
    RefitPlan plan;
    // level 0: every leaf slot; level h >= 1: the inner slots of the nodes of height h
    std::vector<uint32_t> count(top + 2, 0);
    count[0] = (uint32_t)leaf_slots;
    for (uint32_t n = 0; n < N; ++n) {
        const float *nd = &bvh.nodes[32 * (size_t)n];
        for (int k = 0; k < 4; ++k)
            if (!refit_unused(nd[k]) && !(refit_bits(nd[24 + k]) & kRefitLeafBit)) ++count[height[n]];
    }
    plan.level_begin.assign(top + 2, 0);
    for (uint32_t h = 0; h <= top; ++h) plan.level_begin[h + 1] = plan.level_begin[h] + count[h];
    plan.slots.resize(plan.level_begin[top + 1]);
    std::vector<uint32_t> at(plan.level_begin.begin(), plan.level_begin.end() - 1);
    for (uint32_t n = 0; n < N; ++n) {
        const float *nd = &bvh.nodes[32 * (size_t)n];
        for (int k = 0; k < 4; ++k) {
            if (refit_unused(nd[k])) continue;
            const bool leaf = refit_bits(nd[24 + k]) & kRefitLeafBit;
            plan.slots[at[leaf ? 0 : height[n]]++] = 4 * n + (uint32_t)k;
        }
    }
    return plan;
}

std::vector<uint32_t> prim_vertex_ids(const nori_scene_desc &d) {
    std::vector<uint32_t> v;
    for (uint32_t s = 0; s < d.num_shapes; ++s) {
        const nori_shape_desc &sh = d.shapes[s];
        if (sh.type == NORI_SHAPE_SPHERE) {
            v.insert(v.end(), {0u, 0u, 0u});
            continue;
        }
        for (uint32_t t = 0; t < sh.tri_count; ++t) {
            const uint32_t *f = d.indices + 3 * (size_t)(sh.tri_offset + t);
            for (int k = 0; k < 3; ++k)
                if (f[k] >= d.num_vertices) throw NoriException(NORI_ERR_INVALID, "vertex index out of range");
            v.insert(v.end(), {f[0], f[1], f[2]});
        }
    }
    return v;
}

void refit_host(DeviceBvh &bvh, const RefitPlan &plan, const std::vector<uint32_t> &vidx, const float *positions,
                float root_box[6]) {
    const size_t P = bvh.prims.size() / 12;
    auto sphere = [&](const float *r) { return refit_bits(r[7]) == 1u; };
    // ---- triangle records: (p0 | id), (p1 - p0 | w kept), (p2 - p0 | w kept)
    for (size_t i = 0; i < P; ++i) {
        float *r = &bvh.prims[12 * i];
        if (sphere(r)) continue;
        const uint32_t *f = &vidx[3 * (size_t)refit_bits(r[3])];
        const float *p0 = positions + 3 * (size_t)f[0], *p1 = positions + 3 * (size_t)f[1],
                    *p2 = positions + 3 * (size_t)f[2];
        for (int k = 0; k < 3; ++k) {
            r[k] = p0[k];
            r[4 + k] = p1[k] - p0[k];
            r[8 + k] = p2[k] - p0[k];
        }
    }
    // ---- boxes, level by level
    for (uint32_t s : plan.slots) {
        float *nd = &bvh.nodes[32 * (size_t)(s >> 2)];
        const int k = (int)(s & 3u);
        const uint32_t ref = refit_bits(nd[24 + k]);
        float mn[3], mx[3];
        bool first = true;
        auto add = [&](const float lo[3], const float hi[3]) {
            for (int a = 0; a < 3; ++a) {
                mn[a] = first ? lo[a] : box_min(mn[a], lo[a]);
                mx[a] = first ? hi[a] : box_max(mx[a], hi[a]);
            }
            first = false;
        };
        if (ref & kRefitLeafBit) {
            const uint32_t b = refit_leaf_first(ref), e = b + refit_leaf_count(ref);
            for (uint32_t i = b; i < e; ++i) {
                const float *r = &bvh.prims[12 * (size_t)i];
                if (sphere(r)) {  // centre -/+ radius (sphere.cpp:32-41)
                    const float lo[3] = {r[0] - r[4], r[1] - r[4], r[2] - r[4]};
                    const float hi[3] = {r[0] + r[4], r[1] + r[4], r[2] + r[4]};
                    add(lo, hi);
                } else {  // the vertex positions themselves, not v0 + e1
                    const uint32_t *f = &vidx[3 * (size_t)refit_bits(r[3])];
                    for (int j = 0; j < 3; ++j) add(positions + 3 * (size_t)f[j], positions + 3 * (size_t)f[j]);
                }
            }
        } else {
            const float *ch = &bvh.nodes[32 * (size_t)ref];
            for (int j = 0; j < 4; ++j) {
                if (refit_unused(ch[j])) continue;
                const float lo[3] = {ch[j], ch[4 + j], ch[8 + j]}, hi[3] = {ch[12 + j], ch[16 + j], ch[20 + j]};
                add(lo, hi);
            }
        }
        if (first) continue;  // (a child node always has a used slot)
        for (int a = 0; a < 3; ++a) {
            nd[4 * a + k] = mn[a];
            nd[4 * (3 + a) + k] = mx[a];
        }
    }
    if (root_box) refit_root_box(&bvh.nodes[0], root_box);
}

void refit_root_box(const float *root, float box[6]) {
    bool first = true;
    for (int j = 0; j < 4; ++j) {
        if (refit_unused(root[j])) continue;
        for (int a = 0; a < 3; ++a) {
            box[a] = first ? root[4 * a + j] : box_min(box[a], root[4 * a + j]);
            box[3 + a] = first ? root[4 * (3 + a) + j] : box_max(box[3 + a], root[4 * (3 + a) + j]);
        }
        first = false;
    }
}

}  // namespace nori
