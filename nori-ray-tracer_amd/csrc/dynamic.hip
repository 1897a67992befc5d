// dynamic.hip -- geometry that changes under a context: vertex updates with
// a BVH refit (refit.hip), the device rebuild (rebuild.hip), and the read-back.
#include <algorithm>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "ctx.h"
#include "rebuild.h"

namespace nori {
namespace {

// nori_gpu_update_vertices (stated in nori_gpu.h): validate, then on the
// context's stream count the non-finite inputs (nothing is modified before
// that count is back), set the vertices, rebuild the records, refit the boxes
// one launch per level of c.refit, and bring the lights and the scene box up
// to date.
int update_vertices(nori_gpu_ctx &c, const nori_gpu_update_desc &ud, nori_gpu_update_stats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    if (c.stack == 0)
        throw NoriException(NORI_ERR_UNSUPPORTED,
                            "nori_gpu_update_vertices: a scan-mode context (its scan list and specialised kernels "
                            "are functions of the geometry); create the context with NORI_TRAVERSAL=bvh");
    if (c.S.integrator == NORI_INTEGRATOR_PHOTONMAPPER)
        throw NoriException(NORI_ERR_UNSUPPORTED,
                            "nori_gpu_update_vertices: a photonmapper context (its photon map was traced at creation)");
    if (ud.num_vertices != c.num_vertices)
        throw NoriException(NORI_ERR_INVALID, "nori_gpu_update_vertices: num_vertices " + std::to_string(ud.num_vertices) +
                                                  " is not the scene's " + std::to_string(c.num_vertices));
    for (uint32_t r : ud.reserved)
        if (r != 0) throw NoriException(NORI_ERR_INVALID, "nori_gpu_update_vertices: reserved must be 0");
    if (ud.on_device && ((uintptr_t)ud.positions % 4 || (uintptr_t)ud.normals % 4))
        throw NoriException(NORI_ERR_INVALID, "nori_gpu_update_vertices: device pointers must be 4-byte aligned");
    HIP_TRY(hipSetDevice(c.device));
    if (ud.on_device)  // a host pointer here would fault in the first kernel: ask the runtime what it is
        for (const float *p : {ud.positions, ud.normals})
            if (p) require_device_ptr(p, "nori_gpu_update_vertices: on_device with a pointer that is not device memory");
    for (auto &e : c.upd_ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    const uint32_t V = c.num_vertices;
    const size_t nfl = 3 * (size_t)V;
    const float *dp = ud.positions, *dn = ud.normals;
    if (!ud.on_device) {
        c.upd_pos.ensure(nfl * 4);
        HIP_TRY(hipMemcpyAsync(c.upd_pos.p, ud.positions, nfl * 4, hipMemcpyHostToDevice, c.stream));
        dp = c.upd_pos.as<float>();
        if (ud.normals) {
            c.upd_nrm.ensure(nfl * 4);
            HIP_TRY(hipMemcpyAsync(c.upd_nrm.p, ud.normals, nfl * 4, hipMemcpyHostToDevice, c.stream));
            dn = c.upd_nrm.as<float>();
        }
    }
    uint32_t launches = 0;
    // ---- a pass of its own: nothing is modified before its count is back
    c.upd_count.ensure(4);
    HIP_TRY(hipMemsetAsync(c.upd_count.p, 0, 4, c.stream));
    HIP_TRY(launch_refit_count_nonfinite(dp, dn, nfl, c.upd_count.as<uint32_t>(), c.stream));
    ++launches;
    uint32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, c.upd_count.p, 4, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    if (bad)
        throw NoriException(NORI_ERR_INVALID, "nori_gpu_update_vertices: " + std::to_string(bad) +
                                                  " non-finite position or normal values; nothing was changed");
    // ---- vertices, records, boxes
    float4 *pos = c.pos.as<float4>();
    HIP_TRY(hipEventRecord(c.upd_ev[0], c.stream));
    HIP_TRY(launch_refit_set_vertices(pos, c.nrm.as<float4>(), dp, dn, V, c.stream));
    HIP_TRY(launch_refit_records(c.prims.as<float4>(), c.S.tri_vidx, pos, c.S.num_prims, c.stream));
    launches += 2;
    for (uint32_t l = 0; l < c.refit.levels(); ++l) {
        const uint32_t b = c.refit.level_begin[l], n = c.refit.level_begin[l + 1] - b;
        HIP_TRY(launch_refit_level(c.nodes.as<float4>(), c.S.prims, c.S.tri_vidx, pos, c.refit_slots.as<uint32_t>() + b, n,
                                   c.stream));
        launches += n ? 1u : 0u;
    }
    HIP_TRY(hipEventRecord(c.upd_ev[1], c.stream));
    // ---- the scene box: the root node's used slots (128 bytes back)
    float root[32], box[6];
    HIP_TRY(hipMemcpyAsync(root, c.nodes.p, sizeof(root), hipMemcpyDeviceToHost, c.stream));
    // ---- the lights: area CDF and normalisation of every mesh with an emitter, in nori_gpu_create's
    // own order on the host (mesh_area_cdf) from a read-back of that mesh's vertices; emitter meshes are small
    std::vector<std::vector<float>> verts(c.emitter_meshes.size());
    for (size_t m = 0; m < c.emitter_meshes.size(); ++m) {
        const auto &em = c.emitter_meshes[m];
        verts[m].resize(4 * (size_t)em.vtx_count);
        HIP_TRY(hipMemcpyAsync(verts[m].data(), pos + em.vtx_first, 16 * (size_t)em.vtx_count, hipMemcpyDeviceToHost,
                               c.stream));
    }
    HIP_TRY(hipStreamSynchronize(c.stream));
    refit_root_box(root, box);
    for (size_t m = 0; m < c.emitter_meshes.size(); ++m) {
        const auto &em = c.emitter_meshes[m];
        std::vector<float> cdf;
        const float *v = verts[m].data();
        c.hshapes[em.shape].area_norm = mesh_area_cdf(em.tri.data(), (uint32_t)(em.tri.size() / 3),
                                                      [&](uint32_t i) { return v + 4 * (size_t)(i - em.vtx_first); }, cdf);
        HIP_TRY(hipMemcpyAsync(c.cdf.as<float>() + em.cdf_offset, cdf.data(), cdf.size() * 4, hipMemcpyHostToDevice,
                               c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));  // (cdf is a local)
    }
    // the solitary shortcut's precondition was checked against the geometry as loaded: off for good
    for (DevShape &sh : c.hshapes)
        if (sh.type == NORI_SHAPE_SPHERE) sh.solitary = 0;
    HIP_TRY(hipMemcpyAsync(c.shapes.p, c.hshapes.data(), c.hshapes.size() * sizeof(DevShape), hipMemcpyHostToDevice,
                           c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    for (int k = 0; k < 3; ++k) c.S.root_min[k] = box[k], c.S.root_max[k] = box[3 + k];
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        HIP_TRY(hipEventElapsedTime(&stats->ms_device, c.upd_ev[0], c.upd_ev[1]));
        for (int k = 0; k < 3; ++k) stats->root_min[k] = box[k], stats->root_max[k] = box[3 + k];
        stats->nodes = c.bvh_nodes;
        stats->levels = c.refit.levels();
        stats->launches = launches;
        stats->ms = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return NORI_OK;
}

// nori_gpu_rebuild_bvh (stated in nori_gpu.h): a linear BVH for the positions
// the context holds, built in the rb_* scratch buffers on the context's
// stream and swapped in at the end; until then nothing the context renders
// with is written, so every refusal and every failure leaves it as it was.
int rebuild_bvh(nori_gpu_ctx &c, const nori_gpu_rebuild_desc &rd, nori_gpu_rebuild_stats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    if (c.stack == 0)
        throw NoriException(NORI_ERR_UNSUPPORTED,
                            "nori_gpu_rebuild_bvh: a scan-mode context; create the context with NORI_TRAVERSAL=bvh");
    if (c.S.integrator == NORI_INTEGRATOR_PHOTONMAPPER)
        throw NoriException(NORI_ERR_UNSUPPORTED,
                            "nori_gpu_rebuild_bvh: a photonmapper context (its photon map was traced at creation)");
    if (rd.leaf_max > kRebuildLeafMax) throw NoriException(NORI_ERR_INVALID, "nori_gpu_rebuild_bvh: leaf_max above 64");
    for (uint32_t r : rd.reserved)
        if (r != 0) throw NoriException(NORI_ERR_INVALID, "nori_gpu_rebuild_bvh: reserved must be 0");
    const uint32_t L = rd.leaf_max ? rd.leaf_max : kRebuildLeafDefault;
    const uint32_t n = c.S.num_prims;  // (a BVH context: one record per primitive, 1 <= n < 2^25)
    if (n == 0 || n >= kRebuildMaxPrims) throw NoriException(NORI_ERR_UNSUPPORTED, "nori_gpu_rebuild_bvh: primitive count");
    HIP_TRY(hipSetDevice(c.device));
    for (auto &e : c.rb_ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    hipStream_t st = c.stream;
    auto internal = [](const char *what) {
        return NoriException(NORI_ERR_HIP, std::string("nori_gpu_rebuild_bvh: ") + what + " (nothing was changed)");
    };
    // ---- scratch, sized from n alone: a level has at most n / 2 nodes, the tree fewer than n
    size_t sort_bytes = 0, scan_bytes = 0;
    HIP_TRY(rebuild_sort_keys(nullptr, sort_bytes, nullptr, nullptr, n, st));
    HIP_TRY(rebuild_scan_counts(nullptr, scan_bytes, nullptr, nullptr, n + 1, st));
    c.rb_sort_tmp.ensure(sort_bytes);
    c.rb_scan_tmp.ensure(scan_bytes);
    c.rb_box.ensure(24);
    for (auto &b : c.rb_keys) b.ensure(8 * (size_t)n);
    for (auto &b : c.rb_ranges) b.ensure(8 * (size_t)n);
    c.rb_ends.ensure(16 * (size_t)n);
    c.rb_count.ensure(8 * ((size_t)n + 1));
    c.rb_scan.ensure(8 * ((size_t)n + 1));
    c.rb_refs.ensure(16 * (size_t)n);
    c.rb_inner.ensure(4 * (size_t)n);
    c.rb_leaf.ensure(4 * (size_t)n);
    c.rb_prims.ensure(48 * (size_t)n);
    uint32_t launches = 0;
    // ---- the scene box, then the grid on the host (one division per axis)
    HIP_TRY(hipEventRecord(c.rb_ev[0], st));
    HIP_TRY(launch_rebuild_scene_box(c.S, n, c.rb_box.as<uint32_t>(), st));
    uint32_t boxk[6];
    HIP_TRY(hipMemcpyAsync(boxk, c.rb_box.p, sizeof(boxk), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    float lo[3], scale[3];
    for (int k = 0; k < 3; ++k) {
        lo[k] = rebuild_order_value(boxk[k]);
        scale[k] = rebuild_scale(lo[k], rebuild_order_value(boxk[3 + k]));
    }
    // ---- keys, sort, records
    uint64_t *keys = c.rb_keys[0].as<uint64_t>(), *sorted = c.rb_keys[1].as<uint64_t>();
    HIP_TRY(launch_rebuild_keys(c.S, n, lo, scale, keys, st));
    HIP_TRY(rebuild_sort_keys(c.rb_sort_tmp.p, sort_bytes, keys, sorted, n, st));
    HIP_TRY(launch_rebuild_records(c.S, sorted, n, c.rb_prims.as<float4>(), st));
    launches += 3;
    // ---- topology, one breadth-first level per round
    std::vector<uint32_t> node_begin{0};  // first node of every level, then the node count
    uint32_t leaves = 0, depth = 0;
    int stack = c.stack;
    const uint32_t root_ref[4] = {kRefitLeafBit | ((n - 1) << 25), 0xffffffffu, 0xffffffffu, 0xffffffffu};
    const uint32_t zero = 0, root_range[2] = {0, n - 1};
    if (n <= L) {  // one node, one leaf slot
        HIP_TRY(hipMemcpyAsync(c.rb_refs.p, root_ref, 16, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(c.rb_leaf.p, &zero, 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        node_begin.push_back(1);
        leaves = depth = 1;
        stack = bvh_stack_for(depth, c.stack_forced);
    } else {
        HIP_TRY(hipMemcpyAsync(c.rb_ranges[0].p, root_range, 8, hipMemcpyHostToDevice, st));
        uint32_t m = 1, level_off = 0;
        int cur = 0;
        while (m) {  // (bvh_stack_for throws at the depth limit: at most 26 rounds)
            stack = bvh_stack_for(++depth, c.stack_forced);
            const uint2 *ranges = c.rb_ranges[cur].as<uint2>();
            HIP_TRY(launch_rebuild_split(sorted, ranges, m, L, c.rb_ends.as<uint4>(), c.rb_count.as<uint64_t>(), st));
            HIP_TRY(rebuild_scan_counts(c.rb_scan_tmp.p, scan_bytes, c.rb_count.as<uint64_t>(), c.rb_scan.as<uint64_t>(),
                                        m + 1, st));
            uint64_t total = 0;
            HIP_TRY(hipMemcpyAsync(&total, c.rb_scan.as<uint64_t>() + m, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            const uint64_t inner = total & 0xffffffffull, leaf = total >> 32;
            // the counts size the next launches and index the lists: checked against their bounds first
            if (inner + leaf < 2 * (uint64_t)m || inner + leaf > 4 * (uint64_t)m || (uint64_t)level_off + m + inner > n ||
                (uint64_t)leaves + leaf > n)
                throw internal("a level's slot counts are out of bounds");
            HIP_TRY(launch_rebuild_emit(ranges, c.rb_ends.as<uint4>(), c.rb_scan.as<uint64_t>(), m, level_off, leaves, L,
                                        c.rb_refs.as<uint4>(), c.rb_ranges[cur ^ 1].as<uint2>(),
                                        c.rb_inner.as<uint32_t>(), c.rb_leaf.as<uint32_t>(), st));
            launches += 2;
            level_off += m;
            node_begin.push_back(level_off);
            leaves += (uint32_t)leaf;
            m = (uint32_t)inner;
            cur ^= 1;
        }
    }
    const uint32_t N = node_begin.back();
    // ---- the nodes, and the refit schedule: level 0 = every leaf slot, then the inner slots
    // deepest level first (the inner slot of child node c is entry c - 1 of rb_inner)
    c.rb_nodes.ensure(128 * (size_t)N);
    HIP_TRY(launch_rebuild_nodes(c.rb_refs.as<uint4>(), N, c.rb_nodes.as<float4>(), st));
    ++launches;
    RefitPlan plan;  // (its host `slots` stay empty: the schedule is made on the device)
    plan.level_begin = {0, leaves};
    c.rb_slots.ensure(4 * ((size_t)leaves + N - 1));
    uint32_t *slots = c.rb_slots.as<uint32_t>();
    HIP_TRY(hipMemcpyAsync(slots, c.rb_leaf.p, 4 * (size_t)leaves, hipMemcpyDeviceToDevice, st));
    for (uint32_t d = depth - 1; d-- > 0;) {  // node level d's inner slots = the nodes of level d + 1
        const uint32_t b = node_begin[d + 1] - 1, cnt = node_begin[d + 2] - node_begin[d + 1];
        HIP_TRY(hipMemcpyAsync(slots + plan.level_begin.back(), c.rb_inner.as<uint32_t>() + b, 4 * (size_t)cnt,
                               hipMemcpyDeviceToDevice, st));
        plan.level_begin.push_back(plan.level_begin.back() + cnt);
    }
    // ---- the boxes: the refit's kernel over the new schedule
    for (uint32_t l = 0; l < plan.levels(); ++l) {
        const uint32_t b = plan.level_begin[l], cnt = plan.level_begin[l + 1] - b;
        HIP_TRY(launch_refit_level(c.rb_nodes.as<float4>(), c.rb_prims.as<float4>(), c.S.tri_vidx, c.pos.as<float4>(),
                                   slots + b, cnt, st));
        launches += cnt ? 1u : 0u;
    }
    HIP_TRY(hipEventRecord(c.rb_ev[1], st));
    float root[32], box[6];
    HIP_TRY(hipMemcpyAsync(root, c.rb_nodes.p, sizeof(root), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    refit_root_box(root, box);
    // ---- success: the new tree replaces the old one
    auto swap_buf = [](DevBuf &a, DevBuf &b) {
        std::swap(a.p, b.p);
        std::swap(a.bytes, b.bytes);
    };
    swap_buf(c.nodes, c.rb_nodes);
    swap_buf(c.prims, c.rb_prims);
    swap_buf(c.refit_slots, c.rb_slots);
    c.refit = std::move(plan);
    c.S.nodes = c.nodes.as<float4>();
    c.S.prims = c.prims.as<float4>();
    c.S.num_nodes = N;
    c.bvh_nodes = N;
    c.bvh_depth = depth;
    c.stack = stack;
    c.scene_bytes = 128 * (size_t)N + 48 * (size_t)n;
    for (int k = 0; k < 3; ++k) c.S.root_min[k] = box[k], c.S.root_max[k] = box[3 + k];
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        HIP_TRY(hipEventElapsedTime(&stats->ms_device, c.rb_ev[0], c.rb_ev[1]));
        stats->nodes = N;
        stats->depth = depth;
        stats->stack = (uint32_t)stack;
        stats->levels = c.refit.levels();
        stats->launches = launches;
        stats->ms = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return NORI_OK;
}

int bvh_read(nori_gpu_ctx &c, float *nodes, float *prims, uint32_t *counts) {
    HIP_TRY(hipSetDevice(c.device));
    if (counts) counts[0] = c.S.num_nodes, counts[1] = c.S.num_prims;
    HIP_TRY(hipStreamSynchronize(c.stream));
    if (nodes) HIP_TRY(hipMemcpy(nodes, c.nodes.p, 128 * (size_t)c.S.num_nodes, hipMemcpyDeviceToHost));
    if (prims) HIP_TRY(hipMemcpy(prims, c.prims.p, 48 * (size_t)c.S.num_prims, hipMemcpyDeviceToHost));
    return NORI_OK;
}

}  // namespace
}  // namespace nori

extern "C" {

int nori_gpu_update_vertices(nori_gpu_ctx *c, const nori_gpu_update_desc *ud, nori_gpu_update_stats *stats) {
    return guarded([&] {
        if (!c || !ud || !ud->positions) return fail(NORI_ERR_INVALID, "null argument");
        return update_vertices(*c, *ud, stats);
    });
}

int nori_gpu_bvh_read(nori_gpu_ctx *c, float *nodes, float *prims, uint32_t *counts) {
    return guarded([&] {
        if (!c) return fail(NORI_ERR_INVALID, "null argument");
        return bvh_read(*c, nodes, prims, counts);
    });
}

int nori_gpu_rebuild_bvh(nori_gpu_ctx *c, const nori_gpu_rebuild_desc *rd, nori_gpu_rebuild_stats *stats) {
    return guarded([&] {
        if (!c || !rd) return fail(NORI_ERR_INVALID, "null argument");
        return rebuild_bvh(*c, *rd, stats);
    });
}

}  // extern "C"
