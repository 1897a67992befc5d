// scene_plan.h -- everything nori_gpu_create settles before its first HIP
// call: the refusals of a bad nori_scene_desc, the host tables of the scene,
// the environment knobs as parsed values, and the decisions that follow from
// them (scan or BVH, stack, blob, which hipRTC programs to build).  Plain C++
// without HIP types, compiled by the host compiler (scene_plan.cpp), so
// tests/scene_plan_check.cpp runs it under the sanitizers as a program of its
// own.  upload.hip uploads what the plan holds and fills DevScene from it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "dev_records.h"
#include "scene_prep.h"

namespace nori {

// kernels.h's kTraceSpill, stack_lds_entries, kShadeLdsMax and
// shade_integrator, and kernel_config.h's kNeeFull: those headers need hipcc,
// so the values are restated here and upload.hip asserts that they agree.
constexpr int kPlanTraceSpill = 64;
#ifndef NORI_STACK_KEYS
#define NORI_STACK_KEYS 1
#endif
constexpr int plan_lds_entries(int stack) { return NORI_STACK_KEYS ? stack / 2 : stack; }
#ifndef NORI_SHADE_LDS_MAX
#define NORI_SHADE_LDS_MAX 16384
#endif
constexpr uint32_t kPlanShadeLdsMax = NORI_SHADE_LDS_MAX;
#ifndef NORI_NEE_FULL
#define NORI_NEE_FULL 0
#endif
constexpr bool kPlanNeeFull = NORI_NEE_FULL;
constexpr int plan_shade_integrator(int i) {
    return i == NORI_INTEGRATOR_PATH_MATS || i == NORI_INTEGRATOR_VOLUMETRIC ? i : (int)NORI_INTEGRATOR_PATH_MIS;
}

// The environment knobs of a context, parsed.  scene_knobs is the only place
// their text is read; `env` answers like std::getenv (null: unset).
struct SceneKnobs {
    int traversal = 0;         // NORI_TRAVERSAL: 1 "bvh", 2 "scan", 0 by size (any other text)
    int stack_forced = 0;      // NORI_BVH_STACK: 8, 16 or 32, else 0 (bvh_stack_for chooses)
    bool camera_cull = true;   // NORI_CAMERA_CULL: off only for a leading 0
    int trace_cull = 1;        // NORI_TRACE_CULL: 0, 1 or 2; anything else 1
    int nee_inline = -1;       // NORI_NEE_INLINE: -1 unset, else 1 for a leading 1 and 0 otherwise
    int ext_inline = -1;       // NORI_EXT_INLINE: the same
    int fuse_trace = -1;       // NORI_TRACE_FUSE: -1 unset, else 0 for a leading 0 and 1 otherwise
    bool discrete_nee = false; // NORI_DISCRETE_NEE: on only for a leading 1
    bool finish_first = true;  // NORI_FINISH_FIRST: off only for a leading 0
};
using EnvLookup = const char *(*)(const char *name);
SceneKnobs scene_knobs(EnvLookup env);

// The traversal stack of a 4-wide tree of `depth` levels (nori_gpu_create and
// nori_gpu_rebuild_bvh): at most 3 entries per level; the first `stack` live
// in LDS, up to kTraceSpill more in private memory (an 8-wide tree, 256-B
// nodes with a 19-comparator child order, was measured 15 % slower on C3 in
// round 5: DESIGN_LOG.md).  LDS budget 16 words: measured best on the 22.7k
// and 524k triangle scenes -- occupancy beats a deeper LDS part; 32 only when
// the spill area could not cover the rest.  forced: NORI_BVH_STACK's 8, 16 or
// 32 (tuning), or 0.  Throws for a tree too deep for the stack.
int bvh_stack_for(uint32_t depth, int forced);

// The scene box, the tree over it and the primitive count: what every
// nori_scene_* entry point and the plan start from.  Reads the mesh ranges
// unchecked (scene_root_box).
struct SceneTree {
    float rmin[3], rmax[3];
    DeviceBvh bvh;
    uint32_t n = 0;
};
SceneTree build_scene_tree(const nori_scene_desc &d);
// The one traversal rule: scenes of at most kScanMaxPrims primitives are
// intersected by a wave-uniform scan (scalar loads, no divergence), larger
// ones by per-lane BVH traversal; NORI_TRAVERSAL=bvh|scan overrides.
bool scan_mode(uint32_t n, const SceneKnobs &k);
// A scan list as the hipRTC programs take it (pointers into L).
ScanRtcScene scan_rtc_scene(const ScanList &L);

// nori_gpu_update_vertices recomputes the area CDF of a mesh that carries an emitter
struct EmitterMesh {
    uint32_t shape, cdf_offset, vtx_first, vtx_count;  // the vertex range its triangles use
    std::vector<uint32_t> tri;                          // 3 global vertex ids per triangle
};

struct ScenePlan {
    // ---- tables, as they are uploaded
    std::vector<uint32_t> tex;     // 8-bit RGB -> one RGBX word per texel of every image, so a lookup is one 4-byte load
    std::vector<size_t> img_off;   // first texel of image i
    // the records' nmap / img stay null: the texels have no address yet.
    // shape_tex[s] / bsdf_tex[i]: the texel offset of the record's image, or kNoImage
    static constexpr size_t kNoImage = ~(size_t)0;
    std::vector<DevShape> shapes;
    std::vector<DevBsdf> bsdfs;
    std::vector<DevEmitter> emitters;
    std::vector<size_t> shape_tex, bsdf_tex;
    std::vector<uint32_t> prim_shape, tri_vidx;
    std::vector<float> cdf, env;   // per-mesh area CDFs; envmap tables of every envmap emitter
    std::vector<float> pos, nrm;   // float4 per vertex: texture u rides with the position, v with the normal
    std::vector<EmitterMesh> emitter_meshes;
    SceneTree tree;
    ScanList scan_list;            // scan mode
    RefitPlan refit;               // BVH mode: the order in which a refit recomputes the boxes
    uint32_t num_prims = 0;
    const std::vector<float> &prim_list() const { return scan ? scan_list.prims : tree.bvh.prims; }
    // ---- decisions
    bool scan = false;
    int stack = 0, stack_forced = 0;  // 0 = wave-uniform scan, else the LDS stack depth
    int trace_cull = 1;
    bool camera_cull = true, basic = false, chroma = false, nee_inline = false, ext_inline = false, fuse_trace = true,
         finish_first = true, skip_discrete_nee = false;
    int border = 0, jit_lk = 0;
    size_t blob_bytes = 0;         // pack_blob's size
    bool use_blob = false;         // ... uploaded and staged into LDS by the tail finisher
    bool build_scan = false, build_shade = false;  // the hipRTC programs of this scene (rtc.hip)
    int shade_integrator = 0;      // ... the shade program's template arguments
    bool shade_lds = false;
};
// Throws NoriException for a description nori_gpu_create refuses.
ScenePlan plan_scene(const nori_scene_desc &d, const SceneKnobs &k);

// The small-scene blob: the ten tables (records, vertex ids, positions,
// normals, primitive -> shape, shapes, bsdfs, emitters, CDFs, nodes), each
// 16-byte aligned, padded to 16 at the end.  offs: where each begins.  The
// one statement of the layout; its size does not depend on pointer values.
size_t blob_layout(const ScenePlan &p, uint32_t offs[10]);
void pack_blob(const ScenePlan &p, std::vector<char> &blob, uint32_t offs[10]);

}  // namespace nori
