// scene_plan.cpp -- scene_plan.h: knobs, refusals, tables and decisions of a
// context, and the small-scene blob; nori_scene_bvh_info, _scan_list,
// _scan_fast and _bvh_refit.  No HIP here.
#include "scene_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "bsdf_desc.h"

namespace nori {

SceneKnobs scene_knobs(EnvLookup env) {
    SceneKnobs k;
    auto first = [&](const char *name) {  // the text's first character, -1: unset
        const char *e = env(name);
        return e ? (int)(unsigned char)e[0] : -1;
    };
    if (const char *m = env("NORI_TRAVERSAL")) k.traversal = !std::strcmp(m, "bvh") ? 1 : !std::strcmp(m, "scan") ? 2 : 0;
    if (const char *e = env("NORI_BVH_STACK")) {
        const int v = std::atoi(e);
        if (v == 8 || v == 16 || v == 32) k.stack_forced = v;
    }
    k.camera_cull = first("NORI_CAMERA_CULL") != '0';
    if (const char *t = env("NORI_TRACE_CULL")) k.trace_cull = std::atoi(t);
    if (k.trace_cull < 0 || k.trace_cull > 2) k.trace_cull = 1;
    const int nee = first("NORI_NEE_INLINE"), ext = first("NORI_EXT_INLINE"), fuse = first("NORI_TRACE_FUSE");
    k.nee_inline = nee < 0 ? -1 : nee == '1';
    k.ext_inline = ext < 0 ? -1 : ext == '1';
    k.fuse_trace = fuse < 0 ? -1 : fuse != '0';
    k.discrete_nee = first("NORI_DISCRETE_NEE") == '1';
    k.finish_first = first("NORI_FINISH_FIRST") != '0';
    return k;
}

int bvh_stack_for(uint32_t depth, int forced) {
    const uint32_t need = 3 * depth + 1;
    int stack = 32;
    if (need <= (uint32_t)plan_lds_entries(8)) stack = 8;
    else if (need <= (uint32_t)plan_lds_entries(16) + kPlanTraceSpill) stack = 16;
    if (forced) stack = forced;
    if (need > (uint32_t)plan_lds_entries(stack) + kPlanTraceSpill)
        throw NoriException(NORI_ERR_UNSUPPORTED, "BVH too deep for the traversal stack");
    return stack;
}

SceneTree build_scene_tree(const nori_scene_desc &d) {
    SceneTree t;
    scene_root_box(d, t.rmin, t.rmax);
    build_device_bvh(d, t.rmin, t.rmax, t.bvh);
    t.n = (uint32_t)(t.bvh.prims.size() / 12);
    return t;
}
bool scan_mode(uint32_t n, const SceneKnobs &k) { return k.traversal ? k.traversal == 2 : n <= kScanMaxPrims; }
ScanRtcScene scan_rtc_scene(const ScanList &L) {
    return ScanRtcScene{L.prims.data(), (uint32_t)(L.prims.size() / 12), L.plane_c.data(), L.plane_f.data(),
                        (uint32_t)L.plane_c.size(), {L.plane_end[0], L.plane_end[1], L.plane_end[2]}, L.tris, L.real,
                        L.fast_max};
}

namespace {

[[noreturn]] void refuse(int code, const char *msg) { throw NoriException(code, msg); }

void plan_images(const nori_scene_desc &d, ScenePlan &p) {
    p.img_off.resize(d.num_images);
    for (uint32_t i = 0; i < d.num_images; ++i) {
        const nori_image_desc &im = d.images[i];
        if (!im.rgb || im.width <= 0 || im.height <= 0 || (im.wrap != NORI_WRAP_REPEAT && im.wrap != NORI_WRAP_CLAMP))
            refuse(NORI_ERR_INVALID, "bad image description");
        p.img_off[i] = p.tex.size();
        const size_t n = (size_t)im.width * im.height;
        for (size_t t = 0; t < n; ++t)
            p.tex.push_back((uint32_t)im.rgb[3 * t] | ((uint32_t)im.rgb[3 * t + 1] << 8) | ((uint32_t)im.rgb[3 * t + 2] << 16));
    }
    if (p.tex.empty()) p.tex.assign(1, 0u);
}
// The texel offset of image i (negative: none) and, through im, its description
size_t image_texels(const nori_scene_desc &d, const ScenePlan &p, int32_t i, const nori_image_desc *&im) {
    im = nullptr;
    if (i < 0) return ScenePlan::kNoImage;
    if ((uint32_t)i >= d.num_images) refuse(NORI_ERR_INVALID, "image index out of range");
    im = &d.images[i];
    return p.img_off[i];
}

// A mesh's primitives, its area CDF and, where it carries an emitter, what a vertex update needs
void plan_mesh(const nori_scene_desc &d, uint32_t s, DevShape &ds, ScenePlan &p) {
    const nori_shape_desc &sd = d.shapes[s];
    if ((uint64_t)sd.tri_offset + sd.tri_count > d.num_triangles || (uint64_t)sd.vtx_offset + sd.vtx_count > d.num_vertices)
        refuse(NORI_ERR_INVALID, "mesh range outside the scene arrays");
    ds.prim_count = sd.tri_count;
    ds.cdf_offset = (uint32_t)p.cdf.size();
    for (uint32_t t = 0; t < sd.tri_count; ++t) {
        const uint32_t *f = d.indices + 3 * (size_t)(sd.tri_offset + t);
        for (int k = 0; k < 3; ++k)
            if (f[k] >= d.num_vertices) refuse(NORI_ERR_INVALID, "vertex index out of range");
        p.prim_shape.push_back(s);
        p.tri_vidx.insert(p.tri_vidx.end(), {f[0], f[1], f[2]});
    }
    std::vector<float> mc;
    const uint32_t *tri = d.indices + 3 * (size_t)sd.tri_offset;
    ds.area_norm = mesh_area_cdf(tri, sd.tri_count, [&](uint32_t i) { return d.positions + 3 * (size_t)i; }, mc);
    p.cdf.insert(p.cdf.end(), mc.begin(), mc.end());
    if (sd.emitter >= 0 && sd.tri_count) {
        EmitterMesh em;
        em.shape = s;
        em.cdf_offset = ds.cdf_offset;
        em.tri.assign(tri, tri + 3 * (size_t)sd.tri_count);
        const auto mm = std::minmax_element(em.tri.begin(), em.tri.end());
        em.vtx_first = *mm.first;
        em.vtx_count = *mm.second - *mm.first + 1;
        p.emitter_meshes.push_back(std::move(em));
    }
}

void plan_shapes(const nori_scene_desc &d, ScenePlan &p) {
    p.shapes.resize(d.num_shapes);
    p.shape_tex.resize(d.num_shapes);
    uint32_t off = 0;
    for (uint32_t s = 0; s < d.num_shapes; ++s) {
        const nori_shape_desc &sd = d.shapes[s];
        DevShape &ds = p.shapes[s];
        std::memset(&ds, 0, sizeof(ds));
        const nori_image_desc *im;
        p.shape_tex[s] = image_texels(d, p, sd.normal_map, im);
        if (im) {
            ds.nm_w = im->width;
            ds.nm_h = im->height;
            ds.nm_wrap = im->wrap;
        }
        ds.type = sd.type;
        ds.bsdf = sd.bsdf;
        ds.emitter = sd.emitter;
        ds.has_normals = sd.has_normals;
        ds.has_uvs = sd.has_uvs && d.uvs ? 1u : 0u;
        ds.prim_offset = off;
        for (int k = 0; k < 3; ++k) ds.center[k] = sd.center[k];
        ds.radius = sd.radius;
        if (sd.bsdf < 0 || (uint32_t)sd.bsdf >= d.num_bsdfs) refuse(NORI_ERR_INVALID, "shape without a valid bsdf");
        if (sd.type == NORI_SHAPE_SPHERE) {
            ds.prim_count = 1;
            float inv = 1.f / sd.radius;  // sphere.cpp:99-104: pow(1/r, 2) * 1/(4 pi)
            ds.area_norm = (float)((double)inv * (double)inv * (double)(0.25f * 0.31830988618379067154f));
            p.prim_shape.push_back(s);
            p.tri_vidx.insert(p.tri_vidx.end(), {0u, 0u, 0u});
        } else if (sd.type == NORI_SHAPE_MESH) {
            plan_mesh(d, s, ds, p);
        } else {
            refuse(NORI_ERR_INVALID, "unknown shape type");
        }
        off += ds.prim_count;
    }
    p.num_prims = off;
    if (p.cdf.empty()) p.cdf.assign(1, 0.0f);
}

void plan_bsdfs(const nori_scene_desc &d, ScenePlan &p) {
    p.bsdfs.resize(d.num_bsdfs);
    p.bsdf_tex.assign(d.num_bsdfs, ScenePlan::kNoImage);
    for (uint32_t i = 0; i < d.num_bsdfs; ++i) {
        const nori_bsdf_desc &b = d.bsdfs[i];
        DevBsdf &o = p.bsdfs[i];
        dev_bsdf_from_desc(b, o);  // desc values and derived constants (bsdf_desc.h)
        if (b.albedo_texture == NORI_TEXTURE_IMAGE) {
            const nori_image_desc *im;
            p.bsdf_tex[i] = image_texels(d, p, b.albedo_image, im);
            if (!im) refuse(NORI_ERR_INVALID, "ImageTexture albedo without an image");
            o.img_w = im->width;
            o.img_h = im->height;
            o.img_wrap = im->wrap;
        } else if (b.albedo_texture != NORI_TEXTURE_CONSTANT && b.albedo_texture != NORI_TEXTURE_CHECKERBOARD) {
            refuse(NORI_ERR_INVALID, "unknown albedo texture");
        }
        if (b.type < NORI_BSDF_DIFFUSE || b.type > NORI_BSDF_DISNEY) refuse(NORI_ERR_INVALID, "unknown bsdf type");
    }
}

void plan_emitters(const nori_scene_desc &d, ScenePlan &p) {
    p.emitters.resize(d.num_emitters);
    for (uint32_t i = 0; i < d.num_emitters; ++i) {
        const nori_emitter_desc &e = d.emitters[i];
        if (e.type != NORI_EMITTER_AREA && e.type != NORI_EMITTER_ENVMAP && e.type != NORI_EMITTER_POINT &&
            e.type != NORI_EMITTER_SPOT)
            refuse(NORI_ERR_UNSUPPORTED, "unknown emitter type");
        const bool free_standing = e.type == NORI_EMITTER_POINT || e.type == NORI_EMITTER_SPOT;
        if (!free_standing && (e.shape < 0 || (uint32_t)e.shape >= d.num_shapes))
            refuse(NORI_ERR_INVALID, "emitter without a shape");
        DevEmitter &o = p.emitters[i];
        std::memset(&o, 0, sizeof(DevEmitter));
        o.type = e.type;
        o.shape = free_standing ? -1 : e.shape;
        for (int k = 0; k < 3; ++k) {
            o.radiance[k] = e.radiance[k];
            o.position[k] = e.position[k];
            o.power[k] = e.power[k];
            o.direction[k] = e.direction[k];
        }
        o.cos_fs = e.cos_falloff_start;
        o.cos_tw = e.cos_total_width;
        if (e.type == NORI_EMITTER_ENVMAP) {
            const EnvTables t = build_envmap(e, p.env);
            o.weight = e.weight;
            o.R = e.env_rows;
            o.C = e.env_cols;
            o.rgb_off = t.rgb_off, o.pdf_off = t.pdf_off, o.cdf_off = t.cdf_off;
            o.pmarg_off = t.pmarg_off, o.cmarg_off = t.cmarg_off;
        }
    }
}

// The refusals that follow from the description's settings alone.  Output
// size and filter radius come before the tree is built (they cost nothing).
void check_settings(const nori_scene_desc &d, ScenePlan &p) {
    if (d.integrator < NORI_INTEGRATOR_PATH_MATS || d.integrator > NORI_INTEGRATOR_PHOTONMAPPER)
        refuse(NORI_ERR_UNSUPPORTED, "unknown integrator");
    if (d.num_emitters == 0 && d.integrator != NORI_INTEGRATOR_NORMALS && d.integrator != NORI_INTEGRATOR_AV)
        refuse(NORI_ERR_INVALID, "the scene has no emitter");
    if (d.integrator == NORI_INTEGRATOR_PHOTONMAPPER) {
        if (d.photon_count == 0 || !(d.photon_radius > 0.0f) || !std::isfinite(d.photon_radius))
            refuse(NORI_ERR_INVALID, "photonmapper: photon_count and photon_radius must be positive");
        for (uint32_t i = 0; i < d.num_emitters; ++i)  // Emitter::samplePhoton (emitter.h) throws for the others
            if (d.emitters[i].type != NORI_EMITTER_AREA)
                refuse(NORI_ERR_UNSUPPORTED, "photonmapper: photons from area lights only");
    }
    if (d.camera.camera_type < NORI_CAMERA_PERSPECTIVE || d.camera.camera_type > NORI_CAMERA_ADVANCED)
        refuse(NORI_ERR_UNSUPPORTED, "unknown camera type");
    // the reference leaves Scene::m_medium uninitialised without a <medium>
    // (scene.h:141): rejected here, as in the oracle
    if (d.integrator == NORI_INTEGRATOR_VOLUMETRIC && !d.medium.present)
        refuse(NORI_ERR_INVALID, "the volumetric integrator needs a <medium>");
    if (d.camera.width <= 0 || d.camera.height <= 0) refuse(NORI_ERR_INVALID, "bad output size");
    p.border = film_border(d.camera);
    if (p.border > 4) refuse(NORI_ERR_UNSUPPORTED, "filter radius above 4.5 pixels");
}

void plan_vertices(const nori_scene_desc &d, ScenePlan &p) {
    p.pos.resize(4 * (size_t)d.num_vertices);
    p.nrm.resize(4 * (size_t)d.num_vertices);
    for (uint32_t v = 0; v < d.num_vertices; ++v) {
        for (int k = 0; k < 3; ++k) {
            p.pos[4 * (size_t)v + k] = d.positions[3 * (size_t)v + k];
            p.nrm[4 * (size_t)v + k] = d.normals ? d.normals[3 * (size_t)v + k] : 0.0f;
        }
        // texture coordinates ride in the w lanes (u with the position, v with the normal)
        p.pos[4 * (size_t)v + 3] = d.uvs ? d.uvs[2 * (size_t)v] : 0.0f;
        p.nrm[4 * (size_t)v + 3] = d.uvs ? d.uvs[2 * (size_t)v + 1] : 0.0f;
    }
    if (p.pos.empty()) p.pos.assign(4, 0.0f), p.nrm.assign(4, 0.0f);
    if (p.env.empty()) p.env.assign(4, 0.0f);
}

// Tree, traversal, stack, scan list or refit plan
void plan_traversal(const nori_scene_desc &d, const SceneKnobs &k, ScenePlan &p) {
    p.tree = build_scene_tree(d);  // (plan_shapes has validated the mesh ranges scene_root_box reads)
    const std::vector<uint8_t> solitary = solitary_spheres(d, p.tree.rmin, p.tree.rmax);
    for (uint32_t s = 0; s < d.num_shapes; ++s) p.shapes[s].solitary = solitary[s];
    p.scan = scan_mode(p.num_prims, k);
    p.stack_forced = k.stack_forced;
    p.stack = bvh_stack_for(p.tree.bvh.depth, k.stack_forced);
    if (p.scan) {
        p.stack = 0;
        p.scan_list = build_scan_list(p.tree.bvh, p.num_prims);
    } else {
        p.refit = build_refit_plan(p.tree.bvh);
    }
    p.camera_cull = k.camera_cull;
    p.trace_cull = k.trace_cull == 2 && p.scan_list.plane_f.empty() ? 1 : k.trace_cull;  // 2 needs plane pairs
}

void plan_decisions(const nori_scene_desc &d, const SceneKnobs &k, ScenePlan &p) {
    const nori_camera_desc &cam = d.camera;
    p.chroma = cam.camera_type == NORI_CAMERA_ADVANCED &&
               (cam.chromatic[0] != 0.0f || cam.chromatic[1] != 0.0f || cam.chromatic[2] != 0.0f);
    p.basic = basic_scene(d);
    // shadow rays traced inside k_shade (scan-mode scenes): on by default
    // for the basic-plugin kernels (C2 +3-7 %, its 64-spp share +3 %), off
    // for the full ones (C4 -5.7 %, C5 -4.3 %: the full k_shade holds 90-96
    // VGPRs, and the queue's shadow kernel is the scene-specialised one).
    // NORI_NEE_INLINE=0 / 1 forces it off / on for scan-mode scenes whose
    // shade kernel carries it (the basic ones; kernel_config.h kNeeFull).
    p.nee_inline = p.scan && (k.nee_inline >= 0 ? k.nee_inline == 1 : p.basic) && (p.basic || kPlanNeeFull);
    // ... and each vertex's extension ray (k_shade's closest-hit scan in
    // place of the extension launch and the hit's round trip through
    // memory): scan-mode scenes with the basic plugins and the inline
    // shadow rays.  NORI_EXT_INLINE=0 / 1 forces it off / on there.
    p.ext_inline = p.scan && p.basic && p.nee_inline && (k.ext_inline >= 0 ? k.ext_inline == 1 : true);
    // one launch for an iteration's extension and shadow queues: on for
    // the BVH walks (C3 +10 %) and the basic scan kernels that keep the
    // queue; the full-plugin scan scenes run faster with two launches
    // (C4 3942 -> 3957, C5 4217 -> 4288 Msamples/s, 3 interleaved reps,
    // tools/gpu_fuse_ab.sh).  NORI_TRACE_FUSE=0 / 1 forces it.
    p.fuse_trace = k.fuse_trace >= 0 ? k.fuse_trace == 1 : !(p.scan && !p.basic);
    p.finish_first = k.finish_first;
    p.jit_lk = jit_code_lookup(cam.filter_radius, NORI_FILTER_RESOLUTION / cam.filter_radius);
    // deviation D10 (shading.h skip_nee); NORI_DISCRETE_NEE=1 keeps the full NEE everywhere
    bool env = false;
    for (uint32_t i = 0; i < d.num_emitters; ++i) env = env || d.emitters[i].type == NORI_EMITTER_ENVMAP;
    p.skip_discrete_nee = !env && !k.discrete_nee;
    uint32_t offs[10];
    p.blob_bytes = blob_layout(p, offs);
    p.use_blob = p.scan && p.blob_bytes <= kBlobMaxBytes;
    // The scan kernels compiled for this scene's scan list (rtc.hip; else the
    // generic ones), and k_shade where it can hold a scan: the basic plugin
    // set, an integrator of the wavefront loop.
    const size_t records = p.scan_list.prims.size() / 12;
    p.build_scan = p.scan && records <= 2 * kScanMaxPrims;
    p.build_shade = p.build_scan && p.basic && d.integrator < NORI_INTEGRATOR_NORMALS;
    p.shade_integrator = plan_shade_integrator(d.integrator);
    p.shade_lds = p.use_blob && p.blob_bytes <= kPlanShadeLdsMax;
}

// The ten tables of the blob, in order
struct BlobTable {
    const void *p;
    size_t bytes;
};
void blob_tables(const ScenePlan &p, BlobTable t[10]) {
    const std::vector<float> &prims = p.prim_list();
    t[0] = {prims.data(), prims.size() * 4};
    t[1] = {p.tri_vidx.data(), p.tri_vidx.size() * 4};
    t[2] = {p.pos.data(), p.pos.size() * 4};
    t[3] = {p.nrm.data(), p.nrm.size() * 4};
    t[4] = {p.prim_shape.data(), p.prim_shape.size() * 4};
    t[5] = {p.shapes.data(), p.shapes.size() * sizeof(DevShape)};
    t[6] = {p.bsdfs.data(), p.bsdfs.size() * sizeof(DevBsdf)};
    t[7] = {p.emitters.data(), p.emitters.size() * sizeof(DevEmitter)};
    t[8] = {p.cdf.data(), p.cdf.size() * 4};
    t[9] = {p.tree.bvh.nodes.data(), p.tree.bvh.nodes.size() * 4};
}

}  // namespace

ScenePlan plan_scene(const nori_scene_desc &d, const SceneKnobs &k) {
    ScenePlan p;
    plan_images(d, p);
    plan_shapes(d, p);
    plan_bsdfs(d, p);
    plan_emitters(d, p);
    check_settings(d, p);
    plan_traversal(d, k, p);
    plan_vertices(d, p);
    plan_decisions(d, k, p);
    return p;
}

size_t blob_layout(const ScenePlan &p, uint32_t offs[10]) {
    BlobTable t[10];
    blob_tables(p, t);
    size_t n = 0;
    for (int k = 0; k < 10; ++k) {
        n = (n + 15) / 16 * 16;
        offs[k] = (uint32_t)n;
        n += t[k].bytes;
    }
    return (n + 15) / 16 * 16;
}
void pack_blob(const ScenePlan &p, std::vector<char> &blob, uint32_t offs[10]) {
    BlobTable t[10];
    blob_tables(p, t);
    blob.assign(blob_layout(p, offs), 0);
    for (int k = 0; k < 10; ++k)
        if (t[k].bytes) std::memcpy(blob.data() + offs[k], t[k].p, t[k].bytes);
}

}  // namespace nori

using namespace nori;

// The C ABI's entry points that start from the scene's tree and need no device
extern "C" {

int nori_scene_bvh_info(const nori_scene_desc *d, nori_bvh_info *out) {
    return guarded([&] {
        if (!d || !out) return fail(NORI_ERR_INVALID, "null argument");
        if (d->abi_version != NORI_GPU_ABI_VERSION) return fail(NORI_ERR_INVALID, "ABI version mismatch");
        const SceneTree tree = build_scene_tree(*d);
        const DeviceBvh &bvh = tree.bvh;
        std::memset(out, 0, sizeof(*out));
        out->ref_nodes = bvh.ref_nodes;
        out->device_nodes = bvh.num_nodes;
        out->depth = bvh.depth;
        out->num_prims = tree.n;
        out->sah_cost = bvh.sah_cost;
        uint64_t h = 1469598103934665603ull;
        for (size_t i = 0; i < bvh.prims.size(); i += 12) {
            uint32_t id;
            std::memcpy(&id, &bvh.prims[i + 3], 4);
            for (int k = 0; k < 4; ++k) h = (h ^ ((id >> (8 * k)) & 0xFFu)) * 1099511628211ull;
        }
        out->order_hash = h;
        return NORI_OK;
    });
}
int nori_scene_scan_list(const nori_scene_desc *d, nori_scan_info *info, float *records, float *plane_c,
                         float *plane_f) {
    return guarded([&] {
        if (!d || !info) return fail(NORI_ERR_INVALID, "null argument");
        if (d->abi_version != NORI_GPU_ABI_VERSION) return fail(NORI_ERR_INVALID, "ABI version mismatch");
        const SceneTree tree = build_scene_tree(*d);
        std::memset(info, 0, sizeof(*info));
        if (!scan_mode(tree.n, SceneKnobs{})) return NORI_OK;  // a BVH scene by its size: no scan list
        const ScanList L = build_scan_list(tree.bvh, tree.n);
        info->records = (uint32_t)(L.prims.size() / 12);
        info->pairs = (uint32_t)L.plane_c.size();
        for (int a = 0; a < 3; ++a) info->plane_end[a] = L.plane_end[a];
        info->tris = L.tris;
        if (records) std::memcpy(records, L.prims.data(), L.prims.size() * 4);
        if (plane_c && !L.plane_c.empty()) std::memcpy(plane_c, L.plane_c.data(), L.plane_c.size() * 4);
        if (plane_f && !L.plane_f.empty()) std::memcpy(plane_f, L.plane_f.data(), L.plane_f.size() * 4);
        return NORI_OK;
    });
}
int nori_scene_scan_fast(const nori_scene_desc *d, float *fast_max) {
    return guarded([&] {
        if (!d || !fast_max) return fail(NORI_ERR_INVALID, "null argument");
        if (d->abi_version != NORI_GPU_ABI_VERSION) return fail(NORI_ERR_INVALID, "ABI version mismatch");
        const SceneTree tree = build_scene_tree(*d);
        *fast_max = scan_mode(tree.n, SceneKnobs{}) ? build_scan_list(tree.bvh, tree.n).fast_max : 0.0f;
        return NORI_OK;
    });
}

int nori_scene_bvh_refit(const nori_scene_desc *d, const float *positions, float *nodes, float *prims, float *root_box) {
    return guarded([&] {
        if (!d) return fail(NORI_ERR_INVALID, "null argument");
        if (d->abi_version != NORI_GPU_ABI_VERSION) return fail(NORI_ERR_INVALID, "ABI version mismatch");
        if (positions)
            for (size_t i = 0; i < 3 * (size_t)d->num_vertices; ++i)
                if (!std::isfinite(positions[i])) return fail(NORI_ERR_INVALID, "nori_scene_bvh_refit: a non-finite position");
        SceneTree tree = build_scene_tree(*d);
        DeviceBvh &bvh = tree.bvh;
        if (positions) refit_host(bvh, build_refit_plan(bvh), prim_vertex_ids(*d), positions, nullptr);
        if (nodes) std::memcpy(nodes, bvh.nodes.data(), bvh.nodes.size() * 4);
        if (prims) std::memcpy(prims, bvh.prims.data(), bvh.prims.size() * 4);
        if (root_box) refit_root_box(bvh.nodes.data(), root_box);
        return NORI_OK;
    });
}

}  // extern "C"
