// upload.hip -- nori_gpu_create: a scene description becomes a context's
// device buffers, DevScene and scene-specific kernels (rtc.hip).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "bsdf_desc.h"
#include "ctx.h"

namespace nori {

static_assert(kScanListGroup == kScanGroup, "scene_prep.h and dev_scene.h disagree on NORI_SCAN_GROUP");

// The traversal stack of a 4-wide tree of `depth` levels (nori_gpu_create and
// nori_gpu_rebuild_bvh): at most 3 entries per level; the first `stack` live
// in LDS, up to kTraceSpill more in private memory (an 8-wide tree, 256-B
// nodes with a 19-comparator child order, was measured 15 % slower on C3 in
// round 5: DESIGN_LOG.md).  LDS budget 16 words: measured best on the 22.7k
// and 524k triangle scenes -- occupancy beats a deeper LDS part; 32 only when
// the spill area could not cover the rest.  forced: NORI_BVH_STACK's 8, 16 or
// 32 (tuning), or 0.  Throws for a tree too deep for the stack.
int bvh_stack_for(uint32_t depth, int forced) {
    const uint32_t need = 3 * depth + 1;
    int stack = 32;
    if (need <= (uint32_t)stack_lds_entries(8)) stack = 8;
    else if (need <= (uint32_t)stack_lds_entries(16) + kTraceSpill) stack = 16;
    if (forced) stack = forced;
    if (need > (uint32_t)stack_lds_entries(stack) + kTraceSpill) throw NoriException(NORI_ERR_UNSUPPORTED, "BVH too deep for the traversal stack");
    return stack;
}

namespace {

// The size of the small-scene blob upload_scene builds (its ten tables, each
// 16-byte aligned), from the description alone: nori_scene_shade_rtc chooses
// the shade kernel's LDS variant with it, without a device.
size_t scene_blob_bytes(const nori_scene_desc &d, size_t prim_floats, size_t node_floats) {
    size_t prims = 0, cdf = 0;
    for (uint32_t s = 0; s < d.num_shapes; ++s) {
        const bool mesh = d.shapes[s].type == NORI_SHAPE_MESH;
        prims += mesh ? d.shapes[s].tri_count : 1u;
        cdf += mesh ? (size_t)d.shapes[s].tri_count + 1 : 0u;
    }
    const size_t vtx = d.num_vertices ? d.num_vertices : 1u;
    const size_t parts[10] = {prim_floats * 4, prims * 12, vtx * 16, vtx * 16, prims * 4, d.num_shapes * sizeof(DevShape),
                              d.num_bsdfs * sizeof(DevBsdf), d.num_emitters * sizeof(DevEmitter), (cdf ? cdf : 1u) * 4,
                              node_floats * 4};
    size_t n = 0;
    for (size_t b : parts) n = (n + 15) / 16 * 16 + b;
    return (n + 15) / 16 * 16;
}
// Scenes whose k_shade can hold a scan, and so get a compilation of their own
// (rtc.hip): scan mode with a scan list the scan program takes, the basic
// plugin set, an integrator of the wavefront loop.
bool shade_rtc_scene(const nori_scene_desc &d, bool scan, size_t records) {
    return scan && records <= 2 * kScanMaxPrims && basic_scene(d) && d.integrator < NORI_INTEGRATOR_NORMALS;
}

ScanRtcScene rtc_scene_of(const ScanList &L) {
    return ScanRtcScene{L.prims.data(), (uint32_t)(L.prims.size() / 12), L.plane_c.data(), L.plane_f.data(),
                        (uint32_t)L.plane_c.size(), {L.plane_end[0], L.plane_end[1], L.plane_end[2]}, L.tris, L.real,
                        L.fast_max};
}

void upload_scene(nori_gpu_ctx &c, const nori_scene_desc &d) {
    // image textures and normal maps: 8-bit RGB -> one RGBX word per texel, so
    // a lookup is one 4-byte load; DevBsdf/DevShape hold pointers into it
    std::vector<size_t> img_off(d.num_images);
    {
        std::vector<uint32_t> tex;
        for (uint32_t i = 0; i < d.num_images; ++i) {
            const nori_image_desc &im = d.images[i];
            if (!im.rgb || im.width <= 0 || im.height <= 0 || (im.wrap != NORI_WRAP_REPEAT && im.wrap != NORI_WRAP_CLAMP))
                throw NoriException(NORI_ERR_INVALID, "bad image description");
            img_off[i] = tex.size();
            const size_t n = (size_t)im.width * im.height;
            for (size_t t = 0; t < n; ++t)
                tex.push_back((uint32_t)im.rgb[3 * t] | ((uint32_t)im.rgb[3 * t + 1] << 8) | ((uint32_t)im.rgb[3 * t + 2] << 16));
        }
        if (tex.empty()) tex.assign(1, 0u);
        c.tex.upload(tex);
    }
    auto image_ptr = [&](int32_t i) -> const uint32_t * {
        if (i < 0) return nullptr;
        if ((uint32_t)i >= d.num_images) throw NoriException(NORI_ERR_INVALID, "image index out of range");
        return c.tex.as<uint32_t>() + img_off[i];
    };
    std::vector<DevShape> shapes(d.num_shapes);
    std::vector<uint32_t> prim_shape, tri_vidx;
    std::vector<float> cdf;
    std::vector<nori_gpu_ctx::EmitterMesh> emitter_meshes;
    uint32_t off = 0;
    for (uint32_t s = 0; s < d.num_shapes; ++s) {
        const nori_shape_desc &sd = d.shapes[s];
        DevShape &ds = shapes[s];
        std::memset(&ds, 0, sizeof(ds));
        ds.nmap = image_ptr(sd.normal_map);
        if (ds.nmap) {
            ds.nm_w = d.images[sd.normal_map].width;
            ds.nm_h = d.images[sd.normal_map].height;
            ds.nm_wrap = d.images[sd.normal_map].wrap;
        }
        ds.type = sd.type;
        ds.bsdf = sd.bsdf;
        ds.emitter = sd.emitter;
        ds.has_normals = sd.has_normals;
        ds.has_uvs = sd.has_uvs && d.uvs ? 1u : 0u;
        ds.prim_offset = off;
        for (int k = 0; k < 3; ++k) ds.center[k] = sd.center[k];
        ds.radius = sd.radius;
        if (sd.bsdf < 0 || (uint32_t)sd.bsdf >= d.num_bsdfs) throw NoriException(NORI_ERR_INVALID, "shape without a valid bsdf");
        if (sd.type == NORI_SHAPE_SPHERE) {
            ds.prim_count = 1;
            float inv = 1.f / sd.radius;  // sphere.cpp:99-104: pow(1/r, 2) * 1/(4 pi)
            ds.area_norm = (float)((double)inv * (double)inv * (double)(0.25f * 0.31830988618379067154f));
            prim_shape.push_back(s);
            tri_vidx.insert(tri_vidx.end(), {0u, 0u, 0u});
        } else if (sd.type == NORI_SHAPE_MESH) {
            if ((uint64_t)sd.tri_offset + sd.tri_count > d.num_triangles || (uint64_t)sd.vtx_offset + sd.vtx_count > d.num_vertices)
                throw NoriException(NORI_ERR_INVALID, "mesh range outside the scene arrays");
            ds.prim_count = sd.tri_count;
            ds.cdf_offset = (uint32_t)cdf.size();
            for (uint32_t t = 0; t < sd.tri_count; ++t) {
                const uint32_t *f = d.indices + 3 * (size_t)(sd.tri_offset + t);
                for (int k = 0; k < 3; ++k)
                    if (f[k] >= d.num_vertices) throw NoriException(NORI_ERR_INVALID, "vertex index out of range");
                prim_shape.push_back(s);
                tri_vidx.insert(tri_vidx.end(), {f[0], f[1], f[2]});
            }
            std::vector<float> mc;
            const uint32_t *tri = d.indices + 3 * (size_t)sd.tri_offset;
            ds.area_norm = mesh_area_cdf(tri, sd.tri_count, [&](uint32_t i) { return d.positions + 3 * (size_t)i; }, mc);
            cdf.insert(cdf.end(), mc.begin(), mc.end());
            if (sd.emitter >= 0 && sd.tri_count) {  // nori_gpu_update_vertices recomputes this mesh's CDF
                nori_gpu_ctx::EmitterMesh em;
                em.shape = s;
                em.cdf_offset = ds.cdf_offset;
                em.tri.assign(tri, tri + 3 * (size_t)sd.tri_count);
                const auto mm = std::minmax_element(em.tri.begin(), em.tri.end());
                em.vtx_first = *mm.first;
                em.vtx_count = *mm.second - *mm.first + 1;
                emitter_meshes.push_back(std::move(em));
            }
        } else {
            throw NoriException(NORI_ERR_INVALID, "unknown shape type");
        }
        off += ds.prim_count;
    }
    c.num_prims = off;
    float rmin[3], rmax[3];  // (the loop above has validated the mesh ranges scene_root_box reads)
    scene_root_box(d, rmin, rmax);
    const std::vector<uint8_t> solitary = solitary_spheres(d, rmin, rmax);
    for (uint32_t s = 0; s < d.num_shapes; ++s) shapes[s].solitary = solitary[s];
    std::vector<DevBsdf> bsdfs(d.num_bsdfs);
    for (uint32_t i = 0; i < d.num_bsdfs; ++i) {
        const nori_bsdf_desc &b = d.bsdfs[i];
        DevBsdf &o = bsdfs[i];
        dev_bsdf_from_desc(b, o);  // desc values and derived constants (bsdf_desc.h)
        if (b.albedo_texture == NORI_TEXTURE_IMAGE) {
            o.img = image_ptr(b.albedo_image);
            if (!o.img) throw NoriException(NORI_ERR_INVALID, "ImageTexture albedo without an image");
            o.img_w = d.images[b.albedo_image].width;
            o.img_h = d.images[b.albedo_image].height;
            o.img_wrap = d.images[b.albedo_image].wrap;
        } else if (b.albedo_texture != NORI_TEXTURE_CONSTANT && b.albedo_texture != NORI_TEXTURE_CHECKERBOARD) {
            throw NoriException(NORI_ERR_INVALID, "unknown albedo texture");
        }
        if (b.type < NORI_BSDF_DIFFUSE || b.type > NORI_BSDF_DISNEY) throw NoriException(NORI_ERR_INVALID, "unknown bsdf type");
    }
    std::vector<DevEmitter> emitters(d.num_emitters);
    std::vector<float> env;  // envmap tables of every envmap emitter
    for (uint32_t i = 0; i < d.num_emitters; ++i) {
        const nori_emitter_desc &e = d.emitters[i];
        if (e.type != NORI_EMITTER_AREA && e.type != NORI_EMITTER_ENVMAP && e.type != NORI_EMITTER_POINT &&
            e.type != NORI_EMITTER_SPOT)
            throw NoriException(NORI_ERR_UNSUPPORTED, "unknown emitter type");
        const bool free_standing = e.type == NORI_EMITTER_POINT || e.type == NORI_EMITTER_SPOT;
        if (!free_standing && (e.shape < 0 || (uint32_t)e.shape >= d.num_shapes))
            throw NoriException(NORI_ERR_INVALID, "emitter without a shape");
        std::memset(&emitters[i], 0, sizeof(DevEmitter));
        emitters[i].type = e.type;
        emitters[i].shape = free_standing ? -1 : e.shape;
        for (int k = 0; k < 3; ++k) {
            emitters[i].radiance[k] = e.radiance[k];
            emitters[i].position[k] = e.position[k];
            emitters[i].power[k] = e.power[k];
            emitters[i].direction[k] = e.direction[k];
        }
        emitters[i].cos_fs = e.cos_falloff_start;
        emitters[i].cos_tw = e.cos_total_width;
        if (e.type == NORI_EMITTER_ENVMAP) {
            const EnvTables t = build_envmap(e, env);
            DevEmitter &o = emitters[i];
            o.weight = e.weight;
            o.R = e.env_rows;
            o.C = e.env_cols;
            o.rgb_off = t.rgb_off, o.pdf_off = t.pdf_off, o.cdf_off = t.cdf_off;
            o.pmarg_off = t.pmarg_off, o.cmarg_off = t.cmarg_off;
        }
    }
    if (d.integrator < NORI_INTEGRATOR_PATH_MATS || d.integrator > NORI_INTEGRATOR_PHOTONMAPPER)
        throw NoriException(NORI_ERR_UNSUPPORTED, "unknown integrator");
    if (d.num_emitters == 0 && d.integrator != NORI_INTEGRATOR_NORMALS && d.integrator != NORI_INTEGRATOR_AV)
        throw NoriException(NORI_ERR_INVALID, "the scene has no emitter");
    if (d.integrator == NORI_INTEGRATOR_PHOTONMAPPER) {
        if (d.photon_count == 0 || !(d.photon_radius > 0.0f) || !std::isfinite(d.photon_radius))
            throw NoriException(NORI_ERR_INVALID, "photonmapper: photon_count and photon_radius must be positive");
        for (uint32_t i = 0; i < d.num_emitters; ++i)  // Emitter::samplePhoton (emitter.h) throws for the others
            if (d.emitters[i].type != NORI_EMITTER_AREA)
                throw NoriException(NORI_ERR_UNSUPPORTED, "photonmapper: photons from area lights only");
    }
    if (d.camera.camera_type < NORI_CAMERA_PERSPECTIVE || d.camera.camera_type > NORI_CAMERA_ADVANCED)
        throw NoriException(NORI_ERR_UNSUPPORTED, "unknown camera type");
    // the reference leaves Scene::m_medium uninitialised without a <medium>
    // (scene.h:141): rejected here, as in the oracle
    if (d.integrator == NORI_INTEGRATOR_VOLUMETRIC && !d.medium.present)
        throw NoriException(NORI_ERR_INVALID, "the volumetric integrator needs a <medium>");

    // Traversal strategy: scenes of at most kScanMaxPrims primitives are
    // intersected by a wave-uniform scan (scalar loads, no divergence), larger
    // ones by per-lane BVH traversal.  NORI_TRAVERSAL=bvh|scan overrides.
    const char *mode = std::getenv("NORI_TRAVERSAL");
    bool scan = off <= kScanMaxPrims;
    if (mode && std::string(mode) == "bvh") scan = false;
    if (mode && std::string(mode) == "scan") scan = true;
    DeviceBvh bvh;
    build_device_bvh(d, rmin, rmax, bvh);
    c.bvh_depth = bvh.depth;
    c.bvh_nodes = bvh.num_nodes;
    // traversal stack (bvh_stack_for); NORI_BVH_STACK = 8, 16 or 32 forces it (tuning)
    if (const char *e = std::getenv("NORI_BVH_STACK")) {
        const int v = std::atoi(e);
        if (v == 8 || v == 16 || v == 32) c.stack_forced = v;
    }
    c.stack = bvh_stack_for(bvh.depth, c.stack_forced);
    if (scan) c.stack = 0;
    ScanList scan_list;
    if (scan) scan_list = build_scan_list(bvh, off);
    const std::vector<float> &prim_list = scan ? scan_list.prims : bvh.prims;

    std::vector<float> pos(4 * (size_t)d.num_vertices), nrm(4 * (size_t)d.num_vertices);
    for (uint32_t v = 0; v < d.num_vertices; ++v) {
        for (int k = 0; k < 3; ++k) {
            pos[4 * (size_t)v + k] = d.positions[3 * (size_t)v + k];
            nrm[4 * (size_t)v + k] = d.normals ? d.normals[3 * (size_t)v + k] : 0.0f;
        }
        // texture coordinates ride in the w lanes (u with the position, v with the normal)
        pos[4 * (size_t)v + 3] = d.uvs ? d.uvs[2 * (size_t)v] : 0.0f;
        nrm[4 * (size_t)v + 3] = d.uvs ? d.uvs[2 * (size_t)v + 1] : 0.0f;
    }
    if (pos.empty()) pos.assign(4, 0.0f), nrm.assign(4, 0.0f);
    if (cdf.empty()) cdf.assign(1, 0.0f);
    c.nodes.upload(bvh.nodes);
    c.prims.upload(prim_list);
    if (!scan_list.plane_c.empty()) c.plane_c.upload(scan_list.plane_c);
    if (!scan_list.plane_f.empty()) c.plane_f.upload(scan_list.plane_f);
    c.tri_vidx.upload(tri_vidx);
    c.pos.upload(pos);
    c.nrm.upload(nrm);
    c.prim_shape.upload(prim_shape);
    c.shapes.upload(shapes);
    c.bsdfs.upload(bsdfs);
    c.emitters.upload(emitters);
    c.cdf.upload(cdf);
    if (env.empty()) env.assign(4, 0.0f);
    c.env.upload(env);
    c.scene_bytes = c.nodes.bytes + c.prims.bytes;
    // nori_gpu_update_vertices (BVH contexts): the order in which a refit recomputes the boxes
    c.hshapes = shapes;
    c.emitter_meshes = std::move(emitter_meshes);
    c.num_vertices = d.num_vertices;
    if (!scan) {
        c.refit = build_refit_plan(bvh);
        c.refit_slots.upload(c.refit.slots);
    }
    // small-scene blob (staged into LDS by the tail finisher)
    std::vector<char> blob;
    uint32_t offs[10] = {0};
    auto put = [&](int k, const void *p, size_t n) {
        while (blob.size() % 16) blob.push_back(0);
        offs[k] = (uint32_t)blob.size();
        const char *b = static_cast<const char *>(p);
        blob.insert(blob.end(), b, b + n);
    };
    put(0, prim_list.data(), prim_list.size() * 4);
    put(1, tri_vidx.data(), tri_vidx.size() * 4);
    put(2, pos.data(), pos.size() * 4);
    put(3, nrm.data(), nrm.size() * 4);
    put(4, prim_shape.data(), prim_shape.size() * 4);
    put(5, shapes.data(), shapes.size() * sizeof(DevShape));
    put(6, bsdfs.data(), bsdfs.size() * sizeof(DevBsdf));
    put(7, emitters.data(), emitters.size() * sizeof(DevEmitter));
    put(8, cdf.data(), cdf.size() * 4);
    put(9, bvh.nodes.data(), bvh.nodes.size() * 4);
    while (blob.size() % 16) blob.push_back(0);
    const bool use_blob = c.stack == 0 && blob.size() <= kBlobMaxBytes;
    if (use_blob) c.blob.upload(blob);

    DevScene &S = c.S;
    S.nodes = c.nodes.as<float4>();
    S.prims = c.prims.as<float4>();
    S.tri_vidx = c.tri_vidx.as<uint32_t>();
    S.pos = c.pos.as<float4>();
    S.nrm = c.nrm.as<float4>();
    S.prim_shape = c.prim_shape.as<uint32_t>();
    S.shapes = c.shapes.as<DevShape>();
    S.bsdfs = c.bsdfs.as<DevBsdf>();
    S.emitters = c.emitters.as<DevEmitter>();
    S.cdf = c.cdf.as<float>();
    S.env = c.env.as<float>();
    S.num_emitters = d.num_emitters;
    S.num_nodes = bvh.num_nodes;
    S.num_prims = (uint32_t)(prim_list.size() / 12);
    S.num_scan_tris = scan_list.tris;
    S.num_scan_real = scan_list.real;
    S.plane_c = scan_list.plane_c.empty() ? nullptr : c.plane_c.as<float>();
    S.plane_f = scan_list.plane_f.empty() ? nullptr : c.plane_f.as<float4>();
    for (int a = 0; a < 3; ++a) S.plane_end[a] = scan_list.plane_end[a];
    {
        const char *e = std::getenv("NORI_CAMERA_CULL");  // A/B and verification: 0 = no in-plane filter
        S.camera_cull = !(e && e[0] == '0');
        const char *t = std::getenv("NORI_TRACE_CULL");  // trace API: 0, 1 (default) or 2 (needs plane pairs)
        S.trace_cull = t ? std::atoi(t) : 1;
        if (S.trace_cull < 0 || S.trace_cull > 2 || (S.trace_cull == 2 && !S.plane_f)) S.trace_cull = 1;
    }
    const ScanRtcScene sc = rtc_scene_of(scan_list);  // for both hipRTC builds below
    if (scan && scan_list.prims.size() / 12 <= 2 * kScanMaxPrims) {  // the scan kernels compiled for this scene's scan list (rtc.hip); else the generic ones
        std::string why;
        if (!scan_rtc_build(sc, c.device, S.trace_cull, c.rtc, why) && debug_log())
            std::fprintf(stderr, "[nori] generic scan kernels: %s\n", why.c_str());
    }
    for (int k = 0; k < 3; ++k) S.root_min[k] = rmin[k], S.root_max[k] = rmax[k];
    S.blob = use_blob ? c.blob.as<float4>() : nullptr;
    S.blob_bytes = use_blob ? (uint32_t)blob.size() : 0u;
    S.off_prims = offs[0];
    S.off_vidx = offs[1];
    S.off_pos = offs[2];
    S.off_nrm = offs[3];
    S.off_pshape = offs[4];
    S.off_shapes = offs[5];
    S.off_bsdfs = offs[6];
    S.off_emitters = offs[7];
    S.off_cdf = offs[8];
    S.off_nodes = offs[9];
    const nori_camera_desc &cam = d.camera;
    c.cam = cam;
    if (cam.width <= 0 || cam.height <= 0) throw NoriException(NORI_ERR_INVALID, "bad output size");
    S.W = cam.width;
    S.H = cam.height;
    S.invW = 1.0f / (float)cam.width;
    S.invH = 1.0f / (float)cam.height;
    std::memcpy(S.s2c, cam.sample_to_camera, sizeof(S.s2c));
    std::memcpy(S.c2w, cam.camera_to_world, sizeof(S.c2w));
    {  // perspective.cpp:104: Eigen's (c2w * (0,0,0,1)).hnormalized(), column order
        const float *c = S.c2w;
        const float w = ((c[12] * 0.0f + c[13] * 0.0f) + c[14] * 0.0f) + c[15];
        S.cam_o[0] = (((c[0] * 0.0f + c[1] * 0.0f) + c[2] * 0.0f) + c[3]) / w;
        S.cam_o[1] = (((c[4] * 0.0f + c[5] * 0.0f) + c[6] * 0.0f) + c[7]) / w;
        S.cam_o[2] = (((c[8] * 0.0f + c[9] * 0.0f) + c[10] * 0.0f) + c[11]) / w;
    }
    S.near_clip = cam.near_clip;
    S.far_clip = cam.far_clip;
    S.cam_type = cam.camera_type;
    S.lens_radius = cam.lens_radius;
    S.focal = cam.focal_distance;
    S.distortion[0] = cam.distortion[0];
    S.distortion[1] = cam.distortion[1];
    for (int k = 0; k < 3; ++k) S.chromatic[k] = cam.camera_type == NORI_CAMERA_ADVANCED ? cam.chromatic[k] : 0.0f;
    S.chroma = S.chromatic[0] != 0.0f || S.chromatic[1] != 0.0f || S.chromatic[2] != 0.0f;
    S.basic = basic_scene(d) ? 1 : 0;
    {
        // shadow rays traced inside k_shade (scan-mode scenes): on by default
        // for the basic-plugin kernels (C2 +3-7 %, its 64-spp share +3 %), off
        // for the full ones (C4 -5.7 %, C5 -4.3 %: the full k_shade holds 90-96
        // VGPRs, and the queue's shadow kernel is the scene-specialised one).
        // NORI_NEE_INLINE=0 / 1 forces it off / on for scan-mode scenes whose
        // shade kernel carries it (the basic ones; kernels.h kNeeFull).
        const char *n = std::getenv("NORI_NEE_INLINE");
        S.nee_inline = c.stack == 0 && (n ? n[0] == '1' : S.basic != 0) && (S.basic != 0 || kNeeFull);
        // ... and each vertex's extension ray (k_shade's closest-hit scan in
        // place of the extension launch and the hit's round trip through
        // memory): scan-mode scenes with the basic plugins and the inline
        // shadow rays.  NORI_EXT_INLINE=0 / 1 forces it off / on there.
        const char *x = std::getenv("NORI_EXT_INLINE");
        S.ext_inline = c.stack == 0 && S.basic != 0 && S.nee_inline != 0 && (x ? x[0] == '1' : true);
    }
    {
        // one launch for an iteration's extension and shadow queues: on for
        // the BVH walks (C3 +10 %) and the basic scan kernels that keep the
        // queue; the full-plugin scan scenes run faster with two launches
        // (C4 3942 -> 3957, C5 4217 -> 4288 Msamples/s, 3 interleaved reps,
        // tools/gpu_fuse_ab.sh).  NORI_TRACE_FUSE=0 / 1 forces it.
        const char *f = std::getenv("NORI_TRACE_FUSE");
        c.fuse_trace = f ? f[0] != '0' : !(c.stack == 0 && S.basic == 0);
    }
    S.W_max = cam.width > cam.height ? cam.width : cam.height;
    S.av_length = d.av_length;
    filter_table(cam, S.filter);
    S.filter_radius = cam.filter_radius;
    S.lookup = NORI_FILTER_RESOLUTION / cam.filter_radius;
    S.border = film_border(cam);
    if (S.border > 4) throw NoriException(NORI_ERR_UNSUPPORTED, "filter radius above 4.5 pixels");
    S.jit_lk = jit_code_lookup(S.filter_radius, S.lookup);
    S.integrator = d.integrator;
    if (shade_rtc_scene(d, scan, scan_list.prims.size() / 12)) {  // k_shade compiled for this scene (after the scan program)
        std::string why;
        if (!shade_rtc_build(sc, c.device, shade_integrator(S.integrator), shade_lds_bytes(S.blob_bytes) != 0,
                             c.shade_rtc, why) && debug_log())
            std::fprintf(stderr, "[nori] ahead-of-time shade kernel: %s\n", why.c_str());
        if (debug_log() && scene_blob_bytes(d, prim_list.size(), bvh.nodes.size()) != blob.size())
            std::fprintf(stderr, "[nori] scene_blob_bytes %zu != blob %zu\n",
                         scene_blob_bytes(d, prim_list.size(), bvh.nodes.size()), blob.size());
    }
    {  // deviation D10 (shading.h skip_nee); NORI_DISCRETE_NEE=1 keeps the full NEE everywhere
        bool env = false;
        for (uint32_t i = 0; i < d.num_emitters; ++i) env = env || d.emitters[i].type == NORI_EMITTER_ENVMAP;
        const char *e = std::getenv("NORI_DISCRETE_NEE");
        S.skip_discrete_nee = !env && !(e && e[0] == '1');
    }
    S.has_medium = d.medium.present;
    if (S.has_medium) {  // medium.cpp:10-20
        const nori_medium_desc &m = d.medium;
        for (int k = 0; k < 3; ++k) {
            S.mbox_min[k] = m.box_min[k];
            S.mbox_max[k] = m.box_max[k];
            S.sigma_t[k] = m.sigma_a[k] + m.sigma_s[k];
            S.albedo[k] = m.sigma_s[k] / S.sigma_t[k];
        }
    }
}

// PhotonMapper::preprocess (photonmapper.cpp:41-117): photons are traced on
// the device in emission order batches (k_photons count pass) until the
// stored count reaches photonCount, then the emitted photons that contribute
// are traced again writing their photons (store pass), and the host stores
// them as the reference's PhotonData and builds the hash grid.
void photon_preprocess(nori_gpu_ctx &c, const nori_scene_desc &d) {
    const uint64_t N = d.photon_count;
    const uint32_t batch = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(N, 1u << 20), 1u << 24);
    DevBuf cnt;
    cnt.ensure(4 * (size_t)batch);
    std::vector<uint32_t> hc(batch);
    std::vector<uint64_t> pre;  // photons stored before each emitted photon
    uint64_t total = 0, e0 = 0;
    while (total < N) {
        if (e0 >= 64 * N + batch)  // the reference would loop forever
            throw NoriException(NORI_ERR_INVALID, "photonmapper: photons do not reach a diffuse surface");
        HIP_TRY(launch_photons(c.S, e0, batch, cnt.as<uint32_t>(), nullptr, 0, nullptr, c.stack, c.stream));
        HIP_TRY(hipMemcpyAsync(hc.data(), cnt.p, 4 * (size_t)batch, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
        for (uint32_t i = 0; i < batch && total < N; ++i) {
            pre.push_back(total);
            total += hc[i];
        }
        e0 += batch;
    }
    DevBuf dpre, out;
    dpre.upload(pre);
    out.ensure(48 * (size_t)N);
    // all-ones (NaN) first: a slot the store pass leaves unwritten keeps a NaN
    // in its zero pad word and is caught below instead of entering the map
    HIP_TRY(hipMemsetAsync(out.p, 0xFF, 48 * (size_t)N, c.stream));
    HIP_TRY(launch_photons(c.S, 0, (uint32_t)pre.size(), nullptr, dpre.as<uint64_t>(), N, out.as<float4>(), c.stack,
                           c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    std::vector<float> raw(12 * (size_t)N), ph, tab;
    HIP_TRY(hipMemcpy(raw.data(), out.p, 48 * (size_t)N, hipMemcpyDeviceToHost));
    // the store pass must reproduce the count pass photon for photon
    // (position, 0, direction, 0, power, 0 per slot)
    for (size_t i = 0; i < (size_t)N; ++i)
        if (!(raw[12 * i + 3] == 0.0f && raw[12 * i + 7] == 0.0f && raw[12 * i + 11] == 0.0f))
            throw NoriException(NORI_ERR_INVALID, "photonmapper: the store pass left photon slot " + std::to_string(i) +
                                                      " unwritten (count and store passes disagree)");
    std::vector<uint32_t> start, rgbe;
    uint32_t mask = 0;
    build_photon_map(raw, (uint32_t)N, d.photon_radius, ph, rgbe, tab, start, mask);
    c.ph.upload(ph);
    c.ph_rgbe.upload(rgbe);
    c.ph_tab.upload(tab);
    c.ph_start.upload(start);
    c.S.ph_rgbe = c.ph_rgbe.as<uint32_t>();
    c.S.ph_tab = c.ph_tab.as<float>();
    const float r = d.photon_radius;
    c.S.ph = c.ph.as<float4>();
    c.S.ph_start = c.ph_start.as<uint32_t>();
    c.S.ph_mask = mask;
    c.S.ph_inv_cell = 1.0f / r;
    c.S.ph_r2 = r * r;                                 // kdtree.h:266
    c.S.ph_norm = (r * r) * (float)d.photon_count;     // photonmapper.cpp:177
}

}  // namespace
}  // namespace nori

extern "C" {

int nori_scene_scan_rtc(const nori_scene_desc *d, const char *arch, size_t *code_bytes, double *ms) {
    return guarded([&] {
        if (!d || !arch || !code_bytes || !ms) return fail(NORI_ERR_INVALID, "null argument");
        if (d->abi_version != NORI_GPU_ABI_VERSION) return fail(NORI_ERR_INVALID, "ABI version mismatch");
        float rmin[3], rmax[3];
        scene_root_box(*d, rmin, rmax);
        DeviceBvh bvh;
        build_device_bvh(*d, rmin, rmax, bvh);
        const uint32_t n = (uint32_t)(bvh.prims.size() / 12);
        *code_bytes = 0;
        *ms = 0.0;
        if (n > kScanMaxPrims) return NORI_OK;  // a BVH scene: nothing to specialise
        const ScanList L = build_scan_list(bvh, n);
        const ScanRtcScene sc = rtc_scene_of(L);
        std::vector<char> code;
        bool cached = false;
        std::string why;
        if (!rtc_compile(sc, arch, 1, code, *ms, cached, why)) return fail(NORI_ERR_UNSUPPORTED, why);
        *code_bytes = code.size();
        return NORI_OK;
    });
}
int nori_scene_shade_rtc(const nori_scene_desc *d, const char *arch, size_t *code_bytes, double *ms) {
    return guarded([&] {
        if (!d || !arch || !code_bytes || !ms) return fail(NORI_ERR_INVALID, "null argument");
        if (d->abi_version != NORI_GPU_ABI_VERSION) return fail(NORI_ERR_INVALID, "ABI version mismatch");
        float rmin[3], rmax[3];
        scene_root_box(*d, rmin, rmax);
        DeviceBvh bvh;
        build_device_bvh(*d, rmin, rmax, bvh);
        const uint32_t n = (uint32_t)(bvh.prims.size() / 12);
        *code_bytes = 0;
        *ms = 0.0;
        // (the traversal as nori_gpu_create chooses it, NORI_TRAVERSAL included)
        const char *mode = std::getenv("NORI_TRAVERSAL");
        bool scan = n <= kScanMaxPrims;
        if (mode && std::string(mode) == "bvh") scan = false;
        if (mode && std::string(mode) == "scan") scan = true;
        if (!scan) return NORI_OK;
        const ScanList L = build_scan_list(bvh, n);
        if (!shade_rtc_scene(*d, scan, L.prims.size() / 12)) return NORI_OK;  // the ahead-of-time kernel serves it
        const ScanRtcScene sc = rtc_scene_of(L);
        const size_t blob = scene_blob_bytes(*d, L.prims.size(), bvh.nodes.size());
        const bool lds = blob <= kBlobMaxBytes && shade_lds_bytes((uint32_t)blob) != 0;
        std::vector<char> code;
        bool cached = false;
        std::string why;
        if (!rtc_compile_shade(sc, arch, shade_integrator(d->integrator), lds, code, *ms, cached, why))
            return fail(NORI_ERR_UNSUPPORTED, why);
        *code_bytes = code.size();
        return NORI_OK;
    });
}
int nori_gpu_shade_rtc_info(nori_gpu_ctx *c, int *active, int *cached, double *ms, size_t *code_bytes) {
    return guarded([&] {
        if (!c) return fail(NORI_ERR_INVALID, "null argument");
        if (active) *active = c->shade_rtc.shade ? 1 : 0;
        if (cached) *cached = c->shade_rtc.cached ? 1 : 0;
        if (ms) *ms = c->shade_rtc.compile_ms;
        if (code_bytes) *code_bytes = c->shade_rtc.code_bytes;
        return NORI_OK;
    });
}

int nori_gpu_device_count(int *count) {
    return guarded([&] {
        if (!count) return fail(NORI_ERR_INVALID, "null argument");
        int n = 0;
        hipError_t e = hipGetDeviceCount(&n);
        *count = e == hipSuccess ? n : 0;
        return NORI_OK;
    });
}

int nori_gpu_create(const nori_scene_desc *d, int device, nori_gpu_ctx **out) {
    return guarded([&] {
        if (!d || !out) return fail(NORI_ERR_INVALID, "null argument");
        if (d->abi_version != NORI_GPU_ABI_VERSION) return fail(NORI_ERR_INVALID, "scene desc ABI version mismatch");
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(NORI_ERR_HIP, "no HIP device available");
        if (device < 0 || device >= n) return fail(NORI_ERR_INVALID, "device index out of range");
        HIP_TRY(hipSetDevice(device));
        std::unique_ptr<nori_gpu_ctx> c(new nori_gpu_ctx);
        c->device = device;
        c->spp = d->sample_count ? d->sample_count : 1;
        c->scene_spp = d->sample_count;
        if (const char *e = std::getenv("NORI_FINISH_FIRST"); e && e[0] == '0') c->finish_first = false;
        HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
        for (int h = 1; h < kMaxParts; ++h) {
            HIP_TRY(hipStreamCreateWithFlags(&c->parts[h], hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&c->joins[h], hipEventDisableTiming));
        }
        HIP_TRY(hipEventCreateWithFlags(&c->fork, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&c->join, hipEventDisableTiming));
        upload_scene(*c, *d);
        if (d->integrator == NORI_INTEGRATOR_PHOTONMAPPER) photon_preprocess(*c, *d);
        *out = c.release();
        return NORI_OK;
    });
}

int nori_gpu_cancel(nori_gpu_ctx *c) {
    if (!c) return fail(NORI_ERR_INVALID, "null argument");
    c->cancel = 1;
    return NORI_OK;
}
float nori_gpu_progress(const nori_gpu_ctx *c) { return c ? c->progress.load() : 0.0f; }

void nori_gpu_destroy(nori_gpu_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;
}

}  // extern "C"
