// upload.hip -- nori_gpu_create: a scene's plan (scene_plan.h) becomes a
// context's device buffers, DevScene and scene-specific kernels (rtc.hip).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "ctx.h"
#include "scene_plan.h"

namespace nori {

static_assert(kScanListGroup == kScanGroup, "scene_prep.h and dev_scene.h disagree on NORI_SCAN_GROUP");
// scene_plan.h restates what it cannot include
static_assert(kPlanTraceSpill == kTraceSpill && plan_lds_entries(8) == stack_lds_entries(8) &&
                  plan_lds_entries(16) == stack_lds_entries(16) && plan_lds_entries(32) == stack_lds_entries(32),
              "scene_plan.h and kernels.h disagree on the traversal stack");
static_assert(kPlanShadeLdsMax == kShadeLdsMax && kPlanNeeFull == kNeeFull,
              "scene_plan.h and kernel_config.h disagree on NORI_SHADE_LDS_MAX or NORI_NEE_FULL");
static_assert(plan_shade_integrator(NORI_INTEGRATOR_PATH_MATS) == shade_integrator(NORI_INTEGRATOR_PATH_MATS) &&
                  plan_shade_integrator(NORI_INTEGRATOR_PATH_MIS) == shade_integrator(NORI_INTEGRATOR_PATH_MIS) &&
                  plan_shade_integrator(NORI_INTEGRATOR_VOLUMETRIC) == shade_integrator(NORI_INTEGRATOR_VOLUMETRIC) &&
                  plan_shade_integrator(NORI_INTEGRATOR_DIRECT_MIS) == shade_integrator(NORI_INTEGRATOR_DIRECT_MIS),
              "scene_plan.h and kernels.h disagree on k_shade's integrators");

namespace {

const char *env_text(const char *name) { return std::getenv(name); }

// The tables' device pointers, counts and blob offsets
void fill_tables(nori_gpu_ctx &c, const ScenePlan &p, const uint32_t offs[10]) {
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
    S.num_emitters = (uint32_t)p.emitters.size();
    S.num_nodes = p.tree.bvh.num_nodes;
    S.num_prims = (uint32_t)(p.prim_list().size() / 12);
    S.num_scan_tris = p.scan_list.tris;
    S.num_scan_real = p.scan_list.real;
    S.plane_c = p.scan_list.plane_c.empty() ? nullptr : c.plane_c.as<float>();
    S.plane_f = p.scan_list.plane_f.empty() ? nullptr : c.plane_f.as<float4>();
    for (int a = 0; a < 3; ++a) S.plane_end[a] = p.scan_list.plane_end[a];
    for (int k = 0; k < 3; ++k) S.root_min[k] = p.tree.rmin[k], S.root_max[k] = p.tree.rmax[k];
    S.blob = p.use_blob ? c.blob.as<float4>() : nullptr;
    S.blob_bytes = p.use_blob ? (uint32_t)p.blob_bytes : 0u;
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
}

void fill_camera(DevScene &S, const nori_camera_desc &cam, const ScenePlan &p) {
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
    S.chroma = p.chroma;
    S.W_max = cam.width > cam.height ? cam.width : cam.height;
    filter_table(cam, S.filter);
    S.filter_radius = cam.filter_radius;
    S.lookup = NORI_FILTER_RESOLUTION / cam.filter_radius;
    S.border = p.border;
    S.jit_lk = p.jit_lk;
}

// The plan's decisions, the integrator and the medium
void fill_settings(DevScene &S, const nori_scene_desc &d, const ScenePlan &p) {
    S.camera_cull = p.camera_cull;
    S.trace_cull = p.trace_cull;
    S.basic = p.basic ? 1 : 0;
    S.nee_inline = p.nee_inline;
    S.ext_inline = p.ext_inline;
    S.av_length = d.av_length;
    S.integrator = d.integrator;
    S.skip_discrete_nee = p.skip_discrete_nee;
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

// The texels, then the records with their image pointers, then every other table
void upload_tables(nori_gpu_ctx &c, ScenePlan &p, uint32_t offs[10]) {
    c.tex.upload(p.tex);
    for (size_t s = 0; s < p.shapes.size(); ++s)
        if (p.shape_tex[s] != ScenePlan::kNoImage) p.shapes[s].nmap = c.tex.as<uint32_t>() + p.shape_tex[s];
    for (size_t i = 0; i < p.bsdfs.size(); ++i)
        if (p.bsdf_tex[i] != ScenePlan::kNoImage) p.bsdfs[i].img = c.tex.as<uint32_t>() + p.bsdf_tex[i];
    c.nodes.upload(p.tree.bvh.nodes);
    c.prims.upload(p.prim_list());
    if (!p.scan_list.plane_c.empty()) c.plane_c.upload(p.scan_list.plane_c);
    if (!p.scan_list.plane_f.empty()) c.plane_f.upload(p.scan_list.plane_f);
    c.tri_vidx.upload(p.tri_vidx);
    c.pos.upload(p.pos);
    c.nrm.upload(p.nrm);
    c.prim_shape.upload(p.prim_shape);
    c.shapes.upload(p.shapes);
    c.bsdfs.upload(p.bsdfs);
    c.emitters.upload(p.emitters);
    c.cdf.upload(p.cdf);
    c.env.upload(p.env);
    if (!p.scan) c.refit_slots.upload(p.refit.slots);
    // small-scene blob (staged into LDS by the tail finisher)
    if (p.use_blob) {
        std::vector<char> blob;
        pack_blob(p, blob, offs);
        c.blob.upload(blob);
    } else {
        blob_layout(p, offs);
    }
}

// The hipRTC programs the plan asks for: the scan kernels, then k_shade (rtc.hip)
void build_programs(nori_gpu_ctx &c, const ScenePlan &p) {
    const ScanRtcScene sc = scan_rtc_scene(p.scan_list);
    std::string why;
    if (p.build_scan && !scan_rtc_build(sc, c.device, p.trace_cull, c.rtc, why) && debug_log())
        std::fprintf(stderr, "[nori] generic scan kernels: %s\n", why.c_str());
    if (p.build_shade && !shade_rtc_build(sc, c.device, p.shade_integrator, p.shade_lds, c.shade_rtc, why) && debug_log())
        std::fprintf(stderr, "[nori] ahead-of-time shade kernel: %s\n", why.c_str());
}

void upload_scene(nori_gpu_ctx &c, const nori_scene_desc &d, ScenePlan &p) {
    uint32_t offs[10] = {0};
    upload_tables(c, p, offs);
    build_programs(c, p);
    c.num_prims = p.num_prims;
    c.bvh_depth = p.tree.bvh.depth;
    c.bvh_nodes = p.tree.bvh.num_nodes;
    c.stack = p.stack;
    c.stack_forced = p.stack_forced;
    c.fuse_trace = p.fuse_trace;
    c.finish_first = p.finish_first;
    c.scene_bytes = c.nodes.bytes + c.prims.bytes;
    c.num_vertices = d.num_vertices;
    c.num_bsdfs = d.num_bsdfs;
    c.cam = d.camera;
    fill_tables(c, p, offs);
    fill_camera(c.S, d.camera, p);
    fill_settings(c.S, d, p);
    // nori_gpu_update_vertices: the shapes as uploaded, the emitter meshes, the refit schedule (BVH contexts)
    c.hshapes = std::move(p.shapes);
    c.emitter_meshes = std::move(p.emitter_meshes);
    c.refit = std::move(p.refit);
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
        const SceneTree tree = build_scene_tree(*d);
        *code_bytes = 0;
        *ms = 0.0;
        if (!scan_mode(tree.n, SceneKnobs{})) return NORI_OK;  // a BVH scene by its size: nothing to specialise
        const ScanList L = build_scan_list(tree.bvh, tree.n);
        std::vector<char> code;
        bool cached = false;
        std::string why;
        if (!rtc_compile(scan_rtc_scene(L), arch, 1, code, *ms, cached, why)) return fail(NORI_ERR_UNSUPPORTED, why);
        *code_bytes = code.size();
        return NORI_OK;
    });
}
int nori_scene_shade_rtc(const nori_scene_desc *d, const char *arch, size_t *code_bytes, double *ms) {
    return guarded([&] {
        if (!d || !arch || !code_bytes || !ms) return fail(NORI_ERR_INVALID, "null argument");
        if (d->abi_version != NORI_GPU_ABI_VERSION) return fail(NORI_ERR_INVALID, "ABI version mismatch");
        *code_bytes = 0;
        *ms = 0.0;
        // (the program as nori_gpu_create builds it, the knobs included)
        const ScenePlan plan = plan_scene(*d, scene_knobs(env_text));
        if (!plan.build_shade) return NORI_OK;  // a BVH scene, or the ahead-of-time kernel serves it
        std::vector<char> code;
        bool cached = false;
        std::string why;
        if (!rtc_compile_shade(scan_rtc_scene(plan.scan_list), arch, plan.shade_integrator, plan.shade_lds, code, *ms,
                               cached, why))
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
        ScenePlan plan = plan_scene(*d, scene_knobs(env_text));  // every refusal of the description, before anything is created
        std::unique_ptr<nori_gpu_ctx> c(new nori_gpu_ctx);
        c->device = device;
        c->spp = d->sample_count ? d->sample_count : 1;
        c->scene_spp = d->sample_count;
        HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
        for (int h = 1; h < kMaxParts; ++h) {
            HIP_TRY(hipStreamCreateWithFlags(&c->parts[h], hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&c->joins[h], hipEventDisableTiming));
        }
        HIP_TRY(hipEventCreateWithFlags(&c->fork, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&c->join, hipEventDisableTiming));
        upload_scene(*c, *d, plan);
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
