// Stand-alone run of the scene plan (nori-ray-tracer_amd/csrc/scene_plan.h),
// built with the address and undefined-behaviour sanitizers by
// tests/test_scene_plan.py.  Arguments: six scene XMLs -- the Cornell box
// (basic plugins, scan mode), two more basic scan scenes, an environment-map
// scene (full plugins, scan mode), an image-textured one (full plugins, above
// kScanMaxPrims: BVH mode) and a microfacet mesh in BVH mode (the basic plugins
// in BVH mode: the Cornell box under NORI_TRAVERSAL=bvh).  It checks every refusal of plan_scene and
// bvh_stack_for's table, the knob parsing and the decisions that follow from
// it, and the blob layout, and prints one FNV-1a hash per plan table and
// decision of every scene as "<name> <hash>" (the test compares them with
// those of nori_gpu_create before the plan existed), then "ok".
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "scene_plan.h"

using namespace nori;

static int g_failed = 0;
static std::string g_what;  // what the failing check was about
#define CHECK(cond)                                                               \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::printf("FAILED %s:%d: %s [%s]\n", __FILE__, __LINE__, #cond, g_what.c_str()); \
            ++g_failed;                                                           \
        }                                                                         \
    } while (0)
static void failed(const char *how) {
    std::printf("FAILED: %s [%s]\n", how, g_what.c_str());
    ++g_failed;
}

// ---- the environment the knobs are read from
static std::map<std::string, std::string> g_env;
static const char *env_text(const char *name) {
    auto it = g_env.find(name);
    return it == g_env.end() ? nullptr : it->second.c_str();
}
static SceneKnobs knobs_of(std::map<std::string, std::string> env) {
    g_env = std::move(env);
    return scene_knobs(env_text);
}

// ---- hashes
struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void bytes(const void *p, size_t n) {
        const unsigned char *b = static_cast<const unsigned char *>(p);
        for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    }
    template <class T> void vec(const std::vector<T> &v) {
        if (!v.empty()) bytes(v.data(), v.size() * sizeof(T));
    }
    template <class T> void val(const T &v) { bytes(&v, sizeof(T)); }
};
static void say(const char *name, const Fnv &f) { std::printf("%s %016llx\n", name, (unsigned long long)f.h); }
template <class T> static void say_vec(const char *name, const std::vector<T> &v) {
    Fnv f;
    f.vec(v);
    say(name, f);
}
static void say_int(const char *name, int64_t v) {
    Fnv f;
    f.val(v);
    say(name, f);
}

static void print_hashes(const char *path, const ScenePlan &p) {
    std::printf("scene %s\n", path);
    say_vec("tex", p.tex);
    Fnv io;
    for (size_t o : p.img_off) io.val((uint64_t)o);
    say("img_off", io);
    for (const DevShape &s : p.shapes) CHECK(s.nmap == nullptr);
    for (const DevBsdf &b : p.bsdfs) CHECK(b.img == nullptr);
    say_vec("shapes", p.shapes);
    say_vec("bsdfs", p.bsdfs);
    say_vec("emitters", p.emitters);
    say_vec("prim_shape", p.prim_shape);
    say_vec("tri_vidx", p.tri_vidx);
    say_vec("cdf", p.cdf);
    say_vec("env", p.env);
    say_vec("pos", p.pos);
    say_vec("nrm", p.nrm);
    say_vec("nodes", p.tree.bvh.nodes);
    say_vec("prims", p.prim_list());
    say_vec("plane_c", p.scan_list.plane_c);
    say_vec("plane_f", p.scan_list.plane_f);
    Fnv si;
    si.val(p.scan_list.plane_end);
    si.val(p.scan_list.tris);
    si.val(p.scan_list.real);
    si.val(p.scan_list.fast_max);
    say("scan_info", si);
    say_vec("refit_slots", p.refit.slots);
    say_vec("refit_levels", p.refit.level_begin);
    Fnv em;
    for (const EmitterMesh &m : p.emitter_meshes) {
        em.val(m.shape), em.val(m.cdf_offset), em.val(m.vtx_first), em.val(m.vtx_count);
        em.vec(m.tri);
    }
    say("emitter_meshes", em);
    Fnv box;
    box.val(p.tree.rmin), box.val(p.tree.rmax);
    say("root_box", box);
    Fnv ti;
    ti.val(p.tree.bvh.num_nodes), ti.val(p.tree.bvh.depth), ti.val(p.num_prims);
    say("tree_info", ti);
    uint32_t offs[10];
    CHECK(blob_layout(p, offs) == p.blob_bytes);
    Fnv bo;
    bo.val(offs);
    say("blob_offsets", bo);
    say_int("blob_bytes", (int64_t)p.blob_bytes);
    say_int("scan", p.scan), say_int("stack", p.stack), say_int("stack_forced", p.stack_forced);
    say_int("trace_cull", p.trace_cull), say_int("camera_cull", p.camera_cull), say_int("basic", p.basic);
    say_int("chroma", p.chroma), say_int("nee_inline", p.nee_inline), say_int("ext_inline", p.ext_inline);
    say_int("fuse_trace", p.fuse_trace), say_int("finish_first", p.finish_first);
    say_int("skip_discrete_nee", p.skip_discrete_nee), say_int("border", p.border), say_int("jit_lk", p.jit_lk);
    say_int("use_blob", p.use_blob), say_int("build_scan", p.build_scan), say_int("build_shade", p.build_shade);
    say_int("shade_integrator", p.shade_integrator), say_int("shade_lds", p.shade_lds);
}

// ---- 1. refusals
// A description whose arrays can be written: copies of the Cornell box's
struct Mut {
    nori_scene_desc d;
    std::vector<nori_shape_desc> shapes;
    std::vector<nori_bsdf_desc> bsdfs;
    std::vector<nori_emitter_desc> emitters;
    std::vector<uint32_t> indices;
    std::vector<nori_image_desc> images;
    uint8_t texel[3] = {1, 2, 3};
    explicit Mut(const nori_scene_desc &src)
        : d(src), shapes(src.shapes, src.shapes + src.num_shapes), bsdfs(src.bsdfs, src.bsdfs + src.num_bsdfs),
          emitters(src.emitters, src.emitters + src.num_emitters), indices(src.indices, src.indices + 3 * (size_t)src.num_triangles),
          images(1, nori_image_desc{1, 1, NORI_WRAP_REPEAT, texel}) {}
    const nori_scene_desc &desc() {
        d.shapes = shapes.data(), d.num_shapes = (uint32_t)shapes.size();
        d.bsdfs = bsdfs.data(), d.num_bsdfs = (uint32_t)bsdfs.size();
        d.emitters = emitters.data(), d.num_emitters = (uint32_t)emitters.size();
        d.indices = indices.data();
        d.images = images.data(), d.num_images = (uint32_t)images.size();
        return d;
    }
};
static void accepted(const nori_scene_desc &good, const char *what, const std::function<void(Mut &)> &change) {
    g_what = what;
    Mut m(good);
    change(m);
    try {
        plan_scene(m.desc(), SceneKnobs{});
    } catch (const NoriException &e) {
        g_what += std::string(": ") + e.what();
        failed("refused, should be accepted");
    }
}
static void refused(const nori_scene_desc &good, int code, const char *msg, const std::function<void(Mut &)> &breakit) {
    g_what = msg;
    Mut m(good);
    breakit(m);
    try {
        plan_scene(m.desc(), SceneKnobs{});
        failed("accepted, should be refused");
    } catch (const NoriException &e) {
        g_what += std::string(" / got: ") + e.what();
        CHECK(e.code == code && std::string(e.what()) == msg);
    }
}

static void check_refusals(const nori_scene_desc &g) {
    const int INV = NORI_ERR_INVALID, UNS = NORI_ERR_UNSUPPORTED;
    accepted(g, "the valid description, one unused image added", [](Mut &) {});
    refused(g, INV, "bad image description", [](Mut &m) { m.images[0].rgb = nullptr; });
    refused(g, INV, "bad image description", [](Mut &m) { m.images[0].width = 0; });
    refused(g, INV, "bad image description", [](Mut &m) { m.images[0].height = -1; });
    refused(g, INV, "bad image description", [](Mut &m) { m.images[0].wrap = 2; });
    refused(g, INV, "image index out of range", [](Mut &m) { m.shapes[0].normal_map = 1; });
    refused(g, INV, "image index out of range", [](Mut &m) {
        m.bsdfs[0].albedo_texture = NORI_TEXTURE_IMAGE, m.bsdfs[0].albedo_image = 1;
    });
    refused(g, INV, "shape without a valid bsdf", [](Mut &m) { m.shapes[0].bsdf = -1; });
    refused(g, INV, "shape without a valid bsdf", [](Mut &m) { m.shapes[0].bsdf = (int32_t)m.bsdfs.size(); });
    refused(g, INV, "mesh range outside the scene arrays", [](Mut &m) { m.shapes[0].tri_count = m.d.num_triangles + 1; });
    refused(g, INV, "mesh range outside the scene arrays", [](Mut &m) { m.shapes[0].tri_offset = 0xFFFFFFFFu; });
    refused(g, INV, "mesh range outside the scene arrays", [](Mut &m) { m.shapes[0].vtx_offset = m.d.num_vertices; });
    refused(g, INV, "vertex index out of range", [](Mut &m) { m.indices[3 * m.shapes[0].tri_offset + 1] = m.d.num_vertices; });
    refused(g, INV, "unknown shape type", [](Mut &m) { m.shapes[0].type = 2; });
    refused(g, INV, "ImageTexture albedo without an image", [](Mut &m) {
        m.bsdfs[0].albedo_texture = NORI_TEXTURE_IMAGE, m.bsdfs[0].albedo_image = -1;
    });
    refused(g, INV, "unknown albedo texture", [](Mut &m) { m.bsdfs[0].albedo_texture = 3; });
    refused(g, INV, "unknown bsdf type", [](Mut &m) { m.bsdfs[0].type = NORI_BSDF_DISNEY + 1; });
    refused(g, INV, "unknown bsdf type", [](Mut &m) { m.bsdfs[0].type = -1; });
    refused(g, UNS, "unknown emitter type", [](Mut &m) { m.emitters[0].type = 4; });
    refused(g, INV, "emitter without a shape", [](Mut &m) { m.emitters[0].shape = -1; });
    refused(g, INV, "emitter without a shape", [](Mut &m) { m.emitters[0].shape = (int32_t)m.shapes.size(); });
    accepted(g, "a point light needs no shape", [](Mut &m) { m.emitters[0].type = NORI_EMITTER_POINT, m.emitters[0].shape = -1; });
    refused(g, UNS, "unknown integrator", [](Mut &m) { m.d.integrator = NORI_INTEGRATOR_PHOTONMAPPER + 1; });
    refused(g, UNS, "unknown integrator", [](Mut &m) { m.d.integrator = -1; });
    auto no_emitter = [](Mut &m) {
        m.emitters.clear();
        for (auto &s : m.shapes) s.emitter = -1;
    };
    refused(g, INV, "the scene has no emitter", no_emitter);
    for (int exempt : {NORI_INTEGRATOR_NORMALS, NORI_INTEGRATOR_AV})
        accepted(g, "normals / av without an emitter", [&](Mut &m) { no_emitter(m), m.d.integrator = exempt; });
    auto photons = [](Mut &m) { m.d.integrator = NORI_INTEGRATOR_PHOTONMAPPER, m.d.photon_count = 100, m.d.photon_radius = 0.1f; };
    accepted(g, "a photon mapper with count and radius", photons);
    const char *pm = "photonmapper: photon_count and photon_radius must be positive";
    refused(g, INV, pm, [&](Mut &m) { photons(m), m.d.photon_count = 0; });
    refused(g, INV, pm, [&](Mut &m) { photons(m), m.d.photon_radius = 0.0f; });
    refused(g, INV, pm, [&](Mut &m) { photons(m), m.d.photon_radius = __builtin_inff(); });
    refused(g, UNS, "photonmapper: photons from area lights only",
            [&](Mut &m) { photons(m), m.emitters[0].type = NORI_EMITTER_POINT, m.emitters[0].shape = -1; });
    refused(g, UNS, "unknown camera type", [](Mut &m) { m.d.camera.camera_type = NORI_CAMERA_ADVANCED + 1; });
    refused(g, INV, "the volumetric integrator needs a <medium>",
            [](Mut &m) { m.d.integrator = NORI_INTEGRATOR_VOLUMETRIC, m.d.medium.present = 0; });
    refused(g, INV, "bad output size", [](Mut &m) { m.d.camera.width = 0; });
    refused(g, INV, "bad output size", [](Mut &m) { m.d.camera.height = -3; });
    accepted(g, "filter radius 4.5", [](Mut &m) { m.d.camera.filter_radius = 4.5f; });
    refused(g, UNS, "filter radius above 4.5 pixels", [](Mut &m) { m.d.camera.filter_radius = 4.51f; });
}

// bvh_stack_for: need = 3 * depth + 1 entries; a budget of s LDS words holds
// s / 2 (child, distance) pairs, and 64 more entries live in private memory.
static void check_stack_table() {
    g_what = "bvh_stack_for";
    auto thrown = [](uint32_t depth, int forced) {
        try {
            bvh_stack_for(depth, forced);
        } catch (const NoriException &e) {
            return e.code == NORI_ERR_UNSUPPORTED && std::string(e.what()) == "BVH too deep for the traversal stack";
        }
        return false;
    };
    CHECK(bvh_stack_for(0, 0) == 8 && bvh_stack_for(1, 0) == 8);     // need 1, 4 <= 4
    CHECK(bvh_stack_for(2, 0) == 16 && bvh_stack_for(23, 0) == 16);  // need 7 > 4 .. 70 <= 8 + 64
    CHECK(bvh_stack_for(24, 0) == 32 && bvh_stack_for(26, 0) == 32); // need 73 > 72 .. 79 <= 16 + 64
    CHECK(thrown(27, 0));                                            // need 82 > 80
    CHECK(bvh_stack_for(1, 8) == 8 && bvh_stack_for(22, 8) == 8 && thrown(23, 8));      // 67 <= 4 + 64 < 70
    CHECK(bvh_stack_for(1, 16) == 16 && bvh_stack_for(23, 16) == 16 && thrown(24, 16));
    CHECK(bvh_stack_for(1, 32) == 32 && bvh_stack_for(26, 32) == 32 && thrown(27, 32));
}

// ---- 2. knob parsing and the decisions
static void check_knob_parsing() {
    g_what = "scene_knobs";
    const SceneKnobs unset = knobs_of({});
    CHECK(unset.traversal == 0 && unset.stack_forced == 0 && unset.camera_cull && unset.trace_cull == 1);
    CHECK(unset.nee_inline == -1 && unset.ext_inline == -1 && unset.fuse_trace == -1);
    CHECK(!unset.discrete_nee && unset.finish_first);
    for (const char *v : {"0", "1", "junk", "", "01", "10"}) {  // (atoi gives 0, 1, 0, 0, 1, 10)
        g_what = std::string("scene_knobs, every knob = '") + v + "'";
        const SceneKnobs k = knobs_of({{"NORI_TRAVERSAL", v}, {"NORI_BVH_STACK", v}, {"NORI_CAMERA_CULL", v},
                                       {"NORI_TRACE_CULL", v}, {"NORI_NEE_INLINE", v}, {"NORI_EXT_INLINE", v},
                                       {"NORI_TRACE_FUSE", v}, {"NORI_DISCRETE_NEE", v}, {"NORI_FINISH_FIRST", v}});
        const bool lead0 = v[0] == '0', lead1 = v[0] == '1';
        CHECK(k.traversal == 0 && k.stack_forced == 0);
        CHECK(k.camera_cull == !lead0 && k.finish_first == !lead0 && k.fuse_trace == (lead0 ? 0 : 1));
        CHECK(k.nee_inline == (lead1 ? 1 : 0) && k.ext_inline == (lead1 ? 1 : 0) && k.discrete_nee == lead1);
        CHECK(k.trace_cull == (lead1 || std::string(v) == "01" ? 1 : 0));  // 10 is outside 0 .. 2: 1
    }
    g_what = "scene_knobs, NORI_TRACE_CULL";
    CHECK(knobs_of({{"NORI_TRACE_CULL", "junk"}}).trace_cull == 0 && knobs_of({{"NORI_TRACE_CULL", "10"}}).trace_cull == 1);
    CHECK(knobs_of({{"NORI_TRACE_CULL", "2"}}).trace_cull == 2 && knobs_of({{"NORI_TRACE_CULL", "3"}}).trace_cull == 1);
    CHECK(knobs_of({{"NORI_TRACE_CULL", "-1"}}).trace_cull == 1);
    g_what = "scene_knobs, NORI_TRAVERSAL and NORI_BVH_STACK";
    CHECK(knobs_of({{"NORI_TRAVERSAL", "bvh"}}).traversal == 1 && knobs_of({{"NORI_TRAVERSAL", "scan"}}).traversal == 2);
    CHECK(knobs_of({{"NORI_TRAVERSAL", "BVH"}}).traversal == 0 && knobs_of({{"NORI_TRAVERSAL", "scans"}}).traversal == 0);
    for (int v : {8, 16, 32}) CHECK(knobs_of({{"NORI_BVH_STACK", std::to_string(v)}}).stack_forced == v);
    for (const char *v : {"4", "24", "64", "-8"}) CHECK(knobs_of({{"NORI_BVH_STACK", v}}).stack_forced == 0);
    CHECK(!scan_mode(64, knobs_of({{"NORI_TRAVERSAL", "bvh"}})) && scan_mode(65, knobs_of({{"NORI_TRAVERSAL", "scan"}})));
    CHECK(scan_mode(64, SceneKnobs{}) && !scan_mode(65, SceneKnobs{}));
}

// The decisions of one scene under one setting of the knobs, against the rules of scene_plan.h
static void check_decisions(const nori_scene_desc &d, const SceneKnobs &k, bool basic, bool by_size_scan, bool envmap) {
    const ScenePlan p = plan_scene(d, k);
    const bool scan = k.traversal ? k.traversal == 2 : by_size_scan;
    CHECK(p.scan == scan && p.basic == basic);
    CHECK(p.stack_forced == k.stack_forced);
    CHECK(p.stack == (scan ? 0 : bvh_stack_for(p.tree.bvh.depth, k.stack_forced)));
    CHECK(scan ? p.refit.slots.empty() && !p.scan_list.prims.empty() : !p.refit.slots.empty() && p.scan_list.prims.empty());
    const bool pairs = !p.scan_list.plane_f.empty();
    CHECK(p.trace_cull == (k.trace_cull == 2 && !pairs ? 1 : k.trace_cull) && p.camera_cull == k.camera_cull);
    const bool nee = scan && basic && (k.nee_inline < 0 || k.nee_inline == 1);  // (kNeeFull is 0: never for full plugins)
    CHECK(p.nee_inline == nee);
    CHECK(p.ext_inline == (nee && (k.ext_inline < 0 || k.ext_inline == 1)));
    CHECK(!p.ext_inline || p.nee_inline);
    CHECK(p.fuse_trace == (k.fuse_trace >= 0 ? k.fuse_trace == 1 : !(scan && !basic)));
    CHECK(p.finish_first == k.finish_first);
    CHECK(p.skip_discrete_nee == (!envmap && !k.discrete_nee));
    CHECK(p.chroma == false && p.border == film_border(d.camera) && p.border <= 4);
    CHECK(p.jit_lk == jit_code_lookup(d.camera.filter_radius, NORI_FILTER_RESOLUTION / d.camera.filter_radius));
    CHECK(p.use_blob == (scan && p.blob_bytes <= kBlobMaxBytes));
    const bool few = scan && p.scan_list.prims.size() / 12 <= 2 * kScanMaxPrims;
    CHECK(p.build_scan == few && p.build_shade == (few && basic && d.integrator < NORI_INTEGRATOR_NORMALS));
    CHECK(p.shade_integrator == plan_shade_integrator(d.integrator));
    CHECK(p.shade_lds == (p.use_blob && p.blob_bytes <= kPlanShadeLdsMax));
}

static void check_scene_decisions(const char *kind, const nori_scene_desc &d, bool basic, bool by_size_scan, bool envmap) {
    const char *names[] = {"NORI_TRAVERSAL", "NORI_BVH_STACK", "NORI_CAMERA_CULL", "NORI_TRACE_CULL", "NORI_NEE_INLINE",
                           "NORI_EXT_INLINE", "NORI_TRACE_FUSE", "NORI_DISCRETE_NEE", "NORI_FINISH_FIRST"};
    std::vector<std::map<std::string, std::string>> envs = {{}};
    for (const char *n : names)
        for (const char *v : {"0", "1", "junk"}) envs.push_back({{n, v}});
    for (const char *v : {"2", "3"}) envs.push_back({{"NORI_TRACE_CULL", v}});
    for (const char *v : {"bvh", "scan"}) envs.push_back({{"NORI_TRAVERSAL", v}});
    for (const char *v : {"8", "16", "32"}) envs.push_back({{"NORI_BVH_STACK", v}});
    envs.push_back({{"NORI_NEE_INLINE", "0"}, {"NORI_EXT_INLINE", "1"}});  // ext_inline requires nee_inline
    envs.push_back({{"NORI_NEE_INLINE", "1"}, {"NORI_EXT_INLINE", "0"}});
    envs.push_back({{"NORI_TRAVERSAL", "bvh"}, {"NORI_NEE_INLINE", "1"}, {"NORI_TRACE_CULL", "2"}});
    for (const auto &env : envs) {
        g_what = std::string("decisions, ") + kind + ":";
        for (const auto &kv : env) g_what += " " + kv.first + "=" + kv.second;
        check_decisions(d, knobs_of(env), basic, by_size_scan, envmap);
    }
    g_what = std::string("decisions, ") + kind;
    const ScenePlan def = plan_scene(d, SceneKnobs{});
    if (by_size_scan && basic) CHECK(def.nee_inline && def.ext_inline && def.fuse_trace && def.use_blob && def.build_shade);
    if (by_size_scan && !basic) CHECK(!def.nee_inline && !def.ext_inline && !def.fuse_trace && def.build_scan && !def.build_shade);
    if (!by_size_scan) CHECK(def.fuse_trace && !def.use_blob && def.stack >= 8 && !def.build_scan && !def.nee_inline);
    if (!by_size_scan) CHECK(def.trace_cull == 1 && plan_scene(d, knobs_of({{"NORI_TRACE_CULL", "2"}})).trace_cull == 1);
    if (!def.scan_list.plane_f.empty()) CHECK(plan_scene(d, knobs_of({{"NORI_TRACE_CULL", "2"}})).trace_cull == 2);
    // a chromatic aberration counts only on the advanced camera
    nori_scene_desc c = d;
    c.camera.chromatic[1] = 0.01f;
    CHECK(!plan_scene(c, SceneKnobs{}).chroma);
    c.camera.camera_type = NORI_CAMERA_ADVANCED;
    CHECK(plan_scene(c, SceneKnobs{}).chroma && !plan_scene(c, SceneKnobs{}).basic);
}

// ---- 3. one blob
static void check_blob(const char *path, const ScenePlan &p) {
    g_what = std::string("blob of ") + path;
    std::vector<char> blob;
    uint32_t offs[10];
    pack_blob(p, blob, offs);
    CHECK(blob.size() == p.blob_bytes && blob.size() % 16 == 0);
    const std::vector<float> &prims = p.prim_list();
    const std::pair<const void *, size_t> tables[10] = {
        {prims.data(), prims.size() * 4},         {p.tri_vidx.data(), p.tri_vidx.size() * 4},
        {p.pos.data(), p.pos.size() * 4},         {p.nrm.data(), p.nrm.size() * 4},
        {p.prim_shape.data(), p.prim_shape.size() * 4}, {p.shapes.data(), p.shapes.size() * sizeof(DevShape)},
        {p.bsdfs.data(), p.bsdfs.size() * sizeof(DevBsdf)}, {p.emitters.data(), p.emitters.size() * sizeof(DevEmitter)},
        {p.cdf.data(), p.cdf.size() * 4},         {p.tree.bvh.nodes.data(), p.tree.bvh.nodes.size() * 4}};
    size_t end = 0;
    for (int k = 0; k < 10; ++k) {
        CHECK(offs[k] % 16 == 0 && offs[k] >= end && offs[k] - end < 16);  // ascending, aligned, no gap beyond the padding
        end = offs[k] + tables[k].second;
        CHECK(end <= blob.size());
        if (end <= blob.size() && tables[k].second) CHECK(!std::memcmp(blob.data() + offs[k], tables[k].first, tables[k].second));
    }
    CHECK(blob.size() - end < 16);
}

int main(int argc, char **argv) {
    if (argc != 7) {
        std::fprintf(stderr, "usage: scene_plan_check cbox.xml basic.xml basic.xml envmap.xml textured.xml bvh.xml\n");
        return 2;
    }
    try {
        std::vector<std::unique_ptr<HostScene>> hs;
        for (int i = 1; i < argc; ++i) hs.emplace_back(load_scene_xml(argv[i], 0, 0, 0));
        check_refusals(hs[0]->desc);
        check_stack_table();
        check_knob_parsing();
        check_scene_decisions("basic scan", hs[0]->desc, true, true, false);
        check_scene_decisions("full-plugin scan (envmap)", hs[3]->desc, false, true, true);
        check_scene_decisions("BVH (microfacet mesh)", hs[5]->desc, false, false, false);
        check_scene_decisions("full-plugin BVH (textured)", hs[4]->desc, false, false, false);
        for (int i = 1; i < argc; ++i) {
            const ScenePlan p = plan_scene(hs[i - 1]->desc, SceneKnobs{});
            check_blob(argv[i], p);
            print_hashes(argv[i], p);
        }
    } catch (const std::exception &e) {
        std::printf("FAILED: %s [%s]\n", e.what(), g_what.c_str());
        return 1;
    }
    if (g_failed) return 1;
    std::printf("ok\n");
    return 0;
}
