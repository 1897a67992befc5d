// scene_prep.h -- the host arithmetic between a scene description and its
// upload: filter table, environment-map tables, block spiral, scene box,
// solitary spheres, scan list, area CDF, and the shares of a sharded render.
// Plain float / double code, each result pinned bit for bit by a CPU test or
// by the oracle; compiled by the host compiler (scene_prep.cpp, shard.cpp),
// free of HIP types, so tests/scene_prep_check.cpp links it without a device.
// Also the C ABI's error plumbing (fail / guarded) that every unit shares.
#pragma once
#include <cmath>
#include <exception>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "host_scene.h"

struct nori_scene {
    std::unique_ptr<nori::HostScene> hs;
};

namespace nori {

constexpr uint32_t kScanMaxPrims = 64;  // wave-uniform scan instead of BVH at or below this
constexpr size_t kBlobMaxBytes = 48 << 10;  // small-scene blob staged into LDS
// dev_scene.h's kScanGroup, which this header cannot include (upload.hip asserts that the two agree)
#ifndef NORI_SCAN_GROUP
#define NORI_SCAN_GROUP 4
#endif
constexpr uint32_t kScanListGroup = NORI_SCAN_GROUP;

// nori_gpu_last_error's thread-local string (defined in scene_prep.cpp)
std::string &last_error();
inline int fail(int code, const std::string &m) {
    last_error() = m;
    return code;
}
template <class F> int guarded(F &&f) {
    try {
        last_error().clear();
        return f();
    } catch (const NoriException &e) {
        return fail(e.code, e.what());
    } catch (const std::bad_alloc &) {
        return fail(NORI_ERR_OOM, "host allocation failed");
    } catch (const std::exception &e) {
        return fail(NORI_ERR_INVALID, e.what());
    }
}
bool debug_log();  // NORI_DEBUG=1

// rfilter.cpp -> tabulated filter (block.cpp:54-66): NORI_FILTER_RESOLUTION + 1 entries
void filter_table(const nori_camera_desc &c, float *t);
int film_border(const nori_camera_desc &c);
int jit_code_lookup(float radius, float lookup);

// EnvironmentMap tables (envmap.cpp:13-58, 91-109) appended to `env`: where each begins
struct EnvTables {
    uint32_t rgb_off, pdf_off, cdf_off, pmarg_off, cmarg_off;
};
EnvTables build_envmap(const nori_emitter_desc &e, std::vector<float> &env);

// BlockGenerator spiral (block.cpp:140-188)
std::vector<uint32_t> spiral_blocks(int W, int H);
// Scene box = BVH root box: every mesh vertex and every sphere's bounds.
// Reads `positions` unchecked: validate the mesh ranges first.
void scene_root_box(const nori_scene_desc &d, float rmin[3], float rmax[3]);
// DevShape::solitary of every shape (1 only for a sphere that qualifies)
std::vector<uint8_t> solitary_spheres(const nori_scene_desc &d, const float rmin[3], const float rmax[3]);

// The scan list of scan-mode scenes (scan.h scan_core).  Triangles that
// lie in an axis plane -- both edges with an exactly zero component on the
// same axis a, so every vertex has x_a = c -- come first, paired by plane:
// the kernels skip such a pair for a whole wave when no ray of the wave can
// hit it, a test that is exact only under the conditions checked here (no
// cancellation in the one remaining product difference of det and of t's
// numerator, scan.h plane_may_hit).  Pairs are ordered by axis (the
// kernels loop over each axis separately); a plane holding an odd number of
// triangles pads its last pair with a record no ray hits.  The remaining
// triangles follow, padded to kScanGroup, then the spheres.  Every record
// carries its leaf-order position in e2.w: among equal t the scan keeps the
// hit of the later leaf position, the reference's traversal order.
struct ScanList {
    std::vector<float> prims;   // 12 floats per record
    std::vector<float> plane_c; // per pair: the plane coordinate c
    std::vector<float> plane_f; // per pair: the in-plane filter of k_extend_bin (8 floats, plane_filters)
    uint32_t plane_end[3] = {0, 0, 0};  // pairs with axis <= a
    uint32_t tris = 0;          // triangle records (pairs + the rest, padded)
    uint32_t real = 0;          // ... of which the last real one ends here (the padding after it never hits)
    float fast_max = 0.0f;      // scan_fast_max of this list
};
ScanList build_scan_list(const DeviceBvh &bvh, uint32_t n);
// A scan list as the scene-specialised kernels take it (rtc.hip compiles it
// in as literals through hipRTC; kernels.h)
struct ScanRtcScene {
    const float *rec;  // 12 floats per record
    uint32_t nrec;
    const float *plane_c, *plane_f;  // per pair: 1 and 8 floats
    uint32_t pairs;
    uint32_t plane_end[3];
    uint32_t tris, real;
    float fast_max;  // the bound of scan.h's fast body (scan_fast_max), 0: none
};
// The bound M of the scene-specialised scan's fast body (scan.h): a ray whose
// origin and direction components are all at most M in magnitude keeps every
// intermediate of the triangle tests of this list -- tvec, pvec, qvec, det and
// the numerators of u, v and t -- and the sphere test's 2 d.d at or below
// 2^125, so none overflows and det lies in rcp_rn's verified range.  M is the
// largest power of two up to 2^60 for which the bounds below hold; a list
// whose coordinates leave no room for rays around it (M < 16 times its largest
// coordinate or edge) gets 0, no fast body.  NORI_SCAN_FAST=0 gives 0 as well (A/B).
float scan_fast_max(const ScanList &L);

// The path kernels' lite variants (FULL = false) serve scenes made of the
// basic plugins only: constant-albedo diffuse, mirror and dielectric BSDFs,
// area lights, the perspective camera, no normal maps.  NORI_BASIC=0 forces
// the full variants (A/B).
bool basic_scene(const nori_scene_desc &d);

// Mesh::activate's area DiscretePDF (mesh.cpp:30-38, dpdf.h:58-91) of a mesh
// whose triangle t has the vertices tri[3t .. 3t+2] of vtx(id): the serial
// fp32 running sum of the areas, times 1 / sum, last entry 1, in cdf (count + 1
// entries).  Returns DiscretePDF::getNormalization = 1 / sum, 0 for a mesh
// without area (its CDF stays unnormalised).  The one statement of both
// nori_gpu_create and nori_gpu_update_vertices.
template <class Vtx> float mesh_area_cdf(const uint32_t *tri, uint32_t count, Vtx vtx, std::vector<float> &cdf) {
    cdf.assign((size_t)count + 1, 0.0f);
    for (uint32_t t = 0; t < count; ++t) {
        const uint32_t *f = tri + 3 * (size_t)t;
        const float *p0 = vtx(f[0]), *p1 = vtx(f[1]), *p2 = vtx(f[2]);
        float e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
        float cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
        float area = 0.5f * std::sqrt((cx * cx + cy * cy) + cz * cz);
        cdf[t + 1] = cdf[t] + area;
    }
    const float sum = cdf[count];
    if (!(sum > 0)) return 0.0f;
    const float norm = 1.0f / sum;
    for (uint32_t t = 1; t <= count; ++t) cdf[t] *= norm;
    cdf[count] = 1.0f;
    return norm;
}

// ---- sharded renders (shard.cpp)
// This rank's share of a whole-frame render (nori_gpu_shard_desc).  The pass
// count defaults to the scene's sampleCount (0 -> 1) in both entry points, and
// a block list is checked (range) and de-duplicated in both modes, so the
// share always fits the caller's block_buf (capacity = the frame's blocks).
nori_gpu_render_desc shard_of(int W, int H, uint32_t spp, const nori_gpu_render_desc &whole, int mode, int nranks,
                              int rank, std::vector<uint32_t> &blocks);
// Samples of a share (pass count x pixels of its blocks, or of the image).
double share_samples(int W, int H, const nori_gpu_render_desc &s);
double comm_timeout_s(int status, double own_s, double own_samples, double max_samples);
int comm_status_word(int rc, int rank);

}  // namespace nori
