// kernels.h -- launch wrappers for the gfx950 kernels.  Each launch_* is
// defined beside its kernel: launch_shade in kernels_shade.hip; launch_mark,
// launch_tail_prefix and launch_finish in kernels_finish.hip; launch_features
// in kernels_features.hip; launch_surface and launch_camera_rays in
// kernels_query.hip; the shading queries in kernels_shading.hip; the
// materials' adjoint and update in kernels_bsdf_grad.hip; the
// denoisers, the block error and the refit in denoise.hip, block_error.hip
// and refit.hip; the caller-fed film splats in kernels_film.hip; launch_li in
// kernels_li.hip; all others in kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "film_put.h"
#include "kernel_config.h"

namespace nori {

// (kShadeBlock, kShadeLdsMax, kNeeFull: kernel_config.h)
constexpr int kTraceBlock = 128;   // traversal work-group size (LDS stack columns)
constexpr int kTraceSpill = 64;    // traversal stack entries beyond the LDS part (private memory)
#ifndef NORI_STACK_KEYS
#define NORI_STACK_KEYS 1
#endif
// Stack entries held in LDS for an LDS budget of `stack` words per lane: with
// NORI_STACK_KEYS each entry is a (child ref, entry distance) pair.
constexpr int stack_lds_entries(int stack) { return NORI_STACK_KEYS ? stack / 2 : stack; }
constexpr int kSplatBlock = 256;
// The scattered film splat's default form (kernels_film.hip k_splat_scatter;
// measured in DESIGN.md D17)
#ifndef NORI_SCATTER_ROWS
#define NORI_SCATTER_ROWS 1
#endif
#ifndef NORI_SCAN_RAYS
#define NORI_SCAN_RAYS 2
#endif
constexpr int kScanRays = NORI_SCAN_RAYS;  // rays per thread of the scan-mode extension kernel
#ifndef NORI_SCAN_RAYS_SHADOW
#define NORI_SCAN_RAYS_SHADOW 1
#endif
constexpr int kScanRaysShadow = NORI_SCAN_RAYS_SHADOW;  // ... and of the scan-mode shadow kernel

struct SplatDesc {
    uint32_t M;               // pixels per pass in the work list
    uint32_t passes;          // passes in this chunk
    uint32_t pass_begin;      // absolute pass of chunk pass 0
    uint32_t passes_per_wg;   // passes folded by one work-group
    const int4 *blocks;       // (ox, oy, bw | bh << 16, first list entry)
    uint64_t seed;
    float *var;               // per-pixel sample statistics W x H x 8 (sum L, sum L^2, n) or null
};

// Scene-specialised scan kernels (rtc.hip): a scan-mode scene's scan list
// compiled in as literals through hipRTC at context creation.
struct ScanRtcScene;  // scene_prep.h
struct ScanRtc {
    hipModule_t mod = nullptr;
    hipFunction_t extend = nullptr, shadow = nullptr, trace[2] = {nullptr, nullptr};  // trace[any_hit]
    hipFunction_t both = nullptr;  // extension + shadow rays of one iteration in one launch (launch_trace_both)
    int k_extend = 0;         // rays per thread of `extend`
    double compile_ms = 0.0;  // hipRTC compile (or cache read) at context creation
    bool cached = false;      // the code object came from the process or disk cache
    size_t code_bytes = 0;
};
// The scene's own compilation of k_shade (shade_kernel.h through hipRTC):
// scan-mode scenes with the basic plugin set, whose k_shade holds the scans.
struct ShadeRtc {
    hipModule_t mod = nullptr;
    hipFunction_t shade = nullptr;  // nori_rtc_shade = k_shade<integrator, lds, 0> with literal records
    int integrator = 0;
    bool lds = false;
    double compile_ms = 0.0;  // hipRTC compile (or cache read) at context creation
    bool cached = false;
    size_t code_bytes = 0;
};
// Whether contexts use it where it can be built, absent NORI_RTC_SHADE.
constexpr bool kShadeRtcDefault = true;
std::string rtc_const_scene(const ScanRtcScene &sc);
// Compiles (or finds cached) the specialised code object for target `arch`;
// fresh: the cached copies are dropped first.
bool rtc_compile(const ScanRtcScene &sc, const std::string &arch, int trace_cull, std::vector<char> &code, double &ms,
                 bool &cached, std::string &why, bool fresh = false);
// ... and the shade program's, for k_shade<integrator, lds, 0>.
bool rtc_compile_shade(const ScanRtcScene &sc, const std::string &arch, int integrator, bool lds,
                       std::vector<char> &code, double &ms, bool &cached, std::string &why, bool fresh = false);
bool shade_rtc_wanted(std::string &why);  // NORI_RTC / NORI_RTC_SHADE
// Loads it on the current device after checking its ShadeArgs layout; false (with why) leaves `out` empty.
bool shade_rtc_build(const ScanRtcScene &sc, int device, int integrator, bool lds, ShadeRtc &out, std::string &why);
void shade_rtc_release(ShadeRtc &r);
// ... and loads it on the current device; false (with why) leaves `out` empty.
bool scan_rtc_build(const ScanRtcScene &sc, int device, int trace_cull, ScanRtc &out, std::string &why);
void scan_rtc_release(ScanRtc &r);
int rtc_rays_per_thread();

// stack = LDS stack depth (8, 16, 32 or 64) chosen from the BVH depth.
// rtc: the scene's specialised scan kernels, used for stack 0 when present.
hipError_t launch_trace(const DevScene &S, const float4 *rays, uint32_t n, int any_hit, float4 *hits, int stack,
                        hipStream_t st, const ScanRtc *rtc = nullptr);
hipError_t launch_shade(const DevScene &S, const PathQueue &in, const PathQueue &out, const ShadowQueue &sq,
                        const SegState &seg, int in_sel, const WorkDesc &wd, float4 *rec, Counters *C,
                        uint32_t nseg, hipStream_t st, const ShadeRtc *rtc = nullptr);
// The blob size up to which launch_shade stages the scene in LDS (the LDS
// template argument, and the one the scene's ShadeRtc is compiled with).
// The integrator k_shade is instantiated for (launch_shade's switch).
constexpr int shade_integrator(int i) {
    return i == NORI_INTEGRATOR_PATH_MATS || i == NORI_INTEGRATOR_VOLUMETRIC ? i : (int)NORI_INTEGRATOR_PATH_MIS;
}
inline uint32_t shade_lds_bytes(uint32_t blob_bytes) { return blob_bytes <= kShadeLdsMax ? blob_bytes : 0u; }
hipError_t launch_extend(const DevScene &S, const PathQueue &q, const uint32_t *cnt, uint32_t G, int stack,
                         hipStream_t st, const ScanRtc *rtc = nullptr);
hipError_t launch_shadow(const DevScene &S, const ShadowQueue &sq, const uint32_t *shcnt, float4 *rec, uint32_t G,
                         int stack, hipStream_t st, const ScanRtc *rtc = nullptr);
// Both trace launches of an iteration as one (the BVH walks, or the
// specialised scan kernels); false: nothing launched (a scan scene without
// them), use launch_extend + launch_shadow.
bool launch_trace_both(const DevScene &S, const PathQueue &q, const uint32_t *cnt, const ShadowQueue &sq,
                       const uint32_t *shcnt, float4 *rec, uint32_t G, int stack, const ScanRtc *rtc, hipStream_t st,
                       hipError_t &err);
// Marks the record of every queued path pending (w = kRecPending, the jitter
// class bits cleared): k_splat skips it, the finisher splats it itself.
// Zeroes the counters and segment state of a chunk, Counters::exhausted = empty.
hipError_t launch_reset(Counters *C, uint32_t empty, const SegState &seg, uint32_t G, hipStream_t st);
hipError_t launch_mark(const PathQueue &Q, const SegState &seg, int sel, float4 *rec, uint32_t G, hipStream_t st);
// The prefix over the segments' path counts that numbers the tail's paths
// (pre: G + 1 words); launch_finish reads it.
hipError_t launch_tail_prefix(const SegState &seg, int sel, uint32_t G, uint32_t *pre, hipStream_t st);
// Completes every queued path and splats its sample into `film` itself.
// (after launch_tail_prefix on the same stream)
hipError_t launch_finish(const DevScene &S, const PathQueue &Q, const SegState &seg, int sel, float4 *rec,
                         const WorkDesc &wd, float *film, Counters *C, uint32_t G, int stack, uint32_t *pre,
                         hipStream_t st);
// Photon tracing (photonmapper preprocess): count pass (out == null) writes
// the photons stored by each emitted photon e0 + i into count[i]; store pass
// writes the photons of emitted photons i < n at pre[i] (3 float4 each:
// position, direction towards the light, power), `total` photons in all.
hipError_t launch_photons(const DevScene &S, uint64_t e0, uint32_t n, uint32_t *count, const uint64_t *pre,
                          uint64_t total, float4 *out, int stack, hipStream_t st);
// One-bounce integrators (normals, av, direct, direct_ems/mats/mis) and the
// photon mapper: one thread per work id of wd (pass-major, pixels in
// wd.pixels order) writes its record.
hipError_t launch_direct(const DevScene &S, const WorkDesc &wd, float4 *rec, Counters *C, int stack, hipStream_t st);
// NL-means denoiser (denoise.hip, denoiser/denoiser.py): img W x H x 3,
// var W x H, radius R (offsets), box half-width P (= the script's f - 1).
size_t denoise_lds_bytes(int R, int P);
hipError_t launch_denoise(const float *img, const float *var, int W, int H, int R, int P, float k, int mode,
                          float *out, hipStream_t st);
// Feature-guided denoiser (denoise.hip k_guided; stated at
// nori_film_denoise_guided in nori_gpu.h): img W x H x 3, var W x H, feat
// W x H x 7, radius R, patch half-width F; a sigma of +inf switches its term off.
size_t guided_lds_bytes(int R, int F);
hipError_t launch_guided(const float *img, const float *var, const float *feat, int W, int H, int R, int F, float k,
                         float eps, float sigma_a, float sigma_n, float sigma_z, float *out, hipStream_t st);
// First-hit features (kernels_features.hip k_features): one thread per entry
// of `pixels` (M entries, y*W + x) adds the samples of passes [pass_begin,
// pass_begin + np) in pass order to the pixel's eight sums in feat (W x H x 8,
// 16-byte aligned): albedo, shading normal, hit distance, sample count.
hipError_t launch_features(const DevScene &S, const uint32_t *pixels, uint32_t M, uint32_t pass_begin, uint32_t np,
                           uint64_t seed, float *feat, int stack, hipStream_t st);
// Hit records (kernels_query.hip k_surface; stated at nori_scene_surface in
// nori_gpu.h): record i (four float4) of hit i (t, prim, u, v) of ray i (two
// float4), i < n; all three arrays 16-byte aligned.
hipError_t launch_surface(const DevScene &S, const float4 *rays, const float4 *hits, uint32_t n, float4 *out,
                          hipStream_t st);
// The record's adjoint (kernels_surface_grad.hip k_surface_grad; stated at
// nori_scene_surface_grad in nori_gpu.h): the terms of hit i < n, formed from
// the scene's current pos / nrm, are added with float atomics into
// grad_positions and (unless null) grad_normals, num_vertices x 3 floats each.
// rays, hits and grad_surf (four float4 per hit) are 16-byte aligned; all
// device memory.  A vertex id not below num_vertices adds nothing.
hipError_t launch_surface_grad(const DevScene &S, uint32_t num_vertices, const float4 *rays, const float4 *hits,
                               const float4 *grad_surf, uint32_t n, float *grad_positions, float *grad_normals,
                               hipStream_t st);
// bsdf_eval's adjoint in the material rows (kernels_bsdf_grad.hip; stated at
// nori_scene_bsdf_grad in nori_gpu.h).  launch_bsdf_grad: the rows of
// elements [first, first + n) of an array of N elements (the pointers are at
// element `first`, a multiple of bsdf_grad_tile(); slabs_n = bsdf_grad_slabs(N));
// terms (may be null) receives each element's row.  surf (four float4 per
// element), grad_out (two), terms (four) and slabs are 16-byte aligned; all
// device memory.  bsdf_grad_table(num_bsdfs): the reproducible path without
// atomics runs (up to NORI_BSDF_GRAD_MAX_TABLE BSDFs, unless
// NORI_BSDF_GRAD_TABLE=0): the sums go to `slabs` (slabs_n x num_bsdfs x 16
// floats; the launch for first = 0 starts them, later ones continue them) and
// launch_bsdf_grad_sum, after the last chunk, ADDS the slabs' sums into
// grad_materials (num_bsdfs x 16 floats).  Otherwise launch_bsdf_grad adds
// into grad_materials with float atomics and launch_bsdf_grad_sum does nothing.
uint32_t bsdf_grad_slabs(uint32_t n);
uint32_t bsdf_grad_tile();
bool bsdf_grad_table(uint32_t num_bsdfs);
hipError_t launch_bsdf_grad(const DevScene &S, uint32_t num_shapes, uint32_t num_bsdfs, const float4 *surf,
                            const float *wi, const float *wo, const float4 *grad_out, uint32_t n, uint32_t first,
                            uint32_t slabs_n, float *grad_materials, float4 *terms, float *slabs, hipStream_t st);
hipError_t launch_bsdf_grad_sum(uint32_t num_bsdfs, const float *slabs, uint32_t slabs_n, float *grad_materials,
                                hipStream_t st);
// nori_gpu_update_materials: *count += the non-finite floats among the words in
// use of rows (num_bsdfs x 16 floats); then each row set into its record of
// bsdfs and, unless null, of the blob's copy.
hipError_t launch_materials_count(const DevBsdf *bsdfs, const float *rows, uint32_t num_bsdfs, uint32_t *count,
                                  hipStream_t st);
hipError_t launch_materials_set(DevBsdf *bsdfs, DevBsdf *blob_bsdfs, const float *rows, uint32_t num_bsdfs,
                                hipStream_t st);
// Primary rays (kernels_query.hip k_camera_rays): the ray of sample (pass
// pass_begin + k, pixel pix) for k in [k0, k0 + np) and the M entries of
// `pixels` (y*W + x), written at rays[8 * (k * W * H + pix)]; np * M < 2^31.
hipError_t launch_camera_rays(const DevScene &S, const uint32_t *pixels, uint32_t M, uint32_t pass_begin, uint32_t k0,
                              uint32_t np, uint64_t seed, float *rays, hipStream_t st);
// Shading queries (kernels_shading.hip; stated at nori_gpu_bsdf_eval ..
// nori_gpu_sample_uniforms in nori_gpu.h): element i < n of each array, all
// device memory.  surf: 64-byte records (four float4, 16-byte aligned);
// wi / wo / x / from: 3 floats and u: 2 floats per element (4-byte aligned);
// out: 2, 2, 3 and 1 float4 per element.  A record whose shape is not below
// num_shapes and an emitter id not below S.num_emitters give zeros.
hipError_t launch_bsdf_eval(const DevScene &S, uint32_t num_shapes, const float4 *surf, const float *wi,
                            const float *wo, uint32_t n, float4 *out, hipStream_t st);
hipError_t launch_bsdf_sample(const DevScene &S, uint32_t num_shapes, const float4 *surf, const float *wi,
                              const float *u, uint32_t n, float4 *out, hipStream_t st);
// ids == null: `emitter` for every element
hipError_t launch_emitter_sample(const DevScene &S, const int32_t *ids, int32_t emitter, const float *x, const float *u,
                                 uint32_t n, float4 *out, hipStream_t st);
hipError_t launch_emitter_eval(const DevScene &S, uint32_t num_shapes, const float4 *surf, const float *from,
                               uint32_t n, float4 *out, hipStream_t st);
// Draws [first, first + count) of the stream of sample (pass pass_begin + k,
// pixel pix) for k in [k0, k0 + np) and the M entries of `pixels`, written at
// out[count * (k * W * H + pix)]; np * M < 2^31.
hipError_t launch_sample_uniforms(const DevScene &S, const uint32_t *pixels, uint32_t M, uint32_t pass_begin,
                                  uint32_t k0, uint32_t np, uint64_t seed, uint32_t first, uint32_t count, float *out,
                                  hipStream_t st);
// Radiance queries (kernels_li.hip k_li; stated at nori_gpu_li in nori_gpu.h):
// Li of the context's integrator along row i < n of `rays` (two float4, 16-byte
// aligned) on the stream wave_seed(seed, ids ? ids[i] : stream_base + i) after
// first_draw draws, written at out[3 i]; all device memory.  A wave owns
// `range` (>= 64) consecutive rows; refill != 0: a lane whose path has ended
// starts the next row of its wave's range (0: one row per lane, range 64).
// counters[0..2] += closest-hit rays, shadow rays, rows whose value fails
// Color3f::isValid.
struct LiArgs {
    const float4 *rays;
    const uint64_t *ids;  // or null
    float *out;
    uint32_t n, range, refill, first_draw;
    uint64_t seed, stream_base;
    unsigned long long *counters;
};
hipError_t launch_li(const DevScene &S, const LiArgs &a, int stack, hipStream_t st);
hipError_t launch_splat(const DevScene &S, const float4 *rec, const SplatDesc &sd, uint32_t nblocks, float *film,
                        Counters *C, hipStream_t st);
// Caller-supplied samples into the film (kernels_film.hip; stated at
// nori_film_splat in nori_gpu.h).  All pointers are device memory; *dropped +=
// the samples the statement drops.  film: (H+2B) x (W+2B) x 4 and var (or null):
// H x W x 8, both added into with float atomics.
// The passes layout (ordered): pass k < passes of the pixels of `blocks`
// (work_lists' (ox, oy, bw | bh << 16, .)), the sample of pixel (x, y) at
// pos[2 i], val[3 i] with i = k * stride + y * W + x; a work-group folds
// passes_per_wg passes (>= 1, at most 65535 pass ranges).
hipError_t launch_splat_pos(const FilmGeom &F, const int4 *blocks, uint32_t nblocks, uint32_t passes,
                            uint32_t passes_per_wg, uint64_t stride, const float *pos, const float *val, float *film,
                            float *var, unsigned long long *dropped, hipStream_t st);
// Samples i < n anywhere on the image (the owner is the floor of the position);
// rows: a wave walks its samples and adds whole window rows per instruction,
// else one lane per sample (k_splat_scatter).
constexpr bool kScatterRows = NORI_SCATTER_ROWS != 0;
hipError_t launch_splat_scatter(const FilmGeom &F, uint64_t n, bool rows, const float *pos, const float *val,
                                float *film, float *var, unsigned long long *dropped, hipStream_t st);
// The splat's adjoint (kernels_gather.hip; stated at nori_film_gather in
// nori_gpu.h).  All pointers are device memory; val may be null; grad: (H+2B) x
// (W+2B) x 4, 16-byte aligned, read only; gval: three floats per sample,
// written; *dropped += the zero rows.  The layouts are the splat launches'.
hipError_t launch_gather_pos(const FilmGeom &F, const int4 *blocks, uint32_t nblocks, uint32_t passes,
                             uint32_t passes_per_wg, uint64_t stride, const float *pos, const float *val,
                             const float *grad, float *gval, unsigned long long *dropped, hipStream_t st);
hipError_t launch_gather_scatter(const FilmGeom &F, uint64_t n, const float *pos, const float *val, const float *grad,
                                 float *gval, unsigned long long *dropped, hipStream_t st);
// The adaptive sampler's block error (block_error.hip; the metric is stated
// at nori_film_block_error in nori_gpu.h): stats W x H x 8 on the device
// (16-byte aligned), ids = the nblocks frame blocks to evaluate (null: blocks
// 0 .. nblocks-1), err = one float per frame block, written at the block's id.
hipError_t launch_block_error(const float *stats, int W, int H, int nbx, const uint32_t *ids, uint32_t nblocks,
                              float *err, hipStream_t st);
// dst[i] += src[i], i < n (device buffers)
hipError_t launch_add_into(float *dst, const float *src, size_t n, hipStream_t st);
// Dynamic geometry (refit.hip; the refit is stated at nori_scene_bvh_refit in
// nori_gpu.h).  All pointers are device memory.
// *count += the non-finite values among a[0 .. n) and, if given, b[0 .. n).
hipError_t launch_refit_count_nonfinite(const float *a, const float *b, size_t n, uint32_t *count, hipStream_t st);
// pos[v].xyz = p[3v ..] and, if n is given, nrm[v].xyz = n[3v ..], v < V; the w lanes stay.
hipError_t launch_refit_set_vertices(float4 *pos, float4 *nrm, const float *p, const float *n, uint32_t V,
                                     hipStream_t st);
// The P leaf-order records rebuilt from pos through vidx (spheres left alone).
hipError_t launch_refit_records(float4 *prims, const uint32_t *vidx, const float4 *pos, uint32_t P, hipStream_t st);
// One level of the refit schedule (RefitPlan, host_scene.h): the boxes of the n
// (node, slot) entries of `slots`; the levels below have completed on `st`.
hipError_t launch_refit_level(float4 *nodes, const float4 *prims, const uint32_t *vidx, const float4 *pos,
                              const uint32_t *slots, uint32_t n, hipStream_t st);
// The BVH rebuild (rebuild.hip; stated at nori_scene_bvh_rebuild in nori_gpu.h).
// All pointers are device memory; n = S's primitives (>= 1), read through
// S.tri_vidx, S.pos, S.prim_shape and S.shapes.
// box[0..2] / box[3..5] = min / max over the primitive boxes as order keys (rebuild.h).
hipError_t launch_rebuild_scene_box(const DevScene &S, uint32_t n, uint32_t *box, hipStream_t st);
// keys[id] = Morton code << 32 | id on the grid (lo, scale) of the scene box.
hipError_t launch_rebuild_keys(const DevScene &S, uint32_t n, const float lo[3], const float scale[3], uint64_t *keys,
                               hipStream_t st);
// rocprim's radix sort of the n keys / exclusive sum of n counts; temp == null: temp_bytes = the storage needed.
hipError_t rebuild_sort_keys(void *temp, size_t &temp_bytes, const uint64_t *in, uint64_t *out, uint32_t n,
                             hipStream_t st);
hipError_t rebuild_scan_counts(void *temp, size_t &temp_bytes, const uint64_t *in, uint64_t *out, uint32_t n,
                               hipStream_t st);
// The n records in the order of the sorted keys.
hipError_t launch_rebuild_records(const DevScene &S, const uint64_t *sorted, uint32_t n, float4 *prims, hipStream_t st);
// A breadth-first level of m nodes with the record ranges `ranges`: split writes
// each node's slots (ends) and count[0 .. m] (inner | leaf << 32, count[m] = 0);
// after the exclusive scan of count, emit writes the nodes' compact refs at
// refs[level_off ..], the next level's ranges, inner_slots[child - 1] and the
// level's leaf slots from leaf_slots[leaf_base].  The caller has checked
// level_off + m + the level's inner slots <= n and leaf_base + its leaf slots <= n.
hipError_t launch_rebuild_split(const uint64_t *sorted, const uint2 *ranges, uint32_t m, uint32_t leaf_max, uint4 *ends,
                                uint64_t *count, hipStream_t st);
hipError_t launch_rebuild_emit(const uint2 *ranges, const uint4 *ends, const uint64_t *scan, uint32_t m,
                               uint32_t level_off, uint32_t leaf_base, uint32_t leaf_max, uint4 *refs, uint2 *next,
                               uint32_t *inner_slots, uint32_t *leaf_slots, hipStream_t st);
// The N nodes (8 float4 each) from their compact refs: NaN boxes in the unused slots, zero boxes in the used ones.
hipError_t launch_rebuild_nodes(const uint4 *refs, uint32_t N, float4 *nodes, hipStream_t st);

}  // namespace nori
