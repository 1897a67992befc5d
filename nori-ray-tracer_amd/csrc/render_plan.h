// render_plan.h -- the host-pure arithmetic that sizes a call before anything
// is launched: the wavefront render's pool, record chunks and pool parts, the
// passes a splat work-group folds, and the chunks of the queries.  Plain C++
// without HIP types, compiled by the host compiler (render_plan.cpp), so
// tests/render_plan_check.cpp runs it under the sanitizers as a program of its
// own.  A function that follows an environment variable takes the variable's
// text (or null); the callers pass std::getenv(..).
#pragma once
#include <cstddef>
#include <cstdint>

namespace nori {

constexpr int kMaxParts = 4;  // pool parts on separate streams (GPU_MAX_HW_QUEUES is 4)
// seg_index.h's kSeg and dev_scene.h's kChanShift: neither header compiles
// warning-free with the host compiler, so the two values are carried here and
// render.hip asserts that they are equal.
constexpr uint32_t kPlanSeg = 256;
constexpr uint32_t kPlanChanShift = 29;

// NORI_LOOKAHEAD (0 .. 8): iterations queued ahead of the termination check (render.hip), default 6.
int lookahead(const char *text);
// NORI_POOL_PARTS (1 .. kMaxParts): independent pool parts on their own streams.
uint32_t pool_parts(const char *text, bool ext_loop);
// A pool size as the render uses it: a multiple of kSeg, at least kSeg.
inline uint32_t round_pool(uint32_t pool) {
    const uint32_t up = (pool + kPlanSeg - 1) / kPlanSeg * kPlanSeg;
    return up < kPlanSeg ? kPlanSeg : up;
}
// The pool of a render that names none (render_desc.path_pool = 0), rounded by
// round_pool; `bvh`: the scene is traversed with a stack; text: NORI_PATH_POOL.
uint32_t default_pool(uint32_t passes, uint32_t M, bool bvh, bool ext_loop, const char *text);
// Passes per chunk of sample records of M pixels (16 bytes each) within
// `budget` bytes: 1 .. passes, and chunk * M <= 2^kChanShift where that leaves 1.
uint32_t record_chunk(uint32_t passes, uint32_t M, size_t budget);
// Pool part h of `parts` (1 .. kMaxParts, <= G) over G segments: [base, base + count).
struct PartSplit {
    uint32_t base[kMaxParts], count[kMaxParts];
};
PartSplit part_split(uint32_t G, uint32_t parts);
// Sample passes folded by one work-group of k_splat: about target_wgs
// work-groups over np passes of nblocks blocks; text: NORI_SPLAT_PASSES.
uint32_t splat_passes(uint32_t np, size_t nblocks, uint32_t target_wgs, const char *text);
// ... and of k_splat_pos (film_splat.hip); text: NORI_SPLAT_POS_PASSES.
uint32_t passes_per_wg(uint32_t np, size_t nblocks, const char *text);
// ... and walked by one work-group of k_gather_pos: passes_per_wg's, at most 4
// unless the text names a range (1 .. np, at most 65535 ranges a launch);
// text: NORI_GATHER_PASSES.
uint32_t gather_passes(uint32_t np, size_t nblocks, const char *text);
// Passes per launch of the calls that run one kernel over M pixels: about 16M elements.
uint32_t pass_chunk(uint32_t passes, uint32_t M);
// NORI_QUERY_CHUNK: the most elements of a host array staged at once.
uint32_t query_chunk(const char *text);

}  // namespace nori
