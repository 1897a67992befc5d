// refit.h -- the arithmetic of the BVH refit, shared by its host statement
// (bvh_refit.cpp, nori_scene_bvh_refit) and its kernels (refit.hip).
//
// A refit keeps the tree and recomputes its boxes, so the only arithmetic is
// min / max, which do not round -- except that IEEE min / max may return
// either zero for (-0, +0).  box_min / box_max order the zeros (-0 < +0), so a
// box is a function of the SET of its points and every implementation gives
// the same bytes.  Inputs are finite (NaN marks an unused child slot and is
// never passed in).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NORI_REFIT_HD __host__ __device__ inline
#else
#define NORI_REFIT_HD inline
#endif

namespace nori {

NORI_REFIT_HD uint32_t refit_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
NORI_REFIT_HD float box_min(float a, float b) { return (a < b || (a == b && (refit_bits(a) >> 31))) ? a : b; }
NORI_REFIT_HD float box_max(float a, float b) { return (a > b || (a == b && !(refit_bits(a) >> 31))) ? a : b; }
// NaN test on the bits (an unused child slot's box)
NORI_REFIT_HD bool refit_unused(float box_word) { return (refit_bits(box_word) & 0x7fffffffu) > 0x7f800000u; }
NORI_REFIT_HD bool refit_nonfinite(float f) { return (refit_bits(f) & 0x7f800000u) == 0x7f800000u; }

// child ref of a 4-wide node (host_scene.h): bit 31 = leaf, bits 0-24 first record, bits 25-30 count - 1
constexpr uint32_t kRefitLeafBit = 0x80000000u;
NORI_REFIT_HD uint32_t refit_leaf_first(uint32_t ref) { return ref & 0x01ffffffu; }
NORI_REFIT_HD uint32_t refit_leaf_count(uint32_t ref) { return ((ref >> 25) & 63u) + 1u; }

}  // namespace nori
