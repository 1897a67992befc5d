// rebuild.h -- the arithmetic of the linear-BVH rebuild, shared by its host
// statement (bvh_rebuild.cpp, nori_scene_bvh_rebuild) and its kernels
// (rebuild.hip).  Everything here is integer arithmetic or single fp32
// operations in a fixed order (contraction is off in this build), so both
// sides give the same bytes.
#pragma once
#include "refit.h"

namespace nori {

constexpr uint32_t kRebuildLeafDefault = 4;   // leaf_max = 0
constexpr uint32_t kRebuildLeafMax = 64;      // the child ref's count field (refit.h)
constexpr uint32_t kRebuildMaxPrims = 1u << 25;  // the child ref's first-record field
constexpr int kRebuildSearchSteps = 25;       // a binary search over < 2^25 records

// Grid coordinate of a box centre on one axis: c = 0.5 lo + 0.5 hi,
// x = (c - Lo) * scale, clamped to 0 .. 1023; a NaN (inf * 0) gives 0.
NORI_REFIT_HD uint32_t rebuild_cell(float lo, float hi, float Lo, float scale) {
    const float a = 0.5f * lo, b = 0.5f * hi;
    const float c = a + b;
    const float d = c - Lo;
    const float x = d * scale;
    return !(x >= 0.0f) ? 0u : x >= 1023.0f ? 1023u : (uint32_t)x;
}
// scale of an axis from its extent (one correctly rounded division)
inline float rebuild_scale(float Lo, float Hi) {
    const float ext = Hi - Lo;
    return ext > 0.0f ? 1024.0f / ext : 0.0f;
}
// bit k of v -> bit 3k
NORI_REFIT_HD uint32_t rebuild_spread(uint32_t v) {
    v &= 0x3ffu;
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
// 30-bit Morton code: bit 3k+2 = bit k of qx, 3k+1 = bit k of qy, 3k = bit k of qz
NORI_REFIT_HD uint32_t rebuild_morton(uint32_t qx, uint32_t qy, uint32_t qz) {
    return (rebuild_spread(qx) << 2) | (rebuild_spread(qy) << 1) | rebuild_spread(qz);
}

NORI_REFIT_HD int rebuild_clz64(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)v);
#else
    return v ? __builtin_clzll(v) : 64;
#endif
}

// Karras's split of the records a .. b (a < b) of the sorted keys: the largest
// index g in [a, b) whose K shares more leading bits with K[a] than K[b] does,
// K[i] = (sorted[i] & code bits) | i.  The halves are a .. g and g + 1 .. b.
NORI_REFIT_HD uint64_t rebuild_topo_key(const uint64_t *sorted, uint32_t i) {
    return (sorted[i] & 0xffffffff00000000ull) | (uint64_t)i;
}
NORI_REFIT_HD uint32_t rebuild_split(const uint64_t *sorted, uint32_t a, uint32_t b) {
    const uint64_t ka = rebuild_topo_key(sorted, a);
    const int d = rebuild_clz64(ka ^ rebuild_topo_key(sorted, b));
    uint32_t lo = a, hi = b;  // lo shares more than d bits (itself), hi does not
    for (int step = 0; step < kRebuildSearchSteps && hi - lo > 1; ++step) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (rebuild_clz64(ka ^ rebuild_topo_key(sorted, mid)) > d) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The used slots of the 4-wide node of records a .. b (more than leaf_max of
// them): its two halves, every half that is not a leaf replaced by its own two
// halves, in place and in order.  end[k] = last record of slot k (the first is
// a, or end[k - 1] + 1); returns the number of used slots, 2 .. 4.
NORI_REFIT_HD int rebuild_node_slots(const uint64_t *sorted, uint32_t a, uint32_t b, uint32_t leaf_max, uint32_t end[4]) {
    const uint32_t g = rebuild_split(sorted, a, b);
    int n = 0;
    if (g - a + 1 > leaf_max) {
        end[n++] = rebuild_split(sorted, a, g);
        end[n++] = g;
    } else {
        end[n++] = g;
    }
    if (b - g > leaf_max) {
        end[n++] = rebuild_split(sorted, g + 1, b);
        end[n++] = b;
    } else {
        end[n++] = b;
    }
    return n;
}

// float -> uint32 ordered like the values with -0 below +0 (box_min / box_max as integer min / max)
NORI_REFIT_HD uint32_t rebuild_order_key(float f) {
    const uint32_t u = refit_bits(f);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
NORI_REFIT_HD float rebuild_order_value(uint32_t k) {
    const uint32_t u = (k >> 31) ? (k & 0x7fffffffu) : ~k;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

}  // namespace nori
