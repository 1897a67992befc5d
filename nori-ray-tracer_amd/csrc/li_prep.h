// li_prep.h -- the host-pure part of nori_gpu_li (li.hip): the checks of its
// descriptor and pointers that need no device, its two environment knobs and
// the split of a call into launches.  Plain C++ without HIP types, compiled by
// the host compiler (li_prep.cpp), so tests/li_prep_check.cpp runs it under the
// sanitizers as a program of its own.
#pragma once
#include <cstdint>

#include "../../include/nori_gpu.h"

namespace nori {

constexpr uint32_t kLiRangeDefault = 256;  // rows per wave (NORI_LI_RANGE, 64 .. 4096)
constexpr uint32_t kLiRefillDefault = 1;   // lanes whose path has ended start further rows of the range (NORI_LI_REFILL)
constexpr uint32_t kLiLaunchRows = 1u << 24;  // rows per launch, as the other queries (queries.hip)

// The refusals of nori_gpu_li that need no device: null is returned when the
// call may go on, else the message of its NORI_ERR_INVALID.  (That a device
// pointer is device memory is asked of the HIP runtime, in li.hip.)
const char *li_check(const void *ctx, const nori_gpu_li_desc *desc, const void *rays, const void *stream_ids,
                     const void *out);
// NORI_LI_RANGE: `value` (the variable's text, or null) as rows per wave; anything
// but a whole number in [64, 4096] gives the default.
uint32_t li_range(const char *value);
// NORI_LI_REFILL: "0" = every lane takes exactly one row, "1" = a lane whose
// path has ended starts the next row of its wave's range; anything else the default.
uint32_t li_refill(const char *value);
// Launch j of a call over n rows covers rows [first, first + count): at most
// `most` rows each (most >= 1); count = 0 once j is past the last launch.
struct LiSpan {
    uint64_t first;
    uint32_t count;
};
LiSpan li_span(uint64_t n, uint32_t most, uint64_t j);

}  // namespace nori
