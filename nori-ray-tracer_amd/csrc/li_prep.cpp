// li_prep.cpp -- nori_gpu_li's host-pure checks and knobs (li_prep.h).
#include "li_prep.h"

#include <cerrno>
#include <cstdlib>

namespace nori {

const char *li_check(const void *ctx, const nori_gpu_li_desc *desc, const void *rays, const void *stream_ids,
                     const void *out) {
    if (!ctx || !desc || !rays || !out) return "null argument";
    if (desc->reserved != 0) return "nori_gpu_li: reserved must be 0";
    if (desc->first_draw > 65535u) return "nori_gpu_li: first_draw must be at most 65535";
    if (desc->on_device) {
        if ((uintptr_t)rays % 16) return "nori_gpu_li: device rays must be 16-byte aligned";
        if ((uintptr_t)stream_ids % 8) return "nori_gpu_li: device stream_ids must be 8-byte aligned";
        if ((uintptr_t)out % 4) return "nori_gpu_li: device out must be 4-byte aligned";
    }
    return nullptr;
}

namespace {
// A whole decimal number in [lo, hi], or `otherwise`.
uint32_t env_number(const char *value, uint32_t lo, uint32_t hi, uint32_t otherwise) {
    if (!value || !*value) return otherwise;
    char *endp = nullptr;
    errno = 0;
    const unsigned long long v = std::strtoull(value, &endp, 10);
    if (errno || endp == value || *endp != '\0' || value[0] == '-' || value[0] == '+') return otherwise;
    if (v < lo || v > hi) return otherwise;
    return (uint32_t)v;
}
}  // namespace

uint32_t li_range(const char *value) { return env_number(value, 64, 4096, kLiRangeDefault); }
uint32_t li_refill(const char *value) { return env_number(value, 0, 1, kLiRefillDefault); }

LiSpan li_span(uint64_t n, uint32_t most, uint64_t j) {
    if (most == 0) most = 1;
    if (j > n / most) return {n, 0};  // (also keeps j * most from overflowing)
    const uint64_t first = j * most;
    if (first >= n) return {n, 0};
    const uint64_t left = n - first;
    return {first, (uint32_t)(left < most ? left : most)};
}

}  // namespace nori
