// gather_plan_check.cpp -- gather_passes (csrc/render_plan.cpp), the passes one
// work-group of k_gather_pos walks, as a program of its own (run under the
// sanitizers by tests/test_gather_plan.py): prints "ok" or the first mismatch.
#include <cstdio>
#include <initializer_list>

#include "render_plan.h"

using namespace nori;

static int fails = 0;
static void expect(uint32_t got, uint32_t want, const char *what) {
    if (got == want) return;
    std::printf("%s: got %u, want %u\n", what, got, want);
    ++fails;
}

int main() {
    // the default: passes_per_wg's range, at most 4
    expect(gather_passes(8, 256, nullptr), 4, "8 passes, 256 blocks");     // passes_per_wg: 8
    expect(gather_passes(64, 256, nullptr), 4, "64 passes, 256 blocks");   // passes_per_wg: 64
    expect(gather_passes(5, 6, nullptr), 1, "5 passes, 6 blocks");         // passes_per_wg: 1
    expect(gather_passes(3, 256, nullptr), 3, "3 passes, 256 blocks");     // never more than np
    expect(gather_passes(1, 1, nullptr), 1, "1 pass");
    expect(gather_passes(2, 128, nullptr), 1, "2 passes, 128 blocks");
    // text that names no range counts as none
    expect(gather_passes(64, 256, ""), 4, "empty text");
    expect(gather_passes(64, 256, "0"), 4, "text 0");
    expect(gather_passes(64, 256, "-3"), 4, "text -3");
    expect(gather_passes(64, 256, "x"), 4, "text x");
    // a named range is passes_per_wg's own answer, beyond the cap too
    expect(gather_passes(64, 256, "16"), 16, "text 16");
    expect(gather_passes(64, 256, "1"), 1, "text 1");
    expect(gather_passes(5, 6, "2"), 2, "text 2");
    expect(gather_passes(5, 6, "100"), 5, "text 100 of 5 passes");
    expect(gather_passes(64, 256, "64"), passes_per_wg(64, 256, "64"), "text 64");
    // at most 65535 ranges a launch, named or not
    expect(gather_passes(1u << 20, 1, nullptr), 17, "2^20 passes");        // ceil(2^20 / 65535)
    expect(gather_passes(1u << 20, 1, "1"), 17, "2^20 passes, text 1");
    expect(gather_passes(262140, 1, nullptr), 4, "65535 ranges of 4");
    expect(gather_passes(262141, 1, nullptr), 5, "one pass more");
    expect(gather_passes(0xFFFFFFFFu, 1, nullptr), 65537, "2^32 - 1 passes");
    for (uint32_t np : {1u, 2u, 7u, 64u, 4096u, 1u << 20, 0xFFFFFFFFu})
        for (size_t nb : {(size_t)1, (size_t)6, (size_t)256, (size_t)1 << 20}) {
            const uint32_t v = gather_passes(np, nb, nullptr);
            if (v < 1 || v > np || ((uint64_t)np + v - 1) / v > 65535) {
                std::printf("np %u nb %zu: range %u\n", np, nb, v);
                ++fails;
            }
        }
    if (!fails) std::printf("ok\n");
    return fails ? 1 : 0;
}
