// render_plan.cpp -- render_plan.h's sizes; the measurements behind each default stay with it.
#include "render_plan.h"

#include <algorithm>
#include <cstdlib>

namespace nori {

// The termination check reads the done flag as the device has set it by now,
// which may be up to `lag` iterations further than the event just waited for:
// how many iterations a render launches past the one that handed out the last
// work id (and so how its rays divide between the loop and the finisher)
// depends on how far the host runs ahead of the device.  With 0 the host waits
// for every iteration before it reads the flag, and the counts are the same in
// every run (the tests that compare two renders' statistics exactly use it).
int lookahead(const char *text) {
    const int v = text ? std::atoi(text) : 6;
    return v < 0 ? 0 : v > 8 ? 8 : v;
}

// Default 3: each part's launches wait for their own slowest walks / longest
// lanes, and three streams keep the chip busy in between (C3: 2 parts 619,
// 3 parts 651, 4 parts 499 Msamples/s -- 4 streams exceed the hardware
// queues; table scene 517 -> 555; C2 4563 -> 4658; 64-spp share 3026 ->
// 3089; C4 and C5 within 1 %).
// Renders whose shade kernel traces its own extension rays (ext_loop): 2.
// An iteration is one launch there, so no part's scan is left to slip under
// another part's shade launch (C2, 1M pool: 2 parts 6529-6637 Msamples/s;
// 2M pool: 1 part 5579-5615, 2 parts 6404-6460, 3 parts 6311-6410).
uint32_t pool_parts(const char *text, bool ext_loop) {
    const uint32_t def = ext_loop ? 2u : 3u;
    const long v = text ? std::atol(text) : (long)def;
    return (uint32_t)(v >= 1 && v <= kMaxParts ? v : def);
}

// default pool: about 1/16 of the render's samples in flight, between
// 1M and 4M paths (~0.9 GB of queues at 4M).  Large pools hide the shade
// kernel's memory latency (4M measured best among 256K..4M on cbox at 512
// spp); small renders -- the per-GPU share of a strong-scaled frame --
// spend less time draining a smaller pool (round 2, two parts, cbox 64
// spp: 4M 2190, 2M 2320, 1M 2400 Msamples/s; 512 spp: 4M and 2M within
// 1 %).  With three parts (round 3) the 64-spp share peaks at 1.25-1.5M
// (512K 2560, 1M 3030-3160, 1.25M 3320, 1.5M 3275-3296, 2M 3192, 3M 2952)
// and the 128-spp share at 2M (3989 against 3875 at 2.5M, 3773 at 3M).
// Since k_shade traces the shadow rays itself (round 6, nee_inline) the
// 64-spp share peaks at 1M again (4875 against 4702 at 1.5M, 4734 at
// 1.25M, 4555 at 768K; 3 reps), so the floor is 1M.  The BVH walks
// (C3) want about 1/8 in flight: 4M 846-851 against 807-812 at 2M
// (3M 796-798, 6M 796-798, 8M 839-846; 3 interleaved reps).
// Renders whose shade kernel traces its own extension rays (ext_loop)
// keep the 1M floor at every size: with one launch per iteration the
// smaller pool wins (C2 at 512 spp, two parts: 1M 6529-6637, 1.5M
// 6501-6511, 2M 6404-6460, 3M 6103-6210, 4M 6172-6180 Msamples/s; the
// 64-spp share: 768K 4926-4981, 1M 5054-5131, 1.5M 4884-4998).
uint32_t default_pool(uint32_t passes, uint32_t M, bool bvh, bool ext_loop, const char *text) {
    uint32_t pool = 1u << 20;
    if (text && std::atol(text) > 0) {  // NORI_PATH_POOL: default pool size override (tuning)
        pool = (uint32_t)std::min<long>(std::atol(text), 1L << 26);
    } else {
        const uint64_t want = (uint64_t)passes * M / (bvh ? 8 : 16);
        while (!ext_loop && pool < (1u << 22) && pool < want) pool <<= 1;
    }
    return round_pool(pool);
}

uint32_t record_chunk(uint32_t passes, uint32_t M, size_t budget) {
    const uint32_t chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(passes, budget / (16 * (size_t)M)));
    // work ids (record indices) < 2^29: the path queue keeps a chromatic
    // sample's colour channel in bits 29-30 of the same word (kWorkMask)
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(chunk, ((uint64_t)1 << kPlanChanShift) / M));
}

PartSplit part_split(uint32_t G, uint32_t parts) {
    PartSplit s{};
    for (uint32_t h = 0; h < parts; ++h) {
        s.base[h] = (uint32_t)((uint64_t)G * h / parts);
        s.count[h] = (uint32_t)((uint64_t)G * (h + 1) / parts) - s.base[h];
    }
    return s;
}

// Default: about one work-group per CU over the whole launch (passes x blocks
// / 256), so the splat leaves most of the chip to the tail finisher it
// overlaps with (cbox 512x512@512: 256 blocks x 512 passes per work-group,
// splat 3.0 ms and finisher 3.6 ms vs 4.7 / 5.2 ms at 32 passes).  The
// one-bounce integrators' splat has no finisher beside it: it targets 4096
// work-groups instead.
uint32_t splat_passes(uint32_t np, size_t nblocks, uint32_t target_wgs, const char *text) {
    long v = text ? std::atol(text) : (long)(((uint64_t)np * nblocks + target_wgs - 1) / target_wgs);
    if (v < 1) v = 1;
    return (uint32_t)std::min<long>(v, np);
}

// About kPosTargetWgs work-groups over the launch.  A work-group pays for its
// tile once -- zeroing it and the sweep of (32+2B)^2 x 4 atomics into the film
// -- whatever it folds, so few long work-groups beat many short ones: cbox
// 512x512, 8 passes, 1 / 2 / 4 / 8 passes per work-group 0.77 / 0.50 / 0.30 /
// 0.18 ms.  256 is also the target of the path integrators'
// splat.  (A launch has at most 65535 work-groups along the passes.)
uint32_t passes_per_wg(uint32_t np, size_t nblocks, const char *text) {
    constexpr uint64_t kPosTargetWgs = 256;
    uint64_t v = ((uint64_t)np * nblocks + kPosTargetWgs - 1) / kPosTargetWgs;
    if (text && std::atoll(text) > 0) v = (uint64_t)std::atoll(text);
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>({v, 1, ((uint64_t)np + 65534) / 65535}), np);
}

// passes_per_wg's range, at most kGatherRange unless the text names one.  Its
// 256 work-groups suit the forward, whose work-group pays a sweep of atomics
// for its tile; the gather's tile is one 26 KB read and a long range only
// serialises a lane: 64 passes at 512x512 in ranges of 64 / 16 / 4 / 1: 0.470 /
// 0.172 / 0.167 / 0.187 ms.
uint32_t gather_passes(uint32_t np, size_t nblocks, const char *text) {
    constexpr uint32_t kGatherRange = 4;
    const uint32_t v = passes_per_wg(np, nblocks, text);
    if (text && std::atoll(text) > 0) return v;
    return std::max(std::min(v, kGatherRange), (uint32_t)(((uint64_t)np + 65534) / 65535));
}

uint32_t pass_chunk(uint32_t passes, uint32_t M) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(passes, ((uint64_t)1 << 24) / M));
}

uint32_t query_chunk(const char *text) {
    if (text) {
        const long long v = std::atoll(text);
        if (v > 0) return (uint32_t)std::min<long long>(v, 0xFFFFFFFFll);
    }
    return 1u << 22;
}

}  // namespace nori
