// Host check of the tail finisher's path numbering (nori-ray-tracer_amd/csrc/
// tail_index.h), compiled with g++ by tests/test_tail_index.py, once per
// NORI_FINISH_WAVES.  For segment counts G around the points where the 2 * G
// grid overtakes kFinishWaves / wpb, and count vectors with empty, full,
// lone, sparse and dense segments and totals around the steps of K, it
// builds the prefix the way k_tail_prefix's 1024 threads do, walks every
// (work-group, wave, lane) of the finisher's launch exactly as k_finish does,
// and asserts: pre[G] = n; no active lane has gid >= n; the segment found
// holds the gid (pre[sg] <= gid < pre[sg + 1], so it is not empty); the slot
// lies inside the segment's count and the queue index inside the queue; and
// the lanes left after the whole-work-group and whole-wave exits cover every
// gid in [0, n), and every queued entry, exactly once.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tail_index.h"

using namespace nori;

static long fails = 0;
#define CHECK(c, ...)                                  \
    do {                                               \
        if (!(c)) {                                    \
            if (fails++ < 20) std::printf(__VA_ARGS__); \
        }                                              \
    } while (0)

// kTraceBlock (kernels.h, a device header): kernels_finish.hip asserts kSeg == 2 * kTraceBlock
constexpr uint32_t kBlock = kSeg / 2, kWpb = kBlock / 64;

// k_tail_prefix: one work-group of 1024 threads, thread t owning `per` consecutive segments
static std::vector<uint32_t> prefix(const std::vector<uint32_t> &cnt) {
    const uint32_t G = (uint32_t)cnt.size(), per = tail_prefix_per(G);
    std::vector<uint32_t> pre((size_t)G + 1, 0xDEADBEEFu), part(1024);
    for (uint32_t t = 0; t < 1024; ++t) {
        const uint32_t b = t * per, e = std::min(G, b + per);
        uint32_t sum = 0;
        for (uint32_t i = b; i < e; ++i) sum += cnt[i];
        part[t] = sum;
    }
    for (uint32_t t = 1; t < 1024; ++t) part[t] += part[t - 1];  // the inclusive scan
    for (uint32_t t = 0; t < 1024; ++t) {
        const uint32_t b = t * per, e = std::min(G, b + per);
        uint32_t run = t ? part[t - 1] : 0u;
        for (uint32_t i = b; i < e; ++i) {
            pre[i] = run;
            run += cnt[i];
        }
    }
    pre[G] = part[1023];
    return pre;
}

static void run(const std::vector<uint32_t> &cnt, const char *name) {
    const uint32_t G = (uint32_t)cnt.size();
    uint64_t total = 0;
    for (uint32_t c : cnt) {
        CHECK(c <= kSeg, "%s G=%u: the test's own count %u > kSeg\n", name, G, c);
        total += c;
    }
    const std::vector<uint32_t> pre = prefix(cnt);
    const uint32_t n = pre[G];
    CHECK(n == total, "%s G=%u: pre[G] = %u, %llu paths queued\n", name, G, n, (unsigned long long)total);
    uint32_t run_sum = 0;
    for (uint32_t s = 0; s < G; ++s) {
        CHECK(pre[s] == run_sum, "%s G=%u: pre[%u] = %u, want %u\n", name, G, s, pre[s], run_sum);
        run_sum += cnt[s];
    }
    if (n != total) return;  // (the walk below sizes its tables by n)
    std::vector<unsigned char> seen_gid(n, 0), seen_q((size_t)G * kSeg, 0);
    const uint32_t K = tail_paths_per_wave(n), grid = tail_grid(G, kWpb);
    CHECK(K >= 1 && K <= 64, "%s G=%u n=%u: K = %u\n", name, G, n, K);
    for (uint32_t bid = 0; bid < grid; ++bid) {
        CHECK(tail_block_first(bid, kWpb, K) == tail_first(bid * kBlock, K), "%s G=%u n=%u: work-group %u starts at %u, its first wave at %u\n",
              name, G, n, bid, tail_block_first(bid, kWpb, K), tail_first(bid * kBlock, K));
        if (tail_block_first(bid, kWpb, K) >= n) continue;  // whole block idle
        for (uint32_t w = 0; w < kWpb; ++w) {
            const uint32_t first = tail_first(bid * kBlock + w * 64, K);
            if (first >= n) continue;  // whole wave idle
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint32_t gid = first + lane;
                const bool active = lane < K && gid < n;
                if (!active) continue;
                CHECK(gid < n, "%s G=%u n=%u: active gid %u\n", name, G, n, gid);
                const uint32_t sg = tail_segment(pre.data(), G, gid);
                CHECK(sg < G, "%s G=%u n=%u gid=%u: segment %u\n", name, G, n, gid, sg);
                if (sg >= G) continue;
                CHECK(pre[sg] <= gid && gid < pre[sg + 1], "%s G=%u n=%u gid=%u: segment %u holds [%u, %u)\n", name, G,
                      n, gid, sg, pre[sg], pre[sg + 1]);
                const uint32_t q = tail_slot(pre.data(), sg, gid);
                CHECK(q < G * kSeg, "%s G=%u n=%u gid=%u: queue index %u >= %u\n", name, G, n, gid, q, G * kSeg);
                CHECK(q - sg * kSeg < cnt[sg], "%s G=%u n=%u gid=%u: slot %u of segment %u past its count %u\n", name,
                      G, n, gid, q - sg * kSeg, sg, cnt[sg]);
                if (seen_gid[gid] < 255) ++seen_gid[gid];
                if (q < G * kSeg && seen_q[q] < 255) ++seen_q[q];
            }
        }
    }
    // nothing dropped by the early exits, nothing run twice
    for (uint32_t g = 0; g < n; ++g)
        CHECK(seen_gid[g] == 1, "%s G=%u n=%u K=%u grid=%u: gid %u run %d times\n", name, G, n, K, grid, g,
              (int)seen_gid[g]);
    for (uint32_t s = 0; s < G; ++s)
        for (uint32_t j = 0; j < kSeg; ++j) {
            const int want = j < cnt[s] ? 1 : 0;
            CHECK(seen_q[(size_t)s * kSeg + j] == want, "%s G=%u n=%u: entry %u of segment %u run %d times (want %d)\n",
                  name, G, n, j, s, (int)seen_q[(size_t)s * kSeg + j], want);
        }
}

int main() {
    unsigned seed = 24680u;
    auto rnd = [&](uint32_t m) {
        seed = seed * 1103515245u + 12345u;
        return (seed >> 8) % m;
    };
    const uint32_t Gs[] = {1, 2, 3, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 16384};
    const uint32_t totals[] = {1, 1023, 1024, 1025, 65535, 65536, 65537};
    long cases = 0;
    for (uint32_t G : Gs) {
        auto go = [&](const std::vector<uint32_t> &cnt, const char *name) {
            run(cnt, name);
            ++cases;
        };
        std::vector<uint32_t> c(G);
        go(std::vector<uint32_t>(G, 0u), "all zero");
        go(std::vector<uint32_t>(G, kSeg), "all kSeg");
        const uint32_t where[] = {0, G / 2, G - 1};
        for (uint32_t s : where)
            for (uint32_t val : {1u, rnd(kSeg) + 1, kSeg}) {
                std::fill(c.begin(), c.end(), 0u);
                c[s] = val;
                go(c, "single segment");
            }
        for (int pat = 0; pat < 3; ++pat) {  // a run of zeros: leading, trailing, interior
            const uint32_t len = G < 3 ? 1 : G / 3 + rnd(G / 3);
            const uint32_t b = pat == 0 ? 0 : pat == 1 ? G - std::min(G, len) : (G - std::min(G, len)) / 2;
            for (uint32_t s = 0; s < G; ++s) c[s] = s >= b && s < b + len ? 0u : rnd(kSeg) + 1;
            go(c, pat == 0 ? "leading zeros" : pat == 1 ? "trailing zeros" : "interior zeros");
        }
        for (uint32_t s = 0; s < G; ++s) c[s] = rnd(10) == 0 ? rnd(kSeg) + 1 : 0u;
        go(c, "random sparse");
        for (uint32_t s = 0; s < G; ++s) c[s] = rnd(kSeg + 1);
        go(c, "random dense");
        for (uint32_t s = 0; s < G; ++s) c[s] = rnd(4) == 0 ? 0u : kSeg - rnd(2);  // full or nearly, with holes
        go(c, "nearly full");
        for (uint32_t T : totals) {
            if ((uint64_t)T > (uint64_t)G * kSeg) continue;
            for (int spread = 0; spread < 2; ++spread) {  // packed into few segments / scattered over all
                std::fill(c.begin(), c.end(), 0u);
                uint32_t left = T;
                while (left) {
                    const uint32_t s = rnd(G), room = kSeg - c[s];
                    if (!room) continue;
                    const uint32_t add = std::min(left, spread ? std::min(room, rnd(3) + 1) : room);
                    c[s] += add;
                    left -= add;
                }
                go(c, "exact total");
            }
        }
    }
    std::printf("tail_index (NORI_FINISH_WAVES=%u): %ld launches checked, %ld failures\n", kFinishWaves, cases, fails);
    return fails ? 1 : 0;
}
