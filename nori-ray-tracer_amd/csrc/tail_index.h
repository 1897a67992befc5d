// tail_index.h -- how the tail finisher (k_finish, kernels_finish.hip) numbers
// the paths still queued: plain integer arithmetic, host-compilable like
// seg_index.h, so that tests/test_tail_index.py can check with g++ that the
// waves a launch starts cover every queued path exactly once and that no lane
// addresses a queue entry outside its segment's count.
//
// The queued paths of the G segments are numbered 0 .. n-1 through the
// exclusive prefix `pre` of the segment counts (pre[G] = n, k_tail_prefix).
// Wave w takes the K consecutive paths from w * K on, lane l path w * K + l
// (lanes >= K idle); path gid lies in the last segment s with pre[s] <= gid,
// at slot gid - pre[s] of it.  Each count is <= kSeg, so n <= kSeg * G.
#pragma once
#include <stdint.h>

#include "seg_index.h"

namespace nori {

#ifndef NORI_FINISH_WAVES  // 0: 64 paths per wave
// 2048 since the glass-sphere chain (round 3): fewer finisher waves leave the
// film splat beside it more of the chip; 64-spp share 3446 -> 3550 (4096) ->
// 3652 (2048) Msamples/s, 512 spp 4737 -> 4753 / 4744 (one box, interleaved).
// 1024 since round 6's shorter glass chain: 64-spp share 4677 -> 4725 (4
// reps, every 1024 run above every 2048 run), 512 spp 5843 / 5834 (noise)
#define NORI_FINISH_WAVES 1024
#endif
constexpr uint32_t kFinishWaves = NORI_FINISH_WAVES;

NORI_SEG_FN uint32_t tail_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
NORI_SEG_FN uint32_t tail_max(uint32_t a, uint32_t b) { return a > b ? a : b; }

// Segments per thread of k_tail_prefix's one work-group of 1024 threads
// (thread t owns segments [t per, min(G, (t + 1) per))): G / 1024 rounded up.
NORI_SEG_FN uint32_t tail_prefix_per(uint32_t G) { return (G + 1023) / 1024; }
// Paths per wave for n queued paths: n / kFinishWaves rounded up, within
// [1, 64], so the tail spreads over about kFinishWaves waves.
NORI_SEG_FN uint32_t tail_paths_per_wave(uint32_t n) {
    constexpr uint32_t w = kFinishWaves ? kFinishWaves : 1u;
    return kFinishWaves ? tail_min(64u, tail_max(1u, (n + w - 1) / w)) : 64u;
}
// Work-groups of the finisher over G segments, wpb waves per work-group:
// enough waves for any path count n <= kSeg * G = 256 G (kFinishWaves of
// them while K < 64; n / 64 <= 4 G when K = 64, and 2 G work-groups of
// kSeg / 2 threads hold 4 G waves).
NORI_SEG_FN uint32_t tail_grid(uint32_t G, uint32_t wpb) { return tail_max(2 * G, (kFinishWaves + wpb - 1) / wpb); }
// First path of the wave that holds thread `tid` (numbered through the whole
// launch); its lane l < K takes path tail_first + l.  A wave (or a whole
// work-group, by its first thread) with tail_first >= n has no path.
NORI_SEG_FN uint32_t tail_first(uint32_t tid, uint32_t K) { return tid / 64 * K; }
// First path of work-group `bid` of wpb waves (= tail_first of its first thread).
NORI_SEG_FN uint32_t tail_block_first(uint32_t bid, uint32_t wpb, uint32_t K) { return bid * wpb * K; }
// Segment of path gid < pre[G]: the last s < G with pre[s] <= gid (never an
// empty segment: pre[s + 1] > gid).
NORI_SEG_FN uint32_t tail_segment(const uint32_t *pre, uint32_t G, uint32_t gid) {
    uint32_t lo = 0, hi = G;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (pre[mid] <= gid) lo = mid;
        else hi = mid;
    }
    return lo;
}
// Queue index of path gid of segment sg = tail_segment(pre, G, gid).
NORI_SEG_FN uint32_t tail_slot(const uint32_t *pre, uint32_t sg, uint32_t gid) { return sg * kSeg + gid - pre[sg]; }

}  // namespace nori
