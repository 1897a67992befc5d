// shard.cpp -- a rank's share of a sharded render and the watchdog's bounds
// (scene_prep.h), with the entry points that state them without a device.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "scene_prep.h"

namespace nori {

nori_gpu_render_desc shard_of(int W, int H, uint32_t spp, const nori_gpu_render_desc &whole, int mode, int nranks,
                              int rank, std::vector<uint32_t> &blocks) {
    if (nranks < 1 || rank < 0 || rank >= nranks) throw NoriException(NORI_ERR_INVALID, "shard: rank out of range");
    if (mode != NORI_SHARD_PASSES && mode != NORI_SHARD_BLOCKS) throw NoriException(NORI_ERR_INVALID, "shard: unknown mode");
    nori_gpu_render_desc out = whole;
    const uint32_t P = whole.pass_count ? whole.pass_count : std::max<uint32_t>(spp, 1u);
    const uint32_t nb = (uint32_t)(((W + NORI_BLOCK_SIZE - 1) / NORI_BLOCK_SIZE) * ((H + NORI_BLOCK_SIZE - 1) / NORI_BLOCK_SIZE));
    std::vector<char> want(nb, whole.num_blocks ? 0 : 1);
    for (uint32_t i = 0; i < whole.num_blocks; ++i) {
        if (whole.block_ids[i] >= nb) throw NoriException(NORI_ERR_INVALID, "block id out of range");
        want[whole.block_ids[i]] = 1;
    }
    blocks.clear();
    if (mode == NORI_SHARD_PASSES) {
        const uint64_t a = (uint64_t)P * rank / nranks, b = (uint64_t)P * (rank + 1) / nranks;
        out.pass_begin = whole.pass_begin + (uint32_t)a;
        out.pass_count = (uint32_t)(b - a);
        if (whole.num_blocks)  // the restricted frame, each block once, in the caller's order
            for (uint32_t i = 0; i < whole.num_blocks; ++i)
                if (want[whole.block_ids[i]]) {
                    blocks.push_back(whole.block_ids[i]);
                    want[whole.block_ids[i]] = 0;
                }
    } else {
        uint32_t k = 0;  // round-robin over the spiral order (block.cpp:140-188)
        for (uint32_t b : spiral_blocks(W, H))
            if (want[b] && (k++ % (uint32_t)nranks) == (uint32_t)rank) blocks.push_back(b);
        out.pass_count = blocks.empty() ? 0 : P;  // no block of this rank: an empty share
    }
    out.num_blocks = (uint32_t)blocks.size();
    out.block_ids = blocks.empty() ? nullptr : blocks.data();
    return out;
}

// Samples of a share (pass count x pixels of its blocks, or of the image).
double share_samples(int W, int H, const nori_gpu_render_desc &s) {
    if (!s.num_blocks) return (double)s.pass_count * W * H;
    const int nx = (W + NORI_BLOCK_SIZE - 1) / NORI_BLOCK_SIZE;
    double px = 0;
    for (uint32_t i = 0; i < s.num_blocks; ++i) {
        const int bx = (int)(s.block_ids[i] % (uint32_t)nx), by = (int)(s.block_ids[i] / (uint32_t)nx);
        px += (double)std::min(NORI_BLOCK_SIZE, W - bx * NORI_BLOCK_SIZE) * std::min(NORI_BLOCK_SIZE, H - by * NORI_BLOCK_SIZE);
    }
    return px * s.pass_count;
}

// Watchdog of the collectives of a sharded render: how long a rank waits in
// the status exchange or the film sum for its peers before it aborts the
// communicator.  Only a peer that cannot join at all (its device faulted,
// its process died) is waited for: every other failure reaches the peers
// through the status exchange.  NORI_COMM_TIMEOUT_S fixes the bound;
// otherwise, for a rank that rendered its share (status NORI_OK), it scales
// with the frame: max(30 s, 20 x this rank's own render time x largest share
// / own share), since every peer renders a share of about the same size with
// the same code.  A rank whose own render failed or was cancelled, or that
// has no share, has no render time that says how long its peers need: it
// waits up to 600 s.
double comm_timeout_s(int status, double own_s, double own_samples, double max_samples) {
    if (const char *e = std::getenv("NORI_COMM_TIMEOUT_S")) {
        const double v = std::atof(e);
        if (v > 0.0) return v;
    }
    if (status != NORI_OK || !(own_samples > 0.0)) return 600.0;
    return std::max(30.0, 20.0 * own_s * std::max(1.0, max_samples / own_samples));
}

// Status word of the exchange: severity << 16 | rank, reduced by max over the
// ranks, so the worst outcome wins and names its rank (the highest of equals).
// Severity 0 rendered, 1 cancelled, 2 failed.
int comm_status_word(int rc, int rank) {
    const int sev = rc == NORI_OK ? 0 : (rc == NORI_ERR_CANCELLED ? 1 : 2);
    return (sev << 16) | (rank & 0xFFFF);
}

}  // namespace nori

using namespace nori;

extern "C" {

int nori_gpu_shard_desc(const nori_scene_desc *d, const nori_gpu_render_desc *rd, int mode, int nranks, int rank,
                        nori_gpu_render_desc *out, uint32_t *block_buf) {
    return guarded([&] {
        if (!d || !rd || !out || (rd->num_blocks && !rd->block_ids)) return fail(NORI_ERR_INVALID, "null argument");
        std::vector<uint32_t> blocks;
        nori_gpu_render_desc s =
            shard_of(d->camera.width, d->camera.height, d->sample_count, *rd, mode, nranks, rank, blocks);
        if (!blocks.empty()) {
            if (!block_buf) return fail(NORI_ERR_INVALID, "block_buf is null");
            std::memcpy(block_buf, blocks.data(), 4 * blocks.size());
            s.block_ids = block_buf;
        } else {
            s.block_ids = nullptr;
        }
        *out = s;
        return (int)NORI_OK;
    });
}

int nori_gpu_comm_status_word(int rc, int rank) { return comm_status_word(rc, rank); }
double nori_gpu_comm_timeout(int status, double own_seconds, double own_samples, double max_samples) {
    return comm_timeout_s(status, own_seconds, own_samples, max_samples);
}

}  // extern "C"
