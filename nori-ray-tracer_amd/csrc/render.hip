// render.hip -- nori_gpu_render: the wavefront loop and the one-bounce integrators.
//
// nori_gpu_render replaces RenderThread::renderScene's pass loop
// (render.cpp:173-250): instead of spp sequential passes of a
// tbb::parallel_for over 32x32 blocks, every (pass, pixel) sample of the
// requested blocks becomes a work id; a pool of paths stays resident in HBM
// and the shade kernel refills finished slots from a device work counter, so
// the GPU stays full until the last sample.  Radiance accumulates per sample
// record; after the pool drains, k_splat applies ImageBlock::put.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"

namespace nori {
namespace {

void ensure_pool(nori_gpu_ctx &c, uint32_t pool) {
    if (pool <= c.pool_cap) return;
    for (int b = 0; b < 2; ++b) {
        c.q[b][0].ensure(16 * (size_t)pool);
        c.q[b][1].ensure(16 * (size_t)pool);
        c.q[b][2].ensure(16 * (size_t)pool);
        c.q[b][3].ensure(16 * (size_t)pool);
        c.q[b][4].ensure(4 * (size_t)pool);
    }
    for (int k = 0; k < 3; ++k) c.sq[k].ensure(16 * (size_t)pool);
    for (int k = 0; k < 4; ++k) c.seg[k].ensure(4 * (size_t)(pool / kSeg));
    c.segstats.ensure(16 * (size_t)(pool / kSeg));
    c.tailpre.ensure(4 * (size_t)(pool / kSeg + 1));
    c.pool_cap = pool;
}

PathQueue queue_of(nori_gpu_ctx &c, int b) {
    PathQueue q;
    q.ray_o = c.q[b][0].as<float4>();
    q.ray_d = c.q[b][1].as<float4>();
    q.hit = c.q[b][2].as<float4>();
    q.thr = c.q[b][3].as<float4>();
    q.rng = c.q[b][4].as<uint32_t>();
    return q;
}

constexpr int kRing = 16;     // readback ring entries
constexpr int kLookahead = 6;    // iterations queued ahead of the termination check
constexpr int kLookaheadEnd = 2; // ... once work streams run dry
// NORI_LOOKAHEAD=n (0 .. 8) replaces kLookahead.  The termination check reads
// the done flag as the device has set it by now, which may be up to `lag`
// iterations further than the event just waited for: how many iterations a
// render launches past the one that handed out the last work id (and so how
// its rays divide between the loop and the finisher) depends on how far the
// host runs ahead of the device.  With 0 the host waits for every iteration
// before it reads the flag, and the counts are the same in every run (the
// tests that compare two renders' statistics exactly use it).
int lookahead() {
    const char *e = std::getenv("NORI_LOOKAHEAD");
    const int v = e ? std::atoi(e) : kLookahead;
    return v < 0 ? 0 : v > 8 ? 8 : v;
}

// NORI_POOL_PARTS: independent pool parts on their own streams (1..kMaxParts).
// Default 3: each part's launches wait for their own slowest walks / longest
// lanes, and three streams keep the chip busy in between (C3: 2 parts 619,
// 3 parts 651, 4 parts 499 Msamples/s -- 4 streams exceed the hardware
// queues; table scene 517 -> 555; C2 4563 -> 4658; 64-spp share 3026 ->
// 3089; C4 and C5 within 1 %).
// Renders whose shade kernel traces its own extension rays (ext_loop): 2.
// An iteration is one launch there, so no part's scan is left to slip under
// another part's shade launch (C2, 1M pool: 2 parts 6529-6637 Msamples/s;
// 2M pool: 1 part 5579-5615, 2 parts 6404-6460, 3 parts 6311-6410).
uint32_t pool_parts(bool ext_loop) {
    const uint32_t def = ext_loop ? 2u : 3u;
    const char *e = std::getenv("NORI_POOL_PARTS");
    const long v = e ? std::atol(e) : (long)def;
    return (uint32_t)(v >= 1 && v <= kMaxParts ? v : def);
}
// Sample passes folded by one splat work-group.  Default: about one
// work-group per CU over the whole launch (passes x blocks / 256), so the
// splat leaves most of the chip to the tail finisher it overlaps with
// (cbox 512x512@512: 256 blocks x 512 passes per work-group, splat 3.0 ms and
// finisher 3.6 ms vs 4.7 / 5.2 ms at 32 passes).  NORI_SPLAT_PASSES overrides.
// The one-bounce integrators' splat has no finisher beside it: it targets
// 4096 work-groups instead.
uint32_t splat_passes(uint32_t np, size_t nblocks, uint32_t target_wgs = 256) {
    const char *e = std::getenv("NORI_SPLAT_PASSES");
    long v = e ? std::atol(e) : (long)(((uint64_t)np * nblocks + target_wgs - 1) / target_wgs);
    if (v < 1) v = 1;
    return (uint32_t)std::min<long>(v, np);
}
// Per-pixel sample statistics (render_desc.variance_out): the device buffer
// the kernels add into -- the caller's own when it is device memory, else a
// zeroed scratch buffer that var_finish adds into the host array.
float *var_begin(nori_gpu_ctx &c, const nori_gpu_render_desc &rd) {
    if (!rd.variance_out) return nullptr;
    if (rd.output_on_device) return rd.variance_out;
    const size_t n = 8 * (size_t)c.S.W * (size_t)c.S.H;
    c.varbuf.ensure(n * sizeof(float));
    HIP_TRY(hipMemsetAsync(c.varbuf.p, 0, n * sizeof(float), c.stream));
    return c.varbuf.as<float>();
}
void var_finish(nori_gpu_ctx &c, const nori_gpu_render_desc &rd, bool cancelled) {
    if (!rd.variance_out || rd.output_on_device || cancelled) return;
    const size_t n = 8 * (size_t)c.S.W * (size_t)c.S.H;
    std::vector<float> h(n);
    HIP_TRY(hipMemcpy(h.data(), c.varbuf.p, n * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) rd.variance_out[i] += h[i];
}

// normals / av / direct*: no path pool -- per chunk of passes, k_direct runs
// every sample start to end and writes its record, then k_splat filters them.
int render_one_bounce(nori_gpu_ctx &c, const nori_gpu_render_desc &rd, const std::vector<uint32_t> &pixels,
                      const std::vector<int4> &blocks, float *rgbw_out, nori_gpu_stats *stats,
                      std::chrono::steady_clock::time_point t0) {
    const DevScene &S = c.S;
    const int W = S.W, H = S.H, B = S.border;
    const uint32_t M = (uint32_t)pixels.size(), passes = rd.pass_count;
    const size_t rec_budget = (size_t)4 << 30;
    uint32_t chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(passes, rec_budget / (16 * (size_t)M)));
    // work ids (record indices) < 2^29: the path queue keeps a chromatic
    // sample's colour channel in bits 29-30 of the same word (kWorkMask)
    chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(chunk, ((uint64_t)1 << kChanShift) / M));
    c.rec.ensure(16 * (size_t)chunk * M);
    c.counters.ensure(sizeof(Counters));
    const size_t film_elems = 4 * (size_t)(W + 2 * B) * (H + 2 * B);
    float *film = nullptr;
    if (rd.output_on_device) {
        film = rgbw_out;
    } else {
        c.film.ensure(film_elems * sizeof(float));
        film = c.film.as<float>();
        HIP_TRY(hipMemsetAsync(film, 0, film_elems * sizeof(float), c.stream));
    }
    Counters *C = c.counters.as<Counters>();
    HIP_TRY(hipMemsetAsync(C, 0, sizeof(Counters), c.stream));
    if (!c.in_rounds) c.cancel = 0;
    c.report(0.0);
    Timers tm;
    const bool timing = rd.timing != 0;
    double kms[2] = {0, 0};
    std::vector<std::array<hipEvent_t, 3>> spans;
    uint64_t done = 0;
    bool cancelled = false;
    float *var = var_begin(c, rd);
    for (uint32_t p0 = 0; p0 < passes; p0 += chunk) {
        if (c.cancel.load()) {
            cancelled = true;
            break;
        }
        const uint32_t np = std::min(chunk, passes - p0);
        WorkDesc wd{(uint64_t)np * M, M, rd.pass_begin + p0, c.pixels.as<uint32_t>(), rd.seed, 0, nullptr, 1, 0, var};
        SplatDesc sd{M, np, rd.pass_begin + p0, std::max<uint32_t>(1, splat_passes(np, blocks.size(), 4096)), c.blocks.as<int4>(),
                     rd.seed, var};
        std::array<hipEvent_t, 3> ev{};
        if (timing) {
            for (auto &e : ev) e = tm.get();
            HIP_TRY(hipEventRecord(ev[0], c.stream));
        }
        HIP_TRY(launch_direct(S, wd, c.rec.as<float4>(), C, c.stack, c.stream));
        if (timing) HIP_TRY(hipEventRecord(ev[1], c.stream));
        HIP_TRY(launch_splat(S, c.rec.as<float4>(), sd, (uint32_t)blocks.size(), film, C, c.stream));
        if (timing) {
            HIP_TRY(hipEventRecord(ev[2], c.stream));
            spans.push_back(ev);
        }
        HIP_TRY(hipStreamSynchronize(c.stream));
        done += wd.total;
        c.report((double)(p0 + np) / passes);
    }
    Counters hc;
    HIP_TRY(hipMemcpyAsync(&hc, C, sizeof(Counters), hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    for (const auto &e : spans) {
        float a = 0, b = 0;
        HIP_TRY(hipEventElapsedTime(&a, e[0], e[1]));
        HIP_TRY(hipEventElapsedTime(&b, e[1], e[2]));
        kms[0] += a;
        kms[1] += b;
    }
    if (!rd.output_on_device && !cancelled) {
        std::vector<float> hf(film_elems);
        HIP_TRY(hipMemcpy(hf.data(), film, film_elems * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < film_elems; ++i) rgbw_out[i] += hf[i];
    }
    var_finish(c, rd, cancelled);
    c.report(1.0);
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        scene_stats(c, t0, stats);
        stats->samples = done;
        stats->invalid_samples = hc.invalid;
        stats->rays_closest = hc.direct_rays[0];
        stats->rays_shadow = hc.direct_rays[1];
        stats->iterations = 0;
        stats->stream_parts = 1;
        stats->ms_shade = kms[0];  // k_direct: the whole integrator
        stats->ms_splat = kms[1];
    }
    if (cancelled) return fail(NORI_ERR_CANCELLED, "rendering was cancelled");
    return NORI_OK;
}

}  // namespace

// The render's blocks in BlockGenerator order (block.cpp:140-188) with the
// block_subset applied, and the block-major pixel list (camera samples of one
// block are adjacent work ids); cached on the context with their device
// copies, so a render of the same selection neither rebuilds nor uploads them.
void work_lists(nori_gpu_ctx &c, const nori_gpu_render_desc &rd) {
    const int W = c.S.W, H = c.S.H;
    const int nbx = (int)std::ceil(W / (float)NORI_BLOCK_SIZE), nby = (int)std::ceil(H / (float)NORI_BLOCK_SIZE);
    std::vector<uint32_t> order = spiral_blocks(W, H);
    if (rd.num_blocks) {
        std::vector<char> want((size_t)nbx * nby, 0);
        for (uint32_t i = 0; i < rd.num_blocks; ++i) {
            if (rd.block_ids[i] >= (uint32_t)(nbx * nby)) throw NoriException(NORI_ERR_INVALID, "block id out of range");
            want[rd.block_ids[i]] = 1;
        }
        std::vector<uint32_t> sel;
        for (uint32_t b : order)
            if (want[b]) sel.push_back(b);
        order.swap(sel);
    }
    if (c.work_valid && order == c.work_order) return;
    c.work_valid = false;
    c.hpixels.clear();
    c.hblocks.clear();
    for (uint32_t b : order) {
        int bx = (int)(b % (uint32_t)nbx), by = (int)(b / (uint32_t)nbx);
        int ox = bx * NORI_BLOCK_SIZE, oy = by * NORI_BLOCK_SIZE;
        int bw = std::min(NORI_BLOCK_SIZE, W - ox), bh = std::min(NORI_BLOCK_SIZE, H - oy);
        c.hblocks.push_back(make_int4(ox, oy, bw | (bh << 16), (int)c.hpixels.size()));
        for (int y = 0; y < bh; ++y)
            for (int x = 0; x < bw; ++x) c.hpixels.push_back((uint32_t)((oy + y) * W + (ox + x)));
    }
    c.pixels.upload(c.hpixels);
    c.blocks.upload(c.hblocks);
    c.work_order.swap(order);
    c.work_valid = true;
}

int render(nori_gpu_ctx &c, const nori_gpu_render_desc &rd, float *rgbw_out, nori_gpu_stats *stats) {
    auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(c.device));
    const DevScene &S = c.S;
    const int W = S.W, H = S.H, B = S.border;
    work_lists(c, rd);
    const std::vector<uint32_t> &pixels = c.hpixels;
    const std::vector<int4> &blocks = c.hblocks;
    const uint32_t M = (uint32_t)pixels.size();
    const uint32_t passes = rd.pass_count ? rd.pass_count : 0;
    if (passes == 0 || M == 0) throw NoriException(NORI_ERR_INVALID, "nothing to render (pass_count or blocks empty)");
    const bool one_bounce = S.integrator >= NORI_INTEGRATOR_NORMALS;
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
    if (one_bounce) return render_one_bounce(c, rd, pixels, blocks, rgbw_out, stats, t0);
    if (M > kWorkMask) throw NoriException(NORI_ERR_INVALID, "frame too large: more than 2^29 pixels per pass");
    const bool timing = rd.timing != 0;
    // S.ext_inline: an iteration is the shade launch alone.  A timing render
    // keeps the two launches (one event span per kernel), so its shade kernel
    // reads the hits as without the flag, and it keeps the pool and the parts
    // of the two-launch loop.
    const bool ext_loop = S.ext_inline != 0 && !timing;
    uint32_t pool = rd.path_pool;
    if (!pool) {  // NORI_PATH_POOL: default pool size override (tuning)
        const char *e = std::getenv("NORI_PATH_POOL");
        if (e && std::atol(e) > 0) {
            pool = (uint32_t)std::min<long>(std::atol(e), 1L << 26);
        } else {
            const uint64_t want = (uint64_t)passes * M / (c.stack ? 8 : 16);
            pool = 1u << 20;
            while (!ext_loop && pool < (1u << 22) && pool < want) pool <<= 1;
        }
    }
    pool = std::max<uint32_t>(kSeg, (pool + kSeg - 1) / kSeg * kSeg);
    ensure_pool(c, pool);
    // sample-record budget: chunks of passes, each < 2^31 records
    const size_t rec_budget = (size_t)6 << 30;
    uint32_t chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(passes, rec_budget / (16 * (size_t)M)));
    // work ids (record indices) < 2^29: the path queue keeps a chromatic
    // sample's colour channel in bits 29-30 of the same word (kWorkMask)
    chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(chunk, ((uint64_t)1 << kChanShift) / M));
    c.rec.ensure(16 * (size_t)chunk * M);
    c.counters.ensure(sizeof(Counters));
    const size_t film_elems = 4 * (size_t)(W + 2 * B) * (H + 2 * B);
    float *film = nullptr;
    if (rd.output_on_device) {
        film = rgbw_out;
    } else {
        c.film.ensure(film_elems * sizeof(float));
        film = c.film.as<float>();
        HIP_TRY(hipMemsetAsync(film, 0, film_elems * sizeof(float), c.stream));
    }
    if (!c.pinned) {
        // host-mapped, coherent: the shade kernel stores the completion flag here
        HIP_TRY(hipHostMalloc((void **)&c.pinned, 256, hipHostMallocMapped | hipHostMallocCoherent));
        HIP_TRY(hipHostGetDevicePointer((void **)&c.pinned_dev, c.pinned, 0));
        for (auto &r : c.ring) {
            r.resize(kRing);
            for (auto &e : r) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
    }
    Counters *C = c.counters.as<Counters>();
    ShadowQueue sq{c.sq[0].as<float4>(), c.sq[1].as<float4>(), c.sq[2].as<float4>()};
    PathQueue Q[2] = {queue_of(c, 0), queue_of(c, 1)};
    if (!c.in_rounds) c.cancel = 0;
    c.report(0.0);
    const uint64_t total_all = (uint64_t)passes * M;
    uint64_t done_before = 0, rays_c = 0, rays_s = 0, invalid = 0, iters = 0;
    Timers tm;
    struct Span {
        hipEvent_t a, b;
        int kind;
    };
    std::vector<Span> spans;
    DevScene Sk = S;
    if (!ext_loop) Sk.ext_inline = 0;
    auto timed_on = [&](hipStream_t st, int kind, auto &&launch) {
        if (!timing) {
            HIP_TRY(launch());
            return;
        }
        Span s{tm.get(), tm.get(), kind};
        HIP_TRY(hipEventRecord(s.a, st));
        HIP_TRY(launch());
        HIP_TRY(hipEventRecord(s.b, st));
        spans.push_back(s);
    };
    auto timed = [&](int kind, auto &&launch) { timed_on(c.stream, kind, launch); };
    bool cancelled = false;
    const uint32_t parts = std::max<uint32_t>(1, std::min<uint32_t>(pool_parts(ext_loop), pool / kSeg));
    const uint32_t G = pool / kSeg;
    SegState seg{{c.seg[0].as<uint32_t>(), c.seg[1].as<uint32_t>()}, c.seg[2].as<uint32_t>(), c.seg[3].as<uint32_t>(),
                 c.segstats.as<uint4>()};
    std::vector<uint4> hstats(G);
    uint64_t finish_rays = 0, samples_started = 0;
    float *var = var_begin(c, rd);
    for (uint32_t p0 = 0; p0 < passes && !cancelled; p0 += chunk) {
        uint32_t np = std::min(chunk, passes - p0);
        WorkDesc wd{(uint64_t)np * M, M, rd.pass_begin + p0, c.pixels.as<uint32_t>(), rd.seed, G, c.pinned_dev, 1, 0,
                    var};
        wd.rot = stream_rotation(wd.total, M, G);
        __atomic_store_n(&c.pinned[0], 0u, __ATOMIC_RELEASE);
        __atomic_store_n(&c.pinned[1], 0u, __ATOMIC_RELEASE);
        // segments whose stream is empty from the start count as exhausted
        uint32_t empty = 0;
        for (uint32_t b = 0; b < G; ++b) empty += stream_work(wd, b, 0) >= wd.total;
        HIP_TRY(launch_reset(C, empty, seg, G, c.stream));
        int last_out = 0;
        // The pool is split into `parts` independent parts (segments never
        // interact), each driven on its own stream: the memory-bound shade
        // launch of one part overlaps the VALU-bound traversal of another.
        std::vector<uint32_t> Gp(parts), base(parts);
        for (uint32_t h = 0; h < parts; ++h) {
            base[h] = (uint32_t)((uint64_t)G * h / parts);
            Gp[h] = (uint32_t)((uint64_t)G * (h + 1) / parts) - base[h];
        }
        auto q_view = [&](const PathQueue &q, uint32_t b0) {
            const size_t e = (size_t)b0 * kSeg;
            return PathQueue{q.ray_o + e, q.ray_d + e, q.hit + e, q.thr + e, q.rng + e};
        };
        std::vector<std::array<PathQueue, 2>> Qh(parts);
        std::vector<ShadowQueue> sqh(parts);
        std::vector<SegState> segh(parts);
        std::vector<WorkDesc> wdh(parts);
        for (uint32_t h = 0; h < parts; ++h) {
            Qh[h][0] = q_view(Q[0], base[h]);
            Qh[h][1] = q_view(Q[1], base[h]);
            const size_t e = (size_t)base[h] * kSeg;
            sqh[h] = ShadowQueue{sq.ray_o + e, sq.ray_d + e, sq.payload + e};
            segh[h] = SegState{{seg.cnt[0] + base[h], seg.cnt[1] + base[h]}, seg.shcnt + base[h],
                               seg.cursor + base[h], seg.stats + base[h]};
            wdh[h] = wd;
            wdh[h].b0 = base[h];
        }
        HIP_TRY(hipEventRecord(c.fork, c.stream));  // the part streams start after the resets above
        for (uint32_t h = 1; h < parts; ++h) HIP_TRY(hipStreamWaitEvent(c.parts[h], c.fork, 0));
        uint64_t lag = (uint64_t)lookahead();
        // NORI_DEBUG: host time spent enqueuing vs waiting on the ring events
        // (a wait that returns at once means the device ran dry of work)
        const bool dbg = debug_log();
        double t_enq = 0.0, t_wait = 0.0;
        uint32_t idle_waits = 0;
        auto now_us = [] {
            return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
        };
        for (uint64_t it = 0;; ++it) {
            const double te0 = dbg ? now_us() : 0.0;
            int in = (int)(it & 1), out = in ^ 1;
            last_out = out;
            for (uint32_t h = 0; h < parts; ++h) {
                hipStream_t st = h ? c.parts[h] : c.stream;
                const SegState &sg = segh[h];
                timed_on(st, 2, [&] {
                    return launch_shade(Sk, Qh[h][in], Qh[h][out], sqh[h], sg, in, wdh[h], c.rec.as<float4>(), C,
                                        Gp[h], st, &c.shade_rtc);
                });
                hipError_t both_err = hipSuccess;
                if (S.nee_inline) {  // the shadow rays were traced by k_shade itself
                    if (ext_loop) continue;  // ... and so will the next vertex's extension ray be
                    timed_on(st, 0, [&] { return launch_extend(S, Qh[h][out], sg.cnt[out], Gp[h], c.stack, st, &c.rtc); });
                    continue;
                }
                if (!timing && c.fuse_trace &&
                    launch_trace_both(S, Qh[h][out], sg.cnt[out], sqh[h], sg.shcnt, c.rec.as<float4>(), Gp[h], c.stack,
                                      &c.rtc, st, both_err)) {
                    HIP_TRY(both_err);  // (the timed renders keep two launches: one event span per kernel)
                    continue;
                }
                timed_on(st, 0, [&] { return launch_extend(S, Qh[h][out], sg.cnt[out], Gp[h], c.stack, st, &c.rtc); });
                timed_on(st, 1, [&] {
                    return launch_shadow(S, sqh[h], sg.shcnt, c.rec.as<float4>(), Gp[h], c.stack, st, &c.rtc);
                });
            }
            ++iters;
            // an event per iteration; the host waits on the one from `lag`
            // iterations back
            const uint64_t ev = it;
            for (uint32_t h = 0; h < parts; ++h)
                HIP_TRY(hipEventRecord(c.ring[h][ev % kRing], h ? c.parts[h] : c.stream));
            const double te1 = dbg ? now_us() : 0.0;
            t_enq += te1 - te0;
            if (ev >= lag) {
                for (uint32_t h = 0; h < parts; ++h) HIP_TRY(hipEventSynchronize(c.ring[h][(ev - lag) % kRing]));
                if (dbg) {
                    const double w = now_us() - te1;
                    t_wait += w;
                    idle_waits += w < 5.0 ? 1u : 0u;
                }
                uint32_t exhausted = __atomic_load_n(&c.pinned[1], __ATOMIC_ACQUIRE);
                // the streams are running dry: queue fewer iterations ahead,
                // so that few drain iterations (full-grid launches over a
                // thinning pool) are already queued when the last one does
                if (exhausted) lag = std::min<uint64_t>(lag, kLookaheadEnd);
                c.report(std::min(1.0, (double)done_before / (double)total_all +
                                           (double)np / passes * exhausted / G));
                // every work id has been handed out: finish the remaining paths in one launch
                if (__atomic_load_n(&c.pinned[0], __ATOMIC_ACQUIRE)) break;
                if (c.cancel.load()) {
                    cancelled = true;
                    break;
                }
            }
        }
        // ext_loop: the last iteration's survivors and new samples have no hits
        // yet; the finisher below reads them, so they are traced once here
        for (uint32_t h = 0; ext_loop && !cancelled && h < parts; ++h)
            HIP_TRY(launch_extend(S, Qh[h][last_out], segh[h].cnt[last_out], Gp[h], c.stack, h ? c.parts[h] : c.stream,
                                  &c.rtc));
        for (uint32_t h = 1; h < parts; ++h) {  // join: the tail below runs on the whole pool
            HIP_TRY(hipEventRecord(c.joins[h], c.parts[h]));
            HIP_TRY(hipStreamWaitEvent(c.stream, c.joins[h], 0));
        }
        if (cancelled) break;
        // The samples still in flight are marked pending; the film splat of all
        // the others runs on the side stream while the finisher completes the
        // pending ones and splats each itself.
        hipStream_t splat_st = c.side;
        HIP_TRY(launch_mark(Q[last_out], seg, last_out, c.rec.as<float4>(), G, c.stream));
        HIP_TRY(launch_tail_prefix(seg, last_out, G, c.tailpre.as<uint32_t>(), c.stream));
        HIP_TRY(hipEventRecord(c.fork, c.stream));
        HIP_TRY(hipStreamWaitEvent(c.side, c.fork, 0));
        SplatDesc sd{M, np, rd.pass_begin + p0, std::max<uint32_t>(1, splat_passes(np, blocks.size())),
                     c.blocks.as<int4>(), rd.seed, var};
        auto splat = [&] {
            timed_on(splat_st, 3, [&] { return launch_splat(S, c.rec.as<float4>(), sd, (uint32_t)blocks.size(), film, C, splat_st); });
        };
        auto finish = [&] {
            timed(4, [&] {
                return launch_finish(S, Q[last_out], seg, last_out, c.rec.as<float4>(), wd, film, C, G, c.stack,
                                     c.tailpre.as<uint32_t>(), c.stream);
            });
        };
        // both wait for the same fork; the finisher's waves are enqueued first
        // (c.finish_first) so that they are resident before the splat fills the CUs
        if (c.finish_first) {
            finish();
            splat();
        } else {
            splat();
            finish();
        }
        HIP_TRY(hipEventRecord(c.join, c.side));
        HIP_TRY(hipStreamWaitEvent(c.stream, c.join, 0));
        // read-back through pinned staging: both copies queue behind the
        // finisher without a host round trip each (pageable copies stage twice)
        const size_t rb = sizeof(Counters) + 16 * (size_t)G;
        if (c.readback_bytes < rb) {
            if (c.readback) HIP_TRY(hipHostFree(c.readback));
            c.readback = nullptr;
            c.readback_bytes = 0;
            HIP_TRY(hipHostMalloc((void **)&c.readback, rb, hipHostMallocDefault));
            c.readback_bytes = rb;
        }
        HIP_TRY(hipMemcpyAsync(c.readback, C, sizeof(Counters), hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipMemcpyAsync(c.readback + sizeof(Counters), seg.stats, 16 * (size_t)G, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
        Counters hc;
        std::memcpy(&hc, c.readback, sizeof(Counters));
        std::memcpy(hstats.data(), c.readback + sizeof(Counters), 16 * (size_t)G);
        for (const uint4 &st : hstats) {
            rays_c += st.x;
            rays_s += st.y;
            samples_started += st.z;
            finish_rays += st.w;
        }
        invalid += hc.invalid;
        if (debug_log())
        {
            std::fprintf(stderr, "[nori] chunk %u: %lu iterations, finisher %u paths, longest %u rays\n", p0,
                         (unsigned long)iters, hc.finish_paths, hc.finish_max_rays);
            std::fprintf(stderr, "[nori] host loop: %.0f us enqueuing, %.0f us waiting; %u of the waits returned at once\n",
                         t_enq, t_wait, idle_waits);
            if (hc.prof[6])  // NORI_PROF_SHADE builds
                std::fprintf(stderr, "[nori] shade clocks per wave: loads %.0f shade %.0f compact %.0f store %.0f regen %.0f drain %.0f (%llu waves)\n",
                             (double)hc.prof[0] / hc.prof[6], (double)hc.prof[1] / hc.prof[6],
                             (double)hc.prof[2] / hc.prof[6], (double)hc.prof[3] / hc.prof[6],
                             (double)hc.prof[4] / hc.prof[6], (double)hc.prof[5] / hc.prof[6], hc.prof[6]);
            else if (hc.prof[4])  // NORI_PROF_FINISH builds
                std::fprintf(stderr, "[nori] finisher clocks per wave-iteration: shade %.0f shadow %.0f splat %.0f extend %.0f (%llu); "
                             "longest wave %.3f ms over %llu iterations\n",
                             (double)hc.prof[0] / hc.prof[4], (double)hc.prof[1] / hc.prof[4],
                             (double)hc.prof[2] / hc.prof[4], (double)hc.prof[3] / hc.prof[4], hc.prof[4],
                             (double)(hc.prof[5] >> 20) * 1e-5, hc.prof[5] & 0xFFFFFull);
            if (hc.prof[14])  // NORI_PROF_GLASS builds
                std::fprintf(stderr, "[nori] lone-lane glass chains: %llu chord bounces, %.0f ns each\n", hc.prof[14],
                             10.0 * hc.prof[13] / hc.prof[14]);
            if (hc.prof[12])
                std::fprintf(stderr, "[nori] finisher late iterations (lone lanes): shade %.0f shadow %.0f splat %.0f extend %.0f ns (%llu)\n",
                             10.0 * hc.prof[8] / hc.prof[12], 10.0 * hc.prof[9] / hc.prof[12],
                             10.0 * hc.prof[10] / hc.prof[12], 10.0 * hc.prof[11] / hc.prof[12], hc.prof[12]);
        }
        done_before += wd.total;
    }
    if (samples_started != done_before && !cancelled)
        throw NoriException(NORI_ERR_INVALID, "internal: started " + std::to_string(samples_started) + " of " +
                                                  std::to_string(done_before) + " samples");
    double kms[5] = {0, 0, 0, 0, 0};
    if (timing) {
        HIP_TRY(hipStreamSynchronize(c.stream));
        for (const Span &s : spans) {
            float ms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&ms, s.a, s.b));
            kms[s.kind] += ms;
        }
    }
    if (!rd.output_on_device && !cancelled) {
        std::vector<float> hf(film_elems);
        HIP_TRY(hipMemcpy(hf.data(), film, film_elems * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < film_elems; ++i) rgbw_out[i] += hf[i];
    }
    var_finish(c, rd, cancelled);
    HIP_TRY(hipStreamSynchronize(c.stream));
    HIP_TRY(hipStreamSynchronize(c.side));
    for (int h = 1; h < kMaxParts; ++h) HIP_TRY(hipStreamSynchronize(c.parts[h]));
    c.report(1.0);
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        scene_stats(c, t0, stats);
        stats->samples = done_before;
        stats->invalid_samples = invalid;
        stats->rays_closest = rays_c;
        stats->rays_shadow = rays_s;
        stats->iterations = iters;
        stats->stream_parts = parts;
        stats->path_pool = pool;
        stats->ms_extend = kms[0];
        stats->ms_shadow = kms[1];
        stats->ms_shade = kms[2];
        stats->ms_splat = kms[3];
        stats->ms_finish = kms[4];
        stats->rays_finish = finish_rays;
        stats->nee_inline = S.nee_inline ? 1u : 0u;
        stats->ext_inline = S.ext_inline ? 1u : 0u;
    }
    if (cancelled) return fail(NORI_ERR_CANCELLED, "rendering was cancelled");
    return NORI_OK;
}

}  // namespace nori

extern "C" {

int nori_gpu_render(nori_gpu_ctx *c, const nori_gpu_render_desc *rd, float *rgbw_out, nori_gpu_stats *stats) {
    return guarded([&] {
        if (!c || !rd || !rgbw_out) return fail(NORI_ERR_INVALID, "null argument");
        if (rd->num_blocks && !rd->block_ids) return fail(NORI_ERR_INVALID, "block_ids is null");
        return render(*c, *rd, rgbw_out, stats);
    });
}

}  // extern "C"
