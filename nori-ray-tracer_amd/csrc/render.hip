// render.hip -- nori_gpu_render: the wavefront loop and the one-bounce integrators.
//
// nori_gpu_render replaces RenderThread::renderScene's pass loop
// (render.cpp:173-250): instead of spp sequential passes of a
// tbb::parallel_for over 32x32 blocks, every (pass, pixel) sample of the
// requested blocks becomes a work id; a pool of paths stays resident in HBM
// and the shade kernel refills finished slots from a device work counter, so
// the GPU stays full until the last sample.  Radiance accumulates per sample
// record; after the pool drains, k_splat applies ImageBlock::put.
//
// render() reads top to bottom as its steps: Wavefront's constructor plans the
// call (render_plan.h) and takes its views of the context's buffers; per chunk
// of passes, pool_part_views, then enqueue_iteration and wait_iteration until
// every work id is handed out, run_tail, read_back and debug_report.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"

namespace nori {
namespace {

static_assert(kPlanSeg == kSeg, "render_plan.h and seg_index.h disagree on the segment size");
static_assert(kPlanChanShift == kChanShift, "render_plan.h and dev_scene.h disagree on the work id's bits");

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

constexpr int kRing = 16;         // readback ring entries
constexpr int kLookaheadEnd = 2;  // iterations queued ahead of the termination check once work streams run dry

// normals / av / direct*: no path pool -- per chunk of passes, k_direct runs
// every sample start to end and writes its record, then k_splat filters them.
int render_one_bounce(nori_gpu_ctx &c, const nori_gpu_render_desc &rd, float *rgbw_out, nori_gpu_stats *stats,
                      std::chrono::steady_clock::time_point t0) {
    const DevScene &S = c.S;
    const uint32_t M = (uint32_t)c.hpixels.size(), nblocks = (uint32_t)c.hblocks.size(), passes = rd.pass_count;
    const uint32_t chunk = record_chunk(passes, M, (size_t)4 << 30);
    c.rec.ensure(16 * (size_t)chunk * M);
    c.counters.ensure(sizeof(Counters));
    FilmOut out(c, rd.output_on_device != 0, rgbw_out, rd.variance_out);
    out.begin();
    Counters *C = c.counters.as<Counters>();
    HIP_TRY(hipMemsetAsync(C, 0, sizeof(Counters), c.stream));
    if (!c.in_rounds) c.cancel = 0;
    c.report(0.0);
    KernelClock clk(rd.timing != 0);
    uint64_t done = 0;
    bool cancelled = false;
    for (uint32_t p0 = 0; p0 < passes; p0 += chunk) {
        if (c.cancel.load()) {
            cancelled = true;
            break;
        }
        const uint32_t np = std::min(chunk, passes - p0);
        WorkDesc wd{(uint64_t)np * M, M, rd.pass_begin + p0, c.pixels.as<uint32_t>(), rd.seed, 0, nullptr, 1, 0, out.var};
        SplatDesc sd{M, np, rd.pass_begin + p0, splat_passes(np, nblocks, 4096, std::getenv("NORI_SPLAT_PASSES")),
                     c.blocks.as<int4>(), rd.seed, out.var};
        clk.span(c.stream, kKindShade, [&] { return launch_direct(S, wd, c.rec.as<float4>(), C, c.stack, c.stream); });
        clk.span(c.stream, kKindSplat,
                 [&] { return launch_splat(S, c.rec.as<float4>(), sd, nblocks, out.film, C, c.stream); }, true);
        HIP_TRY(hipStreamSynchronize(c.stream));
        done += wd.total;
        c.report((double)(p0 + np) / passes);
    }
    Counters hc;
    HIP_TRY(hipMemcpyAsync(&hc, C, sizeof(Counters), hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    clk.collect();
    out.finish(cancelled);
    c.report(1.0);
    if (begin_stats(c, t0, stats)) {
        stats->samples = done;
        stats->invalid_samples = hc.invalid;
        stats->rays_closest = hc.direct_rays[0];
        stats->rays_shadow = hc.direct_rays[1];
        stats->ms_shade = clk.ms[kKindShade];  // k_direct: the whole integrator
        stats->ms_splat = clk.ms[kKindSplat];
    }
    if (cancelled) return fail(NORI_ERR_CANCELLED, "rendering was cancelled");
    return NORI_OK;
}

// A pool part's views of the queues and its stream.  The pool is split into
// independent parts (segments never interact), each driven on its own stream:
// the memory-bound shade launch of one part overlaps the VALU-bound traversal
// of another.
struct PoolPart {
    hipStream_t st;
    uint32_t G;  // its segments
    PathQueue Q[2];
    ShadowQueue sq;
    SegState seg;
    WorkDesc wd;
};

// One wavefront render: the plan, the views of the context's buffers, the
// sums over its chunks of passes, and the chunk in flight.
struct Wavefront {
    nori_gpu_ctx &c;
    const nori_gpu_render_desc &rd;
    const DevScene &S;
    DevScene Sk;  // ... as k_shade sees it: ext_inline only where the loop relies on it
    const uint32_t M, nblocks, passes;
    const bool timing, ext_loop;
    uint32_t pool, chunk, parts, G;
    PartSplit split;
    Counters *C;
    PathQueue Q[2];
    ShadowQueue sq;
    SegState seg;
    FilmOut out;
    KernelClock clk;
    uint64_t done_before = 0, rays_c = 0, rays_s = 0, invalid = 0, iters = 0, finish_rays = 0, samples_started = 0;
    bool cancelled = false;
    // the chunk in flight
    uint32_t p0 = 0, np = 0;
    WorkDesc wd{};
    PoolPart part[kMaxParts];
    int last_out = 0;
    uint64_t lag = 0;
    // NORI_DEBUG: host time spent enqueuing vs waiting on the ring events
    // (a wait that returns at once means the device ran dry of work)
    const bool dbg = debug_log();
    double t_enq = 0.0, t_wait = 0.0, t_mark = 0.0;
    uint32_t idle_waits = 0;

    Wavefront(nori_gpu_ctx &ctx, const nori_gpu_render_desc &desc, float *rgbw_out);
    hipStream_t stream_of(uint32_t h) const { return h ? c.parts[h] : c.stream; }
};

double now_us() {
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// The plan (pool, record chunk, parts: render_plan.h), the buffers it needs and the film target.
Wavefront::Wavefront(nori_gpu_ctx &ctx, const nori_gpu_render_desc &desc, float *rgbw_out)
    : c(ctx), rd(desc), S(ctx.S), Sk(ctx.S), M((uint32_t)ctx.hpixels.size()), nblocks((uint32_t)ctx.hblocks.size()),
      passes(desc.pass_count), timing(desc.timing != 0),
      // S.ext_inline: an iteration is the shade launch alone.  A timing render
      // keeps the two launches (one event span per kernel), so its shade kernel
      // reads the hits as without the flag, and it keeps the pool and the parts
      // of the two-launch loop.
      ext_loop(ctx.S.ext_inline != 0 && !timing), out(ctx, desc.output_on_device != 0, rgbw_out, desc.variance_out),
      clk(timing) {
    pool = rd.path_pool ? round_pool(rd.path_pool)
                        : default_pool(passes, M, c.stack != 0, ext_loop, std::getenv("NORI_PATH_POOL"));
    ensure_pool(c, pool);
    // sample-record budget: chunks of passes, each < 2^31 records
    chunk = record_chunk(passes, M, (size_t)6 << 30);
    c.rec.ensure(16 * (size_t)chunk * M);
    c.counters.ensure(sizeof(Counters));
    out.begin();
    if (!c.pinned) {
        // host-mapped, coherent: the shade kernel stores the completion flag here
        HIP_TRY(hipHostMalloc((void **)&c.pinned, 256, hipHostMallocMapped | hipHostMallocCoherent));
        HIP_TRY(hipHostGetDevicePointer((void **)&c.pinned_dev, c.pinned, 0));
        for (auto &r : c.ring) {
            r.resize(kRing);
            for (auto &e : r) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
    }
    C = c.counters.as<Counters>();
    sq = ShadowQueue{c.sq[0].as<float4>(), c.sq[1].as<float4>(), c.sq[2].as<float4>()};
    Q[0] = queue_of(c, 0);
    Q[1] = queue_of(c, 1);
    if (!ext_loop) Sk.ext_inline = 0;
    G = pool / kSeg;
    parts = std::max<uint32_t>(1, std::min<uint32_t>(pool_parts(std::getenv("NORI_POOL_PARTS"), ext_loop), G));
    split = part_split(G, parts);
    seg = SegState{{c.seg[0].as<uint32_t>(), c.seg[1].as<uint32_t>()}, c.seg[2].as<uint32_t>(), c.seg[3].as<uint32_t>(),
                   c.segstats.as<uint4>()};
}

// The chunk's work and each part's views of the queues, segment state and work.
void pool_part_views(Wavefront &w) {
    w.wd = WorkDesc{(uint64_t)w.np * w.M, w.M, w.rd.pass_begin + w.p0, w.c.pixels.as<uint32_t>(), w.rd.seed, w.G,
                    w.c.pinned_dev, 1, 0, w.out.var};
    w.wd.rot = stream_rotation(w.wd.total, w.M, w.G);
    auto q_view = [](const PathQueue &q, size_t e) {
        return PathQueue{q.ray_o + e, q.ray_d + e, q.hit + e, q.thr + e, q.rng + e};
    };
    for (uint32_t h = 0; h < w.parts; ++h) {
        PoolPart &p = w.part[h];
        const uint32_t b0 = w.split.base[h];
        const size_t e = (size_t)b0 * kSeg;
        p.st = w.stream_of(h);
        p.G = w.split.count[h];
        p.Q[0] = q_view(w.Q[0], e);
        p.Q[1] = q_view(w.Q[1], e);
        p.sq = ShadowQueue{w.sq.ray_o + e, w.sq.ray_d + e, w.sq.payload + e};
        p.seg = SegState{{w.seg.cnt[0] + b0, w.seg.cnt[1] + b0}, w.seg.shcnt + b0, w.seg.cursor + b0, w.seg.stats + b0};
        p.wd = w.wd;
        p.wd.b0 = b0;
    }
}

// Iteration `it` on every part: k_shade from queue in = it & 1 into out, then
// the traces its survivors and shadow rays still need; an event per part.
void enqueue_iteration(Wavefront &w, uint64_t it) {
    nori_gpu_ctx &c = w.c;
    const DevScene &S = w.S;
    const double te0 = w.dbg ? now_us() : 0.0;
    const int in = (int)(it & 1), out = in ^ 1;
    w.last_out = out;
    float4 *rec = c.rec.as<float4>();
    for (uint32_t h = 0; h < w.parts; ++h) {
        PoolPart &p = w.part[h];
        const SegState &sg = p.seg;
        w.clk.span(p.st, kKindShade, [&] {
            return launch_shade(w.Sk, p.Q[in], p.Q[out], p.sq, sg, in, p.wd, rec, w.C, p.G, p.st, &c.shade_rtc);
        });
        auto extend = [&] {
            w.clk.span(p.st, kKindExtend, [&] { return launch_extend(S, p.Q[out], sg.cnt[out], p.G, c.stack, p.st, &c.rtc); });
        };
        hipError_t both_err = hipSuccess;
        if (S.nee_inline) {  // the shadow rays were traced by k_shade itself
            if (w.ext_loop) continue;  // ... and so will the next vertex's extension ray be
            extend();
            continue;
        }
        if (!w.timing && c.fuse_trace &&
            launch_trace_both(S, p.Q[out], sg.cnt[out], p.sq, sg.shcnt, rec, p.G, c.stack, &c.rtc, p.st, both_err)) {
            HIP_TRY(both_err);  // (the timed renders keep two launches: one event span per kernel)
            continue;
        }
        extend();
        w.clk.span(p.st, kKindShadow, [&] { return launch_shadow(S, p.sq, sg.shcnt, rec, p.G, c.stack, p.st, &c.rtc); });
    }
    ++w.iters;
    for (uint32_t h = 0; h < w.parts; ++h) HIP_TRY(hipEventRecord(c.ring[h][it % kRing], w.part[h].st));
    w.t_mark = w.dbg ? now_us() : 0.0;
    w.t_enq += w.t_mark - te0;
}

// The host waits on the event from `lag` iterations back, then reads the flags
// the shade kernel stores as the device has set them by now.  True: the loop ends
// (every work id has been handed out, or the render was cancelled).
bool wait_iteration(Wavefront &w, uint64_t it) {
    nori_gpu_ctx &c = w.c;
    if (it < w.lag) return false;
    for (uint32_t h = 0; h < w.parts; ++h) HIP_TRY(hipEventSynchronize(c.ring[h][(it - w.lag) % kRing]));
    if (w.dbg) {
        const double t = now_us() - w.t_mark;
        w.t_wait += t;
        w.idle_waits += t < 5.0 ? 1u : 0u;
    }
    const uint32_t exhausted = __atomic_load_n(&c.pinned[1], __ATOMIC_ACQUIRE);
    // the streams are running dry: queue fewer iterations ahead,
    // so that few drain iterations (full-grid launches over a
    // thinning pool) are already queued when the last one does
    if (exhausted) w.lag = std::min<uint64_t>(w.lag, kLookaheadEnd);
    c.report(std::min(1.0, (double)w.done_before / ((double)w.passes * w.M) + (double)w.np / w.passes * exhausted / w.G));
    // every work id has been handed out: finish the remaining paths in one launch
    if (__atomic_load_n(&c.pinned[0], __ATOMIC_ACQUIRE)) return true;
    if (c.cancel.load()) w.cancelled = true;
    return w.cancelled;
}

// The samples still in flight are marked pending; the film splat of all
// the others runs on the side stream while the finisher completes the
// pending ones and splats each itself.
void run_tail(Wavefront &w) {
    nori_gpu_ctx &c = w.c;
    const DevScene &S = w.S;
    const int lo = w.last_out;
    float4 *rec = c.rec.as<float4>();
    HIP_TRY(launch_mark(w.Q[lo], w.seg, lo, rec, w.G, c.stream));
    HIP_TRY(launch_tail_prefix(w.seg, lo, w.G, c.tailpre.as<uint32_t>(), c.stream));
    HIP_TRY(hipEventRecord(c.fork, c.stream));
    HIP_TRY(hipStreamWaitEvent(c.side, c.fork, 0));
    SplatDesc sd{w.M, w.np, w.rd.pass_begin + w.p0, splat_passes(w.np, w.nblocks, 256, std::getenv("NORI_SPLAT_PASSES")),
                 c.blocks.as<int4>(), w.rd.seed, w.out.var};
    auto splat = [&] {
        w.clk.span(c.side, kKindSplat, [&] { return launch_splat(S, rec, sd, w.nblocks, w.out.film, w.C, c.side); });
    };
    auto finish = [&] {
        w.clk.span(c.stream, kKindFinish, [&] {
            return launch_finish(S, w.Q[lo], w.seg, lo, rec, w.wd, w.out.film, w.C, w.G, c.stack, c.tailpre.as<uint32_t>(),
                                 c.stream);
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
}

// The chunk's counters and per-segment statistics, through pinned staging: both
// copies queue behind the finisher without a host round trip each (pageable
// copies stage twice).  Returns when the chunk is complete on the device.
Counters read_back(Wavefront &w) {
    nori_gpu_ctx &c = w.c;
    const size_t rb = sizeof(Counters) + 16 * (size_t)w.G;
    if (c.readback_bytes < rb) {
        if (c.readback) HIP_TRY(hipHostFree(c.readback));
        c.readback = nullptr;
        c.readback_bytes = 0;
        HIP_TRY(hipHostMalloc((void **)&c.readback, rb, hipHostMallocDefault));
        c.readback_bytes = rb;
    }
    HIP_TRY(hipMemcpyAsync(c.readback, w.C, sizeof(Counters), hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipMemcpyAsync(c.readback + sizeof(Counters), w.seg.stats, 16 * (size_t)w.G, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    Counters hc;
    std::memcpy(&hc, c.readback, sizeof(Counters));
    for (uint32_t b = 0; b < w.G; ++b) {
        uint4 st;
        std::memcpy(&st, c.readback + sizeof(Counters) + 16 * (size_t)b, 16);
        w.rays_c += st.x;
        w.rays_s += st.y;
        w.samples_started += st.z;
        w.finish_rays += st.w;
    }
    w.invalid += hc.invalid;
    return hc;
}

// NORI_DEBUG: the chunk's loop, and the clocks of the profiling builds.
void debug_report(const Wavefront &w, const Counters &hc) {
    if (!w.dbg) return;
    std::fprintf(stderr, "[nori] chunk %u: %lu iterations, finisher %u paths, longest %u rays\n", w.p0,
                 (unsigned long)w.iters, hc.finish_paths, hc.finish_max_rays);
    std::fprintf(stderr, "[nori] host loop: %.0f us enqueuing, %.0f us waiting; %u of the waits returned at once\n",
                 w.t_enq, w.t_wait, w.idle_waits);
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

// Passes [p0, p0 + np) of the render: reset, the loop over the parts' streams
// until every work id is handed out, the tail on the whole pool, the read-back.
void run_chunk(Wavefront &w) {
    nori_gpu_ctx &c = w.c;
    pool_part_views(w);
    __atomic_store_n(&c.pinned[0], 0u, __ATOMIC_RELEASE);
    __atomic_store_n(&c.pinned[1], 0u, __ATOMIC_RELEASE);
    // segments whose stream is empty from the start count as exhausted
    uint32_t empty = 0;
    for (uint32_t b = 0; b < w.G; ++b) empty += stream_work(w.wd, b, 0) >= w.wd.total;
    HIP_TRY(launch_reset(w.C, empty, w.seg, w.G, c.stream));
    HIP_TRY(hipEventRecord(c.fork, c.stream));  // the part streams start after the resets above
    for (uint32_t h = 1; h < w.parts; ++h) HIP_TRY(hipStreamWaitEvent(c.parts[h], c.fork, 0));
    w.lag = (uint64_t)lookahead(std::getenv("NORI_LOOKAHEAD"));
    w.t_enq = w.t_wait = 0.0;
    w.idle_waits = 0;
    for (uint64_t it = 0;; ++it) {
        enqueue_iteration(w, it);
        if (wait_iteration(w, it)) break;
    }
    // ext_loop: the last iteration's survivors and new samples have no hits
    // yet; the finisher below reads them, so they are traced once here
    for (uint32_t h = 0; w.ext_loop && !w.cancelled && h < w.parts; ++h) {
        const PoolPart &p = w.part[h];
        HIP_TRY(launch_extend(w.S, p.Q[w.last_out], p.seg.cnt[w.last_out], p.G, c.stack, p.st, &c.rtc));
    }
    for (uint32_t h = 1; h < w.parts; ++h) {  // join: the tail below runs on the whole pool
        HIP_TRY(hipEventRecord(c.joins[h], c.parts[h]));
        HIP_TRY(hipStreamWaitEvent(c.stream, c.joins[h], 0));
    }
    if (w.cancelled) return;
    run_tail(w);
    debug_report(w, read_back(w));
    w.done_before += w.wd.total;
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
    work_lists(c, rd);
    const size_t M = c.hpixels.size();
    if (rd.pass_count == 0 || M == 0) throw NoriException(NORI_ERR_INVALID, "nothing to render (pass_count or blocks empty)");
    if (c.S.integrator >= NORI_INTEGRATOR_NORMALS) return render_one_bounce(c, rd, rgbw_out, stats, t0);
    if (M > kWorkMask) throw NoriException(NORI_ERR_INVALID, "frame too large: more than 2^29 pixels per pass");
    Wavefront w(c, rd, rgbw_out);
    if (!c.in_rounds) c.cancel = 0;
    c.report(0.0);
    for (w.p0 = 0; w.p0 < w.passes && !w.cancelled; w.p0 += w.chunk) {
        w.np = std::min(w.chunk, w.passes - w.p0);
        run_chunk(w);
    }
    if (w.samples_started != w.done_before && !w.cancelled)
        throw NoriException(NORI_ERR_INVALID, "internal: started " + std::to_string(w.samples_started) + " of " +
                                                  std::to_string(w.done_before) + " samples");
    if (w.timing) {
        HIP_TRY(hipStreamSynchronize(c.stream));
        w.clk.collect();
    }
    w.out.finish(w.cancelled);
    HIP_TRY(hipStreamSynchronize(c.stream));
    HIP_TRY(hipStreamSynchronize(c.side));
    for (int h = 1; h < kMaxParts; ++h) HIP_TRY(hipStreamSynchronize(c.parts[h]));
    c.report(1.0);
    if (begin_stats(c, t0, stats)) {
        stats->samples = w.done_before;
        stats->invalid_samples = w.invalid;
        stats->rays_closest = w.rays_c;
        stats->rays_shadow = w.rays_s;
        stats->iterations = w.iters;
        stats->stream_parts = w.parts;
        stats->path_pool = w.pool;
        stats->ms_extend = w.clk.ms[kKindExtend];
        stats->ms_shadow = w.clk.ms[kKindShadow];
        stats->ms_shade = w.clk.ms[kKindShade];
        stats->ms_splat = w.clk.ms[kKindSplat];
        stats->ms_finish = w.clk.ms[kKindFinish];
        stats->rays_finish = w.finish_rays;
        stats->nee_inline = c.S.nee_inline ? 1u : 0u;
        stats->ext_inline = c.S.ext_inline ? 1u : 0u;
    }
    if (w.cancelled) return fail(NORI_ERR_CANCELLED, "rendering was cancelled");
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
