// li.hip -- nori_gpu_li: Integrator::Li of the context's integrator along the
// caller's rays (stated in nori_gpu.h), one k_li launch (kernels_li.hip) per at
// most 16M rays.  The checks that need no device, the two environment knobs and
// the launch split are li_prep.cpp's; staging, events, cancel and progress
// follow query() and the shading queries (queries.hip).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "li_prep.h"

namespace nori {
namespace {

int li(nori_gpu_ctx &c, const nori_gpu_li_desc &ld, const float *rays, const uint64_t *ids, float *out,
       nori_gpu_stats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(c.device));
    const uint32_t n = ld.n;
    if (ld.on_device) {
        require_device_ptr(rays, "nori_gpu_li: on_device with rays that are not device memory");
        if (ids) require_device_ptr(ids, "nori_gpu_li: on_device with stream_ids that are not device memory");
        require_device_ptr(out, "nori_gpu_li: on_device with an out that is not device memory");
    }
    c.clock.reset(true);
    // closest-hit rays, shadow rays, invalid rows: summed on the device over the call's launches
    c.li_count.ensure(3 * sizeof(unsigned long long));
    HIP_TRY(hipMemsetAsync(c.li_count.p, 0, 3 * sizeof(unsigned long long), c.stream));
    LiArgs a{};
    a.range = li_range(std::getenv("NORI_LI_RANGE"));
    a.refill = li_refill(std::getenv("NORI_LI_REFILL"));
    a.first_draw = ld.first_draw;
    a.seed = ld.seed;
    a.counters = c.li_count.as<unsigned long long>();
    c.cancel = 0;
    c.report(0.0);
    bool cancelled = false;
    // rows [i0, i0 + m) of the call from the device arrays r, s (or null) into o
    auto run = [&](uint64_t i0, uint32_t m, const float4 *r, const uint64_t *s, float *o) {
        a.rays = r;
        a.ids = s;
        a.out = o;
        a.n = m;
        a.stream_base = ld.stream_base + i0;
        c.clock.span(c.stream, kKindShade, [&] { return launch_li(c.S, a, c.stack, c.stream); });
    };
    auto finish = [&](uint64_t done) {  // (the stream's work up to here)
        HIP_TRY(hipStreamSynchronize(c.stream));
        c.clock.collect();
        c.report((double)done / n);
    };
    if (ld.on_device) {
        for (uint64_t j = 0;; ++j) {
            const LiSpan sp = li_span(n, kLiLaunchRows, j);
            if (!sp.count) break;
            if (c.cancel.load()) {
                cancelled = true;
                break;
            }
            run(sp.first, sp.count, reinterpret_cast<const float4 *>(rays) + 2 * sp.first, ids ? ids + sp.first : nullptr,
                out + 3 * sp.first);
            finish(sp.first + sp.count);
        }
    } else {
        // a host `out` is left unchanged by a cancelled call: the chunks are
        // collected here and copied out at the end
        const uint32_t chunk = std::min(std::min(n, query_chunk(std::getenv("NORI_QUERY_CHUNK"))), kLiLaunchRows);
        c.q_rays.ensure(32 * (size_t)chunk);
        if (ids) c.sh_in[0].ensure(8 * (size_t)chunk);
        c.sh_out.ensure(12 * (size_t)chunk);
        std::vector<float> res(3 * (size_t)n);
        for (uint64_t j = 0;; ++j) {
            const LiSpan sp = li_span(n, chunk, j);
            if (!sp.count) break;
            if (c.cancel.load()) {
                cancelled = true;
                break;
            }
            HIP_TRY(hipMemcpyAsync(c.q_rays.p, rays + 8 * sp.first, 32 * (size_t)sp.count, hipMemcpyHostToDevice, c.stream));
            if (ids)
                HIP_TRY(hipMemcpyAsync(c.sh_in[0].p, ids + sp.first, 8 * (size_t)sp.count, hipMemcpyHostToDevice, c.stream));
            run(sp.first, sp.count, c.q_rays.as<float4>(), ids ? c.sh_in[0].as<uint64_t>() : nullptr, c.sh_out.as<float>());
            HIP_TRY(hipMemcpyAsync(res.data() + 3 * sp.first, c.sh_out.p, 12 * (size_t)sp.count, hipMemcpyDeviceToHost,
                                   c.stream));
            finish(sp.first + sp.count);
        }
        if (!cancelled) std::memcpy(out, res.data(), res.size() * sizeof(float));
    }
    unsigned long long cnt[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(cnt, c.li_count.p, sizeof(cnt), hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    c.report(1.0);
    if (begin_stats(c, t0, stats)) {
        stats->samples = n;
        stats->rays_closest = cnt[0];
        stats->rays_shadow = cnt[1];
        stats->invalid_samples = cnt[2];
        stats->ms_shade = c.clock.ms[kKindShade];  // k_li: the whole integrator
    }
    if (cancelled) return fail(NORI_ERR_CANCELLED, "nori_gpu_li was cancelled");
    return NORI_OK;
}

}  // namespace
}  // namespace nori

extern "C" {

int nori_gpu_li(nori_gpu_ctx *c, const nori_gpu_li_desc *ld, const float *rays, const uint64_t *stream_ids, float *out,
                nori_gpu_stats *stats) {
    return guarded([&] {
        if (const char *why = li_check(c, ld, rays, stream_ids, out)) return fail(NORI_ERR_INVALID, why);
        if (ld->n == 0) return NORI_OK;
        return li(*c, *ld, rays, stream_ids, out, stats);
    });
}

}  // extern "C"
