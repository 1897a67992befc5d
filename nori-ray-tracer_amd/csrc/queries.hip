// queries.hip -- the calls that run one kernel over the caller's arrays:
// feature buffers, ray and hit-record queries, camera rays, the shading
// queries and the samplers' uniforms; and the hit record's host statement.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "surface_grad.h"

namespace nori {
namespace {

// The selected blocks' pixels M (work_lists), the pass count (0: the scene's
// sampleCount) and the passes per launch: about 16M elements.
struct PassChunks {
    uint32_t M, passes, chunk;
};
PassChunks pass_chunks(nori_gpu_ctx &c, const nori_gpu_render_desc &rd, const char *nothing) {
    work_lists(c, rd);
    const uint32_t M = (uint32_t)c.hpixels.size(), passes = rd.pass_count ? rd.pass_count : c.spp;
    if (passes == 0 || M == 0) throw NoriException(NORI_ERR_INVALID, nothing);
    return {M, passes, pass_chunk(passes, M)};
}

// nori_gpu_render_features: k_features over the selected blocks' pixels, in
// chunks of passes (about 16M samples per launch) between which a cancel
// request is honoured.  The kernel continues each pixel's sums from the values
// in the buffer, so a host buffer is uploaded first and copied back after the
// last chunk: host and device buffers receive the same bits.
int render_features(nori_gpu_ctx &c, const nori_gpu_render_desc &rd, float *features, nori_gpu_stats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(c.device));
    if (rd.variance_out) throw NoriException(NORI_ERR_INVALID, "nori_gpu_render_features: variance_out must be NULL");
    const auto [M, passes, chunk] = pass_chunks(c, rd, "nothing to render (pass_count or blocks empty)");
    const size_t n = 8 * (size_t)c.S.W * (size_t)c.S.H;
    float *dev = features;
    if (rd.output_on_device) {
        if ((uintptr_t)features % 16) throw NoriException(NORI_ERR_INVALID, "device features must be 16-byte aligned");
    } else {
        c.varbuf.ensure(n * sizeof(float));
        dev = c.varbuf.as<float>();
        HIP_TRY(hipMemcpyAsync(dev, features, n * sizeof(float), hipMemcpyHostToDevice, c.stream));
    }
    c.cancel = 0;
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
        clk.span(c.stream, kKindShade, [&, M = M] {
            return launch_features(c.S, c.pixels.as<uint32_t>(), M, rd.pass_begin + p0, np, rd.seed, dev, c.stack, c.stream);
        });
        HIP_TRY(hipStreamSynchronize(c.stream));
        done += (uint64_t)np * M;
        c.report((double)(p0 + np) / passes);
    }
    clk.collect();
    if (!rd.output_on_device && !cancelled)
        HIP_TRY(hipMemcpy(features, dev, n * sizeof(float), hipMemcpyDeviceToHost));
    c.report(1.0);
    if (begin_stats(c, t0, stats)) {
        stats->samples = done;
        stats->rays_closest = done;  // one primary ray per sample
        stats->ms_shade = clk.ms[kKindShade];  // k_features
    }
    if (cancelled) return fail(NORI_ERR_CANCELLED, "rendering was cancelled");
    return NORI_OK;
}

// nori_gpu_query: launch_trace (the kernels of nori_gpu_trace), then k_surface
// on its hits.  Device buffers are used in place; host arrays pass through the
// context's staging buffers in chunks of at most NORI_QUERY_CHUNK rays.
int query(nori_gpu_ctx &c, const nori_gpu_query_desc &qd, const float *rays, nori_gpu_hit *hits,
          nori_gpu_surface *surf, nori_gpu_stats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(c.device));
    const uint32_t n = qd.n;
    c.clock.reset(stats != nullptr);
    // one chunk on the device: rays r -> hits h (-> records s)
    auto run = [&](const float4 *r, uint32_t m, float4 *h, float4 *s) {
        c.clock.span(c.stream, kKindExtend, [&] { return launch_trace(c.S, r, m, qd.any_hit, h, c.stack, c.stream, &c.rtc); });
        if (s) c.clock.span(c.stream, kKindShade, [&] { return launch_surface(c.S, r, h, m, s, c.stream); }, true);
    };
    if (qd.on_device) {
        float4 *h = reinterpret_cast<float4 *>(hits);
        if (!h) {
            c.q_hits.ensure(16 * (size_t)n);
            h = c.q_hits.as<float4>();
        }
        run(reinterpret_cast<const float4 *>(rays), n, h, reinterpret_cast<float4 *>(surf));
        HIP_TRY(hipStreamSynchronize(c.stream));
        c.clock.collect();
    } else {
        const uint32_t chunk = std::min(n, query_chunk(std::getenv("NORI_QUERY_CHUNK")));
        c.q_rays.ensure(32 * (size_t)chunk);
        c.q_hits.ensure(16 * (size_t)chunk);
        if (surf) c.q_surf.ensure(64 * (size_t)chunk);
        for (uint64_t i0 = 0; i0 < n; i0 += chunk) {
            const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, n - i0);
            HIP_TRY(hipMemcpyAsync(c.q_rays.p, rays + 8 * i0, 32 * (size_t)m, hipMemcpyHostToDevice, c.stream));
            run(c.q_rays.as<float4>(), m, c.q_hits.as<float4>(), surf ? c.q_surf.as<float4>() : nullptr);
            if (hits) HIP_TRY(hipMemcpyAsync(hits + i0, c.q_hits.p, 16 * (size_t)m, hipMemcpyDeviceToHost, c.stream));
            if (surf) HIP_TRY(hipMemcpyAsync(surf + i0, c.q_surf.p, 64 * (size_t)m, hipMemcpyDeviceToHost, c.stream));
            HIP_TRY(hipStreamSynchronize(c.stream));
            c.clock.collect();
        }
    }
    if (begin_stats(c, t0, stats)) {
        (qd.any_hit ? stats->rays_shadow : stats->rays_closest) = n;
        stats->ms_extend = c.clock.ms[kKindExtend];
        stats->ms_shade = c.clock.ms[kKindShade];  // k_surface
    }
    return NORI_OK;
}

// nori_gpu_camera_rays: k_camera_rays over the selected blocks' pixels, in
// chunks of passes (about 16M rays per launch).  Only the selected pixels are
// written, so a host buffer is uploaded first and copied back afterwards: the
// other entries keep the caller's values, as in a device buffer.
int camera_rays(nori_gpu_ctx &c, const nori_gpu_render_desc &rd, float *rays) {
    HIP_TRY(hipSetDevice(c.device));
    if (rd.variance_out) throw NoriException(NORI_ERR_INVALID, "nori_gpu_camera_rays: variance_out must be NULL");
    const auto [M, passes, chunk] = pass_chunks(c, rd, "nothing to do (pass_count or blocks empty)");
    const size_t bytes = 32 * (size_t)passes * (size_t)c.S.W * (size_t)c.S.H;
    float *dev = rays;
    if (rd.output_on_device) {
        if ((uintptr_t)rays % 16) throw NoriException(NORI_ERR_INVALID, "device rays must be 16-byte aligned");
    } else {
        c.q_rays.ensure(bytes);
        dev = c.q_rays.as<float>();
        HIP_TRY(hipMemcpyAsync(dev, rays, bytes, hipMemcpyHostToDevice, c.stream));
    }
    for (uint32_t k0 = 0; k0 < passes; k0 += chunk)
        HIP_TRY(launch_camera_rays(c.S, c.pixels.as<uint32_t>(), M, rd.pass_begin, k0, std::min(chunk, passes - k0),
                                   rd.seed, dev, c.stream));
    if (!rd.output_on_device) HIP_TRY(hipMemcpyAsync(rays, dev, bytes, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    return NORI_OK;
}

// The shading queries (nori_gpu_bsdf_eval .. nori_gpu_emitter_eval, stated in
// nori_gpu.h): one element-wise kernel over up to three input arrays and one
// output array.  Device arrays are checked (alignment, and that the runtime
// knows them as device memory: update_vertices' check) and used in place;
// host arrays pass through the context's sh_in / sh_out buffers in chunks of
// at most NORI_QUERY_CHUNK elements.
struct ShadeArr {
    const void *p;   // may be null only where the call allows it (ids)
    size_t stride;   // bytes per element
    size_t align;    // of a device pointer
};
template <class Launch>
int shading_call(nori_gpu_ctx &c, const char *name, const nori_gpu_shading_desc &sd, const ShadeArr (&in)[3], void *out,
                 size_t out_stride, Launch &&launch) {
    HIP_TRY(hipSetDevice(c.device));
    const uint32_t n = sd.n;
    if (sd.on_device) {
        const ShadeArr all[4] = {in[0], in[1], in[2], ShadeArr{out, out_stride, 16}};
        for (const ShadeArr &a : all) {
            if (!a.p) continue;
            if ((uintptr_t)a.p % a.align)
                throw NoriException(NORI_ERR_INVALID, std::string(name) + ": a device pointer is not " +
                                                          std::to_string(a.align) + "-byte aligned");
            require_device_ptr(a.p, std::string(name) + ": on_device with a pointer that is not device memory");
        }
        const void *d[3] = {in[0].p, in[1].p, in[2].p};
        HIP_TRY(launch(d, out, n));
        HIP_TRY(hipStreamSynchronize(c.stream));
        return NORI_OK;
    }
    const uint32_t chunk = std::min(n, query_chunk(std::getenv("NORI_QUERY_CHUNK")));
    for (int k = 0; k < 3; ++k)
        if (in[k].p) c.sh_in[k].ensure(in[k].stride * (size_t)chunk);
    c.sh_out.ensure(out_stride * (size_t)chunk);
    for (uint64_t i0 = 0; i0 < n; i0 += chunk) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, n - i0);
        const void *d[3] = {nullptr, nullptr, nullptr};
        for (int k = 0; k < 3; ++k) {
            if (!in[k].p) continue;
            HIP_TRY(hipMemcpyAsync(c.sh_in[k].p, (const char *)in[k].p + in[k].stride * i0, in[k].stride * (size_t)m,
                                   hipMemcpyHostToDevice, c.stream));
            d[k] = c.sh_in[k].p;
        }
        HIP_TRY(launch(d, c.sh_out.p, m));
        HIP_TRY(hipMemcpyAsync((char *)out + out_stride * i0, c.sh_out.p, out_stride * (size_t)m, hipMemcpyDeviceToHost,
                               c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
    }
    return NORI_OK;
}
// Host records: the shape index must be the miss's -1 or a shape of the scene.
void check_host_records(const nori_gpu_ctx &c, const char *name, const nori_gpu_surface *surf, uint32_t n) {
    const int32_t ns = (int32_t)c.hshapes.size();
    for (uint32_t i = 0; i < n; ++i)
        if (surf[i].shape < -1 || surf[i].shape >= ns)
            throw NoriException(NORI_ERR_INVALID, std::string(name) + ": record " + std::to_string(i) + " names shape " +
                                                      std::to_string(surf[i].shape) + " of " + std::to_string(ns));
}

// nori_gpu_sample_uniforms: k_sample_uniforms over the selected blocks'
// pixels, in chunks of passes like camera_rays (and with its handling of a
// host buffer: uploaded first, so that unselected entries keep their values).
int sample_uniforms(nori_gpu_ctx &c, const nori_gpu_render_desc &rd, uint32_t first, uint32_t count, float *out) {
    HIP_TRY(hipSetDevice(c.device));
    if (rd.variance_out) throw NoriException(NORI_ERR_INVALID, "nori_gpu_sample_uniforms: variance_out must be NULL");
    if (count == 0 || first + count < first)
        throw NoriException(NORI_ERR_INVALID, "nori_gpu_sample_uniforms: count is 0 or first + count overflows");
    const auto [M, passes, chunk] = pass_chunks(c, rd, "nothing to do (pass_count or blocks empty)");
    const size_t bytes = 4 * (size_t)count * (size_t)passes * (size_t)c.S.W * (size_t)c.S.H;
    float *dev = out;
    if (rd.output_on_device) {
        if ((uintptr_t)out % 4) throw NoriException(NORI_ERR_INVALID, "nori_gpu_sample_uniforms: the device buffer must be 4-byte aligned");
        require_device_ptr(out, "nori_gpu_sample_uniforms: output_on_device with a pointer that is not device memory");
    } else {
        c.sh_out.ensure(bytes);
        dev = c.sh_out.as<float>();
        HIP_TRY(hipMemcpyAsync(dev, out, bytes, hipMemcpyHostToDevice, c.stream));
    }
    for (uint32_t k0 = 0; k0 < passes; k0 += chunk)
        HIP_TRY(launch_sample_uniforms(c.S, c.pixels.as<uint32_t>(), M, rd.pass_begin, k0, std::min(chunk, passes - k0),
                                       rd.seed, first, count, dev, c.stream));
    if (!rd.output_on_device) HIP_TRY(hipMemcpyAsync(out, dev, bytes, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    return NORI_OK;
}

// nori_gpu_surface_grad: k_surface_grad over the caller's hits, for the
// vertices in c.pos / c.nrm as they are now.  Device arrays are checked and
// used in place; host inputs pass through q_rays / q_hits / q_surf in chunks
// of at most NORI_QUERY_CHUNK hits, and the sums are formed in sh_out / sh_in[0],
// zeroed first, and added to the caller's arrays at the end.
int surface_grad(nori_gpu_ctx &c, const nori_gpu_surface_grad_desc &gd, const float *rays, const nori_gpu_hit *hits,
                 const nori_gpu_surface *grad_surf, float *grad_positions, float *grad_normals, nori_gpu_stats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    const char *name = "nori_gpu_surface_grad";
    HIP_TRY(hipSetDevice(c.device));
    const uint32_t n = gd.n, V = c.num_vertices;
    if (gd.on_device) {
        const void *all[5] = {rays, hits, grad_surf, grad_positions, grad_normals};
        for (const void *p : all)
            if (p) require_device_ptr(p, std::string(name) + ": on_device with a pointer that is not device memory");
    }
    // a scene without vertex normals has no normal terms: the instantiation without them runs
    bool any_normals = false;
    for (const DevShape &sh : c.hshapes) any_normals |= sh.type != NORI_SHAPE_SPHERE && sh.has_normals;
    c.clock.reset(stats != nullptr);
    auto run = [&](const void *r, const void *h, const void *g, uint32_t m, float *gp, float *gn) {
        c.clock.span(c.stream, kKindShade, [&] {
            return launch_surface_grad(c.S, V, (const float4 *)r, (const float4 *)h, (const float4 *)g, m, gp,
                                       any_normals ? gn : nullptr, c.stream);
        });
    };
    if (gd.on_device) {
        run(rays, hits, grad_surf, n, grad_positions, grad_normals);
        HIP_TRY(hipStreamSynchronize(c.stream));
        c.clock.collect();
    } else {
        const size_t nfl = 3 * (size_t)V;
        const bool gn = grad_normals && any_normals;
        c.sh_out.ensure(4 * nfl);
        HIP_TRY(hipMemsetAsync(c.sh_out.p, 0, 4 * nfl, c.stream));
        if (gn) {
            c.sh_in[0].ensure(4 * nfl);
            HIP_TRY(hipMemsetAsync(c.sh_in[0].p, 0, 4 * nfl, c.stream));
        }
        const uint32_t chunk = std::min(n, query_chunk(std::getenv("NORI_QUERY_CHUNK")));
        c.q_rays.ensure(32 * (size_t)chunk);
        c.q_hits.ensure(16 * (size_t)chunk);
        c.q_surf.ensure(64 * (size_t)chunk);
        for (uint64_t i0 = 0; i0 < n; i0 += chunk) {
            const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, n - i0);
            HIP_TRY(hipMemcpyAsync(c.q_rays.p, rays + 8 * i0, 32 * (size_t)m, hipMemcpyHostToDevice, c.stream));
            HIP_TRY(hipMemcpyAsync(c.q_hits.p, hits + i0, 16 * (size_t)m, hipMemcpyHostToDevice, c.stream));
            HIP_TRY(hipMemcpyAsync(c.q_surf.p, grad_surf + i0, 64 * (size_t)m, hipMemcpyHostToDevice, c.stream));
            run(c.q_rays.p, c.q_hits.p, c.q_surf.p, m, c.sh_out.as<float>(), gn ? c.sh_in[0].as<float>() : nullptr);
            HIP_TRY(hipStreamSynchronize(c.stream));
            c.clock.collect();
        }
        std::vector<float> h(nfl);
        HIP_TRY(hipMemcpy(h.data(), c.sh_out.p, 4 * nfl, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < nfl; ++k) grad_positions[k] += h[k];
        if (gn) {
            HIP_TRY(hipMemcpy(h.data(), c.sh_in[0].p, 4 * nfl, hipMemcpyDeviceToHost));
            for (size_t k = 0; k < nfl; ++k) grad_normals[k] += h[k];
        }
    }
    if (begin_stats(c, t0, stats)) stats->ms_shade = c.clock.ms[kKindShade];  // k_surface_grad
    return NORI_OK;
}

}  // namespace
}  // namespace nori

extern "C" {

int nori_gpu_render_features(nori_gpu_ctx *c, const nori_gpu_render_desc *rd, float *features, nori_gpu_stats *stats) {
    return guarded([&] {
        if (!c || !rd || !features) return fail(NORI_ERR_INVALID, "null argument");
        if (rd->num_blocks && !rd->block_ids) return fail(NORI_ERR_INVALID, "block_ids is null");
        return render_features(*c, *rd, features, stats);
    });
}

int nori_gpu_trace(nori_gpu_ctx *c, const float *rays, uint32_t n, int any_hit, nori_gpu_hit *hits) {
    return guarded([&] {
        if (!c || !rays || !hits) return fail(NORI_ERR_INVALID, "null argument");
        if (n == 0) return NORI_OK;
        HIP_TRY(hipSetDevice(c->device));
        DevBuf r, h;
        r.ensure(32 * (size_t)n);
        h.ensure(16 * (size_t)n);
        HIP_TRY(hipMemcpy(r.p, rays, 32 * (size_t)n, hipMemcpyHostToDevice));
        HIP_TRY(launch_trace(c->S, r.as<float4>(), n, any_hit, h.as<float4>(), c->stack, c->stream, &c->rtc));
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(hits, h.p, 16 * (size_t)n, hipMemcpyDeviceToHost));
        return NORI_OK;
    });
}

int nori_gpu_query(nori_gpu_ctx *c, const nori_gpu_query_desc *qd, const float *rays, nori_gpu_hit *hits,
                   nori_gpu_surface *surf, nori_gpu_stats *stats) {
    return guarded([&] {
        if (!c || !qd || !rays) return fail(NORI_ERR_INVALID, "null argument");
        if (!hits && !surf) return fail(NORI_ERR_INVALID, "nori_gpu_query: hits and surf are both null");
        if (qd->any_hit && surf) return fail(NORI_ERR_INVALID, "nori_gpu_query: an any-hit query has no hit record (surf must be NULL)");
        if (qd->reserved != 0) return fail(NORI_ERR_INVALID, "nori_gpu_query: reserved must be 0");
        if (qd->on_device && ((uintptr_t)rays % 16 || (uintptr_t)hits % 16 || (uintptr_t)surf % 16))
            return fail(NORI_ERR_INVALID, "nori_gpu_query: device pointers must be 16-byte aligned");
        if (qd->n == 0) return NORI_OK;
        return query(*c, *qd, rays, hits, surf, stats);
    });
}

int nori_gpu_camera_rays(nori_gpu_ctx *c, const nori_gpu_render_desc *rd, float *rays) {
    return guarded([&] {
        if (!c || !rd || !rays) return fail(NORI_ERR_INVALID, "null argument");
        if (rd->num_blocks && !rd->block_ids) return fail(NORI_ERR_INVALID, "block_ids is null");
        return camera_rays(*c, *rd, rays);
    });
}

int nori_gpu_bsdf_eval(nori_gpu_ctx *c, const nori_gpu_shading_desc *sd, const nori_gpu_surface *surf, const float *wi,
                       const float *wo, float *out) {
    return guarded([&] {
        if (!c || !sd || !surf || !wi || !wo || !out) return fail(NORI_ERR_INVALID, "null argument");
        if (sd->reserved != 0) return fail(NORI_ERR_INVALID, "nori_gpu_bsdf_eval: reserved must be 0");
        if (sd->n == 0) return NORI_OK;
        if (!sd->on_device) check_host_records(*c, "nori_gpu_bsdf_eval", surf, sd->n);
        const uint32_t shapes = (uint32_t)c->hshapes.size();
        return shading_call(*c, "nori_gpu_bsdf_eval", *sd, {{surf, 64, 16}, {wi, 12, 4}, {wo, 12, 4}}, out, 32,
                            [&](const void *const *d, void *o, uint32_t m) {
                                return launch_bsdf_eval(c->S, shapes, (const float4 *)d[0], (const float *)d[1],
                                                        (const float *)d[2], m, (float4 *)o, c->stream);
                            });
    });
}

int nori_gpu_bsdf_sample(nori_gpu_ctx *c, const nori_gpu_shading_desc *sd, const nori_gpu_surface *surf, const float *wi,
                         const float *u, float *out) {
    return guarded([&] {
        if (!c || !sd || !surf || !wi || !u || !out) return fail(NORI_ERR_INVALID, "null argument");
        if (sd->reserved != 0) return fail(NORI_ERR_INVALID, "nori_gpu_bsdf_sample: reserved must be 0");
        if (sd->n == 0) return NORI_OK;
        if (!sd->on_device) check_host_records(*c, "nori_gpu_bsdf_sample", surf, sd->n);
        const uint32_t shapes = (uint32_t)c->hshapes.size();
        return shading_call(*c, "nori_gpu_bsdf_sample", *sd, {{surf, 64, 16}, {wi, 12, 4}, {u, 8, 4}}, out, 32,
                            [&](const void *const *d, void *o, uint32_t m) {
                                return launch_bsdf_sample(c->S, shapes, (const float4 *)d[0], (const float *)d[1],
                                                          (const float *)d[2], m, (float4 *)o, c->stream);
                            });
    });
}

int nori_gpu_emitter_sample(nori_gpu_ctx *c, const nori_gpu_shading_desc *sd, const int32_t *ids, const float *x,
                            const float *u, float *out) {
    return guarded([&] {
        if (!c || !sd || !x || !u || !out) return fail(NORI_ERR_INVALID, "null argument");
        if (sd->reserved != 0) return fail(NORI_ERR_INVALID, "nori_gpu_emitter_sample: reserved must be 0");
        if (sd->n == 0) return NORI_OK;
        const int32_t ne = (int32_t)c->S.num_emitters;
        // host arrays: the host can look at every id (device arrays: the kernel's guard gives zeros)
        if (!sd->on_device && !ids && (sd->emitter < 0 || sd->emitter >= ne))
            return fail(NORI_ERR_INVALID, "nori_gpu_emitter_sample: desc->emitter " + std::to_string(sd->emitter) +
                                              " is outside the scene's " + std::to_string(ne) + " emitters");
        if (!sd->on_device && ids)
            for (uint32_t i = 0; i < sd->n; ++i)
                if (ids[i] < 0 || ids[i] >= ne)
                    return fail(NORI_ERR_INVALID, "nori_gpu_emitter_sample: ids[" + std::to_string(i) + "] = " +
                                                      std::to_string(ids[i]) + " is outside the scene's " +
                                                      std::to_string(ne) + " emitters");
        return shading_call(*c, "nori_gpu_emitter_sample", *sd, {{ids, 4, 4}, {x, 12, 4}, {u, 8, 4}}, out, 48,
                            [&](const void *const *d, void *o, uint32_t m) {
                                return launch_emitter_sample(c->S, (const int32_t *)d[0], sd->emitter, (const float *)d[1],
                                                             (const float *)d[2], m, (float4 *)o, c->stream);
                            });
    });
}

int nori_gpu_emitter_eval(nori_gpu_ctx *c, const nori_gpu_shading_desc *sd, const nori_gpu_surface *surf,
                          const float *from, float *out) {
    return guarded([&] {
        if (!c || !sd || !surf || !from || !out) return fail(NORI_ERR_INVALID, "null argument");
        if (sd->reserved != 0) return fail(NORI_ERR_INVALID, "nori_gpu_emitter_eval: reserved must be 0");
        if (sd->n == 0) return NORI_OK;
        if (!sd->on_device) check_host_records(*c, "nori_gpu_emitter_eval", surf, sd->n);
        const uint32_t shapes = (uint32_t)c->hshapes.size();
        return shading_call(*c, "nori_gpu_emitter_eval", *sd, {{surf, 64, 16}, {from, 12, 4}, {nullptr, 0, 4}}, out, 16,
                            [&](const void *const *d, void *o, uint32_t m) {
                                return launch_emitter_eval(c->S, shapes, (const float4 *)d[0], (const float *)d[1], m,
                                                           (float4 *)o, c->stream);
                            });
    });
}

int nori_gpu_sample_uniforms(nori_gpu_ctx *c, const nori_gpu_render_desc *rd, uint32_t first, uint32_t count, float *out) {
    return guarded([&] {
        if (!c || !rd || !out) return fail(NORI_ERR_INVALID, "null argument");
        if (rd->num_blocks && !rd->block_ids) return fail(NORI_ERR_INVALID, "block_ids is null");
        return sample_uniforms(*c, *rd, first, count, out);
    });
}

// The hit record's statement (nori_gpu.h): fp32, the operation order of
// k_surface (kernels_query.hip surface_record), which it is tested against bit for bit.
int nori_scene_surface(const nori_scene_desc *d, uint32_t n, const float *rays, const nori_gpu_hit *hits,
                       nori_gpu_surface *out) {
    return guarded([&] {
        if (!d || !rays || !hits || !out) return fail(NORI_ERR_INVALID, "null argument");
        std::vector<uint32_t> first(d->num_shapes + 1, 0u);  // first global primitive id of each shape
        for (uint32_t s = 0; s < d->num_shapes; ++s)
            first[s + 1] = first[s] + (d->shapes[s].type == NORI_SHAPE_SPHERE ? 1u : d->shapes[s].tri_count);
        auto put3 = [](float *o, V3 v) { o[0] = v.x, o[1] = v.y, o[2] = v.z; };
        auto at3 = [](const float *a, uint32_t i) { return V3{a[3 * (size_t)i], a[3 * (size_t)i + 1], a[3 * (size_t)i + 2]}; };
        for (uint32_t i = 0; i < n; ++i) {
            const nori_gpu_hit &h = hits[i];
            nori_gpu_surface &r = out[i];
            std::memset(&r, 0, sizeof(r));
            if (h.prim < 0) {
                r.t = __builtin_inff();
                r.prim = r.shape = -1;
                continue;
            }
            if ((uint32_t)h.prim >= first[d->num_shapes]) return fail(NORI_ERR_INVALID, "primitive id outside the scene");
            const uint32_t s = (uint32_t)(std::upper_bound(first.begin(), first.end(), (uint32_t)h.prim) - first.begin()) - 1;
            const nori_shape_desc &sd = d->shapes[s];
            const float *ray = rays + 8 * (size_t)i;
            const float t = h.t, u = h.u, v = h.v;
            V3 p, ng, ns;
            V2 uv{u, v};
            if (sd.type == NORI_SHAPE_SPHERE) {
                p = V3{ray[0], ray[1], ray[2]} + V3{ray[4], ray[5], ray[6]} * t;
                ng = ns = normalize(p - V3{sd.center[0], sd.center[1], sd.center[2]});
                float phi = atan2f(ng.y, ng.x);  // sphericalCoordinates (common.cpp:264-272)
                if (phi < 0) phi += 2 * kPi;
                uv.x = (float)(0.5 + (double)(acosf(ng.z) / (2 * kPi)));
                uv.y = phi / kPi;
            } else {
                const uint64_t tri = (uint64_t)sd.tri_offset + ((uint32_t)h.prim - first[s]);
                if (tri >= d->num_triangles || !d->indices || !d->positions) return fail(NORI_ERR_INVALID, "mesh range outside the scene arrays");
                const uint32_t *f = d->indices + 3 * tri;
                if (f[0] >= d->num_vertices || f[1] >= d->num_vertices || f[2] >= d->num_vertices)
                    return fail(NORI_ERR_INVALID, "vertex index out of range");
                const V3 p0 = at3(d->positions, f[0]), p1 = at3(d->positions, f[1]), p2 = at3(d->positions, f[2]);
                const float bx = 1 - (u + v);
                p = (p0 * bx + p1 * u) + p2 * v;
                ng = normalize(cross(p1 - p0, p2 - p0));
                ns = ng;
                if (sd.has_uvs && d->uvs) {
                    const float *a = d->uvs + 2 * (size_t)f[0], *b = d->uvs + 2 * (size_t)f[1], *c = d->uvs + 2 * (size_t)f[2];
                    uv = V2{(bx * a[0] + u * b[0]) + v * c[0], (bx * a[1] + u * b[1]) + v * c[1]};
                }
                if (sd.has_normals) {
                    if (!d->normals) return fail(NORI_ERR_INVALID, "a mesh with normals in a scene without a normal array");
                    ns = normalize((at3(d->normals, f[0]) * bx + at3(d->normals, f[1]) * u) + at3(d->normals, f[2]) * v);
                    if (sd.normal_map >= 0) {  // NormalMap::eval (normalmap.cpp:95-134)
                        if ((uint32_t)sd.normal_map >= d->num_images) return fail(NORI_ERR_INVALID, "image index out of range");
                        const nori_image_desc &im = d->images[sd.normal_map];
                        if (!im.rgb || im.width <= 0 || im.height <= 0) return fail(NORI_ERR_INVALID, "bad image description");
                        const int W = im.width, H = im.height;
                        const float x = uv.x * (float)W, y = uv.y * (float)H;
                        int ix, iy;
                        if (im.wrap == NORI_WRAP_REPEAT) {
                            ix = (int)x % W;
                            iy = (int)y % H;
                            ix += ix < 0 ? W : 0;
                            iy += iy < 0 ? H : 0;
                        } else {
                            ix = std::min(std::max((int)x, 0), W - 1);
                            iy = std::min(std::max((int)y, 0), H - 1);
                        }
                        const uint8_t *tx = im.rgb + 3 * ((size_t)iy * W + ix);
                        const V3 c = V3{(float)tx[0] / 255.0f, (float)tx[1] / 255.0f, (float)tx[2] / 255.0f};
                        const V3 m = V3{2.0f * c.x - 1.0f, 2.0f * c.y - 1.0f, 2.0f * c.z - 1.0f};
                        ns = to_world(frame_from(ns), normalize(m));
                    }
                }
            }
            put3(r.p, p);
            r.t = t;
            put3(r.ng, ng);
            r.prim = h.prim;
            put3(r.ns, ns);
            r.shape = (int32_t)s;
            r.uv[0] = uv.x, r.uv[1] = uv.y;
            r.bary[0] = u, r.bary[1] = v;
        }
        return NORI_OK;
    });
}

// The record's adjoint, its statement (nori_gpu.h): the terms are
// surface_grad.h's, which k_surface_grad compiles too; the sums are float64
// per destination, in hit order.  Everything is formed before anything is
// written, so a refusal leaves the caller's arrays alone.
int nori_scene_surface_grad(const nori_scene_desc *d, const float *positions, const float *normals, uint32_t n,
                            const float *rays, const nori_gpu_hit *hits, const nori_gpu_surface *grad_surf,
                            float *grad_positions, float *grad_normals, float *terms) {
    return guarded([&] {
        if (!d || !rays || !hits || !grad_surf || !grad_positions) return fail(NORI_ERR_INVALID, "null argument");
        const float *P = positions ? positions : d->positions, *Nv = normals ? normals : d->normals;
        const size_t nfl = 3 * (size_t)d->num_vertices;
        for (const float *a : {P, Nv})
            if (a)
                for (size_t k = 0; k < nfl; ++k)
                    if (!std::isfinite(a[k])) return fail(NORI_ERR_INVALID, "nori_scene_surface_grad: a non-finite position or normal");
        std::vector<uint32_t> first(d->num_shapes + 1, 0u);  // first global primitive id of each shape
        for (uint32_t s = 0; s < d->num_shapes; ++s)
            first[s + 1] = first[s] + (d->shapes[s].type == NORI_SHAPE_SPHERE ? 1u : d->shapes[s].tri_count);
        auto at3 = [](const float *a, size_t i) { return V3{a[3 * i], a[3 * i + 1], a[3 * i + 2]}; };
        std::vector<float> tm(18 * (size_t)n, 0.0f);
        std::vector<double> accp(nfl, 0.0), accn(grad_normals ? nfl : 0, 0.0);
        std::vector<uint8_t> hasp(nfl, 0), hasn(grad_normals ? nfl : 0, 0);
        for (uint32_t i = 0; i < n; ++i) {
            const nori_gpu_hit &h = hits[i];
            if (h.prim < 0) continue;
            if ((uint32_t)h.prim >= first[d->num_shapes]) return fail(NORI_ERR_INVALID, "primitive id outside the scene");
            const uint32_t s = (uint32_t)(std::upper_bound(first.begin(), first.end(), (uint32_t)h.prim) - first.begin()) - 1;
            const nori_shape_desc &sd = d->shapes[s];
            if (sd.type == NORI_SHAPE_SPHERE) continue;
            const uint64_t tri = (uint64_t)sd.tri_offset + ((uint32_t)h.prim - first[s]);
            if (tri >= d->num_triangles || !d->indices || !P) return fail(NORI_ERR_INVALID, "mesh range outside the scene arrays");
            const uint32_t *f = d->indices + 3 * tri;
            if (f[0] >= d->num_vertices || f[1] >= d->num_vertices || f[2] >= d->num_vertices)
                return fail(NORI_ERR_INVALID, "vertex index out of range");
            if (sd.has_normals && !Nv) return fail(NORI_ERR_INVALID, "a mesh with normals in a scene without a normal array");
            const float *ray = rays + 8 * (size_t)i;
            const nori_gpu_surface &g = grad_surf[i];
            const V3 g_ng{g.ng[0], g.ng[1], g.ng[2]}, g_ns{g.ns[0], g.ns[1], g.ns[2]};
            V3 tp[3], tn[3];
            if (!surface_grad_positions(at3(P, f[0]), at3(P, f[1]), at3(P, f[2]), V3{ray[0], ray[1], ray[2]},
                                        V3{ray[4], ray[5], ray[6]}, h.t, h.u, h.v, V3{g.p[0], g.p[1], g.p[2]}, g.t,
                                        sd.has_normals ? g_ng : g_ng + g_ns, tp))
                continue;
            const bool with_n = grad_normals && sd.has_normals && sd.normal_map < 0 &&
                                surface_grad_normals(at3(Nv, f[0]), at3(Nv, f[1]), at3(Nv, f[2]), h.u, h.v, g_ns, tn);
            float *t18 = tm.data() + 18 * (size_t)i;
            for (int k = 0; k < 3; ++k) {
                const float pk[3] = {tp[k].x, tp[k].y, tp[k].z};
                for (int a = 0; a < 3; ++a) {
                    t18[3 * k + a] = pk[a];
                    accp[3 * (size_t)f[k] + a] += (double)pk[a];
                    hasp[3 * (size_t)f[k] + a] = 1;
                }
                if (!with_n) continue;
                const float nk[3] = {tn[k].x, tn[k].y, tn[k].z};
                for (int a = 0; a < 3; ++a) {
                    t18[9 + 3 * k + a] = nk[a];
                    accn[3 * (size_t)f[k] + a] += (double)nk[a];
                    hasn[3 * (size_t)f[k] + a] = 1;
                }
            }
        }
        for (size_t k = 0; k < nfl; ++k)
            if (hasp[k]) grad_positions[k] = (float)((double)grad_positions[k] + accp[k]);
        for (size_t k = 0; k < hasn.size(); ++k)
            if (hasn[k]) grad_normals[k] = (float)((double)grad_normals[k] + accn[k]);
        if (terms) std::memcpy(terms, tm.data(), tm.size() * sizeof(float));
        return NORI_OK;
    });
}

int nori_gpu_surface_grad(nori_gpu_ctx *c, const nori_gpu_surface_grad_desc *gd, const float *rays,
                          const nori_gpu_hit *hits, const nori_gpu_surface *grad_surf, float *grad_positions,
                          float *grad_normals, nori_gpu_stats *stats) {
    return guarded([&] {
        if (!c || !gd || !rays || !hits || !grad_surf || !grad_positions) return fail(NORI_ERR_INVALID, "null argument");
        if (gd->reserved[0] != 0 || gd->reserved[1] != 0) return fail(NORI_ERR_INVALID, "nori_gpu_surface_grad: reserved must be 0");
        if (gd->on_device && ((uintptr_t)rays % 16 || (uintptr_t)hits % 16 || (uintptr_t)grad_surf % 16))
            return fail(NORI_ERR_INVALID, "nori_gpu_surface_grad: device rays, hits and grad_surf must be 16-byte aligned");
        if (gd->on_device && ((uintptr_t)grad_positions % 4 || (uintptr_t)grad_normals % 4))
            return fail(NORI_ERR_INVALID, "nori_gpu_surface_grad: device grad_positions and grad_normals must be 4-byte aligned");
        if (gd->n == 0) return NORI_OK;
        return surface_grad(*c, *gd, rays, hits, grad_surf, grad_positions, grad_normals, stats);
    });
}

}  // extern "C"
