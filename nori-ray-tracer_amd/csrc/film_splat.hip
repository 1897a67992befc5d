// film_splat.hip -- the film opened to callers: nori_gpu_film_splat (samples
// anywhere on the image) and nori_gpu_film_splat_passes (samples in the layout
// of nori_gpu_camera_rays), stated at nori_film_splat in nori_gpu.h.  Device
// arrays are checked and used in place; host arrays pass through the
// context's staging buffers in chunks of at most NORI_QUERY_CHUNK samples, a
// host film is accumulated on the device and added into the caller's once.
// nori_gpu_film_gather / nori_gpu_film_gather_passes are the two calls'
// adjoints (nori_film_gather): a host film is copied to the device once, and
// each chunk's rows are copied back.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"

namespace nori {
namespace {

FilmGeom film_geom(const nori_gpu_ctx &c) {
    FilmGeom F{};
    F.W = c.S.W, F.H = c.S.H, F.B = c.S.border;
    F.rad = c.S.filter_radius, F.lk = c.S.lookup;
    std::memcpy(F.filter, c.S.filter, sizeof(F.filter));
    return F;
}

void check_device_array(const char *name, const char *what, const void *p, size_t align) {
    if ((uintptr_t)p % align)
        throw NoriException(NORI_ERR_INVALID, std::string(name) + ": device " + what + " is not " + std::to_string(align) +
                                                  "-byte aligned");
    require_device_ptr(p, std::string(name) + ": " + what + " is not device memory");
}

// A splat call's target: the checked film and statistics (ctx.h FilmOut), the
// dropped samples' counter and the HIP-event time of the kernels (c.clock).
struct FilmTarget {
    nori_gpu_ctx &c;
    FilmOut out;
    unsigned long long *dropped = nullptr;
    FilmTarget(nori_gpu_ctx &ctx, const char *name, bool dev, float *rgbw, float *variance)
        : c(ctx), out(ctx, dev, rgbw, variance) {
        if (c.S.border > 4) throw NoriException(NORI_ERR_HIP, std::string(name) + ": filter radius above 4.5 pixels");
        if (dev) {
            check_device_array(name, "rgbw", rgbw, 16);
            if (variance) check_device_array(name, "variance_out", variance, 16);
        }
    }
    void begin() {  // (after every check of the call: nothing is launched before)
        out.begin();
        c.counters.ensure(sizeof(Counters));
        HIP_TRY(hipMemsetAsync(c.counters.p, 0, sizeof(Counters), c.stream));
        dropped = &c.counters.as<Counters>()->invalid;
        c.clock.reset(true);
    }
    // One kernel launch, timed; the stream has drained when it returns (so the
    // staging buffers it read may be refilled).
    template <class Launch> void run(Launch &&launch) {
        c.clock.span(c.stream, kKindSplat, launch);
        HIP_TRY(hipStreamSynchronize(c.stream));
        c.clock.collect();
    }
    // The call's statistics; the film and the variance into a host caller's arrays.
    void finish(std::chrono::steady_clock::time_point t0, uint64_t total, nori_gpu_stats *stats) {
        unsigned long long d = 0;
        HIP_TRY(hipMemcpy(&d, dropped, sizeof(d), hipMemcpyDeviceToHost));
        out.finish(false);
        if (!begin_stats(c, t0, stats)) return;
        stats->samples = total - d;
        stats->invalid_samples = d;
        stats->ms_splat = c.clock.ms[kKindSplat];
    }
};

int film_splat(nori_gpu_ctx &c, const nori_gpu_splat_desc &sd, const float *pos, const float *val, float *rgbw,
               nori_gpu_stats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    const char *name = "nori_gpu_film_splat";
    HIP_TRY(hipSetDevice(c.device));
    if (sd.on_device) {
        check_device_array(name, "pos", pos, 4);
        check_device_array(name, "val", val, 4);
    }
    FilmTarget T(c, name, sd.on_device != 0, rgbw, sd.variance_out);
    const FilmGeom F = film_geom(c);
    T.begin();
    if (sd.on_device) {
        T.run([&] {
            return launch_splat_scatter(F, sd.n, kScatterRows, pos, val, T.out.film, T.out.var, T.dropped, c.stream);
        });
    } else {
        const uint64_t chunk = std::min<uint64_t>(sd.n, query_chunk(std::getenv("NORI_QUERY_CHUNK")));
        c.sh_in[0].ensure(8 * (size_t)chunk);
        c.sh_in[1].ensure(12 * (size_t)chunk);
        for (uint64_t i0 = 0; i0 < sd.n; i0 += chunk) {
            const uint64_t m = std::min<uint64_t>(chunk, sd.n - i0);
            HIP_TRY(hipMemcpyAsync(c.sh_in[0].p, pos + 2 * i0, 8 * (size_t)m, hipMemcpyHostToDevice, c.stream));
            HIP_TRY(hipMemcpyAsync(c.sh_in[1].p, val + 3 * i0, 12 * (size_t)m, hipMemcpyHostToDevice, c.stream));
            T.run([&] {
                return launch_splat_scatter(F, m, kScatterRows, c.sh_in[0].as<float>(), c.sh_in[1].as<float>(), T.out.film,
                                            T.out.var, T.dropped, c.stream);
            });
        }
    }
    T.finish(t0, sd.n, stats);
    return NORI_OK;
}

int film_splat_passes(nori_gpu_ctx &c, const nori_gpu_render_desc &rd, const float *pos, const float *val, float *rgbw,
                      nori_gpu_stats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    const char *name = "nori_gpu_film_splat_passes";
    HIP_TRY(hipSetDevice(c.device));
    const uint32_t passes = rd.pass_count ? rd.pass_count : c.scene_spp;
    if (passes == 0) throw NoriException(NORI_ERR_INVALID, std::string(name) + ": nothing to do (pass_count and the scene's sampleCount are 0)");
    if (rd.output_on_device) {
        check_device_array(name, "pos", pos, 4);
        check_device_array(name, "val", val, 4);
    }
    FilmTarget T(c, name, rd.output_on_device != 0, rgbw, rd.variance_out);
    work_lists(c, rd);
    const uint32_t M = (uint32_t)c.hpixels.size(), nblocks = (uint32_t)c.hblocks.size();
    if (M == 0) throw NoriException(NORI_ERR_INVALID, std::string(name) + ": nothing to do (no blocks)");
    const FilmGeom F = film_geom(c);
    const uint64_t WH = (uint64_t)F.W * (uint64_t)F.H;
    const char *per_wg = std::getenv("NORI_SPLAT_POS_PASSES");
    T.begin();
    if (rd.output_on_device) {
        T.run([&] {
            return launch_splat_pos(F, c.blocks.as<int4>(), nblocks, passes, passes_per_wg(passes, nblocks, per_wg), WH, pos,
                                    val, T.out.film, T.out.var, T.dropped, c.stream);
        });
    } else {
        // whole passes: as many as fit NORI_QUERY_CHUNK samples, at least one
        const uint64_t most = query_chunk(std::getenv("NORI_QUERY_CHUNK"));
        const uint32_t kp = (uint32_t)std::min<uint64_t>(passes, std::max<uint64_t>(1, most / WH));
        c.sh_in[0].ensure(8 * (size_t)kp * WH);
        c.sh_in[1].ensure(12 * (size_t)kp * WH);
        for (uint32_t k0 = 0; k0 < passes; k0 += kp) {
            const uint32_t np = std::min(kp, passes - k0);
            const size_t i0 = (size_t)k0 * WH, m = (size_t)np * WH;
            HIP_TRY(hipMemcpyAsync(c.sh_in[0].p, pos + 2 * i0, 8 * m, hipMemcpyHostToDevice, c.stream));
            HIP_TRY(hipMemcpyAsync(c.sh_in[1].p, val + 3 * i0, 12 * m, hipMemcpyHostToDevice, c.stream));
            T.run([&] {
                return launch_splat_pos(F, c.blocks.as<int4>(), nblocks, np, passes_per_wg(np, nblocks, per_wg), WH,
                                        c.sh_in[0].as<float>(), c.sh_in[1].as<float>(), T.out.film, T.out.var, T.dropped,
                                        c.stream);
            });
        }
    }
    T.finish(t0, (uint64_t)passes * M, stats);
    return NORI_OK;
}

// A gather call (the splat's adjoint, stated at nori_film_gather in
// nori_gpu.h): the film it reads on the device -- the caller's own, or a copy of
// a host film in c.film --, the zero rows' counter and the kernels' time.
struct GatherRun {
    nori_gpu_ctx &c;
    const bool on_device;
    const float *grad = nullptr;
    unsigned long long *dropped = nullptr;
    GatherRun(nori_gpu_ctx &ctx, const char *name, bool dev, const float *pos, const float *val, const float *grad_rgbw,
              const float *grad_val)
        : c(ctx), on_device(dev) {
        if (dev) {
            check_device_array(name, "pos", pos, 4);
            if (val) check_device_array(name, "val", val, 4);
            check_device_array(name, "grad_rgbw", grad_rgbw, 16);
            check_device_array(name, "grad_val", grad_val, 4);
        }
        if (c.S.border > 4) throw NoriException(NORI_ERR_HIP, std::string(name) + ": filter radius above 4.5 pixels");
    }
    void begin(const float *grad_rgbw) {  // (after every check of the call: nothing is launched before)
        grad = grad_rgbw;
        if (!on_device) {
            const size_t bytes = 16 * (size_t)(c.S.W + 2 * c.S.border) * (size_t)(c.S.H + 2 * c.S.border);
            c.film.ensure(bytes);
            HIP_TRY(hipMemcpyAsync(c.film.p, grad_rgbw, bytes, hipMemcpyHostToDevice, c.stream));
            grad = c.film.as<float>();
        }
        c.counters.ensure(sizeof(Counters));
        HIP_TRY(hipMemsetAsync(c.counters.p, 0, sizeof(Counters), c.stream));
        dropped = &c.counters.as<Counters>()->invalid;
        c.clock.reset(true);
    }
    template <class Launch> void run(Launch &&launch) {  // as FilmTarget::run
        c.clock.span(c.stream, kKindSplat, launch);
        HIP_TRY(hipStreamSynchronize(c.stream));
        c.clock.collect();
    }
    void finish(std::chrono::steady_clock::time_point t0, uint64_t total, nori_gpu_stats *stats) {
        unsigned long long d = 0;
        HIP_TRY(hipMemcpy(&d, dropped, sizeof(d), hipMemcpyDeviceToHost));
        if (!begin_stats(c, t0, stats)) return;
        stats->samples = total - d;
        stats->invalid_samples = d;
        stats->ms_splat = c.clock.ms[kKindSplat];
    }
};

int film_gather(nori_gpu_ctx &c, const nori_gpu_gather_desc &gd, const float *pos, const float *val, const float *grad_rgbw,
                float *grad_val, nori_gpu_stats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(c.device));
    GatherRun G(c, "nori_gpu_film_gather", gd.on_device != 0, pos, val, grad_rgbw, grad_val);
    const FilmGeom F = film_geom(c);
    G.begin(grad_rgbw);
    if (gd.on_device) {
        G.run([&] { return launch_gather_scatter(F, gd.n, pos, val, G.grad, grad_val, G.dropped, c.stream); });
    } else {
        const uint64_t chunk = std::min<uint64_t>(gd.n, query_chunk(std::getenv("NORI_QUERY_CHUNK")));
        c.sh_in[0].ensure(8 * (size_t)chunk);
        if (val) c.sh_in[1].ensure(12 * (size_t)chunk);
        c.sh_out.ensure(12 * (size_t)chunk);
        for (uint64_t i0 = 0; i0 < gd.n; i0 += chunk) {
            const uint64_t m = std::min<uint64_t>(chunk, gd.n - i0);
            HIP_TRY(hipMemcpyAsync(c.sh_in[0].p, pos + 2 * i0, 8 * (size_t)m, hipMemcpyHostToDevice, c.stream));
            if (val) HIP_TRY(hipMemcpyAsync(c.sh_in[1].p, val + 3 * i0, 12 * (size_t)m, hipMemcpyHostToDevice, c.stream));
            G.run([&] {
                return launch_gather_scatter(F, m, c.sh_in[0].as<float>(), val ? c.sh_in[1].as<float>() : nullptr, G.grad,
                                             c.sh_out.as<float>(), G.dropped, c.stream);
            });
            HIP_TRY(hipMemcpy(grad_val + 3 * i0, c.sh_out.p, 12 * (size_t)m, hipMemcpyDeviceToHost));
        }
    }
    G.finish(t0, gd.n, stats);
    return NORI_OK;
}

int film_gather_passes(nori_gpu_ctx &c, const nori_gpu_render_desc &rd, const float *pos, const float *val,
                       const float *grad_rgbw, float *grad_val, nori_gpu_stats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    const char *name = "nori_gpu_film_gather_passes";
    HIP_TRY(hipSetDevice(c.device));
    const uint32_t passes = rd.pass_count ? rd.pass_count : c.scene_spp;
    if (passes == 0) throw NoriException(NORI_ERR_INVALID, std::string(name) + ": nothing to do (pass_count and the scene's sampleCount are 0)");
    GatherRun G(c, name, rd.output_on_device != 0, pos, val, grad_rgbw, grad_val);
    work_lists(c, rd);
    const uint32_t M = (uint32_t)c.hpixels.size(), nblocks = (uint32_t)c.hblocks.size();
    if (M == 0) throw NoriException(NORI_ERR_INVALID, std::string(name) + ": nothing to do (no blocks)");
    const FilmGeom F = film_geom(c);
    const uint64_t WH = (uint64_t)F.W * (uint64_t)F.H;
    const char *per_wg = std::getenv("NORI_GATHER_PASSES");
    auto range = [&](uint32_t np) { return gather_passes(np, nblocks, per_wg); };
    G.begin(grad_rgbw);
    if (rd.output_on_device) {
        G.run([&] {
            return launch_gather_pos(F, c.blocks.as<int4>(), nblocks, passes, range(passes), WH, pos, val, G.grad, grad_val,
                                     G.dropped, c.stream);
        });
    } else {
        // whole passes: as many as fit NORI_QUERY_CHUNK samples, at least one
        const uint64_t most = query_chunk(std::getenv("NORI_QUERY_CHUNK"));
        const uint32_t kp = (uint32_t)std::min<uint64_t>(passes, std::max<uint64_t>(1, most / WH));
        c.sh_in[0].ensure(8 * (size_t)kp * WH);
        if (val) c.sh_in[1].ensure(12 * (size_t)kp * WH);
        c.sh_out.ensure(12 * (size_t)kp * WH);
        for (uint32_t k0 = 0; k0 < passes; k0 += kp) {
            const uint32_t np = std::min(kp, passes - k0);
            const size_t i0 = (size_t)k0 * WH, m = (size_t)np * WH;
            HIP_TRY(hipMemcpyAsync(c.sh_in[0].p, pos + 2 * i0, 8 * m, hipMemcpyHostToDevice, c.stream));
            if (val) HIP_TRY(hipMemcpyAsync(c.sh_in[1].p, val + 3 * i0, 12 * m, hipMemcpyHostToDevice, c.stream));
            // a block subset: the rows of the other blocks' pixels go back as they came
            if (rd.num_blocks) HIP_TRY(hipMemcpyAsync(c.sh_out.p, grad_val + 3 * i0, 12 * m, hipMemcpyHostToDevice, c.stream));
            G.run([&] {
                return launch_gather_pos(F, c.blocks.as<int4>(), nblocks, np, range(np), WH, c.sh_in[0].as<float>(), val ? c.sh_in[1].as<float>() : nullptr, G.grad,
                                         c.sh_out.as<float>(), G.dropped, c.stream);
            });
            HIP_TRY(hipMemcpy(grad_val + 3 * i0, c.sh_out.p, 12 * m, hipMemcpyDeviceToHost));
        }
    }
    G.finish(t0, (uint64_t)passes * M, stats);
    return NORI_OK;
}

}  // namespace
}  // namespace nori

extern "C" {

int nori_gpu_film_splat(nori_gpu_ctx *c, const nori_gpu_splat_desc *sd, const float *pos, const float *val, float *rgbw,
                        nori_gpu_stats *stats) {
    return guarded([&] {
        if (!c || !sd || !pos || !val || !rgbw) return fail(NORI_ERR_INVALID, "null argument");
        if (sd->reserved != 0) return fail(NORI_ERR_INVALID, "nori_gpu_film_splat: reserved must be 0");
        if (sd->n == 0) return NORI_OK;
        return film_splat(*c, *sd, pos, val, rgbw, stats);
    });
}

int nori_gpu_film_splat_passes(nori_gpu_ctx *c, const nori_gpu_render_desc *rd, const float *pos, const float *val,
                               float *rgbw, nori_gpu_stats *stats) {
    return guarded([&] {
        if (!c || !rd || !pos || !val || !rgbw) return fail(NORI_ERR_INVALID, "null argument");
        if (rd->num_blocks && !rd->block_ids) return fail(NORI_ERR_INVALID, "block_ids is null");
        return film_splat_passes(*c, *rd, pos, val, rgbw, stats);
    });
}

int nori_gpu_film_gather(nori_gpu_ctx *c, const nori_gpu_gather_desc *gd, const float *pos, const float *val,
                         const float *grad_rgbw, float *grad_val, nori_gpu_stats *stats) {
    return guarded([&] {
        if (!c || !gd || !pos || !grad_rgbw || !grad_val) return fail(NORI_ERR_INVALID, "null argument");
        if (gd->reserved != 0) return fail(NORI_ERR_INVALID, "nori_gpu_film_gather: reserved must be 0");
        if (gd->n == 0) return NORI_OK;
        return film_gather(*c, *gd, pos, val, grad_rgbw, grad_val, stats);
    });
}

int nori_gpu_film_gather_passes(nori_gpu_ctx *c, const nori_gpu_render_desc *rd, const float *pos, const float *val,
                                const float *grad_rgbw, float *grad_val, nori_gpu_stats *stats) {
    return guarded([&] {
        if (!c || !rd || !pos || !grad_rgbw || !grad_val) return fail(NORI_ERR_INVALID, "null argument");
        if (rd->num_blocks && !rd->block_ids) return fail(NORI_ERR_INVALID, "block_ids is null");
        return film_gather_passes(*c, *rd, pos, val, grad_rgbw, grad_val, stats);
    });
}

}  // extern "C"
