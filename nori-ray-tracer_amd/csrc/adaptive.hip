// adaptive.hip -- what follows a render: the per-block error metric, the
// adaptive rounds over render() (ctx.h), and the two denoisers' entry points.
#include <algorithm>
#include <string>
#include <vector>

#include "ctx.h"

namespace nori {
namespace {

int frame_blocks(const nori_gpu_ctx &c, int *nbx_out = nullptr) {
    const int nbx = (c.S.W + NORI_BLOCK_SIZE - 1) / NORI_BLOCK_SIZE, nby = (c.S.H + NORI_BLOCK_SIZE - 1) / NORI_BLOCK_SIZE;
    if (nbx_out) *nbx_out = nbx;
    return nbx * nby;
}

// nori_gpu_block_error: the metric of `stats` for every block of the frame.
int block_error(nori_gpu_ctx &c, const float *stats, bool on_device, float *errors) {
    HIP_TRY(hipSetDevice(c.device));
    int nbx = 0;
    const int nb = frame_blocks(c, &nbx);
    const size_t n = 8 * (size_t)c.S.W * (size_t)c.S.H;
    const float *dev = stats;
    if (on_device) {
        if ((uintptr_t)stats % 16) throw NoriException(NORI_ERR_INVALID, "device statistics must be 16-byte aligned");
    } else {
        c.varbuf.ensure(n * sizeof(float));
        HIP_TRY(hipMemcpyAsync(c.varbuf.p, stats, n * sizeof(float), hipMemcpyHostToDevice, c.stream));
        dev = c.varbuf.as<float>();
    }
    c.errbuf.ensure((size_t)nb * sizeof(float));
    HIP_TRY(launch_block_error(dev, c.S.W, c.S.H, nbx, nullptr, (uint32_t)nb, c.errbuf.as<float>(), c.stream));
    HIP_TRY(hipMemcpyAsync(errors, c.errbuf.p, (size_t)nb * sizeof(float), hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    return NORI_OK;
}

// nori_gpu_render_adaptive (nori_gpu.h has the schedule): one render() per
// round on the blocks still active, film and statistics resident on the
// device throughout; per round only the block errors come back.
int render_adaptive(nori_gpu_ctx &c, const nori_gpu_render_desc &rd0, const nori_gpu_adaptive_desc &ad, float *rgbw_out,
                    nori_gpu_stats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(c.device));
    const uint32_t cap = ad.max_passes ? ad.max_passes : c.spp;
    if (ad.min_passes < 2) throw NoriException(NORI_ERR_INVALID, "adaptive: min_passes must be at least 2");
    if (cap < ad.min_passes) throw NoriException(NORI_ERR_INVALID, "adaptive: the pass cap is below min_passes");
    if (!(ad.threshold >= 0.0f)) throw NoriException(NORI_ERR_INVALID, "adaptive: threshold is negative or NaN");
    if (ad.reserved != 0) throw NoriException(NORI_ERR_INVALID, "adaptive: reserved must be 0");
    if ((uint64_t)rd0.pass_begin + cap > 0xFFFFFFFFull) throw NoriException(NORI_ERR_INVALID, "adaptive: pass range overflows");
    const int W = c.S.W, H = c.S.H;
    int nbx = 0;
    const uint32_t nb = (uint32_t)frame_blocks(c, &nbx);
    // the selected blocks, ascending, duplicates dropped
    std::vector<uint32_t> active;
    if (rd0.num_blocks) {
        std::vector<char> want(nb, 0);
        for (uint32_t i = 0; i < rd0.num_blocks; ++i) {
            if (rd0.block_ids[i] >= nb) throw NoriException(NORI_ERR_INVALID, "block id out of range");
            want[rd0.block_ids[i]] = 1;
        }
        for (uint32_t b = 0; b < nb; ++b)
            if (want[b]) active.push_back(b);
    } else {
        active.resize(nb);
        for (uint32_t b = 0; b < nb; ++b) active[b] = b;
    }
    auto block_pixels = [&](uint32_t b) {
        const int ox = (int)(b % (uint32_t)nbx) * NORI_BLOCK_SIZE, oy = (int)(b / (uint32_t)nbx) * NORI_BLOCK_SIZE;
        return (uint64_t)std::min(NORI_BLOCK_SIZE, W - ox) * (uint64_t)std::min(NORI_BLOCK_SIZE, H - oy);
    };
    auto pixels_of = [&](const std::vector<uint32_t> &ids) {
        uint64_t m = 0;
        for (uint32_t b : ids) m += block_pixels(b);
        return m;
    };
    const double bound = (double)cap * (double)pixels_of(active);  // samples if no block stops early

    // (the statistics are always gathered, in c.varbuf: the rounds' errors are read from them)
    const size_t var_elems = 8 * (size_t)W * (size_t)H;
    FilmOut out(c, rd0.output_on_device != 0, rgbw_out);
    out.begin();
    c.varbuf.ensure(var_elems * sizeof(float));
    c.errbuf.ensure((size_t)nb * sizeof(float));
    c.errids.ensure((size_t)nb * sizeof(uint32_t));
    HIP_TRY(hipMemsetAsync(c.varbuf.p, 0, var_elems * sizeof(float), c.stream));
    HIP_TRY(hipMemsetAsync(c.errbuf.p, 0, (size_t)nb * sizeof(float), c.stream));

    struct Rounds {  // the context reports plain renders as before once the call is over
        nori_gpu_ctx &c;
        explicit Rounds(nori_gpu_ctx &ctx) : c(ctx) {
            c.in_rounds = true;
            c.prog_off = c.prog_scale = 0.0;
        }
        ~Rounds() {
            c.progress = 1.0f;
            c.in_rounds = false;
            c.prog_off = 0.0;
            c.prog_scale = 1.0;
        }
    } rounds(c);
    c.cancel = 0;
    c.progress = 0.0f;

    std::vector<uint32_t> passes(nb, 0);
    std::vector<float> herr(nb, 0.0f);
    nori_gpu_stats sum{}, rs{};
    uint32_t have = 0, np = ad.min_passes;
    while (!active.empty()) {
        if (c.cancel.load()) return fail(NORI_ERR_CANCELLED, "rendering was cancelled");
        const double round_samples = (double)np * (double)pixels_of(active);
        c.prog_off += c.prog_scale;  // where the last round ended, to the bit: the progress never steps back
        c.prog_scale = round_samples / bound;
        nori_gpu_render_desc rd = rd0;
        rd.pass_begin = rd0.pass_begin + have;
        rd.pass_count = np;
        rd.num_blocks = (uint32_t)active.size();
        rd.block_ids = active.data();
        rd.output_on_device = 1;
        rd.variance_out = c.varbuf.as<float>();
        const int rc = render(c, rd, out.film, &rs);
        if (rc != NORI_OK) return rc;
        sum.samples += rs.samples;
        sum.invalid_samples += rs.invalid_samples;
        sum.rays_closest += rs.rays_closest;
        sum.rays_shadow += rs.rays_shadow;
        sum.rays_finish += rs.rays_finish;
        sum.iterations += rs.iterations;
        sum.ms_extend += rs.ms_extend;
        sum.ms_shadow += rs.ms_shadow;
        sum.ms_shade += rs.ms_shade;
        sum.ms_splat += rs.ms_splat;
        sum.ms_finish += rs.ms_finish;
        have += np;
        for (uint32_t b : active) passes[b] = have;
        // E_b of the blocks just rendered (the others' statistics did not change)
        HIP_TRY(hipMemcpyAsync(c.errids.p, active.data(), active.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
        HIP_TRY(launch_block_error(c.varbuf.as<float>(), W, H, nbx, c.errids.as<uint32_t>(), (uint32_t)active.size(),
                                   c.errbuf.as<float>(), c.stream));
        HIP_TRY(hipMemcpyAsync(herr.data(), c.errbuf.p, (size_t)nb * sizeof(float), hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));  // (also orders the pageable upload of `active` before it changes)
        if (have >= cap) break;
        std::vector<uint32_t> next;
        for (uint32_t b : active)
            if (herr[b] > ad.threshold) next.push_back(b);
        active.swap(next);
        np = std::min(have, cap - have);
    }
    if (c.cancel.load()) return fail(NORI_ERR_CANCELLED, "rendering was cancelled");

    out.finish(false);
    if (!rd0.output_on_device && rd0.variance_out) {
        std::vector<float> hv(var_elems);
        HIP_TRY(hipMemcpy(hv.data(), c.varbuf.p, var_elems * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < var_elems; ++i) rd0.variance_out[i] += hv[i];
    } else if (rd0.output_on_device && rd0.variance_out) {
        HIP_TRY(launch_add_into(rd0.variance_out, c.varbuf.as<float>(), var_elems, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
    }
    if (ad.passes_out) std::copy(passes.begin(), passes.end(), ad.passes_out);
    if (ad.error_out) std::copy(herr.begin(), herr.end(), ad.error_out);
    c.progress = 1.0f;
    if (stats) {
        *stats = rs;  // the scene and pool fields of the last round
        stats->samples = sum.samples;
        stats->invalid_samples = sum.invalid_samples;
        stats->rays_closest = sum.rays_closest;
        stats->rays_shadow = sum.rays_shadow;
        stats->rays_finish = sum.rays_finish;
        stats->iterations = sum.iterations;
        stats->ms_extend = sum.ms_extend;
        stats->ms_shadow = sum.ms_shadow;
        stats->ms_shade = sum.ms_shade;
        stats->ms_splat = sum.ms_splat;
        stats->ms_finish = sum.ms_finish;
        stats->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return NORI_OK;
}

}  // namespace
}  // namespace nori

extern "C" {

// denoiser/denoiser.py (NL-means over a rendered image and its per-pixel
// variance) on device `device`: host buffers in, host buffer out.
int nori_denoise(int device, const float *rgb, const float *variance, int width, int height, int radius, int patch,
                 float k, int mode, float *out) {
    return guarded([&] {
        if (!rgb || !variance || !out || width <= 0 || height <= 0 || radius < 0 || radius > 8 || patch < 1 ||
            patch > 5 || mode < 0 || mode > 1 || !(k > 0.0f))
            return fail(NORI_ERR_INVALID, "nori_denoise: invalid arguments");
        HIP_TRY(hipSetDevice(device));
        {  // the tile + halo staging must fit one work-group's LDS
            int lds_max = 0;
            HIP_TRY(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
            const size_t need = denoise_lds_bytes(radius, patch - 1);
            if (need > (size_t)lds_max)
                return fail(NORI_ERR_INVALID, "nori_denoise: radius " + std::to_string(radius) + " / patch " +
                                                  std::to_string(patch) + " need " + std::to_string(need) +
                                                  " bytes of LDS per work-group, the device has " +
                                                  std::to_string(lds_max));
        }
        const size_t n = (size_t)width * (size_t)height;
        DevBuf di, dv, dout;
        di.ensure(12 * n);
        dv.ensure(4 * n);
        dout.ensure(12 * n);
        HIP_TRY(hipMemcpy(di.p, rgb, 12 * n, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dv.p, variance, 4 * n, hipMemcpyHostToDevice));
        HIP_TRY(launch_denoise((const float *)di.p, (const float *)dv.p, width, height, radius, patch - 1, k, mode,
                               (float *)dout.p, nullptr));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(out, dout.p, 12 * n, hipMemcpyDeviceToHost));
        return (int)NORI_OK;
    });
}
// The feature-guided denoiser (nori_film_denoise_guided states it) on device
// `device`: host buffers in, host buffer out.
int nori_denoise_guided(int device, const float *rgb, const float *variance, const float *feat7, int width, int height,
                        const nori_guided_desc *d, float *out) {
    return guarded([&] {
        if (!rgb || !variance || !feat7 || !out || width <= 0 || height <= 0 || !guided_desc_valid(d))
            return fail(NORI_ERR_INVALID, "nori_denoise_guided: invalid arguments");
        HIP_TRY(hipSetDevice(device));
        {  // the tile + halo staging must fit one work-group's LDS
            int lds_max = 0;
            HIP_TRY(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
            const size_t need = guided_lds_bytes(d->radius, d->patch);
            if (need > (size_t)lds_max)
                return fail(NORI_ERR_INVALID, "nori_denoise_guided: radius " + std::to_string(d->radius) + " / patch " +
                                                  std::to_string(d->patch) + " need " + std::to_string(need) +
                                                  " bytes of LDS per work-group, the device has " +
                                                  std::to_string(lds_max));
        }
        const size_t n = (size_t)width * (size_t)height;
        DevBuf di, dv, df, dout;
        di.ensure(12 * n);
        dv.ensure(4 * n);
        df.ensure(28 * n);
        dout.ensure(12 * n);
        HIP_TRY(hipMemcpy(di.p, rgb, 12 * n, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dv.p, variance, 4 * n, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(df.p, feat7, 28 * n, hipMemcpyHostToDevice));
        HIP_TRY(launch_guided((const float *)di.p, (const float *)dv.p, (const float *)df.p, width, height, d->radius,
                              d->patch, d->k, d->eps, d->sigma_albedo, d->sigma_normal, d->sigma_depth,
                              (float *)dout.p, nullptr));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(out, dout.p, 12 * n, hipMemcpyDeviceToHost));
        return (int)NORI_OK;
    });
}

int nori_gpu_block_error(nori_gpu_ctx *c, const float *stats, int stats_on_device, float *errors) {
    return guarded([&] {
        if (!c || !stats || !errors) return fail(NORI_ERR_INVALID, "null argument");
        return block_error(*c, stats, stats_on_device != 0, errors);
    });
}

int nori_gpu_render_adaptive(nori_gpu_ctx *c, const nori_gpu_render_desc *rd, const nori_gpu_adaptive_desc *ad,
                             float *rgbw_out, nori_gpu_stats *stats) {
    return guarded([&] {
        if (!c || !rd || !ad || !rgbw_out) return fail(NORI_ERR_INVALID, "null argument");
        if (rd->num_blocks && !rd->block_ids) return fail(NORI_ERR_INVALID, "block_ids is null");
        return render_adaptive(*c, *rd, *ad, rgbw_out, stats);
    });
}


}  // extern "C"
