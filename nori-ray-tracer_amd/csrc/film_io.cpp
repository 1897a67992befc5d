// film_io.cpp -- LDR output and the per-pixel variance image.
//
// nori_write_png: Bitmap::saveToLDR (bitmap.cpp:109-139, the hdrToLdr tool):
//   byte = (uint8_t) Clamp(255 * GammaCorrect(v) + 0.5, 0, 255) per channel,
//   GammaCorrect = the sRGB transfer curve (12.92 v below 0.0031308, else
//   1.055 v^(1/2.4) - 0.055, std::pow in float); written as an 8-bit RGB PNG
//   (the reference calls stb_image_write; here zlib deflate, filter type 0).
// nori_film_variance: variance of each pixel's mean radiance from the
//   statistics nori_gpu_render accumulates (render_desc.variance_out).
// nori_film_block_error: the adaptive sampler's per-block error from the same
//   statistics (host version of block_error.hip).
// nori_film_features: first-hit feature sums -> per-pixel means.
// nori_film_denoise_guided: the feature-guided denoiser in double precision
//   (host statement of k_guided, denoise.hip).
// nori_film_splat: caller-supplied samples filtered into the film (the host
//   statement of k_splat_pos / k_splat_scatter, kernels_film.hip).
// nori_film_gather: its adjoint (the host statement of k_gather_pos /
//   k_gather_scatter, kernels_gather.hip).
#include <zlib.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "film_put.h"
#include "scene_prep.h"

namespace {

float gamma_correct(float v) {  // bitmap.cpp:109-112
    if (v <= 0.0031308f) return 12.92f * v;
    return 1.055f * std::pow(v, 1.f / 2.4f) - 0.055f;
}
float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }  // bitmap.cpp:113-120

void be32(std::vector<unsigned char> &b, uint32_t v) {
    for (int s = 24; s >= 0; s -= 8) b.push_back((unsigned char)(v >> s));
}
void chunk(std::vector<unsigned char> &out, const char *type, const std::vector<unsigned char> &data) {
    be32(out, (uint32_t)data.size());
    const size_t at = out.size();
    out.insert(out.end(), type, type + 4);
    out.insert(out.end(), data.begin(), data.end());
    uLong crc = crc32(0L, Z_NULL, 0);
    crc = crc32(crc, out.data() + at, (uInt)(out.size() - at));
    be32(out, (uint32_t)crc);
}

}  // namespace

extern "C" int nori_write_png(const char *path, const float *rgb, int width, int height) {
    if (!path || !rgb || width <= 0 || height <= 0) return NORI_ERR_INVALID;
    // scanlines with a leading filter byte (0 = none)
    const size_t row = 1 + 3 * (size_t)width;
    std::vector<unsigned char> raw(row * (size_t)height);
    for (int y = 0; y < height; ++y) {
        unsigned char *d = raw.data() + row * (size_t)y;
        d[0] = 0;
        for (int x = 0; x < 3 * width; ++x)
            d[1 + x] = (uint8_t)clampf(255.f * gamma_correct(rgb[3 * (size_t)y * width + x]) + 0.5f, 0.f, 255.f);
    }
    uLongf zlen = compressBound((uLong)raw.size());
    std::vector<unsigned char> z(zlen);
    if (compress2(z.data(), &zlen, raw.data(), (uLong)raw.size(), 6) != Z_OK) return NORI_ERR_IO;
    z.resize(zlen);
    std::vector<unsigned char> out = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    std::vector<unsigned char> ihdr;
    be32(ihdr, (uint32_t)width);
    be32(ihdr, (uint32_t)height);
    ihdr.insert(ihdr.end(), {8, 2, 0, 0, 0});  // 8-bit, truecolour, deflate, filter 0, no interlace
    chunk(out, "IHDR", ihdr);
    chunk(out, "IDAT", z);
    chunk(out, "IEND", {});
    FILE *f = std::fopen(path, "wb");
    if (!f) return NORI_ERR_IO;
    const bool ok = std::fwrite(out.data(), 1, out.size(), f) == out.size();
    return std::fclose(f) == 0 && ok ? NORI_OK : NORI_ERR_IO;
}

extern "C" int nori_film_variance(const nori_scene_desc *scene, const float *stats, float *out) {
    if (!scene || !stats || !out) return NORI_ERR_INVALID;
    const size_t n_px = (size_t)scene->camera.width * (size_t)scene->camera.height;
    for (size_t i = 0; i < n_px; ++i) {
        const float *s = stats + 8 * i;
        const double n = s[6];
        for (int c = 0; c < 3; ++c) {
            double v = 0.0;
            if (n >= 2.0) {
                const double s1 = s[c], s2 = s[3 + c];
                v = (s2 - s1 * s1 / n) / (n * (n - 1.0));
                if (v < 0.0) v = 0.0;  // rounding of nearly constant pixels
            }
            out[3 * i + c] = (float)v;
        }
    }
    return NORI_OK;
}

// The adaptive sampler's block error; the metric is stated at its declaration
// (nori_gpu.h).  The device version is k_block_error (block_error.hip).
extern "C" int nori_film_block_error(const nori_scene_desc *scene, const float *stats, float *errors) {
    if (!scene || !stats || !errors) return NORI_ERR_INVALID;
    const int W = scene->camera.width, H = scene->camera.height, bs = NORI_BLOCK_SIZE, sub = 8;
    if (W <= 0 || H <= 0) return NORI_ERR_INVALID;
    const int nbx = (W + bs - 1) / bs, nby = (H + bs - 1) / bs;
    for (int by = 0; by < nby; ++by)
        for (int bx = 0; bx < nbx; ++bx) {
            double worst = 0.0;
            for (int ty = by * bs; ty < std::min((by + 1) * bs, H); ty += sub)
                for (int tx = bx * bs; tx < std::min((bx + 1) * bs, W); tx += sub) {
                    double sum = 0.0;
                    int count = 0;
                    for (int y = ty; y < std::min(ty + sub, H); ++y)
                        for (int x = tx; x < std::min(tx + sub, W); ++x) {
                            const float *s = stats + 8 * ((size_t)y * W + x);
                            const double n = s[6];
                            ++count;
                            if (n < 2.0) continue;
                            double v = 0.0, m = 0.0;
                            for (int c = 0; c < 3; ++c) {
                                const double s1 = s[c], s2 = s[3 + c];
                                v += std::max(0.0, s2 - s1 * s1 / n) / (n * (n - 1.0));
                                m += s1 / n;
                            }
                            sum += std::sqrt(v) / std::sqrt(m + 1e-3);
                        }
                    worst = std::max(worst, sum / count);
                }
            errors[(size_t)by * nbx + bx] = (float)worst;
        }
    return NORI_OK;
}

// First-hit feature sums (nori_gpu_render_features) -> per-pixel means.
extern "C" int nori_film_features(const nori_scene_desc *scene, const float *features, float *out) {
    if (!scene || !features || !out) return NORI_ERR_INVALID;
    if (scene->camera.width <= 0 || scene->camera.height <= 0) return NORI_ERR_INVALID;
    const size_t n_px = (size_t)scene->camera.width * (size_t)scene->camera.height;
    for (size_t i = 0; i < n_px; ++i) {
        const float *s = features + 8 * i;
        const double n = s[7];
        for (int c = 0; c < 7; ++c) out[7 * i + c] = n > 0.0 ? (float)((double)s[c] / n) : 0.0f;
    }
    return NORI_OK;
}

bool nori::guided_desc_valid(const nori_guided_desc *d) {
    if (!d) return false;
    if (d->radius < 0 || d->radius > 8 || d->patch < 0 || d->patch > 3 || d->reserved != 0) return false;
    for (float v : {d->k, d->eps, d->sigma_albedo, d->sigma_normal, d->sigma_depth})
        if (!(v > 0.0f)) return false;  // (NaN fails the comparison)
    return true;
}

// The feature-guided denoiser, stated at its declaration (nori_gpu.h); the
// device version is k_guided (denoise.hip).
extern "C" int nori_film_denoise_guided(const float *rgb, const float *variance, const float *feat7, int width,
                                        int height, const nori_guided_desc *d, float *out) {
    if (!rgb || !variance || !feat7 || !out || width <= 0 || height <= 0 || !nori::guided_desc_valid(d))
        return NORI_ERR_INVALID;
    const int W = width, H = height, R = d->radius, F = d->patch;
    const double k2 = (double)d->k * (double)d->k, eps = d->eps;
    // 1 / sigma^2; 0 switches the term off (a sigma of +inf)
    auto inv2 = [](float s) { return std::isinf(s) ? 0.0 : 1.0 / ((double)s * (double)s); };
    const double ia = inv2(d->sigma_albedo), in = inv2(d->sigma_normal), iz = inv2(d->sigma_depth);
    for (int py = 0; py < H; ++py)
        for (int px = 0; px < W; ++px) {
            const size_t p = (size_t)py * W + px;
            const float *fp = feat7 + 7 * p;
            double acc[3] = {0, 0, 0}, wsum = 0.0;
            for (int sy = -R; sy <= R; ++sy)
                for (int sx = -R; sx <= R; ++sx) {
                    const int qy = py + sy, qx = px + sx;
                    if (qy < 0 || qy >= H || qx < 0 || qx >= W) continue;
                    const size_t q = (size_t)qy * W + qx;
                    double sum = 0.0;
                    int count = 0;
                    for (int oy = -F; oy <= F; ++oy)
                        for (int ox = -F; ox <= F; ++ox) {
                            const int ay = py + oy, ax = px + ox, by = qy + oy, bx = qx + ox;
                            if (ay < 0 || ay >= H || ax < 0 || ax >= W || by < 0 || by >= H || bx < 0 || bx >= W)
                                continue;
                            const size_t a = (size_t)ay * W + ax, b = (size_t)by * W + bx;
                            double sq = 0.0;
                            for (int c = 0; c < 3; ++c) {
                                const double e = (double)rgb[3 * a + c] - (double)rgb[3 * b + c];
                                sq += e * e;
                            }
                            const double va = variance[a], vb = variance[b];
                            sum += (sq - (va + std::min(va, vb))) / (eps + k2 * (va + vb));
                            ++count;
                        }
                    const double d2c = sum / count;  // (o = 0 always counts)
                    const float *fq = feat7 + 7 * q;
                    double d2f = 0.0;
                    if (ia != 0.0) {
                        double t = 0.0;
                        for (int c = 0; c < 3; ++c) t += ((double)fp[c] - fq[c]) * ((double)fp[c] - fq[c]);
                        d2f += t * ia;
                    }
                    if (in != 0.0) {
                        double t = 0.0;
                        for (int c = 3; c < 6; ++c) t += ((double)fp[c] - fq[c]) * ((double)fp[c] - fq[c]);
                        d2f += t * in;
                    }
                    if (iz != 0.0) {
                        const double zp = fp[6], zq = fq[6];
                        const double rel = (zp - zq) / std::max(std::max(zp, zq), 1e-6);
                        d2f += rel * rel * iz;
                    }
                    const double w = std::exp(-std::max(0.0, d2c)) * std::exp(-d2f);
                    for (int c = 0; c < 3; ++c) acc[c] += w * (double)rgb[3 * q + c];
                    wsum += w;
                }
            for (int c = 0; c < 3; ++c) out[3 * p + c] = (float)(acc[c] / wsum);
        }
    return NORI_OK;
}

// ImageBlock::put(pos, value) of caller-supplied samples, stated at its
// declaration (nori_gpu.h); the device versions are k_splat_pos and
// k_splat_scatter (kernels_film.hip), which share film_put.h with it.
extern "C" int nori_film_splat(const nori_scene_desc *scene, uint64_t n, int ordered, const float *pos, const float *val,
                               float *rgbw, float *stats, uint64_t counts[2]) {
    return nori::guarded([&] {
        using namespace nori;
        if (!scene || !pos || !val || !rgbw || !counts) return fail(NORI_ERR_INVALID, "null argument");
        const int W = scene->camera.width, H = scene->camera.height;
        if (W <= 0 || H <= 0) return fail(NORI_ERR_INVALID, "nori_film_splat: an empty frame");
        const uint64_t WH = (uint64_t)W * (uint64_t)H;
        if (ordered && n % WH != 0) return fail(NORI_ERR_INVALID, "nori_film_splat: ordered with n not a multiple of H * W");
        FilmGeom F{};
        F.W = W, F.H = H, F.B = film_border(scene->camera);
        F.rad = scene->camera.filter_radius;
        F.lk = NORI_FILTER_RESOLUTION / scene->camera.filter_radius;
        filter_table(scene->camera, F.filter);
        const int FW = W + 2 * F.B;
        counts[0] = counts[1] = 0;
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t pix = i % WH;
            const float r = val[3 * i], g = val[3 * i + 1], b = val[3 * i + 2];
            PutWindow w;
            if (!film_window(F, ordered != 0, (int)(pix % (uint64_t)W), (int)(pix / (uint64_t)W), pos[2 * i], pos[2 * i + 1], w) ||
                !film_color_valid(r, g, b)) {
                ++counts[1];
                continue;
            }
            ++counts[0];
            if (stats) {
                float *v = stats + 8 * ((size_t)w.y * W + w.x);
                v[0] += r, v[1] += g, v[2] += b;
                v[3] += r * r, v[4] += g * g, v[5] += b * b;
                v[6] += 1.0f;
            }
            for (int cy = w.y0; cy <= w.y1; ++cy) {
                const float wy = film_weight(F.filter, F.lk, cy, w.py);
                for (int cx = w.x0; cx <= w.x1; ++cx) {
                    const float wx = film_weight(F.filter, F.lk, cx, w.px);
                    float *f = rgbw + 4 * ((size_t)(w.oy + cy) * FW + (w.ox + cx));
                    f[0] += (r * wx) * wy;
                    f[1] += (g * wx) * wy;
                    f[2] += (b * wx) * wy;
                    f[3] += (1.0f * wx) * wy;
                }
            }
        }
        return NORI_OK;
    });
}

// The film splat's adjoint, stated at its declaration (nori_gpu.h); the device
// versions are k_gather_pos and k_gather_scatter (kernels_gather.hip).
extern "C" int nori_film_gather(const nori_scene_desc *scene, uint64_t n, int ordered, const float *pos, const float *val,
                                const float *grad_rgbw, float *grad_val, uint64_t counts[2]) {
    return nori::guarded([&] {
        using namespace nori;
        if (!scene || !pos || !grad_rgbw || !grad_val || !counts) return fail(NORI_ERR_INVALID, "null argument");
        const int W = scene->camera.width, H = scene->camera.height;
        if (W <= 0 || H <= 0) return fail(NORI_ERR_INVALID, "nori_film_gather: an empty frame");
        const uint64_t WH = (uint64_t)W * (uint64_t)H;
        if (ordered && n % WH != 0) return fail(NORI_ERR_INVALID, "nori_film_gather: ordered with n not a multiple of H * W");
        FilmGeom F{};
        F.W = W, F.H = H, F.B = film_border(scene->camera);
        F.rad = scene->camera.filter_radius;
        F.lk = NORI_FILTER_RESOLUTION / scene->camera.filter_radius;
        filter_table(scene->camera, F.filter);
        const int FW = W + 2 * F.B;
        counts[0] = counts[1] = 0;
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t pix = i % WH;
            float *out = grad_val + 3 * i;
            out[0] = out[1] = out[2] = 0.0f;
            PutWindow w;
            if (!film_window(F, ordered != 0, (int)(pix % (uint64_t)W), (int)(pix / (uint64_t)W), pos[2 * i], pos[2 * i + 1], w) ||
                (val && !film_color_valid(val[3 * i], val[3 * i + 1], val[3 * i + 2]))) {
                ++counts[1];
                continue;
            }
            ++counts[0];
            for (int cy = w.y0; cy <= w.y1; ++cy) {
                const float wy = film_weight(F.filter, F.lk, cy, w.py);
                for (int cx = w.x0; cx <= w.x1; ++cx) {
                    const float wx = film_weight(F.filter, F.lk, cx, w.px);
                    const float *g = grad_rgbw + 4 * ((size_t)(w.oy + cy) * FW + (w.ox + cx));
                    out[0] = out[0] + (g[0] * wx) * wy;
                    out[1] = out[1] + (g[1] * wx) * wy;
                    out[2] = out[2] + (g[2] * wx) * wy;
                }
            }
        }
        return NORI_OK;
    });
}
