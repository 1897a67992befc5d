// film_put.h -- ImageBlock::put(pos, value) for a caller-supplied sample, as
// stated at nori_film_splat in nori_gpu.h: the owner pixel, the drop rules and
// the window of the owner's 32x32 block.  Plain float code shared by the host
// statement (film_io.cpp, host compiler) and the film-splat kernels
// (kernels_film.hip); every operation is a single float operation in the
// order of splat_sample (shading.h) and k_splat (kernels.hip).
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/nori_gpu.h"

#if defined(__HIPCC__)
#define NORI_FILM_HD __host__ __device__ inline
#else
#define NORI_FILM_HD inline
#endif

namespace nori {

// What the put needs of a scene: the frame, the border and the tabulated filter.
struct FilmGeom {
    int32_t W, H, B;
    float rad, lk;  // filter radius; NORI_FILTER_RESOLUTION / radius
    float filter[NORI_FILTER_RESOLUTION + 1];
};

// A kept sample: its owner (x, y), the owner's block origin, the position
// relative to the block's tile (border included) and the clipped window
// [x0, x1] x [y0, y1] in tile cells.
struct PutWindow {
    int32_t x, y, ox, oy, x0, x1, y0, y1;
    float px, py;
};

NORI_FILM_HD bool film_finite(float v) { return __builtin_isfinite(v); }
// Color3f::isValid (common.cpp:224-231)
NORI_FILM_HD bool film_color_valid(float r, float g, float b) {
    return !(r < 0 || !film_finite(r) || g < 0 || !film_finite(g) || b < 0 || !film_finite(b));
}
NORI_FILM_HD int32_t film_imin(int32_t a, int32_t b) { return a < b ? a : b; }
NORI_FILM_HD int32_t film_imax(int32_t a, int32_t b) { return a > b ? a : b; }

// Steps 1 and 2 (position part) and the window of step 3.  ordered: (x, y) is
// the owner and the position must lie in its closed square; else the owner is
// the floor of the position.  false: the sample is dropped.
NORI_FILM_HD bool film_window(const FilmGeom &F, bool ordered, int32_t x, int32_t y, float sx, float sy, PutWindow &w) {
    if (!film_finite(sx) || !film_finite(sy)) return false;
    if (ordered) {
        if (!(sx >= (float)x && sx <= (float)(x + 1) && sy >= (float)y && sy <= (float)(y + 1))) return false;
    } else {
        const float fx = floorf(sx), fy = floorf(sy);
        if (!(fx >= 0.0f && fx < (float)F.W && fy >= 0.0f && fy < (float)F.H)) return false;
        x = (int32_t)fx;
        y = (int32_t)fy;
    }
    const int32_t B = F.B;
    w.x = x;
    w.y = y;
    w.ox = (x / NORI_BLOCK_SIZE) * NORI_BLOCK_SIZE;
    w.oy = (y / NORI_BLOCK_SIZE) * NORI_BLOCK_SIZE;
    const int32_t bw = film_imin(NORI_BLOCK_SIZE, F.W - w.ox), bh = film_imin(NORI_BLOCK_SIZE, F.H - w.oy);
    w.px = sx - 0.5f - (float)(w.ox - B);
    w.py = sy - 0.5f - (float)(w.oy - B);
    // the block's own tile (the reference's m_size-based clip): never leaves the film
    w.x0 = film_imax((int32_t)ceilf(w.px - F.rad), 0);
    w.y0 = film_imax((int32_t)ceilf(w.py - F.rad), 0);
    w.x1 = film_imin((int32_t)floorf(w.px + F.rad), bw + 2 * B - 1);
    w.y1 = film_imin((int32_t)floorf(w.py + F.rad), bh + 2 * B - 1);
    return true;
}

// The tabulated weight of tile cell c for a sample at tile position p.
NORI_FILM_HD float film_weight(const float *table, float lk, int32_t c, float p) {
    return table[film_imin((int32_t)(fabsf((float)c - p) * lk), NORI_FILTER_RESOLUTION)];
}

}  // namespace nori
