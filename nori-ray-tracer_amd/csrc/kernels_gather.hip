// kernels_gather.hip -- the film splat's adjoint (nori_gpu_film_gather /
// nori_gpu_film_gather_passes, stated at nori_film_gather in nori_gpu.h): every
// sample reads the film cells of the window it was splatted into, with the
// same weights, and writes one row of three floats.  k_gather_pos: the layout
// of nori_gpu_camera_rays, one lane per pixel, the block's tile in LDS;
// k_gather_scatter: samples anywhere on the image.  No atomics but the dropped
// samples' count, once per wave.  film_put.h holds the arithmetic they share
// with the host statement and the splat kernels.
#include <algorithm>

#include "film_put.h"
#include "kernels.h"

namespace nori {
namespace {

#ifndef NORI_GATHER_POS_DEPTH
#define NORI_GATHER_POS_DEPTH 4  // samples (20 bytes each) in flight per lane
#endif

// A kept sample's row: for cy ascending, then cx ascending, acc = acc +
// (G[c] * wx) * wy -- the statement's order.  cell(cx, cy): tile cell (cx, cy)
// of the owner's block.  A window has at most floor(2 radius) + 1 <= 2B + 2
// columns, so wx is computed once per column and held in registers.
template <int B, class Cell>
__device__ inline void gather_window(const float *tab, float lk, const PutWindow &w, Cell &&cell, float *out) {
    constexpr int KW = 2 * B + 2;
    const int nx = w.x1 - w.x0 + 1;
    float wx[KW];
#pragma unroll
    for (int d = 0; d < KW; ++d) wx[d] = film_weight(tab, lk, w.x0 + d, w.px);
    float r = 0.0f, g = 0.0f, b = 0.0f;
    for (int cy = w.y0; cy <= w.y1; ++cy) {
        const float wy = film_weight(tab, lk, cy, w.py);
#pragma unroll
        for (int d = 0; d < KW; ++d)
            if (d < nx) {
                const float4 G = cell(w.x0 + d, cy);
                r = r + (G.x * wx[d]) * wy;
                g = g + (G.y * wx[d]) * wy;
                b = b + (G.z * wx[d]) * wy;
            }
    }
    out[0] = r, out[1] = g, out[2] = b;
}

// *dropped += the wave's zero rows (every lane of the wave arrives here)
__device__ inline void count_dropped(uint32_t inval, unsigned long long *dropped) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) inval += __shfl_down(inval, o);
    if ((threadIdx.x & 63) == 0 && inval) atomicAdd(dropped, (unsigned long long)inval);
}

// The passes layout: one work-group per 32x32 block and pass range, as
// k_splat_pos.  The block's tile of grad, (32 + 2B)^2 cells of 16 bytes, is
// staged into LDS once; then one lane per pixel walks its passes with a ring
// of D samples in flight, reads its window from the tile and writes 12 bytes.
// The window is clipped to the tile, so it never leaves it.  val == null: no
// value check.
template <int B>
__global__ __launch_bounds__(kSplatBlock) void k_gather_pos(FilmGeom F, const int4 *blocks, uint32_t passes,
                                                             uint32_t passes_per_wg, uint64_t stride, const float *pos,
                                                             const float *val, const float4 *grad, float *gval,
                                                             unsigned long long *dropped) {
    constexpr int NT = kSplatBlock, D = NORI_GATHER_POS_DEPTH;
    constexpr int TS = NORI_BLOCK_SIZE + 2 * B;
    __shared__ float4 tile[TS * TS];
    __shared__ float ftab[NORI_FILTER_RESOLUTION + 1];
    const int4 bi = blocks[blockIdx.x];
    const int ox = bi.x, oy = bi.y, bw = bi.z & 0xFFFF, bh = bi.z >> 16;
    const uint32_t p0 = blockIdx.y * passes_per_wg, p1 = min(passes, p0 + passes_per_wg);
    const int rows = bh + 2 * B, cols = bw + 2 * B, FW = F.W + 2 * B;
    for (int i = threadIdx.x; i < rows * cols; i += NT) {
        const int yy = i / cols, xx = i - yy * cols;
        tile[yy * TS + xx] = grad[(size_t)(oy + yy) * FW + (ox + xx)];
    }
    if (threadIdx.x <= NORI_FILTER_RESOLUTION) ftab[threadIdx.x] = F.filter[threadIdx.x];
    __syncthreads();
    const int npix = bw * bh;
    const float lk = F.lk;
    uint32_t inval = 0;
    struct Smp {
        float x, y, r, g, b;
    };
    for (int j = threadIdx.x; j < npix; j += NT) {
        const int ly = j / bw, lx = j - ly * bw, x = ox + lx, y = oy + ly;
        const size_t pix = (size_t)y * F.W + x;
        auto load = [&](uint32_t k) {
            const size_t i = (size_t)k * stride + pix;
            const float *p = pos + 2 * i;
            if (!val) return Smp{p[0], p[1], 0.0f, 0.0f, 0.0f};
            const float *v = val + 3 * i;
            return Smp{p[0], p[1], v[0], v[1], v[2]};
        };
        auto row = [&](uint32_t k, const Smp &s) {
            float out[3] = {0.0f, 0.0f, 0.0f};
            PutWindow w;
            if (!film_window(F, true, x, y, s.x, s.y, w) || !film_color_valid(s.r, s.g, s.b))
                ++inval;
            else
                gather_window<B>(ftab, lk, w, [&](int cx, int cy) { return tile[cy * TS + cx]; }, out);
            float *o = gval + 3 * ((size_t)k * stride + pix);
            o[0] = out[0], o[1] = out[1], o[2] = out[2];
        };
        // the next D passes' samples are in flight while one is gathered (a
        // ring of D register sets, the pass loop unrolled by D: no moves)
        Smp q[D];
#pragma unroll
        for (int d = 0; d < D; ++d) q[d] = p0 + d < p1 ? load(p0 + d) : Smp{0, 0, 0, 0, 0};
        for (uint32_t p = p0; p < p1; p += D) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const Smp s = q[d];
                if (p + D + d < p1) q[d] = load(p + D + d);
                if (p + d < p1) row(p + d, s);
            }
        }
    }
    count_dropped(inval, dropped);
}

// Samples anywhere on the image: one lane per sample, the window's cells read
// from global memory as float4 (the film is a few MB and stays in the caches).
constexpr int kGatherBlock = 256;
template <int B>
__global__ __launch_bounds__(kGatherBlock) void k_gather_scatter(FilmGeom F, uint64_t n, const float *pos,
                                                                  const float *val, const float4 *grad, float *gval,
                                                                  unsigned long long *dropped) {
    __shared__ float ftab[NORI_FILTER_RESOLUTION + 1];
    if (threadIdx.x <= NORI_FILTER_RESOLUTION) ftab[threadIdx.x] = F.filter[threadIdx.x];
    __syncthreads();
    const int FW = F.W + 2 * B;
    uint32_t inval = 0;
    const uint64_t step = (uint64_t)gridDim.x * kGatherBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kGatherBlock + threadIdx.x; i < n; i += step) {
        float out[3] = {0.0f, 0.0f, 0.0f};
        PutWindow w;
        bool ok = film_window(F, false, 0, 0, pos[2 * i], pos[2 * i + 1], w);
        if (ok && val) ok = film_color_valid(val[3 * i], val[3 * i + 1], val[3 * i + 2]);
        if (!ok) {
            ++inval;
        } else {
            const float4 *g0 = grad + ((size_t)w.oy * FW + w.ox);
            gather_window<B>(ftab, F.lk, w, [&](int cx, int cy) { return g0[(size_t)cy * FW + cx]; }, out);
        }
        float *o = gval + 3 * i;
        o[0] = out[0], o[1] = out[1], o[2] = out[2];
    }
    count_dropped(inval, dropped);
}

}  // namespace

hipError_t launch_gather_pos(const FilmGeom &F, const int4 *blocks, uint32_t nblocks, uint32_t passes,
                             uint32_t passes_per_wg, uint64_t stride, const float *pos, const float *val,
                             const float *grad, float *gval, unsigned long long *dropped, hipStream_t st) {
    if (nblocks == 0 || passes == 0) return hipSuccess;
    if (passes_per_wg == 0) return hipErrorInvalidValue;
    const dim3 g(nblocks, (passes + passes_per_wg - 1) / passes_per_wg), b(kSplatBlock);
    if (g.y > 65535u) return hipErrorInvalidValue;
    const float4 *grad4 = reinterpret_cast<const float4 *>(grad);
#define NORI_GATHER_POS_CASE(b_)                                                                                     \
    case b_:                                                                                                         \
        hipLaunchKernelGGL((k_gather_pos<b_>), g, b, 0, st, F, blocks, passes, passes_per_wg, stride, pos, val, grad4, \
                           gval, dropped);                                                                           \
        break;
    switch (F.B) {
    NORI_GATHER_POS_CASE(0)
    NORI_GATHER_POS_CASE(1)
    NORI_GATHER_POS_CASE(2)
    NORI_GATHER_POS_CASE(3)
    NORI_GATHER_POS_CASE(4)
    default: return hipErrorInvalidValue;
    }
#undef NORI_GATHER_POS_CASE
    return hipGetLastError();
}

hipError_t launch_gather_scatter(const FilmGeom &F, uint64_t n, const float *pos, const float *val, const float *grad,
                                 float *gval, unsigned long long *dropped, hipStream_t st) {
    if (n == 0) return hipSuccess;
    // grid-stride: at most 2^16 work-groups, a wave's samples adjacent
    const dim3 g((unsigned)std::min<uint64_t>((n + kGatherBlock - 1) / kGatherBlock, 1u << 16)), b(kGatherBlock);
    const float4 *grad4 = reinterpret_cast<const float4 *>(grad);
#define NORI_GATHER_SCATTER_CASE(b_)                                                                     \
    case b_:                                                                                             \
        hipLaunchKernelGGL((k_gather_scatter<b_>), g, b, 0, st, F, n, pos, val, grad4, gval, dropped); \
        break;
    switch (F.B) {
    NORI_GATHER_SCATTER_CASE(0)
    NORI_GATHER_SCATTER_CASE(1)
    NORI_GATHER_SCATTER_CASE(2)
    NORI_GATHER_SCATTER_CASE(3)
    NORI_GATHER_SCATTER_CASE(4)
    default: return hipErrorInvalidValue;
    }
#undef NORI_GATHER_SCATTER_CASE
    return hipGetLastError();
}

}  // namespace nori
