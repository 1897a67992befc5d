// kernels_film.hip -- the film opened to callers: ImageBlock::put(pos, value)
// of samples whose positions and values come from the caller's arrays
// (nori_gpu_film_splat / nori_gpu_film_splat_passes, stated at nori_film_splat
// in nori_gpu.h).  k_splat_pos: the layout of nori_gpu_camera_rays, one lane
// per pixel; k_splat_scatter: samples anywhere on the image.  film_put.h holds
// the arithmetic they share with the host statement.
#include <algorithm>

#include "film_put.h"
#include "kernels.h"

namespace nori {
namespace {

// One kept sample straight into the film with float atomics: splat_sample's
// body (shading.h) on a caller's position.  tab: the filter table.
__device__ inline void put_atomic(const FilmGeom &F, const float *tab, float *film, float *var, const PutWindow &w,
                                  float r, float g, float b) {
    if (var) {  // the owner's sample statistics (nori_gpu_render_desc.variance_out)
        float *v = var + 8 * ((size_t)w.y * F.W + w.x);
        atomicAdd(v + 0, r);
        atomicAdd(v + 1, g);
        atomicAdd(v + 2, b);
        atomicAdd(v + 3, r * r);
        atomicAdd(v + 4, g * g);
        atomicAdd(v + 5, b * b);
        atomicAdd(v + 6, 1.0f);
    }
    const int FW = F.W + 2 * F.B;
    for (int cy = w.y0; cy <= w.y1; ++cy) {
        const float wy = film_weight(tab, F.lk, cy, w.py);
        for (int cx = w.x0; cx <= w.x1; ++cx) {
            const float wx = film_weight(tab, F.lk, cx, w.px);
            float *f = film + 4 * ((size_t)(w.oy + cy) * FW + (w.ox + cx));
            const float a = (r * wx) * wy, c = (g * wx) * wy, d = (b * wx) * wy, e = (1.0f * wx) * wy;
            if (e != 0.0f || a != 0.0f || c != 0.0f || d != 0.0f) {
                atomicAdd(f + 0, a);
                atomicAdd(f + 1, c);
                atomicAdd(f + 2, d);
                atomicAdd(f + 3, e);
            }
        }
    }
}

#ifndef NORI_SPLAT_POS_DEPTH
#define NORI_SPLAT_POS_DEPTH 4  // samples (20 bytes each) in flight per lane
#endif
#ifndef NORI_SPLAT_POS_SWEEP_FROM
#define NORI_SPLAT_POS_SWEEP_FROM 3  // the smallest border that takes two sweeps (k_splat_pos)
#endif

// The passes layout: k_splat<B, false> (kernels.hip) with the position and the
// value of pass k loaded from pos / val at k * stride + y * W + x instead of a
// sample record and the pcg32 jitter.  One work-group per 32x32 block and pass
// range, one lane per pixel: the lane sums its passes' (2B+1)^2 window in
// registers, adds it to the LDS tile once, and the tile goes to the film in
// one sweep of float atomics.  A kept sample whose window is not inside the
// lane's (a position exactly on the pixel's edge when radius + 0.5 is an
// integer) takes put_atomic instead.  The (2B+1)^2 x 4 window sums of B >= 3
// do not fit the register file beside the ring: those borders take two sweeps.
template <int B>
__global__ __launch_bounds__(kSplatBlock) void k_splat_pos(FilmGeom F, const int4 *blocks, uint32_t passes,
                                                            uint32_t passes_per_wg, uint64_t stride, const float *pos,
                                                            const float *val, float *film, float *var,
                                                            unsigned long long *dropped) {
    constexpr int NT = kSplatBlock, D = NORI_SPLAT_POS_DEPTH;
    constexpr int SW = B >= NORI_SPLAT_POS_SWEEP_FROM ? 2 : 1, NH = 2 / SW;  // sweeps over the passes; channel pairs per sweep
    constexpr int TS = NORI_BLOCK_SIZE + 2 * B, K = 2 * B + 1;
    __shared__ float tile[TS * TS * 4];
    __shared__ float ftab[NORI_FILTER_RESOLUTION + 1];
    const int4 bi = blocks[blockIdx.x];
    const int ox = bi.x, oy = bi.y, bw = bi.z & 0xFFFF, bh = bi.z >> 16;
    const uint32_t p0 = blockIdx.y * passes_per_wg, p1 = min(passes, p0 + passes_per_wg);
    for (int i = threadIdx.x; i < TS * TS * 4; i += NT) tile[i] = 0.0f;
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
        typedef float f2 __attribute__((ext_vector_type(2)));
        auto load = [&](uint32_t k) {
            const size_t i = (size_t)k * stride + pix;
            const float *p = pos + 2 * i, *v = val + 3 * i;
            return Smp{p[0], p[1], v[0], v[1], v[2]};
        };
        // SW == 2 (B >= 3): the RG windows over all passes, then the BW
        // windows -- half the window registers, the samples loaded twice
        for (int h = 0; h < SW; ++h) {
            f2 acc[K][K][NH];  // RG, BW (SW == 2: sweep h's pair) of every window cell
#pragma unroll
            for (int a = 0; a < K; ++a)
#pragma unroll
                for (int c = 0; c < K; ++c)
#pragma unroll
                    for (int e = 0; e < NH; ++e) acc[a][c][e] = f2{0.0f, 0.0f};
            bool any = false;
            float vs[7] = {0, 0, 0, 0, 0, 0, 0};
            auto put = [&](const Smp &s) {
                PutWindow w;
                if (!film_window(F, true, x, y, s.x, s.y, w) || !film_color_valid(s.r, s.g, s.b)) {
                    inval += h == 0 ? 1u : 0u;
                    return;
                }
                if (w.x0 < lx || w.x1 > lx + 2 * B || w.y0 < ly || w.y1 > ly + 2 * B) {
                    if (h == 0) put_atomic(F, ftab, film, var, w, s.r, s.g, s.b);
                    return;
                }
                any = true;
                vs[0] += s.r;
                vs[1] += s.g;
                vs[2] += s.b;
                vs[3] += s.r * s.r;
                vs[4] += s.g * s.g;
                vs[5] += s.b * s.b;
                vs[6] += 1.0f;
                float wx[K], wy[K];
#pragma unroll
                for (int d = 0; d < K; ++d) {
                    const int cx = lx + d, cy = ly + d;  // tile column / row of window cell d
                    const float fx = film_weight(ftab, lk, cx, w.px), fy = film_weight(ftab, lk, cy, w.py);
                    wx[d] = (cx >= w.x0 && cx <= w.x1) ? fx : 0.0f;
                    wy[d] = (cy >= w.y0 && cy <= w.y1) ? fy : 0.0f;
                }
                // Color4f(value) * wx, then * wy; (1 * wx) = wx exactly
                const f2 rg{s.r, s.g}, b1{s.b, 1.0f};
                f2 lp[NH][K];
#pragma unroll
                for (int c = 0; c < K; ++c)
#pragma unroll
                    for (int e = 0; e < NH; ++e) lp[e][c] = (SW == 2 ? (h ? b1 : rg) : (e ? b1 : rg)) * wx[c];
#pragma unroll
                for (int a = 0; a < K; ++a)
#pragma unroll
                    for (int c = 0; c < K; ++c)
#pragma unroll
                        for (int e = 0; e < NH; ++e) acc[a][c][e] += lp[e][c] * wy[a];
            };
            // the next D passes' samples are in flight while one is filtered (a
            // ring of D register sets, the pass loop unrolled by D: no moves)
            Smp q[D];
#pragma unroll
            for (int d = 0; d < D; ++d) q[d] = p0 + d < p1 ? load(p0 + d) : Smp{0, 0, 0, 0, 0};
            for (uint32_t p = p0; p < p1; p += D) {
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const Smp s = q[d];
                    if (p + D + d < p1) q[d] = load(p + D + d);
                    if (p + d < p1) put(s);
                }
            }
            if (any && var && h == 0) {
                float *v = var + 8 * pix;
                for (int k = 0; k < 7; ++k) atomicAdd(v + k, vs[k]);
            }
            if (any) {
#pragma unroll
                for (int a = 0; a < K; ++a)
#pragma unroll
                    for (int c = 0; c < K; ++c) {
                        float *t = tile + 4 * ((ly + a) * TS + (lx + c)) + (SW == 2 ? 2 * h : 0);
                        const f2 u = acc[a][c][0], v = acc[a][c][NH - 1];
                        if (SW == 2 ? (u.x != 0.0f || u.y != 0.0f) : (v.y != 0.0f || u.x != 0.0f || u.y != 0.0f || v.x != 0.0f)) {
                            atomicAdd(t + 0, u.x);
                            atomicAdd(t + 1, u.y);
                            if (SW == 1) {
                                atomicAdd(t + 2, v.x);
                                atomicAdd(t + 3, v.y);
                            }
                        }
                    }
            }
        }
    }
    if (inval) atomicAdd(dropped, (unsigned long long)inval);
    __syncthreads();
    const int rows = bh + 2 * B, cols = bw + 2 * B, FW = F.W + 2 * B;
    for (int i = threadIdx.x; i < rows * cols; i += NT) {
        const int yy = i / cols, xx = i - yy * cols;
        const float *c = tile + 4 * (yy * TS + xx);
        float *f = film + 4 * ((size_t)(oy + yy) * FW + (ox + xx));
        if (c[3] != 0.0f || c[0] != 0.0f || c[1] != 0.0f || c[2] != 0.0f) {
            atomicAdd(f + 0, c[0]);
            atomicAdd(f + 1, c[1]);
            atomicAdd(f + 2, c[2]);
            atomicAdd(f + 3, c[3]);
        }
    }
}

// Samples anywhere on the image.  Two forms of the same terms:
// ROWS = false: one lane per sample runs put_atomic -- 64 lanes add into 64
//   different film rows per instruction.
// ROWS = true: a wave loads 64 samples (one per lane: validity, owner block,
//   window, tile position), then walks the kept ones.  It broadcasts one sample
//   at a time and gives each lane one float of that sample's window (row,
//   column, channel), so that a wave-instruction adds whole contiguous window
//   rows of up to (2B+2) * 16 bytes.  A window of at most 32 floats (B = 0)
//   packs 64 / floats samples into one instruction.
// The statistics go to the owner pixel with atomics in both forms.
constexpr int kScatterBlock = 256;
template <int B, bool ROWS>
__global__ __launch_bounds__(kScatterBlock) void k_splat_scatter(FilmGeom F, uint64_t n, const float *pos,
                                                                  const float *val, float *film, float *var,
                                                                  unsigned long long *dropped) {
    __shared__ float ftab[NORI_FILTER_RESOLUTION + 1];
    if (threadIdx.x <= NORI_FILTER_RESOLUTION) ftab[threadIdx.x] = F.filter[threadIdx.x];
    __syncthreads();
    uint32_t inval = 0;
    const uint64_t step = (uint64_t)gridDim.x * kScatterBlock;
    if constexpr (!ROWS) {
        for (uint64_t i = (uint64_t)blockIdx.x * kScatterBlock + threadIdx.x; i < n; i += step) {
            const float sx = pos[2 * i], sy = pos[2 * i + 1], r = val[3 * i], g = val[3 * i + 1], b = val[3 * i + 2];
            PutWindow w;
            if (!film_window(F, false, 0, 0, sx, sy, w) || !film_color_valid(r, g, b)) {
                ++inval;
                continue;
            }
            put_atomic(F, ftab, film, var, w, r, g, b);
        }
    } else {
        // the widest window: floor(2 radius) + 1 <= 2B + 2 cells a side
        constexpr int KW = 2 * B + 2, RL = 4 * KW, NE = RL * KW;
        constexpr int SP = NE <= 32 ? 64 / NE : 1;  // samples per wave-instruction
        constexpr int IT = (NE + 63) / 64;           // wave-instructions per sample (SP == 1)
        const int lane = threadIdx.x & 63;
        const int FW = F.W + 2 * B;
        // (the loop bound is wave-uniform: every lane of a wave takes the same trips)
        for (uint64_t base = (uint64_t)blockIdx.x * kScatterBlock + (threadIdx.x & ~63u); base < n; base += step) {
            const uint64_t i = base + lane;
            PutWindow w{};
            float r = 0.0f, g = 0.0f, b = 0.0f;
            bool ok = false;
            if (i < n) {
                r = val[3 * i], g = val[3 * i + 1], b = val[3 * i + 2];
                ok = film_window(F, false, 0, 0, pos[2 * i], pos[2 * i + 1], w) && film_color_valid(r, g, b);
                if (!ok) ++inval;
            }
            if (ok && var) {
                float *v = var + 8 * ((size_t)w.y * F.W + w.x);
                atomicAdd(v + 0, r);
                atomicAdd(v + 1, g);
                atomicAdd(v + 2, b);
                atomicAdd(v + 3, r * r);
                atomicAdd(v + 4, g * g);
                atomicAdd(v + 5, b * b);
                atomicAdd(v + 6, 1.0f);
            }
            // per sample: the film cell of tile cell (0, 0), the window's first
            // cell and its extent, the tile position, the value
            const int cell0 = w.oy * FW + w.ox, nx = ok ? w.x1 - w.x0 + 1 : 0, ny = ok ? w.y1 - w.y0 + 1 : 0;
            auto term_add = [&](int c0, int x0, int y0, int mx, int my, float px, float py, float vr, float vg,
                                float vb, int e) {
                const int row = e / RL, col = (e - row * RL) >> 2, ch = e & 3;
                if (row >= my || col >= mx) return;
                const int cx = x0 + col, cy = y0 + row;
                const float wx = film_weight(ftab, F.lk, cx, px), wy = film_weight(ftab, F.lk, cy, py);
                const float v = ch == 0 ? vr : ch == 1 ? vg : ch == 2 ? vb : 1.0f;
                const float t = (v * wx) * wy;
                if (t != 0.0f) atomicAdd(film + 4 * ((size_t)c0 + (size_t)cy * FW + cx) + ch, t);
            };
            if constexpr (SP > 1) {
                const int sub = lane / NE, e = lane - sub * NE;
                for (int s0 = 0; s0 < 64; s0 += SP) {
                    const int src = s0 + sub;
                    const int mx = __shfl(nx, src), my = __shfl(ny, src);
                    const int c0 = __shfl(cell0, src), x0 = __shfl(w.x0, src), y0 = __shfl(w.y0, src);
                    const float px = __shfl(w.px, src), py = __shfl(w.py, src);
                    const float vr = __shfl(r, src), vg = __shfl(g, src), vb = __shfl(b, src);
                    term_add(c0, x0, y0, mx, my, px, py, vr, vg, vb, e);
                }
            } else {
                unsigned long long todo = __ballot(ok);
                while (todo) {
                    const int s = __ffsll((long long)todo) - 1;  // wave-uniform
                    todo &= todo - 1;
                    const int mx = __builtin_amdgcn_readlane(nx, s), my = __builtin_amdgcn_readlane(ny, s);
                    const int c0 = __builtin_amdgcn_readlane(cell0, s);
                    const int x0 = __builtin_amdgcn_readlane(w.x0, s), y0 = __builtin_amdgcn_readlane(w.y0, s);
                    const float px = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w.px), s));
                    const float py = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w.py), s));
                    const float vr = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(r), s));
                    const float vg = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(g), s));
                    const float vb = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(b), s));
#pragma unroll
                    for (int it = 0; it < IT; ++it) term_add(c0, x0, y0, mx, my, px, py, vr, vg, vb, it * 64 + lane);
                }
            }
        }
    }
    if (inval) atomicAdd(dropped, (unsigned long long)inval);
}

}  // namespace

hipError_t launch_splat_pos(const FilmGeom &F, const int4 *blocks, uint32_t nblocks, uint32_t passes,
                            uint32_t passes_per_wg, uint64_t stride, const float *pos, const float *val, float *film,
                            float *var, unsigned long long *dropped, hipStream_t st) {
    if (nblocks == 0 || passes == 0) return hipSuccess;
    if (passes_per_wg == 0) return hipErrorInvalidValue;
    const dim3 g(nblocks, (passes + passes_per_wg - 1) / passes_per_wg), b(kSplatBlock);
    if (g.y > 65535u) return hipErrorInvalidValue;
#define NORI_SPLAT_POS_CASE(b_)                                                                                    \
    case b_:                                                                                                       \
        hipLaunchKernelGGL((k_splat_pos<b_>), g, b, 0, st, F, blocks, passes, passes_per_wg, stride, pos, val, film, \
                           var, dropped);                                                                          \
        break;
    switch (F.B) {
    NORI_SPLAT_POS_CASE(0)
    NORI_SPLAT_POS_CASE(1)
    NORI_SPLAT_POS_CASE(2)
    NORI_SPLAT_POS_CASE(3)
    NORI_SPLAT_POS_CASE(4)
    default: return hipErrorInvalidValue;
    }
#undef NORI_SPLAT_POS_CASE
    return hipGetLastError();
}

hipError_t launch_splat_scatter(const FilmGeom &F, uint64_t n, bool rows, const float *pos, const float *val,
                                float *film, float *var, unsigned long long *dropped, hipStream_t st) {
    if (n == 0) return hipSuccess;
    // grid-stride: at most 2^16 work-groups, a wave's samples adjacent
    const dim3 g((unsigned)std::min<uint64_t>((n + kScatterBlock - 1) / kScatterBlock, 1u << 16)), b(kScatterBlock);
#define NORI_SPLAT_SCATTER_CASE(b_)                                                                               \
    case b_:                                                                                                      \
        if (rows) hipLaunchKernelGGL((k_splat_scatter<b_, true>), g, b, 0, st, F, n, pos, val, film, var, dropped); \
        else hipLaunchKernelGGL((k_splat_scatter<b_, false>), g, b, 0, st, F, n, pos, val, film, var, dropped);   \
        break;
    switch (F.B) {
    NORI_SPLAT_SCATTER_CASE(0)
    NORI_SPLAT_SCATTER_CASE(1)
    NORI_SPLAT_SCATTER_CASE(2)
    NORI_SPLAT_SCATTER_CASE(3)
    NORI_SPLAT_SCATTER_CASE(4)
    default: return hipErrorInvalidValue;
    }
#undef NORI_SPLAT_SCATTER_CASE
    return hipGetLastError();
}

}  // namespace nori
