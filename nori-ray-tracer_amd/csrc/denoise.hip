// denoise.hip -- the NL-means denoiser (denoiser/denoiser.py) as one kernel,
// k_nlmeans, and the feature-guided variant k_guided (no reference
// counterpart; described at the kernel below).
//
// The reference script runs, for each of the (2r+1)^2 neighbour offsets s,
// whole-image numpy passes (denoiser.py:55-66):
//   ngb      = roll(img, s)                 (periodic shift, :41-44)
//   d2pixel  = (sum_c (ngb - img)^2 - v1) / (eps + k^2 v2)     (:32-37)
//   d2patch  = box(d2pixel)                 (convolve2d 'same', zero fill)
//   wgt      = box(exp(-max(0, d2patch)))
//   out     += wgt * ngb,  wsum += wgt;     out /= wsum at the end.
// Here one work-group owns a kDnTX x kDnTY output tile: it stages the image
// and variance around the tile (halo r + 2p, periodic like np.roll) in LDS
// once, then for every offset computes d2pixel on the tile +- 2p, the first
// box on the tile +- p and the second box on the tile, accumulating the
// weighted neighbours in registers -- the 49 full-image passes of the
// script become one read of the image and one write.
//
// Variances (denoiser.py:32-37): the script's d2() names its third
// parameter img_variance but is called with the shifted variance, and reads
// the global ngb_variance for the other term, so both v1 and v2 come out as
// 2 * var(ngb) (mode 0, what the script computes).  Mode 1 is the textbook
// form the script spells out (v1 = var_p + min(var_p, var_q),
// v2 = var_p + var_q).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "kernels.h"

namespace nori {

namespace {

constexpr int kDnTX = 32, kDnTY = 16;  // output tile (256 threads, 2 pixels each)
constexpr float kDnEps = 1e-3f;        // denoiser.py:23

__device__ inline int wrap(int v, int n) {
    v %= n;
    return v < 0 ? v + n : v;
}

__global__ __launch_bounds__(256) void k_nlmeans(const float *__restrict__ img, const float *__restrict__ var, int W,
                                                 int H, int R, int P, float k, int mode, float *__restrict__ out) {
    extern __shared__ float lds[];
    const int halo = R + 2 * P;
    const int AW = kDnTX + 2 * halo, AH = kDnTY + 2 * halo;  // staged image/variance region
    const int DW = kDnTX + 4 * P, DH = kDnTY + 4 * P;        // d2pixel region (tile +- 2p)
    const int GW = kDnTX + 2 * P, GH = kDnTY + 2 * P;        // weight region (tile +- p)
    float *A = lds;                   // AW x AH x 4 (r, g, b, variance)
    float *D = A + 4 * AW * AH;       // DW x DH
    float *G = D + DW * DH;           // GW x GH
    float *Hs = G + GW * GH;          // DH x GW: row sums of D (first box, separable)
    float *Hg = D;                    // GH x kDnTX: row sums of G (second box; D is free by then)
    const int x0 = blockIdx.x * kDnTX, y0 = blockIdx.y * kDnTY, tid = threadIdx.x;
    for (int i = tid; i < AW * AH; i += 256) {
        const int ay = i / AW, ax = i - ay * AW;
        const int gy = wrap(y0 - halo + ay, H), gx = wrap(x0 - halo + ax, W);
        const size_t g = (size_t)gy * W + gx;
        A[4 * i + 0] = img[3 * g + 0];
        A[4 * i + 1] = img[3 * g + 1];
        A[4 * i + 2] = img[3 * g + 2];
        A[4 * i + 3] = var[g];
    }
    __syncthreads();
    const float inv_box = 1.0f / (float)((2 * P + 1) * (2 * P + 1));
    const float k2 = k * k;
    float acc[2][3] = {{0, 0, 0}, {0, 0, 0}}, wsum[2] = {0, 0};
    for (int sr = -R; sr <= R; ++sr)      // axis 0 (rows): np.roll(data, dx, 0)
        for (int sc = -R; sc <= R; ++sc) {  // axis 1 (columns)
            // d2pixel on the tile +- 2p; zero outside the image (convolve2d fill)
            for (int i = tid; i < DW * DH; i += 256) {
                const int dy = i / DW, dx = i - dy * DW;
                const int y = y0 - 2 * P + dy, x = x0 - 2 * P + dx;
                float d2 = 0.0f;
                if (y >= 0 && y < H && x >= 0 && x < W) {
                    const int ay = dy - 2 * P + halo, ax = dx - 2 * P + halo;
                    const float *p = A + 4 * (ay * AW + ax);
                    const float *q = A + 4 * ((ay - sr) * AW + (ax - sc));  // ngb = img[y - sr, x - sc]
                    const float e0 = q[0] - p[0], e1 = q[1] - p[1], e2 = q[2] - p[2];
                    const float sq = (e0 * e0 + e1 * e1) + e2 * e2;
                    const float nv = q[3];
                    float v1, v2;
                    if (mode == 0) {
                        v1 = nv + nv;
                        v2 = nv + nv;
                    } else {
                        v1 = p[3] + fminf(p[3], nv);
                        v2 = p[3] + nv;
                    }
                    d2 = (sq - v1) / (kDnEps + k2 * v2);
                }
                D[i] = d2;
            }
            __syncthreads();
            // box means as row sums then column sums (separable, zero outside the image)
            for (int i = tid; i < DH * GW; i += 256) {
                const int y = i / GW, x = i - y * GW;
                float r = 0.0f;
                for (int l = 0; l <= 2 * P; ++l) r += D[y * DW + x + l];
                Hs[i] = r;
            }
            __syncthreads();
            // wgt = exp(-max(0, box(d2pixel))) on the tile +- p
            for (int i = tid; i < GW * GH; i += 256) {
                const int gy = i / GW, gx = i - gy * GW;
                const int y = y0 - P + gy, x = x0 - P + gx;
                float w = 0.0f;
                if (y >= 0 && y < H && x >= 0 && x < W) {
                    float c = 0.0f;
                    for (int j = 0; j <= 2 * P; ++j) c += Hs[(gy + j) * GW + gx];
                    w = expf(-fmaxf(0.0f, c * inv_box));
                }
                G[i] = w;
            }
            __syncthreads();
            for (int i = tid; i < GH * kDnTX; i += 256) {
                const int y = i / kDnTX, x = i - y * kDnTX;
                float r = 0.0f;
                for (int l = 0; l <= 2 * P; ++l) r += G[y * GW + x + l];
                Hg[i] = r;
            }
            __syncthreads();
            for (int h = 0; h < 2; ++h) {
                const int t = tid + 256 * h, ty = t / kDnTX, tx = t - ty * kDnTX;
                float c = 0.0f;
                for (int j = 0; j <= 2 * P; ++j) c += Hg[(ty + j) * kDnTX + tx];
                const float w = c * inv_box;
                const float *q = A + 4 * ((ty + halo - sr) * AW + (tx + halo - sc));
                acc[h][0] += w * q[0];
                acc[h][1] += w * q[1];
                acc[h][2] += w * q[2];
                wsum[h] += w;
            }
            __syncthreads();
        }
    for (int h = 0; h < 2; ++h) {
        const int t = tid + 256 * h, ty = t / kDnTX, tx = t - ty * kDnTX;
        const int y = y0 + ty, x = x0 + tx;
        if (y < H && x < W) {
            const size_t g = (size_t)y * W + x;
            out[3 * g + 0] = acc[h][0] / wsum[h];
            out[3 * g + 1] = acc[h][1] / wsum[h];
            out[3 * g + 2] = acc[h][2] / wsum[h];
        }
    }
}

// Patch offsets o in [-F, F] with both p + o and p + s + o inside [0, n): the
// in-frame count of the guided filter's patch mean along one axis.
__device__ inline int pair_count(int p, int s, int n, int F) {
    const int lo = max(-F, max(-p, -p - s)), hi = min(F, min(n - 1 - p, n - 1 - p - s));
    return hi - lo + 1;
}

// The feature-guided denoiser (stated at nori_film_denoise_guided in
// nori_gpu.h; film_io.cpp computes it in double precision).  Same tiling as
// k_nlmeans: a work-group owns a kDnTX x kDnTY tile, 256 threads, two pixels
// each.  Staged once: colour + variance (one float4 per pixel) on the tile
// +- (R + F) and the 7 features (two float4) on the tile +- R -- the feature
// term reads p and q = p + s only, so its region needs no patch border.  Per
// neighbour offset s: the per-pixel colour term on the tile +- F (0 where
// p + o or q + o is outside the frame), its row sums, then per pixel the
// column sum divided by the in-frame count (pair_count per axis), the feature
// term from the staged features and the weighted neighbour into registers.
__global__ __launch_bounds__(256) void k_guided(const float *__restrict__ img, const float *__restrict__ var,
                                                const float *__restrict__ feat, int W, int H, int R, int F, float k2,
                                                float eps, float inv_sa2, float inv_sn2, float inv_sz2,
                                                float *__restrict__ out) {
    extern __shared__ float4 lds4[];
    const int halo = R + F;
    const int AW = kDnTX + 2 * halo, AH = kDnTY + 2 * halo;  // colour + variance region
    const int FW = kDnTX + 2 * R, FH = kDnTY + 2 * R;        // feature region
    const int DW = kDnTX + 2 * F, DH = kDnTY + 2 * F;        // colour-term region (tile +- F)
    float4 *A = lds4;                                         // AW x AH
    float4 *Fe = A + AW * AH;                                 // FW x FH x 2: (a.rgb, n.x), (n.yz, z, 0)
    float *D = reinterpret_cast<float *>(Fe + 2 * FW * FH);   // DW x DH
    float *Hs = D + DW * DH;                                  // DH x kDnTX: row sums of D
    const int x0 = blockIdx.x * kDnTX, y0 = blockIdx.y * kDnTY, tid = threadIdx.x;
    for (int i = tid; i < AW * AH; i += 256) {
        const int ay = i / AW, ax = i - ay * AW;
        const int gy = y0 - halo + ay, gx = x0 - halo + ax;
        float4 v = make_float4(0, 0, 0, 0);  // outside the frame: never read by an in-frame pair
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const size_t g = (size_t)gy * W + gx;
            v = make_float4(img[3 * g + 0], img[3 * g + 1], img[3 * g + 2], var[g]);
        }
        A[i] = v;
    }
    for (int i = tid; i < FW * FH; i += 256) {
        const int fy = i / FW, fx = i - fy * FW;
        const int gy = y0 - R + fy, gx = x0 - R + fx;
        float4 a = make_float4(0, 0, 0, 0), b = a;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const float *f = feat + 7 * ((size_t)gy * W + gx);
            a = make_float4(f[0], f[1], f[2], f[3]);
            b = make_float4(f[4], f[5], f[6], 0.0f);
        }
        Fe[2 * i] = a;
        Fe[2 * i + 1] = b;
    }
    __syncthreads();
    float acc[2][3] = {{0, 0, 0}, {0, 0, 0}}, wsum[2] = {0, 0};
    for (int sr = -R; sr <= R; ++sr)
        for (int sc = -R; sc <= R; ++sc) {
            for (int i = tid; i < DW * DH; i += 256) {
                const int dy = i / DW, dx = i - dy * DW;
                const int y = y0 - F + dy, x = x0 - F + dx;
                float d2 = 0.0f;
                if (y >= 0 && y < H && x >= 0 && x < W && y + sr >= 0 && y + sr < H && x + sc >= 0 && x + sc < W) {
                    const float4 p = A[(dy + R) * AW + (dx + R)];
                    const float4 q = A[(dy + R + sr) * AW + (dx + R + sc)];
                    const float e0 = p.x - q.x, e1 = p.y - q.y, e2 = p.z - q.z;
                    const float sq = (e0 * e0 + e1 * e1) + e2 * e2;
                    d2 = (sq - (p.w + fminf(p.w, q.w))) / (eps + k2 * (p.w + q.w));
                }
                D[i] = d2;
            }
            __syncthreads();
            for (int i = tid; i < DH * kDnTX; i += 256) {
                const int y = i / kDnTX, x = i - y * kDnTX;
                float r = 0.0f;
                for (int l = 0; l <= 2 * F; ++l) r += D[y * DW + x + l];
                Hs[i] = r;
            }
            __syncthreads();
            // (the next offset's D writes follow every thread's Hs reads of this one: its
            // Hs writes come after the barrier that follows them)
            for (int h = 0; h < 2; ++h) {
                const int t = tid + 256 * h, ty = t / kDnTX, tx = t - ty * kDnTX;
                const int y = y0 + ty, x = x0 + tx;
                if (y >= H || x >= W || y + sr < 0 || y + sr >= H || x + sc < 0 || x + sc >= W) continue;
                float c = 0.0f;
                for (int j = 0; j <= 2 * F; ++j) c += Hs[(ty + j) * kDnTX + tx];
                const float d2c = c / (float)(pair_count(y, sr, H, F) * pair_count(x, sc, W, F));
                const float4 *fp = Fe + 2 * ((ty + R) * FW + (tx + R));
                const float4 *fq = Fe + 2 * ((ty + R + sr) * FW + (tx + R + sc));
                const float4 p0 = fp[0], p1 = fp[1], q0 = fq[0], q1 = fq[1];
                float d2f = 0.0f;
                if (inv_sa2 > 0.0f) {
                    const float a0 = p0.x - q0.x, a1 = p0.y - q0.y, a2 = p0.z - q0.z;
                    d2f += ((a0 * a0 + a1 * a1) + a2 * a2) * inv_sa2;
                }
                if (inv_sn2 > 0.0f) {
                    const float n0 = p0.w - q0.w, n1 = p1.x - q1.x, n2 = p1.y - q1.y;
                    d2f += ((n0 * n0 + n1 * n1) + n2 * n2) * inv_sn2;
                }
                if (inv_sz2 > 0.0f) {
                    const float rel = (p1.z - q1.z) / fmaxf(fmaxf(p1.z, q1.z), 1e-6f);
                    d2f += (rel * rel) * inv_sz2;
                }
                const float w = expf(-(fmaxf(0.0f, d2c) + d2f));
                const float4 q = A[(ty + halo + sr) * AW + (tx + halo + sc)];
                acc[h][0] += w * q.x;
                acc[h][1] += w * q.y;
                acc[h][2] += w * q.z;
                wsum[h] += w;
            }
        }
    for (int h = 0; h < 2; ++h) {
        const int t = tid + 256 * h, ty = t / kDnTX, tx = t - ty * kDnTX;
        const int y = y0 + ty, x = x0 + tx;
        if (y < H && x < W) {
            const size_t g = (size_t)y * W + x;
            out[3 * g + 0] = acc[h][0] / wsum[h];
            out[3 * g + 1] = acc[h][1] / wsum[h];
            out[3 * g + 2] = acc[h][2] / wsum[h];
        }
    }
}

}  // namespace

size_t guided_lds_bytes(int R, int F) {
    const int halo = R + F;
    return sizeof(float) * ((size_t)4 * (kDnTX + 2 * halo) * (kDnTY + 2 * halo) +
                            (size_t)8 * (kDnTX + 2 * R) * (kDnTY + 2 * R) +
                            (size_t)(kDnTX + 2 * F) * (kDnTY + 2 * F) + (size_t)(kDnTY + 2 * F) * kDnTX);
}

hipError_t launch_guided(const float *img, const float *var, const float *feat, int W, int H, int R, int F, float k,
                         float eps, float sigma_a, float sigma_n, float sigma_z, float *out, hipStream_t st) {
    const size_t lds = guided_lds_bytes(R, F);
    // more than the default 64 KiB of dynamic LDS needs the opt-in
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_guided),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    // 1 / sigma^2; 0 (sigma = +inf) switches the term off.  Taken in double and
    // clamped to the largest float: the fp32 square of a sigma below 1e-19
    // underflows to 0, and 0 (an equal feature) x inf would be NaN
    auto inv2 = [](float s) { return (float)fmin(1.0 / ((double)s * (double)s), (double)FLT_MAX); };
    const dim3 g((W + kDnTX - 1) / kDnTX, (H + kDnTY - 1) / kDnTY), b(256);
    hipLaunchKernelGGL(k_guided, g, b, lds, st, img, var, feat, W, H, R, F, k * k, eps, inv2(sigma_a), inv2(sigma_n),
                       inv2(sigma_z), out);
    return hipGetLastError();
}

size_t denoise_lds_bytes(int R, int P) {
    const int halo = R + 2 * P;
    return sizeof(float) * ((size_t)4 * (kDnTX + 2 * halo) * (kDnTY + 2 * halo) +
                            (size_t)(kDnTX + 4 * P) * (kDnTY + 4 * P) + (size_t)(kDnTX + 2 * P) * (kDnTY + 2 * P) +
                            (size_t)(kDnTY + 4 * P) * (kDnTX + 2 * P));
}

hipError_t launch_denoise(const float *img, const float *var, int W, int H, int R, int P, float k, int mode,
                          float *out, hipStream_t st) {
    const dim3 g((W + kDnTX - 1) / kDnTX, (H + kDnTY - 1) / kDnTY), b(256);
    hipLaunchKernelGGL(k_nlmeans, g, b, denoise_lds_bytes(R, P), st, img, var, W, H, R, P, k, mode, out);
    return hipGetLastError();
}

}  // namespace nori
