// block_error.hip -- the adaptive sampler's per-block error metric on the device.
//
// The metric itself is stated once, at nori_film_block_error in
// include/nori_gpu.h (no reference counterpart; deviation D11).
// k_block_error evaluates it from the per-pixel sample statistics
// (render_desc.variance_out: sum L, sum L^2, n) where they were accumulated,
// so that between the rounds of nori_gpu_render_adaptive only one float per
// block crosses to the host.
//
// One work-group owns one 32x32 block, one 64-lane wave one of its sixteen
// 8x8 sub-tiles (lane = pixel): each lane loads its pixel's 8 floats as two
// float4 and forms e_p, a cross-lane sum gives the sub-tile's mean over its
// pixels inside the frame, and the maximum over the sub-tile means goes
// through LDS.  No global atomics.  S2 - S1^2/n is taken in fp64 (in fp32 it
// cancels to rounding noise on a bright, quiet pixel); the rest is fp32.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace nori {

namespace {

constexpr int kSub = 8;                                     // sub-tile edge: 64 pixels = one wave
constexpr int kSubPerRow = NORI_BLOCK_SIZE / kSub;          // 4
constexpr int kErrWaves = kSubPerRow * kSubPerRow;          // 16
constexpr int kErrBlock = 64 * kErrWaves;                   // 1024 threads
static_assert(kSub * kSub == 64, "one wave per sub-tile");

__device__ inline float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ids: the frame blocks to evaluate (null: block id = work-group index);
// err: one float per frame block, written at the block's id.
__global__ __launch_bounds__(kErrBlock) void k_block_error(const float4 *__restrict__ stats, int W, int H, int nbx,
                                                           const uint32_t *__restrict__ ids, float *__restrict__ err) {
    __shared__ float sub_mean[kErrWaves];
    const uint32_t id = ids ? ids[blockIdx.x] : blockIdx.x;
    const int ox = (int)(id % (uint32_t)nbx) * NORI_BLOCK_SIZE, oy = (int)(id / (uint32_t)nbx) * NORI_BLOCK_SIZE;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int x = ox + (wave % kSubPerRow) * kSub + (lane & (kSub - 1));
    const int y = oy + (wave / kSubPerRow) * kSub + (lane >> 3);
    const bool inside = x < W && y < H;
    float e = 0.0f;
    if (inside) {
        const size_t p = 2 * ((size_t)y * (size_t)W + (size_t)x);
        const float4 a = stats[p], b = stats[p + 1];  // S1 r g b, S2 r | S2 g b, n, 0
        const float n = b.z;
        if (n >= 2.0f) {
            const double dn = (double)n;
            const float dr = (float)fmax(0.0, (double)a.w - (double)a.x * (double)a.x / dn);
            const float dg = (float)fmax(0.0, (double)b.x - (double)a.y * (double)a.y / dn);
            const float db = (float)fmax(0.0, (double)b.y - (double)a.z * (double)a.z / dn);
            const float v = (dr + dg + db) / (n * (n - 1.0f));
            const float m = (a.x + a.y + a.z) / n;
            e = sqrtf(v) / sqrtf(m + 1e-3f);
        }
    }
    const float sum = wave_sum(e);
    const float cnt = wave_sum(inside ? 1.0f : 0.0f);
    // a sub-tile wholly outside the frame does not exist: 0 never wins the maximum over e >= 0
    if (lane == 0) sub_mean[wave] = cnt > 0.0f ? sum / cnt : 0.0f;
    __syncthreads();
    if (threadIdx.x == 0) {
        float m = sub_mean[0];
#pragma unroll
        for (int i = 1; i < kErrWaves; ++i) m = fmaxf(m, sub_mean[i]);
        err[id] = m;
    }
}

__global__ __launch_bounds__(256) void k_add_into(float *__restrict__ dst, const float *__restrict__ src, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] += src[i];
}

}  // namespace

hipError_t launch_block_error(const float *stats, int W, int H, int nbx, const uint32_t *ids, uint32_t nblocks,
                              float *err, hipStream_t st) {
    if (nblocks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_block_error, dim3(nblocks), dim3(kErrBlock), 0, st, reinterpret_cast<const float4 *>(stats), W,
                       H, nbx, ids, err);
    return hipGetLastError();
}

hipError_t launch_add_into(float *dst, const float *src, size_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_add_into, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dst, src, n);
    return hipGetLastError();
}

}  // namespace nori
