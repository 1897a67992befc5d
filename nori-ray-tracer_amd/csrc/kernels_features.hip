// kernels_features.hip -- k_features and launch_features: the first-hit
// feature buffers of the guided denoiser.
#include "onebounce.h"

namespace nori {

// nori_gpu_render_features (no reference counterpart): the albedo, shading
// normal and hit distance at the first hit of every camera sample, summed per
// pixel for the guided denoiser.  One thread per selected pixel loops over the
// passes: sample (pass, pixel) draws its jitter and aperture sample from the
// stream k_direct / k_shade give that sample, so its ray is the render's
// primary ray; with chromatic aberration the green channel's ray.  The
// thread reads the pixel's eight sums, adds the samples in pass order and
// writes them back with two 16-byte stores: no atomics, so the buffer is
// bitwise reproducible and independent of how a pass range is split.
template <int STACK>
__global__ __launch_bounds__(kTraceBlock) void k_features(DevScene S, const uint32_t *pixels, uint32_t M,
                                                          uint32_t pass_begin, uint32_t np, uint64_t seed,
                                                          float4 *feat) {
    __shared__ uint32_t stk[stack_words(STACK) * kTraceBlock];
    const uint32_t e = blockIdx.x * kTraceBlock + threadIdx.x;
    if (e >= M) return;
    OneBounce<STACK> ob{S, stk + threadIdx.x};
    const uint32_t pix = pixels[e];
    const uint32_t y = pix / (uint32_t)S.W, x = pix - y * (uint32_t)S.W;
    float4 f0 = feat[2 * (size_t)pix], f1 = feat[2 * (size_t)pix + 1];
    const int ch = (S.chromatic[0] != 0.0f || S.chromatic[1] != 0.0f || S.chromatic[2] != 0.0f) ? 1 : -1;
    for (uint32_t k = 0; k < np; ++k) {
        Pcg rng;
        wave_seed(rng, seed, (uint64_t)(pass_begin + k) * ((uint64_t)S.W * (uint64_t)S.H) + pix);
        const V2 jit = next2D(rng);
        const V2 ap = next2D(rng);  // apertureSample (render.cpp:99)
        V3 o, d;
        float mn, mx, t;
        camera_sample(S, (float)x + jit.x, (float)y + jit.y, ap, ch, o, d, mn, mx);
        SurfHit hs;
        if (ob.closest(o, d, mn, mx, hs, t)) {
            const DevBsdf &B = S.bsdfs[S.shapes[hs.shape].bsdf];
            V3 a{1, 1, 1};  // mirror, dielectric
            if (B.type == NORI_BSDF_DIFFUSE) a = albedo_at(B, hs.uv);
            else if (B.type == NORI_BSDF_MICROFACET) a = V3{B.kd[0], B.kd[1], B.kd[2]};
            else if (B.type == NORI_BSDF_DISNEY) a = V3{B.base[0], B.base[1], B.base[2]};
            f0.x += a.x, f0.y += a.y, f0.z += a.z;
            f0.w += hs.sh.n.x, f1.x += hs.sh.n.y, f1.y += hs.sh.n.z;
            f1.z += t;
        }
        f1.w += 1.0f;
    }
    feat[2 * (size_t)pix] = f0;
    feat[2 * (size_t)pix + 1] = f1;
}

hipError_t launch_features(const DevScene &S, const uint32_t *pixels, uint32_t M, uint32_t pass_begin, uint32_t np,
                           uint64_t seed, float *feat, int stack, hipStream_t st) {
    if (M == 0 || np == 0) return hipSuccess;
    const dim3 g((M + kTraceBlock - 1) / kTraceBlock), b(kTraceBlock);
    float4 *f = reinterpret_cast<float4 *>(feat);
    with_stack<0, 32>(stack, [&](auto N) {
        hipLaunchKernelGGL(k_features<N()>, g, b, 0, st, S, pixels, M, pass_begin, np, seed, f);
    });
    return hipGetLastError();
}

}  // namespace nori
