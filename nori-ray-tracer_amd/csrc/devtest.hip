// devtest.hip -- libnori_devtest.so: the device routines of device_math.h and
// shading.h behind plain C entry points, for the unit tests
// (tests/test_gpu_device_units.py, tests/devtest_util.py).  Not part of
// libnori_gpu.so.  Every kernel is element-wise: one thread per element,
// guarded by i < n, no shared state.  Every entry point takes host arrays,
// allocates, copies, launches, copies back and returns the HIP status.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bsdf_desc.h"
#include "kernels.h"
#include "shading.h"

using namespace nori;

namespace {

constexpr int kBlock = 256;

// Device copies of the host arrays of one call; freed on scope exit.
struct Buffers {
    static constexpr int kMax = 8;
    void *p[kMax] = {};
    int used = 0;
    hipError_t err = hipSuccess;
    // bytes == 0 or src == null with bytes: an uninitialised (output) buffer
    template <class T>
    T *in(const T *src, size_t count) {
        return reinterpret_cast<T *>(get(src, count * sizeof(T), true));
    }
    template <class T>
    T *out(size_t count) {
        return reinterpret_cast<T *>(get(nullptr, count * sizeof(T), false));
    }
    void *get(const void *src, size_t bytes, bool copy) {
        if (err != hipSuccess || used == kMax) {
            if (err == hipSuccess) err = hipErrorOutOfMemory;
            return nullptr;
        }
        void *d = nullptr;
        err = hipMalloc(&d, bytes ? bytes : 4);
        if (err != hipSuccess) return nullptr;
        p[used++] = d;
        if (copy && bytes) err = hipMemcpy(d, src, bytes, hipMemcpyHostToDevice);
        return d;
    }
    template <class T>
    hipError_t back(T *dst, const T *dev, size_t count) {
        if (err != hipSuccess) return err;
        err = hipGetLastError();  // the launch
        if (err == hipSuccess) err = hipDeviceSynchronize();
        if (err == hipSuccess && count) err = hipMemcpy(dst, dev, count * sizeof(T), hipMemcpyDeviceToHost);
        return err;
    }
    ~Buffers() {
        for (int i = 0; i < used; ++i) (void)hipFree(p[i]);
    }
};
inline unsigned grid(uint32_t n) { return n ? (n + kBlock - 1) / kBlock : 1; }

// ------------------------------------------------------------------ math
enum {
    kOpSqrtRn = 0,
    kOpRcpRn = 1,
    kOpRcpFull = 2,
    kOpFsqrtFast = 3,
    kOpFsqrtIeee = 4,
    kOpNormalizeFast = 5,
    kOpNormalizeIeee = 6,
    kOpFrameFast = 7,
    kOpFrameIeee = 8,
    kOpFresnelFast = 9,
    kOpFresnelIeee = 10,
    kOpTanTheta = 11,
    kOpCount = 12
};
// floats per element read / written by each op
__host__ __device__ constexpr int op_in(int op) { return op <= kOpFsqrtIeee || op == kOpFresnelFast || op == kOpFresnelIeee ? 1 : 3; }
__host__ __device__ constexpr int op_out(int op) {
    return op == kOpNormalizeFast || op == kOpNormalizeIeee ? 3 : (op == kOpFrameFast || op == kOpFrameIeee ? 9 : 1);
}

template <int OP>
__global__ void k_math(const float *in, uint32_t n, float ext, float intr, float eta_ei, float eta_ie, float *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if constexpr (op_in(OP) == 1) {
        const float x = in[i];
        float r;
        if constexpr (OP == kOpSqrtRn) r = sqrt_rn(x);
        else if constexpr (OP == kOpRcpRn) r = rcp_rn(x);
        else if constexpr (OP == kOpRcpFull) r = rcp_full(x);
        else if constexpr (OP == kOpFsqrtFast) r = fsqrt<true>(x);
        else if constexpr (OP == kOpFsqrtIeee) r = fsqrt<false>(x);
        else if constexpr (OP == kOpFresnelFast) r = fresnel<true>(x, ext, intr, eta_ei, eta_ie);
        else r = fresnel<false>(x, ext, intr, eta_ei, eta_ie);
        out[i] = r;
    } else {
        const V3 a = V3{in[3 * (size_t)i], in[3 * (size_t)i + 1], in[3 * (size_t)i + 2]};
        if constexpr (OP == kOpTanTheta) {
            out[i] = tan_theta(a);
        } else if constexpr (OP == kOpNormalizeFast || OP == kOpNormalizeIeee) {
            const V3 r = normalize<OP == kOpNormalizeFast>(a);
            float *o = out + 3 * (size_t)i;
            o[0] = r.x, o[1] = r.y, o[2] = r.z;
        } else {
            const Frame f = frame_from<OP == kOpFrameFast>(a);
            float *o = out + 9 * (size_t)i;
            o[0] = f.s.x, o[1] = f.s.y, o[2] = f.s.z;
            o[3] = f.t.x, o[4] = f.t.y, o[5] = f.t.z;
            o[6] = f.n.x, o[7] = f.n.y, o[8] = f.n.z;
        }
    }
}

template <int OP>
void launch_math(const float *in, uint32_t n, const DevBsdf &b, float *out) {
    hipLaunchKernelGGL(k_math<OP>, dim3(grid(n)), dim3(kBlock), 0, 0, in, n, b.ext_ior, b.int_ior, b.eta_ei, b.eta_ie,
                       out);
}

__global__ void k_pcg_skip3(const uint64_t *in, uint32_t n, uint64_t *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Pcg a, b;
    a.state = b.state = in[2 * (size_t)i];
    a.inc = b.inc = in[2 * (size_t)i + 1];
    pcg_skip3(a);
    pcg_skip(b, 1);
    pcg_skip(b, 1);
    pcg_skip(b, 1);
    out[2 * (size_t)i] = a.state;
    out[2 * (size_t)i + 1] = b.state;
}

// ------------------------------------------------------------------ BSDFs
template <bool FULL>
__global__ void k_bsdf_sample(DevBsdf b, const float *wi, const float *u, const float *uv, uint32_t n, float *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    BRec r;
    r.wi = V3{wi[3 * (size_t)i], wi[3 * (size_t)i + 1], wi[3 * (size_t)i + 2]};
    r.wo = V3{0, 0, 0};  // as the oracle's zeroed record: what an early return leaves behind
    r.measure = kMeasureUnknown;
    r.uv = uv ? V2{uv[2 * (size_t)i], uv[2 * (size_t)i + 1]} : V2{0, 0};
    const V3 w = bsdf_sample<FULL>(b, r, V2{u[2 * (size_t)i], u[2 * (size_t)i + 1]});
    float *o = out + 8 * (size_t)i;
    o[0] = r.wo.x, o[1] = r.wo.y, o[2] = r.wo.z;
    o[3] = w.x, o[4] = w.y, o[5] = w.z;
    o[6] = luminance(w);
    o[7] = (float)r.measure;
}

template <bool FULL>
__global__ void k_bsdf_eval_pdf(DevBsdf b, const float *wi, const float *wo, const float *uv, uint32_t n, float *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    BRec r;
    r.wi = V3{wi[3 * (size_t)i], wi[3 * (size_t)i + 1], wi[3 * (size_t)i + 2]};
    r.wo = V3{wo[3 * (size_t)i], wo[3 * (size_t)i + 1], wo[3 * (size_t)i + 2]};
    r.measure = kMeasureSolidAngle;
    r.uv = uv ? V2{uv[2 * (size_t)i], uv[2 * (size_t)i + 1]} : V2{0, 0};
    const V3 f = bsdf_eval<FULL>(b, r);
    float *o = out + 4 * (size_t)i;
    o[0] = f.x, o[1] = f.y, o[2] = f.z;
    o[3] = bsdf_pdf<FULL>(b, r);
}

// ------------------------------------------------------------------ glass chain
// Per lane kGlassWords 32-bit words: flags, t of the first chord, then the
// state (o, d, mint, maxt, beta, prev, rng state low / high, t: 15 words) of
// the input, of route A (glass_step) and of route B (glass_bounce, then
// chord_hit if it survived -- the fallback sequence of k_finish).
constexpr int kGlassState = 15, kGlassWords = 2 + 3 * kGlassState + 1;
enum { kGlassChord = 1, kGlassStepTaken = 2, kGlassBounceAlive = 4, kGlassBounceHit = 8 };

__device__ inline void put_state(uint32_t *w, const PathState &ps, float t) {
    const float f[12] = {ps.o.x, ps.o.y, ps.o.z, ps.d.x, ps.d.y, ps.d.z, ps.mint, ps.maxt, ps.beta.x, ps.beta.y, ps.beta.z,
                         ps.prev};
    for (int k = 0; k < 12; ++k) w[k] = __float_as_uint(f[k]);
    w[12] = (uint32_t)ps.rng.state;
    w[13] = (uint32_t)(ps.rng.state >> 32);
    w[14] = __float_as_uint(t);
}

template <int INTEG>
__global__ void k_glass(DevShape sh, DevBsdf B, uint64_t seed, const float *o, const float *d, const float *beta,
                        uint32_t n, uint32_t *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    PathState ps;
    ps.o = V3{o[3 * (size_t)i], o[3 * (size_t)i + 1], o[3 * (size_t)i + 2]};
    ps.d = V3{d[3 * (size_t)i], d[3 * (size_t)i + 1], d[3 * (size_t)i + 2]};
    ps.mint = kEps;
    ps.maxt = INF_F;
    ps.beta = V3{beta[3 * (size_t)i], beta[3 * (size_t)i + 1], beta[3 * (size_t)i + 2]};
    ps.prev = 0.5f;  // (a solid-angle pdf: path_mis must replace it by -1)
    wave_seed(ps.rng, seed, i);
    ps.work = i;
    ps.cam = false;
    ps.chan = 0;
    ps.invz = 0.0f;
    ps.L = V3{0, 0, 0};
    uint32_t *w = out + (size_t)kGlassWords * i;
    uint32_t flags = 0;
    float t = 0.0f;
    const bool chord = chord_hit<kGlassFast>(sh, ps, t);
    if (!chord) t = 0.0f;
    flags |= chord ? kGlassChord : 0;
    w[1] = __float_as_uint(t);
    put_state(w + 2, ps, t);
    PathState pa = ps, pb = ps;
    float ta = t, tb = t;
    if (chord) {
        if (glass_step<INTEG>(sh, B, pa, ta)) flags |= kGlassStepTaken;
        if (glass_bounce<INTEG>(sh, B, pb, tb)) {
            flags |= kGlassBounceAlive;
            float tc;
            if (chord_hit<kGlassFast>(sh, pb, tc)) {
                flags |= kGlassBounceHit;
                tb = tc;
            }
        }
    }
    put_state(w + 2 + kGlassState, pa, ta);
    put_state(w + 2 + 2 * kGlassState, pb, tb);
    w[2 + 3 * kGlassState] = 0;
    w[0] = flags;
}

}  // namespace

extern "C" {

// Floats per element that op reads and writes; 0 for an unknown op.
__attribute__((visibility("default"))) int nori_devtest_math_in(int op) { return op >= 0 && op < kOpCount ? op_in(op) : 0; }
__attribute__((visibility("default"))) int nori_devtest_math_out(int op) { return op >= 0 && op < kOpCount ? op_out(op) : 0; }

// out[i] = op(in[i]); fresnel reads cosThetaI and takes the IORs (and their
// quotients, derived as the scene upload derives them) from `iors` = {ext, int}.
__attribute__((visibility("default"))) int nori_devtest_math(int op, const float *in, uint32_t n, const float *iors,
                                                              float *out) {
    if (op < 0 || op >= kOpCount || !in || !out) return hipErrorInvalidValue;
    nori_bsdf_desc desc = {};
    desc.type = NORI_BSDF_DIELECTRIC;
    desc.ext_ior = iors ? iors[0] : 1.0f;
    desc.int_ior = iors ? iors[1] : 1.0f;
    DevBsdf b;
    dev_bsdf_from_desc(desc, b);
    Buffers buf;
    const float *din = buf.in(in, (size_t)n * op_in(op));
    float *dout = buf.out<float>((size_t)n * op_out(op));
    if (buf.err != hipSuccess) return buf.err;
    switch (op) {
#define NORI_OP(k) \
    case k: launch_math<k>(din, n, b, dout); break;
        NORI_OP(0) NORI_OP(1) NORI_OP(2) NORI_OP(3) NORI_OP(4) NORI_OP(5) NORI_OP(6) NORI_OP(7) NORI_OP(8) NORI_OP(9)
        NORI_OP(10) NORI_OP(11)
#undef NORI_OP
    }
    return buf.back(out, dout, (size_t)n * op_out(op));
}

// in: n x (state, inc); out: n x (state after pcg_skip3, state after three pcg_skip(r, 1))
__attribute__((visibility("default"))) int nori_devtest_pcg_skip3(const uint64_t *in, uint32_t n, uint64_t *out) {
    if (!in || !out) return hipErrorInvalidValue;
    Buffers buf;
    const uint64_t *din = buf.in(in, 2 * (size_t)n);
    uint64_t *dout = buf.out<uint64_t>(2 * (size_t)n);
    if (buf.err != hipSuccess) return buf.err;
    hipLaunchKernelGGL(k_pcg_skip3, dim3(grid(n)), dim3(kBlock), 0, 0, din, n, dout);
    return buf.back(out, dout, 2 * (size_t)n);
}

// out: n x 8 floats (wo, weight rgb, luminance(weight), measure).  uv may be
// null (0, 0).  full == 0: the basic plugin set (bsdf_sample<false>).
__attribute__((visibility("default"))) int nori_devtest_bsdf_sample(const nori_bsdf_desc *desc, int full,
                                                                     const float *wi, const float *u, const float *uv,
                                                                     uint32_t n, float *out) {
    if (!desc || !wi || !u || !out || desc->albedo_texture == NORI_TEXTURE_IMAGE) return hipErrorInvalidValue;
    DevBsdf b;
    dev_bsdf_from_desc(*desc, b);
    Buffers buf;
    const float *dwi = buf.in(wi, 3 * (size_t)n), *du = buf.in(u, 2 * (size_t)n);
    const float *duv = uv ? buf.in(uv, 2 * (size_t)n) : nullptr;
    float *dout = buf.out<float>(8 * (size_t)n);
    if (buf.err != hipSuccess) return buf.err;
    if (full) hipLaunchKernelGGL(k_bsdf_sample<true>, dim3(grid(n)), dim3(kBlock), 0, 0, b, dwi, du, duv, n, dout);
    else hipLaunchKernelGGL(k_bsdf_sample<false>, dim3(grid(n)), dim3(kBlock), 0, 0, b, dwi, du, duv, n, dout);
    return buf.back(out, dout, 8 * (size_t)n);
}

// out: n x 4 floats (bsdf_eval rgb, bsdf_pdf), solid-angle measure.
__attribute__((visibility("default"))) int nori_devtest_bsdf_eval_pdf(const nori_bsdf_desc *desc, int full,
                                                                       const float *wi, const float *wo,
                                                                       const float *uv, uint32_t n, float *out) {
    if (!desc || !wi || !wo || !out || desc->albedo_texture == NORI_TEXTURE_IMAGE) return hipErrorInvalidValue;
    DevBsdf b;
    dev_bsdf_from_desc(*desc, b);
    Buffers buf;
    const float *dwi = buf.in(wi, 3 * (size_t)n), *dwo = buf.in(wo, 3 * (size_t)n);
    const float *duv = uv ? buf.in(uv, 2 * (size_t)n) : nullptr;
    float *dout = buf.out<float>(4 * (size_t)n);
    if (buf.err != hipSuccess) return buf.err;
    if (full) hipLaunchKernelGGL(k_bsdf_eval_pdf<true>, dim3(grid(n)), dim3(kBlock), 0, 0, b, dwi, dwo, duv, n, dout);
    else hipLaunchKernelGGL(k_bsdf_eval_pdf<false>, dim3(grid(n)), dim3(kBlock), 0, 0, b, dwi, dwo, duv, n, dout);
    return buf.back(out, dout, 4 * (size_t)n);
}

__attribute__((visibility("default"))) int nori_devtest_glass_words(void) { return kGlassWords; }

// One chord bounce per lane on the sphere (center, radius) with the
// dielectric `desc`: o, d, beta are n x 3; lane i draws from
// wave_seed(seed, i).  out: n x nori_devtest_glass_words() words (k_glass).
// integrator: NORI_INTEGRATOR_PATH_MIS or NORI_INTEGRATOR_PATH_MATS.
__attribute__((visibility("default"))) int nori_devtest_glass(int integrator, const float *center, float radius,
                                                               const nori_bsdf_desc *desc, uint64_t seed,
                                                               const float *o, const float *d, const float *beta,
                                                               uint32_t n, uint32_t *out) {
    if (!center || !desc || !o || !d || !beta || !out || desc->type != NORI_BSDF_DIELECTRIC) return hipErrorInvalidValue;
    if (integrator != NORI_INTEGRATOR_PATH_MIS && integrator != NORI_INTEGRATOR_PATH_MATS) return hipErrorInvalidValue;
    DevBsdf b;
    dev_bsdf_from_desc(*desc, b);
    DevShape sh;
    std::memset(&sh, 0, sizeof(sh));
    sh.type = NORI_SHAPE_SPHERE;
    sh.emitter = -1;
    sh.prim_count = 1;
    sh.solitary = 1;
    for (int k = 0; k < 3; ++k) sh.center[k] = center[k];
    sh.radius = radius;
    Buffers buf;
    const float *dor = buf.in(o, 3 * (size_t)n), *dd = buf.in(d, 3 * (size_t)n), *db = buf.in(beta, 3 * (size_t)n);
    uint32_t *dout = buf.out<uint32_t>((size_t)kGlassWords * n);
    if (buf.err != hipSuccess) return buf.err;
    if (integrator == NORI_INTEGRATOR_PATH_MIS)
        hipLaunchKernelGGL(k_glass<NORI_INTEGRATOR_PATH_MIS>, dim3(grid(n)), dim3(kBlock), 0, 0, sh, b, seed, dor, dd, db,
                           n, dout);
    else
        hipLaunchKernelGGL(k_glass<NORI_INTEGRATOR_PATH_MATS>, dim3(grid(n)), dim3(kBlock), 0, 0, sh, b, seed, dor, dd,
                           db, n, dout);
    return buf.back(out, dout, (size_t)kGlassWords * n);
}

}  // extern "C"
