// devtest.hip -- libnori_devtest.so: device routines behind plain C entry
// points, for the unit tests (tests/devtest_util.py).  Not part of
// libnori_gpu.so.  Covered:
//  - device_math.h and shading.h (tests/test_gpu_device_units.py): the
//    correctly rounded and fast math forms, pcg_skip3, the BSDFs, the
//    glass-sphere chain;
//  - the tail finisher's pieces (tests/test_gpu_finish_tail.py): the body of
//    k_tail_prefix (coop_scan.h), the gid -> segment -> queue-slot lookup
//    (tail_index.h), coop_load / coop_scan (coop_scan.h);
//  - the scan's primitive tests (scan.h): tri_hit, tri_hit_nb,
//    tri_hit_plane<A>, sphere_hit, sphere_hit_nb, sphere_hit_fast, box_test.
// Every kernel but the first and third of the finisher group is element-wise:
// one thread per element, guarded by i < n, no shared state; those two run
// whole work-groups (the prefix) or whole waves (the cooperative scan) as the
// finisher does.  Every entry point takes host arrays, allocates, copies,
// launches, copies back and returns the HIP status.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bsdf_desc.h"
#include "coop_scan.h"
#include "kernels.h"
#include "shading.h"
#include "tail_index.h"

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

// ------------------------------------------------------------------ tail finisher
__global__ __launch_bounds__(1024) void k_dt_tail_prefix(const uint32_t *cnt, uint32_t G, uint32_t *pre) {
    tail_prefix(cnt, G, pre);
}

// The outputs are stored, never used as addresses.
__global__ void k_dt_tail_lookup(const uint32_t *pre, uint32_t G, const uint32_t *gids, uint32_t n, uint32_t *seg_out,
                                 uint32_t *slot_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t gid = gids[i], sg = tail_segment(pre, G, gid);
    seg_out[i] = sg;
    slot_out[i] = tail_slot(pre, sg, gid);
}

__device__ inline TRay load_ray(const float *rays, uint32_t i) {
    const float *p = rays + 8 * (size_t)i;
    return TRay{V3{p[0], p[1], p[2]}, V3{p[4], p[5], p[6]}, V3{0, 0, 0}, p[3], p[7]};
}

// Whole waves: the grid covers n rounded up to work-groups of kTraceBlock and
// no thread returns before the scan, so all 64 lanes of every wave reach
// coop_load and coop_scan converged (its precondition); the lanes past n do
// not want a ray.
template <bool ANY>
__global__ __launch_bounds__(kTraceBlock) void k_dt_coop_scan(DevScene S, const float *rays, const uint8_t *want, uint32_t n,
                                                              uint32_t *out) {
    const uint32_t i = blockIdx.x * kTraceBlock + threadIdx.x;
    const bool in = i < n;
    TRay r{V3{0, 0, 0}, V3{0, 0, 0}, V3{0, 0, 0}, 0.0f, 0.0f};
    bool w = false;
    if (in) {
        r = load_ray(rays, i);
        w = want[i] != 0;
    }
    const CoopPrim cp = coop_load(S);
    float t, u, v;
    uint32_t p;
    const bool res = coop_scan<ANY>(S, cp, r, w, t, p, u, v);
    if (in) {
        uint32_t *o = out + 5 * (size_t)i;
        o[0] = res ? 1u : 0u;
        o[1] = __float_as_uint(t);
        o[2] = p;
        o[3] = __float_as_uint(u);
        o[4] = __float_as_uint(v);
    }
}

// ------------------------------------------------------------------ primitive tests
enum {
    kFormTri = 0,
    kFormTriNb = 1,
    kFormTriPlane0 = 2,
    kFormTriPlane1 = 3,
    kFormTriPlane2 = 4,
    kFormSphere = 5,
    kFormSphereNb = 6,
    kFormSphereFast = 7,
    kFormSphereFastNocheck = 8,
    kFormBox = 9,
    kFormCount = 10
};

// Ray i against record i (three float4); mint and maxt as given.  out: 4
// words per element, (hit, t, u, v); for the box (record: min, max, unused)
// (ok, tnear, 0, 0) with the ray's rcp computed as the scan prologue does.
template <int FORM>
__global__ void k_dt_prim_hit(const float4 *rec, const float *rays, uint32_t n, uint32_t *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 a = rec[3 * (size_t)i], b = rec[3 * (size_t)i + 1], c = rec[3 * (size_t)i + 2];
    TRay r = load_ray(rays, i);
    float t = 0.0f, u = 0.0f, v = 0.0f;
    bool h;
    if constexpr (FORM == kFormTri) h = tri_hit(a, b, c, r, t, u, v);
    else if constexpr (FORM == kFormTriNb) h = tri_hit_nb(a, b, c, r, t, u, v);
    else if constexpr (FORM == kFormTriPlane0) h = tri_hit_plane<0>(a, b, c, r, t, u, v);
    else if constexpr (FORM == kFormTriPlane1) h = tri_hit_plane<1>(a, b, c, r, t, u, v);
    else if constexpr (FORM == kFormTriPlane2) h = tri_hit_plane<2>(a, b, c, r, t, u, v);
    else if constexpr (FORM == kFormSphere) h = sphere_hit(a, b, r, t);
    else if constexpr (FORM == kFormSphereNb) h = sphere_hit_nb<false>(a, b, r, t);
    else if constexpr (FORM == kFormSphereFast) h = sphere_hit_fast<false>(a, b, r, t);
    else if constexpr (FORM == kFormSphereFastNocheck) h = sphere_hit_fast<true>(a, b, r, t);
    else {
        r.rcp = V3{rcp_full(r.d.x), rcp_full(r.d.y), rcp_full(r.d.z)};
        h = box_test(a, b, r, t);
    }
    uint32_t *o = out + 4 * (size_t)i;
    o[0] = h ? 1u : 0u;
    o[1] = __float_as_uint(t);
    o[2] = __float_as_uint(u);
    o[3] = __float_as_uint(v);
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

// pre_out[0 .. G]: the exclusive prefix of cnt[0 .. G) and its total, by the
// body of k_tail_prefix launched as launch_tail_prefix does (1 x 1024).
__attribute__((visibility("default"))) int nori_devtest_tail_prefix(const uint32_t *cnt, uint32_t G, uint32_t *pre_out) {
    if (!cnt || !pre_out || G == 0) return hipErrorInvalidValue;
    Buffers buf;
    const uint32_t *dcnt = buf.in(cnt, (size_t)G);
    uint32_t *dpre = buf.out<uint32_t>((size_t)G + 1);
    if (buf.err != hipSuccess) return buf.err;
    hipLaunchKernelGGL(k_dt_tail_prefix, dim3(1), dim3(1024), 0, 0, dcnt, G, dpre);
    return buf.back(pre_out, dpre, (size_t)G + 1);
}

// seg_out[i] = tail_segment(pre, G, gids[i]), slot_out[i] = tail_slot of it; pre has G + 1 entries.
__attribute__((visibility("default"))) int nori_devtest_tail_lookup(const uint32_t *pre, uint32_t G, const uint32_t *gids,
                                                                     uint32_t n, uint32_t *seg_out, uint32_t *slot_out) {
    if (!pre || !gids || !seg_out || !slot_out || G == 0) return hipErrorInvalidValue;
    Buffers buf;
    const uint32_t *dpre = buf.in(pre, (size_t)G + 1), *dg = buf.in(gids, (size_t)n);
    uint32_t *dseg = buf.out<uint32_t>((size_t)n), *dslot = buf.out<uint32_t>((size_t)n);
    if (buf.err != hipSuccess) return buf.err;
    hipLaunchKernelGGL(k_dt_tail_lookup, dim3(grid(n)), dim3(kBlock), 0, 0, dpre, G, dg, n, dseg, dslot);
    const hipError_t e = buf.back(seg_out, dseg, (size_t)n);
    return e != hipSuccess ? e : buf.back(slot_out, dslot, (size_t)n);
}

// coop_load + coop_scan<any_hit> of n rays (8 floats: o, mint, d, maxt) over
// the np <= 64 records (3 float4 each), lanes with want[i] == 0 not tracing.
// out: n x 5 words (res, t, prim, u, v), of every lane.
__attribute__((visibility("default"))) int nori_devtest_coop_scan(const float *records, uint32_t np, const float *root_min,
                                                                   const float *root_max, const float *rays,
                                                                   const uint8_t *want, uint32_t n, int any_hit,
                                                                   uint32_t *out) {
    if (!records || !root_min || !root_max || !rays || !want || !out || np > 64) return hipErrorInvalidValue;
    Buffers buf;
    const float *drec = buf.in(records, 12 * (size_t)np), *dr = buf.in(rays, 8 * (size_t)n);
    const uint8_t *dw = buf.in(want, (size_t)n);
    uint32_t *dout = buf.out<uint32_t>(5 * (size_t)n);
    if (buf.err != hipSuccess) return buf.err;
    DevScene S;  // only what coop_load / coop_scan read
    std::memset(&S, 0, sizeof(S));
    S.prims = reinterpret_cast<const float4 *>(drec);
    S.num_prims = np;
    for (int k = 0; k < 3; ++k) S.root_min[k] = root_min[k], S.root_max[k] = root_max[k];
    const dim3 g(n ? (n + kTraceBlock - 1) / kTraceBlock : 1), b(kTraceBlock);
    if (any_hit) hipLaunchKernelGGL(k_dt_coop_scan<true>, g, b, 0, 0, S, dr, dw, n, dout);
    else hipLaunchKernelGGL(k_dt_coop_scan<false>, g, b, 0, 0, S, dr, dw, n, dout);
    return buf.back(out, dout, 5 * (size_t)n);
}

__attribute__((visibility("default"))) int nori_devtest_prim_forms(void) { return kFormCount; }

// Ray i (8 floats: o, mint, d, maxt) against record i (12 floats) with the
// test `form`; out: n x 4 words (k_dt_prim_hit).
__attribute__((visibility("default"))) int nori_devtest_prim_hit(int form, const float *records, const float *rays,
                                                                  uint32_t n, uint32_t *out) {
    if (form < 0 || form >= kFormCount || !records || !rays || !out) return hipErrorInvalidValue;
    Buffers buf;
    const float4 *drec = reinterpret_cast<const float4 *>(buf.in(records, 12 * (size_t)n));
    const float *dr = buf.in(rays, 8 * (size_t)n);
    uint32_t *dout = buf.out<uint32_t>(4 * (size_t)n);
    if (buf.err != hipSuccess) return buf.err;
    switch (form) {
#define NORI_FORM(k) \
    case k: hipLaunchKernelGGL(k_dt_prim_hit<k>, dim3(grid(n)), dim3(kBlock), 0, 0, drec, dr, n, dout); break;
        NORI_FORM(0) NORI_FORM(1) NORI_FORM(2) NORI_FORM(3) NORI_FORM(4) NORI_FORM(5) NORI_FORM(6) NORI_FORM(7)
        NORI_FORM(8) NORI_FORM(9)
#undef NORI_FORM
    }
    return buf.back(out, dout, 4 * (size_t)n);
}

}  // extern "C"
