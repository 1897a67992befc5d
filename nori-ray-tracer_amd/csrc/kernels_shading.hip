// kernels_shading.hip -- the shading queries: the BSDF and emitter routines of
// device_math.h / shading.h over caller-supplied hit records, one thread per
// element, and the renderer's own random numbers (k_sample_uniforms), with
// their launchers.  nori_gpu_bsdf_eval / _bsdf_sample / _emitter_sample /
// _emitter_eval / _sample_uniforms (stated at those names in nori_gpu.h).
// Nothing is traced, so the kernels serve a context of any integrator and
// traversal mode; FULL = true routines only (every plugin).
//
// The shading frame of a record is frame_from(ns), which is the render's own
// frame bit for bit (surface() in shading.h against surface_record() in
// kernels_query.hip):
//   sphere                  surface(): frame_from(n), n = normalize(p - c); the record's ns is that n
//   mesh without normals    surface(): frame_from(normalize(cross(p1 - p0, p2 - p0))); ns = ng = that vector
//   mesh with normals       surface(): frame_from(normalize(interpolated)); ns = that vector
//   ... and a normal map    surface(): frame_from(to_world(frame_from(n), normalize(m))); ns is the
//                           argument, to_world(frame_from(n), normalize(m)), not renormalised in either
// In every case surface() passes to frame_from the very value the record
// stores in ns, and frame_from is a pure function of it.
//
// Bounds.  Everything in the arrays is the caller's, so no value read from
// them may index memory unchecked:
//   shape index, emitter id   compared against the scene's counts; outside: zeros
//   uv                        texel_at() converts uv * size to int, which is undefined for NaN, inf
//                             and |x| >= 2^31; for an image-textured BSDF sane_uv() first replaces a
//                             coordinate that is NaN or beyond +-2^30 / max(W, H) by 0 (every uv the
//                             conversion is defined for passes unchanged), so the wrap / clamp of
//                             texel_at keeps the texel inside the image.  The checkerboard takes
//                             only x % 2 of its conversion and indexes nothing.
//   light samples u           sample_surface's lower_bound and clamp hold for any x (NaN ends at
//                             triangle 0); env_sample's row = (int)u can leave the table when the
//                             sample equals the last marginal CDF entry or is outside [0, 1):
//                             env_sample<CLAMP = true> (shading.h) clamps the row, and is the
//                             renderers' env_sample<false> otherwise
//   directions, points        arithmetic only
#include <cstdlib>

#include "kernels.h"
#include "shading.h"

namespace nori {

ND V2 sane_uv(const DevBsdf &B, float u, float v) {
    if (B.tex != NORI_TEXTURE_IMAGE) return V2{u, v};
    const float lim = 0x1p30f / (float)max(max(B.img_w, B.img_h), 1);
    return V2{fabsf(u) <= lim ? u : 0.0f, fabsf(v) <= lim ? v : 0.0f};
}
ND V3 ld3p(const float *a, uint32_t q) { return V3{a[3 * (size_t)q], a[3 * (size_t)q + 1], a[3 * (size_t)q + 2]}; }
ND V2 ld2p(const float *a, uint32_t q) { return V2{a[2 * (size_t)q], a[2 * (size_t)q + 1]}; }

// The element's 64-byte record: an array of structures, as k_surface writes
// it.  LDS = false: each lane loads the float4 parts it needs (NEED bit j =
// part j) at a 64-byte stride.  LDS = true: the work-group's 128 records pass
// through LDS -- each of a wave's four load instructions reads one contiguous
// 1 KiB, rows padded to five float4 as in k_surface -- and every lane then
// reads its own row.  Every thread of the block must call it (barrier).
constexpr int kRecRow = 5;
template <bool LDS, int NEED>
ND void load_record(const float4 *surf, uint32_t n, float4 (&r)[4]) {
    const uint32_t q = blockIdx.x * kTraceBlock + threadIdx.x;
    if constexpr (!LDS) {
        if (q < n) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (NEED & (1 << j)) r[j] = surf[4 * (size_t)q + j];
        }
    } else {
        __shared__ float4 rows[kTraceBlock * kRecRow];
        const uint32_t base = blockIdx.x * kTraceBlock;  // first record of the block (< n: the grid is ceil(n / 128))
        const uint32_t left = n - base < (uint32_t)kTraceBlock ? n - base : (uint32_t)kTraceBlock;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t i = j * kTraceBlock + threadIdx.x;
            if (i < 4 * left) rows[(i >> 2) * kRecRow + (i & 3)] = surf[4 * (size_t)base + i];
        }
        __syncthreads();
        if (q < n) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (NEED & (1 << j)) r[j] = rows[threadIdx.x * kRecRow + j];
        }
    }
}

// out: (bsdf_eval rgb, bsdf_pdf), (wo_local.z, wi_local.z, 0, 0)
template <bool LDS>
__global__ __launch_bounds__(kTraceBlock) void k_bsdf_eval(DevScene S, uint32_t num_shapes, const float4 *surf,
                                                           const float *wi, const float *wo, uint32_t n, float4 *out) {
    const uint32_t q = blockIdx.x * kTraceBlock + threadIdx.x;
    float4 r[4];
    load_record<LDS, 0xC>(surf, n, r);
    if (q >= n) return;
    float4 o0 = make_float4(0, 0, 0, 0), o1 = o0;
    const uint32_t shape = __float_as_uint(r[2].w);
    if (shape < num_shapes) {
        const DevBsdf &B = S.bsdfs[S.shapes[shape].bsdf];
        const Frame f = frame_from(ld3(r[2]));
        BRec br;
        br.wi = to_local(f, ld3p(wi, q));
        br.wo = to_local(f, ld3p(wo, q));
        br.measure = kMeasureSolidAngle;
        br.uv = sane_uv(B, r[3].x, r[3].y);
        const V3 e = bsdf_eval(B, br);
        o0 = make_float4(e.x, e.y, e.z, bsdf_pdf(B, br));
        o1 = make_float4(br.wo.z, br.wi.z, 0.0f, 0.0f);
    }
    out[2 * (size_t)q] = o0;
    out[2 * (size_t)q + 1] = o1;
}

// out: (to_world(br.wo), bsdf_pdf of the sampled record), (weight rgb, measure); zeros for a zero weight
template <bool LDS>
__global__ __launch_bounds__(kTraceBlock) void k_bsdf_sample(DevScene S, uint32_t num_shapes, const float4 *surf,
                                                             const float *wi, const float *u, uint32_t n, float4 *out) {
    const uint32_t q = blockIdx.x * kTraceBlock + threadIdx.x;
    float4 r[4];
    load_record<LDS, 0xC>(surf, n, r);
    if (q >= n) return;
    float4 o0 = make_float4(0, 0, 0, 0), o1 = o0;
    const uint32_t shape = __float_as_uint(r[2].w);
    if (shape < num_shapes) {
        const DevBsdf &B = S.bsdfs[S.shapes[shape].bsdf];
        const Frame f = frame_from(ld3(r[2]));
        BRec br;
        br.wi = to_local(f, ld3p(wi, q));
        br.wo = V3{0, 0, 1};
        br.measure = kMeasureUnknown;
        br.uv = sane_uv(B, r[3].x, r[3].y);
        const V3 w = bsdf_sample(B, br, ld2p(u, q));
        if (!is_zero(w)) {  // deviation D1: a zero weight leaves no direction
            const V3 d = to_world(f, br.wo);
            o0 = make_float4(d.x, d.y, d.z, bsdf_pdf(B, br));
            o1 = make_float4(w.x, w.y, w.z, (float)br.measure);
        }
    }
    out[2 * (size_t)q] = o0;
    out[2 * (size_t)q + 1] = o1;
}

// emitter_sample_one; out: (wi, maxt), (Li, pdf_em), (p, 0)
__global__ __launch_bounds__(kTraceBlock) void k_emitter_sample(DevScene S, const int32_t *ids, int32_t emitter,
                                                                const float *x, const float *u, uint32_t n,
                                                                float4 *out) {
    const uint32_t q = blockIdx.x * kTraceBlock + threadIdx.x;
    if (q >= n) return;
    float4 o0 = make_float4(0, 0, 0, 0), o1 = o0, o2 = o0;
    const uint32_t id = (uint32_t)(ids ? ids[q] : emitter);
    if (id < S.num_emitters) {
        const DevEmitter &E = S.emitters[id];
        const V3 ref = ld3p(x, q);
        const V2 s2 = ld2p(u, q);
        const NeeSample r = emitter_sample_one<true, true>(S, E, ref, s2);  // (CLAMP: env_sample's row)
        o0 = make_float4(r.wi.x, r.wi.y, r.wi.z, r.maxt);
        o1 = make_float4(r.Li.x, r.Li.y, r.Li.z, r.pdf_em);
        o2 = make_float4(r.p.x, r.p.y, r.p.z, 0.0f);
    }
    out[3 * (size_t)q] = o0;
    out[3 * (size_t)q + 1] = o1;
    out[3 * (size_t)q + 2] = o2;
}

// emission() of onebounce.h and the emitter pdf of direct_mis at the record; out: (Le, pdf)
template <bool LDS>
__global__ __launch_bounds__(kTraceBlock) void k_emitter_eval(DevScene S, uint32_t num_shapes, const float4 *surf,
                                                              const float *from, uint32_t n, float4 *out) {
    const uint32_t q = blockIdx.x * kTraceBlock + threadIdx.x;
    float4 r[4];
    load_record<LDS, 0x5>(surf, n, r);
    if (q >= n) return;
    float4 o = make_float4(0, 0, 0, 0);
    const uint32_t shape = __float_as_uint(r[2].w);
    if (shape < num_shapes) {
        const int32_t em = S.shapes[shape].emitter;
        if (em >= 0) {
            const DevEmitter &E = S.emitters[em];
            const V3 ns = ld3(r[2]), wi = normalize(ld3(r[0]) - ld3p(from, q));
            const V3 Le = emitter_eval(S, E, ns, wi);
            o = make_float4(Le.x, Le.y, Le.z, emitter_pdf(S, E, ns, wi));
        }
    }
    out[q] = o;
}

// NORI_SHADING_LOAD=direct|lds overrides the default record read (read at
// every launch, so that one process can alternate the two): DESIGN_LOG.md.
static bool record_lds() {
    const char *e = std::getenv("NORI_SHADING_LOAD");
    return e ? e[0] == 'l' : false;
}
static dim3 grid_for(uint32_t n) { return dim3((n + kTraceBlock - 1) / kTraceBlock); }

hipError_t launch_bsdf_eval(const DevScene &S, uint32_t num_shapes, const float4 *surf, const float *wi,
                            const float *wo, uint32_t n, float4 *out, hipStream_t st) {
    if (n == 0) return hipSuccess;
    const dim3 b(kTraceBlock);
    if (record_lds()) hipLaunchKernelGGL(k_bsdf_eval<true>, grid_for(n), b, 0, st, S, num_shapes, surf, wi, wo, n, out);
    else hipLaunchKernelGGL(k_bsdf_eval<false>, grid_for(n), b, 0, st, S, num_shapes, surf, wi, wo, n, out);
    return hipGetLastError();
}
hipError_t launch_bsdf_sample(const DevScene &S, uint32_t num_shapes, const float4 *surf, const float *wi,
                              const float *u, uint32_t n, float4 *out, hipStream_t st) {
    if (n == 0) return hipSuccess;
    const dim3 b(kTraceBlock);
    if (record_lds()) hipLaunchKernelGGL(k_bsdf_sample<true>, grid_for(n), b, 0, st, S, num_shapes, surf, wi, u, n, out);
    else hipLaunchKernelGGL(k_bsdf_sample<false>, grid_for(n), b, 0, st, S, num_shapes, surf, wi, u, n, out);
    return hipGetLastError();
}
hipError_t launch_emitter_sample(const DevScene &S, const int32_t *ids, int32_t emitter, const float *x, const float *u,
                                 uint32_t n, float4 *out, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_emitter_sample, grid_for(n), dim3(kTraceBlock), 0, st, S, ids, emitter, x, u, n, out);
    return hipGetLastError();
}
hipError_t launch_emitter_eval(const DevScene &S, uint32_t num_shapes, const float4 *surf, const float *from,
                               uint32_t n, float4 *out, hipStream_t st) {
    if (n == 0) return hipSuccess;
    const dim3 b(kTraceBlock);
    if (record_lds()) hipLaunchKernelGGL(k_emitter_eval<true>, grid_for(n), b, 0, st, S, num_shapes, surf, from, n, out);
    else hipLaunchKernelGGL(k_emitter_eval<false>, grid_for(n), b, 0, st, S, num_shapes, surf, from, n, out);
    return hipGetLastError();
}

// pcg32's advance (ext/pcg32/pcg32.h advance(): O(log delta) squarings of the
// LCG step), so that a large `first` costs no loop of that length.
ND void pcg_advance(Pcg &r, uint64_t delta) {
    uint64_t cur_mult = kPcgMult, cur_plus = r.inc, acc_mult = 1u, acc_plus = 0u;
    while (delta > 0) {
        if (delta & 1) {
            acc_mult *= cur_mult;
            acc_plus = acc_plus * cur_mult + cur_plus;
        }
        cur_plus = (cur_mult + 1) * cur_plus;
        cur_mult *= cur_mult;
        delta >>= 1;
    }
    r.state = acc_mult * r.state + acc_plus;
}

// Draws [first, first + count) of next1D on the stream of sample (pass
// pass_begin + k, pixel pix), k in [k0, k0 + np), for the M entries of
// `pixels`, at out[count * (k * W * H + pix) + j]; one thread per sample.
__global__ __launch_bounds__(kTraceBlock) void k_sample_uniforms(DevScene S, const uint32_t *pixels, uint32_t M,
                                                                 uint32_t pass_begin, uint32_t k0, uint32_t np,
                                                                 uint64_t seed, uint32_t first, uint32_t count,
                                                                 float *out) {
    const uint32_t e = blockIdx.x * kTraceBlock + threadIdx.x;
    if (e >= np * M) return;
    const uint32_t k = k0 + e / M, pix = pixels[e % M];
    const uint64_t wh = (uint64_t)S.W * (uint64_t)S.H;
    Pcg rng;
    wave_seed(rng, seed, (uint64_t)(pass_begin + k) * wh + pix);
    pcg_advance(rng, first);
    float *o = out + (size_t)count * ((size_t)k * wh + pix);
    for (uint32_t j = 0; j < count; ++j) o[j] = next1D(rng);
}
hipError_t launch_sample_uniforms(const DevScene &S, const uint32_t *pixels, uint32_t M, uint32_t pass_begin,
                                  uint32_t k0, uint32_t np, uint64_t seed, uint32_t first, uint32_t count, float *out,
                                  hipStream_t st) {
    if (M == 0 || np == 0 || count == 0) return hipSuccess;
    if ((uint64_t)np * M > 0x7FFFFFFFull) return hipErrorInvalidValue;  // (the runtime launches in chunks of passes)
    hipLaunchKernelGGL(k_sample_uniforms, grid_for(np * M), dim3(kTraceBlock), 0, st, S, pixels, M, pass_begin, k0, np,
                       seed, first, count, out);
    return hipGetLastError();
}

}  // namespace nori
