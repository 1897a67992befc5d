// kernels_query.hip -- the ray queries: k_surface (full hit records) and
// k_camera_rays (the renderer's own primary rays), with their launchers.
// nori_gpu_query / nori_gpu_camera_rays (stated at nori_scene_surface and
// nori_gpu_camera_rays in nori_gpu.h).
#include <cstdlib>

#include "kernels.h"
#include "shading.h"

namespace nori {

// The hit record of setHitInformation as four float4: (p, t), (ng, prim),
// (ns, shape), (uv, bary).  surface() with two differences: the geometric
// normal is always computed and so is the sphere's uv (surface() skips both
// where no BSDF reads them); the operations it shares keep surface()'s order.
struct SurfRec {
    float4 a, b, c, d;
};
ND SurfRec surface_record(const DevScene &S, float4 hit, float4 ro, float4 rd) {
    const uint32_t prim = __float_as_uint(hit.y);
    SurfRec r;
    if (prim >= S.num_prims) {  // miss (prim = -1)
        r.a = make_float4(0.0f, 0.0f, 0.0f, INF_F);
        r.b = r.c = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xFFFFFFFFu));
        r.d = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return r;
    }
    const float t = hit.x, u = hit.z, v = hit.w;
    const uint32_t shape = S.prim_shape[prim];
    const DevShape &sh = S.shapes[shape];
    V3 p, ng, ns;
    V2 uv{u, v};
    if (sh.type == NORI_SHAPE_SPHERE) {
        p = ld3(ro) + ld3(rd) * t;
        ng = ns = normalize(p - V3{sh.center[0], sh.center[1], sh.center[2]});
        // sphericalCoordinates (common.cpp:264-272); 0.5 is a double literal
        float phi = atan2f(ng.y, ng.x);
        if (phi < 0) phi += 2 * kPi;
        uv.x = (float)(0.5 + (double)(acosf(ng.z) / (2 * kPi)));
        uv.y = phi / kPi;
    } else {
        const uint32_t *f = S.tri_vidx + 3 * (size_t)prim;
        const uint32_t i0 = f[0], i1 = f[1], i2 = f[2];
        const float4 q0 = S.pos[i0], q1 = S.pos[i1], q2 = S.pos[i2];
        const V3 p0 = ld3(q0), p1 = ld3(q1), p2 = ld3(q2);
        const float bx = 1 - (u + v);
        p = (p0 * bx + p1 * u) + p2 * v;
        ng = normalize(cross(p1 - p0, p2 - p0));
        ns = ng;
        if (sh.has_uvs || sh.has_normals) {
            const float4 n0 = S.nrm[i0], n1 = S.nrm[i1], n2 = S.nrm[i2];
            if (sh.has_uvs)  // u in pos.w, v in nrm.w
                uv = V2{(bx * q0.w + u * q1.w) + v * q2.w, (bx * n0.w + u * n1.w) + v * n2.w};
            if (sh.has_normals) {
                ns = normalize((ld3(n0) * bx + ld3(n1) * u) + ld3(n2) * v);
                if (sh.nmap) {  // NormalMap::eval (normalmap.cpp:95-134): 2 * byte / 255 - 1, normalized
                    const V3 c = texel_rgb(texel_at(sh.nmap, sh.nm_w, sh.nm_h, sh.nm_wrap, uv));
                    const V3 m = V3{2.0f * c.x - 1.0f, 2.0f * c.y - 1.0f, 2.0f * c.z - 1.0f};
                    ns = to_world(frame_from(ns), normalize(m));
                }
            }
        }
    }
    r.a = make_float4(p.x, p.y, p.z, t);
    r.b = make_float4(ng.x, ng.y, ng.z, hit.y);
    r.c = make_float4(ns.x, ns.y, ns.z, __uint_as_float(shape));
    r.d = make_float4(uv.x, uv.y, u, v);
    return r;
}

// One thread per ray: 16-byte hit + 32-byte ray in, 64-byte record out.
// The records are an array of structures.  LDS = false: each lane stores its
// own four float4 (four store instructions, each 64 lanes x 16 bytes at a
// 64-byte stride).  LDS = true: the work-group's 128 records pass through LDS
// (rows padded to five float4, so the lanes' 16-byte writes spread over the
// banks) and each of a wave's four store instructions writes one contiguous
// 1 KiB.
constexpr int kSurfRow = 5;  // float4 per record row in LDS (4 + 1 padding)
template <bool LDS>
__global__ __launch_bounds__(kTraceBlock) void k_surface(DevScene S, const float4 *rays, const float4 *hits, uint32_t n,
                                                         float4 *out) {
    const uint32_t q = blockIdx.x * kTraceBlock + threadIdx.x;
    if constexpr (!LDS) {
        if (q >= n) return;
        const SurfRec r = surface_record(S, hits[q], rays[2 * (size_t)q], rays[2 * (size_t)q + 1]);
        float4 *o = out + 4 * (size_t)q;
        o[0] = r.a, o[1] = r.b, o[2] = r.c, o[3] = r.d;
    } else {
        __shared__ float4 rows[kTraceBlock * kSurfRow];
        if (q < n) {
            const SurfRec r = surface_record(S, hits[q], rays[2 * (size_t)q], rays[2 * (size_t)q + 1]);
            float4 *w = rows + threadIdx.x * kSurfRow;
            w[0] = r.a, w[1] = r.b, w[2] = r.c, w[3] = r.d;
        }
        __syncthreads();
        // the block's float4 j * 128 + lane of its 512: record (.. / 4), part (.. % 4)
        const uint32_t base = blockIdx.x * kTraceBlock;  // first record of the block
        const uint32_t left = n - base < (uint32_t)kTraceBlock ? n - base : (uint32_t)kTraceBlock;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t i = j * kTraceBlock + threadIdx.x;
            if (i < 4 * left) out[4 * (size_t)base + i] = rows[(i >> 2) * kSurfRow + (i & 3)];
        }
    }
}

// The LDS transpose is the default: 1.35 - 1.6 x faster than the per-lane
// stores at 1M and 4M rays (DESIGN_LOG.md).  NORI_SURFACE_STORE=direct|lds
// overrides it (read at every launch, so that one process can alternate the two).
static bool surface_lds() {
    const char *e = std::getenv("NORI_SURFACE_STORE");
    return e ? e[0] != 'd' : true;
}
hipError_t launch_surface(const DevScene &S, const float4 *rays, const float4 *hits, uint32_t n, float4 *out,
                          hipStream_t st) {
    if (n == 0) return hipSuccess;
    const dim3 g((n + kTraceBlock - 1) / kTraceBlock), b(kTraceBlock);
    if (surface_lds()) hipLaunchKernelGGL(k_surface<true>, g, b, 0, st, S, rays, hits, n, out);
    else hipLaunchKernelGGL(k_surface<false>, g, b, 0, st, S, rays, hits, n, out);
    return hipGetLastError();
}

// Camera::sampleRay of the renderer's own samples: one thread per (pass k0 + k,
// entry of `pixels`), k < np; the sample's stream, jitter and aperture sample
// are k_features' (and k_direct's, k_shade's), the ray goes to
// rays[2 * ((k0 + k) * W * H + pix)].
__global__ __launch_bounds__(kTraceBlock) void k_camera_rays(DevScene S, const uint32_t *pixels, uint32_t M,
                                                             uint32_t pass_begin, uint32_t k0, uint32_t np,
                                                             uint64_t seed, float4 *rays) {
    const uint32_t e = blockIdx.x * kTraceBlock + threadIdx.x;
    if (e >= np * M) return;
    const uint32_t k = k0 + e / M, pix = pixels[e % M];
    const uint32_t y = pix / (uint32_t)S.W, x = pix - y * (uint32_t)S.W;
    const uint64_t wh = (uint64_t)S.W * (uint64_t)S.H;
    const int ch = (S.chromatic[0] != 0.0f || S.chromatic[1] != 0.0f || S.chromatic[2] != 0.0f) ? 1 : -1;
    Pcg rng;
    wave_seed(rng, seed, (uint64_t)(pass_begin + k) * wh + pix);
    const V2 jit = next2D(rng);
    const V2 ap = next2D(rng);  // apertureSample (render.cpp:99)
    V3 o, d;
    float mn, mx;
    camera_sample(S, (float)x + jit.x, (float)y + jit.y, ap, ch, o, d, mn, mx);
    float4 *r = rays + 2 * ((size_t)k * wh + pix);
    r[0] = make_float4(o.x, o.y, o.z, mn);
    r[1] = make_float4(d.x, d.y, d.z, mx);
}
hipError_t launch_camera_rays(const DevScene &S, const uint32_t *pixels, uint32_t M, uint32_t pass_begin, uint32_t k0,
                              uint32_t np, uint64_t seed, float *rays, hipStream_t st) {
    if (M == 0 || np == 0) return hipSuccess;
    if ((uint64_t)np * M > 0x7FFFFFFFull) return hipErrorInvalidValue;  // (the runtime launches in chunks of passes)
    const dim3 g((np * M + kTraceBlock - 1) / kTraceBlock), b(kTraceBlock);
    hipLaunchKernelGGL(k_camera_rays, g, b, 0, st, S, pixels, M, pass_begin, k0, np, seed,
                       reinterpret_cast<float4 *>(rays));
    return hipGetLastError();
}

}  // namespace nori
