// shading.h -- the path vertex, shared by the kernels that shade: hit
// information (surface), emitters, environment map and next-event estimation,
// the camera, the path state and its queue encoding, the medium,
// shade_vertex / shade_vertex_vol, the glass-sphere chord code and the
// per-sample film splat of the finisher.  Device code for the .hip units.
#pragma once
#include "kernel_config.h"
#include "scan.h"

#if defined(__HIPCC_RTC__) && !defined(M_PI)  // (hipRTC has no <math.h>: glibc's value)
#define M_PI 3.14159265358979323846
#endif

namespace nori {

// ------------------------------------------------------------------ shading helpers
struct SurfHit {
    V3 p;
    Frame sh;
    int shape;
    V2 uv;
};

// setHitInformation: mesh.cpp:122-170, sphere.cpp:78-93 (shading frame and
// texture coordinates; a mesh without UVs keeps the barycentrics in its.uv).
template <bool FULL = true>
ND SurfHit surface(const DevScene &S, uint32_t prim, float t, float u, float v, V3 o, V3 d) {
    SurfHit h;
    h.shape = (int)S.prim_shape[prim];
    const DevShape &sh = S.shapes[h.shape];
    // only a textured albedo reads the texture coordinates (BRec.uv): the
    // sphere's atan2/acos are skipped for every other BSDF
    const bool need_uv = FULL && (S.bsdfs[sh.bsdf].tex != NORI_TEXTURE_CONSTANT || sh.nmap);
    h.uv = V2{u, v};
    if (sh.type == NORI_SHAPE_SPHERE) {
        h.p = o + d * t;
        const V3 n = normalize(h.p - V3{sh.center[0], sh.center[1], sh.center[2]});
        h.sh = frame_from(n);
        if (need_uv) {
            // sphericalCoordinates (common.cpp:264-272); 0.5 is a double literal
            float phi = atan2f(n.y, n.x);
            if (phi < 0) phi += 2 * kPi;
            h.uv.x = (float)(0.5 + (double)(acosf(n.z) / (2 * kPi)));
            h.uv.y = phi / kPi;
        }
    } else {
        const uint32_t *f = S.tri_vidx + 3 * (size_t)prim;
        uint32_t i0 = f[0], i1 = f[1], i2 = f[2];
        const float4 q0 = S.pos[i0], q1 = S.pos[i1], q2 = S.pos[i2];
        V3 p0 = ld3(q0), p1 = ld3(q1), p2 = ld3(q2);
        float bx = 1 - (u + v);
        h.p = (p0 * bx + p1 * u) + p2 * v;
        if (need_uv && sh.has_uvs)  // u in pos.w, v in nrm.w
            h.uv = V2{(bx * q0.w + u * q1.w) + v * q2.w,
                      (bx * S.nrm[i0].w + u * S.nrm[i1].w) + v * S.nrm[i2].w};
        if (sh.has_normals) {
            V3 n = (ld3(S.nrm[i0]) * bx + ld3(S.nrm[i1]) * u) + ld3(S.nrm[i2]) * v;
            h.sh = frame_from(normalize(n));
            if (FULL && sh.nmap) {  // NormalMap::eval (normalmap.cpp:95-134): 2 * byte / 255 - 1, normalized
                const V3 t = texel_rgb(texel_at(sh.nmap, sh.nm_w, sh.nm_h, sh.nm_wrap, h.uv));
                const V3 m = V3{2.0f * t.x - 1.0f, 2.0f * t.y - 1.0f, 2.0f * t.z - 1.0f};
                h.sh = frame_from(to_world(h.sh, normalize(m)));
            }
        } else {
            h.sh = frame_from(normalize(cross(p1 - p0, p2 - p0)));
        }
    }
    return h;
}

// EnvironmentMap (envmap.cpp), restated as the oracle's env_* functions.
constexpr float kEnvTFar = 100000.0f;  // envmap.cpp:9
// sphericalCoordinates (common.cpp:264-272) + mapIntersect (envmap.cpp:61-75)
ND V2 env_map(const DevEmitter &e, V3 vec) {
    float theta = acosf(vec.z), phi = atan2f(vec.y, vec.x);
    if (phi < 0) phi = (float)((double)phi + 2 * M_PI);
    V2 uv;
    uv.x = theta * (float)(e.R - 1) * kInvPi;
    uv.y = (float)((double)phi * 0.5 * (double)(e.C - 1) * (double)kInvPi);
    if (isnan(uv.x) || isnan(uv.y)) uv = V2{0, 0};
    return uv;
}
ND int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
ND V3 env_texel(const DevScene &S, const DevEmitter &e, int i, int j) {
    const float *c = S.env + e.rgb_off + 3 * ((size_t)i * e.C + j);
    return V3{c[0], c[1], c[2]};
}
// EnvironmentMap::eval (envmap.cpp:124-156): bilinear, wrapping at the edges
ND V3 env_eval(const DevScene &S, const DevEmitter &e, V3 wi) {
    const V2 uv = env_map(e, normalize(wi));
    const int u = clampi((int)uv.x, 0, e.R - 1), v = clampi((int)uv.y, 0, e.C - 1);
    const int us = (u + 1) % e.R, vs = (v + 1) % e.C;
    const V3 BL = env_texel(S, e, u, v), UL = env_texel(S, e, u, vs), BR = env_texel(S, e, us, v),
             UR = env_texel(S, e, us, vs);
    const int dusu = us - u, dvsv = vs - v;
    const float dusum = (float)us - uv.x, dumu = uv.x - (float)u, dvmv = uv.y - (float)v, dvsvm = (float)vs - uv.y;
    const V3 acc = ((((BL * dusum) * dvsvm) + ((BR * dumu) * dvsvm)) + ((UL * dusum) * dvmv)) + ((UR * dumu) * dvmv);
    const float inv = (float)(1.0 / (double)(dusu * dvsv));
    const V3 r = V3{inv * acc.x, inv * acc.y, inv * acc.z};
    return V3{e.weight * r.x, e.weight * r.y, e.weight * r.z};
}
// EnvironmentMap::pdf (envmap.cpp:184-192)
ND float env_pdf(const DevScene &S, const DevEmitter &e, V3 wi) {
    const V2 uv = env_map(e, normalize(wi));
    const int i = clampi((int)uv.x, 0, e.R - 1), j = clampi((int)uv.y, 0, e.C - 1);
    return S.env[e.pmarg_off + i] * S.env[e.pdf_off + (size_t)i * e.C + j];
}
// sample1D (envmap.cpp:112-122): the reference scans for the first i with
// P[i] <= s < P[i+1] (the oracle keeps that scan).  P[0..cols-1] is
// nondecreasing (P[0] = 0 plus non-negative pf terms; only the final
// P[cols] = 1 of the literal precompute1D can drop below P[cols-1]), so the
// first such i below cols-1 is upper_bound(P[0..cols-1], s) - 1, and every
// other case -- s >= P[cols-1], or no interval at all (all-zero rows, NaN s)
// -- ends at cols-1 in the scan too.  Binary search: O(log cols) loads
// instead of up to cols dependent pairs per environment sample.
ND void env_sample1D(const float *pf, const float *P, int cols, float s, float &x, float &prob) {
    int lo = 0, hi = cols;  // first j in [0, cols) with P[j] > s, or cols
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (P[mid] <= s) lo = mid + 1;
        else hi = mid;
    }
    const int i = (lo == 0 || lo >= cols) ? cols - 1 : lo - 1;
    const float t = (P[i + 1] - s) / (P[i + 1] - P[i]);
    x = (1 - t) * (float)i + t * (float)(i + 1);
    prob = pf[i];
}
// EnvironmentMap::sample (envmap.cpp:158-181); deviation D4: the Jacobian
// uses the sampled direction (the reference reads lRec.wi uninitialised).
// CLAMP (the shading queries, whose samples are the caller's): the sampled
// row is kept inside the tables for any smp -- row = (int)u for every u in
// [0, R - 1], so nothing else changes; the renderers instantiate CLAMP = false.
template <bool CLAMP = false>
ND V3 env_sample(const DevScene &S, const DevEmitter &e, V2 smp, V3 &wi) {
    float u, v, u_pdf, v_pdf;
    env_sample1D(S.env + e.pmarg_off, S.env + e.cmarg_off, e.R, smp.x, u, u_pdf);
    const int row = CLAMP ? (int)(u >= 0.0f ? smin(u, (float)(e.R - 1)) : 0.0f) : (int)u;  // (CLAMP: NaN -> row 0)
    env_sample1D(S.env + e.pdf_off + (size_t)row * e.C, S.env + e.cdf_off + (size_t)row * (e.C + 1), e.C, smp.y, v,
                 v_pdf);
    const float theta = (float)((double)u * M_PI / (double)(e.R - 1));  // invMapIntersect
    const float phi = (float)((double)(v * 2.0f) * M_PI / (double)(e.C - 1));
    wi = normalize(V3{sinf(theta) * cosf(phi), sinf(theta) * sinf(phi), cosf(theta)});
    const float st2 = 1.0f - wi.z * wi.z, st = st2 <= 0.0f ? 0.0f : sqrtf(st2);  // Frame::sinTheta
    const float jac = (float)((double)((e.C - 1) * (e.R - 1)) / (2 * (M_PI * M_PI) * (double)st));
    v_pdf = env_pdf(S, e, wi) * jac;
    const V3 c = env_eval(S, e, wi);
    return V3{c.x / v_pdf, c.y / v_pdf, c.z / v_pdf};
}

// AreaEmitter (arealight.cpp:39-76) or EnvironmentMap
template <bool FULL = true>
ND float emitter_pdf(const DevScene &S, const DevEmitter &e, V3 n, V3 wi) {
    if (FULL && e.type == NORI_EMITTER_ENVMAP) return env_pdf(S, e, wi);
    return dot(n, -wi) > 0.0f ? S.shapes[e.shape].area_norm : 0.0f;
}
template <bool FULL = true>
ND V3 emitter_eval(const DevScene &S, const DevEmitter &e, V3 n, V3 wi) {
    if (FULL && e.type == NORI_EMITTER_ENVMAP) return env_eval(S, e, wi);
    return dot(n, -wi) > 0.0f ? V3{e.radiance[0], e.radiance[1], e.radiance[2]} : V3{0, 0, 0};
}
// Shape::sampleSurface: Mesh (mesh.cpp:40-58, DiscretePDF::sampleReuse
// dpdf.h:152-157) or Sphere (sphere.cpp:95-100).
ND void sample_surface(const DevScene &S, const DevShape &sh, V2 smp, V3 &p, V3 &n) {
    if (sh.type == NORI_SHAPE_SPHERE) {
        V3 q = sq_uniform_sphere(smp);
        p = V3{sh.center[0], sh.center[1], sh.center[2]} + q * sh.radius;
        n = q;
        return;
    }
    const float *cdf = S.cdf + sh.cdf_offset;
    uint32_t lo = 0, hi = sh.prim_count + 1;
    float x = smp.x;
    while (lo < hi) {  // lower_bound
        uint32_t mid = (lo + hi) >> 1;
        if (cdf[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    uint32_t idx = lo == 0 ? 0 : lo - 1;
    if (idx > sh.prim_count - 1) idx = sh.prim_count - 1;
    float c0 = cdf[idx], c1 = cdf[idx + 1];
    x = (x - c0) / (c1 - c0);
    V3 bc = sq_uniform_triangle(V2{x, smp.y});
    const uint32_t *f = S.tri_vidx + 3 * (size_t)(sh.prim_offset + idx);
    uint32_t i0 = f[0], i1 = f[1], i2 = f[2];
    V3 p0 = ld3(S.pos[i0]), p1 = ld3(S.pos[i1]), p2 = ld3(S.pos[i2]);
    p = (p0 * bc.x + p1 * bc.y) + p2 * bc.z;
    if (sh.has_normals)
        n = normalize((ld3(S.nrm[i0]) * bc.x + ld3(S.nrm[i1]) * bc.y) + ld3(S.nrm[i2]) * bc.z);
    else
        n = normalize(cross(p1 - p0, p2 - p0));
}

// Camera::sampleRay: PerspectiveCamera (perspective.cpp:90-112), ThinLensCamera
// (thinlens.cpp:120-147) and AdvancedCamera (advancedCamera.cpp:85-157: barrel
// distortion, uniform-disk lens, per-channel focus shift with chromatic
// aberration, channel = 0..2 then; -1 otherwise).  Eigen column order.
template <bool FULL = true>
ND void camera_sample(const DevScene &S, float px, float py, V2 ap, int channel, V3 &o, V3 &d, float &mint,
                      float &maxt, float *invz_out = nullptr) {
    const float *m = S.s2c;
    const float qx = px * S.invW, qy = py * S.invH;
    const float r0 = ((m[0] * qx + m[1] * qy) + m[2] * 0.0f) + m[3];
    const float r1 = ((m[4] * qx + m[5] * qy) + m[6] * 0.0f) + m[7];
    const float r2 = ((m[8] * qx + m[9] * qy) + m[10] * 0.0f) + m[11];
    const float r3 = ((m[12] * qx + m[13] * qy) + m[14] * 0.0f) + m[15];
    V3 nearP = V3{r0 / r3, r1 / r3, r2 / r3};
    V3 dl = normalize(nearP);
    float w = 0.0f;
    bool chroma = false;
    if (FULL && S.cam_type == NORI_CAMERA_ADVANCED) {
        const float k1 = S.distortion[0], k2 = S.distortion[1];
        if (k1 != 0.0f || k2 != 0.0f) {  // Newton iterations for the undistorted radius
            const float ux = nearP.x / nearP.z, uy = nearP.y / nearP.z;
            const float y = sqrtf(ux * ux + uy * uy);
            float r = y, rr, f, df;
            int i = 0;
            for (;;) {
                rr = r * r;
                f = r * (1 + (k1 * rr) + k2 * (rr * rr)) - y;
                df = 1 + (3 * k1 * rr) + (5 * k2 * rr * rr);
                r = r - f / df;
                if ((double)fabsf(f) < 1e-6 || i++ > 4) break;
            }
            const float factor = r / y;
            nearP.x *= factor;
            nearP.y *= factor;
            dl = normalize(nearP);
        }
        chroma = S.chromatic[0] != 0.0f || S.chromatic[1] != 0.0f || S.chromatic[2] != 0.0f;
        if (chroma) w = S.chromatic[channel < 0 ? 0 : (channel > 2 ? 2 : channel)];
    }
    const float invZ = rcp_full(dl.z);
    const float *c = S.c2w;
    V3 lo = V3{0, 0, 0};
    if (FULL && S.cam_type != NORI_CAMERA_PERSPECTIVE && (S.lens_radius > 0.0f || chroma)) {
        V2 pl = S.cam_type == NORI_CAMERA_THINLENS ? sq_concentric_disk(ap) : sq_uniform_disk(ap);
        pl = V2{S.lens_radius * pl.x, S.lens_radius * pl.y};
        const float ft = S.focal / dl.z;
        V3 pf = dl * ft;  // Ray3f(0, d)(ft)
        if (S.cam_type == NORI_CAMERA_ADVANCED) {
            float spx = px - 0.5f * (float)S.W, spy = py - 0.5f * (float)S.H;
            spx /= (float)S.W_max;
            spy /= (float)S.W_max;
            const float sq = spx * spx + spy * spy;
            pf = pf + V3{-((spx * sq) * w), (spy * sq) * w, 0.0f};
        }
        lo = V3{pl.x, pl.y, 0.0f};
        dl = normalize(pf - lo);
        const float hw = ((c[12] * lo.x + c[13] * lo.y) + c[14] * lo.z) + c[15];
        o = V3{(((c[0] * lo.x + c[1] * lo.y) + c[2] * lo.z) + c[3]) / hw,
               (((c[4] * lo.x + c[5] * lo.y) + c[6] * lo.z) + c[7]) / hw,
               (((c[8] * lo.x + c[9] * lo.y) + c[10] * lo.z) + c[11]) / hw};
    } else {
        o = V3{S.cam_o[0], S.cam_o[1], S.cam_o[2]};  // cameraToWorld * (0,0,0,1), same for every ray (host)
    }
    d = V3{(c[0] * dl.x + c[1] * dl.y) + c[2] * dl.z, (c[4] * dl.x + c[5] * dl.y) + c[6] * dl.z,
           (c[8] * dl.x + c[9] * dl.y) + c[10] * dl.z};
    mint = S.near_clip * invZ;
    maxt = S.far_clip * invZ;
    if (invz_out) *invz_out = invZ;  // path queue encoding of a camera ray (path_ray)
}

// ------------------------------------------------------------------ shade + regenerate
struct PathState {
    V3 o, d;
    float mint, maxt;
    V3 beta;
    float prev;  // BSDF pdf of the last bounce; -1: w_mats = 1 (camera ray or discrete lobe)
    Pcg rng;
    uint32_t work;
    bool cam;    // the ray is a camera ray (stored with invz instead of prev)
    uint32_t chan;  // chromatic aberration: the colour channel whose Li this path computes (0 otherwise)
    float invz;  // camera ray: 1/z of its camera-space direction
    V3 L;  // finisher only: the sample's radiance so far (the record, held in registers)
};
struct ShadowOut {
    bool emit;
    V3 o, d, contrib;
    float maxt;
    uint32_t work;
    bool has_em;  // S.nee_inline: the vertex's emission (nee_em_lds) waits for k_shade's record update
};

// Sample id of work id w (render.cpp's (pass, pixel) sample; the pcg32 stream
// key of wave_seed): pass = w / M of the chunk, pixel = the work list's entry.
ND uint64_t sample_id(const DevScene &S, const WorkDesc &wd, uint32_t w) {
    const uint32_t pass = w / wd.M;
    return (uint64_t)(wd.pass_begin + pass) * ((uint64_t)S.W * (uint64_t)S.H) + wd.pixels[w - pass * wd.M];
}
ND void load_path(const DevScene &S, const WorkDesc &wd, const PathQueue &Q, uint32_t q, PathState &ps) {
    const float4 ro = Q.ray_o[q], rd = Q.ray_d[q], th = Q.thr[q];
    const uint32_t sh = Q.rng[q];
    ps.o = ld3(ro);
    ps.d = ld3(rd);
    const uint32_t wf = __float_as_uint(rd.w);
    ps.work = wf & kWorkMask;
    ps.chan = (wf >> kChanShift) & 3u;
    ps.cam = (wf & kCameraRay) != 0u;
    ps.invz = ro.w;
    ps.prev = ps.cam ? -1.0f : ro.w;
    ps.mint = ps.cam ? S.near_clip * ro.w : kEps;
    ps.maxt = ps.cam ? S.far_clip * ro.w : INF_F;
    ps.beta = ld3(th);
    ps.rng.state = ((uint64_t)sh << 32) | __float_as_uint(th.w);
    ps.rng.inc = (sample_id(S, wd, ps.work) << 1u) | 1u;  // pcg32 seed(initstate, initseq = sid)
}
ND void store_path(const PathQueue &Q, uint32_t i, const PathState &ps) {
    Q.ray_o[i] = make_float4(ps.o.x, ps.o.y, ps.o.z, ps.cam ? ps.invz : ps.prev);
    Q.ray_d[i] = make_float4(ps.d.x, ps.d.y, ps.d.z,
                             __uint_as_float(ps.work | (ps.chan << kChanShift) | (ps.cam ? kCameraRay : 0u)));
    Q.thr[i] = make_float4(ps.beta.x, ps.beta.y, ps.beta.z, __uint_as_float((uint32_t)ps.rng.state));
    Q.rng[i] = (uint32_t)(ps.rng.state >> 32);
}

// ------------------------------------------------------------------ medium
// HomogeneousMedium (medium.cpp:22-94): box = origin -/+ |size|, sigma_t =
// sigma_a + sigma_s, albedo = sigma_s / sigma_t, isotropic phase function
// (phasefunction.cpp:13-16).
// BoundingBox3f::rayIntersect(ray, nearT, farT) (bbox.h:366-393) for the ray
// (o, d) with dRcp = 1/d; a NaN direction leaves the slab test false.
ND bool mbox_range(const DevScene &S, V3 o, V3 d, float &nearT, float &farT) {
    nearT = -INF_F;
    farT = INF_F;
    const float oc[3] = {o.x, o.y, o.z}, dc[3] = {d.x, d.y, d.z};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float origin = oc[i], mn = S.mbox_min[i], mx = S.mbox_max[i];
        if (dc[i] == 0.0f) {
            if (origin < mn || origin > mx) return false;
        } else {
            const float r = rcp_full(dc[i]);
            float t1 = (mn - origin) * r, t2 = (mx - origin) * r;
            if (t1 > t2) {
                float t = t1;
                t1 = t2;
                t2 = t;
            }
            nearT = smax(t1, nearT);
            farT = smin(t2, farT);
            if (!(nearT <= farT)) return false;
        }
    }
    return true;
}
ND bool mbox_contains(const DevScene &S, V3 p) {  // bbox.h:115-123 (non-strict)
    return p.x >= S.mbox_min[0] && p.y >= S.mbox_min[1] && p.z >= S.mbox_min[2] && p.x <= S.mbox_max[0] &&
           p.y <= S.mbox_max[1] && p.z <= S.mbox_max[2];
}
// HomogeneousMedium::Tr(src, dst): transmittance over the part of [src, dst]
// inside the box.  Tr(p, p) has a NaN direction and is 1, as in the reference.
ND V3 medium_tr(const DevScene &S, V3 src, V3 dst) {
    if (!S.has_medium) return V3{1, 1, 1};
    const V3 d = normalize(dst - src);
    float nearT, farT;
    if (!mbox_range(S, src, d, nearT, farT)) return V3{1, 1, 1};
    const V3 sp = mbox_contains(S, src) ? src : src + normalize(d) * nearT;
    const V3 ep = mbox_contains(S, dst) ? dst : src + normalize(d) * farT;
    const float n = norm(ep - sp);
    return V3{expf(-S.sigma_t[0] * n), expf(-S.sigma_t[1] * n), expf(-S.sigma_t[2] * n)};
}
// HomogeneousMedium::sample: free-flight distance from the box entry point;
// true (and p) when the ray scatters before tmax.  No random number is drawn
// for a ray that misses the box.
ND bool medium_sample(const DevScene &S, V3 o, V3 d, Pcg &rng, float tmax, V3 &p) {
    if (!S.has_medium) return false;
    float nearT, farT;
    if (!mbox_range(S, o, d, nearT, farT)) return false;
    const V3 sp = mbox_contains(S, o) ? o : o + normalize(d) * nearT;
    const float st = smax(smax(S.sigma_t[0], S.sigma_t[1]), S.sigma_t[2]);
    const float distance = norm(sp - o) + (-1.0f * logf(1 - next1D(rng)) / st);  // invTr
    if (distance >= tmax) return false;
    p = o + d * distance;  // Ray3f::operator()
    return true;
}

// PointLight::sample (pointlight.cpp:17-25) and SpotLight::sample
// (spotlight.cpp:20-46, falloff by the angle to the spot direction) from x:
// returns the radiance, sets the direction and the shadow ray's maxt.
ND V3 point_sample(const DevEmitter &E, V3 x, V3 &wi, float &maxt) {
    const V3 pos = V3{E.position[0], E.position[1], E.position[2]};
    const V3 d = pos - x;
    wi = normalize(d);
    maxt = norm(d) - kEps;
    const V3 pw = V3{E.power[0], E.power[1], E.power[2]};
    if (E.type == NORI_EMITTER_POINT) return pw / (4.f * kPi * dot(d, d));
    const V3 w = -wi, dir = V3{E.direction[0], E.direction[1], E.direction[2]};
    const float cosTheta = dot(dir, normalize(w));
    float fo;
    if (cosTheta < E.cos_tw) fo = 0;
    else if (cosTheta > E.cos_fs) fo = 1;
    else fo = (acosf(E.cos_tw) - acosf(cosTheta)) / (acosf(E.cos_tw) - acosf(E.cos_fs));
    const V3 q = x - pos;
    return (pw * fo) / (4.f * kPi * dot(q, q));
}

// Next-event estimation from x (AreaEmitter::sample, arealight.cpp:52-68):
// one emitter chosen uniformly (scene.h:68-74), Li already scaled by N.
struct NeeSample {
    V3 p, wi, Li;
    float pdf_em, maxt;  // maxt: of the shadow ray from x
};
// Emitter::sample of one emitter from x with the 2D sample s2: radiance over
// pdf (not yet scaled by the emitter count), direction, area-measure pdf and
// the shadow ray's maxt.
template <bool FULL = true, bool CLAMP = false>
ND NeeSample emitter_sample_one(const DevScene &S, const DevEmitter &E, V3 x, V2 s2) {
    NeeSample r;
    if (FULL && (E.type == NORI_EMITTER_POINT || E.type == NORI_EMITTER_SPOT)) {
        r.Li = point_sample(E, x, r.wi, r.maxt);
        r.pdf_em = 1.0f;  // PDF_VALUE (pointlight.cpp:32-35) / lRec.pdf (spotlight.cpp:54-57)
        r.p = V3{E.position[0], E.position[1], E.position[2]};
        return r;
    }
    if (FULL && E.type == NORI_EMITTER_ENVMAP) {
        r.Li = env_sample<CLAMP>(S, E, s2, r.wi);
        r.pdf_em = env_pdf(S, E, r.wi);
        r.maxt = kEnvTFar;               // shadow ray (ref, wi, Epsilon, T_FAR)
        r.p = x + r.wi * kEnvTFar;       // D4: lRec.p is never set by the reference
        return r;
    }
    V3 ln;
    sample_surface(S, S.shapes[E.shape], s2, r.p, ln);
    const V3 dv = r.p - x;
    r.wi = normalize(dv);
    r.pdf_em = emitter_pdf<FULL>(S, E, ln, r.wi);
    const float att = dot(ln, -r.wi) / dot(dv, dv);
    r.Li = r.pdf_em > 0.0f ? (emitter_eval<FULL>(S, E, ln, r.wi) * att) / r.pdf_em : V3{0, 0, 0};
    r.maxt = norm(dv) - kEps;
    return r;
}
// Next-event estimation of the path integrators: one emitter chosen uniformly
// (Scene::getRandomEmitter, scene.h:68-74), Li scaled by the emitter count.
// (ul, s2: the emitter-choice draw and the 2D light sample, in that order)
template <bool FULL = true>
ND NeeSample nee_sample_u(const DevScene &S, V3 x, float ul, V2 s2) {
    const uint32_t N = S.num_emitters;
    uint32_t li = (uint32_t)floorf((float)N * ul);
    if (li > N - 1) li = N - 1;
    NeeSample r = emitter_sample_one<FULL>(S, S.emitters[li], x, s2);
    r.Li = r.Li * (float)N;
    return r;
}
template <bool FULL = true>
ND NeeSample nee_sample(const DevScene &S, V3 x, Pcg &rng) {
    const float ul = next1D(rng);
    const V2 s2 = next2D(rng);
    return nee_sample_u<FULL>(S, x, ul, s2);
}

// Chromatic aberration (render.cpp:106-121): a sample's value is
// value0 + value1 + value2 with value_c = e_c * Li_c (e_c the unit colour of
// channel c), so component c of the record gets Li_c.c and the two other
// paths add 0 * Li_k.c there -- +-0, or NaN when that term is not finite,
// which the splat's validity check then drops, as the reference does.  Each
// contribution of channel c's path goes to the record through this mask.
ND V3 chan_only(const DevScene &S, uint32_t ch, const V3 &a) {
    if (!S.chroma) return a;
    return V3{ch == 0 ? a.x : 0.0f * a.x, ch == 1 ? a.y : 0.0f * a.y, ch == 2 ? a.z : 0.0f * a.z};
}

// Emission found by the shade kernel, added to the sample record.  Each record
// has one path, and the shadow kernel's read-modify-write of it runs in a later
// launch, so the adds need no atomicity -- but returnless atomics do not make
// the wave wait for the record's read (a full memory latency in most waves);
// IEEE adds in the same order, so the sums are identical.
// ATOMIC false (finisher): the sum is kept in ps.L, in registers -- a tail
// path's bounces are a serial chain, and a record read per bounce would add a
// memory latency to each.
// S.nee_inline (k_shade traces the vertex's shadow ray itself): the emission
// waits in so.em for the one read-modify-write of the record at the kernel's
// end, which adds it first and then the unoccluded NEE term -- the order of
// the adds above.
// (in LDS by thread, so that it does not hold registers through the rest of
// the vertex)
ND float *nee_em_lds() {
    __shared__ float s_emt[3 * kSeg];
    return s_emt;
}
template <bool ATOMIC, bool INL>
ND void rec_add(const DevScene &S, float4 *rec, PathState &ps, ShadowOut &so, const V3 &a0) {
    const V3 a = chan_only(S, ps.chan, a0);
    if (!ATOMIC) {
        ps.L = ps.L + a;
        return;
    }
    if (INL && S.nee_inline) {
        float *const e = nee_em_lds() + 3 * threadIdx.x;
        e[0] = a.x;
        e[1] = a.y;
        e[2] = a.z;
        so.has_em = true;
        return;
    }
    float *r = reinterpret_cast<float *>(rec + ps.work);
    atomicAdd(r + 0, a.x);
    atomicAdd(r + 1, a.y);
    atomicAdd(r + 2, a.z);
}

// Deviation D10: a mirror or dielectric BSDF evaluates to exactly zero, so
// the NEE term at such a vertex, attenuation * w_ems * 0 * theta * Li, is zero
// whenever its other factors are finite.  Then only its three random numbers
// (emitter choice, 2D light sample) are drawn and no light is sampled: RR and
// the BSDF sample read the same stream positions, the image is bit-identical.
// Kept in full when the attenuation is not finite or the scene has an
// environment map (its Li can be inf/NaN, which the reference turns into an
// invalid sample); for area/point lights Li is finite unless the vertex
// coincides exactly with the sampled light point.
ND bool skip_nee(const DevScene &S, const DevBsdf &B, const V3 &beta) {
    return S.skip_discrete_nee && (B.type == NORI_BSDF_MIRROR || B.type == NORI_BSDF_DIELECTRIC) &&
           isfinite(beta.x) && isfinite(beta.y) && isfinite(beta.z);
}

// One iteration of VolumetricIntegrator::Li (volumetric.cpp:18-156) for the
// current segment (ps.o, ps.d) and its closest hit h (prim ~0: none, t = inf).
// Free flight first: a scattering event does phase-function NEE with
// transmittance, Russian roulette at 0.8 and a uniform-sphere bounce; else
// the surface vertex does path_mis-style emission and NEE, both weighted by
// transmittance.  ps.prev carries the pdf for w_mats at the next emitter hit
// (1/4pi after a scattering event, -1 after a discrete lobe).
template <bool ATOMIC, bool FULL = true>
ND bool shade_vertex_vol(const DevScene &S, PathState &ps, const float4 &h, float4 *rec, ShadowOut &so) {
    so.emit = false;
    so.has_em = false;
    const uint32_t prim = __float_as_uint(h.y);
    const bool inter = prim != 0xFFFFFFFFu;
    SurfHit hs;
    float tmax = INF_F;
    if (inter) {
        hs = surface<FULL>(S, prim, h.x, h.z, h.w, ps.o, ps.d);
        tmax = norm(hs.p - ps.o);
    }
    V3 mp;
    if (medium_sample(S, ps.o, ps.d, ps.rng, tmax, mp)) {
        const V3 wo = sq_uniform_sphere(next2D(ps.rng));
        const float pdf_mat = kInvFourPi;
        NeeSample ne = nee_sample<FULL>(S, mp, ps.rng);
        ps.beta = ps.beta * V3{S.albedo[0], S.albedo[1], S.albedo[2]};
        const V3 tr = medium_tr(S, mp, ne.p);
        so.contrib = chan_only(S, ps.chan, ((ps.beta * tr) * ne.Li) * pdf_mat);
        so.emit = !is_zero(so.contrib);
        so.o = mp;
        so.d = ne.wi;
        so.maxt = ne.maxt;
        so.work = ps.work;
        const float q = smin(ps.beta.x, 0.80f);
        if (next1D(ps.rng) > q) return false;
        ps.beta = ps.beta / q;
        ps.o = mp;
        ps.d = normalize(wo);
        ps.mint = kEps;
        ps.maxt = INF_F;
        ps.prev = pdf_mat;
        return true;
    }
    if (!inter) return false;  // escaped (volumetric.cpp: break)
    const DevShape &sh = S.shapes[hs.shape];
    const DevBsdf &B = S.bsdfs[sh.bsdf];
    if (sh.emitter >= 0) {
        const DevEmitter &E = S.emitters[sh.emitter];
        const V3 wi = normalize(hs.p - ps.o);
        const V3 Le = emitter_eval<FULL>(S, E, hs.sh.n, wi);
        float w = 1.0f;
        if (ps.prev >= 0.0f) {
            const float pe = emitter_pdf<FULL>(S, E, hs.sh.n, wi);
            w = ps.prev + pe > 0.f ? ps.prev / (ps.prev + pe) : ps.prev;
        }
        const V3 Ladd = ((ps.beta * w) * Le) * medium_tr(S, hs.p, hs.p);
        rec_add<ATOMIC, !FULL || kNeeFull>(S, rec, ps, so, Ladd);
    }
    if (skip_nee(S, B, ps.beta)) {
        pcg_skip(ps.rng, 3);
    } else {
        NeeSample ne = nee_sample<FULL>(S, hs.p, ps.rng);
        BRec br;
        br.wi = to_local(hs.sh, -ps.d);
        br.uv = hs.uv;
        br.wo = to_local(hs.sh, ne.wi);
        br.measure = kMeasureSolidAngle;
        const float theta = smax(0.0f, br.wo.z);
        const V3 f = bsdf_eval<FULL>(B, br);
        const float pdf_mat = bsdf_pdf<FULL>(B, br);
        const float w_ems = (pdf_mat + ne.pdf_em) > 0.0f ? ne.pdf_em / (pdf_mat + ne.pdf_em) : ne.pdf_em;
        const V3 tr = medium_tr(S, hs.p, ne.p);
        so.contrib = chan_only(S, ps.chan, ((((ps.beta * w_ems) * f) * theta) * ne.Li) * tr);
        so.emit = !is_zero(so.contrib);
        so.o = hs.p;
        so.d = ne.wi;
        so.maxt = ne.maxt;
        so.work = ps.work;
    }
    const float q = smin(ps.beta.x, 0.80f);
    if (next1D(ps.rng) > q) return false;
    ps.beta = ps.beta / q;
    BRec br;
    br.wi = to_local(hs.sh, -ps.d);
    br.uv = hs.uv;
    br.wo = V3{0, 0, 1};
    br.measure = kMeasureUnknown;
    const V3 w = bsdf_sample<FULL>(B, br, next2D(ps.rng));
    if (is_zero(w)) return false;  // deviation D1
    ps.beta = ps.beta * w;
    const float pm = bsdf_pdf<FULL>(B, br);
    ps.prev = br.measure == kMeasureDiscrete ? -1.0f : pm;
    ps.o = hs.p;
    ps.d = to_world(hs.sh, br.wo);
    ps.mint = kEps;
    ps.maxt = INF_F;
    return true;
}

// One vertex of PathMisIntegrator::Li (path_mis.cpp:32-97) or
// PathMatsIntegrator::Li (path_mats.cpp:26-57) given the closest hit of the
// current ray.  Returns true if the path continues (ps holds the new ray).
template <int INTEG, bool ATOMIC, bool FULL = true>
ND bool shade_vertex(const DevScene &S, PathState &ps, const float4 &h, float4 *rec, ShadowOut &so) {
    if constexpr (INTEG == NORI_INTEGRATOR_VOLUMETRIC) return shade_vertex_vol<ATOMIC, FULL>(S, ps, h, rec, so);
    so.emit = false;
    so.has_em = false;
    uint32_t prim = __float_as_uint(h.y);
    if (prim == 0xFFFFFFFFu) return false;  // escaped: path_mis.cpp:84-85
    constexpr bool MIS = INTEG == NORI_INTEGRATOR_PATH_MIS;
    SurfHit hs = surface<FULL>(S, prim, h.x, h.z, h.w, ps.o, ps.d);
    const DevShape &sh = S.shapes[hs.shape];
    const DevBsdf &B = S.bsdfs[sh.bsdf];
    if (sh.emitter >= 0) {  // emission (path_mis.cpp:35-39, path_mats.cpp:31-35)
        const DevEmitter &E = S.emitters[sh.emitter];
        V3 wi = normalize(hs.p - ps.o);
        V3 Le = emitter_eval<FULL>(S, E, hs.sh.n, wi);
        V3 Ladd;
        if (MIS) {
            float w = 1.0f;  // w_mats (path_mis.cpp:87-97)
            if (ps.prev >= 0.0f) {
                float pe = emitter_pdf<FULL>(S, E, hs.sh.n, wi);
                w = ps.prev + pe > 0.f ? ps.prev / (ps.prev + pe) : ps.prev;
            }
            Ladd = (ps.beta * w) * Le;
        } else {
            Ladd = ps.beta * Le;
        }
        rec_add<ATOMIC, !FULL || kNeeFull>(S, rec, ps, so, Ladd);
    }
    if (MIS && skip_nee(S, B, ps.beta)) {
        pcg_skip3(ps.rng);  // deviation D10: the three NEE draws, unused
    } else if (MIS) {  // next-event estimation (path_mis.cpp:42-61)
        const NeeSample ne = nee_sample<FULL>(S, hs.p, ps.rng);
        BRec br;
        br.wi = to_local(hs.sh, -ps.d);
        br.uv = hs.uv;
        br.wo = to_local(hs.sh, ne.wi);
        br.measure = kMeasureSolidAngle;
        float theta = smax(0.0f, br.wo.z);
        V3 f = bsdf_eval<FULL>(B, br);
        float pdf_mat = bsdf_pdf<FULL>(B, br);
        float w_ems = (pdf_mat + ne.pdf_em) > 0.0f ? ne.pdf_em / (pdf_mat + ne.pdf_em) : ne.pdf_em;
        so.contrib = chan_only(S, ps.chan, (((ps.beta * w_ems) * f) * theta) * ne.Li);
        so.emit = !is_zero(so.contrib);  // a zero contribution adds nothing (NaN still goes)
        so.o = hs.p;
        so.d = ne.wi;
        so.maxt = ne.maxt;
        so.work = ps.work;
    }
    // Russian roulette on the red channel (path_mis.cpp:64-69)
    float qrr = smin(ps.beta.x, 0.99f);
    if (next1D(ps.rng) > qrr) return false;
    ps.beta = ps.beta / qrr;
    BRec br;
    br.wi = to_local(hs.sh, -ps.d);
    br.uv = hs.uv;
    br.wo = V3{0, 0, 1};
    br.measure = kMeasureUnknown;
    V3 w = bsdf_sample<FULL>(B, br, next2D(ps.rng));
    if (is_zero(w)) return false;  // deviation D1: zero-weight samples end the path
    ps.beta = ps.beta * w;
    if (MIS) {
        float pm = bsdf_pdf<FULL>(B, br);
        ps.prev = br.measure == kMeasureDiscrete ? -1.0f : pm;
    }
    ps.o = hs.p;
    ps.d = to_world(hs.sh, br.wo);
    ps.mint = kEps;
    ps.maxt = INF_F;
    return true;
}

// shade_vertex at a vertex of a solitary, non-emitting dielectric sphere
// whose next-event estimation is skipped (skip_nee: deviation D10), reduced
// to the operations that run there -- the same arithmetic in the same order
// (surface(): hit point, normal, frame; the three skipped NEE draws; Russian
// roulette; Dielectric::sample; the discrete pdf) without the plugin
// dispatch: the tail finisher's trapped glass-sphere paths run a chain of
// these.  t: the chord's closest hit.  Returns false if the path ends.
// NORI_GLASS_FAST_SQRT=1: sqrt_rn (range-checked fast sqrt) in the glass
// chain instead of the IEEE sequence -- its branch costs more than it saves
// for a lone lane (958-965 against 1026-1049 ns per chord bounce, round 6).
#ifndef NORI_GLASS_FAST_SQRT
#define NORI_GLASS_FAST_SQRT 0
#endif
constexpr bool kGlassFast = NORI_GLASS_FAST_SQRT;
#ifndef NORI_GLASS_STEP  // 0: every chord bounce through glass_bounce / chord_hit
#define NORI_GLASS_STEP 1
#endif
constexpr bool kGlassStep = NORI_GLASS_STEP;
template <int INTEG>
ND bool glass_bounce(const DevShape &sh, const DevBsdf &B, PathState &ps, float t) {
    const V3 p = ps.o + ps.d * t;
    const Frame f = frame_from<kGlassFast>(normalize<kGlassFast>(p - V3{sh.center[0], sh.center[1], sh.center[2]}));
    if (INTEG == NORI_INTEGRATOR_PATH_MIS) pcg_skip3(ps.rng);
    const float qrr = smin(ps.beta.x, 0.99f);
    if (next1D(ps.rng) > qrr) return false;
    ps.beta = ps.beta / qrr;  // (times the sample weight 1, exactly)
    const V3 wo = dielectric_wo<kGlassFast>(B, to_local(f, -ps.d), next2D(ps.rng));
    if (INTEG == NORI_INTEGRATOR_PATH_MIS) ps.prev = -1.0f;  // discrete measure
    ps.o = p;
    ps.d = to_world(f, wo);
    ps.mint = kEps;
    ps.maxt = INF_F;
    return true;
}

// One chord bounce of a path trapped in a solitary dielectric sphere, as
// straight-line code: glass_bounce at the chord's end t followed by the next
// chord (chord_hit), with every early-out of the reference's functions turned
// into a select -- the same operations in the same order on the same values
// (surface(): hit point, normal, coordinateSystem frame; the three skipped
// NEE draws; Russian roulette; fresnel; the reflected direction; the sphere
// test of the next chord with the adaptive epsilon).  A lone lane pays for
// every branch of the general code in exec-mask switches (the chain is its
// dependent latency: ~1 us per bounce), so the common case -- the ray is
// reflected back inside and hits the sphere again -- runs here; true (and
// ps, t updated) only in that case.  Otherwise nothing is changed and the
// caller runs the bounce through glass_bounce / chord_hit, which produce the
// refraction, the Russian-roulette end or the exit.  (sqrtf and the
// divisions are the IEEE sequences: the range-checked fast forms' branches
// measured slower here)
template <int INTEG>
ND bool glass_step(const DevShape &sh, const DevBsdf &B, PathState &ps, float &t) {
    const V3 c = V3{sh.center[0], sh.center[1], sh.center[2]};
    const V3 p = ps.o + ps.d * t;
    const V3 n = normalize(p - c);
    // frame_from(n) (frame.h:49-51, common.cpp:274-283) with the branch as selects
    const bool bx = fabsf(n.x) > fabsf(n.y);
    const float a = bx ? n.x : n.y;
    const float invLen = 1.0f / sqrtf(a * a + n.z * n.z);  // == rcp_full(), without its range branch
    Frame f;
    f.n = n;
    f.t = bx ? V3{n.z * invLen, 0.0f, -n.x * invLen} : V3{0.0f, n.z * invLen, -n.y * invLen};
    f.s = cross(f.t, n);
    Pcg rng = ps.rng;
    if (INTEG == NORI_INTEGRATOR_PATH_MIS) pcg_skip3(rng);
    const float qrr = smin(ps.beta.x, 0.99f);
    const bool survive = !(next1D(rng) > qrr);
    const V3 beta = ps.beta / qrr;
    const V3 wi = to_local(f, -ps.d);
    const V2 s2 = next2D(rng);
    // fresnel(wi.z, ext, int) (common.cpp:285-314) with its branches as selects
    const bool inside = wi.z < 0.0f;
    const float etaI = inside ? B.int_ior : B.ext_ior, etaT = inside ? B.ext_ior : B.int_ior;
    const float eta = inside ? B.eta_ie : B.eta_ei, ci = inside ? -wi.z : wi.z;
    const float sin2 = eta * eta * (1 - ci * ci);
    const float ct = sqrtf(1.0f - sin2);
    const float Rs = (etaI * ci - etaT * ct) / (etaI * ci + etaT * ct);
    const float Rp = (etaT * ci - etaI * ct) / (etaT * ci + etaI * ct);
    const float F = B.ext_ior == B.int_ior ? 0.0f : (sin2 > 1.0f ? 1.0f : (Rs * Rs + Rp * Rp) / 2.0f);
    const bool reflect = F > s2.x;  // Dielectric::sample's reflection: wo = (-wi.x, -wi.y, wi.z)
    const V3 d = to_world(f, V3{-wi.x, -wi.y, wi.z});
    // the next chord: chord_hit (sphere_hit_nb with the adaptive epsilon, bvh.cpp:412-418)
    TRay r;
    r.o = p;
    r.d = d;
    r.mint = smax(kEps, kEps * smax(smax(fabsf(p.x), fabsf(p.y)), fabsf(p.z)));
    r.maxt = INF_F;
    float tn;
    const bool hit = sphere_hit_nb(make_float4(c.x, c.y, c.z, 0.0f), make_float4(sh.radius, 0.0f, 0.0f, 0.0f), r, tn);
    // path_mis: the next vertex's NEE must still be skippable (skip_nee: a
    // finite throughput), else the caller's general bounce takes over
    const bool fin = INTEG != NORI_INTEGRATOR_PATH_MIS || (isfinite(beta.x) && isfinite(beta.y) && isfinite(beta.z));
    if (!(survive && reflect && hit && fin)) return false;
    ps.rng = rng;
    ps.beta = beta;
    if (INTEG == NORI_INTEGRATOR_PATH_MIS) ps.prev = -1.0f;  // discrete measure
    ps.o = p;
    ps.d = d;
    ps.mint = kEps;
    ps.maxt = INF_F;
    t = tn;
    return true;
}

// New camera sample for work id w (render.cpp:98-126 + independent.cpp).
// pix = wd.pixels[w mod M], loaded by the caller (early: a load issued
// after the path stores would wait for them too -- vmcnt counts in order)
template <bool FULL = true>
ND void regen_path(const DevScene &S, const WorkDesc &wd, uint32_t w, uint32_t pix, PathState &ps, float4 *rec) {
    uint32_t pass = w / wd.M;
    uint32_t W = (uint32_t)S.W;
    uint32_t y = pix / W, x = pix - y * W;
    uint64_t sid = (uint64_t)(wd.pass_begin + pass) * ((uint64_t)S.W * (uint64_t)S.H) + pix;
    wave_seed(ps.rng, wd.seed, sid);
    V2 jit = next2D(ps.rng);
    const V2 ap = next2D(ps.rng);  // apertureSample (render.cpp:99)
    camera_sample<FULL>(S, (float)x + jit.x, (float)y + jit.y, ap, -1, ps.o, ps.d, ps.mint, ps.maxt, &ps.invz);
    ps.cam = true;
    ps.chan = 0;
    ps.beta = V3{1, 1, 1};
    ps.prev = -1.0f;
    ps.work = w;
    rec[w] = make_float4(0, 0, 0, rec_code(S.jit_lk, S.border, x, y, jit));
}

// Chromatic aberration: channel ps.chan's Li has ended, so the sample goes on
// with the next channel's camera ray (render.cpp:106-121: the three rays share
// the pixel and aperture samples, their Li calls consume the sampler in turn,
// so the pcg32 state simply continues).
template <bool FULL = true>
ND void next_channel(const DevScene &S, const WorkDesc &wd, PathState &ps) {
    const uint32_t pass = ps.work / wd.M, pix = wd.pixels[ps.work - pass * wd.M];
    const uint32_t W = (uint32_t)S.W, y = pix / W, x = pix - y * W;
    Pcg r;
    wave_seed(r, wd.seed, (uint64_t)(wd.pass_begin + pass) * ((uint64_t)S.W * (uint64_t)S.H) + pix);
    const V2 jit = next2D(r);
    const V2 ap = next2D(r);
    ps.chan += 1;
    camera_sample<FULL>(S, (float)x + jit.x, (float)y + jit.y, ap, (int)ps.chan, ps.o, ps.d, ps.mint, ps.maxt, &ps.invz);
    ps.cam = true;
    ps.beta = V3{1, 1, 1};
    ps.prev = -1.0f;
}

// The chord of a solitary sphere (DevShape::solitary): a ray leaving a point
// of sphere `sh` that hits the sphere again at t hits nothing else before t,
// and for a ray that starts on the sphere the root box test of the scan
// passes (the ball lies inside the scene box by a margin).  Same arithmetic
// as the scan's sphere test (sphere_hit_nb, the adaptive epsilon of
// bvh.cpp:412-418), so t is the scan's; false: the caller scans as usual.
template <bool FAST = false>
ND bool chord_hit(const DevShape &sh, const PathState &ps, float &t) {
    TRay r;
    r.o = ps.o;
    r.d = ps.d;
    r.mint = ps.mint;
    r.maxt = ps.maxt;
    if (r.mint == kEps) r.mint = smax(r.mint, r.mint * smax(smax(fabsf(r.o.x), fabsf(r.o.y)), fabsf(r.o.z)));
    if (r.maxt < r.mint) return false;
    return sphere_hit_nb<FAST>(make_float4(sh.center[0], sh.center[1], sh.center[2], 0.0f),
                               make_float4(sh.radius, 0.0f, 0.0f, 0.0f), r, t);
}

// ImageBlock::put(pos, val) (block.cpp:93-122) of one sample straight into
// the film, with the block-relative coordinates of the sample's own block so
// the filter weights round exactly as in k_splat.
ND void splat_sample(const DevScene &S, float *film, Counters *C, uint32_t x, uint32_t y, V2 jit, float4 L,
                     float *var) {
    if (L.x < 0 || !isfinite(L.x) || L.y < 0 || !isfinite(L.y) || L.z < 0 || !isfinite(L.z)) {
        atomicAdd(&C->invalid, 1ull);
        return;
    }
    if (var) {  // the pixel's sample statistics (nori_gpu_render_desc.variance_out)
        float *v = var + 8 * ((size_t)y * S.W + x);
        atomicAdd(v + 0, L.x);
        atomicAdd(v + 1, L.y);
        atomicAdd(v + 2, L.z);
        atomicAdd(v + 3, L.x * L.x);
        atomicAdd(v + 4, L.y * L.y);
        atomicAdd(v + 5, L.z * L.z);
        atomicAdd(v + 6, 1.0f);
    }
    const int B = S.border, TS = NORI_BLOCK_SIZE + 2 * B, FW = S.W + 2 * B;
    const int ox = (int)(x / NORI_BLOCK_SIZE) * NORI_BLOCK_SIZE, oy = (int)(y / NORI_BLOCK_SIZE) * NORI_BLOCK_SIZE;
    const float rad = S.filter_radius, lk = S.lookup;
    float px = ((float)x + jit.x) - 0.5f - (float)(ox - B), py = ((float)y + jit.y) - 0.5f - (float)(oy - B);
    int x0 = max((int)ceilf(px - rad), 0), y0 = max((int)ceilf(py - rad), 0);
    int x1 = min((int)floorf(px + rad), TS - 1), y1 = min((int)floorf(py + rad), TS - 1);
    for (int cy = y0; cy <= y1; ++cy) {
        float wy = S.filter[min((int)(fabsf((float)cy - py) * lk), NORI_FILTER_RESOLUTION)];
        for (int cx = x0; cx <= x1; ++cx) {
            float wx = S.filter[min((int)(fabsf((float)cx - px) * lk), NORI_FILTER_RESOLUTION)];
            float *f = film + 4 * ((size_t)(oy + cy) * FW + (ox + cx));
            float a = (L.x * wx) * wy, b = (L.y * wx) * wy, c = (L.z * wx) * wy, w = (1.0f * wx) * wy;
            if (w != 0.0f || a != 0.0f || b != 0.0f || c != 0.0f) {
                atomicAdd(f + 0, a);
                atomicAdd(f + 1, b);
                atomicAdd(f + 2, c);
                atomicAdd(f + 3, w);
            }
        }
    }
}

}  // namespace nori
