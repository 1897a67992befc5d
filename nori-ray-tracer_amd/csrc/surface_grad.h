// surface_grad.h -- the hit record's adjoint in the vertices: the 18 terms of
// one mesh hit, in the operation order stated at nori_scene_surface_grad in
// nori_gpu.h.  One routine for the host statement (queries.hip) and the
// device kernel (kernels_surface_grad.hip), so the two form the same bits.
#pragma once
#include "device_math.h"

namespace nori {

struct SurfGradTerms {
    V3 p[3];  // g_p0, g_p1, g_p2
    V3 n[3];  // g_n0, g_n1, g_n2 (zero unless the mesh interpolates its own normals)
};

// The position terms of a hit (u, v) at distance t of the ray (o, d) on the
// triangle p0 p1 p2, for the record gradient (g_p, g_t, g_ng'), where g_ng' is
// g_ng on a mesh with vertex normals and g_ng + g_ns on one without.  False,
// with nothing written: |N| = 0 or N.d = 0.
NHD bool surface_grad_positions(V3 p0, V3 p1, V3 p2, V3 o, V3 d, float t, float u, float v, V3 g_p, float g_t, V3 g_ngp,
                                V3 (&out)[3]) {
    const float b = 1 - (u + v);
    const V3 e1 = p1 - p0, e2 = p2 - p0;
    const V3 N = cross(e1, e2);
    const float len = sqrtf(dot(N, N));
    const float D = dot(N, d);
    if (!(len > 0.0f) || D == 0.0f) return false;
    const V3 ng = N / len;
    V3 gN = (g_ngp - ng * dot(ng, g_ngp)) / len;
    const float s = g_t / D;
    const V3 ph = o + d * t;
    gN = gN + (p0 - ph) * s;
    const V3 ge1 = cross(e2, gN), ge2 = cross(gN, e1);
    out[0] = (g_p * b + N * s) - (ge1 + ge2);
    out[1] = g_p * u + ge1;
    out[2] = g_p * v + ge2;
    return true;
}

// The normal terms, for a mesh with vertex normals and no normal map.  False,
// with nothing written: |M| = 0.
NHD bool surface_grad_normals(V3 n0, V3 n1, V3 n2, float u, float v, V3 g_ns, V3 (&out)[3]) {
    const float b = 1 - (u + v);
    const V3 M = (n0 * b + n1 * u) + n2 * v;
    const float len = sqrtf(dot(M, M));
    if (!(len > 0.0f)) return false;
    const V3 ns = M / len;
    const V3 gM = (g_ns - ns * dot(ns, g_ns)) / len;
    out[0] = gM * b;
    out[1] = gM * u;
    out[2] = gM * v;
    return true;
}

}  // namespace nori
