// bsdf_grad.h -- bsdf_eval's adjoint in the material row: the 16 terms of one
// element, in the operation order stated at nori_scene_bsdf_grad in
// nori_gpu.h.  One routine for the host statement (materials.hip) and the
// device kernel (kernels_bsdf_grad.hip), so the two form the same bits up to
// the math library's expf (microfacet only).  The forward factors are the
// routines bsdf_eval / bsdf_pdf call (beckmann_D, smith_G1, fresnel, schlick,
// ggx, sq_gtr2_pdf, tan_theta, checker_value1 of device_math.h): the
// derivative cannot drift from the value it differentiates.
//
// Every operation is fp32 rounded once (no contraction), evaluated as written
// below, left to right.  The Disney adjoint, with g = (g_r, g_g, g_b), white =
// (1, 1, 1), w = the luminance weights and the forward's own intermediates
//   l, ctint, smix, tint = lerp(spec_tint, white, ctint), T = tint smix,
//   cspec = lerp(m, T, base), fd90, fl, fv, A = 1 + (fd90 - 1) fl,
//   B = 1 + (fd90 - 1) fv, diffuse, alpha, Ds, FH, Fs, gl = ggx(NdotL),
//   gv = ggx(NdotV), Gs = gl gv, scol = lerp(sheen_tint, white, ctint), fsheen:
//   eval = (diffuse + fsheen) (1 - m) + (Fs Gs) Ds, zero unless wi.z >= 0 and wo.z >= 0
//     g_m   = -dot(g, diffuse + fsheen)
//     gd    = g (1 - m)                      (the gradient in diffuse and in fsheen)
//     gFs   = g (Gs Ds);  q = dot(g, Fs);  g_Gs = q Ds;  g_Ds = q Gs
//     gcs   = gFs (1 - FH)                   (in cspec)
//     g_m   = g_m + dot(gcs, base - T)
//     gbase = gcs m;  gT = gcs (1 - m)
//     g_spec = dot(gT, tint) 0.08;  gtm = gT smix
//     g_spt = dot(gtm, ctint - white);  gct = gtm spec_tint
//     g_sh  = dot(gd, scol) FH;  gsc = gd (FH sheen)
//     g_st  = dot(gsc, ctint - white);  gct = gct + gsc sheen_tint
//     l > 0:  gbase = gbase + (gct - w dot(gct, ctint)) / l
//     gbase = gbase + gd ((A B) ipi)
//     g_fd  = (dot(gd, base) ipi) (fl B + A fv)
//     g_r   = g_fd (2 (VdotH VdotH))
//     r r > 0.001 (float):  g_r = g_r + (g_Ds dDs(alpha) + g_Gs (dgl gv + gl dgv)) (2 r)
//       dDs(a) = Ds ((2 / a) (1 - 2 (a a) (c c) / (1 + (a a - 1) (c c)))), c = wh.z; 0 in gtr2's zero branch
//       dggx(x) = -(ggx ggx) (a (1 - x x) / sqrt(a a + x x - (a a) (x x)))
//   pdf = (1 - m) (c ipi) + m (Dp J), Dp = gtr2(wh, d_alpha), J = wh.z / (4 |wh.wo|), zero unless wo.z > 0
//     g_m = g_m + g_p (Dp J - c ipi)
//     r r > 1e-3 (double):  g_r = g_r + ((g_p m) (dDs(d_alpha) J)) (2 r)
//   row: 0-2 gbase, 4 g_m, 5 g_spec, 6 g_r, 7 g_sh, 8 g_st, 9 g_spt.
#pragma once
#include "device_math.h"
#include "material_row.h"

namespace nori {

// d smith_G1 / d alpha: 0 on the routine's early returns and its a >= 1.6 branch
NHD float smith_G1_dalpha(const DevBsdf &b, V3 v, V3 m) {
    const float tanTheta = tan_theta(v);
    if (tanTheta == 0.0f) return 0.0f;
    if (dot(m, v) * v.z <= 0) return 0.0f;
    const float a = rcp_full(b.alpha * tanTheta);
    if (a >= 1.6f) return 0.0f;
    const float a2 = a * a;
    const float N = 3.535f * a + 2.181f * a2, Q = 1.0f + 2.276f * a + 2.577f * a2;
    return ((3.535f + 4.362f * a) * Q - N * (2.276f + 5.154f * a)) / (Q * Q) * (-(a / b.alpha));
}
// d sq_gtr2_pdf / d alpha, from its value Ds
NHD float gtr2_dalpha(V3 m, float alpha, float Ds) {
    const float c = m.z;
    if (!(c >= 0 && fabsf(dot(m, m) - 1.0f) < 1.0f)) return 0.0f;
    const float a2 = alpha * alpha, c2 = c * c;
    return Ds * ((2.0f / alpha) * (1.0f - 2.0f * a2 * c2 / (1.0f + (a2 - 1.0f) * c2)));
}
// d ggx / d alphaG, from its value gx
NHD float ggx_dalpha(float NdotV, float alphaG, float gx) {
    const float a = alphaG * alphaG, b = NdotV * NdotV;
    return -(gx * gx) * (alphaG * (1.0f - b) / sqrtf(a + b - a * b));
}

// The row of one element in local directions (r as k_bsdf_eval forms it).
// False with t all zero: nothing contributes (a zero branch of the forward, a
// BSDF without parameters, a non-finite gradient word or term).
NHD bool bsdf_grad_row(const DevBsdf &b, const BRec &r, float g_r, float g_g, float g_b, float g_p,
                       float (&t)[NORI_MATERIAL_FLOATS]) {
    for (int w = 0; w < NORI_MATERIAL_FLOATS; ++w) t[w] = 0.0f;
    switch (b.type) {
    case NORI_BSDF_DIFFUSE: {
        if (b.tex == NORI_TEXTURE_IMAGE || r.wi.z <= 0 || r.wo.z <= 0) return false;
        const int o = b.tex == NORI_TEXTURE_CHECKERBOARD && !checker_value1(b, r.uv) ? 10 : 0;
        t[o] = g_r * kInvPi, t[o + 1] = g_g * kInvPi, t[o + 2] = g_b * kInvPi;
        break;
    }
    case NORI_BSDF_MICROFACET: {
        const V3 h = normalize(r.wi + r.wo);
        const float D = beckmann_D(b, h);
        const float F = fresnel(dot(h, r.wi), b.ext_ior, b.int_ior, b.eta_ei, b.eta_ie);
        const float Gi = smith_G1(b, r.wi, h), Go = smith_G1(b, r.wo, h);
        const float den = 4.0f * r.wi.z * r.wo.z;
        const float gs = (g_r + g_g) + g_b;
        const float tt = tan_theta(h) / b.alpha;
        const float dD = D * (2.0f * (tt * tt - 1.0f) / b.alpha);
        const float dG = smith_G1_dalpha(b, r.wi, h) * Go + Gi * smith_G1_dalpha(b, r.wo, h);
        const float s_ks = D * F * (Gi * Go) / den;
        const float s_al = b.ks * F * (dD * (Gi * Go) + D * dG) / den;
        float p_ks = 0.0f, p_al = 0.0f;
        if (!(r.wo.z <= 0.0f)) {
            const float J = h.z / (4.0f * fabsf(dot(h, r.wo)));
            p_ks = D * J - r.wo.z * kInvPi;
            p_al = b.ks * (dD * J);
        }
        t[0] = g_r * kInvPi, t[1] = g_g * kInvPi, t[2] = g_b * kInvPi;
        t[3] = gs * s_al + g_p * p_al;
        int m = b.kd[0] < b.kd[1] ? 1 : 0;  // the first channel that attains max(kd)
        m = b.kd[m] < b.kd[2] ? 2 : m;
        t[m] = t[m] - (gs * s_ks + g_p * p_ks);
        break;
    }
    case NORI_BSDF_DISNEY: {
        const float NdotV = r.wi.z, NdotL = r.wo.z;
        const bool ev = !(NdotV < 0 || NdotL < 0), pd = !(NdotL <= 0.0f);
        if (!ev && !pd) return false;
        const V3 wh = normalize(r.wi + r.wo);
        const V3 base = V3{b.base[0], b.base[1], b.base[2]}, white = V3{1, 1, 1};
        const float m = b.metallic, rr = b.roughness;
        V3 gbase = V3{0, 0, 0};
        float g_m = 0.0f, g_spec = 0.0f, g_rr = 0.0f, g_sh = 0.0f, g_st = 0.0f, g_spt = 0.0f;
        if (ev) {
            const float LdotH = dot(r.wo, wh), VdotH = dot(r.wi, wh);
            const float l = luminance(base);
            const V3 ctint = (l > 0.f) ? V3{base.x / l, base.y / l, base.z / l} : white;
            const float smix = (float)((double)b.specular * 0.08);
            const V3 tint = lerp3(b.spec_tint, white, ctint);
            const V3 T = tint * smix;
            const V3 cspec = lerp3(m, T, base);
            const float fd90 = (float)(0.5 + (double)(2 * rr) * ((double)VdotH * (double)VdotH));
            const float fl = schlick(NdotL), fv = schlick(NdotV);
            const float A = 1.f + (fd90 - 1.f) * fl, B = 1.f + (fd90 - 1.f) * fv;
            const V3 diffuse = ((base * kInvPi) * A) * B;
            const float alpha = smax(0.001f, rr * rr);
            const float Ds = sq_gtr2_pdf(wh, alpha);
            const float FH = schlick(LdotH);
            const V3 Fs = lerp3(FH, cspec, white);
            const float gl = ggx(NdotL, alpha), gv = ggx(NdotV, alpha), Gs = gl * gv;
            const V3 scol = lerp3(b.sheen_tint, white, ctint);
            const V3 fsheen = scol * (FH * b.sheen);
            const V3 g = V3{g_r, g_g, g_b};
            g_m = -dot(g, diffuse + fsheen);
            const V3 gd = g * (1.0f - m);
            const V3 gFs = g * (Gs * Ds);
            const float q = dot(g, Fs);
            const float g_Gs = q * Ds, g_Ds = q * Gs;
            const V3 gcs = gFs * (1.0f - FH);
            g_m = g_m + dot(gcs, base - T);
            gbase = gcs * m;
            const V3 gT = gcs * (1.0f - m);
            g_spec = dot(gT, tint) * 0.08f;
            const V3 gtm = gT * smix;
            g_spt = dot(gtm, ctint - white);
            V3 gct = gtm * b.spec_tint;
            g_sh = dot(gd, scol) * FH;
            const V3 gsc = gd * (FH * b.sheen);
            g_st = dot(gsc, ctint - white);
            gct = gct + gsc * b.sheen_tint;
            if (l > 0.f) gbase = gbase + (gct - V3{0.212671f, 0.715160f, 0.072169f} * dot(gct, ctint)) / l;
            gbase = gbase + gd * ((A * B) * kInvPi);
            const float g_fd = (dot(gd, base) * kInvPi) * (fl * B + A * fv);
            g_rr = g_fd * (2.0f * (VdotH * VdotH));
            if (rr * rr > 0.001f) {
                const float dgl = ggx_dalpha(NdotL, alpha, gl), dgv = ggx_dalpha(NdotV, alpha, gv);
                g_rr = g_rr + (g_Ds * gtr2_dalpha(wh, alpha, Ds) + g_Gs * (dgl * gv + gl * dgv)) * (2.0f * rr);
            }
        }
        if (pd) {
            const float Dp = sq_gtr2_pdf(wh, b.d_alpha);
            const float J = wh.z / (4.0f * fabsf(dot(wh, r.wo)));
            g_m = g_m + g_p * (Dp * J - NdotL * kInvPi);
            if ((double)rr * (double)rr > 1e-3) g_rr = g_rr + ((g_p * m) * (gtr2_dalpha(wh, b.d_alpha, Dp) * J)) * (2.0f * rr);
        }
        t[0] = gbase.x, t[1] = gbase.y, t[2] = gbase.z;
        t[4] = g_m, t[5] = g_spec, t[6] = g_rr, t[7] = g_sh, t[8] = g_st, t[9] = g_spt;
        break;
    }
    default:  // mirror / dielectric: no parameters
        return false;
    }
    // finite throughout, or a zero row: (x - x) is 0 exactly for a finite x, NaN otherwise
    float bad = (g_r - g_r) + (g_g - g_g) + (g_b - g_b) + (g_p - g_p);
    for (int w = 0; w < NORI_MATERIAL_FLOATS; ++w) bad += t[w] - t[w];
    if (bad == 0.0f) return true;
    for (int w = 0; w < NORI_MATERIAL_FLOATS; ++w) t[w] = 0.0f;
    return false;
}

// The row of element (record ns / uv, world wi and wo) on BSDF b: the frame and to_local of k_bsdf_eval.
NHD bool bsdf_grad_element(const DevBsdf &b, V3 ns, float u, float v, V3 wi, V3 wo, float g_r, float g_g, float g_b,
                           float g_p, float (&t)[NORI_MATERIAL_FLOATS]) {
    const Frame f = frame_from(ns);
    BRec br;
    br.wi = to_local(f, wi);
    br.wo = to_local(f, wo);
    br.measure = kMeasureSolidAngle;
    br.uv = V2{u, v};  // (sane_uv changes an image texture's uv only, and that BSDF has a zero row)
    return bsdf_grad_row(b, br, g_r, g_g, g_b, g_p, t);
}

}  // namespace nori
