// onebounce.h -- OneBounce<STACK>: a thread that traces and shades its own
// rays start to end, for k_direct (kernels.hip) and k_features
// (kernels_features.hip).  Device code for the .hip units.
#pragma once
#include "shading.h"
#include "traverse.h"

namespace nori {

// ------------------------------------------------------------------ one-bounce integrators
// normals (normals.cpp:16-24), av (averagevisibility.cpp:16-27), direct
// (direct.cpp:17-45), direct_ems (direct_ems.cpp:17-51), direct_mats
// (direct_mats.cpp:17-44), direct_mis (direct_mis.cpp:17-85).  They trace a
// fixed, small number of rays per camera sample (1 + lights + 1 at most), so
// there is no path state to keep: one thread runs one sample start to end and
// writes its record; k_splat filters the records as for the path integrators.
template <int STACK>
struct OneBounce {
    const DevScene &S;
    uint32_t *stk;
    uint32_t rc = 0, rs = 0;  // rays traced: closest, shadow
    ND bool closest(V3 o, V3 d, float mint, float maxt, SurfHit &hs, float &t) {  // t: the hit distance
        ++rc;
        TRay r{o, d, V3{0, 0, 0}, mint, maxt};
        float u, v;
        uint32_t p;
        if (!traverse<STACK, false>(S, r, stk, t, p, u, v)) return false;
        hs = surface(S, p, t, u, v, o, d);
        return true;
    }
    ND bool closest(V3 o, V3 d, float mint, float maxt, SurfHit &hs) {
        float t;
        return closest(o, d, mint, maxt, hs, t);
    }
    ND bool occluded(V3 o, V3 d, float maxt) {
        ++rs;
        TRay r{o, d, V3{0, 0, 0}, kEps, maxt};
        float t, u, v;
        uint32_t p;
        return traverse<STACK, true>(S, r, stk, t, p, u, v);
    }
    // emission of the hit surface seen from `from` (EmitterQueryRecord(from, its.p, n))
    ND V3 emission(const SurfHit &hs, V3 from) {
        const DevShape &sh = S.shapes[hs.shape];
        if (sh.emitter < 0) return V3{0, 0, 0};
        return emitter_eval(S, S.emitters[sh.emitter], hs.sh.n, normalize(hs.p - from));
    }
    // PhotonMapper::Li (photonmapper.cpp:119-196): emission at every hit, the
    // photon density estimate at the first diffuse surface, Russian roulette
    // and BSDF sampling at the others.  The kd-tree search (kdtree.h:260-316:
    // every photon with |x - p|^2 < r^2) is a 27-cell lookup in a hash grid of
    // cell size r: a bucket may hold photons of colliding cells, so each
    // photon is counted only from its own cell.
    ND V3 Li_pmap(Pcg &rng, V3 o, V3 d, float mint, float maxt) {
        V3 color{0, 0, 0}, att{1, 1, 1};
        for (;;) {
            SurfHit hs;
            if (!closest(o, d, mint, maxt, hs)) return color;
            color = color + att * emission(hs, o);
            const DevBsdf &B = S.bsdfs[S.shapes[hs.shape].bsdf];
            if (B.type == NORI_BSDF_DIFFUSE) {  // Diffuse::isDiffuse (diffuse.cpp:122)
                const float ic = S.ph_inv_cell;
                const int cx = (int)floorf(hs.p.x * ic), cy = (int)floorf(hs.p.y * ic), cz = (int)floorf(hs.p.z * ic);
                const V3 wi = to_local(hs.sh, -d);
                V3 pc{0, 0, 0};
                for (int dz = -1; dz <= 1; ++dz)
                    for (int dy = -1; dy <= 1; ++dy)
                        for (int dx = -1; dx <= 1; ++dx) {
                            const int gx = cx + dx, gy = cy + dy, gz = cz + dz;
                            const uint32_t h = photon_cell_hash(gx, gy, gz) & S.ph_mask;
                            const uint32_t j1 = S.ph_start[h + 1];
#ifndef NORI_PMAP_BATCH
#define NORI_PMAP_BATCH 4  // candidate photons whose positions are loaded together
#endif
                            for (uint32_t j0 = S.ph_start[h]; j0 < j1; j0 += NORI_PMAP_BATCH) {
                              float4 qb[NORI_PMAP_BATCH];
#pragma unroll
                              for (int u = 0; u < NORI_PMAP_BATCH; ++u)
                                  qb[u] = j0 + u < j1 ? gld(S.ph + j0 + u) : make_float4(0, 0, 0, 0);
#pragma unroll
                              for (int u = 0; u < NORI_PMAP_BATCH; ++u) {
                                const uint32_t j = j0 + u;
                                if (j >= j1) break;
                                const float4 pp = qb[u];
                                const V3 dd = ld3(pp) - hs.p;
                                if (!(dot(dd, dd) < S.ph_r2)) continue;
                                // own cell only (a bucket may hold colliding cells)
                                if ((int)floorf(pp.x * ic) != gx || (int)floorf(pp.y * ic) != gy ||
                                    (int)floorf(pp.z * ic) != gz)
                                    continue;
                                BRec br;
                                br.wi = wi;
                                // PhotonData::getDirection / getPower (photon.h:44-55)
                                const uint32_t dir = __float_as_uint(pp.w), rgbe = S.ph_rgbe[j];
                                const float *T = S.ph_tab;
                                const float st = T[768 + (dir & 255u)];
                                const V3 wd{T[(dir >> 8) & 255u] * st, T[256 + ((dir >> 8) & 255u)] * st,
                                            T[512 + (dir & 255u)]};
                                const float sc = T[1024 + (rgbe >> 24)];
                                const V3 pw{(float)(rgbe & 255u) * sc, (float)((rgbe >> 8) & 255u) * sc,
                                            (float)((rgbe >> 16) & 255u) * sc};
                                br.wo = to_local(hs.sh, wd);
                                br.measure = kMeasureSolidAngle;
                                br.uv = hs.uv;
                                pc = pc + bsdf_eval(B, br) * pw;
                              }
                            }
                        }
                return color + att * ((pc * kInvPi) / S.ph_norm);
            }
            const float q = smin(att.x, 0.99f);
            if (next1D(rng) > q) return color;
            att = att / q;
            BRec br;
            br.wi = to_local(hs.sh, -d);
            br.wo = V3{0, 0, 1};
            br.measure = kMeasureUnknown;
            br.uv = hs.uv;
            const V3 w = bsdf_sample(B, br, next2D(rng));
            if (is_zero(w)) return color;  // deviation D1
            att = att * w;
            o = hs.p;
            d = to_world(hs.sh, br.wo);
            mint = kEps;
            maxt = INF_F;
        }
    }
    template <int INTEG>
    ND V3 Li(Pcg &rng, V3 o, V3 d, float mint, float maxt) {
        if constexpr (INTEG == NORI_INTEGRATOR_PHOTONMAPPER) return Li_pmap(rng, o, d, mint, maxt);
        SurfHit hs;
        if (!closest(o, d, mint, maxt, hs)) return INTEG == NORI_INTEGRATOR_AV ? V3{1, 1, 1} : V3{0, 0, 0};
        if (INTEG == NORI_INTEGRATOR_NORMALS) return V3{fabsf(hs.sh.n.x), fabsf(hs.sh.n.y), fabsf(hs.sh.n.z)};
        if (INTEG == NORI_INTEGRATOR_AV) {
            // Warp::sampleUniformHemisphere (warp.cpp:25-42): rejection in the cube
            V3 w;
            do {
                w.x = 1.f - 2.f * next1D(rng);
                w.y = 1.f - 2.f * next1D(rng);
                w.z = 1.f - 2.f * next1D(rng);
            } while (dot(w, w) > 1.f);
            if (dot(w, hs.sh.n) < 0.f) w = -w;
            w = w / norm(w);
            ++rs;
            TRay r{hs.p, w, V3{0, 0, 0}, kEps, S.av_length};
            float t, u, v;
            uint32_t p;
            return traverse<STACK, true>(S, r, stk, t, p, u, v) ? V3{0, 0, 0} : V3{1, 1, 1};
        }
        const DevBsdf &B = S.bsdfs[S.shapes[hs.shape].bsdf];
        V3 color = INTEG == NORI_INTEGRATOR_DIRECT ? V3{0, 0, 0} : emission(hs, o);
        if (INTEG == NORI_INTEGRATOR_DIRECT || INTEG == NORI_INTEGRATOR_DIRECT_EMS ||
            INTEG == NORI_INTEGRATOR_DIRECT_MIS) {
            // every light, one shadow ray each; `direct` passes an unset sample
            // (its lights ignore it): (0, 0) here, nothing drawn
            for (uint32_t i = 0; i < S.num_emitters; ++i) {
                const V2 s2 = INTEG == NORI_INTEGRATOR_DIRECT ? V2{0, 0} : next2D(rng);
                const NeeSample ne = emitter_sample_one(S, S.emitters[i], hs.p, s2);
                if (occluded(hs.p, ne.wi, ne.maxt)) continue;
                const V3 wi = to_local(hs.sh, ne.wi), dv = to_local(hs.sh, -d);
                BRec br;
                br.measure = kMeasureSolidAngle;
                br.uv = hs.uv;
                br.wi = INTEG == NORI_INTEGRATOR_DIRECT ? wi : dv;  // direct.cpp builds (light, view)
                br.wo = INTEG == NORI_INTEGRATOR_DIRECT ? dv : wi;
                const V3 f = bsdf_eval(B, br);
                if (INTEG == NORI_INTEGRATOR_DIRECT_MIS) {
                    const float pdf_mat = bsdf_pdf(B, br);
                    const float w_em = pdf_mat + ne.pdf_em > 0.f ? ne.pdf_em / (pdf_mat + ne.pdf_em) : ne.pdf_em;
                    color = color + ((f * w_em) * ne.Li) * wi.z;
                } else {
                    color = color + (f * wi.z) * ne.Li;
                }
            }
        }
        if (INTEG == NORI_INTEGRATOR_DIRECT_MATS || INTEG == NORI_INTEGRATOR_DIRECT_MIS) {
            BRec br;
            br.wi = to_local(hs.sh, -d);
            br.wo = V3{0, 0, 1};
            br.measure = kMeasureUnknown;
            br.uv = hs.uv;
            const V3 w = bsdf_sample(B, br, next2D(rng));
            if (is_zero(w)) return color;  // deviation D1: no ray along an unset direction
            const float pdf_mat = INTEG == NORI_INTEGRATOR_DIRECT_MIS ? bsdf_pdf(B, br) : 0.0f;
            SurfHit nh;
            if (!closest(hs.p, to_world(hs.sh, br.wo), kEps, INF_F, nh)) return color;
            const DevShape &ns = S.shapes[nh.shape];
            if (ns.emitter < 0) return color;
            const DevEmitter &E = S.emitters[ns.emitter];
            const V3 wl = normalize(nh.p - hs.p);
            const V3 Le = emitter_eval(S, E, nh.sh.n, wl);
            if (INTEG == NORI_INTEGRATOR_DIRECT_MATS) return color + w * Le;
            const float pdf_em = emitter_pdf(S, E, nh.sh.n, wl);
            const float w_mat = pdf_mat + pdf_em > 0.f ? pdf_mat / (pdf_mat + pdf_em) : 0.0f;
            return color + (w * w_mat) * Le;
        }
        return color;
    }
};

}  // namespace nori
