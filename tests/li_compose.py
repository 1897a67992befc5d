"""tests/shading_compose.py generalised from the renderer's camera rays to rays the caller gives:
direct_ems / direct_mats / direct_mis composed in numpy float32 from the public ray and shading
queries of a GpuRenderer, following OneBounce::Li (csrc/onebounce.h) line by line -- the same
draws, the same order of the adds and products.  The first segment is the given ray with its own
mint and maxt; the direction is used as given.  For tests/test_gpu_li.py; no assertions here.

Every operation done on the host is a single IEEE float32 +, * or / (numpy keeps float32 arrays in
float32), which the device code performs with contraction off and correctly rounded division, so
the composed radiance is expected to equal nori_gpu_li's bit for bit."""
import numpy as np

from shading_compose import EPS, _rays, f32


def draws_needed(scene, integrator):
    """Draws of Li per ray: one next2D per emitter (ems, mis), one for the BSDF sample (mats, mis)."""
    n_em = len(scene.emitters())
    return (2 * n_em if integrator in ("direct_ems", "direct_mis") else 0) + \
        (2 if integrator in ("direct_mats", "direct_mis") else 0)


def direct_li_rays(r, scene, integrator, rays, U):
    """(L (n, 3) float32, hit mask (n,)): Li of `integrator` along rays (n, 8) = o, mint, d, maxt,
    ray i drawing U[i] (n, draws_needed) -- the draws of its stream from the integrator's first on."""
    n = rays.shape[0]
    ems = integrator in ("direct_ems", "direct_mis")
    mats = integrator in ("direct_mats", "direct_mis")
    mis = integrator == "direct_mis"
    n_em = len(scene.emitters())
    has_emitter = np.array([sh.emitter >= 0 for sh in scene.shapes()], bool)
    rays = np.ascontiguousarray(rays, f32)
    assert U.shape == (n, draws_needed(scene, integrator))
    surf_all = r.query(rays)["surf"]
    hit = surf_all["shape"] >= 0
    L = np.zeros((n, 3), f32)  # a miss: Li returns 0
    idx = np.flatnonzero(hit)
    if idx.size == 0:
        return L, hit
    surf = np.ascontiguousarray(surf_all[idx])
    o = np.ascontiguousarray(rays[idx, 0:3])
    view = np.ascontiguousarray(-rays[idx, 4:7])  # -d
    p = np.ascontiguousarray(surf["p"])
    U = np.ascontiguousarray(U[idx], f32)
    with np.errstate(all="ignore"):
        color = r.emitter_eval(surf, o)[:, 0:3].copy()  # emission(hs, o)
        col = 0
        if ems:
            for i in range(n_em):
                s2 = np.ascontiguousarray(U[:, col:col + 2])
                col += 2
                es = r.emitter_sample(p, s2, emitter=i)
                wi, maxt, Li, pdf_em = np.ascontiguousarray(es[:, 0:3]), es[:, 3], es[:, 4:7], es[:, 7]
                occluded = r.query(_rays(p, wi, maxt), any_hit=True)["hits"]["prim"] >= 0
                be = r.bsdf_eval(surf, view, wi)
                f, pdf_mat, cos = be[:, 0:3], be[:, 3], be[:, 4]  # cos: to_local(ne.wi).z
                if mis:
                    s = pdf_mat + pdf_em
                    w_em = np.where(s > 0, pdf_em / s, pdf_em).astype(f32)
                    term = ((f * w_em[:, None]) * Li) * cos[:, None]
                else:
                    term = (f * cos[:, None]) * Li
                color = np.where(occluded[:, None], color, color + term).astype(f32)
        if mats:
            s2 = np.ascontiguousarray(U[:, col:col + 2])
            bs = r.bsdf_sample(surf, view, s2)
            d2, pdf_mat, w = np.ascontiguousarray(bs[:, 0:3]), bs[:, 3], bs[:, 4:7]
            go = ~(w == 0).all(1)  # deviation D1: a zero weight ends the sample
            j = np.flatnonzero(go)
            if j.size:
                nh = r.query(_rays(p[j], d2[j], f32(np.inf)))["surf"]
                lit = nh["shape"] >= 0
                lit[lit] = has_emitter[nh["shape"][lit]]
                ee = r.emitter_eval(nh, p[j])
                Le, pdf_em = ee[:, 0:3], ee[:, 3]
                if mis:
                    s = pdf_mat[j] + pdf_em
                    w_mat = np.where(s > 0, pdf_mat[j] / s, f32(0)).astype(f32)
                    add = (w[j] * w_mat[:, None]) * Le
                else:
                    add = w[j] * Le
                cj = color[j]
                color[j] = np.where(lit[:, None], cj + add, cj)
    L[idx] = color
    return L, hit


__all__ = ["EPS", "direct_li_rays", "draws_needed"]
