"""The direct_ems / direct_mats / direct_mis integrators composed in numpy float32 from the public
ray and shading queries of a GpuRenderer, following OneBounce::Li (csrc/onebounce.h) line by line:
the same draws, the same order of the adds and products.  Shared by the tests of the shading
queries; no assertions here.

Every operation done on the host is a single IEEE float32 +, * or / (numpy keeps float32 arrays in
float32), which the device code performs with contraction off and correctly rounded division, so
the composed radiance is expected to equal the built-in integrator's bit for bit."""
import numpy as np

f32 = np.float32
EPS = f32(1e-4)  # NORI_EPSILON
# the scenes of the composition test (scenes/project/spotlight/sphere-texture.xml uses the `direct`
# integrator, none of ems / mats / mis) and the passes it composes
DIRECT_SCENES = [("pa3", "sphere", "sphere_ems.xml"), ("pa3", "sphere", "point_ems.xml"),
                 ("pa3", "odyssey", "odyssey_ems.xml"), ("pa3", "odyssey", "odyssey_mats.xml"),
                 ("pa3", "odyssey", "odyssey_mis.xml"), ("pa3", "veach_mi", "veach_mis.xml")]
PASSES = (0, 3)


def envmap_direct_mis(outdir):
    """The envmap scene of tests/test_gpu_parity.py with direct_mis at 32 x 32 (a 32 x 64 sky)."""
    import synth

    return synth.envmap_scene(outdir, 32, 32, 1, integrator="direct_mis", rows=32, cols=64)


def _rays(o, d, maxt):
    r = np.zeros((o.shape[0], 8), f32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, EPS, d, maxt
    return r


def direct_li(r, scene, integrator, k, seed=0):
    """(L (H, W, 3) float32, hit mask (H, W)) of the samples of pass k: Li of `integrator`
    ("direct_ems", "direct_mats", "direct_mis") for every pixel's camera ray."""
    H, W = scene.height, scene.width
    N = H * W
    ems = integrator in ("direct_ems", "direct_mis")
    mats = integrator in ("direct_mats", "direct_mis")
    mis = integrator == "direct_mis"
    n_em = len(scene.emitters())
    has_emitter = np.array([sh.emitter >= 0 for sh in scene.shapes()], bool)
    rays = r.camera_rays(passes=1, pass_begin=k, seed=seed).reshape(N, 8)
    ndraw = (2 * n_em if ems else 0) + (2 if mats else 0)
    U = r.sample_uniforms(4, ndraw, passes=1, pass_begin=k, seed=seed).reshape(N, ndraw)
    surf_all = r.query(rays)["surf"]
    hit = surf_all["shape"] >= 0
    L = np.zeros((N, 3), f32)  # a miss: Li returns 0
    idx = np.flatnonzero(hit)
    if idx.size == 0:
        return L.reshape(H, W, 3), hit.reshape(H, W)
    surf = np.ascontiguousarray(surf_all[idx])
    o = np.ascontiguousarray(rays[idx, 0:3])
    view = np.ascontiguousarray(-rays[idx, 4:7])  # -d
    p = np.ascontiguousarray(surf["p"])
    U = U[idx]
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
    return L.reshape(H, W, 3), hit.reshape(H, W)
