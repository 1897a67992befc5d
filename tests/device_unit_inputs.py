"""Input sets of the device unit tests, shared by tests/test_bsdf_ref64.py (the
oracle against the float64 model, on the CPU) and
tests/test_gpu_device_units.py (the device against the oracle), and the
tolerances the first measures for the second.  No assertions here."""
import functools
import xml.etree.ElementTree as ET

import numpy as np

import bsdf_ref64
import nori_amd
from conftest import scene_path

A = nori_amd._abi
f32 = np.float32
ONE_M = f32(1) - f32(2.0 ** -24)  # the largest float below 1: pcg_float's maximum

# Measured by tests/test_bsdf_ref64.py on these input sets (the oracle against
# the model), asserted there with a 2x margin.
# E_DIR: largest |difference| of a component of a sampled direction.
E_DIR = 4.62e-7
# E_VAL: largest relative difference (rel_diff below) of eval, pdf and weight
# luminance on the well-conditioned subset (wi.z, wo.z, half-vector z all >=
# WELL), per configuration (one E_val for all would be their maximum).  The
# float32 formulas of the narrow lobes (alpha = 1e-3, Disney roughness <= 0.02)
# are ill-conditioned at their peak whatever the directions' z -- 1 - z*z of a
# float32 half-vector within 1e-6 of the pole, (a2 - 1) + 1/c^2 of GTR2 -- so
# there the oracle is 30 % off the float64 value, and so is anything that
# restates the reference in float32.
E_VAL = {"diffuse": 9.97e-08, "diffuse-checker": 9.97e-08, "microfacet-chi2-0": 2.87e-05, "microfacet-chi2-1": 2.49e-06,
         "microfacet-chi2-2": 1.08e-06, "microfacet-ks1": 1e-05, "microfacet-ks0": 9.97e-08,
         "microfacet-alpha1e-3": 0.317, "disney-m0.0-r0.0": 0.15, "disney-m0.0-r0.02": 0.15,
         "disney-m0.0-r0.5": 4.04e-06, "disney-m0.0-r1.0": 4.79e-07, "disney-m0.5-r0.0": 0.309,
         "disney-m0.5-r0.02": 0.309, "disney-m0.5-r0.5": 6.75e-06, "disney-m0.5-r1.0": 4.76e-07,
         "disney-m1.0-r0.0": 0.309, "disney-m1.0-r0.02": 0.309, "disney-m1.0-r0.5": 7.42e-06,
         "disney-m1.0-r1.0": 4.59e-07}
WELL = 0.05
# Values this small are compared absolutely: expf(-tan^2 / alpha^2) underflows
# float32 below 2^-126 (flushed or denormal: an absolute error of up to 2^-126
# in that factor), and the factors that multiply it, ks F G / (pi alpha^2
# cos^4 4 cos cos), stay below 1 / (pi 1e-6 0.05^4 4 0.05^2) < 2^43 on the
# well-conditioned subset.
TINY = 2.0 ** -83


def rel_diff(a, b):
    """|a - b| / max(|b|, TINY), 0 where a == b (infinities included)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(all="ignore"):
        r = np.abs(a - b) / np.maximum(np.abs(b), TINY)
    return np.where(a == b, 0.0, r)


def _desc(type_, **kw):
    d = A.BsdfDesc()
    d.type = type_
    d.albedo[:] = [0.5, 0.5, 0.5]
    d.int_ior, d.ext_ior = 1.5046, 1.000277
    d.tex_scale[:] = [1, 1]
    d.albedo_image = -1
    for k, v in kw.items():
        if isinstance(v, (list, tuple)):
            getattr(d, k)[:] = v
        else:
            setattr(d, k, v)
    return d


def chi2_microfacets():
    """The three BSDFs of scenes/pa3/tests/chi2test-microfacet.xml."""
    root = ET.parse(scene_path("pa3", "tests", "chi2test-microfacet.xml")).getroot()
    out = []
    for b in root.iter("bsdf"):
        p = {q.get("name"): q.get("value") for q in b}
        out.append(_desc(A.BSDF_MICROFACET, alpha=float(p["alpha"]), int_ior=float(p["intIOR"]),
                         ext_ior=float(p["extIOR"]), kd=[float(x) for x in p["kd"].replace(",", " ").split()]))
    return out


DIELECTRIC_IORS = [(1.5046, 1.000277), (1.33, 1.0), (1.0, 1.5), (1.5, 1.5)]  # (int, ext)


@functools.lru_cache(None)
def configs():
    """[(name, desc)] of section b."""
    out = [("diffuse", _desc(A.BSDF_DIFFUSE, albedo=[0.5, 0.3, 0.7])),
           ("diffuse-checker", _desc(A.BSDF_DIFFUSE, albedo=[0.9, 0.2, 0.4], albedo_texture=A.TEXTURE_CHECKERBOARD,
                                     tex_value2=[0.1, 0.6, 0.3], tex_delta=[0.25, -0.5], tex_scale=[0.1, 0.37])),
           ("mirror", _desc(A.BSDF_MIRROR))]
    for i, e in DIELECTRIC_IORS:
        out.append((f"dielectric-{i}-{e}", _desc(A.BSDF_DIELECTRIC, int_ior=i, ext_ior=e)))
    for k, d in enumerate(chi2_microfacets()):
        out.append((f"microfacet-chi2-{k}", d))
    out.append(("microfacet-ks1", _desc(A.BSDF_MICROFACET, alpha=0.3, kd=[0, 0, 0])))
    out.append(("microfacet-ks0", _desc(A.BSDF_MICROFACET, alpha=0.3, kd=[0.2, 1.0, 0.5])))
    out.append(("microfacet-alpha1e-3", _desc(A.BSDF_MICROFACET, alpha=1e-3, kd=[0.2, 0.1, 0.3])))
    for m in (0.0, 0.5, 1.0):
        for r in (0.0, 0.02, 0.5, 1.0):
            out.append((f"disney-m{m}-r{r}", _desc(A.BSDF_DISNEY, base_color=[0.8, 0.4, 0.2], metallic=m, roughness=r,
                                                   specular=0.5, sheen=0.7, sheen_tint=0.3, specular_tint=0.6)))
    return out


def exact(desc):
    """The sampled path has no transcendental: bit-equal to the oracle."""
    return desc.type in (A.BSDF_MIRROR, A.BSDF_DIELECTRIC)


def exact_eval(desc):
    """eval / pdf have no transcendental (microfacet has expf)."""
    return desc.type != A.BSDF_MICROFACET


def basic(desc):
    """In the FULL = false plugin set."""
    return desc.type in (A.BSDF_MIRROR, A.BSDF_DIELECTRIC) or (
        desc.type == A.BSDF_DIFFUSE and desc.albedo_texture == A.TEXTURE_CONSTANT)


WI_Z = [1.0, float(ONE_M), 0.5, 0.05, 1e-3, 1e-7, 0.0, -0.0, -0.5]
_UV = np.array([[0, 0], [0.3, 0.7], [-0.3, 0.2], [-7.25, -3.5], [1e4, -1e4], [9999.99, 0.05], [-0.05, 1234.5],
                [0.25, 0.185], [0.35, -0.185], [2.5e-2, 3.7e-1]], f32)


def critical_cosines(desc):
    """wi.z at the critical angle on the total-reflection side and the floats around it."""
    i, e = f32(desc.int_ior), f32(desc.ext_ior)
    if i == e:
        return []
    lo, hi = (e, i) if i > e else (i, e)
    c = f32(np.sqrt(1.0 - (float(lo) / float(hi)) ** 2))
    sign = -1.0 if i > e else 1.0  # int > ext: total reflection from inside, wi.z < 0
    out = [c]
    for _ in range(2):
        out = [np.nextafter(out[0], f32(0))] + out + [np.nextafter(out[-1], f32(2))]
    return [float(sign * x) for x in out]


def _dir(z, phi):
    z = np.asarray(z, f32)
    with np.errstate(invalid="ignore"):
        s = np.sqrt(np.maximum(f32(0), f32(1) - z * z)).astype(f32)
    return np.stack([s * f32(np.cos(phi)), s * f32(np.sin(phi)), z], -1).astype(f32)


def sample_inputs(desc):
    """(wi (n, 3), u (n, 2), uv (n, 2)) of section b for one configuration: the
    listed wi.z (and the dielectric's critical angles), u on a grid with the
    end points 0, 2^-24, 1 - 2^-24, u.x exactly ks / metallic / the Fresnel
    value of the row (and its neighbours), plus 2^18 seeded random rows (so the few grid rows that land on the
    horizon, u.x = 0 of the cosine lobe, stay a small share)."""
    zs = list(WI_Z) + (critical_cosines(desc) if desc.type == A.BSDF_DIELECTRIC else [])
    ux = [0.0, 2.0 ** -24, float(ONE_M)] + [(k + 0.5) / 24 for k in range(24)] + [0.25, 0.5, 0.75]
    ks, _ = bsdf_ref64.derived(desc)
    for v in (ks, f32(desc.metallic)):
        v = f32(v)
        ux += [float(v), float(np.nextafter(v, f32(0))), float(np.nextafter(v, f32(1)))]
    uy = [0.0, 2.0 ** -24, float(ONE_M), 0.25, 0.5, 0.75] + [(k + 0.37) / 10 for k in range(10)]
    rows_wi, rows_u = [], []
    for k, z in enumerate(zs):
        wi = _dir(f32(z), 0.7 + 1.3 * k)
        uxs = list(ux)
        if desc.type in (A.BSDF_DIELECTRIC, A.BSDF_MICROFACET):
            F = bsdf_ref64.fresnel32(np.array([wi[2]], f32), desc.ext_ior, desc.int_ior)[0]
            uxs += [float(F), float(np.nextafter(F, f32(0))), float(np.nextafter(F, f32(1)))]
        uxs = sorted({min(max(x, 0.0), float(ONE_M)) for x in uxs})
        g = np.array([(a, b) for a in uxs for b in uy], f32)
        rows_u.append(g)
        rows_wi.append(np.tile(wi, (g.shape[0], 1)))
    rng = np.random.default_rng(77)
    n = 1 << 18
    rows_u.append(rng.random((n, 2), dtype=f32))
    z, ph = rng.random(n, dtype=f32), rng.random(n) * 2 * np.pi
    sn = np.sqrt(np.maximum(f32(0), f32(1) - z * z))
    rows_wi.append(np.stack([sn * np.cos(ph).astype(f32), sn * np.sin(ph).astype(f32), z], 1))
    wi, u = np.concatenate(rows_wi).astype(f32), np.concatenate(rows_u).astype(f32)
    uv = _UV[np.arange(wi.shape[0]) % _UV.shape[0]]
    return wi, u, np.ascontiguousarray(uv)


def eval_inputs(desc, wo_sampled):
    """(wi, wo, uv) for eval / pdf: every sample row with the direction the
    oracle sampled there (where the lobe is), and every listed wi against a
    fixed set of directions (both hemispheres, the horizon, the pole)."""
    wi_s, _, uv_s = sample_inputs(desc)
    zs = WI_Z + [0.999, 0.9, 0.7, 0.3, 0.1, 0.02, -1e-3, -1.0]
    wo_g = np.concatenate([_dir(np.array(zs, f32), p) for p in (0.0, 0.9, 2.5, 4.0, 5.5)])
    wi_g = np.concatenate([_dir(f32(z), 0.7 + 1.3 * k)[None] for k, z in enumerate(WI_Z)])
    a = np.repeat(wi_g, wo_g.shape[0], 0)
    b = np.tile(wo_g, (wi_g.shape[0], 1))
    wi = np.concatenate([wi_s, a]).astype(f32)
    wo = np.concatenate([np.ascontiguousarray(wo_sampled, f32).reshape(-1, 3), b]).astype(f32)
    uv = np.concatenate([uv_s, _UV[np.arange(a.shape[0]) % _UV.shape[0]]]).astype(f32)
    return wi, wo, uv


def well_conditioned(wi, wo):
    """wi.z, wo.z and the half-vector's z all >= WELL (float64)."""
    wi, wo = np.asarray(wi, np.float64), np.asarray(wo, np.float64)
    h = wi + wo
    with np.errstate(all="ignore"):
        hz = h[:, 2] / np.sqrt((h * h).sum(1))
    return (wi[:, 2] >= WELL) & (wo[:, 2] >= WELL) & (hz >= WELL)


# ---------------------------------------------------------------- glass chain
GLASS_SPHERES = [("cbox", (0.4458, 0.3321, 0.3767), 0.3263), ("tiny-far", (100.0, -50.0, 30.0), 0.01),
                 ("large", (0.0, 0.0, 0.0), 50.0)]
GLASS_BETA_X = [1.0, 0.6, 0.25, np.inf, np.nan]


# Incidence cosines at which the chord is about as long as the adaptive epsilon
# (chord = 2 r cos, epsilon = 1e-4 max(1, |o|_max)): extra lanes there see the
# next chord exist for one route's arithmetic and vanish for the other's, if
# the two ever differ.
GLASS_EDGE_COS = {"cbox": (0.0, 3.1e-4), "tiny-far": (0.498, 0.502), "large": (0.0, 1e-4)}


def glass_inputs(center, radius, n, seed, cos_lo=0.0, cos_hi=1.0):
    """n lanes on the sphere: start points uniform on it (float32), inward
    directions with an incidence cosine uniform in (cos_lo, cos_hi), beta.x cycling."""
    rng = np.random.default_rng(seed)
    z = 1 - 2 * rng.random(n)
    ph = 2 * np.pi * rng.random(n)
    s = np.sqrt(1 - z * z)
    nrm = np.stack([s * np.cos(ph), s * np.sin(ph), z], 1)
    o = (np.array(center, f32) + f32(radius) * nrm.astype(f32)).astype(f32)
    c = cos_lo + (cos_hi - cos_lo) * np.clip(rng.random(n), 1e-9, 1 - 1e-9)
    # a tangent of the normal, rotated by a random angle
    t = np.cross(nrm, np.where(np.abs(nrm[:, :1]) < 0.9, [[1.0, 0, 0]], [[0, 1.0, 0]]))
    t /= np.linalg.norm(t, axis=1)[:, None]
    b = np.cross(nrm, t)
    ps = 2 * np.pi * rng.random(n)
    tang = t * np.cos(ps)[:, None] + b * np.sin(ps)[:, None]
    d = (-c[:, None] * nrm + np.sqrt(1 - c * c)[:, None] * tang).astype(f32)
    beta = np.empty((n, 3), f32)
    beta[:, 0] = np.array(GLASS_BETA_X, f32)[np.arange(n) % len(GLASS_BETA_X)]
    beta[:, 1] = 0.8
    beta[:, 2] = 0.5
    return o, d, beta


# ---------------------------------------------------------------- fast math
def math_inputs():
    """About 2^21 floats: every exponent from 2^-149 to 2^127 with 4096
    mantissas each (all-zeros and all-ones included; the 23 denormal binades
    have fewer distinct values), their negatives subsampled, +-0, +-inf, NaN,
    and the switch points 2^-96, 2^96, 2^-125, 2^125 with their neighbours."""
    rng = np.random.default_rng(5)
    fixed = np.array([0, 0x7FFFFF, 1, 0x400000, 0x3FFFFF, 0x7FFFFE], np.uint32)
    drawn = np.setdiff1d(rng.integers(0, 1 << 23, 5000).astype(np.uint32), fixed)
    man = np.concatenate([fixed, rng.permutation(drawn)[:4096 - fixed.size]]).astype(np.uint32)
    exps = np.arange(0, 255, dtype=np.uint32)  # 0: denormals (and zero)
    pos = ((exps[:, None] << 23) | man[None, :]).ravel().astype(np.uint32)
    den = np.concatenate([(np.uint32(1) << np.arange(23, dtype=np.uint32)),
                          (np.uint32(1) << np.arange(1, 24, dtype=np.uint32)) - np.uint32(1)]).astype(np.uint32)
    sw = []
    for e in (-96, 96, -125, 125):
        b = np.array([2.0 ** e], f32).view(np.uint32)[0]
        sw += [b - 1, b, b + 1]
    special = np.array([0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001], np.uint32)
    p = np.concatenate([pos, den, np.array(sw, np.uint32)]).astype(np.uint32)
    bits = np.concatenate([p, p | np.uint32(0x80000000), special]).astype(np.uint32)
    return bits.view(f32)


def vector_inputs():
    """3-vectors for normalize / frame_from: axis-aligned, |x| == |y|, denormal
    components, huge and tiny lengths, and seeded random ones."""
    rng = np.random.default_rng(6)
    t = f32(1e-40)  # denormal
    v = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1], [0, 0, 0], [1, 1, 0], [1, -1, 0],
         [-0.5, 0.5, 0.7], [0.6, 0.6, -0.52915], [t, 0, 0], [0, t, 0], [t, t, 1], [t, 1, t], [1, t, t], [t, t, t],
         [1e19, 1e19, 1e19], [1e-19, 1e-19, 1e-19], [3e18, 0, 4e18], [1e-30, 1e-25, 0], [2.0 ** -48, 0, 2.0 ** -48],
         [2.0 ** 48, 0, 2.0 ** 48], [np.inf, 0, 0], [np.nan, 1, 0], [0.0, -0.0, 1.0]]
    a = rng.standard_normal((1 << 16, 3)).astype(f32)
    unit = bsdf_ref64.normalize32(a.copy())
    tie = a.copy()
    tie[:, 1] = tie[:, 0] * np.where(rng.random(tie.shape[0]) < 0.5, -1, 1).astype(f32)
    scaled = a * (f32(2) ** rng.integers(-70, 70, (a.shape[0], 1)).astype(f32))
    return np.concatenate([np.array(v, f32), a, unit, tie, scaled]).astype(f32)


def cosine_inputs(desc_iors):
    """cosThetaI for fresnel: 0, +-1, a dense sweep, the critical angle and its neighbours."""
    ext, itr = desc_iors
    d = _desc(A.BSDF_DIELECTRIC, int_ior=itr, ext_ior=ext)
    crit = critical_cosines(d)
    rng = np.random.default_rng(7)
    c = np.concatenate([[0.0, -0.0, 1.0, -1.0, float(ONE_M), -float(ONE_M), 1e-7, -1e-7, 1e-38, 2.0, -2.0, np.nan],
                        crit, [-x for x in crit], np.linspace(-1, 1, 1 << 16), rng.random(1 << 16) * 2 - 1])
    if crit:  # a dense sweep across the critical angle
        c0 = f32(crit[2])
        k = np.arange(-2000, 2001)
        sweep = (np.array([c0], f32).view(np.int32)[0] + k).astype(np.int32).view(f32)
        c = np.concatenate([c, sweep])
    return c.astype(f32)
