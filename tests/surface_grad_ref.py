"""Shared by test_surface_grad.py (CPU) and test_gpu_surface_grad.py (GPU): an independent numpy
restatement of the hit record's adjoint in the vertices (nori_scene_surface_grad in
include/nori_gpu.h), written from the header alone.

Two halves.  forward64: the record functions p(P), t(P), ng(P), ns(P, Nrm) at fixed (prim, u, v)
and fixed ray in float64 -- what the adjoint is the adjoint OF; finite differences of it check the
terms.  terms32: the 18 per-hit terms in float32, every operation in the header's order (numpy
float32 arithmetic is IEEE single, unfused), which the library must equal bit for bit.

Conventions of the forward, the header's: barycentrics held for p and ns, the ray held for
t = N.(p0 - o) / (N.d); a miss, a sphere hit and a triangle with |N| = 0 or N.d = 0 are constants
(no derivative), ns of a normal-mapped shape is held (the header leaves that derivative out), ns of
a mesh without normals is ng, and |M| = 0 holds ns alone.
"""
import os

import numpy as np

import nori_amd
from nori_amd import _abi

f32 = np.float32


def smooth_scene_xml(outdir):
    """scenes/pa1/sphere.obj (5,120 triangles with vn lines: smooth vertex normals) alone, scaled
    and moved as in scenes/pa1/sphere-mesh.xml."""
    from conftest import scene_path

    os.makedirs(outdir, exist_ok=True)
    xml = os.path.join(str(outdir), "smooth_sphere.xml")
    with open(xml, "w") as f:
        f.write(f"""<?xml version='1.0' encoding='utf-8'?>
<scene>
  <sampler type="independent"><integer name="sampleCount" value="1"/></sampler>
  <integrator type="normals"/>
  <camera type="perspective">
    <transform name="toWorld"><lookat target="0,0,1" origin="5,5,1" up="0,0,1"/></transform>
    <float name="fov" value="40"/>
    <integer name="width" value="32"/><integer name="height" value="32"/>
  </camera>
  <mesh type="obj">
    <string name="filename" value="{scene_path('pa1', 'sphere.obj')}"/>
    <bsdf type="diffuse"/>
    <transform name="toWorld"><scale value="1.5,1.5,1.5"/><translate value="0,0,1"/></transform>
  </mesh>
</scene>
""")
    return xml


class Tables:
    """Per global primitive id: vertex ids, and whether it is a sphere, carries vertex normals, is
    normal-mapped."""

    def __init__(self, scene):
        idx = scene.indices().astype(np.int64)
        vid, sph, hasn, mapped = [], [], [], []
        for sh in scene.shapes():
            if sh.type == _abi.SHAPE_SPHERE:
                k, v = 1, np.zeros((1, 3), np.int64)
            else:
                k, v = sh.tri_count, idx[sh.tri_offset:sh.tri_offset + sh.tri_count]
            vid.append(v)
            sph.append(np.full(k, sh.type == _abi.SHAPE_SPHERE))
            hasn.append(np.full(k, sh.type != _abi.SHAPE_SPHERE and sh.has_normals != 0))
            mapped.append(np.full(k, sh.type != _abi.SHAPE_SPHERE and sh.has_normals != 0 and sh.normal_map >= 0))
        self.vid, self.sphere = np.concatenate(vid), np.concatenate(sph)
        self.has_normals, self.mapped = np.concatenate(hasn), np.concatenate(mapped)
        self.num_prims = len(self.vid)
        self.num_vertices = scene.desc.num_vertices
        self.triangles = np.nonzero(~self.sphere)[0]


def synthetic_hits(tab, P, prims, seed, t_range=(0.5, 3.0)):
    """Hits on the given primitive ids (-1: a miss) without a tracer: (u, v) inside the triangle, a
    unit direction at least 0.25 off the triangle's plane (any direction on a degenerate one), t,
    and o = p - t d.  Sphere ids get an arbitrary ray.  Returns (rays (n, 8) f32, hits)."""
    g = np.random.default_rng(seed)
    prims = np.asarray(prims, np.int64)
    n = len(prims)
    a, b = g.uniform(0.05, 0.9, n), g.uniform(0.05, 0.9, n)
    flip = a + b > 0.95
    u, v = np.where(flip, 0.95 - a, a) * 0.98 + 0.01, np.where(flip, 0.95 - b, b) * 0.98 + 0.01
    u, v = np.abs(u).astype(f32), np.abs(v).astype(f32)
    k = np.where(prims < 0, 0, prims)
    f = tab.vid[k]
    P64 = np.asarray(P, np.float64)
    p0, p1, p2 = P64[f[:, 0]], P64[f[:, 1]], P64[f[:, 2]]
    p = (1 - (u + v))[:, None] * p0 + u[:, None] * p1 + v[:, None] * p2
    N = np.cross(p1 - p0, p2 - p0)
    ln = np.linalg.norm(N, axis=1)
    ng = np.divide(N, ln[:, None], out=np.zeros_like(N), where=ln[:, None] > 0)
    d = g.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    c = (d * ng).sum(1)
    low = (np.abs(c) < 0.25) & (ln > 0)
    d[low] = d[low] + ng[low] * np.where(c[low] >= 0, 0.6, -0.6)[:, None]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t = g.uniform(*t_range, n)
    rays = np.zeros((n, 8), f32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = p - t[:, None] * d, 1e-4, d, np.inf
    hits = np.zeros(n, nori_amd.HIT_DTYPE)
    hits["t"], hits["prim"], hits["u"], hits["v"] = t, prims, u, v
    miss = prims < 0
    hits["t"][miss], hits["u"][miss], hits["v"][miss] = np.inf, 0, 0
    return rays, hits


def random_grad(n, seed, nan_payload=False):
    """A random record gradient (n, 16) float32; the ignored words (columns 7, 11, 12..15) hold
    random numbers too, or NaN bit patterns with payloads."""
    g = np.random.default_rng(seed)
    a = g.standard_normal((n, 16)).astype(f32)
    if nan_payload:
        a.view(np.uint32)[:, [7, 11, 12, 13, 14, 15]] = (0x7FC00000 | g.integers(1, 1 << 20, (n, 6))).astype(np.uint32)
    return a


def _live(tab, hits):
    prim = hits["prim"].astype(np.int64)
    ok = (prim >= 0) & (prim < tab.num_prims)
    k = np.where(ok, prim, 0)
    return ok & ~tab.sphere[k], k


def forward64(tab, P, Nrm, rays, hits):
    """(n, 16) float64 in the record's layout: p 0:3, t 3, ng 4:7, ns 8:11; everything the adjoint
    does not differentiate is 0 (and rows that contribute nothing are 0 throughout)."""
    P, Nrm = np.asarray(P, np.float64), np.asarray(Nrm, np.float64)
    n = len(hits)
    out = np.zeros((n, 16))
    live, k = _live(tab, hits)
    f = tab.vid[k]
    u, v = hits["u"].astype(np.float64)[:, None], hits["v"].astype(np.float64)[:, None]
    b = 1 - (u + v)
    o, d = rays[:, 0:3].astype(np.float64), rays[:, 4:7].astype(np.float64)
    p0, p1, p2 = P[f[:, 0]], P[f[:, 1]], P[f[:, 2]]
    N = np.cross(p1 - p0, p2 - p0)
    ln = np.linalg.norm(N, axis=1)
    D = (N * d).sum(1)
    # the fp32 statement decides which rows count (|N| = 0, N.d = 0 in ITS arithmetic)
    live = live & (ln > 0) & (D != 0)
    with np.errstate(all="ignore"):
        ng = N / ln[:, None]
        t = (N * (p0 - o)).sum(1) / D
        M = b * Nrm[f[:, 0]] + u * Nrm[f[:, 1]] + v * Nrm[f[:, 2]]
        lm = np.linalg.norm(M, axis=1)
        ns = np.where((tab.has_normals[k] & ~tab.mapped[k] & (lm > 0))[:, None], M / lm[:, None], 0.0)
        ns = np.where(tab.has_normals[k][:, None], ns, ng)
    out[:, 0:3], out[:, 3], out[:, 4:7], out[:, 8:11] = b * p0 + u * p1 + v * p2, t, ng, ns
    out[~live] = 0
    return out


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def terms32(tab, P, Nrm, rays, hits, grad, with_normals=True):
    """The (n, 18) float32 terms of the header, in its operation order."""
    P, Nrm = np.ascontiguousarray(P, f32), np.ascontiguousarray(Nrm, f32)
    grad = np.ascontiguousarray(grad).view(f32).reshape(-1, 16)
    n = len(hits)
    live, k = _live(tab, hits)
    f = tab.vid[k]
    col = lambda a: a[:, None]  # noqa: E731
    with np.errstate(all="ignore"):
        u, v, t = hits["u"].astype(f32), hits["v"].astype(f32), hits["t"].astype(f32)
        o, d = rays[:, 0:3].astype(f32), rays[:, 4:7].astype(f32)
        g_p, g_t, g_ng, g_ns = grad[:, 0:3], grad[:, 3], grad[:, 4:7], grad[:, 8:11]
        p0, p1, p2 = P[f[:, 0]], P[f[:, 1]], P[f[:, 2]]
        b = f32(1) - (u + v)
        e1, e2 = p1 - p0, p2 - p0
        N = _cross(e1, e2)
        ln = np.sqrt(_dot(N, N))
        D = _dot(N, d)
        live = live & (ln > 0) & (D != 0)
        ng = N / col(ln)
        gq = np.where(col(tab.has_normals[k]), g_ng, g_ng + g_ns)
        gN = (gq - ng * col(_dot(ng, gq))) / col(ln)
        s = g_t / D
        ph = o + d * col(t)
        gN = gN + (p0 - ph) * col(s)
        ge1, ge2 = _cross(e2, gN), _cross(gN, e1)
        t0 = (g_p * col(b) + N * col(s)) - (ge1 + ge2)
        t1 = g_p * col(u) + ge1
        t2 = g_p * col(v) + ge2
        M = (Nrm[f[:, 0]] * col(b) + Nrm[f[:, 1]] * col(u)) + Nrm[f[:, 2]] * col(v)
        lm = np.sqrt(_dot(M, M))
        ns = M / col(lm)
        gM = (g_ns - ns * col(_dot(ns, g_ns))) / col(lm)
        nlive = live & tab.has_normals[k] & ~tab.mapped[k] & (lm > 0) & bool(with_normals)
        out = np.zeros((n, 18), f32)
        out[:, 0:3], out[:, 3:6], out[:, 6:9] = t0, t1, t2
        out[:, 9:12], out[:, 12:15], out[:, 15:18] = gM * col(b), gM * col(u), gM * col(v)
    out[~live] = 0
    out[~nlive, 9:] = 0
    assert out.dtype == f32
    return out


def sums(tab, hits, terms):
    """Per destination float of (positions, normals): the float64 sum S of the terms, the sum A of
    their absolute values and the count m of non-zero terms -- the inputs of the GPU bound
    |out - S| <= m 2^-24 A + 2^-120."""
    live, k = _live(tab, hits)
    f = tab.vid[k]
    res = []
    for base in (0, 9):
        S, A, m = (np.zeros((tab.num_vertices, 3)) for _ in range(3))
        for j in range(3):
            tj = terms[:, base + 3 * j:base + 3 * j + 3].astype(np.float64)
            np.add.at(S, f[:, j], tj)
            np.add.at(A, f[:, j], np.abs(tj))
            np.add.at(m, f[:, j], (tj != 0).astype(np.float64))
        res.append({"S": S, "A": A, "m": m})
    return res


def bound(ref):
    return ref["m"] * 2.0 ** -24 * ref["A"] + 2.0 ** -120


def assert_within_bound(out, ref, what):
    """Every component under the bound, components without a contribution exactly 0; returns the
    largest share of the bound used."""
    out = np.asarray(out, np.float64).reshape(ref["S"].shape)
    assert np.isfinite(out).all(), what
    err, cap = np.abs(out - ref["S"]), bound(ref)
    none = ref["m"] == 0
    assert not out[none].any(), f"{what}: a component without a contribution is not 0"
    share = float((err / cap)[~none].max()) if (~none).any() else 0.0
    print(f"{what}: largest share of the bound used {share:.3f} (m up to {int(ref['m'].max())})")
    assert (err <= cap).all(), f"{what}: {int((err > cap).sum())} components over the bound, worst share {share:.3f}"
    return share


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)
