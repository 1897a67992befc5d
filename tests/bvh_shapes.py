"""Deterministic scenes that push the BVH walk off its easy operating point
(test_bvh_shapes.py on the CPU, test_gpu_bvh_shapes.py on the GPU).

nest(outdir, s0, r, n): triangle k is (a,0,0), (0,a,0), (0,0,a) with
    a = s0 * r**k.  The bounding boxes are nested cubes [0,a]^3, the SAH peels
    a few of the largest triangles per level and the 4-wide collapse keeps the
    tree almost a pure chain: depth 23 at 500 triangles (r = 1.08), 44 at 800.
    With `light` the scene also holds a small area light and the camera looks
    at the nest from outside the positive octant at the middle scale
    S = s0 * r**(n // 2), so the image shows many levels of it.
pile(outdir, m): m triangles (0,0,0), (1,0,1), (0,1,t_k), t_k evenly spaced in
    [0.05, 0.95].  All share the bounding box [0,1]^3 and so the centroid
    bounds' extent is on z only; no SAH split beats the leaf, and the
    reference makes one leaf of m primitives -- which the device layout has to
    split into leaves of at most 64 (bvh_builder.cpp leaf_ref).

Every function writes an OBJ and an XML into `outdir` and returns the XML's path.
"""
import os

import numpy as np


# (s0, r, n) of the four nests the tests use, every one with the area light (which changes the
# tree, so n was searched on the final scene).  The names state the 4-wide depth, which
# test_bvh_shapes.py asserts: 22 is the last depth NORI_BVH_STACK=8 can hold (3 * 22 + 1 <= 4 + 64),
# 23 the last for stack 16, 24 the first and 26 the last for stack 32, 27 the first refused.
# s0 = 1e-9 keeps the largest triangle at 1.4e11: Moeller-Trumbore's numerator of t is of the order
# a * a * |o|, and with origins out to a few a it overflows fp32 from a ~ 3e12 on -- both sides
# then accept t = inf at maxt = inf and every overflowing triangle ties (seen with s0 = 1e-4: up
# to 2 % of the rays).  The price: triangles below a = 1e-4 (det < 1e-8, the test's parallel-ray
# threshold) cannot be hit, about 120 of each nest.
NESTS = {"d22": (1e-9, 1.1, 412), "d23": (1e-9, 1.1, 416), "d24": (1e-9, 1.1, 436), "d26": (1e-9, 1.1, 478),
         "d27": (1e-9, 1.1, 488)}


def nest_named(outdir, name, **kw):
    return nest(outdir, *NESTS[name], light=True, **kw)


def nest_rays(s0, r, n, count, seed, mint, beyond=2000):
    """`count` rays with origins uniform(-0.2, 1.2)^3 times a scale drawn log-uniformly over the
    nest's [s0, s0 r^(n-1)] and uniform directions, a tenth of them axis-aligned (the d_i == 0
    slab branch), then `beyond` rays from beyond the largest triangle aimed at the origin: they
    cross every level of the tree, so the traversal stack is as full as it gets."""
    rng = np.random.default_rng(seed)
    a = nest_scales(s0, r, n)
    scale = np.exp(rng.uniform(np.log(a[0]), np.log(a[-1]), size=(count, 1)))
    org = rng.uniform(-0.2, 1.2, size=(count, 3)) * scale
    d = rng.normal(size=(count, 3))
    k = count // 10
    d[:k] = 0.0
    d[np.arange(k), rng.integers(0, 3, size=k)] = rng.choice([-1.0, 1.0], size=k)
    far = rng.uniform(0.2, 1.0, size=(beyond, 3)) * (2.0 * a[-1])
    # ... and as many from inside the smallest one outwards: every box of the chain holds the
    # origin and starts at the shared corner (0,0,0), so the child order is decided by ties
    near = rng.uniform(0.05, 0.3, size=(beyond, 3)) * a[0]
    org, d = np.concatenate([org, far, near]), np.concatenate([d, -far, rng.uniform(0.1, 1.0, size=(beyond, 3))])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((count + 2 * beyond, 8), np.float32)
    rays[:, :3], rays[:, 3], rays[:, 4:7], rays[:, 7] = org, mint, d, np.inf
    return rays


def pile_edge_rays(count):
    """Rays along +y through points (s, 0, s) of the edge every triangle of a pile shares: on
    each of them v = 0 exactly and t = t_k * (1 / t_k), which is 1 for some k and 1 - 2^-24 for
    others -- true ties between many triangles."""
    rays = np.zeros((count, 8), np.float32)
    s = np.linspace(0.1, 0.9, count)
    rays[:, 0], rays[:, 1], rays[:, 2], rays[:, 3], rays[:, 5], rays[:, 7] = s, -1.0, s, 1e-4, 1.0, np.inf
    return rays


def nest_scales(s0, r, n):
    return np.float64(s0) * np.float64(r) ** np.arange(n, dtype=np.float64)


def _write_obj(path, verts, faces):
    with open(path, "w") as f:
        f.write("".join(f"v {x:.9g} {y:.9g} {z:.9g}\n" for x, y, z in verts))
        f.write("".join(f"f {i} {j} {k}\n" for i, j, k in faces))


def _xml(integrator, props, camera, width, height, spp, meshes):
    return f"""<?xml version='1.0' encoding='utf-8'?>
<scene>
  <integrator type="{integrator}">{props}</integrator>
  <camera type="perspective">
    <float name="fov" value="{camera["fov"]}"/>
    <float name="nearClip" value="{camera["near"]:.9g}"/>
    <float name="farClip" value="{camera["far"]:.9g}"/>
    <transform name="toWorld">
      <lookat target="{camera["target"]}" origin="{camera["origin"]}" up="0, 0, 1"/>
    </transform>
    <integer name="height" value="{height}"/>
    <integer name="width" value="{width}"/>
  </camera>
  <sampler type="independent"><integer name="sampleCount" value="{spp}"/></sampler>
{meshes}</scene>
"""


def _vec(v):
    return ", ".join(f"{x:.9g}" for x in v)


def nest(outdir, s0, r, n, integrator="normals", props="", light=False, width=48, height=36, spp=4):
    os.makedirs(outdir, exist_ok=True)
    a = nest_scales(s0, r, n)
    z = np.zeros(n)
    verts = np.stack([np.stack([a, z, z], 1), np.stack([z, a, z], 1), np.stack([z, z, a], 1)], 1).reshape(-1, 3)
    faces = np.arange(1, 3 * n + 1).reshape(n, 3)
    tag = f"nest_{s0:g}_{r:g}_{n}"
    obj = os.path.join(outdir, tag + ".obj")
    _write_obj(obj, verts, faces)
    S = float(a[n // 2])
    # from outside the octant, through its open y < 0 side, towards the origin: the rays enter at
    # every scale below S and meet the front (+(1,1,1)) face of the next smaller triangle
    camera = {"fov": 50, "near": 1e-4 * S, "far": 1e4 * S, "origin": _vec(np.float64([1.5, -0.5, 1.5]) * S),
              "target": _vec(np.float64([0.2, 0.2, 0.2]) * S)}
    meshes = f"""  <mesh type="obj"><string name="filename" value="{obj}"/>
    <bsdf type="diffuse"><color name="albedo" value="0.7 0.6 0.5"/></bsdf></mesh>
"""
    if light:
        c = np.float64([1.3, -0.7, 1.6]) * S  # beside the camera; its normal points at the origin
        nrm = -c / np.linalg.norm(c)
        e1 = np.cross(nrm, [0.0, 0.0, 1.0])
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(nrm, e1)
        h = 0.2 * S
        lobj = os.path.join(outdir, tag + "_light.obj")
        _write_obj(lobj, [c - h * e1 - h * e2, c + h * e1 - h * e2, c + h * e2], [(1, 2, 3)])
        meshes += f"""  <mesh type="obj"><string name="filename" value="{lobj}"/>
    <emitter type="area"><color name="radiance" value="60 60 60"/></emitter></mesh>
"""
    xml = os.path.join(outdir, f"{tag}_{integrator}{'_light' if light else ''}.xml")
    with open(xml, "w") as f:
        f.write(_xml(integrator, props, camera, width, height, spp, meshes))
    return xml


def pile(outdir, m, width=32, height=24, spp=1):
    os.makedirs(outdir, exist_ok=True)
    t = np.linspace(0.05, 0.95, m)
    verts = [(0, 0, 0), (1, 0, 1)] + [(0, 1, tk) for tk in t]
    faces = [(1, 2, 3 + k) for k in range(m)]
    obj = os.path.join(outdir, f"pile_{m}.obj")
    _write_obj(obj, verts, faces)
    camera = {"fov": 40, "near": 1e-4, "far": 1e4, "origin": "2.5, 0.4, 0.5", "target": "0.3, 0.4, 0.5"}
    meshes = f"""  <mesh type="obj"><string name="filename" value="{obj}"/>
    <bsdf type="diffuse"/></mesh>
"""
    xml = os.path.join(outdir, f"pile_{m}.xml")
    with open(xml, "w") as f:
        f.write(_xml("normals", "", camera, width, height, spp, meshes))
    return xml
