"""Shared by test_refit.py (CPU) and test_gpu_refit.py (GPU): the scenes and vertex position sets
of the dynamic-geometry tests and an independent numpy statement of the BVH refit
(nori_scene_bvh_refit in include/nori_gpu.h).

The numpy statement shares nothing with the library but the tree as built (the topology a refit
keeps): it rebuilds the triangle records from the index array, takes each leaf's box from the
vertices its records' primitive ids name, and propagates upwards by recursion over the child refs.
min / max are taken on an integer key that orders floats as their values with -0 below +0 (the
header's rule), so they cannot depend on the order of their operands.
"""
import numpy as np

import bvh_shapes
import nori_amd
import synth
from conftest import scene_path
from nori_amd import _abi

LEAF_BIT = 0x80000000
SCENES = ("hf", "nest", "pile", "cbox", "apart")
SETS = ("a", "b", "c", "d")


def scene_xml(which, outdir):
    """The four scenes, the smallest that take the refit each way it can go wrong: hf -- a 48 x 48
    cell height field in the Cornell box's walls under its two-triangle area light (4,620
    triangles, several work-groups, a normal tree); nest -- depth 26, a near-pure chain, the most
    levels the library accepts; pile -- one reference leaf of 200 triangles split into a chain of
    <= 64-primitive leaves, two vertices shared by all; cbox -- 14 primitives, two spheres, unused
    NaN slots and a leaf at record 0."""
    if which == "hf":
        return synth.heightfield_scene(outdir, n=48, integrator="path_mis", width=32, height=32, spp=4)
    if which == "nest":
        return bvh_shapes.nest_named(outdir, "d26")
    if which == "pile":
        return bvh_shapes.pile(outdir, 200)
    if which == "apart":
        return apart(outdir)
    return scene_path("pa4", "cbox", "cbox_path_mis.xml")


def apart(outdir):
    """One small triangle far from a pair of them: the SAH splits the single one off first, so the
    leaf at record 0 holds one primitive and its ref is the leaf bit alone -- the word an unused
    slot carries too (the trap the header names; none of the four larger scenes has it)."""
    import os

    os.makedirs(outdir, exist_ok=True)
    verts, faces = [], []
    for k, (x, y, z) in enumerate([(-100.0, -100.0, -100.0), (0.0, 0.0, 0.0), (2.0, 0.0, 0.0)]):
        verts += [(x, y, z), (x + 1, y, z + 0.5), (x, y + 1, z + 0.25)]
        faces.append((3 * k + 1, 3 * k + 2, 3 * k + 3))
    obj = os.path.join(outdir, "apart.obj")
    bvh_shapes._write_obj(obj, verts, faces)
    camera = {"fov": 60, "near": 1e-4, "far": 1e4, "origin": "10, 0.5, 30", "target": "10, 0.5, 0"}
    meshes = f"""  <mesh type="obj"><string name="filename" value="{obj}"/>
    <bsdf type="diffuse"/></mesh>
"""
    xml = os.path.join(outdir, "apart.xml")
    with open(xml, "w") as f:
        f.write(bvh_shapes._xml("normals", "", camera, 32, 24, 1, meshes))
    return xml


def load(which, outdir, positions=None, normals=None):
    """The scene loaded; with `positions` (and `normals`) its vertex arrays are overwritten in
    place, so a context created on it is a fresh context on that geometry."""
    s = nori_amd.load_scene(scene_xml(which, outdir), 32, 32, 4) if which == "cbox" else \
        nori_amd.load_scene(scene_xml(which, outdir))
    n = s.desc.num_vertices
    if positions is not None:
        np.ctypeslib.as_array(s.desc.positions, shape=(n, 3))[:] = positions
    if normals is not None:
        np.ctypeslib.as_array(s.desc.normals, shape=(n, 3))[:] = normals
    return s


def used_box(scene):
    """min, max over the vertices the triangles use (float64)."""
    p = scene.positions()[np.unique(scene.indices())].astype(np.float64)
    return p.min(0), p.max(0)


def position_set(scene, which, seed=5):
    """(a) the positions as loaded; (b) a smooth displacement of about a twentieth of each
    vertex's own scale (one cell of the height field; relative, so that the nest's 20 decades all
    move); (c) every vertex at a uniform random point of a box three times the scene's: the boxes
    overlap wildly and the root box grows; (d) the vertices of every tenth triangle collapsed
    onto its first vertex, and a twentieth of all vertices given a coordinate of -0.0."""
    P = scene.positions()
    rng = np.random.default_rng(seed)
    if which == "a":
        return P
    if which == "b":
        s = np.abs(P).max(axis=1, keepdims=True).astype(np.float64)
        q = np.divide(P, s, out=np.zeros(P.shape, np.float64), where=s > 0)
        return (P + 0.05 * s * np.sin(q * [7.1, 5.3, 9.7] + [0.3, 1.1, 2.0])).astype(np.float32)
    if which == "c":
        lo, hi = used_box(scene)
        mid, half = 0.5 * (lo + hi), 1.5 * (hi - lo)
        return rng.uniform(mid - half, mid + half, size=P.shape).astype(np.float32)
    assert which == "d"
    Q = P.copy()
    for f in scene.indices()[::10]:
        Q[f[1]] = Q[f[2]] = Q[f[0]]
    k = rng.choice(len(Q), size=max(1, len(Q) // 20), replace=False)
    Q[k, rng.integers(0, 3, size=len(k))] = np.float32(-0.0)
    return Q


def prim_vertex_ids(scene):
    """(num_prims, 3) vertex ids by global primitive id (shape order; a sphere: zeros) and the sphere flags."""
    idx = scene.indices()
    vid, sph = [], []
    for sh in scene.shapes():
        if sh.type == _abi.SHAPE_SPHERE:
            vid.append(np.zeros((1, 3), np.int64))
            sph.append(np.ones(1, bool))
        else:
            vid.append(idx[sh.tri_offset:sh.tri_offset + sh.tri_count].astype(np.int64))
            sph.append(np.zeros(sh.tri_count, bool))
    return np.concatenate(vid), np.concatenate(sph)


def _key(x):
    """float32 -> int64 ordered like the values, -0 below +0."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.int64)
    return np.where(b >> 31, -(b & 0x7FFFFFFF) - 1, b)


def _unkey(k):
    k = np.asarray(k, np.int64)
    return np.where(k >= 0, k, (-k - 1) | LEAF_BIT).astype(np.uint32).view(np.float32)


def numpy_refit(scene, nodes0, prims0, P):
    """The refit of the tree (nodes0, prims0) as built to positions P: (nodes, prims, root box),
    and the min / max over all primitives for the root-box check."""
    P = np.ascontiguousarray(P, np.float32)
    vid, sphere_of_prim = prim_vertex_ids(scene)
    prims = prims0.copy()
    bits = prims.view(np.uint32)
    sph = bits[:, 7] == 1
    ids = bits[:, 3].astype(np.int64)
    assert np.array_equal(sph, sphere_of_prim[ids]) and np.array_equal(np.sort(ids), np.arange(len(ids)))
    tri = ~sph
    v = vid[ids[tri]]
    p0, p1, p2 = P[v[:, 0]], P[v[:, 1]], P[v[:, 2]]
    prims[tri, 0:3], prims[tri, 4:7], prims[tri, 8:11] = p0, p1 - p0, p2 - p0
    # per-record boxes as keys
    lo = np.zeros((len(prims), 3), np.int64)
    hi = np.zeros((len(prims), 3), np.int64)
    k = _key(np.stack([p0, p1, p2], 1))
    lo[tri], hi[tri] = k.min(1), k.max(1)
    c, r = prims[sph, 0:3], prims[sph, 4:5]
    lo[sph], hi[sph] = _key(c - r), _key(c + r)
    nodes = nodes0.copy()
    refs = nodes0.view(np.uint32)[:, 24:28]
    used = ~np.isnan(nodes0[:, 0:4])

    def fit(n):
        blo, bhi = [], []
        for s in range(4):
            if not used[n, s]:
                continue
            ref = int(refs[n, s])
            if ref & LEAF_BIT:
                first, count = ref & 0x01FFFFFF, ((ref >> 25) & 63) + 1
                l, h = lo[first:first + count].min(0), hi[first:first + count].max(0)
            else:
                l, h = fit(ref)
            nodes[n, [s, 4 + s, 8 + s]] = _unkey(l)
            nodes[n, [12 + s, 16 + s, 20 + s]] = _unkey(h)
            blo.append(l)
            bhi.append(h)
        return np.min(blo, 0), np.max(bhi, 0)

    rl, rh = fit(0)
    root = np.concatenate([_unkey(rl), _unkey(rh)])
    allp = np.concatenate([_unkey(lo.min(0)), _unkey(hi.max(0))])
    return nodes, prims, root, allp


def same_bits(a, b):
    """Bit equality of two float32 arrays; NaN slots (whatever their payload) compare as 'both NaN'."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))
