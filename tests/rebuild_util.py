"""Shared by test_rebuild.py (CPU) and test_gpu_rebuild.py (GPU): two more vertex position sets
and an independent numpy statement of the BVH rebuild (nori_scene_bvh_rebuild in
include/nori_gpu.h).

The numpy statement shares no code with the library: the primitive boxes are min / max on
refit_util's integer key (ordered zeros), the keys are np.float32 arithmetic one operation at a
time, the leaf order is a stable sort of the codes, a range is split where the next key prefix
begins (a search for the first key with a larger prefix, on Python integers -- not the binary
search over leading-bit counts that the library runs), the nodes are numbered breadth-first from
a queue, and the boxes are refit_util.numpy_refit of the topology it made.
"""
import numpy as np

import refit_util as ru
from nori_amd import _abi

LEAF_BIT = ru.LEAF_BIT
SETS = ru.SETS + ("e", "f")
LEAF_MAX = (1, 4, 64)


def position_set(scene, which):
    """refit_util's a-d, and (e) every vertex's y at one constant: a mesh-only scene has extent 0
    on that axis, so its scale is 0; (f) every vertex at one point: all extents of the meshes are
    0 and every triangle's key ties on the code, so the tree comes from the positions' bits."""
    if which in ru.SETS:
        return ru.position_set(scene, which)
    P = scene.positions()
    if which == "e":
        P[:, 1] = np.float32(0.375)
        return P
    assert which == "f"
    P[:] = np.float32([0.25, -1.5, 3.0])
    return P


def _codes(lo, hi):
    """30-bit Morton codes of the boxes' centres on the 1024^3 grid of the scene box."""
    Lo, Hi = ru._unkey(ru._key(lo).min(0)), ru._unkey(ru._key(hi).max(0))
    half = np.float32(0.5)
    with np.errstate(all="ignore"):
        c = (half * lo).astype(np.float32) + (half * hi).astype(np.float32)
        ext = (Hi - Lo).astype(np.float32)
        scale = np.where(ext > 0, np.float32(1024.0) / np.where(ext > 0, ext, np.float32(1)), np.float32(0)).astype(np.float32)
        x = ((c - Lo).astype(np.float32) * scale).astype(np.float32)
    q = np.zeros(x.shape, np.int64)
    ok = x >= 0                                   # False for NaN
    q[ok] = np.where(x[ok] >= 1023, 1023, np.minimum(x[ok], np.float32(1023)).astype(np.int64))
    code = np.zeros(len(q), np.int64)
    for k in range(10):
        for axis, shift in ((0, 2), (1, 1), (2, 0)):
            code |= ((q[:, axis] >> k) & 1) << (3 * k + shift)
    return code


def numpy_rebuild(scene, P, leaf_max):
    """(nodes, prims, root box, info) of the rebuild at positions P with leaves of <= leaf_max."""
    L = leaf_max if leaf_max else 4
    P = np.ascontiguousarray(P, np.float32)
    vid, sph = ru.prim_vertex_ids(scene)
    n = len(vid)
    centre, radius = np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
    i = 0
    for sh in scene.shapes():
        if sh.type == _abi.SHAPE_SPHERE:
            centre[i], radius[i] = np.float32(list(sh.center)), np.float32(sh.radius)
            i += 1
        else:
            i += sh.tri_count
    tri = ~sph
    lo, hi = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    k = ru._key(P[vid[tri]])                       # (tris, 3 vertices, 3 axes)
    lo[tri], hi[tri] = ru._unkey(k.min(1)), ru._unkey(k.max(1))
    lo[sph] = centre[sph] - radius[sph, None]
    hi[sph] = centre[sph] + radius[sph, None]
    code = _codes(lo, hi)
    order = np.argsort(code, kind="stable")        # ties keep the id order: the key is code << 32 | id
    # ---- records in leaf order
    prims = np.zeros((n, 12), np.float32)
    bits = prims.view(np.uint32)
    t = tri[order]
    p0, p1, p2 = (P[vid[order[t], j]] for j in range(3))
    prims[t, 0:3], prims[t, 4:7], prims[t, 8:11] = p0, p1 - p0, p2 - p0
    s = ~t
    prims[s, 0:3], prims[s, 4] = centre[order[s]], radius[order[s]]
    bits[s, 7] = 1
    bits[:, 3] = order
    # ---- topology
    K = (code[order].astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    Kp = [int(v) for v in K]

    def halves(a, b):
        shift = (Kp[a] ^ Kp[b]).bit_length() - 1   # the first bit, from the top, where K[a] and K[b] differ
        nxt = ((Kp[a] >> shift) + 1) << shift       # the smallest key with the next prefix
        g = int(np.searchsorted(K, np.uint64(nxt), side="left")) - 1
        assert a <= g < b
        return (a, g), (g + 1, b)

    def is_leaf(r):
        return r[1] - r[0] + 1 <= L

    rows, level, depth = [], ([(0, n - 1)] if n > L else []), 0
    if n <= L:
        rows.append([(LEAF_BIT | (n - 1) << 25, True)])
        depth = 1
    first_of_next = 1
    while level:
        depth += 1
        nxt_level = []
        for r in level:
            slots = []
            for h in halves(*r):
                slots += [h] if is_leaf(h) else list(halves(*h))
            row = []
            for h in slots:
                if is_leaf(h):
                    row.append((LEAF_BIT | (h[1] - h[0]) << 25 | h[0], True))
                else:
                    row.append((first_of_next + len(nxt_level), True))
                    nxt_level.append(h)
            rows.append(row)
        first_of_next += len(nxt_level)
        level = nxt_level
    nodes = np.zeros((len(rows), 32), np.float32)
    nodes[:, 0:24] = np.nan
    refs = nodes.view(np.uint32)[:, 24:28]
    refs[:] = LEAF_BIT
    for j, row in enumerate(rows):
        for k, (ref, _) in enumerate(row):
            refs[j, k] = ref
            nodes[j, k:24:4] = 0.0
    nodes, prims, root, allp = ru.numpy_refit(scene, nodes, prims, P)
    assert np.array_equal(root.view(np.uint32), allp.view(np.uint32))
    info = {"device_nodes": len(rows), "depth": depth, "num_prims": n, "leaf_max": L}
    return nodes, prims, root, info


def tree_invariants(nodes, prims, leaf_max):
    """Every primitive id once; leaf counts <= leaf_max; inner refs point to higher-numbered
    nodes, each node but the root is referenced once; unused slots are exactly the NaN ones and
    carry the bare leaf bit; the leaves tile the records in order."""
    L = leaf_max if leaf_max else 4
    ids = prims.view(np.uint32)[:, 3]
    assert np.array_equal(np.sort(ids), np.arange(len(prims)))
    refs = nodes.view(np.uint32)[:, 24:28]
    box_nan = np.isnan(nodes[:, :24]).reshape(len(nodes), 6, 4)
    unused = box_nan.all(1)
    assert np.array_equal(unused, box_nan.any(1))              # a slot is NaN in all six rows or in none
    assert (refs[unused] == LEAF_BIT).all() and (nodes.view(np.uint32)[:, 28:32] == 0).all()
    assert (~unused[:, 0]).all() and (np.diff(unused.astype(int), axis=1) >= 0).all()   # filled from slot 0
    used_refs, owner = refs[~unused], np.repeat(np.arange(len(nodes)), 4).reshape(-1, 4)[~unused]
    leaf = (used_refs & LEAF_BIT) != 0
    count = ((used_refs[leaf] >> 25) & 63) + 1
    first = used_refs[leaf] & 0x01FFFFFF
    assert (count <= L).all()
    o = np.argsort(first)
    assert first[o][0] == 0 and np.array_equal(first[o][1:], (first[o] + count[o])[:-1]) \
        and first[o][-1] + count[o][-1] == len(prims)
    inner = used_refs[~leaf]
    assert (inner > owner[~leaf]).all() and np.array_equal(np.sort(inner), np.arange(1, len(nodes)))
    return int(leaf.sum())
