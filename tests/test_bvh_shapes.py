"""The scenes of bvh_shapes.py on the CPU: what the GPU tests of the BVH walk
(test_gpu_bvh_shapes.py) take for granted.

* the host build of every generated scene equals the oracle's (node count, SAH
  cost, leaf order), the nests have the depths their names state and an
  oversized leaf is split the way a few lines of Python predict;
* the oracle's own traversal stack (64 entries, as the reference's) is guarded:
  a walk that needs more fails oracle_trace / oracle_render instead of writing
  past the array.  No generator reaches 64 -- the deepest nest whose a * a stays
  a normal fp32 number (s0 = 1e-16, r = 1.1, n = 800: 4-wide depth 44) needs 48
  entries, and below s0 = 1e-17 the SAH's areas underflow and the build makes
  one leaf -- so the guard is tested on a stand-alone build with the limit
  lowered to 8;
* nori_test_util.prim_hit, the numpy fp32 ray-primitive test behind the tie rule
  of test_gpu_parity._compare_hits, returns the oracle's t, u, v bit for bit;
* _compare_hits accepts a true tie and refuses 10 ids in 22,000 moved to a
  neighbouring triangle and one u changed in its last bit.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bvh_shapes
import nori_amd
import pyoracle
from conftest import ROOT, scene_path
from nori_test_util import prim_hit
from test_bvh_build import _compare
from test_gpu_parity import _compare_hits, _rays

PILES = [64, 65, 128, 129, 200, 1000]
# 4-wide depth bands (scene_plan.cpp bvh_stack_for: need = 3 * depth + 1 entries; 4, 8 or 16 of
# them in LDS for stack 8, 16, 32 and 64 more in private memory)
BANDS = {"d22": (1, 22), "d23": (23, 23), "d24": (24, 26), "d26": (24, 26), "d27": (27, 64)}


@pytest.fixture(scope="module")
def outdir(built, tmp_path_factory):
    return str(tmp_path_factory.mktemp("bvh_shapes"))


@pytest.mark.parametrize("name", list(bvh_shapes.NESTS))
def test_nest_build_matches_oracle_and_depth(outdir, name):
    g = _compare(nori_amd.load_scene(bvh_shapes.nest_named(outdir, name)))
    lo, hi = BANDS[name]
    print(name, bvh_shapes.NESTS[name], g)
    assert lo <= g["depth"] <= hi
    assert g["num_prims"] == bvh_shapes.NESTS[name][2] + 1  # + the light's triangle
    # the same geometry under the other integrators of the render tests
    for integ in ("path_mis", "photonmapper"):
        props = '<integer name="photonCount" value="100"/><float name="photonRadius" value="1"/>'
        s = nori_amd.load_scene(bvh_shapes.nest_named(outdir, name, integrator=integ,
                                                      props=props if integ == "photonmapper" else ""))
        assert nori_amd.bvh_info(s) == g


def _predicted_device_tree(m):
    """(4-wide nodes, depth) of one reference leaf of m primitives (bvh_builder.cpp): the leaf is
    halved down to at most 64 per leaf under a root whose second child is empty, then every node
    opens its first inner child (all boxes are [0,1]^3, so the largest-area choice is the first)
    until it has four children; the empty child takes a slot and is never opened."""
    def halve(c):
        return None if c <= 64 else (halve(c // 2), halve(c - c // 2))

    def collapse(node):
        ch = list(node)
        while len(ch) < 4:
            i = next((i for i, c in enumerate(ch) if isinstance(c, tuple)), None)
            if i is None:
                break
            ch[i:i + 1] = list(ch[i])
        sub = [collapse(c) for c in ch if isinstance(c, tuple)]
        return 1 + sum(n for n, _ in sub), 1 + max([d for _, d in sub], default=0)

    return collapse((halve(m), "empty"))


@pytest.mark.parametrize("m", PILES)
def test_pile_is_one_reference_leaf_split_for_the_device(outdir, m):
    g = _compare(nori_amd.load_scene(bvh_shapes.pile(outdir, m)))
    print(m, g)
    assert g["ref_nodes"] == 1 and g["num_prims"] == m
    assert (g["device_nodes"], g["depth"]) == _predicted_device_tree(m)


def test_predicted_device_tree_by_hand():
    # 129 = 64 + (32 + 33): one node of three leaves; 200 = (50 + 50) + 100 and a node for 50 + 50
    assert [_predicted_device_tree(m) for m in (64, 65, 128, 129, 200, 1000)] == [(1, 1), (1, 1), (1, 1), (1, 1), (2, 2),
                                                                                 (6, 3)]


def _cube_rays(n, seed, mint=1e-4):
    return _rays(n, seed, [-0.5, -0.5, -0.5], [1.5, 1.5, 1.5], mint=mint)


# ---------------------------------------------------------------- the oracle's stack guard
def test_oracle_stack_guard(outdir):
    """nori_oracle.c built on its own with ORACLE_BVH_STACK=8: the depth-26 nest (a chain: the
    walk holds one entry per binary level) fails trace and render with a non-zero code, a scene of
    one node passes, and the oracle proper (64 entries) walks the deepest nest without complaint."""
    so = os.path.join(outdir, "liboracle_stack8.so")
    src = os.path.join(ROOT, "oracle", "nori_oracle.c")
    subprocess.run([os.environ.get("CC", "cc"), "-O2", "-std=gnu11", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
                    "-DORACLE_BVH_STACK=8", "-shared", "-o", so, src, "-lm", "-pthread"], check=True)
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.oracle_scene_create.argtypes = [vp, C.POINTER(vp)]
    lib.oracle_trace.argtypes = [vp, vp, C.c_uint32, C.c_int, vp]
    lib.oracle_render.argtypes = [vp, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32, vp, C.c_uint32, C.c_int, C.c_int,
                                  vp, vp]
    lib.oracle_scene_free.argtypes = [vp]

    def run(scene, rays):
        h = vp()
        assert lib.oracle_scene_create(C.cast(scene.desc_ptr, vp), C.byref(h)) == 0
        hits = np.zeros(rays.shape[0], dtype=[("t", "<f4"), ("prim", "<i4"), ("u", "<f4"), ("v", "<f4")])
        film = np.zeros(scene.film_shape(), np.float32)
        codes = (lib.oracle_trace(h, rays.ctypes.data, rays.shape[0], 0, hits.ctypes.data),
                 lib.oracle_trace(h, rays.ctypes.data, rays.shape[0], 1, hits.ctypes.data),
                 lib.oracle_render(h, 0, 0, 0, 1, None, 0, 2, 0, film.ctypes.data, None))
        lib.oracle_scene_free(h)
        return codes, hits

    deep = nori_amd.load_scene(bvh_shapes.nest_named(outdir, "d26"))
    rays = bvh_shapes.nest_rays(*bvh_shapes.NESTS["d26"], 2000, 3, 1e-4)
    codes, _ = run(deep, rays)
    assert all(c != 0 for c in codes), codes
    flat = nori_amd.load_scene(bvh_shapes.pile(outdir, 64))
    rays1 = _cube_rays(2000, 4)
    codes, hits = run(flat, rays1)
    assert codes == (0, 0, 0)
    want = pyoracle.OracleScene(flat).trace(rays1, any_hit=True)
    assert np.array_equal(hits, want) and (want["prim"] >= 0).sum() > 100
    # the oracle proper: the deepest nest of the table above, and the guard's error reaches Python
    s0, r, n = 1e-16, 1.1, 800
    deepest = nori_amd.load_scene(bvh_shapes.nest(outdir, s0, r, n))
    assert nori_amd.bvh_info(deepest)["depth"] >= 40
    got = pyoracle.OracleScene(deepest).trace(bvh_shapes.nest_rays(s0, r, n, 2000, 5, 0.0))
    assert np.isfinite(got["t"]).mean() > 0.3


# ---------------------------------------------------------------- the numpy restatement and the tie rule
@pytest.fixture(scope="module")
def traced(outdir):
    """(scene, rays, the oracle's closest hits) of cbox and pile(200); shared, never modified."""
    res = {}
    cbox = nori_amd.load_scene(scene_path("pa4", "cbox", "cbox_path_mis.xml"), 32, 32, 1)
    rays = np.concatenate([_rays(20000, 1, [-0.9, 0.05, -0.9], [0.9, 1.5, 0.9]),
                           _rays(2000, 2, [-3, -1, -3], [3, 3, 6], mint=0.0)])
    res["cbox"] = (cbox, rays, pyoracle.OracleScene(cbox).trace(rays))
    pile = nori_amd.load_scene(bvh_shapes.pile(outdir, 200))
    rays = np.concatenate([_cube_rays(20000, 3), _cube_rays(2000, 4, mint=0.0)])
    res["pile"] = (pile, rays, pyoracle.OracleScene(pile).trace(rays))
    for v in res.values():
        v[1].setflags(write=False)
        v[2].setflags(write=False)
    return res


@pytest.mark.parametrize("name", ["cbox", "pile"])
def test_prim_hit_equals_the_oracle_bit_for_bit(traced, name):
    s, rays, c = traced[name]
    fin = np.flatnonzero(np.isfinite(c["t"]))
    assert fin.size > 2000
    if name == "cbox":  # spheres and triangles
        assert len(np.unique(c["prim"][fin])) >= 14
    hit, t, u, v = prim_hit(s, rays[fin], c["prim"][fin])
    assert hit.all()
    for mine, k in ((t, "t"), (u, "u"), (v, "v")):
        assert np.array_equal(mine.view(np.uint32), c[k][fin].view(np.uint32)), k
    # ... and another primitive is not the same hit
    other = (c["prim"][fin] + 1) % nori_amd.bvh_info(s)["num_prims"]
    hit2, t2, _, _ = prim_hit(s, rays[fin], other)
    assert (hit2 & (t2 == c["t"][fin])).mean() < 0.01


@pytest.mark.parametrize("name", ["cbox", "pile"])
def test_compare_hits_bites(traced, name):
    """_compare_hits on the oracle's result against itself passes; with 10 of the 22,000 ids moved
    to a neighbouring triangle (99.95 % still equal: the old rule passed it) and with one u
    changed in its last bit it must fail."""
    s, rays, c = traced[name]
    assert _compare_hits(c.copy(), c, s, rays) == 0
    tri = np.flatnonzero(np.isfinite(c["t"]) & (c["u"] != 0))  # (spheres report u = 0)
    n = nori_amd.bvh_info(s)["num_prims"]
    moved = c.copy()
    pick = tri[:: tri.size // 10][:10]
    for i in pick:  # the triangle next to it in its mesh (cbox: the other half of the wall)
        moved["prim"][i] = c["prim"][i] ^ 1 if name == "cbox" else (c["prim"][i] + 1) % n
    assert (moved["prim"] == c["prim"]).mean() > 0.999
    with pytest.raises(AssertionError, match="not a tie"):
        _compare_hits(moved, c, s, rays)
    with pytest.raises(AssertionError, match="not a tie"):
        _compare_hits(c, moved, s, rays)
    one = c.copy()
    one["u"].view(np.uint32)[tri[7]] ^= 1
    with pytest.raises(AssertionError):
        _compare_hits(one, c, s, rays)
    one = c.copy()
    one["v"].view(np.uint32)[tri[-7]] ^= 1
    with pytest.raises(AssertionError):
        _compare_hits(one, c, s, rays)


def test_compare_hits_accepts_a_true_tie(outdir):
    """Rays along +y through points of the fan's shared edge (0,0,0)-(1,0,1): v is exactly 0 on
    every triangle of the pile and t = t_k * (1 / t_k), so many triangles return the very same t.
    Another id among those is a legitimate answer; one that returns another t is not."""
    s = nori_amd.load_scene(bvh_shapes.pile(outdir, 200))
    rays = bvh_shapes.pile_edge_rays(64)
    c = pyoracle.OracleScene(s).trace(rays)
    assert np.isfinite(c["t"]).all() and (c["v"] == 0).all()
    n = rays.shape[0]
    ties = np.zeros((200, n), bool)
    for k in range(200):
        hit, t, _, _ = prim_hit(s, rays, np.full(n, k))
        ties[k] = hit & (t == c["t"])
    assert ties[c["prim"], np.arange(n)].all()
    assert (ties.sum(0) >= 2).all() and not ties.all(0).any()
    # the rule needs > 99.9 % equal ids: pad with rays that hit nothing
    pad = _rays(4 * 1024, 9, [2, 2, 2], [3, 3, 3])
    pad[:, 4:7] = np.abs(pad[:, 4:7])
    both = np.concatenate([rays[:4], pad])
    cc = pyoracle.OracleScene(s).trace(both)
    assert not np.isfinite(cc["t"][4:]).any()
    g = cc.copy()
    for i in range(4):
        g["prim"][i] = next(k for k in range(200) if ties[k, i] and k != cc["prim"][i])
    assert _compare_hits(g, cc, s, both) == 4
    for i in range(4):
        g["prim"][i] = next(k for k in range(200) if not ties[k, i])
    with pytest.raises(AssertionError, match="not a tie"):
        _compare_hits(g, cc, s, both)
