"""The BVH walk (traverse.h traverse<STACK, ANY>) off its easy operating point, against the CPU
oracle: deep chains at every traversal stack that may hold them, the three stacks against each
other, reference leaves larger than the device's 64-primitive leaves, the scan/BVH switch, every
kernel that walks the tree at stack 32, and the refusal of a tree no stack can hold.

The scenes are bvh_shapes.py's (their builds, depths and the comparison's tie rule are checked on
the CPU in test_bvh_shapes.py).  The stack follows from the depth (scene_plan.cpp bvh_stack_for:
3 * depth + 1 entries needed; stack 8, 16, 32 keep 4, 8, 16 of them in LDS and 64 in private
memory) or from NORI_BVH_STACK, read at context creation; there is no stats field for it.

Why no combination here can overflow: the stack holds the not-yet-visited siblings of the inner
nodes on the current path -- a node pushes at most 3 of its 4 children before it descends into
the fourth, and a popped entry is off the stack before its own children are pushed -- so it never
holds more than 3 * depth entries, one fewer than the capacity check (on the chosen or the
overriding stack alike) asks for.  Every scene x stack pair below is one that check accepts.
The ray sets do fill it: a host port of the walk over these rays and trees holds 66, 69, 72 and
78 entries at most on d22, d23, d24 and d26 (3 * depth each), and about half the rays of a set
go beyond 16 entries, into the private-memory part of even the largest stack (DESIGN_LOG.md).

Hits: t, u, v bit for bit and ids equal or tied (test_gpu_parity._compare_hits).  Images: the
bars of test_gpu_parity.py / test_gpu_photon_map.py, unchanged.
"""
import contextlib
import os

import numpy as np
import pytest

import bvh_shapes
import nori_amd
import pyoracle
from conftest import scene_path
from nori_amd import _abi
from nori_test_util import assert_parity, image_parity
from test_gpu_parity import _compare_hits, _rays

pytestmark = pytest.mark.gpu

PHOTONS = '<integer name="photonCount" value="2000"/><float name="photonRadius" value="{r:.9g}"/>'


@contextlib.contextmanager
def _env(**kw):
    """Environment variables set (None: unset) for the block, always restored."""
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _renderer(scene, stack=None, mode=None, fuse=None):
    """GpuRenderer with the traversal stack (8, 16, 32; None = chosen from the depth), the
    traversal mode and the fused trace launch forced; all three are read at context creation."""
    with _env(NORI_BVH_STACK=stack, NORI_TRAVERSAL=mode, NORI_TRACE_FUSE=fuse):
        return nori_amd.GpuRenderer(scene, 0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_hits(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in ("t", "prim", "u", "v"))


class _Shapes:
    """Scenes, oracles, rays and the oracle's answers, made once per module and only read."""

    def __init__(self, outdir):
        self.outdir = outdir
        self._nest, self._pile, self._img = {}, {}, {}

    def nest(self, name):
        if name not in self._nest:
            s0, r, n = bvh_shapes.NESTS[name]
            s = nori_amd.load_scene(bvh_shapes.nest_named(self.outdir, name))
            o = pyoracle.OracleScene(s)
            sets = []
            for seed, mint in ((11, 0.0), (12, 1e-4)):
                rays = bvh_shapes.nest_rays(s0, r, n, 16000, seed, mint)
                sh = rays.copy()  # occlusion: maxt around the origin's own scale
                sh[:, 7] = (np.random.default_rng(seed + 100).uniform(0.01, 2.0, size=rays.shape[0])
                            * np.abs(rays[:, :3]).max(axis=1))
                sets.append((rays, o.trace(rays), sh, o.trace(sh, any_hit=True)))
            self._nest[name] = (s, nori_amd.bvh_info(s), sets)
        return self._nest[name]

    def pile(self, m):
        if m not in self._pile:
            s = nori_amd.load_scene(bvh_shapes.pile(self.outdir, m))
            rays = np.concatenate([_rays(20000, 20 + m, [-0.5] * 3, [1.5] * 3), bvh_shapes.pile_edge_rays(10)])
            self._pile[m] = (s, rays, pyoracle.OracleScene(s).trace(rays))
        return self._pile[m]

    def render_scene(self, name, integrator):
        """(scene, the oracle's developed image) of a nest under an integrator, 48 x 36 at 4 spp."""
        if (name, integrator) not in self._img:
            s0, r, n = bvh_shapes.NESTS[name]
            props = PHOTONS.format(r=0.1 * bvh_shapes.nest_scales(s0, r, n)[n // 2]) if integrator == "photonmapper" else ""
            s = nori_amd.load_scene(bvh_shapes.nest_named(self.outdir, name, integrator=integrator, props=props))
            self._img[name, integrator] = (s, nori_amd.develop(s, pyoracle.OracleScene(s).render(rng="wave")))
        return self._img[name, integrator]


@pytest.fixture(scope="module")
def shapes(built, tmp_path_factory):
    return _Shapes(str(tmp_path_factory.mktemp("bvh_shapes_gpu")))


# ---------------------------------------------------------------- the walk against the oracle
WALKS = [("d22", 8), ("d22", 16), ("d22", 32), ("d23", 16), ("d23", 32), ("d24", None), ("d24", 32), ("d26", None),
         ("d26", 32)]


@pytest.mark.parametrize("name,stack", WALKS)
def test_walk_matches_oracle(shapes, name, stack):
    s, info, sets = shapes.nest(name)
    n = bvh_shapes.NESTS[name][2]
    with _renderer(s, stack) as r:
        for rays, c, sh, csh in sets:
            fin = np.isfinite(c["t"])
            distinct = len(np.unique(c["prim"][fin]))
            occluded = (csh["prim"] >= 0).mean()
            # (the ray set has not degraded into misses, against the oracle's own result)
            assert fin.mean() >= 0.3 and distinct >= n // 2 and 0.1 <= occluded <= 0.9
            assert (c["prim"][~fin] == -1).all() and not np.isnan(c["u"]).any() and not np.isnan(c["v"]).any()
            closest = r.trace(rays)
            ties = _compare_hits(closest, c, s, rays)
            g = r.trace(sh, any_hit=True)
            assert np.array_equal(g["prim"] >= 0, csh["prim"] >= 0)
            print(f"{name} (n = {n}, depth {info['depth']}) stack {stack}, mint {rays[0, 3]:g}: hit share {fin.mean():.3f}, "
                  f"{distinct} primitives hit, occluded {occluded:.3f}, id mismatches (all ties) {ties}")
        q = r.query(rays[-4096:], surface=False)  # (the last set's rays: the ones that cross every level)
        assert r.last_stats["bvh_depth"] == info["depth"] and r.last_stats["bvh_nodes"] == info["device_nodes"]
        assert r.last_stats["scan_rtc"] == 0
        assert _same_hits(q["hits"], closest[-4096:])


def test_the_three_stacks_agree_bit_for_bit(shapes):
    s, info, sets = shapes.nest("d22")
    assert info["depth"] <= 22
    got = {}
    for stack in (8, 16, 32):
        with _renderer(s, stack) as r:
            got[stack] = [(r.trace(rays), r.trace(sh, any_hit=True)) for rays, _, sh, _ in sets]
    for stack in (16, 32):
        for (a, ash), (b, bsh) in zip(got[8], got[stack]):
            assert _same_hits(a, b) and _same_hits(ash, bsh)


# ---------------------------------------------------------------- oversized leaves and the scan/BVH switch
@pytest.mark.parametrize("m,mode", [(64, "bvh"), (65, None), (129, None), (1000, None)])
def test_oversized_leaf_matches_oracle(shapes, m, mode):
    s, rays, c = shapes.pile(m)
    fin = np.isfinite(c["t"])
    assert fin.mean() > 0.05 and len(np.unique(c["prim"][fin])) >= min(m, 500)
    with _renderer(s, mode=mode) as r:
        ties = _compare_hits(r.trace(rays), c, s, rays)
        r.query(rays[:256], surface=False)
        assert r.last_stats["scan_rtc"] == 0  # the BVH walk, not the scan
        assert r.last_stats["bvh_depth"] == nori_amd.bvh_info(s)["depth"]
    print(f"pile({m}) {mode or 'automatic'}: hit share {fin.mean():.3f}, id mismatches (all ties) {ties}")


def test_64_primitives_scan_and_65_walk(shapes):
    """kScanMaxPrims = 64: pile(64) is scanned (its scan kernels are compiled for the scene, as
    test_gpu_pair_filter.py reads it), pile(65) is not; the scan and the forced BVH walk of
    pile(64) return the same bits, and the scan matches the oracle."""
    s, rays, c = shapes.pile(64)
    with _renderer(s) as scan, _renderer(s, mode="bvh") as bvh:
        a, b = scan.trace(rays), bvh.trace(rays)
        scan.query(rays[:256], surface=False)
        bvh.query(rays[:256], surface=False)
        assert scan.last_stats["scan_rtc"] == 1 and bvh.last_stats["scan_rtc"] == 0
        assert _same_hits(a, b)
        _compare_hits(a, c, s, rays)
    s65, rays65, _ = shapes.pile(65)
    with _renderer(s65) as r:
        r.query(rays65[:256], surface=False)
        assert r.last_stats["scan_rtc"] == 0


# ---------------------------------------------------------------- every kernel at stack 32
def _coverage(shapes, name):
    """Share of the pixels that see geometry, from the oracle's `normals` image."""
    _, img = shapes.render_scene(name, "normals")
    return float((img.sum(-1) > 0).mean())


@pytest.mark.parametrize("fuse", ["0", "1"])
def test_path_mis_at_stack_32(shapes, fuse):
    """k_extend + k_shadow (NORI_TRACE_FUSE=0) or k_trace_both (1), and k_finish, instantiated <32>."""
    s, cpu = shapes.render_scene("d26", "path_mis")
    assert 24 <= nori_amd.bvh_info(s)["depth"] <= 26
    assert _coverage(shapes, "d26") >= 0.25 and float(cpu.mean()) > 0
    with _renderer(s, fuse=fuse) as r:
        gpu = nori_amd.develop(s, r.render())
        st = r.last_stats
    assert st["samples"] == s.width * s.height * s.spp and st["rays_shadow"] > 0 and st["bvh_depth"] >= 24
    assert np.isfinite(gpu).all() and float(gpu.mean()) > 0
    p = image_parity(gpu, cpu)
    print(f"d26 path_mis, fused trace {fuse}: {p}, mean {gpu.mean():.4f}")
    assert_parity(p)


def test_normals_features_and_queries_at_stack_32(shapes):
    """k_direct (`normals` render against the oracle's), k_features (normals bit-equal to the
    `normals` integrator's film statistics, as test_gpu_features.py) and k_trace through
    query(camera_rays()) against trace() and the oracle."""
    sn, cpu = shapes.render_scene("d26", "normals")
    sp, _ = shapes.render_scene("d26", "path_mis")
    assert _coverage(shapes, "d26") >= 0.25
    stat = np.zeros((sn.height, sn.width, 8), np.float32)
    with _renderer(sn) as r:
        gpu = nori_amd.develop(sn, r.render())
        r.render(passes=1, variance=stat, pass_begin=2)
        assert r.last_stats["bvh_depth"] >= 24
    assert_parity(image_parity(gpu, cpu))
    with _renderer(sp) as r:
        feat = r.features(passes=1, pass_begin=2)
        rays = r.camera_rays(passes=2).reshape(-1, 8)
        q, t = r.query(rays), r.trace(rays)
    assert not np.isnan(feat).any() and not np.isnan(stat).any()
    assert np.array_equal(np.abs(feat[..., 3:6]), stat[..., 0:3]) and np.array_equal(feat[..., 7], stat[..., 6])
    assert (np.abs(feat[..., 3:6]).sum(-1) > 0).mean() >= 0.25
    assert _same_hits(q["hits"], t)
    hit = np.isfinite(t["t"])
    assert np.array_equal(_bits(q["surf"]["t"][hit]), _bits(t["t"][hit])) and np.array_equal(q["surf"]["prim"][hit], t["prim"][hit])
    _compare_hits(t, pyoracle.OracleScene(sp).trace(rays), sp, rays)
    assert np.isfinite(t["t"]).mean() >= 0.25


def test_photonmapper_at_stack_32(shapes):
    """k_photons and k_direct's photon gather, at test_gpu_photon_map.py's bars."""
    s, cpu = shapes.render_scene("d26", "photonmapper")
    assert 24 <= nori_amd.bvh_info(s)["depth"] <= 26 and float(cpu.mean()) > 0
    with _renderer(s) as r:
        gpu = nori_amd.develop(s, r.render())
        assert r.last_stats["samples"] == s.width * s.height * s.spp
    l2 = float(np.mean((gpu - cpu) ** 2))
    close = float(np.mean(np.abs(gpu - cpu) <= 1e-4 * np.maximum(np.abs(cpu), 1.0)))
    print(f"d26 photonmapper: L2 {l2:.3e}, cells within 1e-4 rel {close:.4f}, means {gpu.mean():.4f} / {cpu.mean():.4f}")
    assert np.isfinite(gpu).all() and l2 < 1e-7 and close > 0.99


def test_stack_8_renders_the_default_image(shapes):
    """The spill path under a whole render: the same samples, so the same image up to the order
    of the film sums (the bar of test_gpu_parity.test_plane_cull_same_hits)."""
    s, cpu = shapes.render_scene("d22", "path_mis")
    assert nori_amd.bvh_info(s)["depth"] <= 22
    with _renderer(s) as r:
        a = r.render()
    with _renderer(s, stack=8) as r:
        b = r.render()
    assert np.allclose(a, b, rtol=1e-5, atol=1e-6), np.abs(a - b).max()
    assert float(a[..., :3].mean()) > 0
    assert_parity(image_parity(nori_amd.develop(s, b), cpu))


# ---------------------------------------------------------------- limits
def _cbox_still_works():
    s = nori_amd.load_scene(scene_path("pa4", "cbox", "cbox_path_mis.xml"), 32, 32, 1)
    rays = _rays(4000, 31, [-0.9, 0.05, -0.9], [0.9, 1.5, 0.9])
    with nori_amd.GpuRenderer(s, 0) as r:
        _compare_hits(r.trace(rays), pyoracle.OracleScene(s).trace(rays), s, rays)


@pytest.mark.parametrize("name,stack", [("d27", None), ("d27", 32), ("d23", 8)])
def test_too_deep_is_refused(shapes, name, stack):
    """A tree the stack cannot hold is refused at creation (nothing is uploaded or launched
    for it) with NORI_ERR_UNSUPPORTED, and the process goes on working."""
    s, info, _ = shapes.nest(name)
    assert info["depth"] >= 27 or (stack == 8 and info["depth"] == 23)
    with pytest.raises(nori_amd.NoriError, match="traversal stack") as e:
        _renderer(s, stack)
    assert e.value.code == _abi.NORI_ERR_UNSUPPORTED
    _cbox_still_works()
    if name == "d23":  # accepted without the override
        with _renderer(s) as r:
            r.query(shapes.nest(name)[2][0][0][:256], surface=False)
            assert r.last_stats["bvh_depth"] == 23
