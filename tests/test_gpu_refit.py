"""Dynamic geometry on the GPU: nori_gpu_update_vertices (refit.hip) against the refit's host
statement (nori_scene_bvh_refit, itself tied to an independent numpy statement in test_refit.py)
byte for byte, and an updated context against a context created fresh on the same positions --
never a kernel against itself.

Hit distances and barycentrics depend on the triangle record alone, so a refitted tree must give
the same bits as a freshly built one; which of two primitives with the same t a ray reports may
differ with the tree, and is then proven a tie ray by ray (nori_test_util.prim_hit).

Every context is created with NORI_TRAVERSAL=bvh (scan-mode contexts are refused, which
test_refusals_change_nothing checks).  All inputs are finite except in the refusal cases, which
are rejected before anything is launched on the scene.
"""
import contextlib
import os

import numpy as np
import pytest

import bvh_shapes
import nori_amd
import refit_util as ru
from conftest import scene_path
from nori_amd import _abi
from nori_test_util import assert_parity, image_parity, prim_hit
from test_gpu_parity import _rays
from test_query import NMAP, scene_rays

pytestmark = pytest.mark.gpu


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


def _renderer(scene, mode="bvh", stack=None):
    with _env(NORI_TRAVERSAL=mode, NORI_BVH_STACK=stack):
        return nori_amd.GpuRenderer(scene, 0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _rows(records):
    """A structured array (hits, hit records) as one row of uint32 words per record."""
    return _bits(records).reshape(len(records), -1)


class _Cases:
    """Scenes, position sets and host statements, made once per module and only read."""

    def __init__(self, outdir):
        self.outdir = outdir
        self._scene, self._pos, self._host = {}, {}, {}

    def scene(self, which):
        if which not in self._scene:
            self._scene[which] = ru.load(which, self.outdir)
        return self._scene[which]

    def positions(self, which, pset):
        if (which, pset) not in self._pos:
            self._pos[which, pset] = ru.position_set(self.scene(which), pset)
        return self._pos[which, pset]

    def host(self, which, pset):
        """nori_amd.bvh_refit of the scene to a position set (None: as built)."""
        if (which, pset) not in self._host:
            P = None if pset is None else self.positions(which, pset)
            self._host[which, pset] = nori_amd.bvh_refit(self.scene(which), P)
        return self._host[which, pset]

    def fresh(self, which, P, normals=None):
        """The scene loaded again with its vertices at P: a context on it is built from scratch."""
        return ru.load(which, self.outdir, P, normals)


@pytest.fixture(scope="module")
def cases(built, tmp_path_factory):
    return _Cases(str(tmp_path_factory.mktemp("refit_gpu")))


def _assert_tree(r, want, what):
    nodes, prims = r.bvh_nodes()
    assert ru.same_bits(prims, want[1]), (what, "records")
    assert ru.same_bits(nodes, want[0]), (what, "nodes")


# ---------------------------------------------------------------- 1. bytes
@pytest.mark.parametrize("which", ru.SCENES)
def test_tree_equals_the_host_statement(cases, which):
    """As created, then after update(b), update(c), update(d), update(a) in sequence on one
    context: the device tree is the host statement's, byte for byte, each time; after the last
    it is the tree as created again (the refit has no memory)."""
    s = cases.scene(which)
    with _renderer(s) as r:
        _assert_tree(r, cases.host(which, None), "as created")
        for pset in ("b", "c", "d", "a"):
            st = r.update_vertices(cases.positions(which, pset))
            want = cases.host(which, pset)
            _assert_tree(r, want, pset)
            assert np.array_equal(_bits(np.array(st["root_min"] + st["root_max"], np.float32)), _bits(want[2])), pset
            assert st["nodes"] == len(want[0]) and 1 <= st["levels"] <= nori_amd.bvh_info(s)["depth"]
            # one counting pass, the vertices, the records, one launch per level
            assert st["launches"] == st["levels"] + 3 and st["ms"] > 0 and st["ms_device"] > 0
        _assert_tree(r, cases.host(which, None), "back at the loaded positions")
        print(f"{which}: {st['nodes']} nodes, {st['levels']} refit launches of {st['launches']}, "
              f"last update {st['ms']:.3f} ms ({st['ms_device']:.3f} ms on the device)")


def test_update_from_device_memory(cases):
    """The height field from a torch tensor on the device and from a raw device address."""
    torch = pytest.importorskip("torch")
    s = cases.scene("hf")
    with _renderer(s) as r:
        for pset in ("c", "b"):
            P = cases.positions("hf", pset)
            d = torch.from_numpy(P).to("cuda:0")
            r.update_vertices(d)
            _assert_tree(r, cases.host("hf", pset), pset)
            assert np.array_equal(_bits(d.cpu().numpy()), _bits(P))     # the input is only read
        d = torch.from_numpy(cases.positions("hf", "d")).to("cuda:0")
        torch.cuda.synchronize()
        r.update_vertices(d.data_ptr())
        _assert_tree(r, cases.host("hf", "d"), "raw address")
        with pytest.raises(ValueError):
            r.update_vertices(d[:-1])
        with pytest.raises(ValueError):
            r.update_vertices(d.double())
        with pytest.raises(ValueError):
            r.update_vertices(d.cpu())


# ---------------------------------------------------------------- 2. rays against a fresh context
def _case_rays(which, pset, fresh_scene, r):
    """About 4,000 rays: the renderer's own camera rays, then the scene's generator."""
    cam = r.camera_rays(passes=1).reshape(-1, 8)
    lo, hi = ru.used_box(fresh_scene)
    pad = 0.1 * (hi - lo)
    if which == "nest":
        gen = bvh_shapes.nest_rays(*bvh_shapes.NESTS["d26"], 2000, 31, 1e-4, beyond=400)
    elif which == "pile":
        gen = np.concatenate([_rays(3000, 32, lo - pad, hi + pad), bvh_shapes.pile_edge_rays(10)])
    else:
        gen = _rays(3000, 33, lo - pad, hi + pad)   # uniform origins and directions, a tenth axis-aligned
    rays = np.concatenate([cam, gen]).astype(np.float32)
    sh = rays.copy()   # occlusion: maxt around the origin's own scale
    sh[:, 7] = (np.random.default_rng(34).uniform(0.01, 2.0, size=len(rays)) * np.abs(rays[:, :3]).max(axis=1))
    return rays, sh


def _same_answers(a, b, scene, rays):
    """Closest hits a, b of two trees over one geometry: t bit-equal; where the primitive is the
    same, u and v bit-equal; where it differs the two primitives tie -- the ray against each of
    them alone (numpy fp32, the kernels' operation order) hits at the reported t bit for bit.
    Returns the number of ties."""
    assert np.array_equal(_bits(a["t"]), _bits(b["t"]))
    same = a["prim"] == b["prim"]
    for k in ("u", "v"):
        assert np.array_equal(_bits(a[k])[same], _bits(b[k])[same]), k
    diff = np.flatnonzero(~same)
    assert np.isfinite(a["t"][diff]).all()
    for side in (a, b):
        hit, t, _, _ = prim_hit(scene, rays[diff], side["prim"][diff])
        assert (hit & (_bits(t) == _bits(a["t"][diff]))).all(), "the primitives differ and do not tie"
    return int(diff.size)


def _compare_contexts(A, B, fresh_scene, rays, sh, what):
    a, b = A.trace(rays), B.trace(rays)
    ties = _same_answers(a, b, fresh_scene, rays)
    assert np.array_equal(A.trace(sh, any_hit=True)["prim"] >= 0, B.trace(sh, any_hit=True)["prim"] >= 0)
    qa, qb = A.query(rays), B.query(rays)
    assert np.array_equal(_bits(qa["hits"]), _bits(a)) and np.array_equal(_bits(qb["hits"]), _bits(b))
    same = a["prim"] == b["prim"]
    assert np.array_equal(_rows(qa["surf"])[same], _rows(qb["surf"])[same])
    hit = np.isfinite(a["t"])
    print(f"{what}: {len(rays)} rays, hit share {hit.mean():.3f}, {len(np.unique(a['prim'][hit]))} primitives hit, "
          f"ties {ties}")
    return a


@pytest.mark.parametrize("pset", ["b", "c"])
@pytest.mark.parametrize("which", ["hf", "nest", "pile"])
def test_rays_equal_a_fresh_context(cases, which, pset):
    s, P = cases.scene(which), cases.positions(which, pset)
    fs = cases.fresh(which, P)
    with _renderer(s) as A, _renderer(fs) as B:
        rays, sh = _case_rays(which, pset, fs, B)
        before = A.trace(rays)
        A.update_vertices(P)
        assert np.array_equal(_bits(A.camera_rays(passes=1)), _bits(B.camera_rays(passes=1)))
        a = _compare_contexts(A, B, fs, rays, sh, f"{which} ({pset})")
    hit = np.isfinite(a["t"])
    # the rays see the geometry, and the geometry moved
    assert hit.mean() >= 0.05 and len(np.unique(a["prim"][hit])) >= 20
    assert not np.array_equal(_bits(before["t"]), _bits(a["t"]))


def test_every_stack_that_accepts_the_deepest_tree(cases):
    """nest d26 needs 3 * 26 + 1 = 79 stack entries; NORI_BVH_STACK = 8, 16, 32 hold 4, 8, 16 in
    LDS and 64 more in private memory (scene_plan.cpp bvh_stack_for), so only 32 accepts it."""
    s, P = cases.scene("nest"), cases.positions("nest", "b")
    need = 3 * nori_amd.bvh_info(s)["depth"] + 1
    accepted = [k for k in (8, 16, 32) if need <= k // 2 + 64]
    assert accepted == [32]
    fs = cases.fresh("nest", P)
    for stack in accepted:
        with _renderer(s, stack=stack) as A, _renderer(fs, stack=stack) as B:
            rays, sh = _case_rays("nest", "b", fs, B)
            A.update_vertices(P)
            _compare_contexts(A, B, fs, rays, sh, f"nest (b), stack {stack}")


def test_normals_and_texture_coordinates(built, cases):
    """The normal-mapped scene (meshes with normals and uvs): update(P) keeps the normals and the
    uvs (the w lanes of pos / nrm), update(P, N) sets the normals; the records are a fresh context's."""
    s = nori_amd.load_scene(scene_path(*NMAP), 32, 32, 1)
    assert any(sh.has_normals for sh in s.shapes()) and any(sh.has_uvs for sh in s.shapes())
    rays = scene_rays("nmap", s, 4000)
    P = ru.position_set(s, "b")
    N = np.random.default_rng(8).normal(size=P.shape)
    N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(np.float32)

    def fresh(normals):
        f = nori_amd.load_scene(scene_path(*NMAP), 32, 32, 1)
        n = f.desc.num_vertices
        np.ctypeslib.as_array(f.desc.positions, shape=(n, 3))[:] = P
        if normals is not None:
            np.ctypeslib.as_array(f.desc.normals, shape=(n, 3))[:] = normals
        return f

    ns = []
    with _renderer(s) as A:
        for normals in (None, N):
            A.update_vertices(P, normals)
            f = fresh(normals)
            with _renderer(f) as B:
                a, b = A.query(rays), B.query(rays)
            _same_answers(a["hits"], b["hits"], f, rays)
            same = a["hits"]["prim"] == b["hits"]["prim"]
            assert same.mean() > 0.99 and np.array_equal(_rows(a["surf"])[same], _rows(b["surf"])[same])
            mapped = np.array([sh.has_normals != 0 for sh in s.shapes()] + [False])[a["surf"]["shape"]]
            assert mapped.mean() >= 0.01
            ns.append(a["surf"]["ns"][mapped])
    assert not np.array_equal(_bits(ns[0]), _bits(ns[1]))     # the new normals are used


# ---------------------------------------------------------------- 3. lights
def test_lights_follow_the_geometry(cases):
    """The height field's two-triangle area light, path_mis, 32 x 32 at 4 spp: one light vertex moved
    (the ratio of the two areas changes: the CDF), then the whole light scaled by 1.5 (the
    normalisation).  The updated context's film meets the parity bars against a fresh context's
    each time; without the update it does not."""
    s = cases.scene("hf")
    light = [sh for sh in s.shapes() if sh.emitter >= 0]
    assert len(light) == 1 and light[0].tri_count == 2
    v0, nv = light[0].vtx_offset, light[0].vtx_count
    P1 = s.positions()
    P1[v0 + 1] += np.float32([0.25, 0.0, 0.2])     # in the light's plane (y = const); a corner of one triangle only
    P2 = P1.copy()
    c = P2[v0:v0 + nv].mean(0)
    P2[v0:v0 + nv] = c + np.float32(1.5) * (P2[v0:v0 + nv] - c)
    idx = s.indices()[light[0].tri_offset:light[0].tri_offset + 2]

    def areas(P):
        e1, e2 = P[idx[:, 1]] - P[idx[:, 0]], P[idx[:, 2]] - P[idx[:, 0]]
        return 0.5 * np.linalg.norm(np.cross(e1, e2), axis=1)

    a0, a1, a2 = areas(s.positions()), areas(P1), areas(P2)
    assert abs(a1[0] / a1[1] - a0[0] / a0[1]) > 0.1 and abs(a2.sum() / a1.sum() - 2.25) < 1e-3
    with _renderer(s) as A:
        stale = nori_amd.develop(s, A.render())
        for name, P in (("one vertex moved", P1), ("scaled by 1.5", P2)):
            fs = cases.fresh("hf", P)
            with _renderer(fs) as B:
                want = nori_amd.develop(fs, B.render())
            if name == "one vertex moved":   # the control: the test sees the geometry
                p = image_parity(stale, want)
                print(f"light, {name}, NOT updated: {p}")
                with pytest.raises(AssertionError):
                    assert_parity(p)
            A.update_vertices(P)
            got = nori_amd.develop(s, A.render())
            p = image_parity(got, want)
            print(f"light, {name}: {p}, bit-equal: {np.array_equal(_bits(got), _bits(want))}")
            assert float(got.mean()) > 0
            assert_parity(p)


# ---------------------------------------------------------------- 4. features and adaptive rounds
def test_features_and_adaptive_on_the_updated_geometry(cases):
    s, P = cases.scene("hf"), cases.positions("hf", "b")
    fs = cases.fresh("hf", P)
    with _renderer(s) as A, _renderer(fs) as B:
        old = A.features(passes=16)
        A.update_vertices(P)
        fa, fb = A.features(passes=16), B.features(passes=16)
        assert np.array_equal(_bits(fa), _bits(fb))        # albedo, normal and depth sums, counts
        assert not np.array_equal(_bits(old[..., 3:7]), _bits(fa[..., 3:7]))
        assert (fa[..., 7] == 16).all() and (np.abs(fa[..., 3:6]).sum(-1) > 0).mean() > 0.5
        ra, pa, _ = A.render_adaptive(0.0, min_passes=2, max_passes=4)
        rb, pb, _ = B.render_adaptive(0.0, min_passes=2, max_passes=4)
    assert (pa == 4).all() and (pb == 4).all()
    assert_parity(image_parity(nori_amd.develop(s, ra), nori_amd.develop(fs, rb)))


# ---------------------------------------------------------------- 5. refusals
def _state(r, rays):
    """What a context computes, in reproducible form: the tree's bytes, closest hits, feature
    sums (bitwise reproducible by construction) and a 16 x 16 render."""
    return r.bvh_nodes(), r.trace(rays), r.features(passes=2), r.render()


def _assert_unchanged(r, rays, before, what):
    """Byte-identical tree, hits and feature sums.  The film is compared as closely as two
    renders of one context can be: its sums are float atomics whose order varies from run to run
    (the bar of test_gpu_bvh_shapes.test_stack_8_renders_the_default_image)."""
    (n0, p0), h0, f0, film0 = before
    (n1, p1), h1, f1, film1 = _state(r, rays)
    assert ru.same_bits(n0, n1) and ru.same_bits(p0, p1), what
    assert np.array_equal(_bits(h0), _bits(h1)) and np.array_equal(_bits(f0), _bits(f1)), what
    assert np.allclose(film0, film1, rtol=1e-5, atol=1e-6), (what, np.abs(film0 - film1).max())


def _refused(r, code, positions, normals=None, **fields):
    ud = _abi.UpdateDesc()
    keep = [np.ascontiguousarray(positions, np.float32)] if isinstance(positions, np.ndarray) else []
    ud.positions = keep[0].ctypes.data if keep else positions
    ud.num_vertices = r.scene.desc.num_vertices
    for k, v in fields.items():
        setattr(ud, k, v)
    import ctypes as C

    assert nori_amd.lib().nori_gpu_update_vertices(r._h, C.byref(ud), None) == code
    return nori_amd.lib().nori_gpu_last_error().decode()


def test_refusals_change_nothing(built, tmp_path):
    import ctypes as C

    cbox = nori_amd.load_scene(scene_path("pa4", "cbox", "cbox_path_mis.xml"), 16, 16, 2)
    rays = scene_rays("cbox", cbox, 500)
    P = ru.position_set(cbox, "b")
    # a scan-mode context
    with _renderer(cbox, mode=None) as r:
        before = _state(r, rays)
        with pytest.raises(nori_amd.NoriError, match="NORI_TRAVERSAL=bvh") as e:
            r.update_vertices(P)
        assert e.value.code == _abi.NORI_ERR_UNSUPPORTED
        _assert_unchanged(r, rays, before, "scan mode")
    # a photonmapper context
    import synth

    pm = nori_amd.load_scene(synth.cbox_variant(
        str(tmp_path), "pm", integrator="photonmapper", width=16, height=16,
        integrator_props='<integer name="photonCount" value="2000"/><float name="photonRadius" value="0.05"/>'), 0, 0, 2)
    with _renderer(pm) as r:
        before = _state(r, rays)
        with pytest.raises(nori_amd.NoriError, match="photon") as e:
            r.update_vertices(ru.position_set(pm, "b"))
        assert e.value.code == _abi.NORI_ERR_UNSUPPORTED
        _assert_unchanged(r, rays, before, "photonmapper")
    # bad arguments on a context that accepts updates
    with _renderer(cbox) as r:
        before = _state(r, rays)
        bad = P.copy()
        bad[5, 2] = np.nan
        inf_n = np.zeros_like(P)
        inf_n[0, 0] = np.inf
        assert "non-finite" in _refused(r, _abi.NORI_ERR_INVALID, bad)
        with pytest.raises(nori_amd.NoriError) as e:
            r.update_vertices(P, inf_n)
        assert e.value.code == _abi.NORI_ERR_INVALID
        _refused(r, _abi.NORI_ERR_INVALID, P, num_vertices=len(P) - 1)
        _refused(r, _abi.NORI_ERR_INVALID, P, num_vertices=len(P) + 1)
        _refused(r, _abi.NORI_ERR_INVALID, P, reserved=(C.c_uint32 * 4)(0, 0, 0, 1))
        _refused(r, _abi.NORI_ERR_INVALID, None)
        assert nori_amd.lib().nori_gpu_update_vertices(r._h, None, None) == _abi.NORI_ERR_INVALID
        assert nori_amd.lib().nori_gpu_update_vertices(None, None, None) == _abi.NORI_ERR_INVALID
        host_as_device = np.ascontiguousarray(P)
        _refused(r, _abi.NORI_ERR_INVALID, host_as_device, on_device=1)   # not device memory: nothing launched
        _assert_unchanged(r, rays, before, "bad arguments")
        torch = pytest.importorskip("torch")
        d = torch.from_numpy(bad).to("cuda:0")
        with pytest.raises(nori_amd.NoriError, match="non-finite") as e:
            r.update_vertices(d)
        assert e.value.code == _abi.NORI_ERR_INVALID
        _refused(r, _abi.NORI_ERR_INVALID, d.data_ptr() + 2, on_device=1)  # misaligned
        _assert_unchanged(r, rays, before, "a NaN in a device tensor")
        # the process goes on working: the same context takes a valid update
        r.update_vertices(P)
        _assert_tree(r, nori_amd.bvh_refit(cbox, P), "after the refusals")
        assert not np.array_equal(_bits(r.trace(rays)["t"]), _bits(before[1]["t"]))


# ---------------------------------------------------------------- the example
def test_deform_example(built):
    import importlib.util

    from conftest import ROOT

    torch = pytest.importorskip("torch")
    spec = importlib.util.spec_from_file_location("deform_torch", os.path.join(ROOT, "examples", "deform_torch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    s = nori_amd.load_scene(scene_path("pa4", "cbox", "cbox_path_mis.xml"), 32, 32, 1)
    with _renderer(s) as r:
        frames = mod.deform_frames(r, frames=3)
    assert len(frames) == 3
    for f in frames:
        assert f.is_cuda and f.shape == (32, 32, 3) and f.dtype == torch.float32 and bool(torch.isfinite(f).all())
    assert not torch.equal(frames[0], frames[2]) and float(frames[0].abs().sum()) > 0
