"""Ray queries with full hit records (nori_gpu_query, k_surface) and the renderer's primary rays
(nori_gpu_camera_rays, k_camera_rays) on the GPU.

Hits are checked against nori_gpu_trace bit for bit, records against the host statement
(nori_scene_surface, itself checked against a numpy float64 restatement in test_query.py), and
camera rays + query against the feature pass, which the existing tests tie to the `normals`
integrator: never a kernel against itself."""
import importlib.util
import os

import numpy as np
import pytest

import nori_amd
import synth
from conftest import ROOT, scene_path
from nori_amd import _abi
from test_query import CBOX, NMAP, hit_shares, scene_rays, sphere_uv

pytestmark = pytest.mark.gpu

COUNTS = [1, 127, 128, 129, 257, 1000]   # kTraceBlock = 128
THINLENS = '<float name="lensRadius" value="0.08"/><float name="focalDist" value="4.8"/>'
CHROMA = ('<float name="lensRadius" value="0.05"/><float name="focalDist" value="5"/>'
          '<vector name="chromaticAberation" value="4, 2, 3.3"/>')
# Sphere uv: device acosf / atan2f against libm.  Measured on these inputs (both scenes, the three
# traversal modes, every count): the largest difference is 1.192e-7 = 2^-23, one ulp of a value in
# [1, 2) (uv.y = phi / pi reaches 2); the bound is twice that.
SPHERE_UV_TOL = 2.0 ** -22


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _renderer(scene, mode=None):
    """GpuRenderer with a forced traversal mode ('scan' or 'bvh'; None = automatic), as test_gpu_parity.py."""
    old = os.environ.get("NORI_TRAVERSAL")
    if mode:
        os.environ["NORI_TRAVERSAL"] = mode
    try:
        return nori_amd.GpuRenderer(scene, 0)
    finally:
        if old is None:
            os.environ.pop("NORI_TRAVERSAL", None)
        else:
            os.environ["NORI_TRAVERSAL"] = old


def _chunked(n):
    """NORI_QUERY_CHUNK=256 around the n = 1000 case: four staging chunks, the last one partial."""
    class Ctx:
        def __enter__(self):
            self.old = os.environ.get("NORI_QUERY_CHUNK")
            if n == 1000:
                os.environ["NORI_QUERY_CHUNK"] = "256"

        def __exit__(self, *a):
            if self.old is None:
                os.environ.pop("NORI_QUERY_CHUNK", None)
            else:
                os.environ["NORI_QUERY_CHUNK"] = self.old
    return Ctx()


@pytest.fixture(scope="module", params=["cbox", "nmap"])
def scene_and_rays(request, built):
    which = request.param
    scene = nori_amd.load_scene(scene_path(*(CBOX if which == "cbox" else NMAP)), 32, 32, 1)
    return which, scene, scene_rays(which, scene, 1000)


# ---------------------------------------------------------------- hits and records
@pytest.mark.parametrize("mode", [None, "scan", "bvh"])
def test_hits_equal_trace_and_records_equal_the_host_statement(scene_and_rays, mode):
    which, scene, rays = scene_and_rays
    sph = np.array([sh.type == _abi.SHAPE_SPHERE for sh in scene.shapes()] + [False])
    worst_uv = 0.0
    with _renderer(scene, mode) as r:
        for n in COUNTS:
            rn = rays[:n]
            closest, anyhit = r.trace(rn), r.trace(rn, any_hit=True)
            with _chunked(n):
                q = r.query(rn)
                qa = r.query(rn, any_hit=True)
                qh = r.query(rn, surface=False)
            st = r.last_stats
            assert set(q) == {"hits", "surf"} and set(qa) == {"hits"} and set(qh) == {"hits"}
            assert np.array_equal(_bits(q["hits"]), _bits(closest)), n
            assert np.array_equal(_bits(qh["hits"]), _bits(closest)), n
            assert np.array_equal(_bits(qa["hits"]), _bits(anyhit)), n
            assert st["rays_closest"] == n and st["rays_shadow"] == 0 and st["ms_total"] > 0
            if n == 1000:  # the conditions of test_query.py: the batch is not mostly misses
                share, sphere_share, mapped_share = hit_shares(scene, closest)
                assert share >= 0.5 and sphere_share >= 0.01, (share, sphere_share)
                if which == "nmap":
                    assert mapped_share >= 0.01, mapped_share
            got, want = q["surf"], nori_amd.scene_surface(scene, rn, closest)
            for k in ("t", "prim", "shape", "bary"):
                assert np.array_equal(_bits(got[k]), _bits(want[k])), (n, k)
            # the same fp32 operations on both sides, contraction off: bit equality
            for k in ("p", "ng", "ns"):
                assert np.array_equal(_bits(got[k]), _bits(want[k])), (n, k)
            s = sph[got["shape"]]
            assert np.array_equal(_bits(got["uv"][~s]), _bits(want["uv"][~s])), n
            if s.any():
                d = float(np.abs(got["uv"][s].astype(np.float64) - want["uv"][s]).max())
                worst_uv = max(worst_uv, d)
                # ... and against the float64 formula at the record's own normal (test_query.py's bound)
                assert np.abs(got["uv"][s] - sphere_uv(got["ns"][s].astype(np.float64))).max() <= 2e-6
    print(f"{which} {mode}: sphere uv, device against libm: max difference {worst_uv:.3e}")
    assert worst_uv <= SPHERE_UV_TOL <= 2e-6


def test_both_store_variants_of_k_surface_agree(scene_and_rays):
    """The records through the LDS transpose (the default) and through per-lane stores (NORI_SURFACE_STORE)."""
    which, scene, rays = scene_and_rays
    got = {}
    with nori_amd.GpuRenderer(scene, 0) as r:
        for variant in ("lds", "direct"):
            os.environ["NORI_SURFACE_STORE"] = variant
            try:
                got[variant] = [r.query(rays[:n])["surf"] for n in COUNTS]
            finally:
                os.environ.pop("NORI_SURFACE_STORE")
        default = [r.query(rays[:n])["surf"] for n in COUNTS]
        hits = r.trace(rays)
    want = nori_amd.scene_surface(scene, rays, hits)
    for a, b, c, n in zip(got["lds"], got["direct"], default, COUNTS):
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c)), n
        for k in ("p", "ng", "ns", "t", "prim", "shape", "bary"):
            assert np.array_equal(_bits(a[k]), _bits(want[k][:n])), (n, k)


# ---------------------------------------------------------------- camera rays
@pytest.mark.parametrize("camera", ["perspective", "thinlens", "chroma"])
def test_camera_rays_are_the_renderers(built, tmp_path, camera):
    """query(camera_rays()) accumulated per pixel in pass order equals the feature pass bit for bit."""
    kw = {"perspective": {}, "thinlens": dict(camera_type="thinlens", camera_props=THINLENS),
          "chroma": dict(camera_type="advancedCamera", camera_props=CHROMA)}[camera]
    s = nori_amd.load_scene(synth.cbox_variant(str(tmp_path), "p", integrator="path_mis", width=96, height=72, **kw),
                            0, 0, 1)
    with nori_amd.GpuRenderer(s, 0) as r:
        feat = r.features(passes=3, pass_begin=2)
        rays = r.camera_rays(passes=3, pass_begin=2)
        assert rays.shape == (3, 72, 96, 8) and rays.dtype == np.float32
        surf = r.query(rays.reshape(-1, 8))["surf"].reshape(3, 72, 96)
    acc = np.zeros((72, 96, 4), np.float32)
    for k in range(3):
        hit = surf["prim"][k] >= 0
        acc[..., 0:3] += surf["ns"][k]                                   # zero on a miss
        acc[..., 3] += np.where(hit, surf["t"][k], np.float32(0))        # (t is +inf on a miss)
    assert (feat[..., 7] == 3).all()
    assert (surf["prim"] >= 0).mean() > 0.5
    assert np.array_equal(_bits(acc), _bits(feat[..., 3:7]))


def test_camera_rays_pass_and_block_invariance(built):
    s = nori_amd.load_scene(scene_path(*CBOX), 96, 72, 8)   # 3 x 3 blocks
    assert s.num_blocks() >= 6
    with nori_amd.GpuRenderer(s, 0) as r:
        whole = r.camera_rays(passes=5, pass_begin=0, seed=7)
        part = r.camera_rays(passes=3, pass_begin=2, seed=7)
        assert np.array_equal(_bits(part), _bits(whole[2:5]))
        assert not np.array_equal(whole[0], whole[1])
        assert not np.array_equal(whole, r.camera_rays(passes=5, pass_begin=0, seed=8))
        # pass_count 0 means the scene's sampleCount
        assert r.camera_rays(passes=0).shape == r.camera_rays().shape == (8, 72, 96, 8)
        sentinel = np.float32(-12345.0)
        out = np.full((5, 72, 96, 8), sentinel, np.float32)
        got = r.camera_rays(passes=5, pass_begin=0, seed=7, blocks=[1, 4], out=out)
        assert got is out
    inside = np.zeros((72, 96), bool)
    for b in (1, 4):
        by, bx = divmod(b, 3)
        inside[32 * by:32 * by + 32, 32 * bx:32 * bx + 32] = True
    changed = (out != sentinel).any(-1)
    assert np.array_equal(changed, np.broadcast_to(inside, changed.shape))
    assert np.array_equal(_bits(out[:, inside]), _bits(whole[:, inside]))
    assert (out[:, ~inside] == sentinel).all()


# ---------------------------------------------------------------- device buffers
def test_device_buffers_torch(scene_and_rays):
    torch = pytest.importorskip("torch")
    which, scene, rays = scene_and_rays
    with nori_amd.GpuRenderer(scene, 0) as r:
        for n in (129, 1000):
            host = r.query(rays[:n])
            host_any = r.query(rays[:n], any_hit=True)["hits"]
            d_rays = torch.from_numpy(rays[:n]).to("cuda:0")
            d_hits = torch.full((n, 4), 7.0, dtype=torch.float32, device="cuda:0")
            d_surf = torch.full((n, 16), 7.0, dtype=torch.float32, device="cuda:0")
            d_only = torch.full((n, 16), 7.0, dtype=torch.float32, device="cuda:0")
            d_any = torch.full((n, 4), 7.0, dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            assert r.query(d_rays.data_ptr(), n=n, hits_out=d_hits.data_ptr(), surf_out=d_surf.data_ptr()) is None
            r.query(d_rays.data_ptr(), n=n, surf_out=d_only.data_ptr())       # the context's own hit buffer
            r.query(d_rays.data_ptr(), n=n, any_hit=True, hits_out=d_any.data_ptr())
            assert np.array_equal(_bits(d_hits.cpu().numpy()), _bits(host["hits"]).reshape(n, 4))
            assert np.array_equal(_bits(d_surf.cpu().numpy()), _bits(host["surf"]).reshape(n, 16))
            assert np.array_equal(_bits(d_only.cpu().numpy()), _bits(host["surf"]).reshape(n, 16))
            assert np.array_equal(_bits(d_any.cpu().numpy()), _bits(host_any).reshape(n, 4))
            assert np.array_equal(d_rays.cpu().numpy(), rays[:n])
        # a pointer that is not 16-byte aligned: refused, nothing launched
        for kw in (dict(rays=d_rays.data_ptr() + 4, hits_out=d_hits.data_ptr()),
                   dict(rays=d_rays.data_ptr(), hits_out=d_hits.data_ptr() + 4),
                   dict(rays=d_rays.data_ptr(), surf_out=d_surf.data_ptr() + 4)):
            with pytest.raises(nori_amd.NoriError) as e:
                r.query(kw.pop("rays"), n=16, **kw)
            assert e.value.code == _abi.NORI_ERR_INVALID
        with pytest.raises(ValueError):
            r.query(d_rays.data_ptr(), hits_out=d_hits.data_ptr())   # n is required


def test_camera_rays_to_query_on_the_device(built):
    """camera_rays(out=tensor) then query on that tensor, no host copy in between."""
    torch = pytest.importorskip("torch")
    s = nori_amd.load_scene(scene_path(*CBOX), 64, 48, 2)
    n = 2 * 48 * 64
    with nori_amd.GpuRenderer(s, 0) as r:
        d_rays = torch.zeros((2, 48, 64, 8), dtype=torch.float32, device="cuda:0")
        d_surf = torch.zeros((n, 16), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        assert r.camera_rays(passes=2, pass_begin=1, out=d_rays.data_ptr()) is None
        r.query(d_rays.data_ptr(), n=n, surf_out=d_surf.data_ptr())
        host_rays = r.camera_rays(passes=2, pass_begin=1)
        host = r.query(host_rays.reshape(-1, 8))["surf"]
        with pytest.raises(nori_amd.NoriError) as e:
            r.camera_rays(passes=2, out=d_rays.data_ptr() + 4)
        assert e.value.code == _abi.NORI_ERR_INVALID
    assert np.array_equal(_bits(d_rays.cpu().numpy()), _bits(host_rays))
    assert np.array_equal(_bits(d_surf.cpu().numpy()), _bits(host).reshape(n, 16))
    assert (host["prim"] >= 0).mean() > 0.5


# ---------------------------------------------------------------- argument errors
def test_argument_errors_leave_the_context_usable(built):
    import ctypes as C

    s = nori_amd.load_scene(scene_path(*CBOX), 32, 32, 2)
    rays = scene_rays("cbox", s, 64)
    hits = np.zeros(64, nori_amd.HIT_DTYPE)
    surf = np.zeros(64, nori_amd.SURFACE_DTYPE)
    pr, ph, ps = C.c_void_p(rays.ctypes.data), C.c_void_p(hits.ctypes.data), C.c_void_p(surf.ctypes.data)
    f = nori_amd.lib().nori_gpu_query
    with nori_amd.GpuRenderer(s, 0) as r:
        before = r.render()

        def call(qd, rays_p, hits_p, surf_p):
            return f(r._h, C.byref(qd), rays_p, hits_p, surf_p, None)

        assert call(_abi.QueryDesc(64, 1, 0, 0), pr, ph, ps) == _abi.NORI_ERR_INVALID     # any_hit with surf
        assert call(_abi.QueryDesc(64, 0, 0, 0), pr, None, None) == _abi.NORI_ERR_INVALID  # both outputs null
        assert call(_abi.QueryDesc(64, 0, 0, 1), pr, ph, ps) == _abi.NORI_ERR_INVALID      # reserved
        assert call(_abi.QueryDesc(64, 0, 0, 0), None, ph, ps) == _abi.NORI_ERR_INVALID    # null rays
        assert f(r._h, None, pr, ph, ps, None) == _abi.NORI_ERR_INVALID
        assert not hits.view(np.uint32).any() and not surf.view(np.uint32).any()           # nothing written
        assert call(_abi.QueryDesc(0, 0, 0, 0), pr, ph, ps) == _abi.NORI_OK                # n == 0: a no-op
        assert not hits.view(np.uint32).any()
        rd = _abi.RenderDesc()
        rd.pass_count = 1
        out = np.zeros((1, 32, 32, 8), np.float32)
        rd.variance_out = out.ctypes.data
        assert nori_amd.lib().nori_gpu_camera_rays(r._h, C.byref(rd), C.c_void_p(out.ctypes.data)) == _abi.NORI_ERR_INVALID
        assert not out.any()
        # the context works afterwards
        assert call(_abi.QueryDesc(64, 0, 0, 0), pr, ph, ps) == _abi.NORI_OK
        assert np.array_equal(_bits(hits), _bits(r.trace(rays)))
        assert np.allclose(r.render(), before, rtol=1e-4, atol=1e-4)  # (the film sums arrive in another order)


# ---------------------------------------------------------------- the example
def test_ao_example(built):
    torch = pytest.importorskip("torch")
    spec = importlib.util.spec_from_file_location("ao_torch", os.path.join(ROOT, "examples", "ao_torch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    s = nori_amd.load_scene(scene_path(*CBOX), 32, 32, 1)
    with nori_amd.GpuRenderer(s, 0) as r:
        ao = mod.ao_image(r, directions=4)
    assert ao.is_cuda and ao.shape == (32, 32) and ao.dtype == torch.float32
    img = ao.cpu().numpy()
    assert np.isfinite(img).all() and img.min() >= 0 and img.max() <= 1
    assert img.min() < img.max()
