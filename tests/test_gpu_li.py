"""nori_gpu_li on the GPU: Integrator::Li of the context's integrator along the caller's rays
(include/nori_gpu.h).  Its contract is exact, so every comparison here is equality of float values
(NaN equal to NaN): li of the renderer's own camera rays on the renderer's own streams is the
renderer's own sample; li of other rays is the composition of the public queries
(tests/li_compose.py); and a ray's value does not depend on where in a batch, a wave or a call it
is computed.  32 x 32 frames, at most 2 passes."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

import li_compose
import nori_amd
import refit_util
import synth
from conftest import ROOT, scene_path
from nori_amd import _abi
from test_gpu_query import THINLENS
from test_query import scene_rays

pytestmark = pytest.mark.gpu

W = H = 32
N = W * H
SEED = 11
CBOX = ("pa4", "cbox", "cbox_path_mis.xml")
VEACH = ("pa3", "veach_mi", "veach_mis.xml")
# the cases of test 1: name -> (scene, traversal mode).  The CPU oracle drops no sample of any of
# them at this size and seed (pyoracle.OracleScene(scene).render(passes=1, pass_begin=k, seed=11)
# .last_stats: invalid_samples 0 of 1024 for k = 0, 1), inside the test's 1 % bound.
RENDER_CASES = ["cbox_path_mis", "cbox_path_mats", "volumetric", "veach_direct_mis", "cbox_thinlens", "cbox_bvh"]


class env:
    """Environment variables set around a block (the library reads its knobs at every call)."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update({k: str(v) for k, v in self.kw.items()})

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def same(a, b):
    """Equality of float values, NaN equal to NaN (+0 and -0 equal)."""
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def valid(rows):
    return (np.isfinite(rows) & (rows >= 0)).all(-1)


def case_scene(name, tmp):
    xml = {"cbox_path_mis": scene_path(*CBOX), "cbox_bvh": scene_path(*CBOX),
           "cbox_path_mats": scene_path("pa4", "cbox", "cbox_path_mats.xml"),
           "volumetric": scene_path("project", "volumetric", "volumetric.xml"),
           "veach_direct_mis": scene_path(*VEACH)}.get(name)
    if name == "cbox_thinlens":
        xml = synth.cbox_variant(str(tmp), "li_thin", integrator="path_mis", camera_type="thinlens", camera_props=THINLENS)
    return nori_amd.load_scene(xml, W, H, 2)


def renderer(scene, mode=None):
    with env(**({"NORI_TRAVERSAL": mode} if mode else {})):
        return nori_amd.GpuRenderer(scene, 0)


def renderer_samples_equal_li(r, scene, k):
    """Test 1's statement for pass k: every pixel's unfiltered render sample equals li of its
    camera ray on its stream; the pixels whose sample the film dropped have an invalid li row."""
    stats = np.zeros((H, W, 8), np.float32)
    r.render(passes=1, pass_begin=k, seed=SEED, variance=stats)
    dropped = r.last_stats["invalid_samples"]
    rays = r.camera_rays(passes=1, pass_begin=k, seed=SEED).reshape(N, 8)
    L = r.li(rays, seed=SEED, stream_base=k * N, first_draw=4).reshape(H, W, 3)
    st = r.last_stats
    count = stats[..., 6]
    assert set(np.unique(count)) <= {0.0, 1.0}
    one = count == 1
    print(f"pass {k}: {int(one.sum())} of {N} samples valid, render dropped {dropped}, li counted "
          f"{st['invalid_samples']}, rays {st['rays_closest']} + {st['rays_shadow']}, k_li {st['ms_shade']:.3f} ms, "
          f"rows differing {int((~(L[one] == stats[..., 0:3][one]).all(-1)).sum())}")
    assert one.mean() >= 0.99
    assert st["samples"] == N and st["invalid_samples"] == dropped
    assert same(L[one], stats[..., 0:3][one])
    assert not valid(L[~one]).any()
    assert st["rays_closest"] >= N * 0.5 and st["ms_shade"] > 0


# ---------------------------------------------------------------- 1. the renderer's own samples
@pytest.mark.parametrize("case", RENDER_CASES)
def test_li_of_camera_rays_is_the_renderers_sample(built, tmp_path, case):
    scene = case_scene(case, tmp_path)
    with renderer(scene, "bvh" if case == "cbox_bvh" else None) as r:
        for k in range(2):
            renderer_samples_equal_li(r, scene, k)


# ---------------------------------------------------------------- 2. other rays, an independent composition
def test_li_of_given_rays_equals_the_composed_direct_mis(built):
    scene = nori_amd.load_scene(scene_path(*VEACH), W, H, 2)
    assert scene.integrator == "direct_mis"
    rays = scene_rays("veach", scene, 1000)
    n = rays.shape[0]
    assert n == 1000
    # ray i gets the stream of a (pass, pixel) id of a 2-pass frame, so that sample_uniforms has its draws
    ids = np.random.default_rng(3).permutation(2 * N)[:n].astype(np.uint64)
    nd = li_compose.draws_needed(scene, "direct_mis")
    with nori_amd.GpuRenderer(scene, 0) as r:
        U = r.sample_uniforms(4, nd, passes=2, pass_begin=0, seed=SEED).reshape(2 * N, nd)[ids.astype(np.int64)]
        want, hit = li_compose.direct_li_rays(r, scene, "direct_mis", rays, U)
        got = r.li(rays, stream_ids=ids, seed=SEED, first_draw=4)
    print(f"{int(hit.sum())} of {n} rays hit, {int((want != 0).any(1).sum())} rows non-zero, "
          f"rows differing {int((~(got == want).all(1)).sum())}")
    assert hit.mean() > 0.3 and (want != 0).any(1).mean() > 0.1
    assert same(got, want)


# ---------------------------------------------------------------- 3. independence of placement
@pytest.fixture(scope="module")
def cbox(built):
    scene = nori_amd.load_scene(scene_path(*CBOX), W, H, 2)
    with nori_amd.GpuRenderer(scene, 0) as r:
        rays = np.ascontiguousarray(r.camera_rays(passes=1, pass_begin=0, seed=SEED).reshape(N, 8)[:1000])
        ids = (np.uint64(5000) + np.uint64(3) * np.arange(1000, dtype=np.uint64))
        ref = r.li(rays, stream_ids=ids, seed=SEED, first_draw=4)
        yield scene, r, rays, ids, ref


def test_li_does_not_depend_on_placement(cbox):
    scene, r, rays, ids, ref = cbox
    assert (ref != 0).any(1).mean() > 0.5 and valid(ref).all()
    perm = np.random.default_rng(1).permutation(1000)
    assert same(r.li(rays[perm], stream_ids=ids[perm], seed=SEED, first_draw=4), ref[perm])
    with env(NORI_LI_REFILL=0):
        assert same(r.li(rays, stream_ids=ids, seed=SEED, first_draw=4), ref)
    with env(NORI_LI_RANGE=64):
        assert same(r.li(rays, stream_ids=ids, seed=SEED, first_draw=4), ref)
        for n in (1, 63, 64, 65, 127, 128, 129, 257, 1000):
            assert same(r.li(rays[:n], stream_ids=ids[:n], seed=SEED, first_draw=4), ref[:n]), n
    with env(NORI_QUERY_CHUNK=300):
        assert same(r.li(rays, stream_ids=ids, seed=SEED, first_draw=4), ref)
    # another stream, another seed or another first draw is another value
    assert not same(r.li(rays, stream_ids=ids + np.uint64(1), seed=SEED, first_draw=4), ref)
    assert not same(r.li(rays, stream_ids=ids, seed=SEED + 1, first_draw=4), ref)
    assert not same(r.li(rays, stream_ids=ids, seed=SEED, first_draw=5), ref)


def test_li_stream_base_and_device_tensors(cbox):
    torch = pytest.importorskip("torch")
    scene, r, rays, ids, ref = cbox
    base = 777
    by_base = r.li(rays, seed=SEED, stream_base=base, first_draw=4)
    by_ids = r.li(rays, stream_ids=np.uint64(base) + np.arange(1000, dtype=np.uint64), seed=SEED, first_draw=4)
    assert same(by_base, by_ids) and not same(by_base, ref)
    with env(NORI_QUERY_CHUNK=300):  # the chunks' streams continue where the last one ended
        assert same(r.li(rays, seed=SEED, stream_base=base, first_draw=4), by_base)
    d_rays = torch.from_numpy(rays).to("cuda:0")
    d_ids = torch.from_numpy(ids.view(np.int64)).to("cuda:0")
    d_out = torch.full((1000, 3), 7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    assert r.li(d_rays, stream_ids=d_ids, seed=SEED, first_draw=4, n=1000, out=d_out) is None
    assert same(d_out.cpu().numpy(), ref)
    assert r.last_stats["samples"] == 1000
    d_out.fill_(7.0)
    torch.cuda.synchronize()
    r.li(d_rays.data_ptr(), seed=SEED, stream_base=base, first_draw=4, n=1000, out=d_out.data_ptr())
    assert same(d_out.cpu().numpy(), by_base)
    assert np.array_equal(d_rays.cpu().numpy(), rays)


# ---------------------------------------------------------------- 4. the ray's own interval
def test_li_uses_the_rays_own_interval(cbox):
    scene, r, _, _, _ = cbox
    rays = scene_rays("cbox", scene, 1000)
    hits = r.query(rays, surface=False)["hits"]
    hit = hits["prim"] >= 0
    assert 0.5 < hit.mean() < 1.0  # (the box is open towards the camera: some rays leave it)
    full = r.li(rays, seed=SEED, stream_base=0, first_draw=4)
    assert not full[~hit].any() and valid(full).all()
    assert (full[hit] != 0).any(1).mean() > 0.5
    cut = rays.copy()
    cut[hit, 7] = np.nextafter(hits["t"][hit], np.float32(0))  # maxt just below the hit
    still = r.query(cut, surface=False)["hits"]["prim"] >= 0    # (an equal-t neighbour, if any)
    assert still.mean() < 0.01
    got = r.li(cut, seed=SEED, stream_base=0, first_draw=4)
    assert not got[~still].any()
    # mint beyond the hit: the first segment starts behind the surface it would have hit
    far = rays.copy()
    far[hit, 3] = np.nextafter(hits["t"][hit], np.float32(np.inf))
    behind = r.query(far, surface=False)["hits"]["prim"] >= 0
    gone = r.li(far, seed=SEED, stream_base=0, first_draw=4)
    assert not gone[~behind].any()


# ---------------------------------------------------------------- 5. chromatic cameras
def _adv_cam_xml(tmp, chromatic):
    """scenes/project/adv_cam/cbox_adv_cam.xml with its advancedCamera properties switched on (the
    file ships them commented out), with or without the chromaticAberation vector."""
    d = os.path.join(ROOT, "scenes", "project", "adv_cam")
    src = open(os.path.join(d, "cbox_adv_cam.xml")).read()
    src = src.replace("<!--<float name=\"focalDist\"", "<float name=\"focalDist\"").replace("value=\"3, 3\"/>-->", "value=\"3, 3\"/>")
    assert "<!--" not in src.split("</camera>")[0] and "chromaticAberation" in src
    if not chromatic:
        src = re.sub(r'<vector name="chromaticAberation"[^>]*/>', "", src)
        assert "chromaticAberation" not in src
    src = src.replace('value="../../', 'value="' + os.path.join(ROOT, "scenes") + "/")
    src = src.replace('value="meshes/', 'value="' + d + "/meshes/")
    path = os.path.join(str(tmp), f"adv_cam_{int(chromatic)}.xml")
    with open(path, "w") as f:
        f.write(src)
    return path


def test_li_returns_all_channels_on_a_chromatic_camera(built, tmp_path):
    chroma = nori_amd.load_scene(_adv_cam_xml(tmp_path, True), W, H, 2)
    plain = nori_amd.load_scene(_adv_cam_xml(tmp_path, False), W, H, 2)
    assert any(chroma.desc.camera.chromatic) and not any(plain.desc.camera.chromatic)
    with nori_amd.GpuRenderer(plain, 0) as r:
        rays = r.camera_rays(passes=1, pass_begin=0, seed=SEED).reshape(N, 8)
        want = r.li(rays, seed=SEED, stream_base=0, first_draw=4)
    with nori_amd.GpuRenderer(chroma, 0) as r:
        got = r.li(rays, seed=SEED, stream_base=0, first_draw=4)
    assert same(got, want)
    assert (got > 0).any(0).all()  # every channel non-zero somewhere


# ---------------------------------------------------------------- 6. degenerate input and refusals
def test_li_degenerate_rays_and_refusals(cbox):
    torch = pytest.importorskip("torch")
    scene, r, rays, ids, ref = cbox
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    bad = np.repeat(rays[:1], 8, axis=0)
    bad[0] = 0                      # an all-zero ray (an unselected block's entry of camera_rays)
    bad[1, 4:7] = nan               # NaN direction
    bad[2, 0] = inf                 # infinite origin
    bad[3, 3], bad[3, 7] = 2.0, 1.0  # maxt < mint: traced, hits nothing
    bad[4, 7] = nan                 # NaN maxt
    bad[5, 3] = -inf                # infinite mint
    bad[6, 4:7] = 0                 # zero direction
    # row 7 is ray 0 itself
    for refill in (1, 0):
        with env(NORI_LI_REFILL=refill):
            out = r.li(bad, stream_ids=np.repeat(ids[:1], 8), seed=SEED, first_draw=4)
            assert not out[:7].any() and same(out[7], ref[0])
            assert r.last_stats["invalid_samples"] == 0
            # a batch of nothing but rows that are not traced
            assert not r.li(bad[:3], seed=SEED).any()
    f = nori_amd.lib().nori_gpu_li
    out = np.full((1000, 3), 7.0, np.float32)
    pr, po, pi = C.c_void_p(rays.ctypes.data), C.c_void_p(out.ctypes.data), C.c_void_p(ids.ctypes.data)
    ok = _abi.LiDesc(1000, 0, SEED, 0, 4, 0)
    INV = _abi.NORI_ERR_INVALID
    assert f(None, C.byref(ok), pr, pi, po, None) == INV
    assert f(r._h, None, pr, pi, po, None) == INV
    assert f(r._h, C.byref(ok), None, pi, po, None) == INV
    assert f(r._h, C.byref(ok), pr, pi, None, None) == INV
    assert f(r._h, C.byref(_abi.LiDesc(1000, 0, SEED, 0, 4, 1)), pr, pi, po, None) == INV       # reserved
    assert f(r._h, C.byref(_abi.LiDesc(1000, 0, SEED, 0, 65536, 0)), pr, pi, po, None) == INV   # first_draw
    d_rays = torch.from_numpy(rays).to("cuda:0")
    d_ids = torch.from_numpy(ids.view(np.int64)).to("cuda:0")
    d_out = torch.full((1000, 3), 7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    dev = _abi.LiDesc(16, 1, SEED, 0, 4, 0)
    dr, di, do = d_rays.data_ptr(), d_ids.data_ptr(), d_out.data_ptr()
    for a, b, c in ((dr + 4, di, do), (dr, di + 4, do), (dr, di, do + 2),                        # misaligned
                    (rays.ctypes.data, di, do), (dr, ids.ctypes.data, do), (dr, di, out.ctypes.data)):  # host memory
        assert f(r._h, C.byref(dev), C.c_void_p(a), C.c_void_p(b), C.c_void_p(c), None) == INV, (a, b, c)
    assert (out == 7.0).all() and (d_out.cpu().numpy() == 7.0).all()                            # nothing written
    assert f(r._h, C.byref(_abi.LiDesc(0, 0, SEED, 0, 4, 0)), pr, pi, po, None) == _abi.NORI_OK  # n == 0: a no-op
    assert (out == 7.0).all()
    assert f(r._h, C.byref(_abi.LiDesc(1000, 0, SEED, 0, 65535, 0)), pr, pi, po, None) == _abi.NORI_OK
    assert valid(out).all()
    # the context works afterwards and gives what it gave before
    assert f(r._h, C.byref(ok), pr, pi, po, None) == _abi.NORI_OK
    assert same(out, ref)


# ---------------------------------------------------------------- 7. dynamic geometry
def test_li_after_update_vertices(built, tmp_path):
    scene = refit_util.load("hf", str(tmp_path))
    assert (scene.width, scene.height) == (W, H)
    with renderer(scene, "bvh") as r:
        r.update_vertices(refit_util.position_set(scene, "b"))
        renderer_samples_equal_li(r, scene, 1)


# ---------------------------------------------------------------- 8. the example
def test_panorama_example(built, tmp_path):
    pytest.importorskip("torch")
    spec = importlib.util.spec_from_file_location("panorama_torch", os.path.join(ROOT, "examples", "panorama_torch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    png = str(tmp_path / "pano.png")
    mod.main([scene_path(*CBOX), png, "--spp", "2", "--width", "32", "--height", "32"])
    img = nori_amd.read_image(png)
    assert img.shape == (32, 32, 3)
    assert img.min() < img.max()
