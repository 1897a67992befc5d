"""First-hit features (nori_gpu_render_features, k_features) and the feature-guided denoiser
(nori_denoise_guided, k_guided) on the GPU.

The features are checked against independent statements: the shading normal against the
`normals` integrator's own film statistics bit for bit (same sample streams, so the same
primary rays), the albedo against the scene description, the depth against analytic geometry.
The guided kernel is checked against the double-precision host statement
(nori_film_denoise_guided, itself checked against numpy in test_features.py), never against itself.
"""
import os
import shutil
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

import nori_amd
import synth
from conftest import ROOT, scene_path
from nori_amd import _abi
from test_features import INF, PARAMS, RF, SHAPES, box_mean, random_inputs, two_halves

pytestmark = pytest.mark.gpu

CBOX = ("pa4", "cbox", "cbox_path_mis.xml")
NMAP = ("project", "textured", "cbox_normalmap_normals.xml")
THINLENS = '<float name="lensRadius" value="0.08"/><float name="focalDist" value="4.8"/>'
CHROMA = ('<float name="lensRadius" value="0.05"/><float name="focalDist" value="5"/>'
          '<vector name="chromaticAberation" value="4, 2, 3.3"/>')


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


def _normals_stats(scene, mode=None, **kw):
    """The film statistics of one pass of a `normals` scene: sum L = |n| of the pass's one sample."""
    st = np.zeros((scene.height, scene.width, 8), np.float32)
    with _renderer(scene, mode) as r:
        r.render(passes=1, variance=st, **kw)
    return st


def _assert_normals_equal(feat, st):
    assert not np.isnan(feat).any() and not np.isnan(st).any()
    assert np.array_equal(np.abs(feat[..., 3:6]), st[..., 0:3])
    assert np.array_equal(feat[..., 7], st[..., 6])
    assert (feat[..., 7] == 1).all()
    assert (np.abs(feat[..., 3:6]).sum(-1) > 0).mean() > 0.5  # the frame is not mostly misses


# ---------------------------------------------------------------- normals, bit for bit
@pytest.mark.parametrize("mode", [None, "scan", "bvh"])
@pytest.mark.parametrize("pass_begin,seed", [(0, 0), (5, 11)])
def test_normals_match_the_normals_integrator(built, tmp_path, mode, pass_begin, seed):
    """features() on a path_mis context against the film statistics of the `normals` integrator."""
    sn = nori_amd.load_scene(synth.cbox_variant(str(tmp_path), "n", integrator="normals", width=96, height=72), 0, 0, 1)
    sp = nori_amd.load_scene(synth.cbox_variant(str(tmp_path), "p", integrator="path_mis", width=96, height=72), 0, 0, 1)
    st = _normals_stats(sn, mode, pass_begin=pass_begin, seed=seed)
    with _renderer(sp, mode) as r:
        feat = r.features(passes=1, pass_begin=pass_begin, seed=seed)
        stats = r.last_stats
    _assert_normals_equal(feat, st)
    assert stats["samples"] == 96 * 72 and stats["rays_closest"] == 96 * 72 and stats["ms_total"] > 0


def test_normals_thinlens(built, tmp_path):
    kw = dict(camera_type="thinlens", camera_props=THINLENS, width=96, height=72)
    sn = nori_amd.load_scene(synth.cbox_variant(str(tmp_path), "n", integrator="normals", **kw), 0, 0, 1)
    sp = nori_amd.load_scene(synth.cbox_variant(str(tmp_path), "p", integrator="path_mis", **kw), 0, 0, 1)
    st = _normals_stats(sn, pass_begin=2)
    with nori_amd.GpuRenderer(sp, 0) as r:
        _assert_normals_equal(r.features(passes=1, pass_begin=2), st)
    # (the lens matters: the pinhole camera's normals differ)
    s0 = nori_amd.load_scene(synth.cbox_variant(str(tmp_path), "q", integrator="path_mis", width=96, height=72), 0, 0, 1)
    with nori_amd.GpuRenderer(s0, 0) as r:
        assert not np.array_equal(np.abs(r.features(passes=1, pass_begin=2)[..., 3:6]), st[..., 0:3])


def test_normals_chromatic_aberration_follow_the_green_ray(built, tmp_path):
    """With chromatic aberration the render traces one ray per colour channel and weights each by its
    channel's unit colour: the green statistic of the `normals` film is |n_y| of the green ray's hit."""
    xml = synth.cbox_variant(str(tmp_path), "c", integrator="normals", camera_type="advancedCamera",
                             camera_props=CHROMA, width=96, height=72)
    s = nori_amd.load_scene(xml, 0, 0, 1)
    st = np.zeros((72, 96, 8), np.float32)
    with nori_amd.GpuRenderer(s, 0) as r:
        r.render(passes=1, variance=st, pass_begin=1)
        feat = r.features(passes=1, pass_begin=1)
    assert np.array_equal(np.abs(feat[..., 4]), st[..., 1])
    assert not np.array_equal(np.abs(feat[..., 3]), st[..., 0])  # the red ray is another ray


@pytest.mark.parametrize("mode", ["scan", "bvh"])
def test_normals_normal_maps_spheres_mirror(built, mode):
    """Normal-mapped meshes, spheres and the mirror; render and features on the same context."""
    s = nori_amd.load_scene(scene_path(*NMAP), 80, 60, 1)
    st = np.zeros((60, 80, 8), np.float32)
    with _renderer(s, mode) as r:
        r.render(passes=1, variance=st, pass_begin=3)
        feat = r.features(passes=1, pass_begin=3)
    _assert_normals_equal(feat, st)


# ---------------------------------------------------------------- pass splitting, determinism, plumbing
@pytest.fixture(scope="module")
def cbox(built):
    s = nori_amd.load_scene(scene_path(*CBOX), 96, 72, 8)
    with nori_amd.GpuRenderer(s, 0) as r:
        yield s, r


def test_pass_splitting_and_determinism(cbox):
    s, r = cbox
    whole = r.features(passes=4, pass_begin=2, seed=3)
    again = r.features(passes=4, pass_begin=2, seed=3)
    assert np.array_equal(whole, again)
    parts = np.zeros((72, 96, 8), np.float32)
    for k in range(4):
        r.features(passes=1, pass_begin=2 + k, seed=3, out=parts)
    assert np.array_equal(whole, parts)
    assert (whole[..., 7] == 4).all()
    # ADDED into the caller's buffer, continuing from its values
    more = r.features(passes=2, pass_begin=6, seed=3, out=whole.copy())
    assert np.array_equal(more, r.features(passes=6, pass_begin=2, seed=3))
    # pass_count 0 means the scene's sampleCount
    assert (r.features(passes=0)[..., 7] == s.spp).all() and (r.features()[..., 7] == s.spp).all()
    assert r.last_stats["samples"] == 96 * 72 * s.spp


def test_block_subset(cbox):
    s, r = cbox
    full = r.features(passes=3)
    sel = [1, 3, 8]  # 3 x 3 blocks, the last row and column partial
    out = np.full((72, 96, 8), 0.5, np.float32)
    r.features(passes=3, blocks=sel, out=out)
    ys, xs = np.mgrid[0:72, 0:96]
    inside = np.isin((ys // 32) * 3 + xs // 32, sel)
    assert (out[~inside] == 0.5).all()
    base = np.full((72, 96, 8), 0.5, np.float32)
    assert np.array_equal(out[inside], r.features(passes=3, out=base)[inside])
    assert np.array_equal((out - 0.5)[inside][:, 7], full[inside][:, 7])
    alone = r.features(passes=3, blocks=sel)
    assert np.array_equal(alone[inside], full[inside]) and alone[inside].any() and not alone[~inside].any()


def test_device_buffer_equals_host_path(cbox):
    torch = pytest.importorskip("torch")
    s, r = cbox
    host = r.features(passes=3, pass_begin=1)
    dev = torch.zeros((72, 96, 8), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    assert r.features(passes=2, pass_begin=1, out=dev.data_ptr()) is None
    r.features(passes=1, pass_begin=3, out=dev.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy(), host)


def test_features_arguments(cbox):
    s, r = cbox
    rd, st = _abi.RenderDesc(), _abi.Stats()
    rd.pass_count = 1
    buf = np.zeros((72, 96, 8), np.float32)
    f = nori_amd.lib().nori_gpu_render_features
    import ctypes as C

    assert f(r._h, C.byref(rd), None, C.byref(st)) == _abi.NORI_ERR_INVALID
    assert f(None, C.byref(rd), buf.ctypes.data_as(C.c_void_p), C.byref(st)) == _abi.NORI_ERR_INVALID
    rd.variance_out = buf.ctypes.data  # must be NULL
    assert f(r._h, C.byref(rd), buf.ctypes.data_as(C.c_void_p), C.byref(st)) == _abi.NORI_ERR_INVALID
    assert b"variance_out" in nori_amd.lib().nori_gpu_last_error()
    assert not buf.any()
    with pytest.raises(nori_amd.NoriError):
        r.features(passes=1, blocks=[99])
    rd.variance_out = None
    rd.timing = 1
    assert f(r._h, C.byref(rd), buf.ctypes.data_as(C.c_void_p), None) == _abi.NORI_OK  # stats may be NULL
    assert f(r._h, C.byref(rd), buf.ctypes.data_as(C.c_void_p), C.byref(st)) == _abi.NORI_OK
    assert st.ms_shade > 0 and st.ms_total >= st.ms_shade and (buf[..., 7] == 2).all()


# ---------------------------------------------------------------- albedo
def _albedo(b):
    return np.float32(list(b.albedo))


def _triangle_normals(s, shape):
    """Unit geometric normals of a mesh's triangles from the scene description (float64)."""
    tri = s.positions()[s.indices()[shape.tri_offset:shape.tri_offset + shape.tri_count]].astype(np.float64)
    g = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    return g / np.linalg.norm(g, axis=-1, keepdims=True)


def test_albedo_cbox(cbox):
    """Each pixel's albedo follows from its own normal feature.  The meshes of this scene have no
    vertex normals, so a mesh pixel's shading normal is one of its mesh's triangle normals (the
    left wall is slightly tilted: its two are unique to it); the right wall's (-1, 0, 0) is its own;
    the floor, ceiling and back wall share theirs with the light (default diffuse BSDF, albedo 0.5);
    a normal that is no triangle's belongs to a sphere: mirror and dielectric are (1, 1, 1)."""
    s, r = cbox
    feat = r.features(passes=1)
    assert (feat[..., 7] == 1).all()
    a, n = feat[..., 0:3], feat[..., 3:6].astype(np.float64)
    shapes, bsdfs = s.shapes(), s.bsdfs()
    # scene order (cbox_path_mis.xml): walls, right wall, left wall, mirror sphere, glass sphere, light
    WALLS, RIGHT, LEFT, MIRROR, GLASS, LIGHT = range(6)
    assert [sh.type for sh in shapes] == [0, 0, 0, 1, 1, 0] and not any(sh.has_normals for sh in shapes)
    alb = [_albedo(bsdfs[sh.bsdf]) for sh in shapes]
    assert bsdfs[shapes[MIRROR].bsdf].type == _abi.BSDF_MIRROR and bsdfs[shapes[GLASS].bsdf].type == _abi.BSDF_DIELECTRIC
    assert np.allclose(alb[LEFT], [0.630, 0.065, 0.05]) and np.allclose(alb[RIGHT], [0.161, 0.133, 0.427])
    assert np.allclose(alb[WALLS], [0.725, 0.71, 0.68]) and np.allclose(alb[LIGHT], [0.5, 0.5, 0.5])
    # which meshes own a triangle normal equal (to fp32 rounding) to the pixel's normal
    owner = np.zeros((6,) + n.shape[:2], bool)
    for i in (WALLS, RIGHT, LEFT, LIGHT):
        for g in _triangle_normals(s, shapes[i]):
            owner[i] |= np.abs(n - g).max(-1) < 1e-5
    hit = np.abs(n).sum(-1) > 0
    is_left = owner[LEFT] & ~owner[WALLS] & ~owner[RIGHT] & ~owner[LIGHT]
    is_right = owner[RIGHT] & ~owner[WALLS] & ~owner[LEFT] & ~owner[LIGHT]
    other = (owner[WALLS] | owner[LIGHT]) & ~owner[LEFT] & ~owner[RIGHT]
    sphere = hit & ~owner.any(0)
    assert (is_left | is_right | other | sphere | ~hit).all()
    print("left", int(is_left.sum()), "right", int(is_right.sum()), "spheres", int(sphere.sum()), "other",
          int(other.sum()), "miss", int((~hit).sum()))
    assert is_left.sum() > 300 and is_right.sum() > 300 and sphere.sum() > 200 and other.sum() > 1000
    assert (a[is_left] == alb[LEFT]).all()
    assert (a[is_right] == alb[RIGHT]).all()
    assert (a[sphere] == 1).all()
    white, lamp = (a[other] == alb[WALLS]).all(-1), (a[other] == alb[LIGHT]).all(-1)
    assert (white | lamp).all() and white.sum() > 1000 and lamp.sum() > 5
    assert not a[~hit].any()
    # the light: emission plays no part; its pixels carry its BSDF's albedo and its downward normal
    assert (n[other][lamp][:, 1] < -1 + 1e-6).all()


CHECKER = """
<mesh type="sphere">
  <point name="center" value="0.0 0.9 0.3"/>
  <float name="radius" value="0.28"/>
  <bsdf type="diffuse">
    <texture type="checkerboard_color" name="albedo">
      <point name="delta" value="0.5,0.5"/>
      <vector name="scale" value="0.05,0.1"/>
      <color name="value1" value="0.8,0.7,0.6"/>
      <color name="value2" value="0.2,0.25,0.3"/>
    </texture>
  </bsdf>
</mesh>
<mesh type="sphere">
  <point name="center" value="0.0 0.3 0.9"/>
  <float name="radius" value="0.2"/>
  <bsdf type="microfacet"><color name="kd" value="0.1, 0.2, 0.15"/></bsdf>
</mesh>
<mesh type="sphere">
  <point name="center" value="0.0 1.5 0.0"/>
  <float name="radius" value="0.15"/>
  <bsdf type="disney"><color name="baseColor" value="0.3, 0.6, 0.9"/></bsdf>
</mesh>"""


def _on_sphere(s, feat, centre, radius, origin):
    """Pixels whose one sample hit the sphere: the point x = centre + radius n lies at the depth
    feature from the camera and projects into the pixel itself."""
    n, t = feat[..., 3:6].astype(np.float64), feat[..., 6].astype(np.float64)
    x = np.float64(centre) + radius * n
    at_depth = np.abs(np.linalg.norm(x - np.float64(origin), axis=-1) - t) <= 1e-4 * t
    cam = s.desc.camera
    w2c = np.linalg.inv(np.float64(list(cam.camera_to_world)).reshape(4, 4))
    c2s = np.linalg.inv(np.float64(list(cam.sample_to_camera)).reshape(4, 4))
    h = np.concatenate([x, np.ones(x.shape[:2] + (1,))], -1) @ w2c.T
    h = np.concatenate([h[..., :3] / h[..., 3:4], np.ones(x.shape[:2] + (1,))], -1) @ c2s.T
    with np.errstate(invalid="ignore", divide="ignore"):
        px, py = h[..., 0] / h[..., 3] * cam.width, h[..., 1] / h[..., 3] * cam.height
    ys, xs = np.mgrid[0:cam.height, 0:cam.width]
    in_pixel = (np.abs(px - (xs + 0.5)) <= 0.5 + 1e-3) & (np.abs(py - (ys + 0.5)) <= 0.5 + 1e-3)
    return (np.abs(np.linalg.norm(n, axis=-1) - 1) < 1e-5) & at_depth & in_pixel


def test_albedo_checkerboard_microfacet_disney(built, tmp_path):
    xml = synth.cbox_variant(str(tmp_path), "tex", extra=CHECKER, width=96, height=72)
    s = nori_amd.load_scene(xml, 0, 0, 1)
    origin = (0, 0.919769, 5.41159)
    with nori_amd.GpuRenderer(s, 0) as r:
        feat = r.features(passes=1)
    a = feat[..., 0:3]
    by_shape = {b.type: b for b in s.bsdfs()}
    chk = _on_sphere(s, feat, (0.0, 0.9, 0.3), 0.28, origin)
    v1, v2 = np.float32([0.8, 0.7, 0.6]), np.float32([0.2, 0.25, 0.3])
    is1, is2 = (a[chk] == v1).all(-1), (a[chk] == v2).all(-1)
    print("checkerboard sphere pixels", int(chk.sum()), "value1", int(is1.sum()), "value2", int(is2.sum()))
    assert chk.sum() > 100 and (is1 | is2).all() and is1.sum() > 10 and is2.sum() > 10
    mf = _on_sphere(s, feat, (0.0, 0.3, 0.9), 0.2, origin)
    assert mf.sum() > 50 and (a[mf] == np.float32(list(by_shape[_abi.BSDF_MICROFACET].kd))).all()
    assert np.allclose(a[mf][0], [0.1, 0.2, 0.15])
    dis = _on_sphere(s, feat, (0.0, 1.5, 0.0), 0.15, origin)
    assert dis.sum() > 20 and (a[dis] == np.float32(list(by_shape[_abi.BSDF_DISNEY].base_color))).all()
    assert np.allclose(a[dis][0], [0.3, 0.6, 0.9])


def test_albedo_image_texture(built):
    """cbox_normalmap_normals.xml: the right wall and one sphere carry an ImageTexture albedo; every
    other BSDF has a constant one.  The textured pixels' albedos are texels of the image."""
    s = nori_amd.load_scene(scene_path(*NMAP), 80, 60, 1)
    with nori_amd.GpuRenderer(s, 0) as r:
        feat = r.features(passes=1)
    a = feat[..., 0:3]
    const = [np.float32(list(b.albedo)) for b in s.bsdfs() if b.type == _abi.BSDF_DIFFUSE
             and b.albedo_texture == _abi.TEXTURE_CONSTANT] + [np.float32([1, 1, 1])]
    hit = np.abs(feat[..., 3:6]).sum(-1) > 0
    textured = hit & ~np.any([(a == c).all(-1) for c in const], axis=0)
    tex = nori_amd.read_image(os.path.join(os.path.dirname(scene_path(*NMAP)), "textures", "texture.jpg"))
    texf = tex.astype(np.float32) / np.float32(255)
    print("textured pixels", int(textured.sum()), "texture range", texf.min((0, 1)), texf.max((0, 1)))
    assert textured.sum() > 0.1 * 80 * 60
    vals = a[textured]
    assert (vals >= texf.min((0, 1))).all() and (vals <= texf.max((0, 1))).all()
    assert len(np.unique(vals, axis=0)) > 20  # not constant
    # ... and each is a texel of the image (byte / 255 per channel)
    b = np.rint(vals.astype(np.float64) * 255).astype(np.int64)
    assert np.array_equal((b / 255.0).astype(np.float32), vals) or np.array_equal(b.astype(np.float32) / np.float32(255), vals)
    texels = set((tex[..., 0].astype(np.int64) << 16 | tex[..., 1].astype(np.int64) << 8 | tex[..., 2]).ravel().tolist())
    assert all(int(k) in texels for k in (b[:, 0] << 16 | b[:, 1] << 8 | b[:, 2]))


# ---------------------------------------------------------------- depth
def test_depth_analytic(built):
    """scenes/pa1/sphere-analytic.xml: a sphere (centre (0,0,1), radius 1.5) over the plane z = -1,
    seen from (5,5,1)."""
    s = nori_amd.load_scene(scene_path("pa1", "sphere-analytic.xml"), 64, 64, 1)
    with nori_amd.GpuRenderer(s, 0) as r:
        feat = r.features(passes=1)
    n, t = feat[..., 3:6].astype(np.float64), feat[..., 6].astype(np.float64)
    o = np.float64([5, 5, 1])
    hit = np.abs(n).sum(-1) > 0
    plane = hit & (np.abs(n[..., 0]) < 1e-6) & (np.abs(n[..., 1]) < 1e-6)
    sphere = hit & ~plane
    miss = ~hit
    print("sphere", int(sphere.sum()), "plane", int(plane.sum()), "miss", int(miss.sum()))
    assert sphere.sum() > 300 and plane.sum() > 300 and miss.sum() > 300
    want = np.linalg.norm(np.float64([0, 0, 1]) + 1.5 * n - o, axis=-1)
    rel = np.abs(t - want)[sphere] / want[sphere]
    print("sphere depth: max relative error", rel.max())
    assert rel.max() <= 1e-4
    assert (n[plane][:, 2] > 1 - 1e-6).all()
    # the plane's depth between the extremes of (o_z + 1) / (-d_z) over the pixel's corner directions
    cam = s.desc.camera
    s2c = np.float64(list(cam.sample_to_camera)).reshape(4, 4)
    c2w = np.float64(list(cam.camera_to_world)).reshape(4, 4)
    ys, xs = np.mgrid[0:65, 0:65]
    ndc = np.stack([xs / 64.0, ys / 64.0, np.zeros_like(xs, float), np.ones_like(xs, float)], -1) @ s2c.T
    near = ndc[..., :3] / ndc[..., 3:4]
    d = (near / np.linalg.norm(near, axis=-1, keepdims=True)) @ c2w[:3, :3].T
    tc = np.where(d[..., 2] < 0, (o[2] + 1) / -np.where(d[..., 2] < 0, d[..., 2], -1), np.inf)
    corners = np.stack([tc[:-1, :-1], tc[:-1, 1:], tc[1:, :-1], tc[1:, 1:]], 0)
    lo, hi = corners.min(0) * (1 - 1e-4), corners.max(0) * (1 + 1e-4)
    print("plane depth: worst margin", float(np.min(np.minimum(t - lo, hi - t)[plane] / t[plane])))
    assert (t[plane] >= lo[plane]).all() and (t[plane] <= hi[plane]).all()
    assert not feat[miss][:, 0:7].any() and (feat[..., 7] == 1).all()
    assert (feat[hit][:, 0:3] == 1).all()  # both albedos are (1, 1, 1)


# ---------------------------------------------------------------- the guided kernel
@pytest.mark.parametrize("r,f", RF)
@pytest.mark.parametrize("h,w", SHAPES + [(61, 70)])
def test_guided_kernel_matches_host_statement(built, h, w, r, f):
    """k_guided (fp32, expf) against the float64 host statement, at the NL-means kernel's tolerance
    (test_gpu_denoise.py): |gpu - ref| <= 2e-4 max(|ref|, 1e-2) -- the same arithmetic class, fp32
    rounding through box means over at most 289 offsets.  Measured: at most 2.2e-6 (r = 8, f = 3, 61x70)."""
    rgb, var, feat = random_inputs(h, w, seed=7000 + 100 * h + w + r)
    ref = nori_amd.film_denoise_guided(rgb, var, feat, radius=r, patch=f, **PARAMS)
    gpu = nori_amd.denoise_guided(rgb, var, feat, radius=r, patch=f, **PARAMS)
    err = float((np.abs(gpu - ref) / np.maximum(np.abs(ref), 1e-2)).max())
    print(f"{h}x{w} r={r} f={f}: max relative error {err:.2e}")
    assert np.isfinite(gpu).all() and err <= 2e-4


def test_guided_kernel_defaults_and_switched_off_terms(built):
    rgb, var, feat = random_inputs(37, 45, seed=11)
    # (a sigma whose fp32 square underflows must not turn 0 x 1/sigma^2 into NaN)
    for kw in (dict(), dict(sigma_albedo=INF, sigma_depth=INF, k=1.5), dict(sigma_normal=INF, k=1.5, patch=2, radius=6),
               dict(sigma_albedo=1e-25, sigma_normal=1e-30, k=1.5)):
        ref = nori_amd.film_denoise_guided(rgb, var, feat, **kw)
        gpu = nori_amd.denoise_guided(rgb, var, feat, **kw)
        err = float((np.abs(gpu - ref) / np.maximum(np.abs(ref), 1e-2)).max())
        print(kw, f"max relative error {err:.2e}")
        assert np.isfinite(gpu).all() and err <= 2e-4


def test_guided_kernel_edge_stop(built):
    rgb, var, feat, side = two_halves()
    kw = dict(radius=3, patch=1, k=0.45, eps=1e-10, sigma_normal=INF, sigma_depth=INF)
    own = box_mean(rgb, 3, member=side)
    got = nori_amd.denoise_guided(rgb, var, feat, sigma_albedo=0.1, **kw)
    assert np.max(np.abs(got - own)) <= 1e-5
    mixed = nori_amd.denoise_guided(rgb, var, feat, sigma_albedo=INF, **kw)
    assert np.max(np.abs(mixed - box_mean(rgb, 3))) <= 1e-5
    assert np.max(np.abs(mixed - own)) > 1e-2


# ---------------------------------------------------------------- end to end
def test_guided_denoise_lowers_the_error_of_a_16spp_render(built):
    """cbox path_mis 160x120 at 16 spp, denoised with the default parameters, against 512 spp.
    The MSEs of the noisy image, the textbook NL-means (denoise(mode=1)) and the guided filter are
    printed; only guided < noisy is asserted.  Measured on an MI355X (DESIGN_LOG.md, 2026-10-19):
    noisy 3.540e-3, textbook NL-means 5.781e-4, guided 3.083e-3 -- with its (untuned) defaults the
    guided filter lowers the MSE far less than the textbook NL-means does on this scene."""
    s = nori_amd.load_scene(scene_path(*CBOX), 160, 120, 16)
    stats = np.zeros((s.height, s.width, 8), np.float32)
    with nori_amd.GpuRenderer(s, 0) as r:
        noisy = nori_amd.develop(s, r.render(variance=stats))
        feat7 = nori_amd.film_features(s, r.features(passes=16))
    var = nori_amd.film_variance(s, stats).sum(axis=2)
    ref_s = nori_amd.load_scene(scene_path(*CBOX), 160, 120, 512)
    with nori_amd.GpuRenderer(ref_s, 0) as r:
        clean = nori_amd.develop(ref_s, r.render())

    def mse(a):
        return float(np.mean((np.clip(a, 0, 1) - np.clip(clean, 0, 1)) ** 2))

    guided = nori_amd.denoise_guided(noisy, var, feat7)
    textbook = nori_amd.denoise(noisy, var, mode=1, script_scale=False)
    print(f"cbox 160x120 16 spp, MSE vs 512 spp: noisy {mse(noisy):.3e}, textbook NL-means {mse(textbook):.3e}, "
          f"guided {mse(guided):.3e}")
    assert np.isfinite(guided).all()
    assert mse(guided) < mse(noisy)


def test_cli_features_and_denoise(built, tmp_path):
    dst = tmp_path / "cbox"
    shutil.copytree(os.path.dirname(scene_path(*CBOX)), dst)
    xml = str(dst / "cbox_path_mis.xml")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "nori-ray-tracer_amd"))
    cmd = [sys.executable, "-m", "nori_amd", xml, "--width", "64", "--height", "48", "--spp", "8"]
    extra = ["cbox_path_mis_albedo.exr", "cbox_path_mis_normal.exr", "cbox_path_mis_depth.exr",
             "cbox_path_mis_denoised.exr"]
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr
    assert (dst / "cbox_path_mis.exr").exists() and not any((dst / e).exists() for e in extra)
    assert not list(dst.glob("*denoised*")) and not list(dst.glob("*albedo*"))
    p = subprocess.run(cmd + ["--denoise", "--features", "4"], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr
    for e in extra:
        assert (dst / e).exists(), e
    # the features have no atomics: a second context reproduces the files bit for bit
    s = nori_amd.load_scene(xml, 64, 48, 8)
    with nori_amd.GpuRenderer(s, 0) as r:
        feat7 = nori_amd.film_features(s, r.features(passes=4))
    assert np.array_equal(nori_amd.read_exr(str(dst / "cbox_path_mis_albedo.exr")), feat7[..., 0:3])
    assert np.array_equal(nori_amd.read_exr(str(dst / "cbox_path_mis_normal.exr")), feat7[..., 3:6])
    depth = nori_amd.read_exr(str(dst / "cbox_path_mis_depth.exr"))
    assert all(np.array_equal(depth[..., c], feat7[..., 6]) for c in range(3))
    # the denoised file is the Python call with the defaults on exactly the image and the variance the
    # run wrote (the EXR files hold fp32 losslessly, k_guided has no atomics): bit for bit
    img = nori_amd.read_exr(str(dst / "cbox_path_mis.exr"))
    var = nori_amd.read_exr(str(dst / "cbox_path_mis_variance.exr")).sum(axis=2)
    want = nori_amd.denoise_guided(img, var, feat7)
    got = nori_amd.read_exr(str(dst / "cbox_path_mis_denoised.exr"))
    assert np.array_equal(got, want)
    assert np.isfinite(got).all() and not np.array_equal(got, img)


def test_features_cancel(built):
    """nori_gpu_cancel during a long features call: NORI_ERR_CANCELLED, the host buffer unchanged,
    the context usable afterwards."""
    s = nori_amd.load_scene(scene_path(*CBOX), 512, 512, 1)
    with nori_amd.GpuRenderer(s, 0) as r:
        r.features(passes=1)  # context warm
        out = np.full((512, 512, 8), 1.0, np.float32)
        err = []

        def run():
            try:
                r.features(passes=4000000, out=out)  # 62,500 chunks: seconds if it were not cancelled
            except nori_amd.NoriError as e:
                err.append(e)

        th = threading.Thread(target=run)
        t0 = time.time()
        th.start()
        seen = []
        while th.is_alive() and time.time() - t0 < 30:  # cancel once the call is under way
            p = r.progress()
            if p < 1.0:
                seen.append(p)
            if 0.0 < p < 1.0:
                break
            time.sleep(0.001)
        r.cancel()
        th.join(timeout=60)
        assert not th.is_alive()
        print("progress polled", len(seen), "times, last", seen[-1:], "outcome", err)
        assert all(b >= a for a, b in zip(seen, seen[1:])), seen
        assert err and err[0].code == _abi.NORI_ERR_CANCELLED, err
        assert (out == 1.0).all()
        assert r.progress() == 1.0
        assert (r.features(passes=2)[..., 7] == 2).all() and r.last_stats["samples"] == 2 * 512 * 512
