"""GPU: extension rays traced inside the shade kernel (S.ext_inline,
kernels_shade.hip k_shade: the closest hit of the thread's queued ray through
the wave-uniform scan, in place of the hit a separate extension launch wrote)
against the separate launch (NORI_EXT_INLINE=0): the same image up to the
film sums' order, the same ray counts and the same number of wavefront
iterations, for every basic-plugin integrator, with small pools (many
iterations with compaction, regeneration, segments running dry and the
drain), one and three pool parts, waves of camera rays only (the in-plane
filter scan), segments with lanes past their count, and timing renders (which
keep the two launches).  The defaults are checked too: on for the Cornell box,
off without the inline shadow rays, for the full plugin set and for BVH
scenes.  The films are compared to the inline-NEE test's tolerance and not
bit for bit: two renders in one mode differ in the last bits too (the film's
atomic sums; measured 8e-6 to 3e-5 absolute on these scenes, either way)."""
import contextlib
import os
import re

import numpy as np
import pytest

import nori_amd
from conftest import scene_path
import synth

pytestmark = pytest.mark.gpu

COUNTERS = ("samples", "invalid_samples", "rays_closest", "rays_shadow", "rays_finish", "iterations")


@contextlib.contextmanager
def _env(**env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _render(s, env, **kw):
    """One render of a fresh context under `env`: (film, stats)."""
    with _env(**env):
        with nori_amd.GpuRenderer(s, 0) as r:
            img = r.render(**kw)
            return img, r.last_stats


def _scene(kind, tmp_path, width=0, height=0, spp=8):
    if kind == "cbox_path_mis":
        return nori_amd.load_scene(scene_path("pa4", "cbox", "cbox_path_mis.xml"), width or 96, height or 72, spp)
    if kind == "volumetric_basic":  # the Disney sphere made diffuse: the basic plugin set
        src = open(scene_path("project", "volumetric", "volumetric.xml")).read()
        src = src.replace('value="meshes/', f'value="{scene_path("project", "volumetric", "meshes")}/')
        src = re.sub(r'<bsdf type="disney">.*?</bsdf>',
                     '<bsdf type="diffuse"><color name="albedo" value="0.5 0.5 0.5"/></bsdf>', src, flags=re.S)
        xml = str(tmp_path / f"{kind}.xml")
        open(xml, "w").write(src)
        return nori_amd.load_scene(xml, 80, 60, spp)
    assert kind == "path_mats"
    xml = synth.cbox_variant(str(tmp_path), kind, integrator="path_mats", width=80, height=64)
    return nori_amd.load_scene(xml, 0, 0, spp)


def _same(a, sa, b, sb, counters=COUNTERS):
    assert np.allclose(a, b, rtol=1e-5, atol=1e-6), np.abs(a - b).max()
    for k in counters:
        assert sa[k] == sb[k], (k, sa[k], sb[k])
    assert a.mean() > 0.0


@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("pool", [4096, 65536])
@pytest.mark.parametrize("kind", ["cbox_path_mis", "path_mats", "volumetric_basic"])
def test_ext_inline_same_image(built, tmp_path, kind, pool, parts):
    s = _scene(kind, tmp_path)
    a, sa = _render(s, dict(NORI_EXT_INLINE="1", NORI_POOL_PARTS=str(parts)), path_pool=pool)
    b, sb = _render(s, dict(NORI_EXT_INLINE="0", NORI_POOL_PARTS=str(parts)), path_pool=pool)
    assert sa["ext_inline"] == 1 and sb["ext_inline"] == 0
    assert sa["nee_inline"] == 1 and sb["nee_inline"] == 1
    _same(a, sa, b, sb)
    assert sa["rays_closest"] > sa["samples"]


def test_ext_inline_camera_waves(built, tmp_path):
    # 1 spp, the pool larger than the work: every wave of the second launch
    # holds camera rays only, so it takes the in-plane filter scan
    s = _scene("cbox_path_mis", tmp_path, spp=1)
    a, sa = _render(s, dict(NORI_EXT_INLINE="1", NORI_CAMERA_CULL="1"), path_pool=65536)
    b, sb = _render(s, dict(NORI_EXT_INLINE="1", NORI_CAMERA_CULL="0"), path_pool=65536)
    c, sc = _render(s, dict(NORI_EXT_INLINE="0", NORI_CAMERA_CULL="1"), path_pool=65536)
    assert sa["ext_inline"] == 1 and sb["ext_inline"] == 1 and sc["ext_inline"] == 0
    _same(a, sa, b, sb)
    _same(a, sa, c, sc)


def test_ext_inline_partial_segments(built, tmp_path):
    # 50 x 37 = 1850 pixels, no multiple of the 256-entry segment: lanes past
    # a segment's count from the first iteration on
    s = _scene("cbox_path_mis", tmp_path, width=50, height=37)
    a, sa = _render(s, dict(NORI_EXT_INLINE="1"), path_pool=4096)
    b, sb = _render(s, dict(NORI_EXT_INLINE="0"), path_pool=4096)
    assert sa["ext_inline"] == 1 and sb["ext_inline"] == 0
    _same(a, sa, b, sb)


def test_ext_inline_timing_render(built, tmp_path):
    s = _scene("cbox_path_mis", tmp_path)
    a, sa = _render(s, dict(NORI_EXT_INLINE="1"), timing=True)
    b, sb = _render(s, dict(NORI_EXT_INLINE="1"))
    assert sa["ext_inline"] == 1 and sb["ext_inline"] == 1
    _same(a, sa, b, sb, counters=("samples", "invalid_samples"))
    assert sa["ms_extend"] > 0.0 and sa["ms_shade"] > 0.0


def test_ext_inline_defaults(built):
    cbox = nori_amd.load_scene(scene_path("pa4", "cbox", "cbox_path_mis.xml"), 64, 48, 2)
    vol = nori_amd.load_scene(scene_path("project", "volumetric", "volumetric.xml"), 64, 48, 2)
    for s, env, on in ((cbox, {}, 1), (cbox, dict(NORI_NEE_INLINE="0"), 0), (vol, dict(NORI_EXT_INLINE="1"), 0),
                       (cbox, dict(NORI_TRAVERSAL="bvh", NORI_EXT_INLINE="1"), 0)):
        _, st = _render(s, env)
        assert st["ext_inline"] == on, (env, st["ext_inline"])
