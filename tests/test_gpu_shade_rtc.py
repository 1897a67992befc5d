"""GPU: the scene's own compilation of k_shade (rtc.hip's shade program:
shade_kernel.h through hipRTC with the scan list as literals) against the
ahead-of-time kernel (NORI_RTC_SHADE=0), at the shapes of
test_gpu_ext_inline.py, where this kernel can go wrong: every basic-plugin
integrator, small pools (many iterations with compaction, regeneration,
segments running dry and the drain), one and two pool parts, the extension
scan inside the kernel and as a launch of its own, queue-mode shadow rays,
waves of camera rays only (the literal in-plane filter), segments with lanes
past their count, a timing render, and against NORI_RTC=0 (no specialised
kernel at all).  Both compilations run the same operations on the same
values, so they must find the same hits: the ray, sample and iteration
counts are equal exactly, the films to the bar that file uses for two renders
of one scene (the film's atomic sums differ run to run in the last bits)."""
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
    """One render of a fresh context under `env`: (film, stats, the context's shade_rtc info).
    NORI_LOOKAHEAD=0: the host waits for every iteration before it checks whether the work has
    all been handed out.  At its default it queues six iterations ahead and stops when it sees
    the device's flag, so a render launches up to six iterations more or fewer depending on
    how far the host runs ahead, and its rays divide differently between the loop and the
    finisher: with these tiny frames the host does fall behind now and then (measured once in
    the whole suite: 45 against 51 iterations, 173365 against 174535 extension rays, the same
    film).  The kernels, their launches and the segments' life are the same either way."""
    with _env(**dict(env, NORI_LOOKAHEAD="0")):
        with nori_amd.GpuRenderer(s, 0) as r:
            img = r.render(**kw)
            return img, r.last_stats, r.shade_rtc


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
    print("max |a - b| =", np.abs(a - b).max(), {k: (sa[k], sb[k]) for k in counters})
    assert np.allclose(a, b, rtol=1e-5, atol=1e-6), np.abs(a - b).max()
    for k in counters:
        assert sa[k] == sb[k], (k, sa[k], sb[k])
    assert a.mean() > 0.0


def _pair(s, env, **kw):
    """The render with the specialised kernel and the one with the ahead-of-time kernel."""
    a, sa, ia = _render(s, dict(env, NORI_RTC_SHADE="1"), **kw)
    b, sb, ib = _render(s, dict(env, NORI_RTC_SHADE="0"), **kw)
    assert ia["active"] and ia["code_bytes"] > 10000 and ia["ms"] > 0.0
    assert not ib["active"] and ib["code_bytes"] == 0
    return a, sa, b, sb


@pytest.mark.parametrize("ext", ["0", "1"])
@pytest.mark.parametrize("parts", [1, 2])
@pytest.mark.parametrize("kind", ["cbox_path_mis", "path_mats", "volumetric_basic"])
def test_shade_rtc_same_image(built, tmp_path, kind, parts, ext):
    s = _scene(kind, tmp_path)
    a, sa, b, sb = _pair(s, dict(NORI_EXT_INLINE=ext, NORI_POOL_PARTS=str(parts)), path_pool=4096)
    assert sa["ext_inline"] == int(ext) and sb["ext_inline"] == int(ext)
    assert sa["nee_inline"] == 1 and sb["nee_inline"] == 1
    _same(a, sa, b, sb)
    assert sa["rays_closest"] > sa["samples"] and sa["iterations"] > 8  # (cbox: 45 at 96x72, 8 spp)


def test_shade_rtc_queue_mode(built, tmp_path):
    # shadow rays through the queue and the shadow kernel: k_shade holds no scan at all
    s = _scene("cbox_path_mis", tmp_path)
    a, sa, b, sb = _pair(s, dict(NORI_NEE_INLINE="0"), path_pool=4096)
    assert sa["nee_inline"] == 0 and sa["ext_inline"] == 0
    _same(a, sa, b, sb)


@pytest.mark.parametrize("cull", ["0", "1"])
def test_shade_rtc_camera_waves(built, tmp_path, cull):
    # 1 spp, the pool larger than the work: every wave of the second launch
    # holds camera rays only, so it takes the in-plane filter scan (cull 1)
    s = _scene("cbox_path_mis", tmp_path, spp=1)
    a, sa, b, sb = _pair(s, dict(NORI_CAMERA_CULL=cull), path_pool=65536)
    assert sa["ext_inline"] == 1
    _same(a, sa, b, sb)


def test_shade_rtc_partial_segments(built, tmp_path):
    # 50 x 37 = 1850 pixels, no multiple of the 256-entry segment: lanes past
    # a segment's count from the first iteration on
    s = _scene("cbox_path_mis", tmp_path, width=50, height=37)
    a, sa, b, sb = _pair(s, {}, path_pool=4096)
    _same(a, sa, b, sb)


def test_shade_rtc_timing_render(built, tmp_path):
    # a timing render keeps the two-launch loop, with the same specialised object
    s = _scene("cbox_path_mis", tmp_path)
    a, sa, b, sb = _pair(s, {}, timing=True)
    _same(a, sa, b, sb)
    assert sa["ms_extend"] > 0.0 and sa["ms_shade"] > 0.0


def test_shade_rtc_against_no_rtc(built, tmp_path):
    # both programs against none: the specialised kernels of the loop and the generic ones
    s = _scene("cbox_path_mis", tmp_path)
    a, sa, ia = _render(s, dict(NORI_RTC_SHADE="1"), path_pool=4096)
    b, sb, ib = _render(s, dict(NORI_RTC="0"), path_pool=4096)
    assert ia["active"] and sa["scan_rtc"] == 1
    assert not ib["active"] and sb["scan_rtc"] == 0
    _same(a, sa, b, sb)


def test_shade_rtc_info(built):
    cbox = nori_amd.load_scene(scene_path("pa4", "cbox", "cbox_path_mis.xml"), 64, 48, 2)
    vol = nori_amd.load_scene(scene_path("project", "volumetric", "volumetric.xml"), 64, 48, 2)
    for s, env, on in ((cbox, {}, True), (cbox, dict(NORI_RTC="0"), False), (cbox, dict(NORI_RTC_SHADE="0"), False),
                       (cbox, dict(NORI_TRAVERSAL="bvh"), False), (vol, {}, False)):
        with _env(**env):
            with nori_amd.GpuRenderer(s, 0) as r:
                info = r.shade_rtc
        assert info["active"] == on, (env, info)
        assert (info["code_bytes"] > 10000) == on
    # the scan program's statistics keep their meaning: a context without the shade program still reports it
    _, st, info = _render(cbox, dict(NORI_RTC_SHADE="0"))
    assert st["scan_rtc"] == 1 and not info["active"]
