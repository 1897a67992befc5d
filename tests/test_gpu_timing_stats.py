"""GPU: which ms_* fields of nori_gpu_stats each call fills.  The kernel times come from HIP
events around the launches; every call that reports one goes through the same clock (ctx.h
KernelClock), so this file pins, per call, the fields that hold a time and the fields that
stay exactly 0.  cbox_path_mis at 64 x 64 and 8 passes, the suite's smallest render."""
import contextlib
import os

import numpy as np
import pytest

import nori_amd
from conftest import scene_path
import synth

pytestmark = pytest.mark.gpu

KERNEL_MS = ("ms_extend", "ms_shadow", "ms_shade", "ms_splat", "ms_finish")


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


def _cbox():
    return nori_amd.load_scene(scene_path("pa4", "cbox", "cbox_path_mis.xml"), 64, 64, 8)


def _check(st, positive, zero):
    print({k: st[k] for k in KERNEL_MS})
    for k in positive:
        assert st[k] > 0.0, (k, st[k])
    for k in zero:
        assert st[k] == 0.0, (k, st[k])


def _rays(n):
    """n rays from the Cornell box's opening towards its back half."""
    rng = np.random.default_rng(7)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = (0.0, 0.9, 1.5)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d[:, 2] = -np.abs(d[:, 2]) - 0.5
    rays[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 3], rays[:, 7] = 1e-4, np.inf
    return rays


def test_wavefront_render_timed(built):
    with nori_amd.GpuRenderer(_cbox(), 0) as r:
        r.render(timing=True)
        st = r.last_stats
    # the shadow rays have a launch (and a time) of their own unless k_shade traces them
    shadow = ("ms_shadow",)
    if st["nee_inline"] == 0:
        _check(st, ("ms_shade", "ms_extend", "ms_splat", "ms_finish") + shadow, ())
    else:
        _check(st, ("ms_shade", "ms_extend", "ms_splat", "ms_finish"), shadow)
    assert st["samples"] == 64 * 64 * 8


def test_wavefront_render_untimed(built):
    with nori_amd.GpuRenderer(_cbox(), 0) as r:
        r.render()
        st = r.last_stats
    _check(st, (), KERNEL_MS)
    assert st["samples"] == 64 * 64 * 8 and st["ms_total"] > 0.0


def test_one_bounce_render_timed(built, tmp_path):
    xml = synth.cbox_variant(str(tmp_path), "timing", integrator="direct_mis", width=64, height=64)
    s = nori_amd.load_scene(xml, 0, 0, 8)
    assert s.integrator == "direct_mis"
    with nori_amd.GpuRenderer(s, 0) as r:
        r.render(timing=True)
        _check(r.last_stats, ("ms_shade", "ms_splat"), ("ms_extend", "ms_shadow", "ms_finish"))
        r.render()
        _check(r.last_stats, (), KERNEL_MS)


def test_features_timed(built):
    with nori_amd.GpuRenderer(_cbox(), 0) as r:
        r.features(timing=True)
        _check(r.last_stats, ("ms_shade",), ())


def test_query_times_both_kernels_over_chunks(built):
    with _env(NORI_QUERY_CHUNK="300"), nori_amd.GpuRenderer(_cbox(), 0) as r:
        res = r.query(_rays(1000), surface=True)
        _check(r.last_stats, ("ms_extend", "ms_shade"), ())
        assert r.last_stats["rays_closest"] == 1000 and (res["hits"]["prim"] >= 0).any()


def test_any_hit_query_times_the_trace_only(built):
    """No k_surface launch, no k_surface time.  (Before the shared clock the call recorded its three
    events whether or not the second kernel ran, and ms_shade held the gap between two events with
    nothing between them: 0.0063 ms measured, against ms_extend 0.0095 ms.)"""
    with nori_amd.GpuRenderer(_cbox(), 0) as r:
        r.query(_rays(1000), any_hit=True)
        _check(r.last_stats, ("ms_extend",), ("ms_shade",))
        assert r.last_stats["rays_shadow"] == 1000


def test_film_splat_timed_over_chunks(built):
    s = _cbox()
    rng = np.random.default_rng(3)
    pos = (rng.random((1000, 2)) * (s.width, s.height)).astype(np.float32)
    val = rng.random((1000, 3)).astype(np.float32)
    with _env(NORI_QUERY_CHUNK="300"), nori_amd.GpuRenderer(s, 0) as r:
        film = r.film_splat(pos, val)
        _check(r.last_stats, ("ms_splat",), ())
        assert r.last_stats["samples"] == 1000 and film[..., 3].sum() > 0.0
