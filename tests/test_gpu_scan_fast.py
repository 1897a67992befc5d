"""GPU: the fast body of the scene-specialised scan (scan.h: one wave-uniform
guard instead of the per-test range checks, the products with literally zero
record components left out) finds what the generic scan finds.  The trace API
runs one fixed set of about 65k rays -- uniform rays inside the box; origins
exactly on the wall planes and on the spheres; directions with one and two
exactly zero components, +0 and -0; rays lying in a wall's plane; rays through
the shared edge, the outer edges and the corners of every pair (ties at equal
t); path-ray and camera-ray intervals; and rays the guard must turn away
(+-inf, NaN, 2^100), whole waves of them and single lanes -- through the scan
program with the fast body and through the library's generic kernels
(NORI_RTC=0), closest hit and any hit.  The contract of scan.h: t and the
primitive id bit for bit, u and v equal as values, occlusion equal.  The
specialised program without the fast body (NORI_SCAN_FAST=0) is held to the
same."""
import numpy as np
import pytest

import nori_amd
from scan_fast_util import KINDS, env, ray_set, scene

pytestmark = pytest.mark.gpu
f32 = np.float32


def _trace(s, rays, sh, **kv):
    with env(**kv):
        with nori_amd.GpuRenderer(s, 0) as r:
            hit, occ = r.trace(rays), r.trace(sh, any_hit=True)
            r.render(passes=1)
            return hit, occ["prim"] >= 0, r.last_stats["scan_rtc"], r.shade_rtc["code_bytes"]


def _same_value(a, b):
    return np.array_equal(a, b, equal_nan=True)  # (== on floats: -0 and +0 are the same value)


@pytest.mark.parametrize("kind", KINDS)
def test_fast_scan_same_hits(built, kind, tmp_path):
    s = scene(kind, tmp_path)
    assert nori_amd.scan_fast_max(s) >= 1024.0  # these scenes get the fast body
    with env(NORI_SCAN_FAST="0"):
        assert nori_amd.scan_fast_max(s) == 0.0
    rays = ray_set(s)
    sh = rays.copy()
    sh[:, 7] = np.random.default_rng(7).uniform(0.01, 2.0, size=len(sh)).astype(f32)
    gen, gen_occ, gen_rtc, _ = _trace(s, rays, sh, NORI_RTC="0")
    assert gen_rtc == 0
    nhit = int(np.isfinite(gen["t"]).sum())
    print(kind, len(rays), "rays,", nhit, "hits,", int(gen_occ.sum()), "occluded")
    assert nhit > len(rays) // 2
    size = {}
    for fast in ("1", "0"):
        got, occ, rtc, size[fast] = _trace(s, rays, sh, NORI_SCAN_FAST=fast)
        assert rtc == 1
        assert np.array_equal(got["t"].view(np.uint32), gen["t"].view(np.uint32)), fast
        assert np.array_equal(got["prim"], gen["prim"]), fast
        assert _same_value(got["u"], gen["u"]) and _same_value(got["v"], gen["v"]), fast
        assert np.array_equal(occ, gen_occ), fast
    # what the contexts loaded, not what the host would compute again: both programs are generated
    # from one scene record, and the one with the second body is larger by more than a page
    print(kind, "shade program bytes with / without the fast body:", size["1"], size["0"])
    assert size["0"] > 10000 and size["1"] > size["0"] + 4096
