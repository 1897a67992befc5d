"""GPU: renders through the shade kernel whose scans carry the fast body
(scan.h) against the ahead-of-time kernel (NORI_RTC_SHADE=0) and against the
specialised kernel built without it (NORI_SCAN_FAST=0): 64 x 64 at 8 spp of
the three scenes whose shade kernel holds the scans, at the default pool and
with the pool forced to 4096 paths, where waves mix survivors with new
samples and shadow slots with regenerating lanes.  The scans find the same
hits, so the ray, sample and iteration counts are equal exactly and the films
to the bar of tests/test_gpu_shade_rtc.py (the film's atomic sums differ in
their order from run to run)."""
import numpy as np
import pytest

import nori_amd
from scan_fast_util import KINDS, env, scene

pytestmark = pytest.mark.gpu

COUNTERS = ("samples", "invalid_samples", "rays_closest", "rays_shadow", "rays_finish", "iterations")


def _render(s, kv, **kw):
    # NORI_LOOKAHEAD=0: the host launches exactly the iterations the work needs (test_gpu_shade_rtc.py)
    with env(**dict(kv, NORI_LOOKAHEAD="0")):
        with nori_amd.GpuRenderer(s, 0) as r:
            img = r.render(**kw)
            return img, r.last_stats, r.shade_rtc


@pytest.mark.parametrize("pool", [0, 4096])
@pytest.mark.parametrize("kind", KINDS)
def test_fast_shade_same_render(built, kind, pool, tmp_path):
    s = scene(kind, tmp_path, 64, 64, 8)
    assert nori_amd.scan_fast_max(s) >= 1024.0
    a, sa, ia = _render(s, dict(NORI_RTC_SHADE="1"), path_pool=pool)
    assert ia["active"] and sa["scan_rtc"] == 1 and sa["ext_inline"] == 1 and sa["nee_inline"] == 1
    assert sa["samples"] == 64 * 64 * 8 and sa["rays_closest"] >= sa["samples"]
    if pool:  # (the default pool holds the whole frame: its loop hands the paths to the finisher early)
        assert sa["iterations"] > 8 and sa["rays_closest"] > sa["samples"]
    for kv in (dict(NORI_RTC_SHADE="0"), dict(NORI_RTC_SHADE="1", NORI_SCAN_FAST="0")):
        b, sb, ib = _render(s, kv, path_pool=pool)
        assert ib["active"] == (kv["NORI_RTC_SHADE"] == "1")
        print(kind, pool, kv, "max |a - b| =", np.abs(a - b).max(), {k: (sa[k], sb[k]) for k in COUNTERS})
        for k in COUNTERS:
            assert sa[k] == sb[k], (k, sa[k], sb[k])
        assert np.allclose(a, b, rtol=1e-5, atol=1e-6), np.abs(a - b).max()
    assert a.mean() > 0.0
