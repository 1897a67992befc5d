"""The host side of the specialised scan's fast body (scene_prep.cpp
scan_fast_max, scan.h): the bound under which a ray keeps every intermediate
of the triangle tests at or below 2^125.  The three scenes whose shade kernel
holds the scans get one; a Cornell box scaled by 2^55 -- 6 M E^2, the bound on
det, would pass 2^125 for any M that leaves room for rays around the scene --
gets none, and its programs compile without the fast body; NORI_SCAN_FAST=0
switches it off.  The shade program compiles for gfx950 with a cold cache
either way (no device needed), and the fast body is what makes it larger."""
import os
import re

import pytest

import nori_amd
from conftest import scene_path
from scan_fast_util import KINDS, env, scene


def _compile(fn, s):
    return fn(s, "gfx950")  # (a missing hipRTC is an error here, not a skip)


def _scaled_cbox(tmp_path, scale):
    """The Cornell box with every mesh vertex multiplied by `scale` (a power of two: exact)."""
    src = open(scene_path("pa4", "cbox", "cbox_path_mis.xml")).read()
    mesh_dir = scene_path("pa4", "cbox", "meshes")
    out_dir = tmp_path / f"x{scale:g}"
    out_dir.mkdir()
    for name in sorted(os.listdir(mesh_dir)):
        if not name.endswith(".obj"):
            continue
        out = []
        for line in open(os.path.join(mesh_dir, name)):
            p = line.split()
            if p and p[0] == "v":
                line = "v " + " ".join(repr(float(x) * scale) for x in p[1:4]) + "\n"
            out.append(line)
        open(out_dir / name, "w").write("".join(out))
    src = src.replace('value="meshes/', f'value="{out_dir}/')
    xml = str(out_dir / "scaled.xml")
    open(xml, "w").write(src)
    return nori_amd.load_scene(xml, 32, 32, 1)


@pytest.mark.parametrize("kind", KINDS)
def test_bound_accepts_the_scan_scenes(built, kind, tmp_path):
    s = scene(kind, tmp_path, 32, 32, 1)
    m = nori_amd.scan_fast_max(s)
    print(kind, "fast_max =", m)
    # a power of two, at most 2^60, with room for every ray in and around the scene
    assert 1024.0 <= m <= 2.0 ** 60 and re.fullmatch(r"0x1\.0+p\+\d+", float(m).hex())
    rec = nori_amd.scan_list(s)["records"]
    assert m >= 16.0 * abs(rec[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]]).max()
    with env(NORI_SCAN_FAST="0"):
        assert nori_amd.scan_fast_max(s) == 0.0


def test_bound_of_a_bvh_scene_is_zero(built):
    s = nori_amd.load_scene(scene_path("pa1", "sphere-mesh.xml"), 32, 32, 1)
    assert nori_amd.scan_fast_max(s) == 0.0


def test_bound_refuses_a_scene_out_of_range(built, tmp_path, monkeypatch):
    monkeypatch.setenv("NORI_RTC_CACHE", str(tmp_path / "cache"))  # a cold cache: really compile
    big = _scaled_cbox(tmp_path, 2.0 ** 55)
    assert len(nori_amd.scan_list(big)["records"]) > 0  # still a scan scene
    assert nori_amd.scan_fast_max(big) == 0.0
    # (scaling alone is no reason; and a scene of this test's own, so that the process cache of
    # compiled programs holds nothing another test file expects to compile itself)
    cbox = _scaled_cbox(tmp_path, 2.0 ** 10)
    assert nori_amd.scan_fast_max(cbox) > 0.0
    n_fast, ms_fast = _compile(nori_amd.shade_rtc, cbox)
    with env(NORI_SCAN_FAST="0"):
        n_plain, ms_plain = _compile(nori_amd.shade_rtc, cbox)
    n_big, ms_big = _compile(nori_amd.shade_rtc, big)
    print("shade program bytes: fast", n_fast, "NORI_SCAN_FAST=0", n_plain, "scaled scene", n_big,
          f"cold compile {ms_fast:.0f} / {ms_plain:.0f} / {ms_big:.0f} ms")
    assert n_plain > 10000 and n_big > 10000
    assert n_fast > n_plain + 4096  # the second body is in the first program only ...
    assert n_big < n_plain + 4096  # ... and not in the scaled scene's
    # the scan program, which carries five kernels with the second body, compiles cold as well
    n_scan, ms_scan = _compile(nori_amd.scan_rtc, cbox)
    n_scan_big, _ = _compile(nori_amd.scan_rtc, big)
    print("scan program bytes: fast", n_scan, "scaled scene", n_scan_big, f"cold compile {ms_scan:.0f} ms")
    assert n_scan > n_scan_big + 4096 and n_scan_big > 10000
