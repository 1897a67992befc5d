"""The scene's own shade kernel (csrc/rtc.hip, the shade program): the
library's embedded shade_kernel.h compiles through hipRTC for gfx950 with a
scene's scan list as literals (no device needed) for each basic-plugin
integrator of the wavefront loop; scenes whose k_shade holds no scan (BVH
traversal, the full plugin set) have nothing to compile; a damaged cache
file is replaced by a fresh compile, never used.  Parity of the specialised
kernel with the ahead-of-time one is the GPU suite's (test_gpu_shade_rtc.py)."""
import re

import pytest

import nori_amd
from conftest import scene_path
import synth


def _scene(kind, tmp_path):
    if kind == "cbox_path_mis":
        return nori_amd.load_scene(scene_path("pa4", "cbox", "cbox_path_mis.xml"), 32, 32, 1)
    if kind == "volumetric_basic":  # test_gpu_ext_inline.py's: the Disney sphere made diffuse
        src = open(scene_path("project", "volumetric", "volumetric.xml")).read()
        src = src.replace('value="meshes/', f'value="{scene_path("project", "volumetric", "meshes")}/')
        src = re.sub(r'<bsdf type="disney">.*?</bsdf>',
                     '<bsdf type="diffuse"><color name="albedo" value="0.5 0.5 0.5"/></bsdf>', src, flags=re.S)
        xml = str(tmp_path / f"{kind}.xml")
        open(xml, "w").write(src)
        return nori_amd.load_scene(xml, 32, 32, 1)
    assert kind == "path_mats"
    xml = synth.cbox_variant(str(tmp_path), kind, integrator="path_mats", width=32, height=32)
    return nori_amd.load_scene(xml, 0, 0, 1)


def _compile(s):
    try:
        return nori_amd.shade_rtc(s, "gfx950")
    except nori_amd.NoriError as e:
        if "libhiprtc not found" in str(e):
            pytest.skip("hipRTC is not installed")
        raise


@pytest.mark.parametrize("kind", ["cbox_path_mis", "path_mats", "volumetric_basic"])
def test_shade_rtc_compiles(built, kind, tmp_path, monkeypatch):
    cache = tmp_path / "cache"
    monkeypatch.setenv("NORI_RTC_CACHE", str(cache))  # a cold cache: really compile
    s = _scene(kind, tmp_path)
    n, ms = _compile(s)
    print(f"{kind}: {n} bytes, cold {ms:.1f} ms")
    assert n > 10000 and ms > 0.0
    assert len(list(cache.glob("shade_*.co"))) == 1
    assert not list(cache.glob("*.tmp*"))  # the writer's temporary file was renamed into place
    assert cache.stat().st_mode & 0o777 == 0o700
    n2, ms2 = nori_amd.shade_rtc(s, "gfx950")  # the process cache
    print(f"{kind}: cached {ms2:.3f} ms")
    assert n2 == n and ms2 < ms
    assert len(list(cache.glob("*.co"))) == 1  # (the scan program's scan_*.co is test_scan_rtc.py's)


def test_shade_rtc_nothing_to_specialise(built, monkeypatch, tmp_path):
    monkeypatch.setenv("NORI_RTC_CACHE", str(tmp_path))
    bvh = nori_amd.load_scene(scene_path("pa1", "sphere-mesh.xml"), 32, 32, 1)
    assert len(nori_amd.scan_list(bvh)["records"]) == 0  # a BVH scene
    assert nori_amd.shade_rtc(bvh, "gfx950") == (0, 0.0)
    full = nori_amd.load_scene(scene_path("project", "volumetric", "volumetric.xml"), 32, 32, 1)
    assert len(nori_amd.scan_list(full)["records"]) > 0  # scan mode, but the full plugin set (Disney)
    assert nori_amd.shade_rtc(full, "gfx950") == (0, 0.0)
    assert not list(tmp_path.glob("shade_*.co"))


_CHILD = """
import sys
sys.path[:0] = {path!r}
import nori_amd
s = nori_amd.load_scene({scene!r}, 32, 32, 1)
n, ms = nori_amd.shade_rtc(s, "gfx950")
print("RESULT", n, ms)
"""


def _child_compile():
    """(bytes, ms) of the Cornell box's shade program as a fresh interpreter gets it (this
    process would answer from its in-memory cache and never touch the file)."""
    import subprocess
    import sys

    code = _CHILD.format(path=[p for p in sys.path if p], scene=scene_path("pa4", "cbox", "cbox_path_mis.xml"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    if "libhiprtc not found" in out.stderr:
        pytest.skip("hipRTC is not installed")
    assert out.returncode == 0, out.stderr[-2000:]
    n, ms = out.stdout.split("RESULT")[1].split()
    return int(n), float(ms)


@pytest.mark.parametrize("damage", ["truncated", "empty", "not_elf"])
def test_shade_rtc_replaces_a_damaged_cache_file(built, damage, tmp_path, monkeypatch):
    """A cached object that is empty, cut short or no ELF image is compiled
    afresh and replaced, not used; an intact one is read.  Each request comes
    from a fresh interpreter: reading the file is what the test is about."""
    cache = tmp_path / "cache"
    monkeypatch.setenv("NORI_RTC_CACHE", str(cache))
    n, cold = _child_compile()
    (path,) = cache.glob("shade_*.co")
    good = path.read_bytes()
    assert good[:4] == b"\x7fELF" and len(good) == n
    n1, warm = _child_compile()  # the intact file is read, not compiled again
    assert n1 == n and warm < cold / 10
    path.write_bytes({"truncated": good[:len(good) // 2], "empty": b"", "not_elf": b"X" * len(good)}[damage])
    n2, again = _child_compile()
    print(f"{damage}: cold {cold:.1f} ms, from the file {warm:.2f} ms, after the damage {again:.1f} ms")
    assert n2 == n
    assert again > cold / 4  # a compile, not a file read
    (path2,) = cache.glob("shade_*.co")  # the same key, no stray temporary file
    assert path2 == path and not list(cache.glob("*.tmp*"))
    fresh = path.read_bytes()
    assert fresh[:4] == b"\x7fELF" and len(fresh) == n


def test_abi_version_is_still_7(built):
    from nori_amd import _abi

    assert _abi.ABI_VERSION == 7 and nori_amd.lib().nori_gpu_abi_version() == 7
