"""The scene plan (nori-ray-tracer_amd/csrc/scene_plan.h: the refusals of a bad scene description,
the knobs, the decisions, the host tables and the small-scene blob) on the CPU, under the address
and undefined-behaviour sanitizers: tests/scene_plan_check.cpp links the host-compiled units alone
and runs as a plain program, without Python in the process and without a device.  The hashes it
prints of every table and decision must equal those nori_gpu_create computed before the plan
existed (tests/golden/scene_plan_hashes.json, recorded from the commit named there)."""
import json
import os
import shutil
import subprocess

import pytest

import synth
from conftest import ROOT, scene_path

PKG = os.path.join(ROOT, "nori-ray-tracer_amd")
CSRC = os.path.join(PKG, "csrc")
UNITS = ["scene_plan.cpp", "scene_prep.cpp", "shard.cpp", "scene_loader.cpp", "bvh_builder.cpp", "bvh_refit.cpp",
         "bvh_rebuild.cpp", "image_decode.cpp", "image_io.cpp"]
GOLDEN = os.path.join(ROOT, "tests", "golden", "scene_plan_hashes.json")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_scene_plan_sanitized(tmp_path):
    exe = tmp_path / "scene_plan_check"
    gxx = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-pthread",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC]
    srcs = [os.path.join(ROOT, "tests", "scene_plan_check.cpp")] + [os.path.join(CSRC, u) for u in UNITS]
    objs = [str(tmp_path / (os.path.basename(s) + ".o")) for s in srcs]
    jobs = [subprocess.Popen(gxx + ["-c", s, "-o", o]) for s, o in zip(srcs, objs)]  # the units side by side
    assert [j.wait() for j in jobs] == [0] * len(jobs)
    # the sanitizer runtime is linked into the program: with the shared one ASan refuses to start
    # wherever the environment preloads any other library
    subprocess.run(gxx + ["-static-libasan"] + objs + ["-o", str(exe), "-lz"], check=True)
    scenes = {
        "cbox": scene_path("pa4", "cbox", "cbox_path_mis.xml"),
        "odyssey": scene_path("pa3", "odyssey", "odyssey_mis.xml"),
        "veach": scene_path("pa3", "veach_mi", "veach_mis.xml"),
        "envmap": synth.envmap_scene(str(tmp_path), 32, 32, 1, rows=32, cols=64),
        "textured": scene_path("project", "textured", "cbox_path_mis.xml"),
        "bvh": synth.heightfield_scene(str(tmp_path), n=8, width=32, height=32, spp=1),  # 140 primitives: BVH mode
    }
    env = {k: v for k, v in os.environ.items() if not k.startswith("NORI_")}  # (the units' own A/B knobs)
    r = subprocess.run([str(exe)] + list(scenes.values()), capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert r.stderr == "", r.stderr[-4000:]  # the sanitizers' reports go to stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok"

    got, cur = {}, None
    for line in lines[:-1]:
        name, value = line.split(" ", 1)
        if name == "scene":
            cur = got.setdefault(value, {})
        else:
            cur[name] = value
    assert list(got) == list(scenes.values())
    want = json.load(open(GOLDEN))["scenes"]
    assert sorted(want) == sorted(scenes)
    for key, xml in scenes.items():
        assert sorted(got[xml]) == sorted(want[key]), key
        differ = [n for n in want[key] if got[xml][n] != want[key][n]]
        assert not differ, (key, differ)


def test_scene_plan_is_host_pure():
    """No HIP in the unit; the knobs' text is read in one place and the runtime keeps no second
    statement of the blob layout or the traversal rule."""
    for f in ("scene_plan.h", "scene_plan.cpp", "dev_records.h"):
        text = open(os.path.join(CSRC, f)).read()
        assert "#include <hip" not in text and "getenv(" not in text, f
    upload = open(os.path.join(CSRC, "upload.hip")).read()
    assert upload.count("getenv") == 1 and "scene_blob_bytes" not in upload and "kScanMaxPrims" not in upload
    for f in ("upload.hip", "scene_prep.cpp"):
        assert "build_device_bvh" not in open(os.path.join(CSRC, f)).read(), f
