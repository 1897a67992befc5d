"""The host arithmetic of scene preparation (nori-ray-tracer_amd/csrc/scene_prep.h: scene box, BVH
build, scan list and its in-plane filters, filter table, block spiral, area CDFs, environment-map
tables, solitary spheres, shares of a sharded render) under the address and undefined-behaviour
sanitizers: tests/scene_prep_check.cpp links the host-compiled units alone, so it runs as a plain
program, without Python in the process and without a device.  Its hashes of the scan list, the
plane filters, the filter table and the BVH info must equal those of the same arrays from the built
library (nori_scene_scan_list, nori_filter_table, nori_scene_bvh_info)."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import nori_amd
import synth
from conftest import ROOT, scene_path

CSRC = os.path.join(ROOT, "nori-ray-tracer_amd", "csrc")
UNITS = ["scene_prep.cpp", "scene_plan.cpp", "shard.cpp", "scene_loader.cpp", "bvh_builder.cpp", "bvh_refit.cpp", "bvh_rebuild.cpp",
         "image_decode.cpp", "image_io.cpp"]
SCENES = [("pa4", "cbox", "cbox_path_mis.xml"), ("pa3", "odyssey", "odyssey_mis.xml"), ("pa3", "veach_mi", "veach_mis.xml")]


def fnv1a(*arrays):
    h = 1469598103934665603
    for a in arrays:
        for b in (a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes()):
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_scene_prep_sanitized(built, tmp_path):
    exe = tmp_path / "scene_prep_check"
    gxx = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", CSRC]
    srcs = [os.path.join(ROOT, "tests", "scene_prep_check.cpp")] + [os.path.join(CSRC, u) for u in UNITS]
    objs = [str(tmp_path / (os.path.basename(s) + ".o")) for s in srcs]
    jobs = [subprocess.Popen(gxx + ["-c", s, "-o", o]) for s, o in zip(srcs, objs)]  # the units side by side
    assert [j.wait() for j in jobs] == [0] * len(jobs)
    # the sanitizer runtime is linked into the program: with the shared one ASan refuses to start
    # wherever the environment preloads any other library
    subprocess.run(gxx + ["-static-libasan"] + objs + ["-o", str(exe), "-lz"], check=True)
    xmls = [scene_path(*p) for p in SCENES]
    xmls.append(synth.envmap_scene(str(tmp_path), 32, 32, 1, rows=32, cols=64))  # no envmap scene ships in scenes/
    r = subprocess.run([str(exe)] + xmls, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stderr == "", r.stderr[-4000:]  # the sanitizers' reports go to stderr

    got, cur = {}, None
    for line in r.stdout.splitlines():
        name, value = line.split(" ", 1)
        if name == "scene":
            cur = got.setdefault(value, {})
        else:
            cur[name] = value
    assert list(got) == xmls
    assert got[xmls[1]]["scan_pairs"] == "18" and got[xmls[3]]["envmaps"] == "1"
    for xml in xmls:
        s, g = nori_amd.load_scene(xml), got[xml]
        assert g["filter_table"] == fnv1a(s.filter_table()), xml
        assert int(g["film_border"]) == s.border, xml
        i = nori_amd.bvh_info(s)
        assert g["bvh_info"] == fnv1a(struct.pack("<4IfQ", i["ref_nodes"], i["device_nodes"], i["depth"], i["num_prims"],
                                                  i["sah_cost"], i["order_hash"])), xml
        nodes, prims, _ = nori_amd.bvh_refit(s)
        assert g["bvh_arrays"] == fnv1a(nodes, prims), xml
        sl = nori_amd.scan_list(s)
        assert ("scan_records" in g) == (len(sl["records"]) > 0), xml
        if "scan_records" in g:
            assert g["scan_records"] == fnv1a(sl["records"]), xml
            assert g["plane_c"] == fnv1a(sl["plane_c"]) and g["plane_f"] == fnv1a(sl["plane_f"]), xml
            assert int(g["scan_pairs"]) == len(sl["plane_c"]), xml
