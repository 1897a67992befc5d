"""Shared by test_scan_fast.py, test_gpu_scan_fast.py and test_gpu_shade_fast.py:
the three scenes whose shade kernel holds the scans (tests/test_shade_rtc.py's),
and the fixed ray set for the trace API."""
import contextlib
import os
import re

import numpy as np

import nori_amd
from conftest import scene_path
import synth

f32 = np.float32
KINDS = ["cbox_path_mis", "path_mats", "volumetric_basic"]


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def scene(kind, tmp_path, width=64, height=64, spp=8):
    if kind == "cbox_path_mis":
        return nori_amd.load_scene(scene_path("pa4", "cbox", "cbox_path_mis.xml"), width, height, spp)
    if kind == "volumetric_basic":  # the Disney sphere made diffuse: the basic plugin set
        src = open(scene_path("project", "volumetric", "volumetric.xml")).read()
        src = src.replace('value="meshes/', f'value="{scene_path("project", "volumetric", "meshes")}/')
        src = re.sub(r'<bsdf type="disney">.*?</bsdf>',
                     '<bsdf type="diffuse"><color name="albedo" value="0.5 0.5 0.5"/></bsdf>', src, flags=re.S)
        xml = str(tmp_path / f"{kind}.xml")
        open(xml, "w").write(src)
        return nori_amd.load_scene(xml, width, height, spp)
    assert kind == "path_mats"
    xml = synth.cbox_variant(str(tmp_path), kind, integrator="path_mats", width=width, height=height)
    return nori_amd.load_scene(xml, 0, 0, spp)


def _dirs(rng, n):
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)


def ray_set(s, seed=101):
    """About 65k rays (65 024 for the Cornell box), (n, 8) = o, mint, d, maxt, in blocks of whole
    waves (multiples of 64) so that the blocks meant for the fast body are not mixed with the rays that the guard sends to the
    checked one -- except the last block, which mixes both inside its waves."""
    L = nori_amd.scan_list(s)
    rec = L["records"]
    tri = np.arange(len(rec)) < L["tris"]
    real = tri & (np.abs(rec[:, 4:7]).sum(axis=1) > 0)
    v0, e1, e2 = rec[real, 0:3], rec[real, 4:7], rec[real, 8:11]
    pts = np.concatenate([v0, v0 + e1, v0 + e2])
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    sph = rec[~tri]
    rng = np.random.default_rng(seed)
    npairs = len(L["plane_c"])
    assert npairs > 0
    axis = [int(np.searchsorted(L["plane_end"], g, side="right")) for g in range(npairs)]
    blocks = []

    def inside(n):
        return rng.uniform(lo, hi, size=(n, 3)).astype(f32)

    # 1. uniform rays from inside the box
    blocks.append((inside(22528), _dirs(rng, 22528)))
    # 2. origins exactly on each wall plane, and on the spheres
    o, d = inside(8192), _dirs(rng, 8192)
    for i in range(len(o)):
        g = i % npairs
        o[i, axis[g]] = L["plane_c"][g]
    blocks.append((o, d))
    if len(sph):
        n = 4096
        k = rng.integers(0, len(sph), n)
        o = (sph[k, 0:3] + sph[k, 4:5] * _dirs(rng, n)).astype(f32)
        blocks.append((o, _dirs(rng, n)))
    # 3. directions with one and two exactly zero components, +0 and -0
    o, d = inside(8192), _dirs(rng, 8192)
    a = rng.integers(0, 3, len(d))
    b = (a + rng.integers(1, 3, len(d))) % 3
    two = rng.random(len(d)) < 0.5
    d[np.arange(len(d)), a] = np.where(rng.random(len(d)) < 0.5, f32(0.0), f32(-0.0))
    d[two, b[two]] = np.where(rng.random(two.sum()) < 0.5, f32(0.0), f32(-0.0))
    blocks.append((o, d))
    # 4. rays lying in a wall's plane
    o, d = inside(4096), _dirs(rng, 4096)
    for i in range(len(o)):
        g = i % npairs
        o[i, axis[g]] = L["plane_c"][g]
        d[i, axis[g]] = f32(-0.0) if i & 8 else f32(0.0)
    blocks.append((o, d))
    # 5. axis-parallel and aimed rays through the shared edge, the outer edges and the corners of
    # each pair (points k / 64 along an edge: both triangles of a pair accept the ones on their
    # common edge at the same t, which the tie rule decides)
    os_, ds = [], []
    for g in range(npairs):
        A = axis[g]
        ra, rb = rec[2 * g], rec[2 * g + 1]
        corners = [r[0:3] + x for r in (ra, rb) if np.abs(r[4:7]).sum() > 0 for x in (0 * r[4:7], r[4:7], r[8:11])]
        for i in range(len(corners)):
            for j in range(i + 1, len(corners)):
                p = corners[i] + (np.arange(65, dtype=f32) / f32(64))[:, None] * (corners[j] - corners[i])
                p = p.astype(f32)
                o = p.copy()
                o[:, A] = f32(0.5) * (lo[A] + hi[A]) + f32(0.125) * (hi[A] - lo[A])
                dd = np.zeros_like(p)
                dd[:, A] = p[:, A] - o[:, A]  # along the axis, towards the plane
                os_.append(o), ds.append(dd)
                o2 = inside(len(p))
                os_.append(o2), ds.append((p - o2).astype(f32))  # from anywhere, unnormalised
    o, d = np.concatenate(os_), np.concatenate(ds)
    n = min(len(o) // 64 * 64, 12288)
    sel = rng.permutation(len(o))[:n]
    blocks.append((o[sel], d[sel]))
    o, d = np.concatenate([b[0] for b in blocks]), np.concatenate([b[1] for b in blocks])
    # mint / maxt of path rays (Epsilon scaled as scan_prologue's callers do, inf) and of camera rays
    mint = np.maximum(f32(1e-4), f32(1e-4) * np.abs(o).max(axis=1)).astype(f32)
    maxt = np.full(len(o), np.inf, f32)
    cam = rng.random(len(o)) < 0.3
    maxt[cam] = (rng.uniform(0.05, 2.0, cam.sum()) * np.linalg.norm(hi - lo)).astype(f32)
    mint[cam] = rng.uniform(1e-4, 1e-2, cam.sum()).astype(f32)
    # 6. the rays that must not take the fast body: a component that is +-inf, NaN, +-2^100 (beyond
    # every bound) -- and denormal components, which are within it and harmless there; the first
    # half as whole waves, the second half scattered among ordinary rays
    n = 8192
    o6, d6 = inside(n), _dirs(rng, n)
    special = np.array([np.inf, -np.inf, np.nan, 2.0 ** 100, -2.0 ** 100, 1e-40, -1e-42, 2.0 ** 100], f32)
    od = np.concatenate([o6, d6], axis=1)
    which = rng.integers(0, 6, n)
    hitme = np.ones(n, bool)
    hitme[n // 2:] = rng.random(n - n // 2) < 0.1
    od[hitme, which[hitme]] = special[rng.integers(0, len(special), hitme.sum())]
    o = np.concatenate([o, od[:, :3]])
    d = np.concatenate([d, od[:, 3:]])
    mint = np.concatenate([mint, np.full(n, 1e-4, f32)])
    maxt = np.concatenate([maxt, np.full(n, np.inf, f32)])
    rays = np.zeros((len(o), 8), f32)
    rays[:, :3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, mint, d, maxt
    return rays
