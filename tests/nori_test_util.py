"""Test helpers: the reference's statistical harness restated in Python.

students_t_test  <- hypothesis::students_t_test (ext/hypothesis/hypothesis.h:314-345)
parse_test_xml   <- StudentsTTest property parsing (src/ttest.cpp:60-80)
load_test_scenes <- <test type="ttest"> children: each <scene> is written to its
                    own XML next to the original so relative OBJ paths resolve.
"""
import os
import xml.etree.ElementTree as ET

import numpy as np
from scipy import stats

import nori_amd


def students_t_test(mean, variance, reference, n, alpha, num_tests):
    t = abs(mean - reference) * np.sqrt(n / max(variance, 1e-5))
    p = 2 * (1 - stats.t.cdf(t, n - 1))
    sidak = 1.0 - (1.0 - alpha) ** (1.0 / num_tests)
    ok = not (p < sidak or not np.isfinite(p))
    return ok, p


def _floats(s):
    return [float(x) for x in s.replace(",", " ").split()]


def parse_test_xml(path):
    root = ET.parse(path).getroot()
    out = {"sampleCount": 100000, "significanceLevel": 0.01, "angles": [], "references": []}
    for ch in root:
        name = ch.get("name")
        if ch.tag == "string" and name in ("references", "angles"):
            out[name] = _floats(ch.get("value"))
        elif ch.tag == "integer" and name == "sampleCount":
            out["sampleCount"] = int(ch.get("value"))
        elif ch.tag == "float" and name == "significanceLevel":
            out["significanceLevel"] = float(ch.get("value"))
        elif ch.tag == "bsdf":
            props = {}
            for p in ch:
                v = p.get("value")
                props[p.get("name")] = _floats(v) if p.tag == "color" else float(v)
            out["bsdf_props"] = props
            out["bsdf_type"] = ch.get("type")
    return out


def load_test_scenes(path, tmpdir, width=0, height=0, spp=0):
    """Return [(Scene, integrator name)] for every <scene> child of a test XML."""
    root = ET.parse(path).getroot()
    base = os.path.dirname(os.path.abspath(path))
    res = []
    for i, sc in enumerate([c for c in root if c.tag == "scene"]):
        # rewrite relative filenames to absolute so the temp XML can live anywhere
        for s in sc.iter("string"):
            if s.get("name") == "filename" and not os.path.isabs(s.get("value")):
                s.set("value", os.path.join(base, s.get("value")))
        p = os.path.join(str(tmpdir), f"scene_{i}.xml")
        ET.ElementTree(sc).write(p)
        scene = nori_amd.load_scene(p, width, height, spp)
        res.append((scene, scene.integrator))
    return res


def read_png(path):
    """8-bit non-interlaced PNG (grey / RGB / RGBA) -> uint8 (H, W, C).

    Independent test-side decoder (PNG spec: zlib stream of scanlines, each
    prefixed by a filter type 0..4), used to open the reference's LDR renders
    and to check the product's own PNG codec."""
    import struct
    import zlib

    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n", path
    pos, idat, hdr = 8, [], None
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if kind == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
        pos += 12 + n
    w, h, depth, ctype, _, _, interlace = hdr
    assert depth == 8 and interlace == 0 and ctype in (0, 2, 6), hdr
    ch = {0: 1, 2: 3, 6: 4}[ctype]
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8).reshape(h, 1 + w * ch)
    out = np.zeros((h, w * ch), np.int32)
    prev = np.zeros(w * ch, np.int32)
    for y in range(h):
        f, line = raw[y, 0], raw[y, 1:].astype(np.int32)
        cur = np.zeros(w * ch, np.int32)
        if f == 0:
            cur = line
        elif f == 2:
            cur = (line + prev) & 255
        else:
            for x in range(w * ch):  # 1, 3, 4 depend on the left neighbour
                a = cur[x - ch] if x >= ch else 0
                b = prev[x]
                c = prev[x - ch] if x >= ch else 0
                if f == 1:
                    p = a
                elif f == 3:
                    p = (a + b) >> 1
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    p = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                cur[x] = (line[x] + p) & 255
        out[y] = cur
        prev = cur
    return out.reshape(h, w, ch).astype(np.uint8)


def png_linear(path):
    """A reference LDR render back to linear RGB (inverse sRGB, float64).

    The PNGs were written by Bitmap::saveToLDR (bitmap.cpp:109-139): clamp to
    [0, 1], sRGB encode, 8-bit.  Linearising and comparing block means keeps
    the comparison unbiased by Monte Carlo noise (the sRGB curve is concave,
    so noisier images have darker 8-bit means)."""
    v = read_png(path)[..., :3].astype(np.float64) / 255.0
    return np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)


# (scene XML under scenes/, PNG under tests/golden/, rendered spp of the PNG)
# Every pair renders the scene file the reference fork committed next to the
# PNG (scenes/project/**, pa4/cbox); see DESIGN.md section 2 for the three
# reference PNGs that were rendered with parameters other than the committed
# XML's (disney/cbox_path_mis.png, volumetric.png, disney/images/sheen_only.png).
REFERENCE_PNG_PAIRS = [
    ("pa4/cbox/cbox_path_mis.xml", "cbox_path_mis.png"),                       # C2 scene: mirror + dielectric
    ("project/disney/specular_rough_00.xml", "project/disney_specular_rough_00.png"),
    ("project/disney/specular_rough_03.xml", "project/disney_specular_rough_03.png"),
    ("project/disney/specular_rough_05.xml", "project/disney_specular_rough_05.png"),
    ("project/disney/specular_rough_08.xml", "project/disney_specular_rough_08.png"),
    ("project/disney/cbox_specular_10.xml", "project/disney_cbox_specular_10.png"),  # specularTint 0.2
    ("project/volumetric/volumetric_no_scatter.xml", "project/volumetric_no_scatter.png"),
    ("project/volumetric/volumetric_with_bb.xml", "project/volumetric_with_bb.png"),  # sigma_t 1, box 0.3
    # scenes/project/euler/file.png: the C2 scene again, rendered on the Euler cluster
    ("pa4/cbox/cbox_path_mis.xml", "euler_cbox_path_mis.png"),
    # scenes/project/windowed sync filter/: the C2 scene through the windowed sinc
    # filter (rfilter.cpp:123-156); its windowed.png / base_filter.png are plots
    # of the filter shape, not renders
    ("project/windowed/cbox_path_mis.xml", "project/windowed_cbox_path_mis.png"),
    # scenes/project/spotlight/: direct integrator, spotlight over a
    # checkerboard-textured sphere and plane
    ("project/spotlight/sphere-texture.xml", "project/spotlight_sphere_texture.png"),
]


def compare_to_png(img, ref_lin, block=50, scale=1.0):
    """Channel-mean ratios and block-mean relative errors of a linear render
    (clamped to [0, 1] like saveToLDR) against a linearised reference PNG."""
    img = np.clip(np.asarray(img, np.float64) * scale, 0.0, 1.0)
    assert img.shape == ref_lin.shape, (img.shape, ref_lin.shape)
    H, W = img.shape[0] // block, img.shape[1] // block

    def bm(a):
        return a[:H * block, :W * block].reshape(H, block, W, block, 3).mean(axis=(1, 3))

    rel = np.abs(bm(img) - bm(ref_lin)) / (bm(ref_lin) + 1e-2)
    ratio = img.reshape(-1, 3).mean(0) / np.maximum(ref_lin.reshape(-1, 3).mean(0), 1e-12)
    return {"mean_ratio": ratio, "rel_median": float(np.median(rel)), "rel_p95": float(np.percentile(rel, 95)),
            "rel_max": float(rel.max())}


def prim_hit(scene, rays, prim):
    """Ray i against the one primitive prim[i] (global ids, as trace() reports them) in numpy
    fp32: (hit, t, u, v).  The operation order is tri_hit / sphere_hit of scan.h with dot() and
    cross() of device_math.h -- Mesh::rayIntersect (mesh.cpp:83-120) and Sphere::rayIntersect
    (sphere.cpp:43-76), every +, -, *, / and sqrt rounded once to fp32, nothing fused -- and the
    walk's adaptive epsilon (mint == 1e-4f grows with the origin's largest coordinate).  An
    independent third statement of the test: the tie rule of test_gpu_parity._compare_hits and
    the oracle's own t, u, v are checked against it (test_bvh_shapes.py)."""
    f32 = np.float32
    rays = np.ascontiguousarray(rays, f32)
    prim = np.asarray(prim, np.int64)
    n = rays.shape[0]
    o, d = rays[:, 0:3], rays[:, 4:7]
    mint, maxt = rays[:, 3].copy(), rays[:, 7]
    eps = mint == f32(1e-4)
    mint[eps] = np.maximum(mint[eps], mint[eps] * np.abs(o[eps]).max(axis=1))

    def dot(a, b):
        return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]

    def cross(a, b):
        return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                         a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)

    shapes = scene.shapes()
    counts = [1 if sh.type == nori_amd._abi.SHAPE_SPHERE else sh.tri_count for sh in shapes]
    first = np.concatenate([[0], np.cumsum(counts)])
    shape = np.searchsorted(first, prim, side="right") - 1
    sphere = np.array([sh.type == nori_amd._abi.SHAPE_SPHERE for sh in shapes])[shape]
    hit, t = np.zeros(n, bool), np.full(n, np.inf, f32)
    u, v = np.zeros(n, f32), np.zeros(n, f32)
    with np.errstate(all="ignore"):
        m = np.flatnonzero(~sphere)
        if m.size:
            tri = np.array([sh.tri_offset for sh in shapes], np.int64)[shape[m]] + (prim[m] - first[shape[m]])
            p = scene.positions()[scene.indices()[tri]]
            p0, e1, e2 = p[:, 0], p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
            pvec = cross(d[m], e2)
            det = dot(e1, pvec)
            inv = f32(1) / det
            tvec = o[m] - p0
            uu = dot(tvec, pvec) * inv
            qvec = cross(tvec, e1)
            vv = dot(d[m], qvec) * inv
            tt = dot(e2, qvec) * inv
            ok = (~((det > f32(-1e-8)) & (det < f32(1e-8))) & ~((uu < 0) | (uu > 1)) & ~((vv < 0) | (uu + vv > 1))
                  & (tt >= mint[m]) & (tt <= maxt[m]))
            hit[m], t[m], u[m], v[m] = ok, tt, uu, vv
        m = np.flatnonzero(sphere)
        if m.size:
            cen = np.array([list(sh.center) for sh in shapes], f32)[shape[m]]
            rad = np.array([sh.radius for sh in shapes], f32)[shape[m]]
            oc = o[m] - cen
            A = dot(d[m], d[m])
            B = f32(2) * dot(oc, d[m])
            Cc = dot(oc, oc) - rad * rad
            disc = B * B - f32(4) * A * Cc
            delta = np.sqrt(disc)
            t1, t2 = (-B - delta) / (f32(2) * A), (-B + delta) / (f32(2) * A)
            in1 = (mint[m] <= t1) & (t1 <= maxt[m])
            in2 = (mint[m] <= t2) & (t2 <= maxt[m])
            hit[m] = (disc > 0) & (in1 | in2)
            t[m] = np.where(in1, t1, t2)
    t[~hit] = np.inf
    return hit, t, u, v


# Image parity against the oracle on identical WAVE streams (tests/test_gpu_*.py).
# BASELINE.json's bar is per-pixel L2 < 1e-3; the tests assert what the code
# achieves.  Transcendentals differ by a few ulp between the ROCm device
# library and glibc, which can flip a rare branch: one flipped sample moves one
# pixel, so up to 0.01 % of the pixels (at least one) are left out of the
# trimmed L2; the film sums arrive in a different order on the two sides.
L2_TOL = 1e-7           # whole-image L2 (one flipped sample of an 80x60 frame stays under it)
L2_TRIMMED_TOL = 1e-9   # L2 without the worst 0.01 % of the pixels
# pixels whose three channels agree to 1e-3 relative (1e-5 absolute): a few-ulp
# direction difference grows along a long glass-sphere path (chaotic), so
# paths that stay inside the sphere for a hundred bounces may end a little
# apart (measured 99.4 % of the pixels within 1e-4 on 64x48 cbox path_mis)
PIXEL_MATCH = 0.99


def image_parity(gpu, cpu):
    """L2, trimmed L2 and matching-pixel fraction of two (H, W, 3) images."""
    d = np.mean((np.asarray(gpu, np.float64) - np.asarray(cpu, np.float64)) ** 2, axis=-1).ravel()
    k = max(1, int(d.size * 1e-4))
    trimmed = float(np.sort(d)[:-k].mean()) if d.size > k else 0.0
    match = float(np.mean(np.all(np.isclose(gpu, cpu, rtol=1e-3, atol=1e-5), axis=-1)))
    return {"l2": float(d.mean()), "l2_trimmed": trimmed, "pixel_match": match}


def assert_parity(p, l2_tol=L2_TOL):
    assert p["l2"] < l2_tol, p
    assert p["l2_trimmed"] < L2_TRIMMED_TOL, p
    assert p["pixel_match"] >= PIXEL_MATCH, p
