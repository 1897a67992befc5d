"""Shared by the material tests (tests/test_bsdf_grad.py, tests/test_gpu_bsdf_grad.py,
tests/test_gpu_update_materials.py, tests/test_gpu_material_autograd.py): a scene of spheres
with one BSDF of every kind, synthetic hit records, material rows against float64 descriptors,
and scene XML files rewritten to new parameter values.  No assertions here."""
import os
import xml.etree.ElementTree as ET

import numpy as np

import nori_amd
from conftest import scene_path

A = nori_amd._abi
f32 = np.float32
MF = 16
# the words in use, by kind (include/nori_gpu.h)
WORDS = {"diffuse": [0, 1, 2], "checker": [0, 1, 2, 10, 11, 12], "microfacet": [0, 1, 2, 3],
         "disney": [0, 1, 2, 4, 5, 6, 7, 8, 9], "mirror": [], "dielectric": [], "image": []}
ZOO = ["diffuse", "checker", "microfacet", "disney", "mirror", "dielectric", "image"]  # BSDF b of the zoo = shape b
_HEAD = """<scene>
  <integrator type="path_mis"/>
  <camera type="perspective">
    <float name="fov" value="40"/>
    <transform name="toWorld"><lookat target="0,0,0" origin="0,2,12" up="0,1,0"/></transform>
    <integer name="width" value="32"/><integer name="height" value="32"/>
  </camera>
  <sampler type="independent"><integer name="sampleCount" value="2"/></sampler>
"""
_BSDF = {
    "diffuse": '<bsdf type="diffuse"><color name="albedo" value="0.5,0.3,0.7"/></bsdf>',
    "checker": '<bsdf type="diffuse"><texture type="checkerboard_color" name="albedo"><point name="delta" value="0.25,-0.5"/>'
               '<vector name="scale" value="0.1,0.37"/><color name="value1" value="0.9,0.2,0.4"/>'
               '<color name="value2" value="0.1,0.6,0.3"/></texture></bsdf>',
    "microfacet": '<bsdf type="microfacet"><color name="kd" value="0.2,0.1,0.3"/><float name="alpha" value="0.3"/></bsdf>',
    "disney": '<bsdf type="disney"><color name="baseColor" value="0.8,0.4,0.2"/><float name="metallic" value="0.5"/>'
              '<float name="specular" value="0.5"/><float name="specularTint" value="0.6"/><float name="roughness" value="0.5"/>'
              '<float name="sheen" value="0.7"/><float name="sheenTint" value="0.3"/></bsdf>',
    "mirror": '<bsdf type="mirror"/>',
    "dielectric": '<bsdf type="dielectric"/>',
}


def _sphere(x, bsdf, radius=0.5, emitter=""):
    return (f'  <mesh type="sphere"><point name="center" value="{x},0,0"/><float name="radius" value="{radius}"/>'
            f'{bsdf}{emitter}</mesh>\n')


def zoo_xml(directory):
    """A scene file with seven spheres, one BSDF of each kind in ZOO's order, and a light."""
    tex = scene_path("project", "textured", "textures", "texture.jpg")
    image = f'<bsdf type="diffuse"><texture type="ImageTexture" name="albedo"><string name="fileName" value="{tex}"/>' \
            '<string name="wrap" value="repeat"/></texture></bsdf>'
    body = "".join(_sphere(-4.5 + 1.5 * k, image if kind == "image" else _BSDF[kind]) for k, kind in enumerate(ZOO))
    light = ('  <mesh type="sphere"><point name="center" value="0,6,3"/><float name="radius" value="0.5"/>'
             '<bsdf type="diffuse"/><emitter type="area"><color name="radiance" value="40,40,40"/></emitter></mesh>\n')
    path = os.path.join(directory, "zoo.xml")
    with open(path, "w") as f:
        f.write(_HEAD + body + light + "</scene>\n")
    return path


def many_xml(directory, count=70):
    """A scene file of `count` diffuse spheres, each with its own albedo, and a light."""
    rng = np.random.default_rng(3)
    body = ""
    for k in range(count):
        a = rng.uniform(0.1, 0.9, 3)
        bsdf = f'<bsdf type="diffuse"><color name="albedo" value="{a[0]:.4f},{a[1]:.4f},{a[2]:.4f}"/></bsdf>'
        body += (f'  <mesh type="sphere"><point name="center" value="{-4.5 + (k % 10)},{-3 + k // 10},0"/>'
                 f'<float name="radius" value="0.4"/>{bsdf}</mesh>\n')
    light = ('  <mesh type="sphere"><point name="center" value="0,8,3"/><float name="radius" value="0.5"/>'
             '<bsdf type="diffuse"/><emitter type="area"><color name="radiance" value="40,40,40"/></emitter></mesh>\n')
    path = os.path.join(directory, "many.xml")
    with open(path, "w") as f:
        f.write(_HEAD + body + light + "</scene>\n")
    return path


def kind_of(desc):
    """The kind (a key of WORDS) of a nori_bsdf_desc."""
    if desc.type == A.BSDF_DIFFUSE:
        return {A.TEXTURE_CONSTANT: "diffuse", A.TEXTURE_CHECKERBOARD: "checker"}.get(desc.albedo_texture, "image")
    return {A.BSDF_MICROFACET: "microfacet", A.BSDF_DISNEY: "disney", A.BSDF_MIRROR: "mirror"}.get(desc.type, "dielectric")


def kinds(scene):
    return [kind_of(scene.desc.bsdfs[b]) for b in range(scene.desc.num_bsdfs)]


def shape_bsdfs(scene):
    return np.array([scene.desc.shapes[s].bsdf for s in range(scene.desc.num_shapes)], np.int64)


def desc_with_row(desc, row):
    """A copy of a nori_bsdf_desc with the row's words in use set (the float64 forward's input)."""
    d = A.BsdfDesc()
    import ctypes as C
    C.memmove(C.byref(d), C.byref(desc), C.sizeof(d))
    k = kind_of(desc)
    row = [float(f32(x)) for x in row]
    if k in ("diffuse", "checker"):
        d.albedo[:] = row[0:3]
    if k == "checker":
        d.tex_value2[:] = row[10:13]
    if k == "microfacet":
        d.kd[:] = row[0:3]
        d.alpha = row[3]
    if k == "disney":
        d.base_color[:] = row[0:3]
        d.metallic, d.specular, d.roughness, d.sheen, d.sheen_tint, d.specular_tint = row[4:10]
    return d


def records(n, shape, ns=None, uv=None):
    """n hit records of which only ns, shape and uv matter (the rest is zero)."""
    r = np.zeros(n, nori_amd.SURFACE_DTYPE)
    r["ns"] = (0, 0, 1) if ns is None else ns
    r["shape"] = shape
    r["prim"] = np.where(np.asarray(shape) < 0, -1, 0)
    if uv is not None:
        r["uv"] = uv
    return r


def directions(n, seed, zmin=0.05, zmax=0.98):
    """n unit vectors of the upper hemisphere with z in [zmin, zmax] (float32)."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(zmin, zmax, n)
    ph = rng.uniform(0, 2 * np.pi, n)
    s = np.sqrt(1 - z * z)
    return np.stack([s * np.cos(ph), s * np.sin(ph), z], 1).astype(f32)


def random_frames(n, seed):
    """n unit normals all over the sphere (float32, normalised in float32)."""
    v = np.random.default_rng(seed).standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    return v.astype(f32)


def world_dirs(ns, local):
    """Local directions taken to the world with the float64 frame of ns (to_local of the result is
    the local direction up to fp32 rounding)."""
    import bsdf_ref64
    fr = bsdf_ref64.frame32(ns).astype(np.float64).reshape(-1, 3, 3)
    loc = np.asarray(local, np.float64)
    w = fr[:, 0] * loc[:, :1] + fr[:, 1] * loc[:, 1:2] + fr[:, 2] * loc[:, 2:3]
    return w.astype(f32)


# ---------------------------------------------------------------- XML with new values
_NAMES = {"microfacet": {"kd": (0, 3), "alpha": (3, 4)},
          "disney": {"baseColor": (0, 3), "metallic": (4, 5), "specular": (5, 6), "roughness": (6, 7), "sheen": (7, 8),
                     "sheenTint": (8, 9), "specularTint": (9, 10)},
          "diffuse": {"albedo": (0, 3)}}


def _fmt(vals):
    return ",".join(repr(float(f32(v))) for v in vals)


def write_with_rows(src_xml, rows, dst_xml):
    """A copy of the scene file whose shapes' BSDFs (one per shape, in document order) carry the rows'
    values, every float written so that it parses back to the same float32.  Mesh and texture
    file names are made absolute.  Checkerboards: value1 / value2."""
    tree = ET.parse(src_xml)
    root = tree.getroot()
    base = os.path.dirname(os.path.abspath(src_xml))
    for s in root.iter("string"):
        if s.get("name") in ("filename", "fileName") and not os.path.isabs(s.get("value")):
            s.set("value", os.path.join(base, s.get("value")))
    meshes = list(root.iter("mesh"))  # one entry of bsdfs[] per shape, in document order
    assert len(meshes) == len(rows), (len(meshes), len(rows))
    for m, row in zip(meshes, rows):
        b = m.find("bsdf")
        if b is None:  # the loader's default: a diffuse BSDF
            b = ET.SubElement(m, "bsdf", {"type": "diffuse"})
        kind = b.get("type")
        tex = b.find("texture")
        if kind == "diffuse" and tex is not None:
            if tex.get("type") == "checkerboard_color":
                for c in tex.findall("color"):
                    c.set("value", _fmt(row[0:3] if c.get("name") == "value1" else row[10:13]))
            continue
        for name, (a, e) in _NAMES.get(kind, {}).items():
            el = next((c for c in b if c.get("name") == name), None)
            if el is None:
                el = ET.SubElement(b, "color" if e - a == 3 else "float", {"name": name})
            el.set("value", _fmt(row[a:e]))
    tree.write(dst_xml)
    return dst_xml
