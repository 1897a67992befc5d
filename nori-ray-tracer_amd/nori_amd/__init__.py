"""nori_amd -- MI355X wavefront path tracer behind Nori's scene/plugin API.

Host-side mirror of the reference's render entry points:

* :func:`load_scene` -- ``loadFromXML`` + ``Scene::activate`` (parser.cpp:28,
  scene.cpp:43); the XML `type` names, properties and defaults are Nori's.
* :class:`GpuRenderer` -- one HIP context per device (``nori_gpu_create``);
  ``render`` replaces ``RenderThread::renderScene``'s pass loop
  (render.cpp:173-250) and returns the RGBW image block with its filter
  border (``ImageBlock``, block.h:48).
* :class:`RenderThread` -- ``renderScene(xml)`` writing ``<stem>.exr`` like
  render.cpp:158-261, with ``getProgress``/``stopRendering``.

All compute goes through ``lib/libnori_gpu.so`` (C ABI, include/nori_gpu.h);
there is no CPU fallback: without the library or a GPU the calls raise.
"""
import ctypes as C
import os
import threading
import time

import numpy as np

from . import _abi
from ._abi import NoriError, check, lib  # noqa: F401

__all__ = ["load_scene", "Scene", "GpuRenderer", "RenderThread", "NoriError", "device_count",
           "develop", "write_exr", "write_png", "read_exr", "film_variance", "ldr_bytes", "variance_gray",
           "denoise", "read_image", "block_error", "film_features", "denoise_guided", "film_denoise_guided",
           "scene_surface", "surface_grad", "scene_materials", "bsdf_grad", "bvh_refit", "bvh_rebuild", "film_splat", "film_gather"]


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class Scene:
    """A loaded, flattened scene (owner of the nori_scene handle)."""

    def __init__(self, handle, path):
        self._h = C.c_void_p(handle)
        self.path = path
        self.desc_ptr = lib().nori_scene_get_desc(self._h)
        self.desc = self.desc_ptr.contents
        # kept on the instance: at interpreter exit the module globals may be gone before __del__ runs
        self._free = lib().nori_scene_free

    def __del__(self):
        h, free = getattr(self, "_h", None), getattr(self, "_free", None)
        if h is not None and h.value and free is not None:
            free(h)
            self._h = None

    # convenience views
    @property
    def width(self):
        return self.desc.camera.width

    @property
    def height(self):
        return self.desc.camera.height

    @property
    def spp(self):
        return self.desc.sample_count

    @property
    def border(self):
        return lib().nori_film_border(self.desc_ptr)

    @property
    def integrator(self):
        return _abi.INTEGRATOR_NAMES[self.desc.integrator]

    def film_shape(self):
        b = self.border
        return (self.height + 2 * b, self.width + 2 * b, 4)

    def positions(self):
        n = self.desc.num_vertices
        return np.ctypeslib.as_array(self.desc.positions, shape=(n, 3)).copy()

    def normals(self):
        """Per-vertex normals (num_vertices, 3); zeros for the vertices of meshes without normals."""
        n = self.desc.num_vertices
        if not self.desc.normals:
            return np.zeros((n, 3), np.float32)
        return np.ctypeslib.as_array(self.desc.normals, shape=(n, 3)).copy()

    def uvs(self):
        """Per-vertex texture coordinates (num_vertices, 2); zeros where a mesh has none."""
        n = self.desc.num_vertices
        if not self.desc.uvs:
            return np.zeros((n, 2), np.float32)
        return np.ctypeslib.as_array(self.desc.uvs, shape=(n, 2)).copy()

    def indices(self):
        n = self.desc.num_triangles
        return np.ctypeslib.as_array(self.desc.indices, shape=(n, 3)).copy()

    def shapes(self):
        return [self.desc.shapes[i] for i in range(self.desc.num_shapes)]

    def bsdfs(self):
        return [self.desc.bsdfs[i] for i in range(self.desc.num_bsdfs)]

    def emitters(self):
        return [self.desc.emitters[i] for i in range(self.desc.num_emitters)]

    def filter_table(self):
        t = np.zeros(_abi.FILTER_RESOLUTION + 1, np.float32)
        check(lib().nori_filter_table(self.desc_ptr, _fptr(t)))
        return t

    def num_blocks(self):
        bs = _abi.BLOCK_SIZE
        return ((self.width + bs - 1) // bs) * ((self.height + bs - 1) // bs)


def load_scene(path, width=0, height=0, spp=0):
    """Parse a Nori XML scene; width/height/spp > 0 override the XML values."""
    h = C.c_void_p()
    check(lib().nori_scene_load_xml(os.fsencode(path), int(width), int(height), int(spp), C.byref(h)))
    return Scene(h.value, path)


def device_count():
    n = C.c_int(0)
    check(lib().nori_gpu_device_count(C.byref(n)))
    return n.value


def develop(scene, rgbw):
    """ImageBlock::toBitmap (block.cpp:76-82): RGB / W without the border."""
    rgbw = np.ascontiguousarray(rgbw, dtype=np.float32)
    if rgbw.shape != scene.film_shape():
        raise ValueError(f"film shape {rgbw.shape} != {scene.film_shape()}")
    out = np.zeros((scene.height, scene.width, 3), np.float32)
    check(lib().nori_film_develop(scene.desc_ptr, _fptr(rgbw), _fptr(out)))
    return out


def write_exr(path, rgb):
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    check(lib().nori_write_exr(os.fsencode(path), _fptr(rgb), rgb.shape[1], rgb.shape[0]))


def write_png(path, rgb):
    """Bitmap::saveToLDR (bitmap.cpp:109-139): sRGB curve, 8-bit RGB PNG."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    check(lib().nori_write_png(os.fsencode(path), _fptr(rgb), rgb.shape[1], rgb.shape[0]))


def film_variance(scene, stats):
    """Variance of each pixel's mean (H, W, 3) from the (H, W, 8) sample
    statistics GpuRenderer.render(variance=...) accumulates (nori_film_variance)."""
    stats = np.ascontiguousarray(stats, dtype=np.float32)
    if stats.shape != (scene.height, scene.width, 8):
        raise ValueError(f"statistics shape {stats.shape} != {(scene.height, scene.width, 8)}")
    out = np.zeros((scene.height, scene.width, 3), np.float32)
    check(lib().nori_film_variance(scene.desc_ptr, _fptr(stats), _fptr(out)))
    return out


def film_splat(scene, pos, val, ordered=False, out=None, variance=None):
    """Caller-supplied samples filtered into the film on the host (nori_film_splat, where the
    operation is stated): pos (n, 2) sample positions in pixel units, val (n, 3) radiance.
    ordered: the layout of camera_rays() / sample_uniforms() -- sample i belongs to pixel
    i mod (H W) and must lie in its closed square.  Returns (film, (splatted, dropped)): the RGBW
    film (H+2b, W+2b, 4), added into `out` when given.  `variance`: an (H, W, 8) float32 array the
    owner pixels' sample statistics are added into (see film_variance).
    GpuRenderer.film_splat and film_splat_passes are the device versions."""
    pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 2)
    val = np.ascontiguousarray(val, dtype=np.float32).reshape(-1, 3)
    if pos.shape[0] != val.shape[0]:
        raise ValueError(f"film_splat: {pos.shape[0]} positions and {val.shape[0]} values")
    if out is None:
        out = np.zeros(scene.film_shape(), np.float32)
    assert out.dtype == np.float32 and out.flags.c_contiguous and out.shape == scene.film_shape()
    if variance is not None:
        assert (isinstance(variance, np.ndarray) and variance.dtype == np.float32 and variance.flags.c_contiguous
                and variance.shape == (scene.height, scene.width, 8))
    counts = (C.c_uint64 * 2)()
    check(lib().nori_film_splat(scene.desc_ptr, pos.shape[0], int(bool(ordered)), C.c_void_p(pos.ctypes.data),
                                C.c_void_p(val.ctypes.data), C.c_void_p(out.ctypes.data),
                                None if variance is None else C.c_void_p(variance.ctypes.data), counts))
    return out, (int(counts[0]), int(counts[1]))


def film_gather(scene, pos, grad, val=None, ordered=False):
    """The film splat's adjoint on the host (nori_film_gather, where the operation is stated):
    with `grad` (H+2b, W+2b, 4) the derivative of some scalar by the film that film_splat(scene,
    pos, val, ordered) returns, the derivative by `val` -- every sample reads the cells of its own
    window with the weights it was splatted with.  Returns (grad_val (n, 3), (kept, dropped)); a
    sample film_splat drops gets a zero row (val=None: no value check).  pos has no derivative.
    GpuRenderer.film_gather and film_gather_passes are the device versions."""
    pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 2)
    grad = np.ascontiguousarray(grad, dtype=np.float32)
    if grad.shape != scene.film_shape():
        raise ValueError(f"film_gather: grad shape {grad.shape} != {scene.film_shape()}")
    if val is not None:
        val = np.ascontiguousarray(val, dtype=np.float32).reshape(-1, 3)
        if pos.shape[0] != val.shape[0]:
            raise ValueError(f"film_gather: {pos.shape[0]} positions and {val.shape[0]} values")
    out = np.zeros((pos.shape[0], 3), np.float32)
    counts = (C.c_uint64 * 2)()
    check(lib().nori_film_gather(scene.desc_ptr, pos.shape[0], int(bool(ordered)), C.c_void_p(pos.ctypes.data),
                                 None if val is None else C.c_void_p(val.ctypes.data), C.c_void_p(grad.ctypes.data),
                                 C.c_void_p(out.ctypes.data), counts))
    return out, (int(counts[0]), int(counts[1]))


def block_error(scene, stats):
    """The adaptive sampler's error E_b of every 32x32 block (one float per frame block, id = by*nbx + bx)
    from (H, W, 8) sample statistics, on the host in double precision (nori_film_block_error, where
    the metric is stated).  GpuRenderer.block_error is the device version."""
    stats = np.ascontiguousarray(stats, dtype=np.float32)
    if stats.shape != (scene.height, scene.width, 8):
        raise ValueError(f"statistics shape {stats.shape} != {(scene.height, scene.width, 8)}")
    out = np.zeros(scene.num_blocks(), np.float32)
    check(lib().nori_film_block_error(scene.desc_ptr, _fptr(stats), _fptr(out)))
    return out


def ldr_bytes(rgb):
    """The 8-bit sRGB values Bitmap::saveToLDR writes (bitmap.cpp:122-139;
    nori_write_png): (uint8) clamp(255 * GammaCorrect(v) + 0.5, 0, 255), float32."""
    v = np.asarray(rgb, np.float32)
    with np.errstate(invalid="ignore"):
        g = np.where(v <= np.float32(0.0031308), np.float32(12.92) * v,
                     np.float32(1.055) * np.power(np.maximum(v, 0).astype(np.float32), np.float32(1.0 / 2.4))
                     - np.float32(0.055)).astype(np.float32)
    return np.clip(np.float32(255) * g + np.float32(0.5), 0, 255).astype(np.uint8)


def variance_gray(var_rgb):
    """The variance image denoiser.py:19-21 reads: the `<stem>_variance.exr`
    taken to an 8-bit PNG by hdrToLdr (saveToLDR), loaded by OpenCV as BGR
    and converted with COLOR_RGB2GRAY -- so the blue byte takes the red
    weight -- then divided by 255.  OpenCV's 8-bit grey conversion is fixed
    point: (4899 c0 + 9617 c1 + 1868 c2 + 2^13) >> 14.  (OpenCV is not in
    this image: this step is a restatement, unpinned.)"""
    return variance_gray_bytes(ldr_bytes(var_rgb))


def variance_gray_bytes(rgb8):
    """variance_gray() of an 8-bit RGB image as stored in a PNG (H, W, 3)."""
    bgr = np.asarray(rgb8).astype(np.int64)[..., ::-1]
    gray = (4899 * bgr[..., 0] + 9617 * bgr[..., 1] + 1868 * bgr[..., 2] + (1 << 13)) >> 14
    return (gray.astype(np.float64) / 255.0).astype(np.float32)


def denoise(img, var, radius=3, patch=3, k=0.02, mode=0, device=0, script_scale=True):
    """NL-means denoiser (denoiser/denoiser.py) on the GPU (nori_denoise).

    img: (H, W, 3) linear image; var: (H, W) per-pixel variance in the
    script's units (variance_gray()).  script_scale: divide the image by 255
    first, as the script does with its EXR input (denoiser.py:16), and return
    the result in the input's scale.  mode 0 = the script's distance (both
    variance terms 2 var(neighbour)), 1 = the textbook form."""
    img = np.ascontiguousarray(img, dtype=np.float32)
    var = np.ascontiguousarray(var, dtype=np.float32)
    if img.ndim != 3 or img.shape[2] != 3 or var.shape != img.shape[:2]:
        raise ValueError(f"image {img.shape} / variance {var.shape}: expected (H, W, 3) and (H, W)")
    src = np.ascontiguousarray(img / np.float32(255)) if script_scale else img
    out = np.empty_like(src)
    check(lib().nori_denoise(device, _fptr(src), _fptr(var), img.shape[1], img.shape[0], radius, patch, k, mode,
                             _fptr(out)))
    return out * np.float32(255) if script_scale else out


def film_features(scene, feats):
    """Per-pixel feature means (H, W, 7) -- albedo, shading normal (not renormalised), depth --
    from the (H, W, 8) sums of GpuRenderer.features (nori_film_features); zeros where no sample fell."""
    feats = np.ascontiguousarray(feats, dtype=np.float32)
    if feats.shape != (scene.height, scene.width, 8):
        raise ValueError(f"feature shape {feats.shape} != {(scene.height, scene.width, 8)}")
    out = np.zeros((scene.height, scene.width, 7), np.float32)
    check(lib().nori_film_features(scene.desc_ptr, _fptr(feats), _fptr(out)))
    return out


HIT_DTYPE = np.dtype([("t", "<f4"), ("prim", "<i4"), ("u", "<f4"), ("v", "<f4")])
SURFACE_DTYPE = np.dtype([("p", "<f4", 3), ("t", "<f4"), ("ng", "<f4", 3), ("prim", "<i4"), ("ns", "<f4", 3),
                          ("shape", "<i4"), ("uv", "<f4", 2), ("bary", "<f4", 2)])


def scene_surface(scene, rays, hits):
    """The hit records of `hits` (structured t, prim, u, v, as trace() returns them) of `rays`
    (n, 8) on the host in fp32 (nori_scene_surface, where the record is stated; no GPU needed):
    a structured array p, t, ng, prim, ns, shape, uv, bary.  GpuRenderer.query is the device version."""
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    if rays.ndim != 2 or rays.shape[1] != 8 or hits.shape != (rays.shape[0],):
        raise ValueError(f"rays {rays.shape} / hits {hits.shape}: expected (n, 8) and (n,)")
    out = np.zeros(rays.shape[0], SURFACE_DTYPE)
    check(lib().nori_scene_surface(scene.desc_ptr, rays.shape[0], _fptr(rays), C.c_void_p(hits.ctypes.data),
                                   C.c_void_p(out.ctypes.data)))
    return out


def _grad_records(grad_surf, n):
    """A record gradient as n contiguous 64-byte rows: a SURFACE_DTYPE array or (n, 16) float32."""
    g = np.asarray(grad_surf)
    g = np.ascontiguousarray(g) if g.dtype == SURFACE_DTYPE else np.ascontiguousarray(g, dtype=np.float32)
    if g.nbytes != 64 * n:
        raise ValueError(f"grad_surf {g.shape} {g.dtype}: expected {n} records of 16 floats")
    return g


def surface_grad(scene, rays, hits, grad_surf, positions=None, normals=None, with_terms=False):
    """The hit record's adjoint in the mesh vertices, on the host (nori_scene_surface_grad, where it
    is stated; no GPU needed): for `grad_surf`, the gradient of some scalar in the records of `hits`
    of `rays` -- a SURFACE_DTYPE array or (n, 16) float32 in the record's layout, of which only p,
    t, ng and ns are read --, that scalar's gradient in the vertex positions and vertex normals,
    two (num_vertices, 3) float32 arrays (sums taken in float64).  positions / normals: the
    geometry to differentiate at, (num_vertices, 3); None: as loaded.  with_terms: also the (n, 18)
    per-hit terms g_p0, g_p1, g_p2, g_n0, g_n1, g_n2.

    The barycentrics are held for p and ns and the ray for t; the hit set is held.  A caller who
    wants the point where the fixed ray meets the moving triangle (p = o + t d) adds d . g_p to
    g_t and passes g_p = 0.  GpuRenderer.surface_grad is the device version."""
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    if rays.ndim != 2 or rays.shape[1] != 8 or hits.shape != (rays.shape[0],):
        raise ValueError(f"rays {rays.shape} / hits {hits.shape}: expected (n, 8) and (n,)")
    n, V = rays.shape[0], scene.desc.num_vertices
    g = _grad_records(grad_surf, n)
    arrs = []
    for a, what in ((positions, "positions"), (normals, "normals")):
        if a is not None:
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.shape != (V, 3):
                raise ValueError(f"{what} {a.shape}: expected {(V, 3)}")
        arrs.append(a)
    gp, gn = np.zeros((V, 3), np.float32), np.zeros((V, 3), np.float32)
    terms = np.zeros((n, 18), np.float32) if with_terms else None
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    check(lib().nori_scene_surface_grad(scene.desc_ptr, ptr(arrs[0]), ptr(arrs[1]), n, ptr(rays), ptr(hits), ptr(g),
                                        ptr(gp), ptr(gn), ptr(terms)))
    return (gp, gn, terms) if with_terms else (gp, gn)


MATERIAL_FLOATS = _abi.MATERIAL_FLOATS


def scene_materials(scene):
    """The scene's material rows as loaded (nori_scene_materials): (num_bsdfs, 16) float32, one row
    per entry of the scene's bsdfs -- words 0-2 the colour (diffuse albedo / checkerboard value1,
    microfacet kd, disney base_color), 3 microfacet alpha, 4-9 disney metallic, specular,
    roughness, sheen, sheen_tint, specular_tint, 10-12 checkerboard value2, 13-15 reserved; words a
    BSDF's type does not use are 0."""
    rows = np.zeros((scene.desc.num_bsdfs, MATERIAL_FLOATS), np.float32)
    check(lib().nori_scene_materials(scene.desc_ptr, C.c_void_p(rows.ctypes.data)))
    return rows


def _shading_inputs(name, surf, wi, wo, grad_out):
    """The host arrays of a bsdf_grad call, checked: records, (n, 3) directions, (n, 8) gradient rows."""
    surf = np.ascontiguousarray(surf, dtype=SURFACE_DTYPE).reshape(-1)
    n = surf.shape[0]
    wi, wo = np.ascontiguousarray(wi, dtype=np.float32), np.ascontiguousarray(wo, dtype=np.float32)
    g = np.ascontiguousarray(grad_out, dtype=np.float32)
    if wi.shape != (n, 3) or wo.shape != (n, 3) or g.shape != (n, 8):
        raise ValueError(f"{name}: wi {wi.shape}, wo {wo.shape}, grad_out {g.shape}: expected {(n, 3)}, {(n, 3)}, {(n, 8)}")
    return surf, wi, wo, g, n


def bsdf_grad(scene, surf, wi, wo, grad_out, materials=None, grad_materials=None, with_terms=False):
    """bsdf_eval's adjoint in the material rows, on the host (nori_scene_bsdf_grad, where it is
    stated; no GPU needed): for `grad_out`, the (n, 8) gradient of some scalar in the rows
    GpuRenderer.bsdf_eval(surf, wi, wo) returns -- columns 0-2 (eval) and 3 (pdf) are read, 4-7
    never --, that scalar's gradient in the material rows, ADDED into grad_materials ((num_bsdfs,
    16) float32; None: a new zero array), sums taken in float64.  materials: the rows to
    differentiate at; None: the scene's own (scene_materials).  with_terms: also the (n, 16)
    per-element rows.  No gradient in surf, wi or wo."""
    surf, wi, wo, g, n = _shading_inputs("bsdf_grad", surf, wi, wo, grad_out)
    nb = scene.desc.num_bsdfs
    if materials is not None:
        materials = np.ascontiguousarray(materials, dtype=np.float32)
        if materials.shape != (nb, MATERIAL_FLOATS):
            raise ValueError(f"materials {materials.shape}: expected {(nb, MATERIAL_FLOATS)}")
    if grad_materials is None:
        grad_materials = np.zeros((nb, MATERIAL_FLOATS), np.float32)
    assert (isinstance(grad_materials, np.ndarray) and grad_materials.dtype == np.float32 and
            grad_materials.flags.c_contiguous and grad_materials.shape == (nb, MATERIAL_FLOATS))
    terms = np.zeros((n, MATERIAL_FLOATS), np.float32) if with_terms else None
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    check(lib().nori_scene_bsdf_grad(scene.desc_ptr, ptr(materials), n, ptr(surf), ptr(wi), ptr(wo), ptr(g),
                                     ptr(grad_materials), ptr(terms)))
    return (grad_materials, terms) if with_terms else grad_materials


def _guided_args(img, var, feat7, radius, patch, k, eps, sigma_albedo, sigma_normal, sigma_depth):
    img = np.ascontiguousarray(img, dtype=np.float32)
    var = np.ascontiguousarray(var, dtype=np.float32)
    feat7 = np.ascontiguousarray(feat7, dtype=np.float32)
    if img.ndim != 3 or img.shape[2] != 3 or var.shape != img.shape[:2] or feat7.shape != img.shape[:2] + (7,):
        raise ValueError(f"image {img.shape} / variance {var.shape} / features {feat7.shape}: "
                         "expected (H, W, 3), (H, W) and (H, W, 7)")
    d = _abi.GuidedDesc(int(radius), int(patch), float(k), float(eps), float(sigma_albedo), float(sigma_normal),
                        float(sigma_depth), 0)
    return img, var, feat7, d


def denoise_guided(img, var, feat7, radius=5, patch=1, k=0.45, eps=1e-10, sigma_albedo=0.1, sigma_normal=0.25,
                   sigma_depth=0.1, device=0):
    """Feature-guided NL-means denoiser on the GPU (nori_denoise_guided; the filter is stated at
    nori_film_denoise_guided in nori_gpu.h).

    img: (H, W, 3) linear radiance; var: (H, W) variance of the pixel mean (film_variance(...)
    summed over its channels); feat7: (H, W, 7) film_features().  The parameter values are
    defaults, not tuned values; a sigma of inf switches its feature term off."""
    img, var, feat7, d = _guided_args(img, var, feat7, radius, patch, k, eps, sigma_albedo, sigma_normal, sigma_depth)
    out = np.empty_like(img)
    check(lib().nori_denoise_guided(int(device), _fptr(img), _fptr(var), _fptr(feat7), img.shape[1], img.shape[0],
                                    C.byref(d), _fptr(out)))
    return out


def film_denoise_guided(img, var, feat7, radius=5, patch=1, k=0.45, eps=1e-10, sigma_albedo=0.1, sigma_normal=0.25,
                        sigma_depth=0.1):
    """denoise_guided() on the host in double precision (nori_film_denoise_guided): the
    filter's statement, which the GPU kernel is tested against."""
    img, var, feat7, d = _guided_args(img, var, feat7, radius, patch, k, eps, sigma_albedo, sigma_normal, sigma_depth)
    out = np.empty_like(img)
    check(lib().nori_film_denoise_guided(_fptr(img), _fptr(var), _fptr(feat7), img.shape[1], img.shape[0],
                                         C.byref(d), _fptr(out)))
    return out


class BvhInfo(C.Structure):
    _fields_ = [("ref_nodes", C.c_uint32), ("device_nodes", C.c_uint32), ("depth", C.c_uint32),
                ("num_prims", C.c_uint32), ("sah_cost", C.c_float), ("pad", C.c_uint32), ("order_hash", C.c_uint64)]


def bvh_info(scene):
    """Host build of the scene's BVH as the GPU context builds it (nori_scene_bvh_info)."""
    info = BvhInfo()
    check(lib().nori_scene_bvh_info(scene.desc_ptr, C.byref(info)))
    return {k: getattr(info, k) for k, _ in BvhInfo._fields_ if k != "pad"}


def bvh_refit(scene, positions=None):
    """The scene's device BVH as GpuRenderer builds it, refitted to `positions` ((num_vertices, 3)
    float32; None: the tree as built) on the host -- nori_scene_bvh_refit, where the refit is stated;
    no GPU needed.  Returns (nodes (n, 32), prims (p, 12), root_box (6,)) as float32: the arrays
    GpuRenderer.bvh_nodes() returns after update_vertices(positions), byte for byte."""
    info = bvh_info(scene)
    nodes = np.zeros((info["device_nodes"], 32), np.float32)
    prims = np.zeros((info["num_prims"], 12), np.float32)
    box = np.zeros(6, np.float32)
    p = None
    if positions is not None:
        p = np.ascontiguousarray(positions, dtype=np.float32)
        if p.shape != (scene.desc.num_vertices, 3):
            raise ValueError(f"positions {p.shape}: expected {(scene.desc.num_vertices, 3)}")
    check(lib().nori_scene_bvh_refit(scene.desc_ptr, None if p is None else _fptr(p), _fptr(nodes), _fptr(prims),
                                     _fptr(box)))
    return nodes, prims, box


def bvh_rebuild(scene, positions=None, leaf_max=0, refit_positions=None):
    """The linear BVH of the scene's primitives at `positions` ((num_vertices, 3) float32; None: the
    scene's own) with leaves of at most `leaf_max` records (1 .. 64; 0: the default, 4), built on
    the host -- nori_scene_bvh_rebuild, where the rebuild is stated; no GPU needed.  With
    `refit_positions` the finished tree is then refitted to them as bvh_refit states.  Returns
    (nodes (n, 32), prims (p, 12), root_box (6,), info dict: device_nodes, depth, num_prims,
    leaf_max): the arrays GpuRenderer.bvh_nodes() returns after update_vertices(positions) and
    rebuild_bvh(leaf_max), byte for byte."""
    nv = scene.desc.num_vertices

    def arg(a, what):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.shape != (nv, 3):
            raise ValueError(f"{what} {a.shape}: expected {(nv, 3)}")
        return a

    p, q = arg(positions, "positions"), arg(refit_positions, "refit_positions")
    pp, qq = (None if a is None else _fptr(a) for a in (p, q))
    info = _abi.BvhRebuildInfo()
    check(lib().nori_scene_bvh_rebuild(scene.desc_ptr, pp, leaf_max, qq, C.byref(info), None, None, None))
    nodes = np.zeros((info.device_nodes, 32), np.float32)
    prims = np.zeros((info.num_prims, 12), np.float32)
    box = np.zeros(6, np.float32)
    check(lib().nori_scene_bvh_rebuild(scene.desc_ptr, pp, leaf_max, qq, C.byref(info), _fptr(nodes), _fptr(prims),
                                       _fptr(box)))
    return nodes, prims, box, {k: getattr(info, k) for k in ("device_nodes", "depth", "num_prims", "leaf_max")}


class ScanInfo(C.Structure):
    _fields_ = [("records", C.c_uint32), ("pairs", C.c_uint32), ("plane_end", C.c_uint32 * 3), ("tris", C.c_uint32)]


def scan_list(scene):
    """The small-scene scan list as the GPU context builds it (nori_scene_scan_list): a dict with
    records (n, 12) float32, plane_c (pairs,), plane_f (pairs, 8), plane_end (3,), tris; records is
    empty for a BVH scene."""
    info = ScanInfo()
    check(lib().nori_scene_scan_list(scene.desc_ptr, C.byref(info), None, None, None))
    rec = np.zeros((info.records, 12), np.float32)
    pc = np.zeros(max(info.pairs, 1), np.float32)
    pf = np.zeros((max(info.pairs, 1), 8), np.float32)
    check(lib().nori_scene_scan_list(scene.desc_ptr, C.byref(info), _fptr(rec), _fptr(pc), _fptr(pf)))
    return {"records": rec, "plane_c": pc[:info.pairs], "plane_f": pf[:info.pairs],
            "plane_end": np.array(list(info.plane_end)), "tris": info.tris}


def scan_fast_max(scene):
    """The bound of the fast body in the scene's specialised scan and shade programs
    (nori_scene_scan_fast): a wave whose rays all have sum(|o|) + sum(|d|) at or below it takes
    that body; 0.0 when the programs are built without one."""
    m = C.c_float()
    check(lib().nori_scene_scan_fast(scene.desc_ptr, C.byref(m)))
    return m.value


def scan_rtc(scene, arch="gfx950"):
    """Compile the scene's scan kernels specialised for its scan list for `arch` (the hipRTC program
    GpuRenderer loads for scan-mode scenes; no device needed): (code object bytes, milliseconds);
    (0, 0.0) for a BVH scene."""
    n, ms = C.c_size_t(), C.c_double()
    check(lib().nori_scene_scan_rtc(scene.desc_ptr, arch.encode(), C.byref(n), C.byref(ms)))
    return n.value, ms.value


def shade_rtc(scene, arch="gfx950"):
    """Compile the scene's own shade kernel for `arch` (the second hipRTC program GpuRenderer loads:
    k_shade for the scene's integrator with the scan list as literals; no device needed): (code
    object bytes, milliseconds); (0, 0.0) for a scene the ahead-of-time kernels serve (BVH
    traversal, the full plugin set, a one-bounce integrator)."""
    n, ms = C.c_size_t(), C.c_double()
    check(lib().nori_scene_shade_rtc(scene.desc_ptr, arch.encode(), C.byref(n), C.byref(ms)))
    return n.value, ms.value


def read_exr(path):
    """R, G, B planes of an OpenEXR file as a (height, width, 3) float32 array (nori_read_exr)."""
    w, h = C.c_int(), C.c_int()
    check(lib().nori_read_exr(os.fsencode(path), C.byref(w), C.byref(h), None))
    out = np.zeros((h.value, w.value, 3), np.float32)
    check(lib().nori_read_exr(os.fsencode(path), C.byref(w), C.byref(h), _fptr(out)))
    return out


def read_image(path):
    """An image texture file decoded like the reference's stbi_load(.., STBI_rgb): (height, width, 3) uint8
    (nori_read_image; baseline JPEG or 8-bit PNG)."""
    w, h = C.c_int(), C.c_int()
    check(lib().nori_read_image(os.fsencode(path), C.byref(w), C.byref(h), None))
    out = np.zeros((h.value, w.value, 3), np.uint8)
    check(lib().nori_read_image(os.fsencode(path), C.byref(w), C.byref(h),
                                out.ctypes.data_as(C.POINTER(C.c_uint8))))
    return out


def _addr(a):
    """The device address of a torch tensor or an int device address (None stays None)."""
    return None if a is None else int(a.data_ptr() if hasattr(a, "data_ptr") else a)


class GpuRenderer:
    """HIP context holding one scene on one device (nori_gpu_create)."""

    def __init__(self, scene, device=0):
        self.scene = scene  # keeps the host arrays alive
        h = C.c_void_p()
        check(lib().nori_gpu_create(scene.desc_ptr, int(device), C.byref(h)))
        self._h = h
        self._destroy = lib().nori_gpu_destroy  # usable in __del__ at interpreter exit
        self.device = device
        self.last_stats = None
        self.geometry_version = 0  # bumped by every successful update_vertices / rebuild_bvh

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def shade_rtc(self):
        """The context's own shade kernel (nori_gpu_shade_rtc_info): {"active": renders launch it in
        place of the ahead-of-time kernel, "cached": its code object came from the cache, "ms": the
        compile or cache-read time paid at creation, "code_bytes"}."""
        a, c, ms, n = C.c_int(), C.c_int(), C.c_double(), C.c_size_t()
        check(lib().nori_gpu_shade_rtc_info(self._h, C.byref(a), C.byref(c), C.byref(ms), C.byref(n)))
        return {"active": bool(a.value), "cached": bool(c.value), "ms": ms.value, "code_bytes": n.value}

    def _call(self, fn, *args):
        """fn(context, *args, stats), checked; the call's statistics become last_stats."""
        st = _abi.Stats()
        check(fn(self._h, *args, C.byref(st)))
        self.last_stats = st.as_dict()

    def _film_arg(self, out, device_ptr):
        """(the film argument, the film to return) of a call that adds into a film: the device film
        at `device_ptr`, else the host film `out` (a new one when None)."""
        if device_ptr is not None:
            return C.c_void_p(int(device_ptr)), None
        if out is None:
            out = np.zeros(self.scene.film_shape(), np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.shape == self.scene.film_shape()
        return out.ctypes.data_as(C.c_void_p), out

    def _variance_arg(self, variance, on_device):
        """The address of a per-pixel statistics argument: an int device address, else an (H, W, 8) array."""
        if variance is None:
            return None
        if on_device:
            return int(variance)
        assert (isinstance(variance, np.ndarray) and variance.dtype == np.float32 and variance.flags.c_contiguous
                and variance.shape == (self.scene.height, self.scene.width, 8))
        return variance.ctypes.data

    def render(self, passes=None, pass_begin=0, blocks=None, seed=0, out=None, path_pool=0,
               device_ptr=None, timing=False, variance=None):
        """Render passes [pass_begin, pass_begin+passes) of `blocks` (all if None).

        Returns the RGBW film (H+2b, W+2b, 4) as float32, accumulated into
        `out` when given.  With `device_ptr` (an int device address, e.g. a
        torch tensor's data_ptr()) the film is accumulated on the GPU instead.
        `variance`: an (H, W, 8) float32 array (host mode) or an int device
        address (device mode) that the per-pixel sample statistics are added
        into (see film_variance).
        """
        rd, ids = self._desc(passes, pass_begin, blocks, seed, path_pool, timing)
        rd.variance_out = self._variance_arg(variance, device_ptr is not None)
        rd.output_on_device = int(device_ptr is not None)
        film, out = self._film_arg(out, device_ptr)
        self._call(lib().nori_gpu_render, C.byref(rd), film)
        return out

    def _desc(self, passes, pass_begin, blocks, seed, path_pool, timing):
        rd = _abi.RenderDesc()
        rd.pass_begin = int(pass_begin)
        rd.pass_count = int(self.scene.spp if passes is None else passes)
        ids = None
        if blocks is not None:
            ids = np.ascontiguousarray(np.asarray(blocks, dtype=np.uint32))
            rd.num_blocks = ids.size
            rd.block_ids = ids.ctypes.data_as(C.POINTER(C.c_uint32))
        rd.seed = int(seed)
        rd.path_pool = int(path_pool)
        rd.timing = int(bool(timing))
        return rd, ids

    def block_error(self, stats):
        """block_error() of the scene on the GPU (nori_gpu_block_error): `stats` is an (H, W, 8)
        float32 array, or an int device address of such a buffer (e.g. a torch tensor's data_ptr())."""
        out = np.zeros(self.scene.num_blocks(), np.float32)
        if isinstance(stats, np.ndarray):
            stats = np.ascontiguousarray(stats, dtype=np.float32)
            if stats.shape != (self.scene.height, self.scene.width, 8):
                raise ValueError(f"statistics shape {stats.shape} != {(self.scene.height, self.scene.width, 8)}")
            check(lib().nori_gpu_block_error(self._h, C.c_void_p(stats.ctypes.data), 0, _fptr(out)))
        else:
            check(lib().nori_gpu_block_error(self._h, C.c_void_p(int(stats)), 1, _fptr(out)))
        return out

    def render_adaptive(self, threshold, min_passes=8, max_passes=None, pass_begin=0, blocks=None, seed=0, out=None,
                        device_ptr=None, variance=None, path_pool=0):
        """Adaptive render (nori_gpu_render_adaptive): every block of `blocks` (all if None) gets
        min_passes passes, then rounds that double its count until its error E_b (block_error) is at
        most `threshold` or the count reaches max_passes (None: the scene's spp).

        Returns (film, passes, errors): the RGBW film as render() returns it (None with `device_ptr`),
        the passes each frame block received (0: not selected) and E_b of its final statistics.
        `out`, `device_ptr` and `variance` are render()'s."""
        rd, ids = self._desc(0, pass_begin, blocks, seed, path_pool, False)
        ad = _abi.AdaptiveDesc()
        ad.min_passes = int(min_passes)
        ad.max_passes = int(self.scene.spp if max_passes is None else max_passes)
        ad.threshold = float(threshold)
        passes = np.zeros(self.scene.num_blocks(), np.uint32)
        errors = np.zeros(self.scene.num_blocks(), np.float32)
        ad.passes_out = passes.ctypes.data_as(C.POINTER(C.c_uint32))
        ad.error_out = _fptr(errors)
        rd.variance_out = self._variance_arg(variance, device_ptr is not None)
        rd.output_on_device = int(device_ptr is not None)
        film, out = self._film_arg(out, device_ptr)
        self._call(lib().nori_gpu_render_adaptive, C.byref(rd), C.byref(ad), film)
        return out, passes, errors

    def render_sharded(self, comm, device_ptr, passes=None, pass_begin=0, blocks=None, mode="passes", root=0,
                       seed=0, path_pool=0, timing=False, variance=None):
        """This rank's share of the frame into the device film at `device_ptr`
        (zeroed first), then the RCCL sum of every rank's film into root's
        (root=-1: into every rank's) -- nori_gpu_render_sharded.  A cancel or
        failure on any rank raises NoriError on every rank (no rank hangs in
        the sum).  `variance` must stay None: the library rejects per-pixel
        statistics for sharded renders (they are not summed across ranks)."""
        rd, ids = self._desc(passes, pass_begin, blocks, seed, path_pool, timing)
        if variance is not None:
            rd.variance_out = int(variance)
        self._call(lib().nori_gpu_render_sharded, comm.handle, C.byref(rd), _abi.SHARD_MODES[mode], int(root),
                   C.c_void_p(int(device_ptr)))

    def features(self, passes=None, pass_begin=0, blocks=None, seed=0, out=None, timing=False):
        """First-hit features of the camera samples of passes [pass_begin, pass_begin+passes) of
        `blocks` (all if None), on the render's own primary rays (nori_gpu_render_features).

        Returns the (H, W, 8) float32 sums -- albedo (3), signed shading normal (3), hit distance,
        sample count -- added into `out` when given.  `out` may also be an int device address of
        such a buffer (16-byte aligned, e.g. a torch tensor's data_ptr()): the sums are then
        added on the GPU and None is returned.  film_features() turns the sums into means."""
        rd, ids = self._desc(passes, pass_begin, blocks, seed, 0, timing)
        shape = (self.scene.height, self.scene.width, 8)
        if out is not None and not isinstance(out, np.ndarray):
            rd.output_on_device = 1
            self._call(lib().nori_gpu_render_features, C.byref(rd), C.c_void_p(int(out)))
            return None
        if out is None:
            out = np.zeros(shape, np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.shape == shape
        self._call(lib().nori_gpu_render_features, C.byref(rd), out.ctypes.data_as(C.c_void_p))
        return out

    def trace(self, rays, any_hit=False):
        """Scene::rayIntersect on a batch: rays (n, 8) = o.xyz, mint, d.xyz, maxt."""
        rays = np.ascontiguousarray(rays, dtype=np.float32)
        n = rays.shape[0]
        hits = (_abi.Hit * n)()
        check(lib().nori_gpu_trace(self._h, _fptr(rays), n, int(bool(any_hit)), hits))
        a = np.frombuffer(hits, dtype=np.dtype([("t", "<f4"), ("prim", "<i4"), ("u", "<f4"), ("v", "<f4")]))
        return a.copy()

    def query(self, rays, any_hit=False, surface=True, hits_out=None, surf_out=None, n=None):
        """Scene::rayIntersect(ray, its) on a batch, with the whole hit record (nori_gpu_query).

        Host form: `rays` is an (n, 8) float32 array (o.xyz, mint, d.xyz, maxt); returns a dict
        with "hits" (structured array t, prim, u, v -- the result of trace()) and, for a closest-hit
        query with `surface`, "surf" (structured array p, t, ng, prim, ns, shape, uv, bary; the
        record is stated at nori_scene_surface in nori_gpu.h).
        Device form: `rays` is an int device address of n x 8 floats (`n` is required), `hits_out`
        and `surf_out` are int device addresses of n x 16 and n x 64 bytes (either may be None, not
        both; all 16-byte aligned, e.g. torch tensors' data_ptr()); nothing is copied and None is
        returned.  The buffers must be ready before the call (torch.cuda.synchronize())."""
        qd = _abi.QueryDesc(0, int(bool(any_hit)), 0, 0)
        if not isinstance(rays, np.ndarray):
            if n is None:
                raise ValueError("query: a device address needs n=")
            qd.n, qd.on_device = int(n), 1
            self._call(lib().nori_gpu_query, C.byref(qd), C.c_void_p(int(rays)),
                       None if hits_out is None else C.c_void_p(int(hits_out)),
                       None if surf_out is None else C.c_void_p(int(surf_out)))
            return None
        rays = np.ascontiguousarray(rays, dtype=np.float32)
        if rays.ndim != 2 or rays.shape[1] != 8:
            raise ValueError(f"rays {rays.shape}: expected (n, 8)")
        qd.n = rays.shape[0]
        hits = np.zeros(qd.n, HIT_DTYPE)
        surf = np.zeros(qd.n, SURFACE_DTYPE) if surface and not any_hit else None
        self._call(lib().nori_gpu_query, C.byref(qd), C.c_void_p(rays.ctypes.data), C.c_void_p(hits.ctypes.data),
                   None if surf is None else C.c_void_p(surf.ctypes.data))
        return {"hits": hits} if surf is None else {"hits": hits, "surf": surf}

    def surface_grad(self, rays, hits, grad_surf, grad_positions=None, grad_normals=None, n=None):
        """The hit record's adjoint in the mesh vertices (nori_gpu_surface_grad; stated at
        nori_scene_surface_grad in nori_gpu.h), for the vertices the context holds now: with
        `grad_surf` the gradient of some scalar in the records query() gave for `rays` / `hits`
        (the record's own layout; only p, t, ng and ns are read), that scalar's gradient in the
        vertex positions and normals is ADDED into grad_positions / grad_normals.

        Host form: rays (n, 8), hits (structured t, prim, u, v), grad_surf (a SURFACE_DTYPE array
        or (n, 16) float32); returns (grad_positions, grad_normals), two (num_vertices, 3) float32
        arrays -- the ones given, or new zero ones.
        Device form: torch tensors or int device addresses (then with n=) for rays, hits and
        grad_surf (16-byte aligned) and for grad_positions (required) and grad_normals (None: the
        normal terms are skipped), num_vertices x 3 floats each; everything is used in place and
        None is returned.  The buffers must be ready before the call.

        The barycentrics are held for p and ns, the ray for t, the hit set throughout; a caller
        who wants the point where the fixed ray meets the moving triangle (p = o + t d) adds
        d . g_p to g_t and passes g_p = 0.  Sums of several terms are formed in no fixed order.
        last_stats: ms_total, ms_shade (the kernel)."""
        gd = _abi.SurfaceGradDesc()
        V = self.scene.desc.num_vertices
        given = (rays, hits, grad_surf)
        host = [isinstance(a, np.ndarray) for a in given]
        if any(host) != all(host):
            raise ValueError("surface_grad: rays, hits and grad_surf must all be numpy arrays or all be device arrays")
        if not all(host):
            if grad_positions is None or isinstance(grad_positions, np.ndarray) or isinstance(grad_normals, np.ndarray):
                raise ValueError("surface_grad: device arrays need a device grad_positions= (and grad_normals=)")
            if n is None:
                if not hasattr(rays, "numel"):
                    raise ValueError("surface_grad: int device addresses need n=")
                n = rays.numel() // 8
            gd.n, gd.on_device = int(n), 1
            self._call(lib().nori_gpu_surface_grad, C.byref(gd), C.c_void_p(_addr(rays)), C.c_void_p(_addr(hits)),
                       C.c_void_p(_addr(grad_surf)), C.c_void_p(_addr(grad_positions)), C.c_void_p(_addr(grad_normals)))
            return None
        rays = np.ascontiguousarray(rays, dtype=np.float32)
        hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        if rays.ndim != 2 or rays.shape[1] != 8 or hits.shape != (rays.shape[0],):
            raise ValueError(f"rays {rays.shape} / hits {hits.shape}: expected (n, 8) and (n,)")
        if n is not None and int(n) != rays.shape[0]:
            raise ValueError(f"surface_grad: {rays.shape[0]} rays, expected {int(n)}")
        g = _grad_records(grad_surf, rays.shape[0])
        outs = []
        for a in (grad_positions, grad_normals):
            if a is None:
                a = np.zeros((V, 3), np.float32)
            assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags.c_contiguous and a.size == 3 * V
            outs.append(a)
        gd.n = rays.shape[0]
        self._call(lib().nori_gpu_surface_grad, C.byref(gd), C.c_void_p(rays.ctypes.data), C.c_void_p(hits.ctypes.data),
                   C.c_void_p(g.ctypes.data), C.c_void_p(outs[0].ctypes.data), C.c_void_p(outs[1].ctypes.data))
        return outs[0], outs[1]

    @property
    def materials_version(self):
        """The number of successful update_materials calls on this context so far."""
        v = C.c_uint64()
        check(lib().nori_gpu_materials(self._h, None, C.byref(v)))
        return int(v.value)

    def materials(self):
        """The material rows the context holds now (nori_gpu_materials): (num_bsdfs, 16) float32 in
        scene_materials' layout."""
        rows = np.zeros((self.scene.desc.num_bsdfs, MATERIAL_FLOATS), np.float32)
        check(lib().nori_gpu_materials(self._h, C.c_void_p(rows.ctypes.data), None))
        return rows

    def update_materials(self, rows):
        """Set every BSDF's parameters from material rows (nori_gpu_update_materials): every later
        render, li, feature pass and shading query of this context sees them, bit-identical to a
        context created from a scene loaded with these values.

        rows: (num_bsdfs, 16) float32 in scene_materials' layout -- a numpy array, a torch tensor
        on the context's device (used in place; work queued on it is waited for first) or an int
        device address.  Words a BSDF's type does not use are ignored.  A non-finite value in a
        word in use, a wrong shape and a photonmapper context raise (NoriError / ValueError) with
        nothing changed.  `self.scene` keeps describing the materials as loaded."""
        md = _abi.MaterialsDesc()
        nb = self.scene.desc.num_bsdfs
        md.num_bsdfs = nb
        keep = rows
        if isinstance(rows, np.ndarray):
            keep = np.ascontiguousarray(rows, dtype=np.float32)
            if keep.shape != (nb, MATERIAL_FLOATS):
                raise ValueError(f"rows {keep.shape}: expected {(nb, MATERIAL_FLOATS)}")
            p = keep.ctypes.data
        elif hasattr(rows, "data_ptr"):
            if tuple(rows.shape) != (nb, MATERIAL_FLOATS) or "float32" not in str(rows.dtype) or not rows.is_contiguous():
                raise ValueError(f"rows: expected a contiguous float32 tensor of shape {(nb, MATERIAL_FLOATS)}")
            if not rows.is_cuda or (rows.device.index or 0) != self.device:
                raise ValueError(f"rows: a tensor on {rows.device}, the context is on device {self.device}")
            import torch  # (the caller's: a tensor was passed)

            torch.cuda.synchronize(self.device)
            p, md.on_device = rows.data_ptr(), 1
        else:
            p, md.on_device = int(rows), 1
        check(lib().nori_gpu_update_materials(self._h, C.byref(md), C.c_void_p(p)))
        del keep

    def bsdf_grad(self, surf, wi, wo, grad_out, grad_materials=None, terms=None, n=None):
        """bsdf_eval's adjoint in the material rows (nori_gpu_bsdf_grad; stated at
        nori_scene_bsdf_grad in nori_gpu.h), for the materials the context holds now: with
        `grad_out` the (n, 8) gradient of some scalar in the rows bsdf_eval(surf, wi, wo) returns
        (columns 0-2 and 3 are read, 4-7 never), that scalar's gradient in the material rows is
        ADDED into grad_materials.

        Host form: numpy arrays; returns grad_materials ((num_bsdfs, 16) float32: the one given, or
        a new zero one), or (grad_materials, terms) with terms=True (the (n, 16) per-element rows).
        Device form: torch tensors or int device addresses (then with n=) for surf, wi, wo and
        grad_out, and for grad_materials (required) and terms (optional; n x 16 floats); everything
        is used in place and None is returned.  The buffers must be ready before the call.

        Up to 64 BSDFs the sums are formed without atomics in a fixed order: the same inputs give
        the same bits on every call, host or device form, whatever NORI_QUERY_CHUNK.  No gradient
        in surf, wi or wo.  last_stats: ms_total, ms_shade (the kernels)."""
        gd = _abi.BsdfGradDesc()
        nb = self.scene.desc.num_bsdfs
        given = (surf, wi, wo, grad_out)
        host = [isinstance(a, np.ndarray) for a in given]
        if any(host) != all(host):
            raise ValueError("bsdf_grad: surf, wi, wo and grad_out must all be numpy arrays or all be device arrays")
        if not all(host):
            if grad_materials is None or isinstance(grad_materials, np.ndarray) or isinstance(terms, (np.ndarray, bool)):
                raise ValueError("bsdf_grad: device arrays need a device grad_materials= (and terms=)")
            if n is None:
                if not hasattr(wi, "numel"):
                    raise ValueError("bsdf_grad: int device addresses need n=")
                n = wi.numel() // 3
            gd.n, gd.on_device = int(n), 1
            self._call(lib().nori_gpu_bsdf_grad, C.byref(gd), C.c_void_p(_addr(surf)), C.c_void_p(_addr(wi)),
                       C.c_void_p(_addr(wo)), C.c_void_p(_addr(grad_out)), C.c_void_p(_addr(grad_materials)),
                       C.c_void_p(_addr(terms)))
            return None
        surf, wi, wo, g, cnt = _shading_inputs("bsdf_grad", surf, wi, wo, grad_out)
        if n is not None and int(n) != cnt:
            raise ValueError(f"bsdf_grad: {cnt} elements, expected {int(n)}")
        if grad_materials is None:
            grad_materials = np.zeros((nb, MATERIAL_FLOATS), np.float32)
        assert (isinstance(grad_materials, np.ndarray) and grad_materials.dtype == np.float32 and
                grad_materials.flags.c_contiguous and grad_materials.shape == (nb, MATERIAL_FLOATS))
        tm = np.zeros((cnt, MATERIAL_FLOATS), np.float32) if terms else None
        gd.n = cnt
        self._call(lib().nori_gpu_bsdf_grad, C.byref(gd), C.c_void_p(surf.ctypes.data), C.c_void_p(wi.ctypes.data),
                   C.c_void_p(wo.ctypes.data), C.c_void_p(g.ctypes.data), C.c_void_p(grad_materials.ctypes.data),
                   None if tm is None else C.c_void_p(tm.ctypes.data))
        return (grad_materials, tm) if terms else grad_materials

    def camera_rays(self, passes=None, pass_begin=0, blocks=None, seed=0, out=None):
        """Camera::sampleRay of the renderer's own samples (nori_gpu_camera_rays): the primary rays
        of passes [pass_begin, pass_begin+passes) of `blocks` (all if None) as (passes, H, W, 8)
        float32 (o.xyz, mint, d.xyz, maxt) -- the rays render() and features() trace for the same
        seed.  Only the selected blocks' pixels are written (into `out` when given).  `out` may be
        an int device address of such a buffer (16-byte aligned): None is returned then."""
        rd, ids = self._desc(passes, pass_begin, blocks, seed, 0, False)
        if rd.pass_count == 0:  # the library's "0 = the scene's sampleCount": the buffer is sized here
            rd.pass_count = max(1, int(self.scene.spp))
        shape = (rd.pass_count, self.scene.height, self.scene.width, 8)
        if out is not None and not isinstance(out, np.ndarray):
            rd.output_on_device = 1
            check(lib().nori_gpu_camera_rays(self._h, C.byref(rd), C.c_void_p(int(out))))
            return None
        if out is None:
            out = np.zeros(shape, np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.shape == shape
        check(lib().nori_gpu_camera_rays(self._h, C.byref(rd), C.c_void_p(out.ctypes.data)))
        return out

    def _shading(self, fn, name, arrays, cols, n, out, emitter=0):
        """One shading query.  arrays: [(argument, dtype or None for records, columns, optional)];
        all numpy (host form, the result is returned) or all device addresses with n= and out=."""
        sd = _abi.ShadingDesc(0, 0, int(emitter), 0)
        given = [a for a, _, _, opt in arrays if not (opt and a is None)]
        host = [isinstance(a, np.ndarray) for a in given]
        if any(host) != all(host):
            raise ValueError(f"{name}: the arrays must all be numpy arrays or all be device addresses")
        if not all(host):
            if n is None or out is None or isinstance(out, np.ndarray):
                raise ValueError(f"{name}: device addresses need n= and a device address out=")
            sd.n, sd.on_device = int(n), 1
            check(fn(self._h, C.byref(sd), *[C.c_void_p(_addr(a)) for a, _, _, _ in arrays], C.c_void_p(_addr(out))))
            return None
        conv = []
        for a, dt, k, opt in arrays:
            if a is None:
                conv.append(None)
                continue
            if dt is None:  # hit records
                a = np.ascontiguousarray(a, dtype=SURFACE_DTYPE).reshape(-1)
            else:
                a = np.ascontiguousarray(a, dtype=dt)
                a = a.reshape(-1) if k == 1 else a
                if k > 1 and (a.ndim != 2 or a.shape[1] != k):
                    raise ValueError(f"{name}: an array of shape {a.shape}, expected (n, {k})")
            conv.append(a)
        sizes = {a.shape[0] for a in conv if a is not None}
        if len(sizes) != 1:
            raise ValueError(f"{name}: the arrays have different lengths {sorted(sizes)}")
        sd.n = sizes.pop()
        if out is None:
            out = np.zeros((sd.n, cols), np.float32)
        assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags.c_contiguous and out.shape == (sd.n, cols)
        ptrs = [None if a is None else C.c_void_p(a.ctypes.data) for a in conv]
        check(fn(self._h, C.byref(sd), *ptrs, C.c_void_p(out.ctypes.data)))
        return out

    def bsdf_eval(self, surf, wi, wo, n=None, out=None):
        """BSDF::eval and BSDF::pdf at hit records (nori_gpu_bsdf_eval, stated in nori_gpu.h).

        surf: the "surf" records of query(); wi (towards where the path came from) and wo: (n, 3)
        world-space directions.  Returns (n, 8) float32: eval rgb (no cosine), pdf, wo_local.z,
        wi_local.z, 0, 0; a miss record gives zeros.  Device form: every argument an int device
        address or a torch tensor on the context's device, with n= and out= (n x 8 floats, 16-byte
        aligned); None is returned and the buffers must be ready before the call."""
        return self._shading(lib().nori_gpu_bsdf_eval, "bsdf_eval",
                             [(surf, None, 0, False), (wi, np.float32, 3, False), (wo, np.float32, 3, False)], 8, n, out)

    def bsdf_sample(self, surf, wi, u, n=None, out=None):
        """BSDF::sample at hit records with the 2D samples u (n, 2) (nori_gpu_bsdf_sample).
        Returns (n, 8) float32: the sampled world direction, BSDF::pdf of the sampled pair, the
        weight rgb, the measure (1 solid angle, 2 discrete); a zero weight gives a zero row.
        Device form as bsdf_eval."""
        return self._shading(lib().nori_gpu_bsdf_sample, "bsdf_sample",
                             [(surf, None, 0, False), (wi, np.float32, 3, False), (u, np.float32, 2, False)], 8, n, out)

    def emitter_sample(self, x, u, ids=None, emitter=0, n=None, out=None):
        """Emitter::sample from the points x (n, 3) with the 2D samples u (n, 2) (nori_gpu_emitter_sample):
        emitter ids[i] (int32), or `emitter` for every element when ids is None.  Returns (n, 12)
        float32: wi, the shadow ray's maxt, radiance * attenuation / pdf rgb (not scaled by the emitter
        count), pdf_em, the sampled point, 0.  The shadow ray is (x, 1e-4, wi, maxt).  Device form as
        bsdf_eval (out: n x 12 floats)."""
        return self._shading(lib().nori_gpu_emitter_sample, "emitter_sample",
                             [(ids, np.int32, 1, True), (x, np.float32, 3, False), (u, np.float32, 2, False)], 12, n, out,
                             emitter=emitter)

    def emitter_eval(self, surf, origin, n=None, out=None):
        """What the emitter of each hit shape radiates towards `origin` (n, 3), and the density with
        which emitter_sample would have produced the hit (nori_gpu_emitter_eval).  Returns (n, 4)
        float32: Emitter::eval rgb, Emitter::pdf; zeros for a shape without an emitter and for a
        miss.  Device form as bsdf_eval (out: n x 4 floats)."""
        return self._shading(lib().nori_gpu_emitter_eval, "emitter_eval",
                             [(surf, None, 0, False), (origin, np.float32, 3, False)], 4, n, out)

    def sample_uniforms(self, first, count, passes=None, pass_begin=0, blocks=None, seed=0, out=None):
        """The renderer's own random numbers (nori_gpu_sample_uniforms): draws [first, first+count)
        of the stream of every sample of passes [pass_begin, pass_begin+passes) of `blocks` (all if
        None) as (passes, H, W, count) float32.  Draws 0-1 are the pixel jitter, 2-3 the aperture
        sample, the integrator's start at 4; a 2D sample is two consecutive draws, x first.  Only the
        selected blocks' pixels are written (into `out` when given).  `out` may be an int device
        address (or torch tensor) of such a buffer: None is returned then."""
        rd, ids = self._desc(passes, pass_begin, blocks, seed, 0, False)
        if rd.pass_count == 0:
            rd.pass_count = max(1, int(self.scene.spp))
        shape = (rd.pass_count, self.scene.height, self.scene.width, int(count))
        if out is not None and not isinstance(out, np.ndarray):
            rd.output_on_device = 1
            check(lib().nori_gpu_sample_uniforms(self._h, C.byref(rd), int(first), int(count),
                                                 C.c_void_p(_addr(out))))
            return None
        if out is None:
            out = np.zeros(shape, np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.shape == shape
        check(lib().nori_gpu_sample_uniforms(self._h, C.byref(rd), int(first), int(count), C.c_void_p(out.ctypes.data)))
        return out

    def li(self, rays, stream_ids=None, seed=0, stream_base=0, first_draw=0, n=None, out=None):
        """Integrator::Li of the context's integrator along the caller's rays (nori_gpu_li, stated in
        nori_gpu.h): ray i draws from the stream wave_seed(seed, stream_ids[i]) -- stream_base + i
        when stream_ids is None -- after `first_draw` draws.  With the rays of camera_rays(passes=k,
        pass_begin=p, seed=s) as rows, seed=s, stream_base=p * W * H and first_draw=4 give the
        radiance of the samples render() takes for those passes.
        Host form: `rays` (n, 8) float32 (o.xyz, mint, d.xyz, maxt), `stream_ids` None or n uint64;
        returns (n, 3) float32 (written into `out` when given).  Device form: int device addresses
        or torch tensors on the context's device with n= and out= (n x 3 floats; rays 16-byte,
        stream_ids 8-byte aligned): used in place, None is returned, and the buffers must be ready
        before the call.  last_stats: samples, invalid_samples, rays_closest, rays_shadow, ms_shade."""
        ld = _abi.LiDesc(0, 0, int(seed), int(stream_base), int(first_draw), 0)
        if not isinstance(rays, np.ndarray):
            if isinstance(stream_ids, np.ndarray) or isinstance(out, np.ndarray):
                raise ValueError("li: the arrays must all be numpy arrays or all be device addresses")
            if n is None or out is None:
                raise ValueError("li: device addresses need n= and a device address out=")
            ld.n, ld.on_device = int(n), 1
            self._call(lib().nori_gpu_li, C.byref(ld), *[C.c_void_p(_addr(a)) for a in (rays, stream_ids, out)])
            return None
        rays = np.ascontiguousarray(rays, dtype=np.float32)
        if rays.ndim != 2 or rays.shape[1] != 8:
            raise ValueError(f"rays {rays.shape}: expected (n, 8)")
        ld.n = rays.shape[0]
        if n is not None and int(n) != ld.n:
            raise ValueError(f"li: {ld.n} rays, expected {int(n)}")
        ids = None
        if stream_ids is not None:
            ids = np.ascontiguousarray(stream_ids, dtype=np.uint64).reshape(-1)
            if ids.shape[0] != ld.n:
                raise ValueError(f"li: {ids.shape[0]} stream ids for {ld.n} rays")
        if out is None:
            out = np.zeros((ld.n, 3), np.float32)
        assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags.c_contiguous and out.shape == (ld.n, 3)
        self._call(lib().nori_gpu_li, C.byref(ld), C.c_void_p(rays.ctypes.data),
                   None if ids is None else C.c_void_p(ids.ctypes.data), C.c_void_p(out.ctypes.data))
        return out

    def _splat_args(self, name, pos, val, n, out, variance):
        """(on_device, n, pos, val, film, variance addresses, the film to return) of a film splat:
        all numpy (host form) or all device addresses / torch tensors with a device film out=."""
        host = [isinstance(a, np.ndarray) for a in (pos, val)]
        if any(host) != all(host):
            raise ValueError(f"{name}: pos and val must both be numpy arrays or both be device addresses")
        if not all(host):
            if out is None or isinstance(out, np.ndarray) or isinstance(variance, np.ndarray):
                raise ValueError(f"{name}: device arrays need a device film out= (and a device variance=)")
            if n is None:
                if not hasattr(val, "numel"):
                    raise ValueError(f"{name}: int device addresses need the sample count")
                n = val.numel() // 3
            return 1, int(n), _addr(pos), _addr(val), _addr(out), _addr(variance), None, ()
        pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 2)
        val = np.ascontiguousarray(val, dtype=np.float32).reshape(-1, 3)
        if pos.shape[0] != val.shape[0]:
            raise ValueError(f"{name}: {pos.shape[0]} positions and {val.shape[0]} values")
        if n is not None and int(n) != pos.shape[0]:
            raise ValueError(f"{name}: {pos.shape[0]} samples, expected {int(n)}")
        assert out is None or isinstance(out, np.ndarray)
        film, out = self._film_arg(out, None)
        var = self._variance_arg(variance, False)
        return 0, pos.shape[0], pos.ctypes.data, val.ctypes.data, film.value, var, out, (pos, val)

    def film_splat(self, pos, val, n=None, out=None, variance=None):
        """Samples anywhere on the image filtered into the film (nori_gpu_film_splat; the operation
        is stated at nori_film_splat in nori_gpu.h): pos (n, 2) positions in pixel units, val (n, 3)
        radiance; the owner pixel of a sample is the floor of its position.  With numpy arrays the
        RGBW film (H+2b, W+2b, 4) is returned, added into `out` when given, and `variance` is an
        (H, W, 8) float32 array for the owner pixels' sample statistics.  With torch tensors or int
        device addresses (then with n=), `out` must be a device film (16-byte aligned, like
        `variance`), everything is used in place and None is returned; the buffers must be ready
        before the call.  last_stats: samples = splatted, invalid_samples = dropped, ms_splat."""
        dev, n, p, v, film, var, ret, keep = self._splat_args("film_splat", pos, val, n, out, variance)
        sd = _abi.SplatDesc(n, dev, 0, var)
        self._call(lib().nori_gpu_film_splat, C.byref(sd), C.c_void_p(p), C.c_void_p(v), C.c_void_p(film))
        return ret

    def film_splat_passes(self, pos, val, passes=None, blocks=None, out=None, variance=None):
        """Samples in the layout of camera_rays() / sample_uniforms() filtered into the film
        (nori_gpu_film_splat_passes): pos (passes, H, W, 2) with the sample of pass k and pixel
        (x, y) inside the closed square [x, x+1] x [y, y+1] -- for the renderer's own samples
        pixel + sample_uniforms(0, 2) in float32 -- and val (passes, H, W, 3).  Only the pixels of
        `blocks` (all if None) are read.  Host and device forms, `out`, `variance` and last_stats
        as film_splat."""
        rd, ids = self._desc(passes, 0, blocks, 0, 0, False)
        # (pass_count 0 is the library's "the scene's sampleCount"; a scene of 0 spp is refused there)
        n = rd.pass_count * self.scene.width * self.scene.height if rd.pass_count else None
        dev, n, p, v, film, var, ret, keep = self._splat_args("film_splat_passes", pos, val, n, out, variance)
        rd.output_on_device = dev
        rd.variance_out = var
        self._call(lib().nori_gpu_film_splat_passes, C.byref(rd), C.c_void_p(p), C.c_void_p(v), C.c_void_p(film))
        return ret

    def _gather_args(self, name, pos, grad, val, n, out):
        """(on_device, n, pos, val, grad, out addresses, the rows to return, keep-alive) of a film
        gather: all numpy (host form) or all device addresses / torch tensors with a device out=."""
        given = [a for a in (pos, grad, val) if a is not None]
        host = [isinstance(a, np.ndarray) for a in given]
        if any(host) != all(host):
            raise ValueError(f"{name}: pos, grad and val must all be numpy arrays or all be device addresses")
        if not all(host):
            if out is None or isinstance(out, np.ndarray):
                raise ValueError(f"{name}: device arrays need a device out=")
            if n is None:
                if not hasattr(pos, "numel"):
                    raise ValueError(f"{name}: int device addresses need the sample count")
                n = pos.numel() // 2
            return 1, int(n), _addr(pos), _addr(val), _addr(grad), _addr(out), None, ()
        pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 2)
        grad = np.ascontiguousarray(grad, dtype=np.float32)
        if grad.shape != self.scene.film_shape():
            raise ValueError(f"{name}: grad shape {grad.shape} != {self.scene.film_shape()}")
        if val is not None:
            val = np.ascontiguousarray(val, dtype=np.float32).reshape(-1, 3)
            if pos.shape[0] != val.shape[0]:
                raise ValueError(f"{name}: {pos.shape[0]} positions and {val.shape[0]} values")
        if n is not None and int(n) != pos.shape[0]:
            raise ValueError(f"{name}: {pos.shape[0]} samples, expected {int(n)}")
        if out is None:
            out = np.zeros((pos.shape[0], 3), np.float32)
        assert (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags.c_contiguous
                and out.size == 3 * pos.shape[0])
        return (0, pos.shape[0], pos.ctypes.data, None if val is None else val.ctypes.data, grad.ctypes.data,
                out.ctypes.data, out, (pos, val, grad))

    def film_gather(self, pos, grad, val=None, n=None, out=None):
        """The adjoint of film_splat (nori_gpu_film_gather; stated at nori_film_gather in nori_gpu.h):
        with `grad` (H+2b, W+2b, 4) the derivative by the film, the derivative by val -- (n, 3), a
        zero row for a sample film_splat drops (val=None: no value check).  With numpy arrays the
        rows are returned (written into `out` when given).  With torch tensors or int device
        addresses (then with n=), `out` must be a device array of n x 3 floats (grad 16-byte
        aligned), everything is used in place and None is returned; the buffers must be ready
        before the call.  last_stats: samples = kept, invalid_samples = zero rows, ms_splat."""
        dev, n, p, v, g, o, ret, keep = self._gather_args("film_gather", pos, grad, val, n, out)
        gd = _abi.GatherDesc(n, dev, 0)
        self._call(lib().nori_gpu_film_gather, C.byref(gd), C.c_void_p(p), C.c_void_p(v), C.c_void_p(g), C.c_void_p(o))
        return ret

    def film_gather_passes(self, pos, grad, val=None, passes=None, blocks=None, out=None):
        """The adjoint of film_splat_passes (nori_gpu_film_gather_passes): pos (passes, H, W, 2), val
        (passes, H, W, 3) or None; returns (passes, H, W, 3).  Only the rows of the pixels of
        `blocks` (all if None) are written: every other entry of `out` stays as it is (zero in a
        new array).  Host and device forms, `out` and last_stats as film_gather."""
        rd, ids = self._desc(passes, 0, blocks, 0, 0, False)
        n = rd.pass_count * self.scene.width * self.scene.height if rd.pass_count else None
        dev, n, p, v, g, o, ret, keep = self._gather_args("film_gather_passes", pos, grad, val, n, out)
        rd.output_on_device = dev
        self._call(lib().nori_gpu_film_gather_passes, C.byref(rd), C.c_void_p(p), C.c_void_p(v), C.c_void_p(g),
                   C.c_void_p(o))
        if ret is not None and out is None:
            ret = ret.reshape(-1, self.scene.height, self.scene.width, 3)
        return ret

    def _vertex_arg(self, a, what):
        """(address, on_device, keep-alive) of a positions / normals argument of update_vertices."""
        n = self.scene.desc.num_vertices
        if isinstance(a, np.ndarray):
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.shape != (n, 3):
                raise ValueError(f"{what} {a.shape}: expected {(n, 3)}")
            return a.ctypes.data, 0, a
        if hasattr(a, "data_ptr"):  # a torch tensor: used in place, no host copy
            if not a.is_cuda or a.device.index != self.device:
                raise ValueError(f"{what}: a tensor on {a.device}, the context is on device {self.device}")
            if tuple(a.shape) != (n, 3) or "float32" not in str(a.dtype) or not a.is_contiguous():
                raise ValueError(f"{what}: expected a contiguous float32 tensor of shape {(n, 3)}")
            return a.data_ptr(), 1, a
        return int(a), 1, None  # an int device address of n x 3 floats

    def update_vertices(self, positions, normals=None):
        """Move the scene's mesh vertices and refit the BVH on the device (nori_gpu_update_vertices):
        every later render, features, trace and query of this context sees the new geometry.

        positions, normals (optional: the vertex normals stay): (num_vertices, 3) float32 numpy
        arrays, or torch tensors on the context's device (used in place: no host copy; work queued
        on them is waited for first), or int device addresses (the caller has made them ready).
        Both must be of the same kind.  Spheres do not move, the topology stays, and `self.scene`
        keeps describing the geometry as loaded.  Scan-mode contexts (create with
        NORI_TRAVERSAL=bvh) and photonmapper contexts raise NoriError (unsupported); non-finite
        values raise NoriError (invalid) with nothing changed.  Returns the stats as a dict: ms,
        ms_device, root_min, root_max, nodes, levels, launches."""
        ud = _abi.UpdateDesc()
        p, dev, keep_p = self._vertex_arg(positions, "positions")
        ud.positions, ud.on_device = p, dev
        keep_n = None
        if normals is not None:
            q, dev_n, keep_n = self._vertex_arg(normals, "normals")
            if dev_n != dev:
                raise ValueError("positions and normals must both be host arrays or both be device buffers")
            ud.normals = q
        ud.num_vertices = self.scene.desc.num_vertices
        if dev and (hasattr(positions, "data_ptr") or hasattr(normals, "data_ptr")):
            import torch  # (the caller's: a tensor was passed)

            torch.cuda.synchronize(self.device)
        st = _abi.UpdateStats()
        check(lib().nori_gpu_update_vertices(self._h, C.byref(ud), C.byref(st)))
        self.geometry_version += 1
        del keep_p, keep_n
        return st.as_dict()

    def rebuild_bvh(self, leaf_max=0):
        """Rebuild the context's BVH on the device for the vertex positions it holds now
        (nori_gpu_rebuild_bvh): a linear BVH with leaves of at most `leaf_max` records (1 .. 64;
        0: the default, 4), byte for byte bvh_rebuild(scene, positions, leaf_max).  Call it after
        update_vertices has moved the geometry far from where the current tree was built (a refit
        keeps that tree's topology); later update_vertices calls refit the rebuilt tree.  Scan-mode
        and photonmapper contexts raise NoriError (unsupported) with nothing changed.  Returns the
        stats as a dict: ms, ms_device, nodes, depth, stack, levels, launches."""
        rd = _abi.RebuildDesc()
        rd.leaf_max = leaf_max
        st = _abi.RebuildStats()
        check(lib().nori_gpu_rebuild_bvh(self._h, C.byref(rd), C.byref(st)))
        self.geometry_version += 1
        return st.as_dict()

    def bvh_nodes(self):
        """The context's BVH as it is on the device (nori_gpu_bvh_read; introspection for tests):
        (nodes (n, 32), prims (p, 12)) float32 -- 4-wide nodes and leaf-order primitive records
        (a scan-mode context holds its scan list in prims)."""
        counts = (C.c_uint32 * 2)()
        check(lib().nori_gpu_bvh_read(self._h, None, None, counts))
        nodes = np.zeros((counts[0], 32), np.float32)
        prims = np.zeros((counts[1], 12), np.float32)
        check(lib().nori_gpu_bvh_read(self._h, _fptr(nodes), _fptr(prims), counts))
        return nodes, prims

    def cancel(self):
        check(lib().nori_gpu_cancel(self._h))

    def progress(self):
        return lib().nori_gpu_progress(self._h)


class RenderThread:
    """Mirror of nori::RenderThread (render.h:29-52) over the GPU path."""

    def __init__(self, device=0):
        self.device = device
        self._thread = None
        self._renderer = None
        self._status = 0  # 0 idle, 1 rendering, 2 stop requested, 3 done
        self.error = None
        self.image = None
        self.variance = None

    def renderScene(self, filename, width=0, height=0, spp=0):
        """Writes <stem>.exr and <stem>_variance.exr (render.cpp:158-169, 256-276;
        the variance image is the variance of each pixel's mean, deviation D5)."""
        scene = load_scene(filename, width, height, spp)
        stem = os.path.splitext(filename)[0]

        def run():
            try:
                self._renderer = GpuRenderer(scene, self.device)
                t0 = time.time()
                print("Rendering .. ", end="", flush=True)
                stats = np.zeros((scene.height, scene.width, 8), np.float32)
                film = self._renderer.render(variance=stats)
                print(f"done. (took {1e3 * (time.time() - t0):.1f}ms)")
                self.image = develop(scene, film)
                write_exr(stem + ".exr", self.image)
                self.variance = film_variance(scene, stats)
                write_exr(stem + "_variance.exr", self.variance)
            except NoriError as e:
                self.error = e
            finally:
                if self._renderer is not None:
                    self._renderer.close()
                self._status = 3

        self._status = 1
        self._thread = threading.Thread(target=run)
        self._thread.start()

    def isBusy(self):
        if self._status == 3:
            self._thread.join()
            self._status = 0
        return self._status != 0

    def isRenderingDone(self):
        return self._status == 3

    def getProgress(self):
        r = self._renderer
        return r.progress() if (r is not None and self._status in (1, 2)) else 1.0

    def stopRendering(self):
        if self._status in (1, 2) and self._renderer is not None:
            self._status = 2
            self._renderer.cancel()
            self._thread.join()
            self._status = 0
