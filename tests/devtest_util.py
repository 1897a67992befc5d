"""ctypes loader of libnori_devtest.so (nori-ray-tracer_amd/csrc/devtest.hip):
the device routines of device_math.h and shading.h, the pieces of the tail
finisher (coop_scan.h, tail_index.h) and the primitive tests of scan.h behind
C entry points, with thin numpy wrappers.  No assertions here; a HIP error
raises RuntimeError."""
import ctypes as C
import os

import numpy as np

import nori_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "nori-ray-tracer_amd", "lib", "libnori_devtest.so")

# ops of nori_devtest_math (devtest.hip)
SQRT_RN, RCP_RN, RCP_FULL, FSQRT_FAST, FSQRT_IEEE = 0, 1, 2, 3, 4
NORMALIZE_FAST, NORMALIZE_IEEE, FRAME_FAST, FRAME_IEEE = 5, 6, 7, 8
FRESNEL_FAST, FRESNEL_IEEE, TAN_THETA = 9, 10, 11

# forms of nori_devtest_prim_hit (devtest.hip)
TRI, TRI_NB, TRI_PLANE0, TRI_PLANE1, TRI_PLANE2 = 0, 1, 2, 3, 4
SPHERE, SPHERE_NB, SPHERE_FAST, SPHERE_FAST_NOCHECK, BOX = 5, 6, 7, 8, 9

# flags word of a glass lane
GLASS_CHORD, GLASS_STEP, GLASS_ALIVE, GLASS_HIT = 1, 2, 4, 8
GLASS_STATE = 15  # o, d, mint, maxt, beta, prev, rng low, rng high, t

_lib = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(LIB_PATH)
        pf, u32 = C.POINTER(C.c_float), C.c_uint32
        pd = C.POINTER(nori_amd._abi.BsdfDesc)
        l.nori_devtest_math_in.argtypes = l.nori_devtest_math_out.argtypes = [C.c_int]
        l.nori_devtest_math.argtypes = [C.c_int, pf, u32, pf, pf]
        l.nori_devtest_pcg_skip3.argtypes = [C.POINTER(C.c_uint64), u32, C.POINTER(C.c_uint64)]
        l.nori_devtest_bsdf_sample.argtypes = [pd, C.c_int, pf, pf, pf, u32, pf]
        l.nori_devtest_bsdf_eval_pdf.argtypes = [pd, C.c_int, pf, pf, pf, u32, pf]
        l.nori_devtest_glass_words.argtypes = []
        l.nori_devtest_glass.argtypes = [C.c_int, pf, C.c_float, pd, C.c_uint64, pf, pf, pf, u32, C.POINTER(u32)]
        pu32, pu8 = C.POINTER(u32), C.POINTER(C.c_uint8)
        l.nori_devtest_tail_prefix.argtypes = [pu32, u32, pu32]
        l.nori_devtest_tail_lookup.argtypes = [pu32, u32, pu32, u32, pu32, pu32]
        l.nori_devtest_coop_scan.argtypes = [pf, u32, pf, pf, pf, pu8, u32, C.c_int, pu32]
        l.nori_devtest_prim_forms.argtypes = []
        l.nori_devtest_prim_hit.argtypes = [C.c_int, pf, pf, u32, pu32]
        _lib = l
    return _lib


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


def _f32(a, cols):
    a = np.ascontiguousarray(a, np.float32)
    return a.reshape(-1, cols) if cols > 1 else a.reshape(-1)


def _rows(n, *arrays):
    for a in arrays:
        if a is not None and a.shape[0] != n:
            raise ValueError(f"{a.shape[0]} rows where {n} are expected")


def _check(status, what):
    if status != 0:
        raise RuntimeError(f"{what}: HIP error {status}")


def math(op, x, ext_ior=1.0, int_ior=1.0):
    """op over x: (n,) or (n, 3) float32 in, (n,), (n, 3) or (n, 9: s, t, n) out."""
    cin, cout = lib().nori_devtest_math_in(op), lib().nori_devtest_math_out(op)
    x = _f32(x, cin)
    n = x.shape[0]
    out = np.zeros((n, cout) if cout > 1 else n, np.float32)
    iors = np.array([ext_ior, int_ior], np.float32)
    _check(lib().nori_devtest_math(op, _fp(x), n, _fp(iors), _fp(out)), "nori_devtest_math")
    return out


def pcg_skip3(state, inc):
    """(state after pcg_skip3, state after three single steps), uint64 each."""
    a = np.ascontiguousarray(np.stack([state, inc], 1), np.uint64)
    out = np.zeros_like(a)
    p64 = C.POINTER(C.c_uint64)
    _check(lib().nori_devtest_pcg_skip3(a.ctypes.data_as(p64), a.shape[0], out.ctypes.data_as(p64)),
           "nori_devtest_pcg_skip3")
    return out[:, 0], out[:, 1]


def bsdf_sample(desc, wi, u, uv=None, full=True):
    """(n, 8): wo, weight rgb, luminance(weight), measure."""
    wi, u = _f32(wi, 3), _f32(u, 2)
    uv = _f32(uv, 2) if uv is not None else None
    _rows(wi.shape[0], u, uv)
    out = np.zeros((wi.shape[0], 8), np.float32)
    _check(lib().nori_devtest_bsdf_sample(C.byref(desc), int(full), _fp(wi), _fp(u), _fp(uv), wi.shape[0], _fp(out)),
           "nori_devtest_bsdf_sample")
    return out


def bsdf_eval_pdf(desc, wi, wo, uv=None, full=True):
    """(n, 4): bsdf_eval rgb, bsdf_pdf."""
    wi, wo = _f32(wi, 3), _f32(wo, 3)
    uv = _f32(uv, 2) if uv is not None else None
    _rows(wi.shape[0], wo, uv)
    out = np.zeros((wi.shape[0], 4), np.float32)
    _check(lib().nori_devtest_bsdf_eval_pdf(C.byref(desc), int(full), _fp(wi), _fp(wo), _fp(uv), wi.shape[0],
                                            _fp(out)), "nori_devtest_bsdf_eval_pdf")
    return out


def glass(integrator, center, radius, desc, seed, o, d, beta):
    """One chord bounce per lane.  Returns a dict of uint32 arrays: flags (n,),
    and the 15-word states `input`, `step` (glass_step) and `bounce`
    (glass_bounce + chord_hit), each (n, GLASS_STATE)."""
    o, d, beta = _f32(o, 3), _f32(d, 3), _f32(beta, 3)
    n, words = o.shape[0], lib().nori_devtest_glass_words()
    _rows(n, d, beta)
    out = np.zeros((n, words), np.uint32)
    c = np.asarray(center, np.float32)
    _check(lib().nori_devtest_glass(integrator, _fp(c), float(radius), C.byref(desc), seed, _fp(o), _fp(d), _fp(beta),
                                    n, out.ctypes.data_as(C.POINTER(C.c_uint32))), "nori_devtest_glass")
    s = GLASS_STATE
    return {"flags": out[:, 0], "input": out[:, 2:2 + s], "step": out[:, 2 + s:2 + 2 * s],
            "bounce": out[:, 2 + 2 * s:2 + 3 * s]}


def _up(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def tail_prefix(cnt):
    """k_tail_prefix's body over the G counts: (G + 1,) uint32, pre[G] the total."""
    cnt = np.ascontiguousarray(cnt, np.uint32).reshape(-1)
    pre = np.full(cnt.size + 1, 0xDEADBEEF, np.uint32)
    _check(lib().nori_devtest_tail_prefix(_up(cnt), cnt.size, _up(pre)), "nori_devtest_tail_prefix")
    return pre


def tail_lookup(pre, gids):
    """(segment, queue index) of each gid through the prefix pre (G + 1 entries)."""
    pre = np.ascontiguousarray(pre, np.uint32).reshape(-1)
    gids = np.ascontiguousarray(gids, np.uint32).reshape(-1)
    seg, slot = np.zeros(gids.size, np.uint32), np.zeros(gids.size, np.uint32)
    _check(lib().nori_devtest_tail_lookup(_up(pre), pre.size - 1, _up(gids), gids.size, _up(seg), _up(slot)),
           "nori_devtest_tail_lookup")
    return seg, slot


def coop_scan(records, root_min, root_max, rays, want, any_hit=False):
    """coop_load + coop_scan<any_hit> in whole waves of 64 consecutive rays:
    a dict of res (bool), t, u, v (float32) and prim (uint32) per ray."""
    records, rays = _f32(records, 12), _f32(rays, 8)
    want = np.ascontiguousarray(want, np.uint8).reshape(-1)
    n = rays.shape[0]
    _rows(n, want)
    lo, hi = np.asarray(root_min, np.float32), np.asarray(root_max, np.float32)
    out = np.zeros((n, 5), np.uint32)
    _check(lib().nori_devtest_coop_scan(_fp(records), records.shape[0], _fp(lo), _fp(hi), _fp(rays),
                                        want.ctypes.data_as(C.POINTER(C.c_uint8)), n, int(any_hit), _up(out)),
           "nori_devtest_coop_scan")
    return {"res": out[:, 0] != 0, "t": out[:, 1].copy().view(np.float32), "prim": out[:, 2].copy(),
            "u": out[:, 3].copy().view(np.float32), "v": out[:, 4].copy().view(np.float32)}


def prim_hit(form, records, rays):
    """Ray i against record i with one of the forms above: hit (bool), t, u, v
    (float32); BOX: record = (min, ., max, ., unused), returns ok, tnear, 0, 0."""
    records, rays = _f32(records, 12), _f32(rays, 8)
    n = rays.shape[0]
    _rows(n, records)
    out = np.zeros((n, 4), np.uint32)
    _check(lib().nori_devtest_prim_hit(form, _fp(records), _fp(rays), n, _up(out)), "nori_devtest_prim_hit")
    return (out[:, 0] != 0, out[:, 1].copy().view(np.float32), out[:, 2].copy().view(np.float32),
            out[:, 3].copy().view(np.float32))
