"""ctypes loader of libnori_devtest.so (nori-ray-tracer_amd/csrc/devtest.hip):
the device routines of device_math.h and shading.h as element-wise kernels
behind C entry points, with thin numpy wrappers.  No assertions here; a HIP
error raises RuntimeError."""
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
