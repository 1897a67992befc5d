"""First-hit features and the feature-guided denoiser, host side: the ABI mirror,
nori_film_features, and nori_film_denoise_guided -- the filter's double-precision
statement (include/nori_gpu.h) -- against a numpy restatement written here, its
structural properties and its argument validation.  tests/test_gpu_features.py
checks the kernels against these host functions."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import nori_amd
from conftest import ROOT, scene_path
from nori_amd import _abi

HEADER = os.path.join(ROOT, "include", "nori_gpu.h")
INF = float("inf")
SHAPES = [(4, 5), (17, 23), (33, 40)]          # (height, width)
RF = [(0, 0), (1, 1), (5, 1), (8, 3)]          # (radius, patch)
# parameters of the comparisons with random inputs: weights spread over (0, 1) instead of the
# near-binary weights the defaults give on white noise
PARAMS = dict(k=1.5, eps=1e-10, sigma_albedo=1.5, sigma_normal=2.0, sigma_depth=1.0)


def random_inputs(h, w, seed):
    """rgb in [0, 1], variance in [0, 0.05], features: albedo in [0, 1], normals in [-1, 1],
    depth in [0.5, 5]; about one pixel in ten is a miss (all seven features zero)."""
    g = np.random.default_rng(seed)
    rgb = g.random((h, w, 3)).astype(np.float32)
    var = (0.05 * g.random((h, w))).astype(np.float32)
    feat = np.concatenate([g.random((h, w, 3)), 2 * g.random((h, w, 3)) - 1, 0.5 + 4.5 * g.random((h, w, 1))], -1)
    feat[g.random((h, w)) < 0.1] = 0.0
    return rgb, var, feat.astype(np.float32)


def _shifted(a, dy, dx):
    """b[y, x] = a[y + dy, x + dx] where that is inside the frame (0 elsewhere), and the mask."""
    h, w = a.shape[:2]
    b, ok = np.zeros_like(a), np.zeros((h, w), bool)
    y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
    if y0 < y1 and x0 < x1:
        b[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        ok[y0:y1, x0:x1] = True
    return b, ok


def np_guided(rgb, var, feat, radius, patch, k, eps, sigma_albedo, sigma_normal, sigma_depth):
    """The guided filter of include/nori_gpu.h in float64: loops over the neighbour and patch
    offsets, whole-image numpy inside."""
    I, v, f = rgb.astype(np.float64), var.astype(np.float64), feat.astype(np.float64)
    h, w = v.shape
    acc, wsum = np.zeros((h, w, 3)), np.zeros((h, w))
    k2, eps = float(np.float32(k)) ** 2, float(np.float32(eps))  # (the descriptor holds float32)
    inv = [0.0 if np.isinf(s) else 1.0 / float(np.float32(s)) ** 2 for s in (sigma_albedo, sigma_normal, sigma_depth)]
    for sy in range(-radius, radius + 1):
        for sx in range(-radius, radius + 1):
            Iq, q_in = _shifted(I, sy, sx)
            fq, _ = _shifted(f, sy, sx)
            total, count = np.zeros((h, w)), np.zeros((h, w))
            for oy in range(-patch, patch + 1):
                for ox in range(-patch, patch + 1):
                    Ia, a_in = _shifted(I, oy, ox)
                    va, _ = _shifted(v, oy, ox)
                    Ib, b_in = _shifted(I, sy + oy, sx + ox)
                    vb, _ = _shifted(v, sy + oy, sx + ox)
                    ok = a_in & b_in
                    term = (((Ia - Ib) ** 2).sum(-1) - (va + np.minimum(va, vb))) / (eps + k2 * (va + vb))
                    total += np.where(ok, term, 0.0)
                    count += ok
            d2c = total / np.maximum(count, 1)
            d2f = np.zeros((h, w))
            if inv[0]:
                d2f += ((f[..., 0:3] - fq[..., 0:3]) ** 2).sum(-1) * inv[0]
            if inv[1]:
                d2f += ((f[..., 3:6] - fq[..., 3:6]) ** 2).sum(-1) * inv[1]
            if inv[2]:
                rel = (f[..., 6] - fq[..., 6]) / np.maximum(np.maximum(f[..., 6], fq[..., 6]), 1e-6)
                d2f += rel ** 2 * inv[2]
            wgt = np.where(q_in, np.exp(-np.maximum(0.0, d2c)) * np.exp(-d2f), 0.0)
            acc += wgt[..., None] * Iq
            wsum += wgt
    return acc / wsum[..., None]


def box_mean(img, radius, member=None):
    """Mean over the in-frame (2r+1)^2 neighbours; `member[y, x]` restricts pixel p's neighbours
    to those q with member[q] == member[p]."""
    h, w = img.shape[:2]
    out = np.zeros((h, w, 3))
    for y in range(h):
        for x in range(w):
            ys, xs = slice(max(0, y - radius), min(h, y + radius + 1)), slice(max(0, x - radius), min(w, x + radius + 1))
            sel = np.ones((ys.stop - ys.start, xs.stop - xs.start), bool) if member is None else \
                member[ys, xs] == member[y, x]
            out[y, x] = img[ys, xs][sel].astype(np.float64).sum(0) / sel.sum()
    return out


def two_halves(seed=5):
    """The edge-stop input: a 16x16 image of multiples of 1/64 (so that sums are exact), a variance so
    large that the colour distance is <= 0 everywhere, and an albedo feature that is 0 in the left
    half and 1 in the right half."""
    g = np.random.default_rng(seed)
    rgb = (g.integers(0, 65, (16, 16, 3)) / 64.0).astype(np.float32)
    var = np.full((16, 16), 1e6, np.float32)
    feat = np.zeros((16, 16, 7), np.float32)
    feat[:, 8:, 0:3] = 1.0
    side = np.zeros((16, 16), int)
    side[:, 8:] = 1
    return rgb, var, feat, side


def test_abi_mirror(built, tmp_path):
    assert _abi.ABI_VERSION == 7 and nori_amd.lib().nori_gpu_abi_version() == 7
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             'printf("size %zu\\n", sizeof(nori_guided_desc));']
    for name, _ in _abi.GuidedDesc._fields_:
        lines.append(f'printf("{name} %zu\\n", offsetof(nori_guided_desc, {name}));')
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                 check=True).stdout.splitlines() if l)
    assert int(out["size"]) == C.sizeof(_abi.GuidedDesc) == 32
    for name, _ in _abi.GuidedDesc._fields_:
        assert int(out[name]) == getattr(_abi.GuidedDesc, name).offset, name
    for fn in ("nori_gpu_render_features", "nori_film_features", "nori_film_denoise_guided", "nori_denoise_guided"):
        assert hasattr(nori_amd.lib(), fn) and fn in open(HEADER).read()


def test_film_features_means(built):
    s = nori_amd.load_scene(scene_path("pa4", "cbox", "cbox_path_mis.xml"), 3, 2, 1)
    sums = np.zeros((2, 3, 8), np.float32)
    sums[0, 0] = [0.5, 1.0, 1.5, 0.0, 2.0, -2.0, 7.0, 2.0]      # two samples
    sums[0, 1] = [0.3, 0.3, 0.3, -3.0, 0.0, 0.0, 9.0, 3.0]      # three samples
    sums[0, 2] = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 4.0]       # four misses
    sums[1, 0] = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 0.0]       # count 0: zeros, whatever the sums hold
    sums[1, 1] = [0.725, 0.71, 0.68, 0.6, 0.0, 0.8, 3.25, 1.0]  # one sample: the values themselves
    sums[1, 2] = [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 7.0]
    got = nori_amd.film_features(s, sums)
    assert got.shape == (2, 3, 7) and got.dtype == np.float32
    n = sums[..., 7:8].astype(np.float64)
    want = np.where(n > 0, sums[..., 0:7].astype(np.float64) / np.maximum(n, 1), 0.0).astype(np.float32)
    assert np.array_equal(got, want)
    assert not got[1, 0].any() and not got[0, 2].any()
    assert np.array_equal(got[1, 1], sums[1, 1, 0:7])
    # the normal is the mean, not renormalised
    assert np.array_equal(got[0, 0, 3:6], np.float32([0.0, 1.0, -1.0]))


def test_film_features_errors(built):
    s = nori_amd.load_scene(scene_path("pa4", "cbox", "cbox_path_mis.xml"), 3, 2, 1)
    f = nori_amd.lib().nori_film_features
    a, b = np.zeros((2, 3, 8), np.float32), np.zeros((2, 3, 7), np.float32)
    pa, pb = nori_amd._fptr(a), nori_amd._fptr(b)
    assert f(s.desc_ptr, pa, pb) == _abi.NORI_OK
    assert f(None, pa, pb) == _abi.NORI_ERR_INVALID
    assert f(s.desc_ptr, None, pb) == _abi.NORI_ERR_INVALID
    assert f(s.desc_ptr, pa, None) == _abi.NORI_ERR_INVALID
    with pytest.raises(ValueError):
        nori_amd.film_features(s, np.zeros((2, 3, 7), np.float32))


@pytest.mark.parametrize("r,f", RF)
@pytest.mark.parametrize("h,w", SHAPES)
def test_host_statement_matches_numpy(built, h, w, r, f):
    """Both sides are float64; the library returns float32, so the restatement is rounded the same way."""
    rgb, var, feat = random_inputs(h, w, seed=1000 * h + 10 * w + r)
    got = nori_amd.film_denoise_guided(rgb, var, feat, radius=r, patch=f, **PARAMS)
    want = np_guided(rgb, var, feat, r, f, **PARAMS).astype(np.float32)
    assert got.shape == (h, w, 3) and np.isfinite(got).all()
    err = np.max(np.abs(got.astype(np.float64) - want) / np.abs(want))
    print("max relative difference", err)
    assert err <= 1e-12
    if r > 0:  # the filter does something on these inputs
        assert np.max(np.abs(got - rgb)) > 1e-2


def test_host_statement_infinite_sigma_is_exactly_off(built):
    """A term whose sigma is +inf is exactly 0 -- also where the features are not finite."""
    rgb, var, feat = random_inputs(17, 23, seed=3)
    p = dict(PARAMS, sigma_normal=INF)
    want = np_guided(rgb, var, feat, 2, 1, **p).astype(np.float32)
    bad = feat.copy()
    bad[3, 4, 3:6] = [np.nan, np.inf, -np.inf]
    got = nori_amd.film_denoise_guided(rgb, var, bad, radius=2, patch=1, **p)
    assert np.max(np.abs(got.astype(np.float64) - want) / np.abs(want)) <= 1e-12
    assert np.max(np.abs(got - nori_amd.film_denoise_guided(rgb, var, feat, radius=2, patch=1, **PARAMS))) > 1e-4


@pytest.mark.parametrize("r,f", [(1, 0), (3, 1), (8, 3)])
def test_box_mean_when_every_weight_is_one(built, r, f):
    g = np.random.default_rng(r)
    rgb = (g.integers(0, 65, (13, 19, 3)) / 64.0).astype(np.float32)
    _, _, feat = random_inputs(13, 19, seed=r)
    got = nori_amd.film_denoise_guided(rgb, np.full((13, 19), 1e6, np.float32), feat, radius=r, patch=f, k=0.45,
                                       eps=1e-10, sigma_albedo=INF, sigma_normal=INF, sigma_depth=INF)
    assert np.array_equal(got, box_mean(rgb, r).astype(np.float32))


def test_edge_stop(built):
    rgb, var, feat, side = two_halves()
    kw = dict(radius=3, patch=1, k=0.45, eps=1e-10, sigma_normal=INF, sigma_depth=INF)
    got = nori_amd.film_denoise_guided(rgb, var, feat, sigma_albedo=0.1, **kw)
    own = box_mean(rgb, 3, member=side).astype(np.float32)
    assert np.max(np.abs(got.astype(np.float64) - own)) <= 1e-9  # the cross weight is e^-100
    # without the albedo term the halves mix: the assertion above can fail
    mixed = nori_amd.film_denoise_guided(rgb, var, feat, sigma_albedo=INF, **kw)
    assert np.array_equal(mixed, box_mean(rgb, 3).astype(np.float32))
    near = np.abs(np.arange(16) - 7.5) < 3
    assert np.max(np.abs(mixed.astype(np.float64) - own)[:, near]) > 1e-2
    assert np.array_equal(mixed[:, ~near], own[:, ~near])  # windows that do not reach the other half


def test_constant_image_is_unchanged(built):
    _, var, feat = random_inputs(17, 23, seed=9)
    rgb = np.empty((17, 23, 3), np.float32)
    rgb[...] = np.float32([0.3, 0.7, 1.9])
    assert np.array_equal(nori_amd.film_denoise_guided(rgb, var, feat, radius=5, patch=1, **PARAMS), rgb)
    assert np.array_equal(nori_amd.film_denoise_guided(rgb, var, feat), rgb)  # the defaults


def _call(fn_name, rgb, var, feat, w, h, desc, out):
    f = getattr(nori_amd.lib(), fn_name)
    args = [None if a is None else nori_amd._fptr(a) for a in (rgb, var, feat)]
    o = None if out is None else nori_amd._fptr(out)
    d = None if desc is None else C.byref(desc)
    if fn_name == "nori_denoise_guided":
        return f(0, *args, w, h, d, o)
    return f(*args, w, h, d, o)


def _good_desc(**kw):
    d = _abi.GuidedDesc(2, 1, 0.45, 1e-10, 0.1, 0.25, 0.1, 0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


BAD_DESC = ([dict(radius=-1), dict(radius=9), dict(patch=-1), dict(patch=4), dict(reserved=1)]
            + [{name: v} for name in ("k", "eps", "sigma_albedo", "sigma_normal", "sigma_depth")
               for v in (0.0, -1.0, float("nan"))])


# (the device entry point checks its arguments before it touches the device, so both run here)
@pytest.mark.parametrize("fn", ["nori_film_denoise_guided", "nori_denoise_guided"])
def test_invalid_arguments(built, fn):
    rgb, var, feat = random_inputs(4, 5, seed=1)
    out = np.full((4, 5, 3), -7.0, np.float32)
    ok = (rgb, var, feat, 5, 4, _good_desc(), out)
    if fn == "nori_film_denoise_guided":
        assert _call(fn, *ok) == _abi.NORI_OK
        assert _call(fn, rgb, var, feat, 5, 4, _good_desc(sigma_albedo=INF, sigma_normal=INF, sigma_depth=INF),
                     out) == _abi.NORI_OK
        out[...] = -7.0
    for i in (0, 1, 2, 5, 6):  # a null pointer: rgb, variance, feat7, the descriptor, out
        a = list(ok)
        a[i] = None
        assert _call(fn, *a) == _abi.NORI_ERR_INVALID, i
    for w, h in ((0, 4), (5, 0), (-5, 4), (5, -4)):
        assert _call(fn, rgb, var, feat, w, h, _good_desc(), out) == _abi.NORI_ERR_INVALID, (w, h)
    for kw in BAD_DESC:
        assert _call(fn, rgb, var, feat, 5, 4, _good_desc(**kw), out) == _abi.NORI_ERR_INVALID, kw
    assert (out == -7.0).all()
    with pytest.raises(ValueError):
        nori_amd.film_denoise_guided(rgb, var, feat[..., :6])
