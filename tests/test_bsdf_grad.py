"""bsdf_eval's adjoint in the material rows, host side: nori_scene_bsdf_grad and
nori_scene_materials (their statement is in include/nori_gpu.h, the arithmetic in
csrc/bsdf_grad.h) against central differences of the float64 forward of tests/bsdf_ref64.py,
which shares nothing with the code under test.  The scene is material_util's zoo (one BSDF of
every kind, shape b = BSDF b); records are synthetic with ns = (0, 0, 1), whose frame is the
identity, so the directions given are the local ones.  tests/test_gpu_bsdf_grad.py checks the
kernel against this host function.

The finite-difference figures.  Per parameter word w and element: e = |fd - t_w s| / (|t_w| |s|)
with s the step actually taken (the two float32 rows' difference) and fd the central difference of
<g, (eval, pdf)> of the float64 forward, h = 2e-5 relative (some 300 float32 steps).  The terms
are fp32 (2^-24 = 6e-8 per operation, a few dozen operations deep for Disney, with cancellation between the lobes), the
quotient has an O(h^2) truncation.  Margins that keep the directions off the kinks: wi.z, wo.z >=
0.1; kd channels 0.2, 0.1, 0.3 (the maximum is unique by 0.1); Smith's a = 1 / (alpha tan) not
within 2 % of 1.6 (elements inside that band are dropped, they are counted); roughness 0.5
(r^2 = 0.25 against 0.001); luminance 0.47.  Elements whose |t_w| is below 1e-3 of the row's
largest word are measured against the row's largest instead (a word that nearly vanishes has no
relative accuracy to speak of).  Observed (this file's print, largest over words and elements):
diffuse 9.9e-08, checkerboard 9.9e-08, microfacet 9.2e-04 (alpha; 2.3e-04 in the kd channel that
carries ks), disney 4.4e-04 (metallic; roughness 3.1e-04, the other words below 2.1e-05).  The
large ones do not move with h: they are elements in which the word's term is what is left of two
pieces that nearly cancel (g_b / pi against the ks part, the diffuse lobe against the specular one
in metallic), where the fp32 pieces' rounding is large against the rest; the medians are 1e-7.
Cap FD_CAP = 1e-2: the largest times ten, rounded up to one digit; a wrong or missing term shows
as O(1).

The kink conventions are checked where they bite: r^2 <= 0.001 (the flat side's derivative, also at
the largest float r with r r <= 0.001), a >= 1.6, tied kd, zero luminance."""
import ctypes as C

import numpy as np
import pytest

import bsdf_ref64 as R
import material_util as M
import nori_amd
from nori_amd import _abi

f32, f64 = np.float32, np.float64
FD_CAP = 1e-2
INV_PI = f32(0.31830988618379067154)
N = 3000


@pytest.fixture(scope="module")
def zoo(built, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("bgrad"))
    return nori_amd.load_scene(M.zoo_xml(d)), d


def elements(n, seed, zmin=0.1):
    g = np.random.default_rng(seed)
    gout = np.full((n, 8), np.nan, f32)  # words 4-7 are never read
    gout[:, :4] = g.standard_normal((n, 4))
    return M.directions(n, seed + 1, zmin), M.directions(n, seed + 2, zmin), g.uniform(-2, 2, (n, 2)).astype(f32), gout


def fd_error(scene, b, rows, wi, wo, uv, gout, words, h=2e-5, keep=None):
    """Largest e per word of BSDF b at the material rows `rows`."""
    n = len(wi)
    rec = M.records(n, b, uv=uv)
    _, t = nori_amd.bsdf_grad(scene, rec, wi, wo, gout, materials=rows, with_terms=True)
    t = t.astype(f64)
    big = np.abs(t).max(1)
    out = {}
    for w in words:
        p, m = rows.copy(), rows.copy()
        p[b, w] = f32(rows[b, w] * (1 + h) + (h if rows[b, w] == 0 else 0))
        m[b, w] = f32(rows[b, w] * (1 - h) - (h if rows[b, w] == 0 else 0))
        s = f64(p[b, w]) - f64(m[b, w])
        f = []
        for rr in (p, m):
            ev, pdf = R.eval_pdf64(M.desc_with_row(scene.desc.bsdfs[b], rr[b]), wi, wo, uv)
            f.append((ev * gout[:, :3].astype(f64)).sum(1) + pdf * f64(gout[:, 3]))
        fd = f[0] - f[1]
        den = np.maximum(np.abs(t[:, w]), 1e-3 * big) * abs(s)
        sel = (den > 0) if keep is None else (den > 0) & keep
        e = np.abs(fd - t[:, w] * s)[sel] / den[sel]
        assert np.all((fd == 0) | (den > 0)), f"word {w}: a zero row where the forward moves"
        out[w] = float(e.max()) if sel.any() else 0.0
    return out


def smith_band(alpha, v):
    """Elements whose Smith argument a = 1 / (alpha tan theta) is within 2 % of 1.6."""
    with np.errstate(all="ignore"):
        a = 1 / (alpha * R._tan_theta(v.astype(f64)))
    return np.abs(a - 1.6) < 0.032


@pytest.mark.parametrize("kind", ("diffuse", "checker", "microfacet", "disney"))
def test_central_differences_per_word(zoo, kind):
    scene, _ = zoo
    b = M.ZOO.index(kind)
    rows = nori_amd.scene_materials(scene)
    wi, wo, uv, gout = elements(N, 10 + b)
    keep = None
    if kind == "microfacet":
        keep = ~(smith_band(rows[b, 3], wi) | smith_band(rows[b, 3], wo))
        print(f"microfacet: {int((~keep).sum())} of {N} elements inside the a = 1.6 band dropped")
    if kind == "checker":
        first = R.checkerboard(scene.desc.bsdfs[b], uv)
        assert 0.3 < first.mean() < 0.7  # both parities
    e = fd_error(scene, b, rows, wi, wo, uv, gout, M.WORDS[kind], keep=keep)
    print(f"{kind}: largest e per word {{{', '.join(f'{w}: {v:.2e}' for w, v in e.items())}}} -> {max(e.values()):.3e}")
    assert max(e.values()) <= FD_CAP


def test_kink_conventions(zoo):
    scene, _ = zoo
    rows = nori_amd.scene_materials(scene)
    bd, bm = M.ZOO.index("disney"), M.ZOO.index("microfacet")
    wi, wo, uv, gout = elements(N, 40)
    # ---- disney, r^2 <= 0.001: alpha is the constant 0.001 in eval and pdf, only fd90 carries roughness
    flat = rows.copy()
    flat[bd, 6] = 0.03
    e = fd_error(scene, bd, flat, wi, wo, uv, gout, [6])
    print(f"disney r = 0.03 (flat alpha): {e[6]:.3e}")
    assert e[6] <= FD_CAP
    r0 = f32(np.sqrt(0.001))
    while f32(r0 * r0) > f32(0.001) or f64(r0) ** 2 > 1e-3:
        r0 = np.nextafter(r0, f32(0))
    at, below = rows.copy(), rows.copy()
    at[bd, 6], below[bd, 6] = r0, np.nextafter(r0, f32(0))
    rec = M.records(N, bd, uv=uv)
    ta = nori_amd.bsdf_grad(scene, rec, wi, wo, gout, materials=at, with_terms=True)[1]
    tb = nori_amd.bsdf_grad(scene, rec, wi, wo, gout, materials=below, with_terms=True)[1]
    up = rows.copy()
    up[bd, 6] = f32(r0 * f32(1.01))
    tu = nori_amd.bsdf_grad(scene, rec, wi, wo, gout, materials=up, with_terms=True)[1]
    scale = np.abs(tu[:, 6]).max()
    assert np.abs(ta[:, 6] - tb[:, 6]).max() < 1e-4 * scale, "the kink itself is not on the flat side"
    assert np.abs(tu[:, 6] - ta[:, 6]).max() > 1e-2 * scale, "no alpha term above the kink"
    # ---- microfacet, a >= 1.6 for both directions: G = 1 and dG = 0 (alpha 0.1, directions within 60 degrees)
    steep = rows.copy()
    steep[bm, 3] = 0.1
    near = (wi[:, 2] > 0.5) & (wo[:, 2] > 0.5)
    with np.errstate(all="ignore"):
        assert np.all(1 / (0.1 * R._tan_theta(wi[near].astype(f64))) > 1.6)
    e = fd_error(scene, bm, steep, wi, wo, uv, gout, [3], keep=near)
    print(f"microfacet alpha = 0.1, a >= 1.6: {e[3]:.3e}")
    assert e[3] <= FD_CAP
    # ---- tied kd: the ks gradient goes to the first channel that attains the maximum, only
    tied = rows.copy()
    tied[bm, 0:3] = (0.3, 0.3, 0.1)
    tt = nori_amd.bsdf_grad(scene, M.records(N, bm, uv=uv), wi, wo, gout, materials=tied, with_terms=True)[1]
    plain = (gout[:, :3] * INV_PI).astype(f32)
    live = tt.any(1)
    assert live.mean() > 0.9
    assert np.array_equal(tt[live, 1:3].view(np.uint32), plain[live, 1:3].view(np.uint32))
    assert (tt[live, 0] != plain[live, 0]).mean() > 0.9
    # ---- zero luminance: ctint = white carries no derivative, so the tints do not reach base_color
    black, black0 = rows.copy(), rows.copy()
    black[bd, 0:3] = 0
    black0[bd, 0:3] = 0
    black0[bd, 8:10] = 0
    t1 = nori_amd.bsdf_grad(scene, rec, wi, wo, gout, materials=black, with_terms=True)[1]
    t0 = nori_amd.bsdf_grad(scene, rec, wi, wo, gout, materials=black0, with_terms=True)[1]
    assert np.isfinite(t1).all() and t1[:, 0:3].any()
    assert np.allclose(t1[:, 0:3], t0[:, 0:3], rtol=1e-5, atol=1e-6 * np.abs(t0[:, 0:3]).max())


def test_rows_sums_and_payloads(zoo):
    scene, _ = zoo
    nb = scene.desc.num_bsdfs
    g = np.random.default_rng(5)
    n = 2000
    shape = np.where(np.arange(n) % 9 == 8, -1, g.integers(scene.desc.num_shapes, size=n))
    wi, wo, uv, gout = elements(n, 50, zmin=0.05)
    wo[g.random(n) < 0.15, 2] *= -1  # below the surface: the forward's zero branches
    rec = M.records(n, shape, uv=uv)
    sb, kinds = M.shape_bsdfs(scene), M.kinds(scene)
    kind = np.array(["miss" if s < 0 else kinds[sb[s]] for s in shape])
    gm, t = nori_amd.bsdf_grad(scene, rec, wi, wo, gout, with_terms=True)
    assert np.isfinite(t).all() and not t[:, 13:].any()
    # misses, mirror, dielectric and the image-textured diffuse: zero rows
    assert not t[np.isin(kind, ["miss", "mirror", "dielectric", "image"])].any()
    # diffuse and checkerboard rows are g * (1 / pi), bit for bit, routed by the cell's parity
    up = (wi[:, 2] > 0) & (wo[:, 2] > 0)
    want = (gout[:, :3] * INV_PI).astype(f32)
    d = kind == "diffuse"
    assert np.array_equal(t[d & up, 0:3].view(np.uint32), want[d & up].view(np.uint32)) and not t[d & ~up].any()
    c = kind == "checker"
    first = R.checkerboard(scene.desc.bsdfs[M.ZOO.index("checker")], uv)
    assert np.array_equal(t[c & up & first, 0:3].view(np.uint32), want[c & up & first].view(np.uint32))
    assert np.array_equal(t[c & up & ~first, 10:13].view(np.uint32), want[c & up & ~first].view(np.uint32))
    assert not t[c & up & first, 10:13].any() and not t[c & up & ~first, 0:3].any() and not t[c & ~up].any()
    # words outside a kind's set stay zero
    for k, words in M.WORDS.items():
        rest = [w for w in range(16) if w not in words]
        assert not t[kind == k][:, rest].any(), k
    # the sums: float64 in element order, added once to what is there; terms = NULL changes nothing
    pre = g.standard_normal((nb, 16)).astype(f32)
    S = np.zeros((nb, 16))
    hit = shape >= 0
    np.add.at(S, sb[shape[hit]], t[hit].astype(f64))
    want_gm = np.where(S != 0, (pre.astype(f64) + S).astype(f32), pre)
    got = nori_amd.bsdf_grad(scene, rec, wi, wo, gout, grad_materials=pre.copy())
    assert np.array_equal(got.view(np.uint32), want_gm.view(np.uint32))
    assert np.array_equal(gm.view(np.uint32), np.where(S != 0, S.astype(f32), 0).astype(f32).view(np.uint32))
    # NaN payloads in words 4-7 against zeros there
    clean = gout.copy()
    clean[:, 4:] = 0
    assert np.array_equal(nori_amd.bsdf_grad(scene, rec, wi, wo, clean, with_terms=True)[1].view(np.uint32), t.view(np.uint32))
    # linearity in grad_out: exact for a power of two, to rounding for a sum
    t2 = nori_amd.bsdf_grad(scene, rec, wi, wo, (clean * f32(4)).astype(f32), with_terms=True)[1]
    assert np.array_equal(t2.view(np.uint32), (t * f32(4)).astype(f32).view(np.uint32))
    other = clean.copy()
    other[:, :4] = g.standard_normal((n, 4))
    ta = nori_amd.bsdf_grad(scene, rec, wi, wo, other, with_terms=True)[1]
    ts = nori_amd.bsdf_grad(scene, rec, wi, wo, (clean + other).astype(f32), with_terms=True)[1]
    both = t.any(1) & ta.any(1) & ts.any(1)
    assert np.all(np.abs(ts - (t + ta))[both] <= 1e-4 * (np.abs(t) + np.abs(ta))[both].max(1, keepdims=True))
    # a non-finite word 0 zeroes that element's row and no other
    bad = gout.copy()
    victims = np.flatnonzero(t.any(1))[:5]
    bad[victims[0], 0], bad[victims[1], 3], bad[victims[2], 1] = np.nan, np.inf, -np.inf
    tb = nori_amd.bsdf_grad(scene, rec, wi, wo, bad, with_terms=True)[1]
    assert not tb[victims[:3]].any()
    rest = np.ones(n, bool)
    rest[victims[:3]] = False
    assert np.array_equal(tb[rest].view(np.uint32), t[rest].view(np.uint32))


def test_materials_argument_against_a_scene_loaded_with_them(zoo, tmp_path):
    scene, d = zoo
    rows = nori_amd.scene_materials(scene)
    g = np.random.default_rng(6)
    for b, kind in enumerate(M.kinds(scene)):
        rows[b, M.WORDS[kind]] = g.uniform(0.1, 0.9, len(M.WORDS[kind])).astype(f32)
    copy = nori_amd.load_scene(M.write_with_rows(f"{d}/zoo.xml", rows, str(tmp_path / "copy.xml")))
    assert np.array_equal(nori_amd.scene_materials(copy).view(np.uint32), rows.view(np.uint32))
    n = 1500
    wi, wo, uv, gout = elements(n, 60)
    rec = M.records(n, g.integers(scene.desc.num_shapes, size=n), uv=uv)
    a = nori_amd.bsdf_grad(scene, rec, wi, wo, gout, materials=rows, with_terms=True)
    c = nori_amd.bsdf_grad(copy, rec, wi, wo, gout, with_terms=True)
    assert a[1].any() and np.array_equal(a[0].view(np.uint32), c[0].view(np.uint32))
    assert np.array_equal(a[1].view(np.uint32), c[1].view(np.uint32))
    own = nori_amd.bsdf_grad(scene, rec, wi, wo, gout)
    assert not np.array_equal(own, a[0])  # (the rows matter)


def test_scene_materials_against_the_descriptors(zoo):
    scene, _ = zoo
    rows = nori_amd.scene_materials(scene)
    assert rows.shape == (scene.desc.num_bsdfs, 16)
    for b, kind in enumerate(M.kinds(scene)):
        d = scene.desc.bsdfs[b]
        want = np.zeros(16, f32)
        if kind in ("diffuse", "checker"):
            want[0:3] = list(d.albedo)
        if kind == "checker":
            want[10:13] = list(d.tex_value2)
        if kind == "microfacet":
            want[0:3], want[3] = list(d.kd), d.alpha
        if kind == "disney":
            want[0:3] = list(d.base_color)
            want[4:10] = [d.metallic, d.specular, d.roughness, d.sheen, d.sheen_tint, d.specular_tint]
        assert np.array_equal(rows[b].view(np.uint32), want.view(np.uint32)), (b, kind)
    assert M.kinds(scene)[:7] == M.ZOO


def test_refusals_write_nothing(zoo):
    scene, _ = zoo
    nb, n = scene.desc.num_bsdfs, 50
    wi, wo, uv, gout = elements(n, 70)
    rec = M.records(n, 0, uv=uv)
    gm, tm = np.full((nb, 16), 5.0, f32), np.full((n, 16), 5.0, f32)
    lib = nori_amd.lib()
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    args = [scene.desc_ptr, None, n, ptr(rec), ptr(wi), ptr(wo), ptr(gout), ptr(gm), ptr(tm)]
    assert lib.nori_scene_bsdf_grad(*args) == 0 and (gm != 5.0).any()
    gm[:], tm[:] = 5.0, 5.0
    for k in (0, 3, 4, 5, 6, 7):
        bad = list(args)
        bad[k] = None
        assert lib.nori_scene_bsdf_grad(*bad) == _abi.NORI_ERR_INVALID, k
    for s in (-2, scene.desc.num_shapes):
        r2 = rec.copy()
        r2["shape"][n - 1] = s
        bad = list(args)
        bad[3] = ptr(r2)
        assert lib.nori_scene_bsdf_grad(*bad) == _abi.NORI_ERR_INVALID, s
    assert np.all(gm == 5.0) and np.all(tm == 5.0)
    assert lib.nori_scene_materials(None, ptr(gm)) == _abi.NORI_ERR_INVALID
    assert lib.nori_scene_materials(scene.desc_ptr, None) == _abi.NORI_ERR_INVALID
