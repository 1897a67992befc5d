"""bsdf_eval's adjoint in the material rows on the GPU: nori_gpu_bsdf_grad (k_bsdf_grad and
k_bsdf_grad_sum, csrc/kernels_bsdf_grad.hip), stated at nori_scene_bsdf_grad in include/nori_gpu.h.

Hit records are the caller's, so they are synthesised: a shape per element, a random unit ns, local
directions taken to the world, a random gradient row whose words 4-7 hold NaN.  Scenes: the veach
plates (microfacet), the Disney box, pa1/mesh-texture.xml (checkerboard), a box of 70 diffuse
spheres (more BSDFs than NORI_BSDF_GRAD_MAX_TABLE = 64: the atomic path) and the zoo of
material_util (one BSDF of every kind).  NORI_BSDF_GRAD_TABLE=0 sends the small scenes down the
atomic path too.

1. The device's terms against the host statement's.  Both run bsdf_grad.h's fp32 sequence on the
   same inputs, so diffuse, checkerboard and the parameter-free kinds agree bit for bit.  Microfacet
   calls expf in beckmann_D: glibc's and the device library's are each within 1 ulp, so D differs
   by at most 2 ulp (what EXPF_TOL of tests/test_gpu_device_units.py starts from); D enters every
   piece of the row but kd / pi and wo.z / pi linearly, and each of the at most 14 operations
   between D and a term can round the two slightly different values apart by one more ulp:
   16 ulp = TOL_U = 16 * 2^-23, relative to the magnitude of the pieces that are added, not to
   their sum.  The test gets those magnitudes from the statement itself, by linearity: |T_rgb|
   (the row for (|g_r|, |g_g|, |g_b|, 0)) + |T_p| (for (0, 0, 0, |g_p|)) + 2 |g_p| wo.z / pi (the
   two sides of p_ks = D J - wo.z / pi) + |g| / pi, all times rho >= 1, the float64 ratio
   (|dD| G + D |dG|) / |dD G + D dG| of the one sum inside s_al that linearity cannot split.
   Directions are exact on both sides (to_local is + and * only), so DIR_TOL has nothing to
   grant here.  Disney has no transcendental; it is held to the same bound and its exact share is
   printed.  The share of the bound in use is printed (observed: see DESIGN.md D21).
2. Every output float against the float64 sum S of the device's own terms:
   |out - S| <= m 2^-24 A + 2^-120 (m non-zero terms, A their magnitude sum), sizes 1 .. 1000,
   six patterns, both paths.
3. Two identical calls agree bit for bit on the table path; 4. host, device and chunked forms;
5. refusals."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import bsdf_ref64 as R
import material_util as M
import nori_amd
from conftest import scene_path
from nori_amd import _abi

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
SIZES = (1, 63, 64, 65, 257, 1000)
PATTERNS = ("one", "alt", "runs", "distinct", "miss3", "misswaves")
SCENES = ("zoo", "veach", "disney", "checker", "many")
TOL_U = 16 * 2.0 ** -23
_CACHE = {}


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    try:
        os.environ.update({k: str(v) for k, v in kw.items()})
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    """The module's contexts are destroyed when it ends: a context left open keeps its HIP streams,
    and the streams of later modules' renders would share the hardware queues with them."""
    yield
    for _, r in _CACHE.values():
        r.close()
    _CACHE.clear()


def scene_of(tmp_path_factory, which):
    """(scene, renderer): one context per scene for the whole module."""
    if which not in _CACHE:
        if which in ("zoo", "many"):
            d = str(tmp_path_factory.mktemp(f"bgrad_{which}"))
            s = nori_amd.load_scene(M.zoo_xml(d) if which == "zoo" else M.many_xml(d), 32, 32, 1)
        else:
            path = {"veach": ("pa3", "veach_mi", "veach_ems.xml"), "disney": ("project", "disney", "cbox_path_mis.xml"),
                    "checker": ("pa1", "mesh-texture.xml")}[which]
            s = nori_amd.load_scene(scene_path(*path), 32, 32, 1)
        _CACHE[which] = (s, nori_amd.GpuRenderer(s, 0))
    return _CACHE[which]


def shapes_for(scene, kind, n, seed):
    """The shape of every element: patterns over the scene's shapes (one BSDF each here or several
    shapes per BSDF, either way the BSDF id follows the shape)."""
    ns = scene.desc.num_shapes
    sb = M.shape_bsdfs(scene)
    kinds = M.kinds(scene)
    live = [s for s in range(ns) if M.WORDS[kinds[sb[s]]]]  # shapes whose BSDF has parameters
    g = np.random.default_rng(2000 + seed)
    i = np.arange(n)
    if kind == "one":
        return np.full(n, live[seed % len(live)])
    if kind == "alt":
        return np.where(i % 2 == 0, live[0], live[-1])
    if kind == "runs":  # runs of equal ids whose boundaries fall inside a wave
        out, lengths, k = [], (5, 17, 1, 40, 3, 64, 9, 2, 70, 1, 1, 30), 0
        while len(out) < n:
            out += [int(g.integers(ns))] * lengths[k % len(lengths)]
            k += 1
        return np.array(out[:n])
    if kind == "distinct":  # every lane of a wave another shape (as far as the scene has them)
        return (i + 7 * (i // 64)) % ns
    if kind == "miss3":
        return np.where(i % 3 == 2, -1, g.integers(ns, size=n))
    assert kind == "misswaves"
    return np.where((i // 64) % 2 == 1, -1, g.integers(ns, size=n))


def inputs(scene, shape, seed):
    n = len(shape)
    g = np.random.default_rng(3000 + seed)
    nsv = M.random_frames(n, seed)
    wi = M.world_dirs(nsv, M.directions(n, seed + 1))
    lo = M.directions(n, seed + 2)
    lo[g.random(n) < 0.1, 2] *= -1  # a tenth below the surface: the forward's zero branches
    wo = M.world_dirs(nsv, lo)
    uv = g.uniform(-3, 3, (n, 2)).astype(f32)
    gout = np.full((n, 8), np.nan, f32)
    gout[:, :4] = g.standard_normal((n, 4))
    return M.records(n, shape, ns=nsv, uv=uv), wi, wo, gout


def float64_sums(scene, shape, terms):
    """(S, m, A) per destination float from per-element rows: float64 sum, non-zero count, magnitude sum."""
    nb = scene.desc.num_bsdfs
    sb = M.shape_bsdfs(scene)
    S, m, A = np.zeros((nb, 16)), np.zeros((nb, 16)), np.zeros((nb, 16))
    hit = shape >= 0
    b = sb[shape[hit]]
    t = terms[hit].astype(f64)
    np.add.at(S, b, t)
    np.add.at(m, b, (t != 0).astype(f64))
    np.add.at(A, b, np.abs(t))
    return S, m, A


def assert_sum_bound(out, S, m, A, what):
    bound = m * 2.0 ** -24 * A + 2.0 ** -120
    err = np.abs(out.astype(f64) - S)
    assert np.all(out[m == 0] == 0), f"{what}: a destination without terms was written"
    assert np.all(err <= bound), f"{what}: {err.max():.3e} beyond the bound at {np.argwhere(err > bound)[:4].tolist()}"
    return float((err / bound).max())


def _dG1(v, m, alpha):
    """d smith_G1 / d alpha in float64 (0 on the early returns and for a >= 1.6)."""
    tt = R._tan_theta(v)
    with np.errstate(all="ignore"):
        a = 1 / (alpha * tt)
        N, Q = 3.535 * a + 2.181 * a * a, 1 + 2.276 * a + 2.577 * a * a
        d = ((3.535 + 4.362 * a) * Q - N * (2.276 + 5.154 * a)) / (Q * Q) * (-a / alpha)
    d = np.where((a >= 1.6) | ((m * v).sum(1) * v[:, 2] <= 0) | (tt == 0), 0.0, d)
    return np.nan_to_num(d)


def microfacet_rho(row, wi_l, wo_l):
    """(|dD| G + D |dG|) / |dD G + D dG| in float64, 1 where the sum is 0 or the lobe underflows."""
    alpha = float(row[3])
    wi_l, wo_l = wi_l.astype(f64), wo_l.astype(f64)
    h = wi_l + wo_l
    h /= np.sqrt((h * h).sum(1))[:, None]
    with np.errstate(all="ignore"):
        tt = R._tan_theta(h) / alpha
        dD = 2 * (tt * tt - 1) / alpha  # (over D)
        Gi, Go = R._smith_g1(wi_l, h, alpha), R._smith_g1(wo_l, h, alpha)
        dG = _dG1(wi_l, h, alpha) * Go + Gi * _dG1(wo_l, h, alpha)
        rho = (np.abs(dD) * Gi * Go + np.abs(dG)) / np.abs(dD * Gi * Go + dG)
    return np.where(np.isfinite(rho), np.maximum(rho, 1.0), 1.0)


@pytest.mark.parametrize("which", SCENES)
def test_terms_against_the_host_statement(built, tmp_path_factory, which):
    scene, r = scene_of(tmp_path_factory, which)
    n = 1000
    shape = shapes_for(scene, "miss3", n, 1)
    rec, wi, wo, gout = inputs(scene, shape, 11)
    _, host = nori_amd.bsdf_grad(scene, rec, wi, wo, gout, with_terms=True)
    _, dev = r.bsdf_grad(rec, wi, wo, gout, terms=True)
    assert np.all(dev[:, 13:] == 0) and np.all(np.isfinite(dev))
    sb, kinds = M.shape_bsdfs(scene), M.kinds(scene)
    kind = np.array(["miss" if s < 0 else kinds[sb[s]] for s in shape])
    rows = nori_amd.scene_materials(scene)
    exact = np.isin(kind, ["miss", "diffuse", "checker", "mirror", "dielectric", "image"])
    assert np.array_equal(dev[exact].view(np.uint32), host[exact].view(np.uint32)), "diffuse / checkerboard rows differ in bits"
    assert not dev[np.isin(kind, ["miss", "mirror", "dielectric", "image"])].any()
    share = 0.0
    for k in ("microfacet", "disney"):
        sel = kind == k
        if not sel.any():
            continue
        ga = np.abs(gout[sel]).copy()
        g_rgb, g_p = ga.copy(), ga.copy()
        g_rgb[:, 3:] = 0
        g_p[:, :3] = 0
        g_p[:, 4:] = 0
        _, t_rgb = nori_amd.bsdf_grad(scene, rec[sel], wi[sel], wo[sel], g_rgb, with_terms=True)
        _, t_p = nori_amd.bsdf_grad(scene, rec[sel], wi[sel], wo[sel], g_p, with_terms=True)
        fr = R.frame32(rec["ns"][sel]).reshape(-1, 3, 3).astype(f64)
        wi_l = np.einsum("nkj,nj->nk", fr, wi[sel].astype(f64))
        wo_l = np.einsum("nkj,nj->nk", fr, wo[sel].astype(f64))
        rho = np.ones(sel.sum())
        if k == "microfacet":
            for b in np.unique(sb[shape[sel]]):
                on = sb[shape[sel]] == b
                rho[on] = microfacet_rho(rows[b], wi_l[on], wo_l[on])
        mag = rho[:, None] * (np.abs(t_rgb).astype(f64) + np.abs(t_p)) \
            + (2 * ga[:, 3] * np.abs(wo_l[:, 2]) / np.pi + ga[:, :3].sum(1) / np.pi)[:, None]
        err = np.abs(dev[sel].astype(f64) - host[sel].astype(f64))
        zero_both = ~host[sel].any(1) & ~dev[sel].any(1)
        # a row that is zeroed as a whole on one side only (a non-finite float within an ulp of the
        # other side's finite one) would show here as a full-size error: none is allowed
        tol = TOL_U * mag + 2.0 ** -120
        assert np.all(err[~zero_both] <= tol[~zero_both]), f"{which} {k}: {(err / tol).max():.3f} of the bound"
        same = float((dev[sel].view(np.uint32) == host[sel].view(np.uint32)).all(1).mean())
        share = max(share, float((err / tol).max()))
        print(f"{which} {k}: {int(sel.sum())} rows, {same:.3f} bit-equal, share of the bound {float((err / tol).max()):.3f}")
    print(f"{which}: largest share {share:.3f}")


@pytest.mark.parametrize("table", (1, 0))
@pytest.mark.parametrize("kind", PATTERNS)
def test_sums_against_the_devices_own_terms(built, tmp_path_factory, kind, table):
    import torch

    worst = 0.0
    for which in SCENES:
        scene, r = scene_of(tmp_path_factory, which)
        nb = scene.desc.num_bsdfs
        for n in SIZES:
            shape = shapes_for(scene, kind, n, n)
            rec, wi, wo, gout = inputs(scene, shape, n)
            d = [torch.from_numpy(a.view(f32).reshape(n, -1) if a.dtype == nori_amd.SURFACE_DTYPE else a).cuda()
                 for a in (rec, wi, wo, gout)]
            gm = torch.zeros((nb, 16), dtype=torch.float32, device="cuda")
            tm = torch.full((n, 16), 7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            with _env(NORI_BSDF_GRAD_TABLE=table):
                r.bsdf_grad(*d, grad_materials=gm, terms=tm)
            S, m, A = float64_sums(scene, shape, tm.cpu().numpy())
            worst = max(worst, assert_sum_bound(gm.cpu().numpy(), S, m, A, f"{which} {kind} n={n} table={table}"))
    print(f"{kind} table={table}: largest share of m 2^-24 A: {worst:.3f}")


@pytest.mark.parametrize("which", ("zoo", "veach"))
def test_two_calls_agree_bit_for_bit(built, tmp_path_factory, which):
    scene, r = scene_of(tmp_path_factory, which)
    n = 70001  # 274 tiles: every work-group sums several
    shape = shapes_for(scene, "runs", n, 5)
    rec, wi, wo, gout = inputs(scene, shape, 5)
    a = r.bsdf_grad(rec, wi, wo, gout)
    b = r.bsdf_grad(rec, wi, wo, gout)
    assert a.any() and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("which,table", (("zoo", 1), ("disney", 1), ("zoo", 0), ("many", 1)))
def test_host_device_and_chunked_forms_agree(built, tmp_path_factory, which, table):
    import torch

    scene, r = scene_of(tmp_path_factory, which)
    nb = scene.desc.num_bsdfs
    n = 3000
    shape = shapes_for(scene, "miss3", n, 9)
    rec, wi, wo, gout = inputs(scene, shape, 9)
    pre = np.random.default_rng(4).standard_normal((nb, 16)).astype(f32)
    with _env(NORI_BSDF_GRAD_TABLE=table):
        host, th = r.bsdf_grad(rec, wi, wo, gout, grad_materials=pre.copy(), terms=True)
        with _env(NORI_QUERY_CHUNK=700):
            chunked, tc = r.bsdf_grad(rec, wi, wo, gout, grad_materials=pre.copy(), terms=True)
        d = [torch.from_numpy(a.view(f32).reshape(n, -1) if a.dtype == nori_amd.SURFACE_DTYPE else a).cuda()
             for a in (rec, wi, wo, gout)]
        gm = torch.from_numpy(pre.copy()).cuda()
        torch.cuda.synchronize()
        r.bsdf_grad(*d, grad_materials=gm)
        dev = gm.cpu().numpy()
    assert np.array_equal(th.view(np.uint32), tc.view(np.uint32))
    if table and nb <= _abi.BSDF_GRAD_MAX_TABLE:
        assert np.array_equal(host.view(np.uint32), dev.view(np.uint32)), "host and device forms differ"
        assert np.array_equal(host.view(np.uint32), chunked.view(np.uint32)), "the chunking shows in the bits"
    else:
        S, m, A = float64_sums(scene, shape, th)
        for out in (host, chunked, dev):
            # (the pre-filled value joins the sum as one more term)
            err = np.abs(out.astype(f64) - (S + pre))
            assert np.all(err <= (m + 1) * 2.0 ** -24 * (A + np.abs(pre)) + 2.0 ** -120)


def test_refusals_leave_outputs_and_context_alone(built, tmp_path_factory):
    import torch

    scene, r = scene_of(tmp_path_factory, "zoo")
    nb, n = scene.desc.num_bsdfs, 100
    shape = shapes_for(scene, "miss3", n, 2)
    rec, wi, wo, gout = inputs(scene, shape, 2)
    good = r.bsdf_grad(rec, wi, wo, gout)
    lib = nori_amd.lib()
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    gm = np.full((nb, 16), 3.0, f32)

    def call(gd, *ptrs):
        return lib.nori_gpu_bsdf_grad(r._h, C.byref(gd), *ptrs, None)

    gd = _abi.BsdfGradDesc(n, 0)
    gd.reserved[1] = 1
    assert call(gd, ptr(rec), ptr(wi), ptr(wo), ptr(gout), ptr(gm), None) == _abi.NORI_ERR_INVALID
    gd = _abi.BsdfGradDesc(n, 0)
    assert call(gd, None, ptr(wi), ptr(wo), ptr(gout), ptr(gm), None) == _abi.NORI_ERR_INVALID
    bad = rec.copy()
    bad["shape"][5] = scene.desc.num_shapes
    assert call(gd, ptr(bad), ptr(wi), ptr(wo), ptr(gout), ptr(gm), None) == _abi.NORI_ERR_INVALID
    bad["shape"][5] = -2
    assert call(gd, ptr(bad), ptr(wi), ptr(wo), ptr(gout), ptr(gm), None) == _abi.NORI_ERR_INVALID
    # device form: a host pointer, a misaligned pointer
    d = [torch.from_numpy(a.view(f32).reshape(n, -1) if a.dtype == nori_amd.SURFACE_DTYPE else a).cuda()
         for a in (rec, wi, wo, gout)]
    dgm = torch.full((nb, 16), 3.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    gd = _abi.BsdfGradDesc(n, 1)
    dp = [C.c_void_p(t.data_ptr()) for t in d]
    assert call(gd, dp[0], dp[1], dp[2], ptr(gout), C.c_void_p(dgm.data_ptr()), None) == _abi.NORI_ERR_INVALID
    assert call(gd, C.c_void_p(d[0].data_ptr() + 4), dp[1], dp[2], dp[3], C.c_void_p(dgm.data_ptr()), None) == _abi.NORI_ERR_INVALID
    assert call(gd, dp[0], dp[1], dp[2], dp[3], C.c_void_p(dgm.data_ptr() + 4), None) == _abi.NORI_ERR_INVALID
    assert np.all(gm == 3.0) and bool((dgm == 3.0).all())
    again = r.bsdf_grad(rec, wi, wo, gout)
    assert np.array_equal(good.view(np.uint32), again.view(np.uint32))
