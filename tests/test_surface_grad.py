"""The hit record's adjoint in the vertices, host side: nori_scene_surface_grad (its statement is in
include/nori_gpu.h) against the numpy restatement of tests/surface_grad_ref.py.  Hits are
synthetic (a primitive, barycentrics, a direction and a distance; o = p - t d), so no tracer runs.
tests/test_gpu_surface_grad.py checks the kernel against this host function.

1. the terms bit for bit; 2. central differences of the float64 forward; 3. the adjoint identity
over a whole call; 4. accumulation; 5. zero contributions and payloads; 6. refusals; 7. positions /
normals given against a scene loaded with them.

The finite-difference figures.  Per hit, with a random record gradient g and random vertex
directions dP, dN: e = |fd - <terms, d>| / sum |terms| |d|, fd the central difference of
<g, forward64> at h = 1e-5 in float64.  The terms are fp32 (relative rounding 2^-24 = 6e-8 per
operation, a dozen operations deep, with cancellation in the projections), the difference
quotient is float64 with an O(h^2) truncation, so e is a small multiple of 1e-6 at best.  Observed
(this file's print, max over the hits): hf 2.05e-05, smooth 4.84e-06, cbox 8.12e-07, nmap 7.73e-06
(medians 3e-08 .. 2e-07); whole-call identity 6.4e-10 .. 4.2e-08.  Cap: 2e-4, an order of
magnitude above the largest; a wrong or missing term shows as O(1)."""
import ctypes as C

import numpy as np
import pytest

import nori_amd
import refit_util as U
import surface_grad_ref as G
from conftest import scene_path
from nori_amd import _abi

f32 = np.float32
FD_CAP = 2e-4
NMAP = ("project", "textured", "cbox_normalmap_normals.xml")
SCENES = ("hf", "smooth", "cbox", "nmap")
_CACHE = {}


def scene_of(tmp_path_factory, which):
    if which not in _CACHE:
        d = str(tmp_path_factory.mktemp(f"sgrad_{which}"))
        if which == "smooth":
            s = nori_amd.load_scene(G.smooth_scene_xml(d))
        elif which == "nmap":
            s = nori_amd.load_scene(scene_path(*NMAP), 32, 32, 1)
        else:
            s = U.load(which, d)
        _CACHE[which] = (s, G.Tables(s), d)
    return _CACHE[which]


def mixed_prims(tab, n, seed, misses=True):
    """n primitive ids over every triangle class of the scene, with spheres and misses between."""
    g = np.random.default_rng(seed)
    prims = g.choice(tab.triangles, n)
    sph = np.nonzero(tab.sphere)[0]
    if len(sph):
        prims[3::11] = g.choice(sph, len(prims[3::11]))
    if misses:
        prims[5::13] = -1
    return prims


def call(scene, rays, hits, grad, positions=None, normals=None):
    return nori_amd.surface_grad(scene, rays, hits, grad, positions, normals, with_terms=True)


@pytest.mark.parametrize("which", SCENES)
def test_terms_equal_the_float32_restatement(built, tmp_path_factory, which):
    s, tab, _ = scene_of(tmp_path_factory, which)
    P, Nv = s.positions(), s.normals()
    prims = mixed_prims(tab, 3000, 1)
    rays, hits = G.synthetic_hits(tab, P, prims, 2)
    grad = G.random_grad(len(hits), 3)
    gp, gn, terms = call(s, rays, hits, grad)
    want = G.terms32(tab, P, Nv, rays, hits, grad)
    assert terms.shape == (3000, 18) and np.isfinite(terms).all()
    assert np.array_equal(G.bits(terms), G.bits(want))
    live = want[:, :9].any(1)
    assert live.sum() > 2000 and not terms[hits["prim"] < 0].any()
    if which in ("smooth", "nmap"):
        assert want[:, 9:].any(1).sum() > 300
    if which == "nmap":  # mapped and unmapped meshes with normals both occur
        k = np.where(hits["prim"] < 0, 0, hits["prim"])
        assert (tab.mapped[k] & live).sum() > 100 and (tab.has_normals[k] & ~tab.mapped[k] & live).sum() > 100
    # the sums: float64 per destination, rounded once
    refp, refn = G.sums(tab, hits, want)
    assert np.array_equal(G.bits(gp), G.bits(refp["S"].astype(f32)))
    assert np.array_equal(G.bits(gn), G.bits(refn["S"].astype(f32)))


def _fd(tab, P, Nv, rays, hits, grad, dP, dN, h=1e-5):
    g = grad.astype(np.float64)
    g[:, [7, 11, 12, 13, 14, 15]] = 0
    P, Nv = P.astype(np.float64), Nv.astype(np.float64)
    plus = G.forward64(tab, P + h * dP, Nv + h * dN, rays, hits)
    minus = G.forward64(tab, P - h * dP, Nv - h * dN, rays, hits)
    return (g * (plus - minus)).sum(1) / (2 * h)


def _pairing(tab, hits, terms, dP, dN):
    """Per hit: <terms, direction> and sum |terms| |direction| in float64."""
    k = np.where(hits["prim"] < 0, 0, hits["prim"]).astype(np.int64)
    f = tab.vid[k]
    t = terms.astype(np.float64)
    d = np.concatenate([dP[f[:, 0]], dP[f[:, 1]], dP[f[:, 2]], dN[f[:, 0]], dN[f[:, 1]], dN[f[:, 2]]], 1)
    return (t * d).sum(1), (np.abs(t) * np.abs(d)).sum(1)


@pytest.mark.parametrize("which", SCENES)
def test_central_differences_and_adjoint_identity(built, tmp_path_factory, which):
    s, tab, _ = scene_of(tmp_path_factory, which)
    P, Nv = s.positions(), s.normals()
    rng = np.random.default_rng(11)
    prims = mixed_prims(tab, 2000, 4)
    rays, hits = G.synthetic_hits(tab, P, prims, 5)
    grad = G.random_grad(len(hits), 6)
    scale = float(np.abs(P).max())
    dP = rng.standard_normal(P.shape) * scale
    dN = rng.standard_normal(P.shape)
    gp, gn, terms = call(s, rays, hits, grad)
    fd = _fd(tab, P, Nv, rays, hits, grad, dP, dN)
    an, mag = _pairing(tab, hits, terms, dP, dN)
    live = mag > 0
    assert live.sum() > 1500 and not fd[~live].any()
    e = np.abs(fd - an)[live] / mag[live]
    # the whole call: <grad_surf, J d> = <grad_positions, dP> + <grad_normals, dN>
    lhs = fd.sum()
    rhs = (gp.astype(np.float64) * dP).sum() + (gn.astype(np.float64) * dN).sum()
    whole = abs(lhs - rhs) / mag.sum()
    print(f"{which}: per-hit finite-difference error max {e.max():.2e} median {np.median(e):.2e}; "
          f"adjoint identity |lhs - rhs| / sum|terms||d| = {whole:.2e} (cap {FD_CAP:g})")
    assert e.max() <= FD_CAP
    assert whole <= FD_CAP


def test_outputs_are_added_into(built, tmp_path_factory):
    s, tab, _ = scene_of(tmp_path_factory, "smooth")
    V = s.desc.num_vertices
    rays, hits = G.synthetic_hits(tab, s.positions(), mixed_prims(tab, 800, 7), 8)
    g1, g2 = G.random_grad(800, 9), G.random_grad(800, 10)
    lib = nori_amd.lib()
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731

    def raw(grad, gp, gn):
        assert lib.nori_scene_surface_grad(s.desc_ptr, None, None, 800, p(rays), p(hits), p(grad), p(gp), p(gn), None) == 0

    a_p, a_n, _ = call(s, rays, hits, g1)
    b_p, b_n, _ = call(s, rays, hits, g2)
    gp, gn = np.zeros((V, 3), f32), np.zeros((V, 3), f32)
    raw(g1, gp, gn)
    assert np.array_equal(G.bits(gp), G.bits(a_p)) and np.array_equal(G.bits(gn), G.bits(a_n)) and gn.any()
    raw(g2, gp, gn)
    # the second call's float64 sum lands on the first's value and is rounded once
    t2 = G.terms32(tab, s.positions(), s.normals(), rays, hits, g2)
    rp, rn = G.sums(tab, hits, t2)
    assert np.array_equal(G.bits(gp), G.bits((a_p.astype(np.float64) + rp["S"]).astype(f32)))
    assert np.array_equal(G.bits(gn), G.bits((a_n.astype(np.float64) + rn["S"]).astype(f32)))
    assert np.abs(gp - (a_p + b_p)).max() <= 1e-5 * np.abs(gp).max()
    # a destination without a term is not touched
    marked = np.full((V, 3), 7, f32)
    raw(g1, marked, None)
    assert (marked[rp["m"] == 0] == 7).all() and (rp["m"] == 0).any()
    # grad_normals = NULL: the positions' result is the same bits
    only = np.zeros((V, 3), f32)
    raw(g1, only, None)
    assert np.array_equal(G.bits(only), G.bits(a_p))


def test_zero_contributions_and_payloads(built, tmp_path_factory):
    # degenerate triangles, misses: exactly zero, no NaN
    s, tab, _ = scene_of(tmp_path_factory, "hf")
    Q = U.position_set(s, "d")
    fv = tab.vid[tab.triangles]
    same = (Q[fv[:, 0]] == Q[fv[:, 1]]).all(1) & (Q[fv[:, 0]] == Q[fv[:, 2]]).all(1)
    collapsed = tab.triangles[same]  # (every tenth, less the few that a -0.0 coordinate reopened)
    assert len(collapsed) >= 300
    prims = np.concatenate([collapsed[:300], tab.triangles[~same][1:301], np.full(50, -1)])
    rays, hits = G.synthetic_hits(tab, Q, prims, 12)
    grad = G.random_grad(len(hits), 13)
    gp, gn, terms = call(s, rays, hits, grad, positions=Q)
    assert np.isfinite(terms).all() and np.isfinite(gp).all() and not gn.any()
    f = tab.vid[collapsed[:300]]
    assert (Q[f[:, 0]] == Q[f[:, 1]]).all() and (Q[f[:, 0]] == Q[f[:, 2]]).all()
    # (a neighbour of a collapsed triangle that shares two of its vertices has |N| = 0 as well)
    assert not terms[:300].any() and not terms[600:].any() and terms[300:600].any(1).sum() > 150
    assert np.array_equal(G.bits(terms), G.bits(G.terms32(tab, Q, s.normals(), rays, hits, grad)))
    # spheres among the meshes
    s, tab, _ = scene_of(tmp_path_factory, "cbox")
    prims = np.resize(np.concatenate([np.nonzero(tab.sphere)[0], tab.triangles[:4], [-1]]), 700)
    rays, hits = G.synthetic_hits(tab, s.positions(), prims, 14)
    grad = G.random_grad(700, 15)
    gp, gn, terms = call(s, rays, hits, grad)
    k = np.where(prims < 0, 0, prims)
    assert not terms[tab.sphere[k] | (prims < 0)].any() and terms[~tab.sphere[k] & (prims >= 0)].any(1).all()
    # NaN payloads in the ignored words change nothing
    nan = grad.copy()
    nan.view(np.uint32)[:, [7, 11, 12, 13, 14, 15]] = G.random_grad(700, 16, nan_payload=True).view(np.uint32)[:, [7, 11, 12, 13, 14, 15]]
    assert np.isnan(nan[:, 7]).all()
    gp2, gn2, terms2 = call(s, rays, hits, nan)
    assert np.array_equal(G.bits(terms2), G.bits(terms)) and np.array_equal(G.bits(gp2), G.bits(gp))
    # a structured gradient array is the same call
    gp3, _, _ = call(s, rays, hits, nan.view(nori_amd.SURFACE_DTYPE).reshape(-1))
    assert np.array_equal(G.bits(gp3), G.bits(gp))
    # a normal-mapped shape: g_ns contributes nothing, g_p, g_t, g_ng still do
    s, tab, _ = scene_of(tmp_path_factory, "nmap")
    mapped = np.nonzero(tab.mapped)[0]
    assert len(mapped) > 100
    rays, hits = G.synthetic_hits(tab, s.positions(), mapped[:500], 17)
    grad = G.random_grad(500, 18)
    _, gn, terms = call(s, rays, hits, grad)
    assert not gn.any() and not terms[:, 9:].any()
    only_ns = np.zeros_like(grad)
    only_ns[:, 8:11] = grad[:, 8:11]
    gp, gn, t_ns = call(s, rays, hits, only_ns)
    assert not t_ns.any() and not gp.any() and not gn.any()
    for cols in (slice(0, 3), slice(3, 4), slice(4, 7)):
        one = np.zeros_like(grad)
        one[:, cols] = grad[:, cols]
        assert call(s, rays, hits, one)[2][:, :9].any(1).all(), cols


def test_refusals(built, tmp_path_factory):
    s, tab, d = scene_of(tmp_path_factory, "smooth")
    V = s.desc.num_vertices
    n = 64
    rays, hits = G.synthetic_hits(tab, s.positions(), tab.triangles[:n], 19)
    grad = G.random_grad(n, 20)
    gp, gn, terms = np.full((V, 3), 5, f32), np.full((V, 3), 5, f32), np.full((n, 18), 5, f32)
    f = nori_amd.lib().nori_scene_surface_grad
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    good = [s.desc_ptr, None, None, n, p(rays), p(hits), p(grad), p(gp), p(gn), p(terms)]

    def untouched():
        return (gp == 5).all() and (gn == 5).all() and (terms == 5).all()

    for k in (0, 4, 5, 6, 7):
        a = list(good)
        a[k] = None
        assert f(*a) == _abi.NORI_ERR_INVALID and untouched(), k
    bad = hits.copy()
    bad["prim"][n - 1] = tab.num_prims
    a = list(good)
    a[5] = p(bad)
    assert f(*a) == _abi.NORI_ERR_INVALID and untouched()
    assert "outside the scene" in nori_amd.lib().nori_gpu_last_error().decode()
    for k, value in ((1, np.nan), (1, np.inf), (2, np.nan), (2, -np.inf)):
        arr = (s.positions() if k == 1 else s.normals()).copy()
        arr[V // 2, 1] = value  # (a vertex no hit of the batch uses: the arrays are checked whole)
        a = list(good)
        a[k] = p(arr)
        assert f(*a) == _abi.NORI_ERR_INVALID and untouched(), (k, value)
        assert "non-finite" in nori_amd.lib().nori_gpu_last_error().decode()
    a = list(good)
    a[3] = 0
    assert f(*a) == _abi.NORI_OK and untouched()  # n == 0
    assert f(*good) == _abi.NORI_OK and not untouched()
    with pytest.raises(ValueError):
        nori_amd.surface_grad(s, rays, hits, grad[:, :15])
    with pytest.raises(ValueError):
        nori_amd.surface_grad(s, rays, hits, grad, positions=s.positions()[:-1])


@pytest.mark.parametrize("which", ["hf", "smooth"])
def test_given_arrays_equal_a_scene_loaded_with_them(built, tmp_path_factory, which):
    s, tab, d = scene_of(tmp_path_factory, which)
    Q = U.position_set(s, "b")
    rng = np.random.default_rng(21)
    Nq = None
    if which == "smooth":
        Nq = s.normals() + 0.2 * rng.standard_normal(s.normals().shape).astype(f32)
        Nq = (Nq / np.linalg.norm(Nq, axis=1, keepdims=True)).astype(f32)
    rays, hits = G.synthetic_hits(tab, Q, mixed_prims(tab, 1500, 22), 23)
    grad = G.random_grad(1500, 24)
    got = call(s, rays, hits, grad, positions=Q, normals=Nq)
    if which == "smooth":
        other = nori_amd.load_scene(G.smooth_scene_xml(d))
        np.ctypeslib.as_array(other.desc.positions, shape=Q.shape)[:] = Q
        np.ctypeslib.as_array(other.desc.normals, shape=Q.shape)[:] = Nq
    else:
        other = U.load(which, d, Q)
    want = call(other, rays, hits, grad)
    for a, b in zip(got, want):
        assert np.array_equal(G.bits(a), G.bits(b))
    base = call(s, rays, hits, grad)
    assert not np.array_equal(G.bits(base[0]), G.bits(got[0]))
    assert np.array_equal(G.bits(got[2]), G.bits(G.terms32(tab, Q, s.normals() if Nq is None else Nq, rays, hits, grad)))
