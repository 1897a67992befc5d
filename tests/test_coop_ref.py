"""tests/coop_ref.py, the numpy reference the GPU tests of the tail finisher
compare the device against (tests/test_gpu_finish_tail.py), pinned on the CPU
to what the project already trusts, on a real scan-mode scene (pa4 cbox, its
own scan list: axis-plane pairs, padding records, two spheres):

* ray against one record: the reference equals nori_test_util.prim_hit (the
  independent statement of mesh.cpp:83-120 / sphere.cpp:43-76 on the scene's
  vertices) bit for bit -- hit, t, u, v;
* the scan rule (root box, adaptive epsilon, closest t, the later leaf-order
  position among equal t) over all the scene's records passes
  test_gpu_parity._compare_hits against the oracle's BVH walk
  (pyoracle.OracleScene.trace), closest and any-hit;
* the plane form (test_plane_cull.moller_trumbore_plane, reused by the
  reference) and the generic form agree on the scene's axis-plane records;
* box_test's reference against a plain per-ray statement of
  BoundingBox3f::rayIntersect."""
import numpy as np
import pytest

import coop_ref as R
import nori_amd
import pyoracle
from conftest import scene_path
from nori_test_util import prim_hit
from test_gpu_parity import _compare_hits, _rays

f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _edge_rays(rec, rng, per_edge):
    """Rays from well inside the box through points on the triangles' edges
    (a few on their corners): the diagonal two triangles of a wall share is
    hit by both, often at the same t.  The origins stay away from the walls'
    planes: a ray grazing a wall into its corner can pass the triangle test
    and miss an inner box of the oracle's BVH by a rounding, which is a
    property of that walk, not of the scan rule pinned here."""
    pts = []
    for r in rec[R.is_triangle(rec) & (rec.view(np.uint32)[:, 3] != R.NO_PRIM)]:
        v0, e1, e2 = r[0:3].astype(np.float64), r[4:7].astype(np.float64), r[8:11].astype(np.float64)
        V = [v0, v0 + e1, v0 + e2]
        for i in range(3):
            a, b = V[i], V[(i + 1) % 3]
            p = a + rng.random(per_edge)[:, None] * (b - a)
            p[:4] = a
            pts.append(p)
    p = np.concatenate(pts)
    o = rng.uniform([-0.6, 0.3, -0.6], [0.6, 1.2, 0.6], size=p.shape)
    d = p - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((len(p), 8), f32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, 1e-4, d, np.inf
    return rays


@pytest.fixture(scope="module")
def cbox(built):
    s = nori_amd.load_scene(scene_path("pa4", "cbox", "cbox_path_mis.xml"), 32, 32, 1)
    rec = nori_amd.scan_list(s)["records"]
    box = nori_amd.bvh_refit(s)[2]
    rays = np.concatenate([_rays(6000, 21, [-0.9, 0.05, -0.9], [0.9, 1.5, 0.9]),
                           _rays(3000, 22, [-3, -1, -3], [3, 3, 6], mint=0.01)])
    return s, rec, box, np.concatenate([rays, _edge_rays(rec, np.random.default_rng(3), 160)])


def test_scan_list_shape(cbox):
    """The layout the reference assumes: triangles (w of e1 zero), padding
    records with id 0xFFFFFFFF and zero edges, spheres last; positions are a
    permutation of the leaf order."""
    _, rec, _, _ = cbox
    w = rec.view(np.uint32)
    tri = R.is_triangle(rec)
    pad = w[:, 3] == R.NO_PRIM
    assert 0 < len(rec) <= 64 and pad.any() and (~tri).sum() == 2
    assert tri[pad].all() and not rec[pad][:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].any()
    assert not tri[-2:].any()
    real = ~pad
    assert sorted(w[real, 11]) == list(range(real.sum()))
    assert len(set(w[real, 3])) == real.sum()


def test_record_tests_equal_prim_hit(cbox):
    s, rec, _, rays = cbox
    grown = R.grow_mint(rays)  # prim_hit grows mint == kEps itself
    ids = rec.view(np.uint32)[:, 3]
    hits = 0
    for p in np.flatnonzero(ids != R.NO_PRIM):
        r = np.broadcast_to(rec[p], (len(rays), 12))
        h0, t0, u0, v0 = prim_hit(s, rays, np.full(len(rays), ids[p]))
        if R.is_triangle(rec[p:p + 1])[0]:
            h, t, u, v = R.tri(r, grown)
            assert np.array_equal(_bits(u), _bits(u0)) and np.array_equal(_bits(v), _bits(v0)), p
        else:
            h, t = R.sphere(r, grown)[:2]
        assert np.array_equal(h, h0), p
        assert np.array_equal(_bits(t[h]), _bits(t0[h])), p
        hits += int(h.sum())
    assert hits > len(rays) // 2


def test_padding_record_never_hits(cbox):
    _, _, _, rays = cbox
    h = R.tri(np.broadcast_to(R.padding_records(1)[0], (len(rays), 12)), rays)[0]
    assert not h.any()


def _as_hits(out):
    g = np.zeros(len(out["t"]), np.dtype([("t", "<f4"), ("prim", "<i4"), ("u", "<f4"), ("v", "<f4")]))
    g["t"], g["prim"], g["u"], g["v"] = out["t"], out["prim"].view(np.int32), out["u"], out["v"]
    return g


def test_scan_rule_matches_oracle(cbox):
    s, rec, box, rays = cbox
    o = pyoracle.OracleScene(s)
    out = R.scan(rec, box[:3], box[3:], rays)
    c = o.trace(rays)
    ties = _compare_hits(_as_hits(out), c, s, rays)
    assert np.array_equal(out["res"], np.isfinite(c["t"]))
    # the tie rule is the oracle's: not one id differs, and ties do occur (shared edges)
    assert ties == 0 and out["ties"].sum() > 50, (ties, out["ties"].sum())
    assert (~out["live"]).sum() > 100  # rays that miss the root box are among them
    shadow = R.scan(rec, box[:3], box[3:], rays, any_hit=True)
    assert np.array_equal(shadow["res"], np.isfinite(o.trace(rays, any_hit=True)["t"]))
    assert np.array_equal(shadow["res"], out["res"])
    assert np.isinf(shadow["t"]).all() and (shadow["prim"] == R.NO_PRIM).all()


def test_scan_wanting_lanes_only(cbox):
    _, rec, box, rays = cbox
    want = np.arange(len(rays)) % 3 == 0
    full = R.scan(rec, box[:3], box[3:], rays)
    part = R.scan(rec, box[:3], box[3:], rays, want)
    for k in ("res", "t", "prim", "u", "v"):
        assert np.array_equal(_bits(part[k][want]) if part[k].dtype == f32 else part[k][want],
                              _bits(full[k][want]) if full[k].dtype == f32 else full[k][want]), k
    off = ~want
    assert not part["res"][off].any() and np.isinf(part["t"][off]).all() and (part["prim"][off] == R.NO_PRIM).all()
    assert not part["u"][off].any() and not part["v"][off].any()


def test_plane_form_is_generic_form(cbox):
    """On the scan list's axis-plane records the two numpy forms accept the
    same rays with the same t bits and u, v equal as values."""
    _, rec, _, rays = cbox
    grown = R.grow_mint(rays)
    checked = 0
    for p in np.flatnonzero(R.is_triangle(rec) & (rec.view(np.uint32)[:, 3] != R.NO_PRIM)):
        for A in range(3):
            if rec[p, 4 + A] != 0 or rec[p, 8 + A] != 0:
                continue
            r = np.broadcast_to(rec[p], (len(rays), 12))
            h, t, u, v = R.tri(r, grown)
            hp, tp, up, vp = R.tri_plane(r, grown, A)
            assert np.array_equal(h, hp) and np.array_equal(_bits(t[h]), _bits(tp[h]))
            assert np.array_equal(u[h], up[h]) and np.array_equal(v[h], vp[h])
            checked += int(h.sum())
    assert checked > 1000


def _ray_box_plain(mn, mx, o, d, mint, maxt):
    """BoundingBox3f::rayIntersect (bbox.h:336-363) for one ray, in float32."""
    near, far = f32(-np.inf), f32(np.inf)
    with np.errstate(all="ignore"):
        for i in range(3):
            if d[i] == 0:
                if o[i] < mn[i] or o[i] > mx[i]:
                    return False
            else:
                rcp = f32(1) / d[i]
                t1, t2 = (mn[i] - o[i]) * rcp, (mx[i] - o[i]) * rcp
                if t1 > t2:
                    t1, t2 = t2, t1
                near = near if t1 < near else t1  # std::max(t1, nearT)
                far = far if far < t2 else t2  # std::min(t2, farT)
                if not near <= far:
                    return False
    return bool(mint <= far and near <= maxt)


def test_box_reference_against_plain_statement():
    rng = np.random.default_rng(5)
    n = 4000
    rays = _rays(n, 23, [-2, -2, -2], [2, 2, 2], mint=0.0, axis_aligned=0.4)
    rays[: n // 4, 0:3] = rng.choice([-1.0, 0.0, 1.0, 0.5], (n // 4, 3))  # origins on faces and edges
    rays[:, 7] = np.where(rng.random(n) < 0.3, rng.uniform(0, 3, n), np.inf)
    mn, mx = np.full(3, -1, f32), np.array([1, 1, -1], f32)  # degenerate in z
    for lo, hi in ((np.full(3, -1, f32), np.full(3, 1, f32)), (mn, mx)):
        ok, _ = R.box(lo, hi, rays)
        want = [_ray_box_plain(lo, hi, r[0:3], r[4:7], r[3], r[7]) for r in rays]
        assert np.array_equal(ok, np.array(want))
        assert 0.05 < ok.mean() < 0.95


def test_finish_tail_inputs_are_not_vacuous():
    """The inputs of tests/test_gpu_finish_tail.py reach, on the reference
    alone, the shares that file requires before it asserts a device result."""
    import finish_tail_inputs as I

    for case in I.coop_cases():
        I.check_coop_case(case)
    rec, rays = I.sphere_rows(np.random.default_rng(31), 1 << 17)
    hit, _, normal, aux = R.sphere(rec, rays)
    I.check_sphere_rows(rays, hit, normal, aux)
    for G in (1, 3, 257, 1025):
        for _, cnt in I.count_vectors(G, np.random.default_rng(G)):
            pre = np.concatenate([[0], np.cumsum(cnt.astype(np.uint64))]).astype(np.uint32)
            gids = I.lookup_gids(pre, np.random.default_rng(1))
            assert gids.size == min(int(pre[-1]), gids.size) and (gids < max(1, pre[-1])).all()
