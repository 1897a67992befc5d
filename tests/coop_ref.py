"""numpy reference of the scan's primitive tests on raw records (scan.h:
tri_hit / tri_hit_nb, tri_hit_plane<A>, sphere_hit / sphere_hit_nb /
sphere_hit_fast, box_test) and of the finisher's cooperative scan
(coop_scan.h), for tests/test_gpu_finish_tail.py.  Pinned on the CPU against
nori_test_util.prim_hit and the oracle by tests/test_coop_ref.py.

Arithmetic: float32 arrays throughout, so every +, -, *, / and sqrt is
rounded once to fp32 (numpy rounds like the GPU's IEEE operations), nothing is
fused, dot = (a0 b0 + a1 b1) + a2 b2 and cross as device_math.h states them.

Records are the upload's (scene_prep.cpp build_scan_list, dev_scene.h), three
float4 (12 floats, ids and positions as raw uint32 bits):
  triangle  (v0, id), (e1, 0), (e2, leaf-order position)
  sphere    (centre, id), (radius, ., ., non-zero w), (., ., ., position)
  padding   (0, 0, 0, 0xFFFFFFFF), 0, 0: a triangle with zero edges, never hit
Rays are (o, mint, d, maxt), 8 floats."""
import numpy as np

from test_plane_cull import moller_trumbore_plane

f32 = np.float32
EPS = f32(1e-4)  # kEps
NO_PRIM = np.uint32(0xFFFFFFFF)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _cols(a, k):
    return (a[:, k], a[:, k + 1], a[:, k + 2])


def _rays(rays):
    rays = np.ascontiguousarray(rays, f32).reshape(-1, 8)
    return _cols(rays, 0), _cols(rays, 4), rays[:, 3], rays[:, 7]


def _recs(records):
    return np.ascontiguousarray(records, f32).reshape(-1, 12)


def make_records(p0, p1, p2, ids, pos, sphere=False):
    """(n, 12) records from three (n, 3) float arrays, the ids (p0.w) and the
    leaf-order positions (p2.w); sphere: p1 = (radius, 0, 0) with w = 1 (bits)."""
    n = len(p0)
    r = np.zeros((n, 12), f32)
    r[:, 0:3], r[:, 4:7], r[:, 8:11] = p0, p1, p2
    w = r.view(np.uint32)
    w[:, 3], w[:, 11] = ids, pos
    w[:, 7] = 1 if sphere else 0
    return r


def padding_records(n):
    r = np.zeros((n, 12), f32)
    r.view(np.uint32)[:, 3] = NO_PRIM
    return r


def is_triangle(records):
    return _recs(records).view(np.uint32)[:, 7] == 0


def tri(records, rays):
    """tri_hit_nb (and, on the hit rows, tri_hit): ray i against record i -> hit, t, u, v."""
    rec = _recs(records)
    o, d, mint, maxt = _rays(rays)
    p0, e1, e2 = _cols(rec, 0), _cols(rec, 4), _cols(rec, 8)
    with np.errstate(all="ignore"):
        pvec = _cross(d, e2)
        det = _dot(e1, pvec)
        inv = f32(1) / det
        tvec = (o[0] - p0[0], o[1] - p0[1], o[2] - p0[2])
        u = _dot(tvec, pvec) * inv
        qvec = _cross(tvec, e1)
        v = _dot(d, qvec) * inv
        t = _dot(e2, qvec) * inv
        hit = (~((det > f32(-1e-8)) & (det < f32(1e-8))) & ~((u < 0) | (u > 1)) & ~((v < 0) | (u + v > 1)) &
               (t >= mint) & (t <= maxt))
    return hit, t, u, v


def tri_plane(records, rays, A):
    """tri_hit_plane<A> (test_plane_cull.moller_trumbore_plane): ray i against record i."""
    rec = _recs(records)
    o, d, mint, maxt = _rays(rays)
    return moller_trumbore_plane(_cols(rec, 0), _cols(rec, 4), _cols(rec, 8), o, d, mint, maxt, A)


def sphere(records, rays):
    """sphere_hit / sphere_hit_nb: ray i against record i -> hit, t, normal, aux.
    t is t1 where t1 is in [mint, maxt], else t2 (the device's value on every
    row).  normal: no intermediate of the row is subnormal (each is zero,
    normal, inf or NaN).  aux: dict of disc, y = 2A, x1 = -B - delta, x2 = -B +
    delta, t1, t2 (the quantities sphere_hit_fast gates on)."""
    rec = _recs(records)
    o, d, mint, maxt = _rays(rays)
    c, rad = _cols(rec, 0), rec[:, 4]
    tiny = np.finfo(f32).tiny
    sub = np.zeros(len(rec), bool)

    def T(x):  # track subnormal intermediates
        nonlocal sub
        sub |= (x != 0) & (np.abs(x) < tiny)
        return x

    def dot(a, b):
        return T(T(T(a[0] * b[0]) + T(a[1] * b[1])) + T(a[2] * b[2]))

    with np.errstate(all="ignore"):
        oc = (T(o[0] - c[0]), T(o[1] - c[1]), T(o[2] - c[2]))
        A = dot(d, d)
        B = T(f32(2) * dot(oc, d))
        C = T(dot(oc, oc) - T(rad * rad))
        disc = T(T(B * B) - T(T(f32(4) * A) * C))
        delta = T(np.sqrt(disc))
        y = T(f32(2) * A)
        x1, x2 = T(-B - delta), T(-B + delta)
        t1, t2 = T(x1 / y), T(x2 / y)
        h1 = (mint <= t1) & (t1 <= maxt)
        h2 = (mint <= t2) & (t2 <= maxt)
        hit = (disc > 0) & (h1 | h2)
    return hit, np.where(h1, t1, t2), ~sub, {"disc": disc, "y": y, "x1": x1, "x2": x2, "t1": t1, "t2": t2}


def _smax(a, b):  # device_math.h: std::max, (a < b) ? b : a
    return np.where(a < b, b, a)


def _smin(a, b):  # std::min, (b < a) ? b : a
    return np.where(b < a, b, a)


def box(mn, mx, rays):
    """box_test with rcp = 1 / d (rcp_full): (ok, tnear).  mn, mx: (n, 3) or (3,)."""
    o, d, mint, maxt = _rays(rays)
    n = len(mint)
    mn = np.broadcast_to(np.asarray(mn, f32), (n, 3))
    mx = np.broadcast_to(np.asarray(mx, f32), (n, 3))
    ok = np.ones(n, bool)
    near, far = np.full(n, -np.inf, f32), np.full(n, np.inf, f32)
    with np.errstate(all="ignore"):
        for k in range(3):
            rcp = f32(1) / d[k]
            t1, t2 = (mn[:, k] - o[k]) * rcp, (mx[:, k] - o[k]) * rcp
            lo, hi = np.where(t1 > t2, t2, t1), np.where(t1 > t2, t1, t2)
            zero = d[k] == 0
            n2, f2 = _smax(lo, near), _smin(hi, far)
            ok &= np.where(zero, ~((o[k] < mn[:, k]) | (o[k] > mx[:, k])), n2 <= f2)
            near, far = np.where(zero, near, n2), np.where(zero, far, f2)
        return ok & (mint <= far) & (near <= maxt), near


def grow_mint(rays):
    """The scans' adaptive epsilon: a ray with mint == kEps gets
    max(mint, mint * max|o_i|).  Returns a copy of the rays."""
    rays = np.array(rays, f32).reshape(-1, 8)
    m = rays[:, 3] == EPS
    with np.errstate(all="ignore"):
        big = _smax(_smax(np.abs(rays[m, 0]), np.abs(rays[m, 1])), np.abs(rays[m, 2]))
        rays[m, 3] = _smax(rays[m, 3], rays[m, 3] * big)
    return rays


def record_hits(records, rays):
    """Every ray against every record, mint / maxt as given: hit (n, P) bool,
    t, u, v (n, P) float32 (u = v = 0 for spheres)."""
    rec = _recs(records)
    rays = np.ascontiguousarray(rays, f32).reshape(-1, 8)
    n, P = len(rays), len(rec)
    hit = np.zeros((n, P), bool)
    t, u, v = (np.zeros((n, P), f32) for _ in range(3))
    triangle = is_triangle(rec)
    for p in range(P):
        r = np.broadcast_to(rec[p], (n, 12))
        if triangle[p]:
            hit[:, p], t[:, p], u[:, p], v[:, p] = tri(r, rays)
        else:
            hit[:, p], t[:, p] = sphere(r, rays)[:2]
    return hit, t, u, v


def scan(records, root_min, root_max, rays, want=None, any_hit=False):
    """coop_scan<any_hit> over the records for the rays of the wanting lanes:
    a dict of res (bool), t, prim (uint32), u, v per ray, and for the tests'
    own statistics live (the ray passes maxt >= mint and the root box), hits
    (n, P) and ties (the closest t is shared by more than one record).

    live = !(maxt < mint) and box_test(root), after the mint == kEps growth;
    the closest t over the hitting records wins, among bit-equal t the
    largest leaf-order position; any_hit returns live and any hit, with the
    defaults in t, prim, u, v.  A lane that does not want a ray returns
    (false, inf, 0xFFFFFFFF, 0, 0)."""
    rec = _recs(records)
    rays = grow_mint(rays)
    n = len(rays)
    want = np.ones(n, bool) if want is None else np.asarray(want, bool)
    ids, pos = rec.view(np.uint32)[:, 3], rec.view(np.uint32)[:, 11]
    with np.errstate(all="ignore"):
        live = ~(rays[:, 7] < rays[:, 3]) & box(root_min, root_max, rays)[0]
    hit, t, u, v = record_hits(rec, rays)
    hit &= live[:, None]
    res = hit.any(axis=1) & want
    out = {"res": res, "t": np.full(n, np.inf, f32), "prim": np.full(n, NO_PRIM, np.uint32), "u": np.zeros(n, f32),
           "v": np.zeros(n, f32), "live": live, "hits": hit, "ties": np.zeros(n, bool)}
    if any_hit or not len(rec):
        return out
    # accepted t are > 0 or +-0 with mint <= 0; t + 0.0f (the device's key) makes -0 a +0
    tk = np.where(hit, t + f32(0), f32(np.inf))
    tmin = tk.min(axis=1)
    cand = hit & (tk.view(np.uint32) == tmin.view(np.uint32)[:, None])
    key = np.where(cand, pos[None, :].astype(np.int64), -1)
    w = key.argmax(axis=1)
    # equal positions among candidates: the later lane wins (`pos >= best_pos`)
    top = key == key.max(axis=1, keepdims=True)
    w = np.where(top.sum(axis=1) > 1, key.shape[1] - 1 - top[:, ::-1].argmax(axis=1), w)
    rows = np.arange(n)
    out["t"][res] = tmin[res]
    out["prim"][res] = ids[w][res]
    out["u"][res] = u[rows, w][res]
    out["v"][res] = v[rows, w][res]
    out["ties"] = res & (cand.sum(axis=1) > 1)
    return out
