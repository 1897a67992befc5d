"""Inputs of tests/test_gpu_finish_tail.py, numpy only, so that their coverage
(the shares of hits, misses, root-box rejections and resolved ties each set
must reach before a GPU result is asserted) is checked on the CPU as well
(tests/test_coop_ref.py): segment-count vectors for the prefix and the
lookup, record sets, rays and want masks for the cooperative scan, and the
rows of the primitive-form tests."""
import numpy as np

import coop_ref as R

f32, u32 = np.float32, np.uint32
KSEG = 256  # seg_index.h kSeg

# k_tail_prefix: per = 1, 2 and 17 segments per thread, threads with empty
# ranges, the last thread's range cut by G
PREFIX_GS = [1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 16384, 16385]
TOTALS = [1, 1023, 1024, 1025, 65535, 65536, 65537]  # both sides of the steps of K


def count_vectors(G, rng):
    """[(name, counts (G,) uint32)], each count <= kSeg: the vectors of
    tests/tail_index_check.cpp, and all-kSeg."""
    out = [("all zero", np.zeros(G, u32)), ("all kSeg", np.full(G, KSEG, u32))]
    for where in sorted({0, G // 2, G - 1}):
        for val in (1, int(rng.integers(1, KSEG + 1)), KSEG):
            c = np.zeros(G, u32)
            c[where] = val
            out.append((f"single {val} at {where}", c))
    for name in ("leading", "trailing", "interior"):
        c = rng.integers(1, KSEG + 1, G).astype(u32)
        ln = max(1, G // 3)
        b = 0 if name == "leading" else G - ln if name == "trailing" else (G - ln) // 2
        c[b:b + ln] = 0
        out.append((f"{name} zeros", c))
    out.append(("random sparse", np.where(rng.random(G) < 0.1, rng.integers(1, KSEG + 1, G), 0).astype(u32)))
    out.append(("random dense", rng.integers(0, KSEG + 1, G).astype(u32)))
    for T in TOTALS:
        if T > G * KSEG:
            continue
        c = np.zeros(G, u32)  # packed into a few segments, in random places
        order, left = rng.permutation(G), T
        for s in order:
            c[s] = min(KSEG, left)
            left -= int(c[s])
            if not left:
                break
        out.append((f"total {T} packed", c))
        c = np.full(G, T // G, u32)  # spread over all
        c[rng.permutation(G)[:T % G]] += 1
        out.append((f"total {T} spread", c))
    for _, c in out:
        assert c.dtype == u32 and c.shape == (G,) and c.max() <= KSEG
    return out


def lookup_gids(pre, rng):
    """Every gid in [0, n) when n <= 65536; otherwise every gid within 2 of a
    segment boundary and 4096 random ones."""
    n = int(pre[-1])
    if n <= 65536:
        return np.arange(n, dtype=u32)
    edge = (pre[:, None].astype(np.int64) + np.arange(-2, 3)[None, :]).ravel()
    g = np.concatenate([edge[(edge >= 0) & (edge < n)], rng.integers(0, n, 4096)])
    return np.unique(g).astype(u32)


# ---------------------------------------------------------------- record sets
def _ids_and_positions(rng, n):
    return 100 + rng.permutation(n), rng.permutation(n)  # positions not monotone in the lane


def triangles(rng, n, scale=1.0):
    v0 = rng.uniform(-1, 1, (n, 3))
    e1, e2 = rng.normal(size=(n, 3)) * 0.7, rng.normal(size=(n, 3)) * 0.7
    ids, pos = _ids_and_positions(rng, n)
    return R.make_records(v0 * scale, e1 * scale, e2 * scale, ids, pos)


def spheres(rng, n, scale=1.0):
    c = rng.uniform(-1, 1, (n, 3))
    p1 = np.zeros((n, 3))
    p1[:, 0] = rng.uniform(0.15, 0.5, n)
    ids, pos = _ids_and_positions(rng, n)
    return R.make_records(c * scale, p1 * scale, np.zeros((n, 3)), ids, pos, sphere=True)


def renumber(rng, rec):
    """Fresh distinct ids and positions for the real records of a stacked set."""
    real = np.flatnonzero(rec.view(u32)[:, 3] != R.NO_PRIM)
    ids, pos = _ids_and_positions(rng, len(real))
    rec.view(u32)[real, 3], rec.view(u32)[real, 11] = ids, pos
    return rec


def scan_shape(rng, tris, pad, sph, scale=1.0):
    """The scan list's own shape: triangles, padding records, then spheres."""
    return renumber(rng, np.concatenate([triangles(rng, tris, scale), R.padding_records(pad), spheres(rng, sph, scale)]))


def box_scene(rng):
    """A real scene's proportions: five walls of a box (axis-plane pairs of
    triangles, the front open), two spheres inside, in scan-list order."""
    recs = []
    for axis, side in ((0, -1), (0, 1), (1, -1), (1, 1), (2, 1)):
        b, c = (axis + 1) % 3, (axis + 2) % 3
        v0, v1 = np.full(3, -1.0), np.full(3, 1.0)
        v0[axis] = v1[axis] = side
        eb, ec = np.zeros(3), np.zeros(3)
        eb[b], ec[c] = 2, 2
        recs.append(R.make_records([v0, v1], [eb, -eb], [ec, -ec], [0, 0], [0, 0]))
    sp = R.make_records([[-0.4, -0.6, -0.3], [0.45, -0.55, 0.35]], [[0.4, 0, 0], [0.35, 0, 0]], np.zeros((2, 3)), [0, 0],
                        [0, 0], sphere=True)
    return renumber(rng, np.concatenate(recs + [R.padding_records(2), sp]))


TIE_LAYOUTS = {  # lane -> (id, leaf-order position) of the copies of the tied triangle
    3: {2: (50, 7), 5: (41, 12), 9: (3, 0)},
    4: {1: (50, 5), 4: (2, 0), 6: (49, 14), 11: (51, 9)},
    5: {0: (60, 3), 3: (1, 0), 7: (61, 15), 8: (62, 11), 12: (63, 6)},
    # Two copies share the largest position.  The upload never numbers two
    # records alike; the case is here because nothing else can see the
    # comparison's `>=` (the later lane of the two wins, not the earlier).
    "dup": {2: (50, 7), 5: (41, 12), 8: (3, 12), 11: (44, 0)},
}


def tie_set(rng, copies):
    """One triangle repeated `copies` times with distinct ids and positions:
    the winner (largest position) sits in neither the first nor the last of
    their lanes and has neither the lowest nor the highest id; position 0 is
    among them.  A nearer triangle covers part of it from one side, a farther
    one lies behind all of it; a few unrelated triangles fill the other lanes."""
    lay = TIE_LAYOUTS[copies]
    n = 14
    rec = triangles(rng, n) * f32(0.3)
    rec[:, 0:3] += f32(3)  # the fillers: small, off to one side
    w = rec.view(u32)
    w[:, 3], w[:, 11] = 200 + np.arange(n), 20 + rng.permutation(n)
    tied = R.make_records([[-1, -1, 0]], [[2, 0, 0]], [[0, 2, 0]], [0], [0])[0]
    for lane, (i, pos) in lay.items():
        rec[lane] = tied
        w[lane, 3], w[lane, 11] = i, pos
    free = [k for k in range(n) if k not in lay]
    rec[free[0]] = R.make_records([[-1, -1, -0.5]], [[1.2, 0, 0]], [[0, 1.2, 0]], [300], [40])[0]  # nearer from -z
    rec[free[1]] = R.make_records([[-1.5, -1.5, 0.5]], [[4, 0, 0]], [[0, 4, 0]], [301], [41])[0]  # behind, from -z
    win = max(lay.items(), key=lambda kv: (kv[1][1], kv[0]))  # largest position, then the later lane
    lanes, ids = sorted(lay), sorted(v[0] for v in lay.values())
    assert win[0] not in (lanes[0], lanes[-1]) and win[1][0] != ids[-1] and (copies == "dup" or win[1][0] != ids[0])
    return rec, np.array(sorted(lay)), win[1][0]


def bbox(rec):
    """Box of the real records' vertices and spheres (float32)."""
    rec = rec[rec.view(u32)[:, 3] != R.NO_PRIM]
    tri = R.is_triangle(rec)
    t, s = rec[tri], rec[~tri]
    pts = [t[:, 0:3], t[:, 0:3] + t[:, 4:7], t[:, 0:3] + t[:, 8:11], s[:, 0:3] - s[:, 4:5], s[:, 0:3] + s[:, 4:5]]
    p = np.concatenate(pts)
    return p.min(0).astype(f32), p.max(0).astype(f32)


def root_box(rec, shrink=0.5):
    """The root box handed to the scan: the records' box, narrowed in x and y
    so that parts of the primitives stick out of it -- a ray can then miss the
    root box and still cross a primitive, which only the box test rejects."""
    lo, hi = bbox(rec)
    c, h = (lo + hi) / 2, (hi - lo) / 2
    h[:2] *= shrink
    return (c - h).astype(f32), (c + h).astype(f32)


def _surface_points(rng, rec, which):
    """A point on each of the records rec[which]."""
    r = rec[which].astype(np.float64)
    a, b = rng.random(len(r)), rng.random(len(r))
    flip = a + b > 1
    a[flip], b[flip] = 1 - a[flip], 1 - b[flip]
    on_tri = r[:, 0:3] + a[:, None] * r[:, 4:7] + b[:, None] * r[:, 8:11]
    n = rng.normal(size=(len(r), 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    on_sph = r[:, 0:3] + n * r[:, 4:5]
    return np.where(R.is_triangle(rec[which])[:, None], on_tri, on_sph)


def _unit(d):
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def scan_rays(rng, rec, rmn, rmx, n=2048, targets=None):
    """n rays (o, mint, d, maxt) for a record set and its root box, shuffled:
    origins inside and outside the root box, aimed at the primitives and
    random, 10 % axis-aligned; rays outside aimed at what sticks out of the
    root box; maxt < mint; mint == kEps with the hit within a few epsilons of
    the origin (the adaptive epsilon decides); mint other than kEps; maxt
    between the first and the second hit, maxt before the first, mint between
    the two."""
    rmn, rmx = rmn.astype(np.float64), rmx.astype(np.float64)
    c, h = (rmn + rmx) / 2, (rmx - rmn) / 2
    real = np.flatnonzero(rec.view(u32)[:, 3] != R.NO_PRIM) if targets is None else np.asarray(targets)
    kind = rng.choice(7, n, p=[0.32, 0.13, 0.15, 0.10, 0.05, 0.10, 0.15])
    p = _surface_points(rng, rec, real[rng.integers(0, len(real), n)])
    inside = c + rng.uniform(-1, 1, (n, 3)) * h
    shell = c + rng.uniform(-3, 3, (n, 3)) * h
    ax = rng.integers(0, 3, n)  # push the outside origins out of the box on one axis at least
    far = np.abs(shell[np.arange(n), ax] - c[ax]) <= h[ax]
    shell[far, ax[far]] = c[ax[far]] + rng.choice([-1, 1], far.sum()) * h[ax[far]] * rng.uniform(1.05, 3, far.sum())
    o = np.where(np.isin(kind, (2, 3))[:, None], shell, inside)
    d = _unit(p - o)
    rnd = np.isin(kind, (1, 3))
    d[rnd] = _unit(rng.normal(size=(rnd.sum(), 3)))
    axis = np.flatnonzero(rng.random(n) < 0.10)  # d_i == 0 slabs
    d[axis] = 0
    d[axis, rng.integers(0, 3, len(axis))] = rng.choice([-1.0, 1.0], len(axis))
    d *= rng.choice([0.5, 1.0, 2.0], n)[:, None]
    near = kind == 5  # the hit a few (grown) epsilons ahead, either side of the threshold
    dn = _unit(rng.normal(size=(near.sum(), 3)))
    g = 1e-4 * np.maximum(1.0, np.abs(p[near]).max(axis=1)) * rng.uniform(0.3, 3, near.sum())
    o[near], d[near] = p[near] - dn * g[:, None], dn
    rays = np.zeros((n, 8), f32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, R.EPS, d, np.inf
    other = rng.random(n) < 0.15  # a mint that is not kEps: no growth
    rays[other & ~near, 3] = rng.choice([0.0, 1e-3, 0.01], (other & ~near).sum())
    dead = kind == 4
    rays[dead, 3], rays[dead, 7] = 1.0, 0.5
    span = np.flatnonzero(kind == 6)
    hit, t, _, _ = R.record_hits(rec, R.grow_mint(rays[span]))
    ts = np.sort(np.where(hit, t, np.inf), axis=1)
    t1, t2 = ts[:, 0], ts[:, 1] if ts.shape[1] > 1 else np.full(len(span), np.inf, f32)
    two = np.isfinite(t2) & (t2 > t1)
    mid = ((t1.astype(np.float64) + t2) / 2).astype(f32)
    how = rng.integers(0, 3, len(span))
    m = span[two & (how == 0)]
    rays[m, 7] = mid[two & (how == 0)]  # maxt between the first and the second hit
    m = span[np.isfinite(t1) & (how == 1)]
    rays[m, 7] = (t1[np.isfinite(t1) & (how == 1)] * f32(0.5))  # maxt before the first
    m = span[two & (how == 2)]
    rays[m, 3] = mid[two & (how == 2)]  # mint between the two
    return rays


def shares(rays, ref):
    """Fractions of the rays that hit, that pass the root box and hit nothing,
    that the root box rejects (maxt >= mint), and that resolve a tie."""
    grown = R.grow_mint(rays)
    boxed = ~(grown[:, 7] < grown[:, 3]) & ~ref["live"]
    return {"hit": float(ref["res"].mean()), "miss": float((ref["live"] & ~ref["res"]).mean()),
            "box": float(boxed.mean()), "tie": float(ref["ties"].mean())}


WAVE_POPCOUNTS = [0, 1, 2, 4, 5, 17, 64]
LONE_LANES = [0, 31, 32, 63]


def want_mask(rng, n):
    """Per wave of 64 rays a popcount of WAVE_POPCOUNTS in turn; the waves of
    popcount 1 take LONE_LANES in turn as their only wanting lane.  Returns
    (mask, the popcount of each wave)."""
    assert n % 64 == 0
    want = np.zeros(n, bool)
    waves, lone = n // 64, 0
    pops = []
    for w in range(waves):
        pc = WAVE_POPCOUNTS[w % len(WAVE_POPCOUNTS)]
        if pc == 1:
            lanes = [LONE_LANES[lone % 4]]
            lone += 1
        else:
            lanes = rng.permutation(64)[:pc]
        want[64 * w + np.asarray(lanes, int)] = True
        pops.append(pc)
    return want, np.array(pops)


# ---------------------------------------------------------------- primitive forms
def sphere_rows(rng, n):
    """(records, rays): a unit-sized configuration (centre, radius, origin
    inside, on and far outside the sphere, aimed, random and grazing rays)
    scaled as a whole by 2^k, k in [-70, 70], with directions of length 2^m,
    m in [-35, 35]: disc ~ 2^(2k+2m) crosses its gates at 2^+-96, y = 2 d.d ~
    2^(2m+1) and x1, x2 ~ 2^(k+m) theirs at 2^+-60, each while the others
    hold.  Half of the rows keep |k| <= 30 so that few intermediates are
    subnormal.  maxt between t1 and t2, mint between them, mint 0 and below."""
    c = rng.uniform(-1, 1, (n, 3))
    rad = rng.uniform(0.2, 1.0, n)
    u = _unit(rng.normal(size=(n, 3)))
    where = rng.choice(4, n, p=[0.3, 0.15, 0.4, 0.15])  # inside, on, outside, far outside
    dist = np.choose(where, [rng.uniform(0, 0.95, n), np.ones(n), rng.uniform(1.05, 4, n), rng.uniform(100, 1000, n)])
    o = c + u * (rad * dist)[:, None]
    aim = c + _unit(rng.normal(size=(n, 3))) * (rad * rng.uniform(0, 1.2, n))[:, None]
    d = _unit(aim - o)
    graze = rng.random(n) < 0.25  # tangent rays: disc a rounding either side of 0
    tp = c + _unit(rng.normal(size=(n, 3))) * rad[:, None]
    tang = _unit(np.cross(tp - c, rng.normal(size=(n, 3))))
    o[graze] = (tp - tang * rng.uniform(0.5, 3, n)[:, None])[graze]
    d[graze] = tang[graze]
    k = np.where(rng.random(n) < 0.5, rng.integers(-30, 31, n), rng.integers(-70, 71, n))
    m = rng.integers(-35, 36, n)
    S, Ld = 2.0 ** k, 2.0 ** m
    rec = R.make_records(c * S[:, None], np.stack([rad * S, np.zeros(n), np.zeros(n)], 1), np.zeros((n, 3)), np.arange(n),
                         np.zeros(n), sphere=True)
    rays = np.zeros((n, 8), f32)
    rays[:, 0:3], rays[:, 4:7] = o * S[:, None], d * Ld[:, None]
    rays[:, 3], rays[:, 7] = 0, np.inf
    # the roots in float64, for the bounds placed between them
    oc = rays[:, 0:3].astype(np.float64) - rec[:, 0:3]
    dd = rays[:, 4:7].astype(np.float64)
    A, B = (dd * dd).sum(1), 2 * (oc * dd).sum(1)
    C = (oc * oc).sum(1) - rec[:, 4].astype(np.float64) ** 2
    with np.errstate(all="ignore"):
        sq = np.sqrt(B * B - 4 * A * C)
        t1, t2 = (-B - sq) / (2 * A), (-B + sq) / (2 * A)
        mid = ((t1 + t2) / 2).astype(f32)
    how = rng.integers(0, 6, n)
    ok = np.isfinite(mid) & (mid > 0)
    rays[:, 3] = np.choose(how, [0, 0, 0, -S, S * 1e-4, 0]).astype(f32)
    rays[ok & (how == 1), 7] = mid[ok & (how == 1)]  # maxt between t1 and t2
    rays[ok & (how == 2), 3] = mid[ok & (how == 2)]  # mint between them
    return rec, rays


def plane_rows(rng, recs, A, n):
    """(records, rays) for one axis-plane pair `recs` of axis A: the ray
    generators of test_pair_filter.py (random with tiny components, and aimed
    within a few ulps of the edges and corners, origins close to the plane),
    origins exactly on the plane, mint = 0 among them."""
    from test_pair_filter import random_rays, targeted_rays

    o1, d1 = random_rays(rng, n // 2)
    o2, d2 = targeted_rays(rng, recs, A, 6 * 24 * max(1, n // (2 * 6 * 24 * 2)))
    o, d = np.concatenate([o1, o2]), np.concatenate([d1, d2])
    n = len(o)
    plane = rng.random(n) < 0.15
    o[plane, A] = recs[0][A]
    rays = np.zeros((n, 8), f32)
    rays[:, 0:3], rays[:, 4:7] = o, d
    rays[:, 3] = np.maximum(f32(1e-4), f32(1e-4) * np.abs(o).max(axis=1))
    rays[:, 7] = np.inf
    cam = rng.random(n) < 0.2
    rays[cam, 7] = rng.uniform(0.5, 20, cam.sum())
    rays[cam, 3] = rng.uniform(1e-4, 1e-2, cam.sum())
    zero = rng.random(n) < 0.3
    rays[zero, 3] = 0.0
    which = rng.integers(0, len(recs), n)
    return np.stack(recs)[which].astype(f32), rays, plane & zero


def box_rows(rng, n):
    """(min, max, rays): boxes with and without a degenerate axis; d_i == 0
    with the origin inside, outside and exactly on a face; tiny and subnormal
    d_i (infinite 1 / d_i: infinite and, from an origin on the face, NaN
    slabs); infinite and NaN origins and bounds."""
    mn = rng.uniform(-2, 0, (n, 3)).astype(f32)
    mx = (mn + rng.uniform(0.1, 2, (n, 3))).astype(f32)
    flat = rng.random(n) < 0.25
    fa = rng.integers(0, 3, n)
    mx[flat, fa[flat]] = mn[flat, fa[flat]]
    o = rng.uniform(-3, 3, (n, 3)).astype(f32)
    d = _unit(rng.normal(size=(n, 3)))
    aimed = rng.random(n) < 0.7  # through a point of the box
    d[aimed] = _unit(mn + rng.random((n, 3)) * (mx - mn) - o)[aimed]
    d = d.astype(f32)
    rows = np.arange(n)
    for axis_share, what in ((0.35, "zero"), (0.15, "tiny")):
        m = rng.random(n) < axis_share
        a = rng.integers(0, 3, n)
        d[m, a[m]] = 0.0 if what == "zero" else rng.choice([1e-40, -1e-40, 1e-38, -3e-39], m.sum()).astype(f32)
        place = rng.integers(0, 4, n)  # inside, outside, on the lower face, on the upper face
        mid = ((mn + mx) / 2)[rows, a]
        val = np.choose(place, [mid, mx[rows, a] + 1, mn[rows, a], mx[rows, a]])
        o[m, a[m]] = val[m]
    odd = np.flatnonzero(rng.random(n) < 0.05)
    o[odd, rng.integers(0, 3, len(odd))] = rng.choice([np.inf, -np.inf, np.nan], len(odd))
    odd = np.flatnonzero(rng.random(n) < 0.03)
    mx[odd, rng.integers(0, 3, len(odd))] = rng.choice([np.inf, np.nan], len(odd))
    rays = np.zeros((n, 8), f32)
    rays[:, 0:3], rays[:, 4:7] = o, d
    rays[:, 3] = rng.choice([0.0, 1e-4, 1.0], n)
    rays[:, 7] = np.where(rng.random(n) < 0.3, rng.uniform(0, 4, n), np.inf)
    return mn, mx, rays


# ---------------------------------------------------------------- the coop_scan cases
def coop_cases():
    """[(name, records, root_min, root_max, rays, tie info or None)], built once."""
    rng = np.random.default_rng(20240)
    cases = []

    def add(name, rec, box=None, targets=None, tie=None):
        rmn, rmx = box if box is not None else root_box(rec)
        cases.append((name, rec, rmn, rmx, scan_rays(rng, rec, rmn, rmx, targets=targets), tie))

    for n in (1, 2, 31, 32, 33, 63, 64):
        add(f"{n} triangles", triangles(rng, n))
        add(f"{n} spheres", spheres(rng, n))
    add("scan list shape, 10", scan_shape(rng, 5, 3, 2))
    add("scan list shape, 33", scan_shape(rng, 26, 2, 5))
    add("scan list shape, 64", scan_shape(rng, 45, 3, 16))
    add("scan list shape, 2^-10", scan_shape(rng, 9, 3, 4, 2.0 ** -10))
    add("scan list shape, 2^10", scan_shape(rng, 9, 3, 4, 2.0 ** 10))
    add("box scene", box_scene(rng))
    for copies in (3, 4, 5, "dup"):
        rec, lanes, winner = tie_set(rng, copies)
        lo, hi = bbox(rec)
        # aimed at the tied triangle and its two neighbours more often than at the fillers
        free = [k for k in range(len(rec)) if k not in lanes][:2]
        name = "tie set, a position twice" if copies == "dup" else f"tie set, {copies} copies"
        add(name, rec, (lo, hi), np.concatenate([np.repeat(lanes, 3), free]), (lanes, winner))
    return cases


# ---------------------------------------------------------------- the inputs are not vacuous
def check_coop_case(case):
    """Asserts, on the numpy reference alone, that a case of coop_cases()
    exercises what it is there for."""
    name, rec, rmn, rmx, rays, tie = case
    full = R.scan(rec, rmn, rmx, rays)
    s = shares(rays, full)
    assert s["hit"] >= 0.20 and s["miss"] >= 0.05 and s["box"] >= 0.05, (name, s)
    grown = R.grow_mint(rays)
    dead = grown[:, 7] < grown[:, 3]
    assert dead.mean() >= 0.02, name  # maxt < mint
    if np.abs(rays[:, 0:3]).max() > 1:  # the adaptive epsilon grows
        assert ((rays[:, 3] == R.EPS) & (grown[:, 3] > rays[:, 3])).sum() >= 20, name
    assert (rays[:, 3] != R.EPS).mean() >= 0.05, name
    assert (np.count_nonzero(rays[:, 4:7] == 0, axis=1) == 2).mean() >= 0.05, name  # axis-aligned
    inside = ((rays[:, 0:3] >= rmn) & (rays[:, 0:3] <= rmx)).all(axis=1)
    assert 0.2 < inside.mean() < 0.9, name
    assert np.isfinite(rays[:, 7]).mean() >= 0.05, name  # maxt placed around the hits
    if tie is None:
        would = ~full["live"] & ~dead & R.record_hits(rec, grown)[0].any(axis=1)
        assert would.mean() >= 0.01, (name, would.mean())  # only the root box test rejects these
    else:
        lanes, winner = tie
        assert s["tie"] >= 0.10, (name, s)
        # largest position: neither the first nor the last lane, nor an extreme id
        assert (full["prim"][full["ties"]] == winner).all(), name
        ids = rec.view(u32)[:, 3]
        others = ids[~np.isin(np.arange(len(rec)), lanes)]
        assert ((full["prim"] == others[0]) & full["res"]).any(), name  # the nearer triangle wins some rays
        assert ((full["prim"] == others[1]) & full["res"]).any(), name  # the farther one others


def _in60(x):
    with np.errstate(all="ignore"):
        return (np.abs(x) >= f32(2.0 ** -60)) & (np.abs(x) <= f32(2.0 ** 60))


def check_sphere_rows(rays, hit, normal, a):
    """Asserts, on the reference's results for sphere_rows(): every gate of
    sphere_hit_fast fails on accepted rays while the other three hold,
    accepted discriminants fall in the binades either side of both of its
    gates, both roots are returned, grazing discriminants fall on both sides
    of zero, and at least 90 % of the rows have no subnormal intermediate."""
    assert normal.mean() >= 0.90, normal.mean()
    with np.errstate(all="ignore"):
        gd = (a["disc"] >= f32(2.0 ** -96)) & (a["disc"] < f32(2.0 ** 96))
        e = np.frexp(a["disc"])[1]  # disc in [2^(e-1), 2^e)
    gy, g1, g2 = _in60(a["y"]), _in60(a["x1"]), _in60(a["x2"])
    assert (hit & gd & gy & g1 & g2).sum() > 10000  # the fast forms
    for name, g, others in (("disc", gd, gy & g1 & g2), ("y", gy, gd & g1 & g2), ("x1", g1, gd & gy & g2),
                            ("x2", g2, gd & gy & g1)):
        assert (hit & ~g & others).sum() >= 10, name  # the IEEE fallback, by this gate alone
    for gate in (-96, 96):
        assert ((e == gate) & hit).any() and ((e == gate + 1) & hit).any(), gate
    h1 = (rays[:, 3] <= a["t1"]) & (a["t1"] <= rays[:, 7])
    assert (hit & h1).sum() > 10000 and (hit & ~h1).sum() > 10000
    assert (a["disc"] < 0).mean() > 0.03 and (a["disc"] == 0).mean() > 0.01
    assert (rays[:, 3] < 0).any() and (rays[:, 3] == 0).any()
    assert np.isfinite(rays[:, 7]).mean() > 0.05  # maxt between the roots
