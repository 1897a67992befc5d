"""nori_film_splat (include/nori_gpu.h) restated in numpy, and the inputs the film-splat tests share.

splat_ref computes every term of the statement in float32, one float operation per step in the
order written there, and returns per film float
  film -- the float32 sum taken in index order (what the host statement returns, bit for bit),
  S    -- the sum of the same terms in float64,
  A    -- the sum of their magnitudes,
  m    -- their count,
plus the statistics (float32, index order) and the (splatted, dropped) counts.  Any order or
grouping of a float32 sum of m <= 4096 terms is within m 2^-24 A of the exact sum; within_bound
asserts that, with 2^-120 for what a hardware atomic may flush.
"""
import os

import numpy as np

from conftest import scene_path

F32 = np.float32
BLOCK = 32
RES = 32  # NORI_FILTER_RESOLUTION

# (name, the <rfilter> element, border)
FILTERS = [
    ("box", '<rfilter type="box"/>', 0),
    ("tent", '<rfilter type="tent"/>', 1),
    ("gaussian", '<rfilter type="gaussian"/>', 2),
    ("mitchell", '<rfilter type="mitchell"/>', 2),
    ("gaussian3", '<rfilter type="gaussian"><float name="radius" value="3.0"/></rfilter>', 3),
    ("gaussian45", '<rfilter type="gaussian"><float name="radius" value="4.5"/></rfilter>', 4),
]
FRAMES = [(72, 56), (33, 31)]  # 33 x 31: a 1-pixel-wide block column, a partial block row


def filter_scene_xml(tmp_dir, rfilter, name="cbox_filter.xml"):
    """cbox_path_mis with `rfilter` set (the rewrite of tests/test_gpu_parity.py); returns the path."""
    path = scene_path("pa4", "cbox", "cbox_path_mis.xml")
    src = open(path).read().replace('name="filename" value="', f'name="filename" value="{os.path.dirname(path)}/')
    out = os.path.join(str(tmp_dir), name)
    with open(out, "w") as f:
        f.write(src.replace('<camera type="perspective">', '<camera type="perspective">' + rfilter, 1))
    return out


def scene_filter(scene):
    """(radius, table) of a loaded scene."""
    return float(scene.desc.camera.filter_radius), scene.filter_table()


def splat_ref(W, H, radius, table, pos, val, ordered=False, want_stats=True):
    radius = F32(radius)
    table = np.asarray(table, F32)
    b = int(np.ceil(radius - F32(0.5)))
    lookup = F32(RES) / radius
    FW, FH = W + 2 * b, H + 2 * b
    pos = np.asarray(pos, F32).reshape(-1, 2)
    val = np.asarray(val, F32).reshape(-1, 3)
    n = pos.shape[0]
    if ordered:
        assert n % (W * H) == 0
    film = np.zeros((FH, FW, 4), F32)
    S = np.zeros((FH, FW, 4), np.float64)
    A = np.zeros((FH, FW, 4), np.float64)
    m = np.zeros((FH, FW, 4), np.int64)
    stats = np.zeros((H, W, 8), F32)
    counts = [0, 0]
    half = F32(0.5)
    one = F32(1.0)
    with np.errstate(all="ignore"):
        for i in range(n):
            sx, sy = pos[i]
            v = val[i]
            ok = bool(np.isfinite(sx) and np.isfinite(sy))
            if ok and ordered:
                pix = i % (W * H)
                x, y = pix % W, pix // W
                ok = bool(F32(x) <= sx <= F32(x + 1) and F32(y) <= sy <= F32(y + 1))
            elif ok:
                fx, fy = np.floor(sx), np.floor(sy)
                ok = bool(0 <= fx < W and 0 <= fy < H)
                if ok:
                    x, y = int(fx), int(fy)
            ok = ok and bool(np.all(np.isfinite(v)) and np.all(v >= 0))  # Color3f::isValid
            if not ok:
                counts[1] += 1
                continue
            counts[0] += 1
            if want_stats:
                st = stats[y, x]
                st[0:3] += v
                st[3:6] += v * v
                st[6] += one
            ox, oy = (x // BLOCK) * BLOCK, (y // BLOCK) * BLOCK
            bw, bh = min(BLOCK, W - ox), min(BLOCK, H - oy)
            px = sx - half - F32(ox - b)
            py = sy - half - F32(oy - b)
            x0, x1 = max(int(np.ceil(px - radius)), 0), min(int(np.floor(px + radius)), bw + 2 * b - 1)
            y0, y1 = max(int(np.ceil(py - radius)), 0), min(int(np.floor(py + radius)), bh + 2 * b - 1)
            if x1 < x0 or y1 < y0:
                continue
            cx = np.arange(x0, x1 + 1).astype(F32)
            cy = np.arange(y0, y1 + 1).astype(F32)
            wx = table[np.minimum((np.abs(cx - px) * lookup).astype(np.int32), RES)]
            wy = table[np.minimum((np.abs(cy - py) * lookup).astype(np.int32), RES)]
            v4 = np.array([v[0], v[1], v[2], one], F32)
            t = (v4[None, None, :] * wx[None, :, None]) * wy[:, None, None]  # float32: (val.c * wx) * wy
            assert t.dtype == F32
            sl = (slice(oy + y0, oy + y1 + 1), slice(ox + x0, ox + x1 + 1))
            film[sl] += t
            t64 = t.astype(np.float64)
            S[sl] += t64
            A[sl] += np.abs(t64)
            m[sl] += 1
    return {"film": film, "S": S, "A": A, "m": m, "stats": stats, "counts": tuple(counts), "border": b}


def add_refs(a, b):
    """The restatement of two sample sets splatted into one film (S, A, m and the counts add)."""
    return {"S": a["S"] + b["S"], "A": a["A"] + b["A"], "m": a["m"] + b["m"],
            "counts": (a["counts"][0] + b["counts"][0], a["counts"][1] + b["counts"][1]), "border": a["border"]}


def bound(ref):
    return ref["m"] * 2.0 ** -24 * ref["A"] + 2.0 ** -120


def assert_within_bound(film, ref, what=""):
    """|film - S| <= m 2^-24 A + 2^-120 for every film float; no excluded pixels."""
    assert ref["m"].max() <= 4096, ref["m"].max()
    film = np.asarray(film)
    assert film.shape == ref["S"].shape and np.isfinite(film).all(), what
    err = np.abs(film.astype(np.float64) - ref["S"])
    lim = bound(ref)
    worst = np.unravel_index(np.argmax(err - lim), err.shape)
    print(f"{what}: max |film - S| = {err.max():.3e}, worst margin at {worst}: err {err[worst]:.3e} bound {lim[worst]:.3e}, "
          f"m max {ref['m'].max()}")
    assert (err <= lim).all(), (what, worst, err[worst], lim[worst])


def scattered_inputs(W, H, n=2000, seed=1):
    """n seeded samples anywhere on (and around) the frame, with the special cases of the issue:
    positions on exact integers, on the frame's four edges and just outside, NaN / inf positions,
    negative / NaN / inf values."""
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.uniform(-1.0, W + 1.0, n), rng.uniform(-1.0, H + 1.0, n)], 1).astype(F32)
    val = rng.uniform(0.0, 2.0, (n, 3)).astype(F32)
    fW, fH = F32(W), F32(H)
    k = 0

    def put(x, y, v=None):
        nonlocal k
        pos[k] = (x, y)
        if v is not None:
            val[k] = v
        k += 1

    # exact integers (block corners and edges among them)
    for x, y in [(0, 0), (W - 1, H - 1), (32, 32), (31, 5), (5, 31), (32, 0), (0, 32), (17, 9), (W - 1, 0), (0, H - 1)]:
        put(F32(x), F32(y))
    # the frame's four edges and just outside / inside
    for x in [F32(0), np.nextafter(F32(0), F32(-1)), F32(-0.0), fW, np.nextafter(fW, F32(0)), np.nextafter(fW, F32(2) * fW),
              F32(-0.5), fW + F32(0.5)]:
        put(x, F32(H / 2 + 0.25))
    for y in [F32(0), np.nextafter(F32(0), F32(-1)), F32(-0.0), fH, np.nextafter(fH, F32(0)), np.nextafter(fH, F32(2) * fH),
              F32(-0.5), fH + F32(0.5)]:
        put(F32(W / 2 + 0.75), y)
    # corners of the frame, half-integers (the box filter's reach ends on a cell)
    for x, y in [(0.5, 0.5), (W - 0.5, H - 0.5), (31.5, 31.5), (32.5, 0.5)]:
        put(F32(x), F32(y))
    # positions that are not finite, or far away
    for x, y in [(np.nan, 3), (3, np.nan), (np.inf, 3), (3, -np.inf), (1e30, 3), (3, -1e30), (np.nan, np.nan)]:
        put(F32(x), F32(y))
    # values that fail Color3f::isValid (at positions inside the frame), and ones that pass
    for v in [(-1, 1, 1), (1, -1e-30, 1), (1, 1, np.nan), (np.inf, 1, 1), (1, -np.inf, 1), (np.nan, np.nan, np.nan)]:
        put(F32(10.25), F32(7.5), v)
    for v in [(0, 0, 0), (-0.0, 1, 1), (1e-40, 1e30, 3)]:
        put(F32(20.75), F32(11.5), v)
    assert k <= n
    return pos, val


def ordered_inputs(W, H, passes, seed=2):
    """Samples in the passes layout: pos = (float32) pixel + u, u in [0, 1).  Pass 0 also holds
    samples exactly on their pixel's far edge and near edge (kept), outside their pixel (dropped)
    and with invalid values (dropped), in the frame's first, an inner and its last blocks."""
    rng = np.random.default_rng(seed)
    u = rng.random((passes, H, W, 2), dtype=F32)
    ys, xs = np.mgrid[0:H, 0:W]
    pix = np.stack([xs, ys], -1).astype(F32)
    pos = pix[None] + u
    assert pos.dtype == F32
    val = rng.uniform(0.0, 2.0, (passes, H, W, 3)).astype(F32)
    spots = [(3, 2), (31, 4), (4, 31), (31, 31), (32, 7), (W - 1, 9), (9, H - 1), (W - 1, H - 1), (0, 0), (W // 2, H // 2)]
    spots = [(min(x, W - 1), min(y, H - 1)) for x, y in spots]
    for j, (x, y) in enumerate(spots):
        # far edge: x + 1 and / or y + 1 exactly
        pos[0, y, x] = (x + 1, y + 0.25) if j % 3 == 0 else (x + 0.75, y + 1) if j % 3 == 1 else (x + 1, y + 1)
    for j, (x, y) in enumerate([(5, 6), (W - 2, 12), (12, H - 2), (W - 2, H - 2)]):
        pos[0, y, x] = (x, y + 0.5) if j % 2 == 0 else (x, y)  # near edge
    for (x, y), p in [((7, 3), (8.5, 3.5)), ((8, 3), (7.75, 3.5)), ((9, 3), (9.5, 2.5)), ((10, 3), (10.5, np.nan)),
                      ((11, 3), (np.inf, 3.5)), ((W - 1, 3), (W + 0.5, 3.5))]:
        pos[0, y, x] = p  # outside the owner's square, or not finite
    for (x, y), v in [((7, 5), (-1, 1, 1)), ((8, 5), (1, np.nan, 1)), ((9, 5), (1, 1, np.inf))]:
        val[0, y, x] = v
    return pos, val
