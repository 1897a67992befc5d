"""nori_film_gather (include/nori_gpu.h), the film splat's adjoint, restated in numpy.

gather_ref computes every term (G[c] * wx) * wy of the statement in float32, one float operation
per step, and returns per output float
  out -- the float32 sum taken in the stated order (cy ascending, then cx ascending, from 0.0f):
         what the host statement returns, bit for bit,
  S   -- the sum of the same float32 terms in float64,
  A   -- the sum of their magnitudes,
  m   -- their count (per sample: the three channels share it),
plus the kept samples' mask and the (kept, dropped) counts.  Any order of a float32 sum of m
terms is within m 2^-24 A of the exact sum; assert_within_bound asserts that, with the 2^-120 of
film_splat_ref.  Filters, frames and inputs are film_splat_ref's.
"""
import numpy as np

from film_splat_ref import BLOCK, F32, RES


def gather_ref(W, H, radius, table, pos, grad, val=None, ordered=False):
    radius = F32(radius)
    table = np.asarray(table, F32)
    b = int(np.ceil(radius - F32(0.5)))
    lookup = F32(RES) / radius
    grad = np.asarray(grad, F32)
    assert grad.shape == (H + 2 * b, W + 2 * b, 4)
    pos = np.asarray(pos, F32).reshape(-1, 2)
    n = pos.shape[0]
    if val is not None:
        val = np.asarray(val, F32).reshape(-1, 3)
        assert val.shape[0] == n
    if ordered:
        assert n % (W * H) == 0
    out = np.zeros((n, 3), F32)
    S = np.zeros((n, 3), np.float64)
    A = np.zeros((n, 3), np.float64)
    m = np.zeros(n, np.int64)
    kept = np.zeros(n, bool)
    half = F32(0.5)
    zero = np.zeros((1, 3), F32)
    with np.errstate(all="ignore"):
        for i in range(n):
            sx, sy = pos[i]
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
            if ok and val is not None:
                ok = bool(np.all(np.isfinite(val[i])) and np.all(val[i] >= 0))  # Color3f::isValid
            if not ok:
                continue
            kept[i] = True
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
            G = grad[oy + y0:oy + y1 + 1, ox + x0:ox + x1 + 1, 0:3]
            t = (G * wx[None, :, None]) * wy[:, None, None]  # float32: (G[c] * wx) * wy
            assert t.dtype == F32
            t = t.reshape(-1, 3)  # cy ascending, then cx ascending
            # acc = 0.0f, then one float32 addition per term in that order (accumulate is sequential)
            out[i] = np.add.accumulate(np.concatenate([zero, t]), axis=0, dtype=F32)[-1]
            t64 = t.astype(np.float64)
            S[i] = t64.sum(0)
            A[i] = np.abs(t64).sum(0)
            m[i] = t.shape[0]
    k = int(kept.sum())
    return {"out": out, "S": S, "A": A, "m": m, "kept": kept, "counts": (k, n - k), "border": b}


def bound(ref):
    return ref["m"][:, None] * 2.0 ** -24 * ref["A"] + 2.0 ** -120


def assert_within_bound(rows, ref, what=""):
    """|rows - S| <= m 2^-24 A + 2^-120 for every output float; no excluded rows; dropped rows exactly 0."""
    rows = np.asarray(rows).reshape(-1, 3)
    assert rows.shape == ref["S"].shape and np.isfinite(rows).all(), what
    err = np.abs(rows.astype(np.float64) - ref["S"])
    lim = bound(ref)
    worst = np.unravel_index(np.argmax(err - lim), err.shape)
    used = (err / lim).max()
    print(f"{what}: max |out - S| = {err.max():.3e}, worst margin at {worst}: err {err[worst]:.3e} bound {lim[worst]:.3e}, "
          f"share of the bound {used:.3f}, m max {ref['m'].max()}")
    assert (err <= lim).all(), (what, worst, err[worst], lim[worst])
    assert not rows[~ref["kept"]].view(np.uint32).any(), what  # (+0.0 exactly)


def seeded_grad(shape, seed=11):
    """A seeded normal film gradient; channel 3 holds NaN: the statement never reads it."""
    g = np.random.default_rng(seed).standard_normal(shape).astype(F32)
    g[..., 3] = np.nan
    return g


def adjoint_check(film, grad, val, rows, ref, m_forward, what=""):
    """The adjoint identity <film[..., :3], grad[..., :3]> = <val_kept, rows> under the bound
    (m_max + 4) 2^-24 T: both sums in float64, T the float64 sum of |val| A over the kept samples,
    m_max the larger of the two term counts -- the forward's per film float (`m_forward`, from
    splat_ref) and the gather's per row.  `rows` is the gather under test, `ref` its restatement."""
    film = np.asarray(film, np.float64)
    grad = np.asarray(grad, np.float64)
    rows = np.asarray(rows, np.float64).reshape(-1, 3)
    val = np.asarray(val, np.float64).reshape(-1, 3)
    k = ref["kept"]
    lhs = float((film[..., :3] * grad[..., :3]).sum())
    rhs = float((val[k] * rows[k]).sum())
    T = float((np.abs(val[k]) * ref["A"][k]).sum())
    m_max = max(int(np.max(m_forward)), int(ref["m"].max()))
    lim = (m_max + 4) * 2.0 ** -24 * T
    print(f"{what}: <film, grad> = {lhs:.9e}, <val, grad_val> = {rhs:.9e}, gap {abs(lhs - rhs):.3e}, "
          f"bound {lim:.3e} (m_max {m_max}), share {abs(lhs - rhs) / lim:.3f}")
    assert np.isfinite(lhs) and np.isfinite(rhs) and T > 0, what
    assert abs(lhs - rhs) <= lim, (what, lhs, rhs, lim)
