"""Unit tests of the tail finisher's hand-written pieces and of the scan's
primitive tests, run on the GPU through libnori_devtest.so (csrc/devtest.hip,
tests/devtest_util.py) -- whole renders only see them through a loose image
comparison, on a handful of samples per frame.

a. k_tail_prefix's body (coop_scan.h tail_prefix, launched 1 x 1024 as
   launch_tail_prefix does) against np.cumsum;
b. the gid -> segment -> queue-slot lookup of k_finish (tail_index.h) against
   np.searchsorted;
c. coop_load / coop_scan, closest and any-hit, in whole converged waves,
   against the numpy scan rule of tests/coop_ref.py (pinned to the oracle on
   the CPU by tests/test_coop_ref.py) -- res, t, prim, u, v of every lane;
d. the primitive forms against each other and against numpy: sphere_hit_fast
   == sphere_hit_nb == sphere_hit across its range gates, sphere_hit_fast's
   NOCHECK form on its precondition, tri_hit_plane<A> == tri_hit_nb ==
   tri_hit, box_test.

Every comparison is of 32-bit patterns (NaN against NaN counting as equal):
both sides state the same fp32 operations.  The inputs come from
tests/finish_tail_inputs.py; each case first checks on the CPU side that it
is not vacuous (shares of hits, misses, root-box rejections, resolved ties).

One claim did not hold as scan.h used to state it and is pinned as found
(test_plane_zero_t_keeps_its_own_sign): a ray with mint <= 0 whose origin
lies in the triangle's plane is accepted at t = +-0, and the sign of that
zero differs between tri_hit_plane and tri_hit_nb.  scan_core already sends
waves holding such rays to the generic test (ZMINT); path rays have mint > 0.
"""
import numpy as np
import pytest

import coop_ref as R
import devtest_util as D
import finish_tail_inputs as I
import nori_amd
from conftest import scene_path
from test_gpu_device_units import assert_same_bits, same_bits

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32


# ---------------------------------------------------------------- a, b. prefix and lookup
@pytest.fixture(scope="module")
def count_sets(built):
    rng = np.random.default_rng(77)
    return {G: I.count_vectors(G, rng) for G in I.PREFIX_GS}


@pytest.mark.parametrize("G", I.PREFIX_GS)
def test_tail_prefix_is_cumsum(count_sets, G):
    for name, cnt in count_sets[G]:
        ref = np.concatenate([[0], np.cumsum(cnt.astype(np.uint64))])
        pre = D.tail_prefix(cnt)
        assert pre.shape == (G + 1,)
        assert int(pre[G]) == int(ref[G]), (name, G, int(pre[G]), int(ref[G]))
        bad = np.flatnonzero(pre.astype(np.uint64) != ref)
        assert bad.size == 0, (name, G, bad[:5], pre[bad[:5]], ref[bad[:5]])


@pytest.mark.parametrize("G", I.PREFIX_GS)
def test_tail_lookup_is_searchsorted(count_sets, G):
    rng = np.random.default_rng(78)
    looked = 0
    for name, cnt in count_sets[G]:
        pre = np.concatenate([[0], np.cumsum(cnt.astype(np.uint64))]).astype(u32)
        gids = I.lookup_gids(pre, rng)
        if not gids.size:
            continue  # (n = 0: the finisher starts no lane)
        seg, q = D.tail_lookup(pre, gids)
        want = (np.searchsorted(pre, gids, side="right") - 1).astype(np.int64)
        bad = np.flatnonzero(seg != want)
        assert bad.size == 0, (name, G, gids[bad[:5]], seg[bad[:5]], want[bad[:5]])
        assert (cnt[want] > 0).all()  # the reference itself never names an empty segment
        slot = want * I.KSEG + gids - pre[want]
        bad = np.flatnonzero(q != slot)
        assert bad.size == 0, (name, G, gids[bad[:5]], q[bad[:5]], slot[bad[:5]])
        assert (q - seg * I.KSEG < cnt[seg]).all() and (q < G * I.KSEG).all()
        looked += gids.size
    assert looked > 0


# ---------------------------------------------------------------- c. coop_scan
CASES = None


def _cases():
    global CASES
    if CASES is None:
        CASES = I.coop_cases()
        for c in CASES:
            for a in c[1:5]:
                a.setflags(write=False)
    return CASES


CASE_NAMES = [f"{n} {k}" for n in (1, 2, 31, 32, 33, 63, 64) for k in ("triangles", "spheres")] + [
    "scan list shape, 10", "scan list shape, 33", "scan list shape, 64", "scan list shape, 2^-10",
    "scan list shape, 2^10", "box scene", "tie set, 3 copies", "tie set, 4 copies", "tie set, 5 copies",
    "tie set, a position twice"]


def _assert_scan(got, ref, what):
    for k in ("res", "prim"):
        bad = np.flatnonzero(got[k] != ref[k])
        assert bad.size == 0, (what, k, bad.size, bad[:5], got[k][bad[:5]], ref[k][bad[:5]])
    for k in ("t", "u", "v"):
        assert_same_bits(got[k], ref[k], f"{what}: {k}")


@pytest.mark.parametrize("name", CASE_NAMES)
def test_coop_scan_matches_reference(built, name):
    case = [c for c in _cases() if c[0] == name]
    assert len(case) == 1
    _, rec, rmn, rmx, rays, tie = case[0]
    n, P = len(rays), len(rec)
    assert n == 2048 and P <= 64
    I.check_coop_case(case[0])  # not vacuous: on the reference alone, before any device result
    rng = np.random.default_rng(len(name))
    want, pops = I.want_mask(rng, n)
    assert set(pops) == set(I.WAVE_POPCOUNTS)
    lone = [int(np.flatnonzero(want[64 * w:64 * w + 64])[0]) for w in np.flatnonzero(pops == 1)]
    assert set(lone) == set(I.LONE_LANES)
    if P < 64:
        assert (want & (np.arange(n) % 64 >= P)).any()  # a wanting lane that holds no primitive
    for mask, label in ((want, "mixed waves"), (np.ones(n, bool), "every lane")):
        for any_hit in (False, True):
            ref = R.scan(rec, rmn, rmx, rays, mask, any_hit)
            assert ref["res"][mask].any() and not ref["res"][mask].all()
            got = D.coop_scan(rec, rmn, rmx, rays, mask, any_hit)
            _assert_scan(got, ref, f"{name}, {label}, {'any-hit' if any_hit else 'closest'}")
            off = ~mask  # untouched defaults
            assert not got["res"][off].any() and (got["prim"][off] == R.NO_PRIM).all()
            assert np.isposinf(got["t"][off]).all()
            assert not got["u"][off].view(u32).any() and not got["v"][off].view(u32).any()


def test_coop_scan_rejects_bad_arguments(built):
    rec = R.padding_records(65)
    rays = np.zeros((64, 8), f32)
    with pytest.raises(RuntimeError):
        D.coop_scan(rec, np.zeros(3, f32), np.ones(3, f32), rays, np.ones(64, bool))


# ---------------------------------------------------------------- d. primitive forms
SPHERE_ROWS = 1 << 17


@pytest.fixture(scope="module")
def sphere_rows(built):
    rec, rays = I.sphere_rows(np.random.default_rng(31), SPHERE_ROWS)
    hit, t, normal, aux = R.sphere(rec, rays)
    forms = {f: D.prim_hit(f, rec, rays) for f in (D.SPHERE, D.SPHERE_NB, D.SPHERE_FAST, D.SPHERE_FAST_NOCHECK)}
    return rec, rays, (hit, t, normal, aux), forms


def _assert_hits_equal(a, b, what, rows=None):
    ha, ta = a[0], a[1]
    hb, tb = b[0], b[1]
    rows = np.ones(len(ha), bool) if rows is None else rows
    bad = np.flatnonzero((ha != hb) & rows)
    assert bad.size == 0, (what, "hit flags", bad.size, bad[:5], ta[bad[:5]], tb[bad[:5]])
    h = ha & rows
    assert_same_bits(ta[h], tb[h], f"{what}: t")
    return int(h.sum())


def test_sphere_rows_cross_every_gate(sphere_rows):
    _, rays, (hit, _, normal, aux), _ = sphere_rows
    I.check_sphere_rows(rays, hit, normal, aux)


def test_sphere_forms_agree(sphere_rows):
    _, _, (hit, t, normal, _), forms = sphere_rows
    n = _assert_hits_equal(forms[D.SPHERE_FAST], forms[D.SPHERE_NB], "sphere_hit_fast<false> against sphere_hit_nb")
    assert n > SPHERE_ROWS // 4
    _assert_hits_equal(forms[D.SPHERE_NB], forms[D.SPHERE], "sphere_hit_nb against sphere_hit")
    for f, name in ((D.SPHERE, "sphere_hit"), (D.SPHERE_NB, "sphere_hit_nb"), (D.SPHERE_FAST, "sphere_hit_fast")):
        _assert_hits_equal(forms[f], (hit, t), f"{name} against numpy", normal)


def test_sphere_nocheck_on_its_precondition(sphere_rows):
    _, _, (_, _, _, a), forms = sphere_rows
    pre = (a["y"] >= f32(2.0 ** -60)) & (a["y"] <= f32(2.0 ** 60))
    assert 0.5 < pre.mean() < 1.0
    n = _assert_hits_equal(forms[D.SPHERE_FAST_NOCHECK], forms[D.SPHERE_FAST],
                           "sphere_hit_fast<true> against sphere_hit_fast<false>", pre)
    assert n > SPHERE_ROWS // 4


@pytest.fixture(scope="module")
def plane_pairs(built):
    s = nori_amd.load_scene(scene_path("pa4", "cbox", "cbox_path_mis.xml"), 32, 32, 1)
    L = nori_amd.scan_list(s)
    out = []
    for g in range(len(L["plane_c"])):
        A = int(np.searchsorted(L["plane_end"], g, side="right"))
        recs = [L["records"][2 * g + k] for k in range(2)]
        for r in recs:
            assert r[4 + A] == 0 and r[8 + A] == 0
        out.append((A, recs))
    assert sorted({a for a, _ in out}) == [0, 1, 2]
    return out


def _plane_forms(A, recs, seed):
    rec, rays, plane0 = I.plane_rows(np.random.default_rng(seed), recs, A, 40000)
    dev = {f: D.prim_hit(f, rec, rays) for f in (D.TRI, D.TRI_NB, D.TRI_PLANE0 + A)}
    return rec, rays, plane0, dev, R.tri(rec, rays), R.tri_plane(rec, rays, A)


def _eq_up_to_zero_sign(a, b):
    return same_bits(a, b) | ((a == 0) & (b == 0))


def test_plane_form_is_generic_form(plane_pairs):
    hits = zero_t = 0
    for g, (A, recs) in enumerate(plane_pairs):
        rec, rays, plane0, dev, ref, ref_plane = _plane_forms(A, recs, 40 + g)
        pl, nb, br = dev[D.TRI_PLANE0 + A], dev[D.TRI_NB], dev[D.TRI]
        what = f"pair {g} (axis {A})"
        for other, name in ((nb, "tri_hit_nb"), (br, "tri_hit"), (ref, "numpy")):
            assert np.array_equal(pl[0], other[0]), (what, name, np.flatnonzero(pl[0] != other[0])[:5])
        h = pl[0]
        # each device form against its own statement in numpy: all bits, the sign of a zero included
        for k in range(1, 4):
            assert_same_bits(pl[k][h], ref_plane[k][h], f"{what}: tri_hit_plane against numpy, column {k}")
            assert_same_bits(nb[k][h], ref[k][h], f"{what}: tri_hit_nb against numpy, column {k}")
            assert_same_bits(br[k][h], ref[k][h], f"{what}: tri_hit against numpy, column {k}")
        # the forms against each other: t bit for bit; u, v as values, bit for bit but for the sign of a zero
        nz = h & (pl[1] != 0)
        assert_same_bits(pl[1][nz], nb[1][nz], f"{what}: t of tri_hit_plane against tri_hit_nb")
        assert (pl[1][h] == nb[1][h]).all()
        for k in (2, 3):
            assert _eq_up_to_zero_sign(pl[k][h], nb[k][h]).all(), (what, k)
        # an accepted zero t needs mint <= 0 and an origin in the plane (the regression case below)
        z = h & (pl[1] == 0)
        assert (rays[z, 3] <= 0).all() and (rays[z, A] == rec[z, A]).all()
        assert (h & plane0).sum() >= z.sum() > 0
        hits += int(h.sum())
        zero_t += int(z.sum())
    assert hits > 10000 and zero_t > 100


def test_plane_zero_t_keeps_its_own_sign(plane_pairs):
    """Regression case for scan.h's claim about tri_hit_plane: origin in the
    triangle's plane, mint = 0.  Both forms accept the ray at t = +-0; the sign
    is that of each form's own numerator (the generic form adds the signed
    zero products the plane form leaves out), so it differs on some rays and
    never anywhere else.  Pinned: each form equals its numpy statement bit for
    bit, and the two differ in nothing but that sign."""
    differ = hits = 0
    for g, (A, recs) in enumerate(plane_pairs):
        rng = np.random.default_rng(60 + g)
        rec, rays, _ = I.plane_rows(rng, recs, A, 8000)
        rays[:, A] = rec[:, A]
        rays[:, 3], rays[:, 7] = 0.0, np.inf
        pl, nb = D.prim_hit(D.TRI_PLANE0 + A, rec, rays), D.prim_hit(D.TRI_NB, rec, rays)
        ref, ref_plane = R.tri(rec, rays), R.tri_plane(rec, rays, A)
        assert np.array_equal(pl[0], nb[0]) and np.array_equal(pl[0], ref[0])
        h = pl[0]
        assert h.sum() > 50 and (pl[1][h] == 0).all() and (nb[1][h] == 0).all()  # (the light is small)
        hits += int(h.sum())
        assert_same_bits(pl[1][h], ref_plane[1][h], "tri_hit_plane's zero t against numpy")
        assert_same_bits(nb[1][h], ref[1][h], "tri_hit_nb's zero t against numpy")
        differ += int((np.signbit(pl[1][h]) != np.signbit(nb[1][h])).sum())
    assert hits > 2000
    assert differ > 0  # (if this ever becomes 0, scan_core's ZMINT detour has lost its reason)


def test_box_test(built):
    mn, mx, rays = I.box_rows(np.random.default_rng(51), 1 << 16)
    ok, near = R.box(mn, mx, rays)
    assert 0.2 < ok.mean() < 0.8 and np.isnan(near).any() and np.isinf(near[ok]).any()
    zero = rays[:, 4:7] == 0
    assert (zero.any(axis=1) & ok).sum() > 1000 and (zero.any(axis=1) & ~ok).sum() > 1000
    on_face = ((rays[:, 0:3] == mn) | (rays[:, 0:3] == mx)) & zero
    assert (on_face.any(axis=1) & ok).sum() > 100  # d_i == 0 on a face counts as inside
    assert ((mn == mx).any(axis=1) & ok).sum() > 100  # a degenerate axis
    rec = np.zeros((len(rays), 12), f32)
    rec[:, 0:3], rec[:, 4:7] = mn, mx
    got = D.prim_hit(D.BOX, rec, rays)
    bad = np.flatnonzero(got[0] != ok)
    assert bad.size == 0, (bad.size, bad[:5], rays[bad[:5]], mn[bad[:5]], mx[bad[:5]])
    assert_same_bits(got[1], near, "box_test: tnear")
