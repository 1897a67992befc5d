"""The film gather on the GPU: nori_gpu_film_gather (k_gather_scatter) and nori_gpu_film_gather_passes
(k_gather_pos), csrc/kernels_gather.hip, stated at nori_film_gather in include/nori_gpu.h, and the
torch.autograd wrapper on top of them (nori_amd/autograd.py, examples/fit_albedo_torch.py).

The device calls produce the statement's float32 terms and may add a sample's terms in another
order, so every row is compared with the float64 sum S of the numpy restatement
(tests/film_gather_ref.py) under |out - S| <= m 2^-24 A + 2^-120: no fitted tolerance, no excluded
rows, dropped rows exactly 0.

1. scattered samples; 2. the passes layout; 3. block subsets; 4. host and device forms; 5. the
adjoint identity; 6. autograd; 7. refusals; 8. examples/fit_albedo_torch.py."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import film_gather_ref as G
import film_splat_ref as R
import nori_amd
from conftest import ROOT, scene_path
from nori_amd import _abi

pytestmark = pytest.mark.gpu
f32 = np.float32
FILTER = {f[0]: f for f in R.FILTERS}
_SCENES, _REFS = {}, {}


def scene_of(tmp_path_factory, name, W, H, spp=2):
    key = (name, W, H, spp)
    if key not in _SCENES:
        d = tmp_path_factory.mktemp(f"gather_{name}_{W}x{H}")
        s = nori_amd.load_scene(R.filter_scene_xml(d, FILTER[name][1]), W, H, spp)
        _SCENES[key] = (s,) + R.scene_filter(s) + (G.seeded_grad(s.film_shape()),)
    return _SCENES[key]


def counts_of(r):
    return (r.last_stats["samples"], r.last_stats["invalid_samples"])


def head(ref, n):
    """The restatement of the first n samples (every row depends on its own sample only)."""
    k = int(ref["kept"][:n].sum())
    return {"out": ref["out"][:n], "S": ref["S"][:n], "A": ref["A"][:n], "m": ref["m"][:n], "kept": ref["kept"][:n],
            "counts": (k, n - k), "border": ref["border"]}


def cached(key, make):
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


def scattered_ref(name, W, H, rad, tab, grad, with_val=True):
    pos, val = R.scattered_inputs(W, H)
    return cached(("scat", name, W, H, with_val), lambda: G.gather_ref(W, H, rad, tab, pos, grad, val if with_val else None))


def ordered(W, H):
    return cached(("ord", W, H), lambda: R.ordered_inputs(W, H, 5))


def ordered_ref(name, W, H, rad, tab, grad, with_val=True):
    po, vo = ordered(W, H)
    return cached(("ordref", name, W, H, with_val),
                  lambda: G.gather_ref(W, H, rad, tab, po, grad, vo if with_val else None, ordered=True))


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---------------------------------------------------------------- 1. scattered
@pytest.mark.parametrize("frame", R.FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("filt", [f[0] for f in R.FILTERS])
def test_scattered_against_the_statement(built, tmp_path_factory, filt, frame):
    W, H = frame
    s, rad, tab, grad = scene_of(tmp_path_factory, filt, W, H)
    pos, val = R.scattered_inputs(W, H)
    full = scattered_ref(filt, W, H, rad, tab, grad)
    with nori_amd.GpuRenderer(s, 0) as r:
        for n in (1, 63, 64, 65, 1000, 2000):
            ref = head(full, n)
            rows = r.film_gather(pos[:n], grad, val[:n])
            assert rows.shape == (n, 3) and counts_of(r) == ref["counts"], n
            assert r.last_stats["ms_splat"] > 0 and r.last_stats["ms_total"] > 0
            G.assert_within_bound(rows, ref, f"{filt} {W}x{H} n={n}")
        assert full["counts"][1] >= 20 and full["counts"] == nori_amd.film_gather(s, pos, grad, val)[1]
        # val=None keeps the invalid-value rows
        ref0 = scattered_ref(filt, W, H, rad, tab, grad, with_val=False)
        rows = r.film_gather(pos, grad)
        assert counts_of(r) == ref0["counts"] and ref0["counts"][0] == full["counts"][0] + 6
        G.assert_within_bound(rows, ref0, f"{filt} {W}x{H} val=None")
        # 4096 samples inside one pixel (the forward's contention case: here every row stands alone)
        rng = np.random.default_rng(7)
        px = np.array([min(40, W - 1), min(20, H - 1)], f32)
        cpos = (px + rng.random((4096, 2), dtype=f32)).astype(f32)
        cpos = np.minimum(cpos, np.nextafter(px + f32(1), f32(0)))
        cval = rng.uniform(0.0, 2.0, (4096, 3)).astype(f32)
        ref = G.gather_ref(W, H, rad, tab, cpos, grad, cval)
        assert ref["counts"] == (4096, 0)
        rows = r.film_gather(cpos, grad, cval)
        assert counts_of(r) == (4096, 0)
        G.assert_within_bound(rows, ref, f"{filt} {W}x{H} one pixel")
        # n == 0 is a no-op
        out = np.full((0, 3), 1, f32)
        assert r.film_gather(cpos[:0], grad, cval[:0], out=out) is out


# ---------------------------------------------------------------- 2. the passes layout
@pytest.mark.parametrize("fold", ["default", "5", "2"])  # passes walked by one work-group (NORI_GATHER_PASSES)
@pytest.mark.parametrize("case", [("gaussian", 72, 56), ("box", 33, 31), ("box", 72, 56), ("tent", 33, 31), ("mitchell", 33, 31),
                                  ("gaussian3", 33, 31), ("gaussian45", 33, 31)], ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}")
def test_passes_layout_against_the_statement(built, tmp_path_factory, monkeypatch, case, fold):
    """1, 3 and 5 passes, so that a work-group's pass range is not a multiple of the kernel's ring
    depth (4); small frames have few blocks, so by default a work-group walks one pass:
    NORI_GATHER_PASSES = 5 makes one work-group walk all of them, 2 gives ranges of 2, 2 and 1."""
    name, W, H = case
    s, rad, tab, grad = scene_of(tmp_path_factory, name, W, H)
    po, vo = ordered(W, H)
    full = ordered_ref(name, W, H, rad, tab, grad)
    # the same samples flattened: the owner is the floor of the position there
    flat = cached(("flat", name, W, H), lambda: G.gather_ref(W, H, rad, tab, po, grad, vo))
    if fold != "default":
        monkeypatch.setenv("NORI_GATHER_PASSES", fold)
    with nori_amd.GpuRenderer(s, 0) as r:
        for k in (1, 3, 5):
            ref = head(full, k * W * H)
            rows = r.film_gather_passes(po[:k], grad, vo[:k], passes=k)
            assert rows.shape == (k, H, W, 3) and counts_of(r) == ref["counts"], k
            assert ref["counts"][1] == 9  # the outside-pixel and invalid samples of pass 0
            G.assert_within_bound(rows, ref, f"{name} {W}x{H} passes={k} fold={fold}")
            # ... and film_gather of the same samples flattened, against its own restatement; a
            # sample whose owner is the same pixel in both layouts has the same terms in both
            fref = head(flat, k * W * H)
            frows = r.film_gather(po[:k].reshape(-1, 2), grad, vo[:k].reshape(-1, 3))
            assert counts_of(r) == fref["counts"]
            G.assert_within_bound(frows, fref, f"{name} {W}x{H} passes={k} flattened")
            pix = np.tile(np.stack(np.mgrid[0:H, 0:W][::-1], -1).reshape(-1, 2), (k, 1))
            own = ref["kept"] & fref["kept"] & (np.floor(po[:k].reshape(-1, 2)) == pix).all(1)
            assert own.sum() >= 0.95 * k * W * H
            assert np.array_equal(ref["S"][own], fref["S"][own])
            gap = np.abs(rows.reshape(-1, 3)[own].astype(np.float64) - frows[own])
            assert (gap <= 2 * G.bound(ref)[own]).all()


# ---------------------------------------------------------------- 3. block subsets
def test_block_subsets_leave_the_other_rows_untouched(built, tmp_path_factory):
    torch = pytest.importorskip("torch")
    W, H, P = 72, 56, 2
    s, rad, tab, grad = scene_of(tmp_path_factory, "gaussian", W, H)
    po, vo = ordered(W, H)
    po, vo = po[:P], vo[:P]
    ref = head(ordered_ref("gaussian", W, H, rad, tab, grad), P * W * H)
    nb = s.num_blocks()
    assert nb == 6
    ys, xs = np.mgrid[0:H, 0:W]
    block_of = (ys // 32) * 3 + xs // 32
    nan = np.array([0x7FC00123], np.uint32).view(f32)[0]  # a NaN with a payload: "untouched" is checked bit for bit
    tg = torch.from_numpy(grad).cuda()
    with nori_amd.GpuRenderer(s, 0) as r:
        for device in (False, True):
            for ids in (list(range(0, nb, 2)), list(range(1, nb, 2)), [4]):
                sel = np.isin(block_of, ids)
                p, v = po.copy(), vo.copy()
                p[:, ~sel], v[:, ~sel] = np.nan, np.nan  # the unselected entries are never used
                out = np.full((P, H, W, 3), nan, f32)
                if device:
                    tp, tv, to = torch.from_numpy(p).cuda(), torch.from_numpy(v).cuda(), torch.from_numpy(out).cuda()
                    torch.cuda.synchronize()
                    assert r.film_gather_passes(tp, tg, tv, passes=P, blocks=ids, out=to) is None
                    out = to.cpu().numpy()
                else:
                    assert r.film_gather_passes(p, grad, v, passes=P, blocks=ids, out=out) is out
                assert sum(counts_of(r)) == P * int(sel.sum())
                assert (_bits(out[:, ~sel]) == 0x7FC00123).all()
                assert np.isfinite(out[:, sel]).all()
                full = np.where(sel[None, :, :, None], out, ref["out"].reshape(P, H, W, 3))
                G.assert_within_bound(full, ref, f"blocks {ids}, device={device}")
        with pytest.raises(nori_amd.NoriError):
            r.film_gather_passes(po, grad, vo, passes=P, blocks=[nb])


# ---------------------------------------------------------------- 4. host and device forms
def test_device_arrays_and_chunked_host_arrays(built, tmp_path_factory, monkeypatch):
    torch = pytest.importorskip("torch")
    W, H = 72, 56
    s, rad, tab, grad = scene_of(tmp_path_factory, "gaussian", W, H)
    pos, val = R.scattered_inputs(W, H)
    ref = scattered_ref("gaussian", W, H, rad, tab, grad)
    po, vo = ordered(W, H)
    po, vo = po[:3], vo[:3]
    ref_o = head(ordered_ref("gaussian", W, H, rad, tab, grad), 3 * W * H)
    with nori_amd.GpuRenderer(s, 0) as r:
        host = r.film_gather(pos, grad, val)
        G.assert_within_bound(host, ref, "scattered, host arrays")
        host0 = r.film_gather(pos, grad)
        host_o = r.film_gather_passes(po, grad, vo, passes=3)
        G.assert_within_bound(host_o, ref_o, "passes, host arrays")
        host_o0 = r.film_gather_passes(po, grad, passes=3)
        # torch tensors: the same rows bit for bit
        tg = torch.from_numpy(grad).cuda()
        tp, tv = torch.from_numpy(pos).cuda(), torch.from_numpy(val).cuda()
        out = torch.full((pos.shape[0], 3), 7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert r.film_gather(tp, tg, tv, out=out) is None
        assert counts_of(r) == ref["counts"]
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(host))
        assert r.film_gather(tp, tg, out=out) is None  # val=None
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(host0))
        # int device addresses with n=
        out.fill_(7.0)
        torch.cuda.synchronize()
        assert r.film_gather(tp.data_ptr(), tg.data_ptr(), tv.data_ptr(), n=pos.shape[0], out=out.data_ptr()) is None
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(host))
        tp, tv = torch.from_numpy(po).cuda(), torch.from_numpy(vo).cuda()
        out = torch.full((3, H, W, 3), 7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert r.film_gather_passes(tp, tg, tv, passes=3, out=out) is None
        assert counts_of(r) == ref_o["counts"]
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(host_o))
        assert r.film_gather_passes(tp, tg, passes=3, out=out) is None
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(host_o0))
        with pytest.raises(ValueError):
            r.film_gather(tp, tg, tv)  # device arrays need a device out=
        with pytest.raises(ValueError):
            r.film_gather(pos, tg, val)  # mixed
        # host arrays across chunk boundaries: 2000 samples in chunks of 1000; one pass (4032 samples) per chunk
        monkeypatch.setenv("NORI_QUERY_CHUNK", "1000")
        rows = r.film_gather(pos, grad, val)
        assert counts_of(r) == ref["counts"] and np.array_equal(_bits(rows), _bits(host))
        assert np.array_equal(_bits(r.film_gather(pos, grad)), _bits(host0))
        rows = r.film_gather_passes(po, grad, vo, passes=3)
        assert counts_of(r) == ref_o["counts"] and np.array_equal(_bits(rows), _bits(host_o))
        assert np.array_equal(_bits(r.film_gather_passes(po, grad, passes=3)), _bits(host_o0))


# ---------------------------------------------------------------- 5. the adjoint identity
@pytest.mark.parametrize("case", [("box", 33, 31), ("gaussian", 72, 56), ("gaussian45", 33, 31)], ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}")
def test_adjoint_identity_on_the_device(built, tmp_path_factory, case):
    name, W, H = case
    s, rad, tab, grad = scene_of(tmp_path_factory, name, W, H)
    pos, val = R.scattered_inputs(W, H)
    ref = scattered_ref(name, W, H, rad, tab, grad)
    fwd = R.splat_ref(W, H, rad, tab, pos, val, want_stats=False)
    po, vo = ordered(W, H)
    po, vo = po[:3], vo[:3]
    ref_o = head(ordered_ref(name, W, H, rad, tab, grad), 3 * W * H)
    fwd_o = R.splat_ref(W, H, rad, tab, po, vo, ordered=True, want_stats=False)
    with nori_amd.GpuRenderer(s, 0) as r:
        G.adjoint_check(r.film_splat(pos, val), grad, val, r.film_gather(pos, grad, val), ref, fwd["m"], f"{name} scattered")
        G.adjoint_check(r.film_splat_passes(po, vo, passes=3), grad, vo, r.film_gather_passes(po, grad, vo, passes=3), ref_o,
                        fwd_o["m"], f"{name} passes")


# ---------------------------------------------------------------- 6. autograd
def test_autograd_backward_is_the_gather(built, tmp_path_factory):
    torch = pytest.importorskip("torch")
    from nori_amd import autograd as A
    W, H, P = 72, 56, 2
    s, rad, tab, grad = scene_of(tmp_path_factory, "gaussian", W, H)
    po, vo = ordered(W, H)
    po, vo = po[:P], vo[:P]
    g1 = np.random.default_rng(3).standard_normal(s.film_shape()).astype(f32)
    g2 = np.random.default_rng(4).standard_normal(s.film_shape()).astype(f32)
    with nori_amd.GpuRenderer(s, 0) as r:
        want1, want2 = r.film_gather_passes(po, g1, vo, passes=P), r.film_gather_passes(po, g2, vo, passes=P)
        pos = torch.from_numpy(po).cuda().requires_grad_(True)
        val = torch.from_numpy(vo).cuda().requires_grad_(True)
        film = A.film_splat_passes(r, pos, val, passes=P)
        assert film.requires_grad and tuple(film.shape) == s.film_shape() and film.dtype == torch.float32
        R.assert_within_bound(film.detach().cpu().numpy(), R.splat_ref(W, H, rad, tab, po, vo, ordered=True, want_stats=False),
                              "autograd forward")
        film.backward(torch.from_numpy(g1).cuda())
        assert pos.grad is None
        assert np.array_equal(_bits(val.grad.cpu().numpy()), _bits(want1))
        # two uses in one graph accumulate
        val.grad = None
        f1, f2 = A.film_splat_passes(r, pos, val, passes=P), A.film_splat_passes(r, pos, val, passes=P)
        ((f1 * torch.from_numpy(g1).cuda()).sum() + (f2 * torch.from_numpy(g2).cuda()).sum()).backward()
        assert np.array_equal(_bits(val.grad.cpu().numpy()), _bits(want1 + want2))
        # a block subset: the other blocks' samples get a zero gradient
        val.grad = None
        A.film_splat_passes(r, pos, val, passes=P, blocks=[1, 4]).backward(torch.from_numpy(g1).cuda())
        ys, xs = np.mgrid[0:H, 0:W]
        sel = np.isin((ys // 32) * 3 + xs // 32, [1, 4])
        got = val.grad.cpu().numpy()
        assert not got[:, ~sel].any() and np.array_equal(_bits(got[:, sel]), _bits(want1[:, sel]))
        # the scattered call
        ps, vs = R.scattered_inputs(W, H)
        want = r.film_gather(ps, g1, vs)
        val = torch.from_numpy(vs).cuda().requires_grad_(True)
        A.film_splat(r, torch.from_numpy(ps).cuda(), val).backward(torch.from_numpy(g1).cuda())
        assert np.array_equal(_bits(val.grad.cpu().numpy()), _bits(want))


def test_autograd_develop(built):
    torch = pytest.importorskip("torch")
    from nori_amd import autograd as A
    s = nori_amd.load_scene(scene_path("pa4", "cbox", "cbox_path_mis.xml"), 72, 56, 2)
    with nori_amd.GpuRenderer(s, 0) as r:
        film = r.render(passes=2, blocks=[0, 4])  # the other blocks' cells keep w == 0
    want = nori_amd.develop(s, film)
    b = s.border
    assert (film[b:-b, b:-b, 3] == 0).sum() > 500 and want.max() > 0
    t = torch.from_numpy(film).cuda().requires_grad_(True)
    img = A.develop(s, t)
    assert img.dtype == torch.float32 and np.array_equal(_bits(img.detach().cpu().numpy()), _bits(want))
    (img * img).sum().backward()
    g = t.grad.cpu().numpy()
    assert np.isfinite(g).all() and g[b:-b, b:-b][film[b:-b, b:-b, 3] != 0].any()
    assert not g[b:-b, b:-b][film[b:-b, b:-b, 3] == 0].any()


# ---------------------------------------------------------------- 7. refusals
def test_refusals_leave_the_context_usable(built, tmp_path_factory, tmp_path):
    """After every group of refusals the gather's rows equal the ones before bit for bit (it has no
    atomics), and a render equals the one before up to the order of its float atomics: at one pass
    a film float is a sum of non-negative terms, one per pixel within radius + 0.5 of its cell --
    at most 6 x 6 = 36 <= 64 for the gaussian of radius 2 -- so two orders of the m terms differ
    by at most 2 m 2^-24 of the value."""
    torch = pytest.importorskip("torch")
    W, H = 33, 31
    s, rad, tab, grad = scene_of(tmp_path_factory, "gaussian", W, H)
    pos, val = R.scattered_inputs(W, H)
    n = pos.shape[0]
    lib = nori_amd.lib()
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    out = np.full((n, 3), 5, f32)
    po, vo, oo = np.zeros((H, W, 2), f32), np.zeros((H, W, 3), f32), np.full((H, W, 3), 5, f32)
    with nori_amd.GpuRenderer(s, 0) as r:
        rows0, film0 = r.film_gather(pos, grad, val), r.render(passes=1)

        def still_works():
            assert np.array_equal(_bits(r.film_gather(pos, grad, val)), _bits(rows0))
            assert np.allclose(r.render(passes=1), film0, rtol=2 * 64 * 2.0 ** -24, atol=0)
            assert (out == 5).all() and (oo == 5).all()

        gd, rd = _abi.GatherDesc(n, 0, 0), _abi.RenderDesc()
        rd.pass_count = 1
        spare = out.copy()
        assert lib.nori_gpu_film_gather(r._h, C.byref(gd), p(pos), None, p(grad), p(spare), None) == 0  # val may be NULL
        assert (spare != 5).any()
        for args in [(None, C.byref(gd), p(pos), p(val), p(grad), p(out), None), (r._h, None, p(pos), p(val), p(grad), p(out), None),
                     (r._h, C.byref(gd), None, p(val), p(grad), p(out), None), (r._h, C.byref(gd), p(pos), p(val), None, p(out), None),
                     (r._h, C.byref(gd), p(pos), p(val), p(grad), None, None)]:
            assert lib.nori_gpu_film_gather(*args) == -1
        for args in [(None, C.byref(rd), p(po), p(vo), p(grad), p(oo), None), (r._h, None, p(po), p(vo), p(grad), p(oo), None),
                     (r._h, C.byref(rd), None, p(vo), p(grad), p(oo), None), (r._h, C.byref(rd), p(po), p(vo), None, p(oo), None),
                     (r._h, C.byref(rd), p(po), p(vo), p(grad), None, None)]:
            assert lib.nori_gpu_film_gather_passes(*args) == -1
        still_works()
        bad = _abi.GatherDesc(n, 0, 1)  # reserved != 0
        assert lib.nori_gpu_film_gather(r._h, C.byref(bad), p(pos), p(val), p(grad), p(out), None) == -1
        assert "reserved" in lib.nori_gpu_last_error().decode()
        still_works()
        # on_device with a misaligned or a host pointer
        tp, tv, tg = torch.from_numpy(pos).cuda(), torch.from_numpy(val).cuda(), torch.from_numpy(grad).cuda()
        to = torch.full((n, 3), 5.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        dev = _abi.GatherDesc(n - 1, 1, 0)
        good = (tp.data_ptr(), tv.data_ptr(), tg.data_ptr(), to.data_ptr())
        assert lib.nori_gpu_film_gather(r._h, C.byref(dev), *map(C.c_void_p, good), None) == 0
        to.fill_(5.0)
        torch.cuda.synchronize()
        for k, off in [(0, 2), (1, 2), (2, 4), (2, 8), (3, 2)]:
            a = list(good)
            a[k] += off
            assert lib.nori_gpu_film_gather(r._h, C.byref(dev), *map(C.c_void_p, a), None) == -1
        for k, host in [(0, pos), (1, val), (2, grad), (3, out)]:
            a = list(good)
            a[k] = host.ctypes.data
            assert lib.nori_gpu_film_gather(r._h, C.byref(dev), *map(C.c_void_p, a), None) == -1
        rdev = _abi.RenderDesc()
        rdev.pass_count, rdev.output_on_device = 1, 1
        assert lib.nori_gpu_film_gather_passes(r._h, C.byref(rdev), p(po), p(vo), C.c_void_p(tg.data_ptr()),
                                               C.c_void_p(to.data_ptr()), None) == -1
        assert (to == 5).all().item()
        still_works()
        # a block id out of range
        ids = np.array([s.num_blocks()], np.uint32)
        rd.num_blocks, rd.block_ids = 1, ids.ctypes.data_as(C.POINTER(C.c_uint32))
        assert lib.nori_gpu_film_gather_passes(r._h, C.byref(rd), p(po), p(vo), p(grad), p(oo), None) == -1
        still_works()
        # a border above 4 is refused as by the splat: no context exists for such a scene (nori_gpu_create
        # refuses it, so the calls' own check is a second line); the host statement has no such limit
        wide = nori_amd.load_scene(R.filter_scene_xml(tmp_path, '<rfilter type="gaussian"><float name="radius" value="5.5"/></rfilter>'),
                                   W, H, 1)
        assert wide.border == 5
        with pytest.raises(nori_amd.NoriError, match="radius above 4.5"):
            nori_amd.GpuRenderer(wide, 0)
        still_works()
        gw = G.seeded_grad(wide.film_shape())
        rows, counts = nori_amd.film_gather(wide, pos, gw, val)
        ref = G.gather_ref(W, H, *R.scene_filter(wide), pos, gw, val)
        assert counts == ref["counts"] and np.array_equal(_bits(rows), _bits(ref["out"])) and ref["m"].max() > 100


# ---------------------------------------------------------------- 8. the example
def _example():
    spec = importlib.util.spec_from_file_location("fit_albedo_torch", os.path.join(ROOT, "examples", "fit_albedo_torch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fit_albedo_gradient_against_central_differences(built):
    """The autograd gradient of the example's loss against the central difference at h = 0.25, for
    the two diffuse shapes with the most samples and one channel each, at ratio = 1.3 there and 1
    elsewhere.  The loss is quadratic in ratio, so the central difference is exact up to the
    rounding of float32 image values summed in float64; the cap is |fd - grad| <= 1e-3 max|grad|,
    which any missing factor would break by O(1).  Observed on an MI355X: |fd - grad| / max|grad| =
    1.5e-07 (shape 0, red) and 8.1e-10 (shape 2, blue)."""
    torch = pytest.importorskip("torch")
    mod = _example()
    s = nori_amd.load_scene(scene_path("pa4", "cbox", "cbox_path_mis.xml"), 48, 48, 2)
    with nori_amd.GpuRenderer(s, 0) as r:
        data = mod.prepare(r, 2, 0)
        ns = len(s.shapes())
        assert tuple(data["pos"].shape) == (2, 48, 48, 2) and tuple(data["shape"].shape) == (2, 48, 48)
        seen = torch.bincount(data["shape"].reshape(-1), minlength=ns + 1)[:ns] * data["diffuse"]
        picks = [(int(i), c) for i, c in zip(torch.argsort(seen, descending=True)[:2].tolist(), (0, 2))]
        assert all(seen[i] > 100 for i, _ in picks)
        ones = torch.ones((ns, 3), device="cuda")
        with torch.no_grad():
            target = mod.image(r, data, ones)
        assert target.max() > 0 and float(mod.loss(r, data, ones, target)) < 1e-8  # (up to the order of the film's atomics)
        ratio = ones.clone()
        for i, c in picks:
            ratio[i, c] = 1.3
        ratio.requires_grad_(True)
        mod.loss(r, data, ratio, target).backward()
        grad = ratio.grad.cpu().numpy().astype(np.float64)
        assert np.isfinite(grad).all() and not grad[~data["diffuse"].cpu().numpy()].any()
        cap = 1e-3 * np.abs(grad).max()
        for i, c in picks:
            e = torch.zeros_like(ones)
            e[i, c] = 0.25
            with torch.no_grad():
                fd = (float(mod.loss(r, data, ratio + e, target)) - float(mod.loss(r, data, ratio - e, target))) / 0.5
            print(f"shape {i} channel {c}: grad {grad[i, c]:.9e}, central difference {fd:.9e}, "
                  f"|fd - grad| / max|grad| = {abs(fd - grad[i, c]) / np.abs(grad).max():.3e}")
            assert grad[i, c] > 0 and abs(fd - grad[i, c]) <= cap, (i, c, fd, grad[i, c])


def test_fit_albedo_command_line(built, monkeypatch, capsys):
    pytest.importorskip("torch")
    mod = _example()
    monkeypatch.setattr("sys.argv", ["fit_albedo_torch.py", scene_path("pa4", "cbox", "cbox_path_mis.xml"), "--spp", "2",
                                     "--steps", "20", "--width", "48", "--height", "48"])
    first, last = mod.main()
    text = capsys.readouterr().out
    assert "48x48, 2 spp, 20 steps of Adam" in text and "shape 0: ratio" in text
    assert 0 <= last < first
