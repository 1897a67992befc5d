"""The film splat on the GPU: nori_gpu_film_splat (k_splat_scatter) and nori_gpu_film_splat_passes
(k_splat_pos), csrc/kernels_film.hip, stated at nori_film_splat in include/nori_gpu.h.

The device calls add the statement's float32 terms in another order, so every film is compared with
the float64 sum S of the numpy restatement (tests/film_splat_ref.py) under
|film - S| <= m 2^-24 A + 2^-120 (m terms of magnitude sum A per film float): no fitted tolerance,
no excluded pixels.

1. scattered samples; 2. the passes layout; 3. against the built-in film; 4. statistics; 5. block
subsets; 6. device (torch) arrays and chunked host arrays; 7. refusals; 8. examples/direct_torch.py."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import film_splat_ref as R
import nori_amd
from conftest import ROOT, scene_path
from nori_amd import _abi

pytestmark = pytest.mark.gpu
f32 = np.float32
FILTER = {f[0]: f for f in R.FILTERS}
_SCENES = {}


def scene_of(tmp_path_factory, name, W, H, spp=2):
    key = (name, W, H, spp)
    if key not in _SCENES:
        d = tmp_path_factory.mktemp(f"splat_{name}_{W}x{H}")
        s = nori_amd.load_scene(R.filter_scene_xml(d, FILTER[name][1]), W, H, spp)
        _SCENES[key] = (s,) + R.scene_filter(s)
    return _SCENES[key]


def counts_of(r):
    return (r.last_stats["samples"], r.last_stats["invalid_samples"])


def pixel_grid(W, H):
    ys, xs = np.mgrid[0:H, 0:W]
    return np.stack([xs, ys], -1).astype(f32)


# ---------------------------------------------------------------- 1. scattered
@pytest.mark.parametrize("frame", R.FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("filt", [f[0] for f in R.FILTERS])
def test_scattered_against_the_statement(built, tmp_path_factory, filt, frame):
    W, H = frame
    s, rad, tab = scene_of(tmp_path_factory, filt, W, H)
    pos, val = R.scattered_inputs(W, H)
    with nori_amd.GpuRenderer(s, 0) as r:
        for n in (1, 63, 64, 65, 1000):
            ref = R.splat_ref(W, H, rad, tab, pos[:n], val[:n], want_stats=False)
            film = r.film_splat(pos[:n], val[:n])
            assert counts_of(r) == ref["counts"] == nori_amd.film_splat(s, pos[:n], val[:n])[1], n
            assert r.last_stats["ms_splat"] > 0 and r.last_stats["ms_total"] > 0
            R.assert_within_bound(film, ref, f"{filt} {W}x{H} n={n}")
        # contention: 4096 samples inside one pixel (every film float of its window sums m = 4096 terms)
        rng = np.random.default_rng(7)
        px = np.array([min(40, W - 1), min(20, H - 1)], f32)
        cpos = (px + rng.random((4096, 2), dtype=f32)).astype(f32)
        cpos = np.minimum(cpos, np.nextafter(px + f32(1), f32(0)))
        cval = rng.uniform(0.0, 2.0, (4096, 3)).astype(f32)
        ref = R.splat_ref(W, H, rad, tab, cpos, cval, want_stats=False)
        assert ref["counts"] == (4096, 0) and ref["m"].max() == 4096
        film = r.film_splat(cpos, cval)
        assert counts_of(r) == (4096, 0)
        R.assert_within_bound(film, ref, f"{filt} {W}x{H} one pixel")
        # n == 0 is a no-op
        out = film.copy()
        assert r.film_splat(cpos[:0], cval[:0], out=out) is out and np.array_equal(out, film)


# ---------------------------------------------------------------- 2. the passes layout
@pytest.mark.parametrize("fold", ["default", "5", "2"])  # passes folded by one work-group (NORI_SPLAT_POS_PASSES)
@pytest.mark.parametrize("case", [("gaussian", 72, 56), ("box", 33, 31), ("box", 72, 56), ("tent", 33, 31), ("mitchell", 33, 31),
                                  ("gaussian3", 33, 31), ("gaussian45", 33, 31)], ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}")
def test_passes_layout_against_the_statement(built, tmp_path_factory, monkeypatch, case, fold):
    """1, 3 and 5 passes, so that a work-group's pass range is not a multiple of the kernel's prefetch
    depth (4); small frames have few blocks, so by default a work-group folds one pass: NORI_SPLAT_POS_PASSES
    = 5 makes one work-group fold all of them, 2 gives ranges of 2, 2 and 1."""
    name, W, H = case
    s, rad, tab = scene_of(tmp_path_factory, name, W, H)
    po, vo = _ordered(W, H)
    per_pass = _ordered_refs(name, W, H, rad, tab)
    if fold != "default":
        monkeypatch.setenv("NORI_SPLAT_POS_PASSES", fold)
    with nori_amd.GpuRenderer(s, 0) as r:
        for k in (1, 3, 5):
            ref = per_pass[0]
            for q in per_pass[1:k]:
                ref = R.add_refs(ref, q)
            film = r.film_splat_passes(po[:k], vo[:k], passes=k)
            assert counts_of(r) == ref["counts"], k
            assert ref["counts"][1] == 9  # the outside-pixel and invalid samples of pass 0
            R.assert_within_bound(film, ref, f"{name} {W}x{H} passes={k} fold={fold}")
        # the same samples (pass 0, with its far-edge samples) through film_splat: the owner is the floor there
        ref = _unordered_ref(name, W, H, rad, tab)
        film = r.film_splat(po[0].reshape(-1, 2), vo[0].reshape(-1, 3))
        assert counts_of(r) == ref["counts"]
        R.assert_within_bound(film, ref, f"{name} {W}x{H} pass 0 scattered")


_ORD = {}


def _ordered(W, H):
    if (W, H) not in _ORD:
        _ORD[W, H] = R.ordered_inputs(W, H, 5)
    return _ORD[W, H]


def _ordered_refs(name, W, H, rad, tab):
    key = ("ord", name, W, H)
    if key not in _ORD:
        po, vo = _ordered(W, H)
        _ORD[key] = [R.splat_ref(W, H, rad, tab, po[k], vo[k], ordered=True, want_stats=False) for k in range(5)]
    return _ORD[key]


def _unordered_ref(name, W, H, rad, tab):
    key = ("unord", name, W, H)
    if key not in _ORD:
        po, vo = _ordered(W, H)
        _ORD[key] = R.splat_ref(W, H, rad, tab, po[0], vo[0], want_stats=False)
    return _ORD[key]


# ---------------------------------------------------------------- 3. / 4. the built-in film and its statistics
@pytest.fixture(scope="module")
def builtin(built):
    """cbox_path_mis (default gaussian) at 72 x 56: position and radiance of every sample of passes 0-2 from
    public calls -- L from the one-pass statistics (they hold 0 + L; a count of 0 marks an invalid sample,
    which gets a NaN value so that the splat drops it too), pos = pixel + draws 0, 1 -- and the renders."""
    W, H, P = 72, 56, 3
    s = nori_amd.load_scene(scene_path("pa4", "cbox", "cbox_path_mis.xml"), W, H, P)
    pos, val = np.zeros((P, H, W, 2), f32), np.zeros((P, H, W, 3), f32)
    with nori_amd.GpuRenderer(s, 0) as r:
        for k in range(P):
            var = np.zeros((H, W, 8), f32)
            r.render(passes=1, pass_begin=k, variance=var)
            val[k] = np.where(var[..., 6:7] == 0, f32(np.nan), var[..., 0:3])
            pos[k] = pixel_grid(W, H) + r.sample_uniforms(0, 2, passes=1, pass_begin=k)[0]
        film3 = r.render(passes=3)
        var2 = np.zeros((H, W, 8), f32)
        r.render(passes=2, variance=var2)
    return s, pos, val, film3, var2


def test_passes_layout_against_the_builtin_film(builtin):
    s, pos, val, film3, _ = builtin
    W, H = s.width, s.height
    ref = R.splat_ref(W, H, *R.scene_filter(s), pos, val, ordered=True, want_stats=False)
    assert ref["counts"][0] >= 0.99 * 3 * W * H
    R.assert_within_bound(film3, ref, "render(passes=3) against S")
    with nori_amd.GpuRenderer(s, 0) as r:
        film = r.film_splat_passes(pos, val, passes=3)
        assert counts_of(r) == ref["counts"]
    R.assert_within_bound(film, ref, "film_splat_passes against S")


def test_statistics_equal_the_renders(builtin):
    s, pos, val, _, var2 = builtin
    var = np.zeros_like(var2)
    with nori_amd.GpuRenderer(s, 0) as r:
        r.film_splat_passes(pos[:2], val[:2], passes=2, variance=var)
        assert np.array_equal(var.view(np.uint32), var2.view(np.uint32))  # two addends commute
        assert var[..., 6].max() == 2 and var[..., 0:3].max() > 0
        # ... and the scattered call's, on the same samples
        var = np.zeros_like(var2)
        r.film_splat(pos[:2].reshape(-1, 2), val[:2].reshape(-1, 3), variance=var)
        assert np.array_equal(var.view(np.uint32), var2.view(np.uint32))


# ---------------------------------------------------------------- 5. block subsets
def test_block_subsets_tile_the_frame(built, tmp_path_factory):
    torch = pytest.importorskip("torch")
    W, H, P = 72, 56, 2
    s, rad, tab = scene_of(tmp_path_factory, "gaussian", W, H)
    po, vo = _ordered(W, H)
    po, vo = po[:P], vo[:P]
    per_pass = _ordered_refs("gaussian", W, H, rad, tab)
    ref = R.add_refs(per_pass[0], per_pass[1])
    nb = s.num_blocks()
    assert nb == 6
    bx, by = pixel_grid(W, H)[..., 0].astype(int) // 32, pixel_grid(W, H)[..., 1].astype(int) // 32
    block_of = by * 3 + bx
    with nori_amd.GpuRenderer(s, 0) as r:
        whole = r.film_splat_passes(po, vo, passes=P)
        R.assert_within_bound(whole, ref, "all blocks")
        for device in (False, True):
            film = torch.zeros(s.film_shape(), dtype=torch.float32, device="cuda") if device else np.zeros(s.film_shape(), f32)
            total = [0, 0]
            for ids in (list(range(0, nb, 2)), list(range(1, nb, 2))):
                sel = np.isin(block_of, ids)
                p, v = po.copy(), vo.copy()
                p[:, ~sel], v[:, ~sel] = np.nan, np.nan  # the unselected entries are never read
                if device:
                    tp, tv = torch.from_numpy(p).cuda(), torch.from_numpy(v).cuda()
                    torch.cuda.synchronize()
                    assert r.film_splat_passes(tp, tv, passes=P, blocks=ids, out=film) is None
                else:
                    assert r.film_splat_passes(p, v, passes=P, blocks=ids, out=film) is film
                assert sum(counts_of(r)) == P * int(sel.sum())
                total = [total[0] + counts_of(r)[0], total[1] + counts_of(r)[1]]
            assert tuple(total) == ref["counts"]
            R.assert_within_bound(film.cpu().numpy() if device else film, ref, f"even + odd blocks, device={device}")
        with pytest.raises(nori_amd.NoriError):
            r.film_splat_passes(po, vo, passes=P, blocks=[nb])


# ---------------------------------------------------------------- 6. device arrays, chunked host arrays
def test_device_arrays_and_chunked_host_arrays(built, tmp_path_factory, monkeypatch):
    torch = pytest.importorskip("torch")
    W, H = 72, 56
    s, rad, tab = scene_of(tmp_path_factory, "gaussian", W, H)
    pos, val = R.scattered_inputs(W, H)
    ref = R.splat_ref(W, H, rad, tab, pos, val)
    po, vo = _ordered(W, H)
    po, vo = po[:3], vo[:3]
    per_pass = _ordered_refs("gaussian", W, H, rad, tab)
    ref_o = R.add_refs(R.add_refs(per_pass[0], per_pass[1]), per_pass[2])
    with nori_amd.GpuRenderer(s, 0) as r:
        # torch tensors, the statistics on the device too
        film = torch.zeros(s.film_shape(), dtype=torch.float32, device="cuda")
        var = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda")
        tp, tv = torch.from_numpy(pos).cuda(), torch.from_numpy(val).cuda()
        torch.cuda.synchronize()
        assert r.film_splat(tp, tv, out=film, variance=var) is None
        assert counts_of(r) == ref["counts"]
        R.assert_within_bound(film.cpu().numpy(), ref, "scattered, device arrays")
        hvar = np.zeros((H, W, 8), f32)
        hfilm = r.film_splat(pos, val, variance=hvar)
        R.assert_within_bound(hfilm, ref, "scattered, host arrays")
        few = ref["stats"][..., 6] <= 2  # at most two addends: they commute, so the sums are the statement's bit for bit
        assert few.sum() > 1000
        for got in (var.cpu().numpy(), hvar):
            assert np.array_equal(got[few].view(np.uint32), ref["stats"][few].view(np.uint32))
        # int device addresses with n=
        film.zero_()
        torch.cuda.synchronize()
        assert r.film_splat(tp.data_ptr(), tv.data_ptr(), n=pos.shape[0], out=film.data_ptr()) is None
        R.assert_within_bound(film.cpu().numpy(), ref, "scattered, device addresses")
        film.zero_()
        tp, tv = torch.from_numpy(po).cuda(), torch.from_numpy(vo).cuda()
        torch.cuda.synchronize()
        assert r.film_splat_passes(tp, tv, passes=3, out=film) is None
        assert counts_of(r) == ref_o["counts"]
        R.assert_within_bound(film.cpu().numpy(), ref_o, "passes, device arrays")
        with pytest.raises(ValueError):
            r.film_splat(tp, tv)  # device arrays need a device film
        # host arrays across chunk boundaries: 2000 samples in chunks of 1000 and 999; whole passes of 4032
        for chunk in ("1000", "999"):
            monkeypatch.setenv("NORI_QUERY_CHUNK", chunk)
            out = r.film_splat(pos, val)
            assert counts_of(r) == ref["counts"]
            R.assert_within_bound(out, ref, f"scattered, host chunks of {chunk}")
        out = r.film_splat_passes(po, vo, passes=3)
        assert counts_of(r) == ref_o["counts"]
        R.assert_within_bound(out, ref_o, "passes, one pass per host chunk")
        monkeypatch.setenv("NORI_QUERY_CHUNK", str(2 * W * H + 5))
        out = r.film_splat_passes(po, vo, passes=3)
        R.assert_within_bound(out, ref_o, "passes, two passes per host chunk")


# ---------------------------------------------------------------- 7. refusals
def test_refusals_leave_the_context_usable(built, tmp_path_factory, tmp_path):
    torch = pytest.importorskip("torch")
    W, H = 33, 31
    s, rad, tab = scene_of(tmp_path_factory, "gaussian", W, H)
    pos, val = R.scattered_inputs(W, H)
    ref = R.splat_ref(W, H, rad, tab, pos, val, want_stats=False)
    n = pos.shape[0]
    lib = nori_amd.lib()
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    film = np.zeros(s.film_shape(), f32)
    with nori_amd.GpuRenderer(s, 0) as r:
        def still_works():
            R.assert_within_bound(r.film_splat(pos, val), ref, "after a refusal")
            assert not film.any()

        sd, rd = _abi.SplatDesc(n, 0, 0, None), _abi.RenderDesc()
        rd.pass_count = 1
        po, vo = np.zeros((H, W, 2), f32), np.zeros((H, W, 3), f32)
        for args in [(None, C.byref(sd), p(pos), p(val), p(film), None), (r._h, None, p(pos), p(val), p(film), None),
                     (r._h, C.byref(sd), None, p(val), p(film), None), (r._h, C.byref(sd), p(pos), None, p(film), None),
                     (r._h, C.byref(sd), p(pos), p(val), None, None)]:
            assert lib.nori_gpu_film_splat(*args) == -1
        for args in [(None, C.byref(rd), p(po), p(vo), p(film), None), (r._h, None, p(po), p(vo), p(film), None),
                     (r._h, C.byref(rd), None, p(vo), p(film), None), (r._h, C.byref(rd), p(po), None, p(film), None),
                     (r._h, C.byref(rd), p(po), p(vo), None, None)]:
            assert lib.nori_gpu_film_splat_passes(*args) == -1
        still_works()
        bad = _abi.SplatDesc(n, 0, 1, None)  # reserved != 0
        assert lib.nori_gpu_film_splat(r._h, C.byref(bad), p(pos), p(val), p(film), None) == -1
        assert "reserved" in lib.nori_gpu_last_error().decode()
        still_works()
        # on_device with a misaligned or a host pointer
        tp, tv = torch.from_numpy(pos).cuda(), torch.from_numpy(val).cuda()
        tf = torch.zeros(s.film_shape(), dtype=torch.float32, device="cuda")
        tvar = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        dev = _abi.SplatDesc(n - 1, 1, 0, None)
        good = (tp.data_ptr(), tv.data_ptr(), tf.data_ptr())
        for k, off in [(0, 2), (1, 2), (2, 4), (2, 8)]:
            a = list(good)
            a[k] += off
            assert lib.nori_gpu_film_splat(r._h, C.byref(dev), *map(C.c_void_p, a), None) == -1
        for k, host in [(0, pos), (1, val), (2, film)]:
            a = list(good)
            a[k] = host.ctypes.data
            assert lib.nori_gpu_film_splat(r._h, C.byref(dev), *map(C.c_void_p, a), None) == -1
        for v in (tvar.data_ptr() + 4, np.zeros((H, W, 8), f32).ctypes.data):
            dv = _abi.SplatDesc(n - 1, 1, 0, v)
            assert lib.nori_gpu_film_splat(r._h, C.byref(dv), *map(C.c_void_p, good), None) == -1
        rdev = _abi.RenderDesc()
        rdev.pass_count, rdev.output_on_device = 1, 1
        assert lib.nori_gpu_film_splat_passes(r._h, C.byref(rdev), p(po), p(vo), C.c_void_p(tf.data_ptr()), None) == -1
        assert not tf.any().item() and not tvar.any().item()
        still_works()
    # the passes layout with pass_count 0 on a scene of 0 spp: nothing to do
    src = open(R.filter_scene_xml(tmp_path, FILTER["gaussian"][1])).read()
    assert '<integer name="sampleCount" value="512"/>' in src
    zero = tmp_path / "cbox_0spp.xml"
    zero.write_text(src.replace('<integer name="sampleCount" value="512"/>', '<integer name="sampleCount" value="0"/>'))
    s0 = nori_amd.load_scene(str(zero), W, H, 0)
    assert s0.spp == 0
    with nori_amd.GpuRenderer(s0, 0) as r:
        with pytest.raises(nori_amd.NoriError):
            r.film_splat_passes(po, vo)
        R.assert_within_bound(r.film_splat_passes(po, vo, passes=1),
                              R.splat_ref(W, H, rad, tab, po, vo, ordered=True, want_stats=False), "0 spp scene, one pass")
        R.assert_within_bound(r.film_splat(pos, val), ref, "after the refusal")


# ---------------------------------------------------------------- 8. the example
def _example():
    spec = importlib.util.spec_from_file_location("direct_torch", os.path.join(ROOT, "examples", "direct_torch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_direct_film_example(built):
    """direct_film at 2 spp against the built-in direct_mis render of the same passes."""
    torch = pytest.importorskip("torch")
    mod = _example()
    W = H = 32
    s = nori_amd.load_scene(scene_path("pa3", "odyssey", "odyssey_mis.xml"), W, H, 2)
    with nori_amd.GpuRenderer(s, 0) as r:
        film = mod.direct_film(r, "mis", spp=2)
        assert film.is_cuda and tuple(film.shape) == s.film_shape() and film.dtype == torch.float32
        want = r.render(passes=2)
        # the example's inputs, for the restatement's m and A
        pos = np.stack([pixel_grid(W, H) + r.sample_uniforms(0, 2, passes=1, pass_begin=k)[0] for k in range(2)])
        val = np.stack([mod.sample_radiance(r, "mis", k).cpu().numpy().reshape(H, W, 3) for k in range(2)])
    ref = R.splat_ref(W, H, *R.scene_filter(s), pos, val, ordered=True, want_stats=False)
    assert ref["counts"][0] >= 0.99 * 2 * W * H and want[..., 3].max() > 0
    R.assert_within_bound(film.cpu().numpy(), ref, "direct_film against S")
    R.assert_within_bound(want, ref, "render(passes=2) against S")


def test_direct_torch_command_line_film(built, tmp_path, monkeypatch, capsys):
    pytest.importorskip("torch")
    mod = _example()
    png = str(tmp_path / "film.png")
    monkeypatch.setattr("sys.argv", ["direct_torch.py", scene_path("pa3", "odyssey", "odyssey_mis.xml"), png, "--spp", "2",
                                     "--integrator", "mis", "--width", "48", "--height", "32", "--film"])
    mod.main()
    assert "48x32, direct_mis, 2 spp" in capsys.readouterr().out
    img = nori_amd.read_image(png)
    assert img.shape == (32, 48, 3) and img.max() > 0
    # the developed built-in film of the same passes: the same image up to the order of the film's
    # additions, so at most one 8-bit step apart
    s = nori_amd.load_scene(scene_path("pa3", "odyssey", "odyssey_mis.xml"), 48, 32, 2)
    with nori_amd.GpuRenderer(s, 0) as r:
        want = nori_amd.ldr_bytes(nori_amd.develop(s, r.render(passes=2)))
    assert np.abs(img.astype(int) - want.astype(int)).max() <= 1
