"""Adaptive sampling on the GPU: the device block-error kernel
(nori_gpu_block_error) against the host function, and nori_gpu_render_adaptive
against compositions of plain renders -- a block that received k passes holds
exactly the samples of passes [pass_begin, pass_begin + k), so the adaptive
film equals one plain render() per distinct count on the blocks that have it.
The expected pass counts come from the CPU oracle's per-sample radiance on the
same WAVE streams, the numpy metric and the numpy schedule (test_adaptive.py).
"""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import nori_amd
import pyoracle
from conftest import ROOT, scene_path
from nori_amd import _abi
from test_adaptive import SHAPES, np_block_error, np_schedule, synth_stats

pytestmark = pytest.mark.gpu

CBOX = ("pa4", "cbox", "cbox_path_mis.xml")
W, H, MIN, MAX, THR = 70, 52, 8, 64, 0.10
# the device metric against the host function on identical fp32 inputs, the cancelling difference
# in fp64 on both sides: what remains is fp32 rounding through a square root, a divide and a
# 64-term mean, about 100 ulp
ERR_TOL = dict(rtol=1e-5, atol=1e-6)
# the same samples in another accumulation order (test_gpu_parity.py)
FILM_TOL = dict(rtol=1e-4, atol=1e-4)


def _oracle_pass_stats(s, passes, pass_begin=0, seed=0):
    """(passes, H, W, 7) float64: L, L^2 and validity of every sample, from the oracle
    (as test_gpu_outputs._oracle_stats, kept per pass)."""
    w, h = s.width, s.height
    ids = np.arange(pass_begin * w * h, (pass_begin + passes) * w * h, dtype=np.uint64)
    smp = pyoracle.OracleScene(s).wave_samples(ids, seed=seed)
    L = smp[:, 2:5].astype(np.float64).reshape(passes, h, w, 3)
    ok = np.all(np.isfinite(L) & (L >= 0), axis=-1, keepdims=True)
    L = np.where(ok, L, 0.0)
    return np.concatenate([L, L * L, ok.astype(np.float64)], axis=-1)


def _error_after(per_pass):
    def f(k):
        st = np.zeros(per_pass.shape[1:3] + (8,))
        st[..., 0:7] = per_pass[:k].sum(0)
        return np_block_error(st)
    return f


def _fit(decisions, thr, margin=0.10):
    """Every stop/continue decision at least `margin` (relative) away from the threshold."""
    return all(abs(e - thr) >= margin * thr for _, _, e in decisions)


def _compose(r, s, passes, **kw):
    """The film of plain renders: one call per distinct count on the blocks that have it."""
    film = np.zeros(s.film_shape(), np.float32)
    for k in sorted(set(int(p) for p in passes if p)):
        r.render(passes=k, blocks=[b for b, p in enumerate(passes) if p == k], out=film, **kw)
    return film


def _block_of_pixels(s):
    ys, xs = np.mgrid[0:s.height, 0:s.width]
    return (ys // 32) * ((s.width + 31) // 32) + xs // 32


@pytest.fixture(scope="module")
def cbox(built):
    s = nori_amd.load_scene(scene_path(*CBOX), W, H, MAX)
    with nori_amd.GpuRenderer(s, 0) as r:
        yield s, r


@pytest.fixture(scope="module")
def cbox_expected(cbox):
    """The oracle's pass map for (MIN, MAX, THR) and its decisions."""
    s, _ = cbox
    passes, decisions = np_schedule(_error_after(_oracle_pass_stats(s, MAX)), range(s.num_blocks()), MIN, MAX, THR)
    return [passes[b] for b in range(s.num_blocks())], decisions


@pytest.mark.parametrize("w,h", SHAPES)
def test_device_block_error_matches_host(built, w, h):
    torch = pytest.importorskip("torch")
    s = nori_amd.load_scene(scene_path(*CBOX), w, h, 1)
    st = synth_stats(w, h, seed=w * 1000 + h)
    want = nori_amd.block_error(s, st)
    assert want.max() > 0
    with nori_amd.GpuRenderer(s, 0) as r:
        got_host = r.block_error(st)
        dev = torch.from_numpy(st).to("cuda:0")
        torch.cuda.synchronize()
        got_dev = r.block_error(dev.data_ptr())
    print("max relative difference", np.max(np.abs(got_host - want) / np.maximum(want, 1e-30)))
    assert np.allclose(got_host, want, **ERR_TOL)
    assert np.allclose(got_dev, want, **ERR_TOL)


def test_adaptive_equals_composition(cbox, cbox_expected):
    s, r = cbox
    expected, decisions = cbox_expected
    print("oracle decisions (block, passes, E_b):", [(b, k, round(e, 3)) for b, k, e in decisions])
    assert _fit(decisions, THR), "input unfit: a decision within 10 % of the threshold"
    assert expected == [64, 64, 8, 32, 64, 8]
    st = np.zeros((H, W, 8), np.float32)
    film, passes, errors = r.render_adaptive(THR, min_passes=MIN, max_passes=MAX, variance=st)
    stats = r.last_stats
    print("passes", passes.tolist(), "errors", errors.tolist())
    assert passes.tolist() == expected
    assert np.allclose(film, _compose(r, s, passes), **FILM_TOL)
    n = st[..., 6]
    assert n.astype(np.float64).sum() == stats["samples"] - stats["invalid_samples"]
    assert stats["samples"] == sum(int(p) * int((_block_of_pixels(s) == b).sum()) for b, p in enumerate(passes))
    assert (n <= passes[_block_of_pixels(s)]).all()
    assert np.allclose(errors, nori_amd.block_error(s, st), **ERR_TOL)


def test_adaptive_extremes(cbox):
    s, r = cbox
    film, passes, _ = r.render_adaptive(0.0, min_passes=MIN, max_passes=MAX)
    assert (passes == MAX).all()
    assert np.allclose(film, r.render(passes=MAX), **FILM_TOL)
    film, passes, errors = r.render_adaptive(float("inf"), min_passes=MIN, max_passes=MAX)
    assert (passes == MIN).all()
    assert r.last_stats["samples"] == W * H * MIN
    assert np.allclose(film, r.render(passes=MIN), **FILM_TOL)
    assert (errors > 0).all()  # evaluated after the last (only) round too


def test_adaptive_argument_plumbing(cbox):
    s, r = cbox
    sel, kw = [0, 2, 5], dict(pass_begin=3, seed=7)
    st = np.zeros((H, W, 8), np.float32)
    film, passes, errors = r.render_adaptive(THR, min_passes=MIN, max_passes=MAX, blocks=sel, variance=st, **kw)
    assert all((passes[b] >= MIN) == (b in sel) and (passes[b] > 0) == (b in sel) for b in range(s.num_blocks()))
    assert all(errors[b] == 0 for b in range(s.num_blocks()) if b not in sel)
    assert np.allclose(film, _compose(r, s, passes, **kw), **FILM_TOL)
    assert (st[..., 6][~np.isin(_block_of_pixels(s), sel)] == 0).all()
    # the statistics are added into the caller's array, not written over it
    st1 = np.ones((H, W, 8), np.float32)
    _, passes1, _ = r.render_adaptive(THR, min_passes=MIN, max_passes=MAX, blocks=sel, variance=st1, **kw)
    assert passes1.tolist() == passes.tolist()
    assert np.allclose(st1 - 1.0, st, **FILM_TOL)
    # ... and so is the film
    film1 = np.ones(s.film_shape(), np.float32)
    r.render_adaptive(THR, min_passes=MIN, max_passes=MAX, blocks=sel, out=film1, **kw)
    assert np.allclose(film1 - 1.0, film, **FILM_TOL)


def test_adaptive_one_bounce(built):
    w, h, lo, hi = 48, 27, 4, 16
    s = nori_amd.load_scene(scene_path("pa3", "odyssey", "odyssey_mis.xml"), w, h, hi)
    assert s.integrator == "direct_mis"
    err = _error_after(_oracle_pass_stats(s, hi))
    thr = float(np.median(err(lo)))
    expected, decisions = np_schedule(err, range(s.num_blocks()), lo, hi, thr)
    fit = _fit(decisions, thr)
    print("threshold", thr, "decisions", decisions, "fit", fit)
    checked = 0
    with nori_amd.GpuRenderer(s, 0) as r:
        film, passes, errors = r.render_adaptive(thr, min_passes=lo, max_passes=hi)
        if fit:  # else a decision lies within 10 % of the threshold: the exact map is not asserted
            assert passes.tolist() == [expected[b] for b in range(s.num_blocks())]
            checked += 1
        assert set(passes.tolist()) <= {4, 8, 16}
        checked += 1
        assert r.last_stats["samples"] == sum(int(p) * int((_block_of_pixels(s) == b).sum())
                                              for b, p in enumerate(passes))
        checked += 1
        assert np.allclose(film, _compose(r, s, passes), **FILM_TOL)
        checked += 1
    assert checked >= 3  # no more than the exact-map condition is skipped


def test_adaptive_device_buffers(cbox):
    torch = pytest.importorskip("torch")
    s, r = cbox
    st = np.zeros((H, W, 8), np.float32)
    film, passes, errors = r.render_adaptive(THR, min_passes=MIN, max_passes=MAX, variance=st)
    dfilm = torch.zeros(s.film_shape(), dtype=torch.float32, device="cuda:0")
    dst = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    none, dpasses, derrors = r.render_adaptive(THR, min_passes=MIN, max_passes=MAX, device_ptr=dfilm.data_ptr(),
                                               variance=dst.data_ptr())
    torch.cuda.synchronize()
    assert none is None
    assert dpasses.tolist() == passes.tolist()
    assert np.allclose(dfilm.cpu().numpy(), film, **FILM_TOL)
    assert np.allclose(dst.cpu().numpy(), st, **FILM_TOL)
    assert np.allclose(derrors, errors, **ERR_TOL)


def test_adaptive_progress_and_cancel(built):
    """nori_gpu_progress rises over the whole call (it does not fall back to 0 at each round) and
    nori_gpu_cancel ends it with NORI_ERR_CANCELLED; the context renders normally afterwards."""
    import threading
    import time

    s = nori_amd.load_scene(scene_path(*CBOX), 512, 512, 1024)
    with nori_amd.GpuRenderer(s, 0) as r:
        r.render(passes=1)  # context warm
        err, seen = [], []

        def run():
            try:
                r.render_adaptive(0.0, min_passes=16, max_passes=1024)
            except nori_amd.NoriError as e:
                err.append(e)

        th = threading.Thread(target=run)
        t0 = time.time()
        th.start()
        # cancel once the third round is under way (16 + 16 of 1024 passes done), not after a fixed sleep
        while th.is_alive() and time.time() - t0 < 30:
            p = r.progress()
            if p < 1.0:
                seen.append(p)
            if 0.035 < p < 1.0:
                break
            time.sleep(0.001)
        r.cancel()
        th.join(timeout=60)
        assert not th.is_alive()
        print("progress polled", len(seen), "times, last", seen[-1:], "outcome", err)
        assert all(b >= a for a, b in zip(seen, seen[1:])), seen
        if seen and 0.035 < seen[-1] < 0.2:  # cancelled with the long rounds still to come
            assert err and err[0].code == _abi.NORI_ERR_CANCELLED, err
        else:  # the call ran ahead of the polling: a normal finish is possible
            assert not err or err[0].code == _abi.NORI_ERR_CANCELLED, err
        assert r.progress() == 1.0
        r.render(passes=1)
        assert r.last_stats["samples"] == 512 * 512 and r.progress() == 1.0


def test_cli_adaptive(built, tmp_path):
    src = os.path.dirname(scene_path(*CBOX))
    dst = tmp_path / "cbox"
    shutil.copytree(src, dst)
    xml = str(dst / "cbox_path_mis.xml")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "nori-ray-tracer_amd"))
    cmd = [sys.executable, "-m", "nori_amd", xml, "--adaptive", "0.10", "--min-spp", "8", "--spp", "32",
           "--width", "70", "--height", "52"]
    p = subprocess.run(cmd + ["--png"], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr
    assert "Adaptive sampling:" in p.stdout and f"of {70 * 52 * 32} samples" in p.stdout
    for name in ("cbox_path_mis.exr", "cbox_path_mis_variance.exr", "cbox_path_mis_samples.exr", "cbox_path_mis.png"):
        assert (dst / name).exists(), name
    img = nori_amd.read_exr(str(dst / "cbox_path_mis.exr"))
    smp = nori_amd.read_exr(str(dst / "cbox_path_mis_samples.exr"))
    assert img.shape == smp.shape == (52, 70, 3)
    assert smp.min() >= 0 and smp.max() <= 32
    assert np.array_equal(smp[..., 0], smp[..., 1]) and np.array_equal(smp[..., 0], smp[..., 2])
    block_counts = {float(smp[by * 32:(by + 1) * 32, bx * 32:(bx + 1) * 32, 0].max()) for by in range(2)
                    for bx in range(3)}
    assert len(block_counts) >= 2, block_counts
    assert img.mean() > 0.05
    # adaptive rendering runs on one GPU
    p = subprocess.run(cmd + ["--gpus", "2"], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode != 0 and "one GPU" in p.stderr


@pytest.mark.parametrize("kw", [dict(threshold=0.1, min_passes=1), dict(threshold=0.1, min_passes=8, max_passes=4),
                                dict(threshold=-0.5), dict(threshold=float("nan"))])
def test_adaptive_invalid_arguments(cbox, kw):
    _, r = cbox
    with pytest.raises(nori_amd.NoriError) as e:
        r.render_adaptive(**kw)
    assert e.value.code == _abi.NORI_ERR_INVALID


def test_adaptive_reserved_must_be_zero(cbox):
    import ctypes as C

    s, r = cbox
    rd, ad, st = _abi.RenderDesc(), _abi.AdaptiveDesc(), _abi.Stats()
    ad.min_passes, ad.max_passes, ad.threshold, ad.reserved = 8, 16, 0.1, 1
    film = np.zeros(s.film_shape(), np.float32)
    rc = nori_amd.lib().nori_gpu_render_adaptive(r._h, C.byref(rd), C.byref(ad), film.ctypes.data_as(C.c_void_p),
                                                 C.byref(st))
    assert rc == _abi.NORI_ERR_INVALID and b"reserved" in nori_amd.lib().nori_gpu_last_error()
    assert not film.any()
