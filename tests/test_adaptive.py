"""Adaptive sampling, host side: the nori_gpu_adaptive_desc layout and the
block error metric nori_film_block_error against a numpy restatement.

The metric (include/nori_gpu.h, at nori_film_block_error), restated here in
float64 with a plain loop over sub-tiles: per pixel with statistics
(S1_c, S2_c, n): e_p = 0 if n < 2, else with m_c = S1_c / n and
v_c = max(0, S2_c - S1_c^2 / n) / (n (n - 1)),
e_p = sqrt(v_r + v_g + v_b) / sqrt(m_r + m_g + m_b + 1e-3); per 32x32 block
E_b = the maximum over its 8x8 sub-tiles (tiled from the block's origin) of the
mean of e_p over the sub-tile's pixels inside the frame.

tests/test_gpu_adaptive.py imports the restatement, the schedule and the
synthetic statistics from here.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import nori_amd
from nori_amd import _abi
from conftest import ROOT, scene_path

HEADER = os.path.join(ROOT, "include", "nori_gpu.h")
BS, SUB = 32, 8
SHAPES = [(70, 52),   # sub-tiles 6 wide and 4 high at the frame's edge
          (33, 9),    # a block column one pixel wide
          (8, 8),     # a single sub-tile
          (96, 64)]   # exact tiling


def np_pixel_error(stats):
    """e_p of (H, W, 8) statistics, float64."""
    st = np.asarray(stats, np.float64)
    n = st[..., 6]
    ok = n >= 2
    nn = np.where(ok, n, 2.0)
    v = np.zeros(n.shape)
    m = np.zeros(n.shape)
    for c in range(3):
        s1, s2 = st[..., c], st[..., 3 + c]
        v += np.maximum(0.0, s2 - s1 * s1 / nn) / (nn * (nn - 1.0))
        m += s1 / nn
    return np.where(ok, np.sqrt(v) / np.sqrt(m + 1e-3), 0.0)


def np_block_error(stats):
    """E_b of every frame block (id = by * nbx + bx), float64."""
    e = np_pixel_error(stats)
    H, W = e.shape
    nbx, nby = (W + BS - 1) // BS, (H + BS - 1) // BS
    out = np.zeros(nbx * nby)
    for by in range(nby):
        for bx in range(nbx):
            worst = 0.0
            for ty in range(by * BS, min((by + 1) * BS, H), SUB):
                for tx in range(bx * BS, min((bx + 1) * BS, W), SUB):
                    tile = e[ty:min(ty + SUB, H), tx:min(tx + SUB, W)]
                    worst = max(worst, float(tile.mean()))
            out[by * nbx + bx] = worst
    return out


def np_schedule(error_after, blocks, min_passes, max_passes, threshold):
    """The round schedule of nori_gpu_render_adaptive.  error_after(k) = E_b of every frame block
    after k passes.  Returns ({block: passes}, [(block, passes, E_b) of every stop/continue
    decision taken below the cap])."""
    have, step, active = 0, min_passes, list(blocks)
    passes, decisions = {}, []
    while active:
        have += step
        for b in active:
            passes[b] = have
        if have >= max_passes:
            break
        e = error_after(have)
        decisions += [(b, have, float(e[b])) for b in active]
        active = [b for b in active if e[b] > threshold]
        step = min(have, max_passes - have)
    return passes, decisions


def synth_stats(W, H, seed=0, nmax=24):
    """(H, W, 8) float32 statistics of synthetic samples: per pixel n random RGB samples summed in
    float32, among them pixels with n = 0, n = 1, constant radiance and all-black samples."""
    rng = np.random.default_rng(seed)
    n = rng.integers(0, nmax + 1, size=(H, W))
    scale = rng.choice([0.02, 1.0, 30.0], size=(H, W, 1, 1))  # dim, mid, bright pixels
    L = (rng.random((H, W, nmax, 3)) * scale).astype(np.float32)
    kind = rng.integers(0, 8, size=(H, W))
    L[kind == 0] = np.float32([0.7, 0.3, 0.1])  # constant radiance: true variance 0, the clamp matters
    L[kind == 1] = 0.0                          # all black
    n[kind == 2] = 0
    n[kind == 3] = 1
    flat = n.ravel()
    flat[:4] = [0, 1, 16, 16]                   # each special kind is present whatever the draw
    Lf = L.reshape(H * W, nmax, 3)
    Lf[2] = np.float32([0.7, 0.3, 0.1])
    Lf[3] = 0.0
    st = np.zeros((H, W, 8), np.float32)
    for k in range(nmax):
        take = (k < n)[..., None]
        st[..., 0:3] += np.where(take, L[:, :, k], np.float32(0))
        st[..., 3:6] += np.where(take, L[:, :, k] * L[:, :, k], np.float32(0))
    st[..., 6] = n
    return st


def _scene(W, H):
    return nori_amd.load_scene(scene_path("pa4", "cbox", "cbox_path_mis.xml"), W, H, 1)


def test_adaptive_desc_layout_matches_c(built, tmp_path):
    cname, py = "nori_gpu_adaptive_desc", _abi.AdaptiveDesc
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             f'printf("{cname} %zu\\n", sizeof({cname}));']
    for fname, _ in py._fields_:
        lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    out = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                         check=True).stdout.split("\n") if l)
    assert int(out[cname]) == C.sizeof(py)
    assert [f for f, _ in py._fields_] == ["min_passes", "max_passes", "threshold", "reserved", "passes_out",
                                           "error_out"]
    for fname, _ in py._fields_:
        assert int(out[f"{cname}.{fname}"]) == getattr(py, fname).offset, fname
    assert _abi.ABI_VERSION == 7  # no existing signature or struct changed


@pytest.mark.parametrize("W,H", SHAPES)
def test_host_block_error_matches_numpy(built, W, H):
    st = synth_stats(W, H, seed=W * 1000 + H)
    n = st[..., 6]
    assert (n == 0).any() and (n == 1).any() and (n >= 2).any()
    got = nori_amd.block_error(_scene(W, H), st)
    want = np_block_error(st)
    assert got.shape == want.shape == (((W + 31) // 32) * ((H + 31) // 32),)
    assert want.max() > 0
    # the library returns float32: its double-precision value rounded once
    assert np.allclose(got.astype(np.float64), want.astype(np.float32).astype(np.float64), rtol=1e-12, atol=0.0)


def test_block_error_is_the_worst_sub_tile_not_the_block_mean(built):
    """One noisy pixel in an otherwise constant 32x32 block.  Constant pixels: 4 samples of 0.5 per
    channel (S1 = 2, S2 = 1, S2 - S1^2/n = 0 exactly).  The noisy pixel: samples 0, 0, 1, 1 per
    channel (S1 = 2, S2 = 2): v_c = (2 - 1) / 12, m_c = 0.5, e_p = sqrt(3/12) / sqrt(1.501), and E_b
    is e_p / 64 (its sub-tile's mean), not e_p / 1024."""
    st = np.zeros((32, 32, 8), np.float32)
    st[..., 0:3] = 2.0
    st[..., 3:6] = 1.0
    st[..., 6] = 4.0
    st[10, 19, 3:6] = 2.0
    e_p = np.sqrt(3.0 / 12.0) / np.sqrt(1.5 + 1e-3)
    got = nori_amd.block_error(_scene(32, 32), st)
    assert got.shape == (1,)
    assert np.isclose(float(got[0]), e_p / 64.0, rtol=1e-6, atol=0.0)  # fp32 output of a double value
    assert np.isclose(np_block_error(st)[0], e_p / 64.0, rtol=1e-12, atol=0.0)
