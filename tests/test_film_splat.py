"""nori_film_splat, the host statement of the film splat, on the CPU:
1. against its numpy restatement (tests/film_splat_ref.py) bit for bit -- both add in index
   order -- for every filter and border, a frame with partial blocks, scattered samples with all
   the special positions and values, and the ordered layout; counts and statistics too;
2. anchored to the reference's restatement: the oracle's own samples (position and radiance of
   every sample id of four passes) through nori_film_splat(ordered) against the oracle's render of
   those passes, which merges block tiles -- another grouping of the same terms -- under the
   bound m 2^-24 A + 2^-120 derived in film_splat_ref.py;
3. refusals, the ABI version, the ctypes mirror against the C layout."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import film_splat_ref as R
import nori_amd
import pyoracle
from conftest import ROOT, scene_path
from nori_amd import _abi

f32 = np.float32
HEADER = os.path.join(ROOT, "include", "nori_gpu.h")
CALLS = ("nori_film_splat", "nori_gpu_film_splat", "nori_gpu_film_splat_passes")


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.mark.parametrize("frame", R.FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("filt", R.FILTERS, ids=lambda f: f[0])
def test_host_statement_matches_the_numpy_restatement(built, tmp_path, filt, frame):
    name, rfilter, border = filt
    W, H = frame
    s = nori_amd.load_scene(R.filter_scene_xml(tmp_path, rfilter), W, H, 2)
    rad, tab = R.scene_filter(s)
    assert s.film_shape() == (H + 2 * border, W + 2 * border, 4)
    # scattered: 2000 seeded samples with the special positions and values
    pos, val = R.scattered_inputs(W, H)
    ref = R.splat_ref(W, H, rad, tab, pos, val)
    assert ref["border"] == border and ref["counts"][1] >= 20 and ref["counts"][0] >= 1500
    var = np.zeros((H, W, 8), f32)
    film, counts = nori_amd.film_splat(s, pos, val, variance=var)
    assert counts == ref["counts"] and sum(counts) == 2000
    assert np.array_equal(_bits(film), _bits(ref["film"]))
    assert np.array_equal(_bits(var), _bits(ref["stats"]))
    # ... added into a film and statistics that already hold something: the same additions again
    film2, _ = nori_amd.film_splat(s, pos, val, out=film.copy())
    again = R.splat_ref(W, H, rad, tab, np.concatenate([pos, pos]), np.concatenate([val, val]))
    assert np.array_equal(_bits(film2), _bits(again["film"]))
    # the ordered layout at 2 passes, with far-edge (kept) and outside-pixel (dropped) samples
    po, vo = R.ordered_inputs(W, H, 2)
    ref = R.splat_ref(W, H, rad, tab, po, vo, ordered=True)
    assert ref["counts"][1] == 9  # 6 positions and 3 values
    var = np.zeros((H, W, 8), f32)
    film, counts = nori_amd.film_splat(s, po, vo, ordered=True, variance=var)
    assert counts == ref["counts"]
    assert np.array_equal(_bits(film), _bits(ref["film"]))
    assert np.array_equal(_bits(var), _bits(ref["stats"]))
    assert var[2, 3, 6] == 2 and var[3, 7, 6] == 1  # a far-edge sample counts in its owner; a dropped one does not


def test_far_edge_sample_reaches_past_the_pixel_window(built, tmp_path):
    """The box filter (radius + 0.5 = 1): a sample exactly on its pixel's far edge is kept by the
    ordered layout and belongs to its owner's block, so on a block's last column it is clipped to the
    block's tile where the unordered layout, whose owner is the next pixel, puts it into the next block."""
    W, H = 72, 56
    s = nori_amd.load_scene(R.filter_scene_xml(tmp_path, R.FILTERS[0][1]), W, H, 1)
    pos = np.zeros((H, W, 2), f32)
    pos[..., 0], pos[..., 1] = np.arange(W)[None, :] + 0.5, np.arange(H)[:, None] + 0.5
    val = np.zeros((H, W, 3), f32)
    val[4, 31] = 1.0
    pos[4, 31] = (32.0, 4.5)
    film, counts = nori_amd.film_splat(s, pos, val, ordered=True)
    assert counts == (W * H, 0)
    ref = R.splat_ref(W, H, *R.scene_filter(s), pos, val, ordered=True)
    assert np.array_equal(_bits(film), _bits(ref["film"]))
    # unordered, the same position is pixel 32's
    one, counts = nori_amd.film_splat(s, pos[4, 31][None], val[4, 31][None])
    assert counts == (1, 0)
    ref1 = R.splat_ref(W, H, *R.scene_filter(s), pos[4, 31][None], val[4, 31][None])
    assert np.array_equal(_bits(one), _bits(ref1["film"]))


def test_oracle_samples_through_the_statement_match_the_oracle_render(built):
    W, H, passes = 72, 56, 4
    s = nori_amd.load_scene(scene_path("pa4", "cbox", "cbox_path_mis.xml"), W, H, passes)
    o = pyoracle.OracleScene(s)
    smp = o.wave_samples(np.arange(passes * W * H, dtype=np.uint64))  # ps.x, ps.y, L of sample id pass W H + y W + x
    pos, val = smp[:, 0:2].copy(), smp[:, 2:5].copy()
    want = o.render(passes=passes, rng="wave")
    film, counts = nori_amd.film_splat(s, pos, val, ordered=True)
    ref = R.splat_ref(W, H, *R.scene_filter(s), pos, val, ordered=True, want_stats=False)
    assert counts == ref["counts"] and counts[0] >= 0.99 * passes * W * H
    assert counts[1] == o.last_stats.get("invalid_samples", counts[1])
    assert want[..., 3].max() > 0
    R.assert_within_bound(want, ref, "oracle render against S")
    R.assert_within_bound(film, ref, "host statement against S")


def test_refusals_and_abi(built, tmp_path):
    lib = nori_amd.lib()
    s = nori_amd.load_scene(scene_path("pa4", "cbox", "cbox_path_mis.xml"), 33, 31, 1)
    n = 33 * 31
    pos, val = np.zeros((n, 2), f32), np.zeros((n, 3), f32)
    film = np.zeros(s.film_shape(), f32)
    counts = (C.c_uint64 * 2)()
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    ok = lib.nori_film_splat(s.desc_ptr, n, 0, p(pos), p(val), p(film), None, counts)  # (all in pixel 0, 0)
    assert ok == 0 and tuple(counts) == (n, 0)
    for args in [(None, n, 0, p(pos), p(val), p(film), None, counts), (s.desc_ptr, n, 0, None, p(val), p(film), None, counts),
                 (s.desc_ptr, n, 0, p(pos), None, p(film), None, counts), (s.desc_ptr, n, 0, p(pos), p(val), None, None, counts),
                 (s.desc_ptr, n, 0, p(pos), p(val), p(film), None, None),
                 (s.desc_ptr, n - 1, 1, p(pos), p(val), p(film), None, counts)]:  # ordered: not a multiple of H W
        before = film.copy()
        assert lib.nori_film_splat(*args) == -1  # NORI_ERR_INVALID
        assert np.array_equal(film, before)
    assert lib.nori_film_splat(s.desc_ptr, 0, 1, p(pos), p(val), p(film), None, counts) == 0  # n = 0: a multiple
    with pytest.raises(nori_amd.NoriError):
        nori_amd.film_splat(s, pos[:-1], val[:-1], ordered=True)
    # the ABI: version 7, the calls exported, mirrored and declared
    assert _abi.ABI_VERSION == 7 and lib.nori_gpu_abi_version() == 7
    raw = C.CDLL(_abi.LIB_PATH)
    text = open(HEADER).read()
    for name in CALLS:
        assert hasattr(raw, name), name
        assert name in _abi.SIGNATURES and name in _abi.ADDED_IN_7, name
        assert f"int {name}(" in text, name
    # nori_gpu_splat_desc's mirror against the C layout
    py = _abi.SplatDesc
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             'printf("size %zu\\n", sizeof(nori_gpu_splat_desc));']
    for fname, _ in py._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(nori_gpu_splat_desc, {fname}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(py) == 24
    assert [f for f, _ in py._fields_] == ["n", "on_device", "reserved", "variance_out"]
    for fname, _ in py._fields_:
        assert int(out[fname]) == getattr(py, fname).offset, fname
