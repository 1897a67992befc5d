"""nori_film_gather, the host statement of the film splat's adjoint, on the CPU:
1. against its numpy restatement (tests/film_gather_ref.py) bit for bit -- both add in the stated
   order -- for every filter and border, both frames, scattered samples with all the special
   positions and values, the ordered layout at 3 passes, and val=None (which keeps the
   invalid-value rows); the counts too;
2. the adjoint identity <film_splat(val), grad> = <val, film_gather(grad)> under the bound
   (m_max + 4) 2^-24 T of film_gather_ref.adjoint_check;
3. refusals, the ABI version, the ctypes mirror against the C layout."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import film_gather_ref as G
import film_splat_ref as R
import nori_amd
from conftest import ROOT, scene_path
from nori_amd import _abi

f32 = np.float32
HEADER = os.path.join(ROOT, "include", "nori_gpu.h")
CALLS = ("nori_film_gather", "nori_gpu_film_gather", "nori_gpu_film_gather_passes")


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.mark.parametrize("frame", R.FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("filt", R.FILTERS, ids=lambda f: f[0])
def test_host_statement_matches_the_numpy_restatement(built, tmp_path, filt, frame):
    name, rfilter, border = filt
    W, H = frame
    s = nori_amd.load_scene(R.filter_scene_xml(tmp_path, rfilter), W, H, 2)
    rad, tab = R.scene_filter(s)
    grad = G.seeded_grad(s.film_shape())
    for what, (pos, val), ordered in [("scattered", R.scattered_inputs(W, H), False),
                                      ("ordered", R.ordered_inputs(W, H, 3), True)]:
        n = pos.reshape(-1, 2).shape[0]
        ref = G.gather_ref(W, H, rad, tab, pos, grad, val, ordered=ordered)
        assert ref["border"] == border and ref["counts"][1] >= 9 and ref["counts"][0] >= 0.75 * n
        rows, counts = nori_amd.film_gather(s, pos, grad, val, ordered=ordered)
        assert counts == ref["counts"] and sum(counts) == n
        assert rows.shape == (n, 3) and np.array_equal(_bits(rows), _bits(ref["out"]))
        G.assert_within_bound(rows, ref, f"{name} {W}x{H} {what}: sequential sums")
        # the counts are the forward's, and the identity holds with the forward's film
        film, fcounts = nori_amd.film_splat(s, pos, val, ordered=ordered)
        assert fcounts == counts
        fwd = R.splat_ref(W, H, rad, tab, pos, val, ordered=ordered, want_stats=False)
        G.adjoint_check(film, grad, val, rows, ref, fwd["m"], f"{name} {W}x{H} {what}")
        # val=None: no value check -- the invalid-value rows are kept and gathered
        ref0 = G.gather_ref(W, H, rad, tab, pos, grad, None, ordered=ordered)
        assert ref0["counts"][0] > ref["counts"][0]
        rows0, counts0 = nori_amd.film_gather(s, pos, grad, None, ordered=ordered)
        assert counts0 == ref0["counts"]
        assert np.array_equal(_bits(rows0), _bits(ref0["out"]))
        k = ref["kept"]
        assert np.array_equal(_bits(rows0[k]), _bits(rows[k])) and rows0[ref0["kept"] & ~k].any()


def test_integer_positions_take_the_wide_window(built, tmp_path):
    """radius + 0.5 an integer (box, gaussian 4.5): a position on an exact integer has a window of
    2b + 2 cells on that axis, all of which the gather reads."""
    for name, rfilter, b in (R.FILTERS[0], R.FILTERS[5]):
        s = nori_amd.load_scene(R.filter_scene_xml(tmp_path, rfilter), 72, 56, 1)
        rad, tab = R.scene_filter(s)
        pos = np.array([[40.0, 20.0], [40.0, 20.5], [40.5, 20.0]], f32)
        ref = G.gather_ref(72, 56, rad, tab, pos, G.seeded_grad(s.film_shape()))
        assert list(ref["m"]) == [(2 * b + 2) ** 2, (2 * b + 2) * (2 * b + 1), (2 * b + 1) * (2 * b + 2)]
        rows, _ = nori_amd.film_gather(s, pos, G.seeded_grad(s.film_shape()))
        assert np.array_equal(_bits(rows), _bits(ref["out"]))


def test_refusals_and_abi(built, tmp_path):
    lib = nori_amd.lib()
    s = nori_amd.load_scene(scene_path("pa4", "cbox", "cbox_path_mis.xml"), 33, 31, 1)
    n = 33 * 31
    pos, val = np.zeros((n, 2), f32), np.zeros((n, 3), f32)
    grad = np.ones(s.film_shape(), f32)
    out = np.full((n, 3), 7, f32)
    counts = (C.c_uint64 * 2)()
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    assert lib.nori_film_gather(s.desc_ptr, n, 0, p(pos), p(val), p(grad), p(out), counts) == 0  # (all in pixel 0, 0)
    assert tuple(counts) == (n, 0) and (out == out[0]).all() and out[0, 0] > 0  # written, not added into
    assert lib.nori_film_gather(s.desc_ptr, n, 0, p(pos), None, p(grad), p(out), counts) == 0  # val may be NULL
    for args in [(None, n, 0, p(pos), p(val), p(grad), p(out), counts), (s.desc_ptr, n, 0, None, p(val), p(grad), p(out), counts),
                 (s.desc_ptr, n, 0, p(pos), p(val), None, p(out), counts), (s.desc_ptr, n, 0, p(pos), p(val), p(grad), None, counts),
                 (s.desc_ptr, n, 0, p(pos), p(val), p(grad), p(out), None),
                 (s.desc_ptr, n - 1, 1, p(pos), p(val), p(grad), p(out), counts)]:  # ordered: not a multiple of H W
        before = out.copy()
        assert lib.nori_film_gather(*args) == -1  # NORI_ERR_INVALID
        assert np.array_equal(out, before)
    assert lib.nori_film_gather(s.desc_ptr, 0, 1, p(pos), p(val), p(grad), p(out), counts) == 0  # n = 0: a multiple
    # an empty frame
    empty = _abi.SceneDesc.from_buffer_copy(s.desc)
    empty.camera.width = 0
    assert lib.nori_film_gather(C.byref(empty), n, 0, p(pos), p(val), p(grad), p(out), counts) == -1
    assert "empty frame" in lib.nori_gpu_last_error().decode()
    with pytest.raises(nori_amd.NoriError):
        nori_amd.film_gather(s, pos[:-1], grad, val[:-1], ordered=True)
    with pytest.raises(ValueError):
        nori_amd.film_gather(s, pos, grad[1:], val)
    # the ABI: version 7, the calls exported, mirrored and declared
    assert _abi.ABI_VERSION == 7 and lib.nori_gpu_abi_version() == 7
    raw = C.CDLL(_abi.LIB_PATH)
    text = open(HEADER).read()
    for name in CALLS:
        assert hasattr(raw, name), name
        assert name in _abi.SIGNATURES and name in _abi.ADDED_IN_7, name
        assert f"int {name}(" in text, name
    # nori_gpu_gather_desc's mirror against the C layout
    py = _abi.GatherDesc
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             'printf("size %zu\\n", sizeof(nori_gpu_gather_desc));']
    for fname, _ in py._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(nori_gpu_gather_desc, {fname}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    res = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(res["size"]) == C.sizeof(py) == 16
    assert [f for f, _ in py._fields_] == ["n", "on_device", "reserved"]
    for fname, _ in py._fields_:
        assert int(res[fname]) == getattr(py, fname).offset, fname
