"""Materials that change under a context: nori_gpu_update_materials / nori_gpu_materials
(csrc/materials.hip, k_materials_count and k_materials_set in csrc/kernels_bsdf_grad.hip).

Everything renders at 32 x 32 with 2 passes.  Scenes: pa4 cbox_path_mis (a scan-mode scene: the
small-scene blob and the tail finisher read the blob's copy of the BSDF table), the veach plates
under NORI_TRAVERSAL=bvh (microfacet) and the Disney box.

1. identity: a context updated with its own rows renders as the untouched context does;
2. new values: written into a tmp-path copy of the XML; the updated context renders, and answers
   bsdf_eval, li and features, as a context created from that copy; materials() reads them
   back; 3. refusals (a wrong count, NaN in a word in use, a misaligned device pointer, a
   photonmapper context) leave the context rendering as before; 4. NaN in words the type ignores
   is accepted.

"As": bit for bit wherever the renderer itself is reproducible -- the BSDF table read back
(materials()), bsdf_eval, the feature sums, and li along every camera ray of the render's two
passes on the render's own streams, which is the radiance of every sample the render splats.  The
film itself is not: the renderer adds its samples into the film with float atomics, whose order
differs run to run (two renders of one untouched context already differ in the last bits;
tests/test_gpu_shade_rtc.py), so two films are held to that file's bar for two renders of one
scene, np.allclose(rtol=1e-5, atol=1e-6) with equal sample and ray counts, and the test prints
whether they were bit-equal as well.  The film is what exercises the blob's copy of the table
(k_shade and the tail finisher read it), and a stale or damaged copy shows there as a difference
of the size of the change (checked: the new values move the film by far more than the bar)."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import material_util as M
import nori_amd
from conftest import scene_path
from nori_amd import _abi

pytestmark = pytest.mark.gpu
f32 = np.float32
SCENES = {"cbox": (("pa4", "cbox", "cbox_path_mis.xml"), {}),
          "veach": (("pa3", "veach_mi", "veach_ems.xml"), {"NORI_TRAVERSAL": "bvh"}),
          "disney": (("project", "disney", "cbox_path_mis.xml"), {})}


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    try:
        os.environ.update({k: str(v) for k, v in kw.items()})
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def load(path):
    return nori_amd.load_scene(path, 32, 32, 2)


def renderer(scene, env):
    with _env(**env):
        return nori_amd.GpuRenderer(scene, 0)


COUNTERS = ("samples", "invalid_samples", "rays_closest", "rays_shadow", "rays_finish", "iterations")


def render(r):
    """(film, counters) of the scene's two passes; NORI_LOOKAHEAD=0 makes the iteration count
    reproducible (tests/test_gpu_shade_rtc.py)."""
    with _env(NORI_LOOKAHEAD="0"):
        film = r.render()
    return film, {k: r.last_stats[k] for k in COUNTERS}


def same_film(a, b, what):
    (fa, ca), (fb, cb) = a, b
    print(f"{what}: max |a - b| = {np.abs(fa - fb).max():.3e}, bit-equal: {np.array_equal(fa.view(np.uint32), fb.view(np.uint32))}")
    assert ca == cb, (what, ca, cb)
    assert np.allclose(fa, fb, rtol=1e-5, atol=1e-6), (what, np.abs(fa - fb).max())
    assert fa.mean() > 0


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def new_rows(scene):
    """The scene's rows with every word in use moved to another valid value."""
    rows = nori_amd.scene_materials(scene)
    g = np.random.default_rng(8)
    for b, kind in enumerate(M.kinds(scene)):
        for w in M.WORDS[kind]:
            if kind == "microfacet" and w == 3:
                rows[b, w] = f32(rows[b, w] * g.uniform(1.5, 3.0))  # alpha
            elif kind == "microfacet":
                rows[b, w] = f32(g.uniform(0.05, 0.4))  # kd: ks = 1 - max(kd) changes too
            else:
                rows[b, w] = f32(g.uniform(0.1, 0.9))
    return rows


def probes(scene, r):
    """li along every camera ray of the render's two passes on the render's own streams (the
    samples' radiance), bsdf_eval at the first pass's hits, the feature sums; and the hit mask."""
    rays = r.camera_rays(passes=2).reshape(-1, 8)
    li = r.li(rays, seed=0, stream_base=0, first_draw=4)
    first = rays[:scene.width * scene.height]
    q = r.query(first)
    hit = q["surf"]["shape"] >= 0
    wo = M.world_dirs(q["surf"]["ns"], M.directions(len(first), 3))
    return r.bsdf_eval(q["surf"], -first[:, 4:7], wo), li, r.features(passes=2), hit


@pytest.mark.parametrize("which", sorted(SCENES))
def test_update_matches_a_context_created_with_the_values(built, tmp_path, which):
    path, env = SCENES[which]
    src = scene_path(*path)
    scene = load(src)
    own = nori_amd.scene_materials(scene)
    with renderer(scene, env) as r:
        base = render(r)
        same_film(base, render(r), f"{which}: two renders of the untouched context")
        ev0, li0, ft0, _ = probes(scene, r)
        assert r.materials_version == 0
        assert np.array_equal(bits(r.materials()), bits(own))
        r.update_materials(own)  # ---- identity
        assert r.materials_version == 1
        same_film(base, render(r), f"{which}: identity update")
        ev1, li1, ft1, _ = probes(scene, r)
        assert np.array_equal(bits(ev0), bits(ev1)) and np.array_equal(bits(li0), bits(li1)) and np.array_equal(bits(ft0), bits(ft1))
        rows = new_rows(scene)  # ---- new values
        nan_unused = rows.copy()
        for b, kind in enumerate(M.kinds(scene)):
            nan_unused[b, [w for w in range(16) if w not in M.WORDS[kind]]] = np.nan
        r.update_materials(nan_unused)  # NaN in words the type ignores is accepted
        assert r.materials_version == 2
        assert np.array_equal(bits(r.materials()), bits(rows)), "materials() differs from what was set"
        film = render(r)
        ev, li, ft, hit = probes(scene, r)
    copy = load(M.write_with_rows(src, rows, str(tmp_path / "copy.xml")))
    assert np.array_equal(bits(nori_amd.scene_materials(copy)), bits(rows)), "the XML copy does not hold the rows"
    with renderer(copy, env) as r2:
        film2 = render(r2)
        ev2, li2, ft2, _ = probes(copy, r2)
    assert not np.allclose(film[0], base[0], rtol=1e-2, atol=1e-3), "the new values do not show in the film"
    same_film(film, film2, f"{which}: updated against created")
    assert hit.sum() > 100 and not np.array_equal(bits(li), bits(li0))
    assert np.array_equal(bits(ev), bits(ev2)), "bsdf_eval differs"
    assert np.array_equal(bits(li), bits(li2)), "li differs"
    assert np.array_equal(bits(ft), bits(ft2)), "the feature sums differ"


def test_device_rows_are_used_in_place(built):
    import torch

    path, env = SCENES["disney"]
    scene = load(scene_path(*path))
    rows = new_rows(scene)
    with renderer(scene, env) as r:
        r.update_materials(rows)
        a = render(r)
        la = probes(scene, r)[1]
    with renderer(scene, env) as r:
        r.update_materials(torch.from_numpy(rows).cuda())
        assert np.array_equal(bits(r.materials()), bits(rows))
        same_film(a, render(r), "host rows against device rows")
        assert np.array_equal(bits(la), bits(probes(scene, r)[1]))


def test_refusals_change_nothing(built, tmp_path):
    import torch

    path, env = SCENES["disney"]
    scene = load(scene_path(*path))
    rows = new_rows(scene)
    nb = scene.desc.num_bsdfs
    lib = nori_amd.lib()
    with renderer(scene, env) as r:
        base = render(r)
        li0 = probes(scene, r)[1]

        def call(count, on_device, p, reserved=0):
            md = _abi.MaterialsDesc(count, on_device)
            md.reserved[0] = reserved
            return lib.nori_gpu_update_materials(r._h, C.byref(md), C.c_void_p(p))

        assert call(nb + 1, 0, rows.ctypes.data) == _abi.NORI_ERR_INVALID
        assert call(nb, 0, rows.ctypes.data, reserved=1) == _abi.NORI_ERR_INVALID
        assert call(nb, 0, None) == _abi.NORI_ERR_INVALID
        for bad_value in (np.nan, np.inf):
            bad = rows.copy()
            b = M.kinds(scene).index("disney")
            bad[b, 6] = bad_value  # roughness
            with pytest.raises(nori_amd.NoriError):
                r.update_materials(bad)
        dev = torch.zeros(nb * 16 + 4, dtype=torch.float32, device="cuda")
        dev[1:1 + nb * 16] = torch.from_numpy(rows.ravel()).cuda()
        torch.cuda.synchronize()
        assert call(nb, 1, dev.data_ptr() + 2) == _abi.NORI_ERR_INVALID  # misaligned
        assert call(nb, 1, rows.ctypes.data) == _abi.NORI_ERR_INVALID  # not device memory
        assert r.materials_version == 0
        assert np.array_equal(r.materials().view(np.uint32), nori_amd.scene_materials(scene).view(np.uint32))
        same_film(base, render(r), "after the refusals")
        assert np.array_equal(bits(li0), bits(probes(scene, r)[1])), "a refused update changed li"
        assert call(nb, 1, dev.data_ptr() + 4) == 0  # (4-byte aligned is enough)
        assert np.array_equal(r.materials().view(np.uint32), rows.view(np.uint32))
    # a photonmapper context: its map was traced with the materials as loaded
    xml = open(M.zoo_xml(str(tmp_path))).read().replace(
        '<integrator type="path_mis"/>',
        '<integrator type="photonmapper"><integer name="photonCount" value="2000"/><float name="photonRadius" value="0.2"/></integrator>')
    pm = tmp_path / "pm.xml"
    pm.write_text(xml)
    ps = load(str(pm))
    with nori_amd.GpuRenderer(ps, 0) as r:
        with pytest.raises(nori_amd.NoriError) as e:
            r.update_materials(nori_amd.scene_materials(ps))
        assert e.value.code == _abi.NORI_ERR_UNSUPPORTED and r.materials_version == 0
