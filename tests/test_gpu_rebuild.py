"""The BVH rebuilt on the GPU: nori_gpu_rebuild_bvh (rebuild.hip) against the rebuild's host
statement (nori_scene_bvh_rebuild, itself tied to an independent numpy statement in
test_rebuild.py) byte for byte, and a rebuilt context against a context created fresh on the same
positions -- never a kernel against itself.

Hit distances and barycentrics depend on the triangle record alone, so the rebuilt tree must give
the same bits as the SAH tree of a fresh context; which of two primitives with the same t a ray
reports may differ with the tree, and is then proven a tie ray by ray (nori_test_util.prim_hit).

Every context is created with NORI_TRAVERSAL=bvh, except the scan-mode one that is refused.
"""
import ctypes as C

import numpy as np
import pytest

import nori_amd
import rebuild_util as bu
import refit_util as ru
import synth
from conftest import scene_path
from nori_amd import _abi
from nori_test_util import assert_parity, image_parity
from test_gpu_refit import _assert_tree, _bits, _case_rays, _Cases, _compare_contexts, _renderer
from test_query import scene_rays

pytestmark = pytest.mark.gpu


class _RebuildCases(_Cases):
    def positions(self, which, pset):
        if (which, pset) not in self._pos:
            self._pos[which, pset] = bu.position_set(self.scene(which), pset)
        return self._pos[which, pset]

    def rebuilt(self, which, pset, leaf_max, refit=None):
        """nori_amd.bvh_rebuild of the scene at a position set (then refitted to another)."""
        key = (which, pset, leaf_max, refit)
        if key not in self._host:
            Q = None if refit is None else self.positions(which, refit)
            self._host[key] = nori_amd.bvh_rebuild(self.scene(which), self.positions(which, pset), leaf_max, Q)
        return self._host[key]


@pytest.fixture(scope="module")
def cases(built, tmp_path_factory):
    return _RebuildCases(str(tmp_path_factory.mktemp("rebuild_gpu")))


def _create_rule_stack(depth):
    """nori_gpu_create's stack for a 4-wide tree of `depth` levels: 3 entries per level and one;
    stacks 8, 16, 32 hold 4, 8, 16 in LDS and 64 more in private memory."""
    need = 3 * depth + 1
    return 8 if need <= 4 else 16 if need <= 8 + 64 else 32


def _assert_stats(st, info, what):
    assert st["nodes"] == info["device_nodes"] and st["depth"] == info["depth"], (what, st, info)
    assert st["stack"] == _create_rule_stack(info["depth"]), (what, st)
    assert st["levels"] == info["depth"] and st["launches"] > 0 and st["ms"] > 0 and st["ms_device"] > 0, (what, st)


# ---------------------------------------------------------------- 1. bytes
@pytest.mark.parametrize("which", ru.SCENES)
def test_tree_equals_the_host_statement(cases, which):
    """update(b), (c), (e), (f), (a) in sequence on one context, each followed by a rebuild with
    leaf_max 1, 4 and 64: the device tree is the host statement's, byte for byte, each time."""
    s = cases.scene(which)
    with _renderer(s) as r:
        for pset in ("b", "c", "e", "f", "a"):
            r.update_vertices(cases.positions(which, pset))
            for L in bu.LEAF_MAX:
                st = r.rebuild_bvh(L)
                want = cases.rebuilt(which, pset, L)
                _assert_tree(r, want, (pset, L))
                _assert_stats(st, want[3], (which, pset, L))
        print(f"{which}: {st['nodes']} nodes, depth {st['depth']}, stack {st['stack']}, {st['launches']} launches, "
              f"last rebuild {st['ms']:.3f} ms ({st['ms_device']:.3f} ms on the device)")


# ---------------------------------------------------------------- 2. a sort of several work-groups
def test_a_sort_beyond_one_work_group(cases, tmp_path):
    """rebuild.hip configures rocprim's radix sort with a merge-sort limit of 1,024: up to 1,024
    keys take the single-block sort (256 threads x 4 keys), more take Onesweep, whose blocks on
    gfx950 hold 512 x 12 = 6,144 keys of 8 bytes (rocprim's device_radix_sort_onesweep
    configuration).  The 4,620 triangles of `hf` are one Onesweep block; this 96 x 96 height field
    has 18,444 triangles, four blocks, whose digit offsets pass from block to block."""
    s = nori_amd.load_scene(synth.heightfield_scene(str(tmp_path), n=96, integrator="path_mis", width=32, height=32, spp=1))
    assert s.desc.num_triangles == 2 * 96 * 96 + 12 > 3 * 6144
    with _renderer(s) as r:
        for pset in ("b", "c"):
            P = bu.position_set(s, pset)
            r.update_vertices(P)
            st = r.rebuild_bvh(4)
            want = nori_amd.bvh_rebuild(s, P, 4)
            _assert_tree(r, want, pset)
            _assert_stats(st, want[3], pset)
    print(f"18,444 triangles: {st['nodes']} nodes, depth {st['depth']}, rebuild {st['ms']:.3f} ms "
          f"({st['ms_device']:.3f} ms on the device, {st['launches']} launches)")


# ---------------------------------------------------------------- 3. rays against a fresh context
@pytest.mark.parametrize("which", ["hf", "cbox", "nest"])
def test_rays_equal_a_fresh_context(cases, which):
    s, P = cases.scene(which), cases.positions(which, "c")
    fs = cases.fresh(which, P)
    with _renderer(s) as A, _renderer(fs) as B:
        rays, sh = _case_rays(which, "c", fs, B)
        A.update_vertices(P)
        refit_nodes, _ = A.bvh_nodes()
        A.rebuild_bvh()
        assert not ru.same_bits(A.bvh_nodes()[0], refit_nodes)      # another tree ...
        a = _compare_contexts(A, B, fs, rays, sh, f"{which} (c), rebuilt")   # ... the same answers
    hit = np.isfinite(a["t"])
    assert hit.mean() >= 0.05 and len(np.unique(a["prim"][hit])) >= (20 if which != "cbox" else 8)


# ---------------------------------------------------------------- 4. render
@pytest.mark.parametrize("which", ["hf", "cbox"])
def test_render_equals_a_fresh_context(cases, which):
    """path_mis, 32 x 32 at 4 spp, on the displaced geometry (set b): the rebuilt context's film
    meets the parity bars against a fresh context's, as a refitted context's does."""
    s, P = cases.scene(which), cases.positions(which, "b")
    fs = cases.fresh(which, P)
    assert (s.desc.camera.width, s.desc.camera.height) == (32, 32)
    with _renderer(s) as A, _renderer(fs) as B:
        A.update_vertices(P)
        A.rebuild_bvh()
        got, want = nori_amd.develop(s, A.render(passes=4)), nori_amd.develop(fs, B.render(passes=4))
    p = image_parity(got, want)
    print(f"{which}, rebuilt against fresh: {p}, bit-equal: {np.array_equal(_bits(got), _bits(want))}")
    assert float(got.mean()) > 0
    assert_parity(p)


# ---------------------------------------------------------------- 5. refit after rebuild
@pytest.mark.parametrize("which", ru.SCENES)
def test_refit_after_rebuild(cases, which):
    """update_vertices after a rebuild refits the REBUILT tree (the new schedule), and a second
    rebuild depends on the positions alone: the rebuild has no memory."""
    s, L = cases.scene(which), 4
    with _renderer(s) as r:
        r.update_vertices(cases.positions(which, "c"))
        r.rebuild_bvh(L)
        st = r.update_vertices(cases.positions(which, "b"))
        want = cases.rebuilt(which, "c", L, refit="b")
        _assert_tree(r, want, "rebuilt at c, refitted to b")
        assert np.array_equal(_bits(np.array(st["root_min"] + st["root_max"], np.float32)), _bits(want[2]))
        assert st["nodes"] == want[3]["device_nodes"] and st["levels"] == want[3]["depth"]
        r.rebuild_bvh(L)
        _assert_tree(r, cases.rebuilt(which, "b", L), "rebuilt at b")


# ---------------------------------------------------------------- 6. refusals
def _refused(r, code, **fields):
    rd = _abi.RebuildDesc()
    for k, v in fields.items():
        setattr(rd, k, v)
    assert nori_amd.lib().nori_gpu_rebuild_bvh(r._h, C.byref(rd), None) == code
    return nori_amd.lib().nori_gpu_last_error().decode()


def _state(r, rays):
    return r.bvh_nodes(), r.trace(rays)


def _assert_unchanged(r, rays, before, what):
    (n0, p0), h0 = before
    (n1, p1), h1 = _state(r, rays)
    assert ru.same_bits(n0, n1) and ru.same_bits(p0, p1), what
    assert np.array_equal(_bits(h0), _bits(h1)), what


def test_refusals_change_nothing(built, tmp_path):
    cbox = nori_amd.load_scene(scene_path("pa4", "cbox", "cbox_path_mis.xml"), 16, 16, 2)
    rays = scene_rays("cbox", cbox, 2000)
    # a scan-mode context
    with _renderer(cbox, mode=None) as r:
        before = _state(r, rays)
        with pytest.raises(nori_amd.NoriError, match="NORI_TRAVERSAL=bvh") as e:
            r.rebuild_bvh()
        assert e.value.code == _abi.NORI_ERR_UNSUPPORTED
        _assert_unchanged(r, rays, before, "scan mode")
    # a photonmapper context
    pm = nori_amd.load_scene(synth.cbox_variant(
        str(tmp_path), "pm", integrator="photonmapper", width=16, height=16,
        integrator_props='<integer name="photonCount" value="2000"/><float name="photonRadius" value="0.05"/>'), 0, 0, 2)
    with _renderer(pm) as r:
        before = _state(r, rays)
        with pytest.raises(nori_amd.NoriError, match="photon") as e:
            r.rebuild_bvh()
        assert e.value.code == _abi.NORI_ERR_UNSUPPORTED
        _assert_unchanged(r, rays, before, "photonmapper")
    # bad arguments on a context that accepts rebuilds
    with _renderer(cbox) as r:
        before = _state(r, rays)
        with pytest.raises(nori_amd.NoriError) as e:
            r.rebuild_bvh(65)
        assert e.value.code == _abi.NORI_ERR_INVALID
        assert "reserved" in _refused(r, _abi.NORI_ERR_INVALID, reserved=(C.c_uint32 * 7)(0, 0, 0, 0, 0, 0, 1))
        assert nori_amd.lib().nori_gpu_rebuild_bvh(r._h, None, None) == _abi.NORI_ERR_INVALID
        assert nori_amd.lib().nori_gpu_rebuild_bvh(None, None, None) == _abi.NORI_ERR_INVALID
        _assert_unchanged(r, rays, before, "bad arguments")
        # the same context then takes a valid rebuild, and traces the same distances from the new tree
        r.rebuild_bvh()
        _assert_tree(r, nori_amd.bvh_rebuild(cbox), "after the refusals")
        assert np.array_equal(_bits(r.trace(rays)["t"]), _bits(before[1]["t"]))


# ---------------------------------------------------------------- the example
def test_deform_example_with_rebuilds(built):
    import importlib.util
    import os

    from conftest import ROOT

    torch = pytest.importorskip("torch")
    spec = importlib.util.spec_from_file_location("deform_torch", os.path.join(ROOT, "examples", "deform_torch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    s = nori_amd.load_scene(scene_path("pa4", "cbox", "cbox_path_mis.xml"), 32, 32, 1)
    with _renderer(s) as r:
        created = r.bvh_nodes()[0]
        frames = mod.deform_frames(r, frames=3, rebuild_every=2)
        assert not ru.same_bits(r.bvh_nodes()[0][:, 24:28], created[:, 24:28]) or len(r.bvh_nodes()[0]) != len(created)
    assert len(frames) == 3
    for f in frames:
        assert f.is_cuda and f.shape == (32, 32, 3) and bool(torch.isfinite(f).all())
