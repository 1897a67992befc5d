"""The BVH rebuild's host statement (nori_scene_bvh_rebuild, nori_amd.bvh_rebuild) against an
independent numpy statement (rebuild_util.numpy_rebuild), bit for bit; no GPU.

The kernels of nori_gpu_rebuild_bvh are tested against the host statement in
test_gpu_rebuild.py, so this file is what ties them to the rebuild's definition in nori_gpu.h:
Morton keys of the box centres, leaf order by ascending key, Karras's split with ties broken by
position, 4-wide nodes numbered breadth-first, boxes by the refit's rule.
"""
import ctypes as C

import numpy as np
import pytest

import nori_amd
import rebuild_util as bu
import refit_util as ru
from nori_amd import _abi


@pytest.fixture(scope="module")
def scenes(built, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rebuild"))
    return {which: ru.load(which, out) for which in ru.SCENES}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("leaf_max", bu.LEAF_MAX)
@pytest.mark.parametrize("which", ru.SCENES)
def test_host_statement_equals_the_numpy_statement(scenes, which, leaf_max):
    s = scenes[which]
    for pset in bu.SETS:
        P = bu.position_set(s, pset)
        nodes, prims, box, info = nori_amd.bvh_rebuild(s, P, leaf_max)
        want_nodes, want_prims, want_box, want_info = bu.numpy_rebuild(s, P, leaf_max)
        assert info == want_info, (pset, info, want_info)
        assert ru.same_bits(prims, want_prims), pset
        assert ru.same_bits(nodes, want_nodes), pset
        assert np.array_equal(_bits(box), _bits(want_box)), pset
        leaves = bu.tree_invariants(nodes, prims, leaf_max)
        assert nodes.shape == (info["device_nodes"], 32) and prims.shape == (info["num_prims"], 12)
        if leaf_max == 1:
            # one record per leaf: the leaf at record 0 has the bare leaf bit as its ref, the word
            # an unused slot carries too (the trap the refit's statement names)
            refs, used = nodes.view(np.uint32)[:, 24:28], ~np.isnan(nodes[:, 0:4])
            assert leaves == len(prims) and (refs[used] == ru.LEAF_BIT).sum() == 1
        if pset == "f" and which in ("hf", "nest", "pile", "apart"):
            # every code ties: the splits come from the positions' bits, so the tree is balanced
            n = info["num_prims"]
            binary = int(np.ceil(np.log2(max(2, -(-n // leaf_max)))))
            assert info["depth"] <= binary // 2 + 1, (info, binary)


def test_the_scenes_are_the_cases_they_stand_for(scenes):
    s = scenes["cbox"]
    nodes, prims, _, info = nori_amd.bvh_rebuild(s, None, 64)
    assert info == {"device_nodes": 1, "depth": 1, "num_prims": 14, "leaf_max": 64}   # n <= leaf_max: one leaf slot
    assert nodes.view(np.uint32)[0, 24] == ru.LEAF_BIT | 13 << 25 and np.isnan(nodes[0, 1:4]).all()
    assert (prims.view(np.uint32)[:, 7] == 1).sum() == 2
    assert nori_amd.bvh_rebuild(s)[3]["leaf_max"] == 4                                 # the default
    hf = scenes["hf"]
    assert nori_amd.bvh_rebuild(hf, None, 4)[3]["device_nodes"] > 256                  # several work-groups per level
    # the nest's 20 decades: almost all codes collide
    nest = scenes["nest"]
    vid, _ = ru.prim_vertex_ids(nest)
    k = ru._key(nest.positions()[vid])
    code = bu._codes(ru._unkey(k.min(1)), ru._unkey(k.max(1)))
    assert len(np.unique(code)) < len(code) // 4
    # set e: the mesh-only scenes have no extent in y
    for which in ("hf", "nest", "pile", "apart"):
        P = bu.position_set(scenes[which], "e")
        assert np.ptp(P[np.unique(scenes[which].indices())][:, 1]) == 0


@pytest.mark.parametrize("which", ru.SCENES)
def test_refit_positions_and_defaults(scenes, which):
    s = scenes[which]
    Pc, Pb = bu.position_set(s, "c"), bu.position_set(s, "b")
    nodes0, prims0, _, info0 = nori_amd.bvh_rebuild(s, Pc, 4)
    nodes, prims, box, info = nori_amd.bvh_rebuild(s, Pc, 4, refit_positions=Pb)
    want_nodes, want_prims, want_root, _ = ru.numpy_refit(s, nodes0, prims0, Pb)
    assert info == info0
    assert ru.same_bits(nodes, want_nodes) and ru.same_bits(prims, want_prims)
    assert np.array_equal(_bits(box), _bits(want_root))
    # positions=None is the scene's own positions; the statement has no memory
    a = nori_amd.bvh_rebuild(s, None, 4)
    b = nori_amd.bvh_rebuild(s, s.positions(), 4)
    assert all(ru.same_bits(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def test_arguments(scenes):
    s = scenes["cbox"]
    with pytest.raises(nori_amd.NoriError) as e:
        nori_amd.bvh_rebuild(s, None, 65)
    assert e.value.code == _abi.NORI_ERR_INVALID
    P = s.positions()
    P[3, 1] = np.nan
    for kw in ({"positions": P}, {"refit_positions": P}):
        with pytest.raises(nori_amd.NoriError) as e:
            nori_amd.bvh_rebuild(s, **kw)
        assert e.value.code == _abi.NORI_ERR_INVALID
    with pytest.raises(ValueError):
        nori_amd.bvh_rebuild(s, P[:-1])
    fn = nori_amd.lib().nori_scene_bvh_rebuild
    assert fn(None, None, 0, None, None, None, None, None) == _abi.NORI_ERR_INVALID
    assert fn(s.desc_ptr, None, 0, None, None, None, None, None) == _abi.NORI_OK   # every output is optional
    info = _abi.BvhRebuildInfo()
    assert fn(s.desc_ptr, None, 0, None, C.byref(info), None, None, None) == _abi.NORI_OK   # info alone: the sizes
    assert info.num_prims == 14 and info.device_nodes >= 2 and info.leaf_max == 4


def test_new_struct_layouts_match_c(built, tmp_path):
    """As test_abi.test_struct_layout_matches_c, for the three structs these calls add."""
    import os
    import subprocess

    from conftest import ROOT

    structs = {"nori_bvh_rebuild_info": _abi.BvhRebuildInfo, "nori_gpu_rebuild_desc": _abi.RebuildDesc,
               "nori_gpu_rebuild_stats": _abi.RebuildStats}
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.join(ROOT, "include", "nori_gpu.h")}"',
             "int main(void) {"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in py._fields_]
    lines.append("return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = dict(l.rsplit(" ", 1) for l in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True,
                                                         check=True).stdout.split("\n") if l)
    for cname, py in structs.items():
        assert int(out[cname]) == C.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(out[f"{cname}.{f}"]) == getattr(py, f).offset, (cname, f)


def test_abi_version_is_still_7(built):
    assert _abi.ABI_VERSION == 7 and nori_amd.lib().nori_gpu_abi_version() == 7
    for name in ("nori_scene_bvh_rebuild", "nori_gpu_rebuild_bvh"):
        assert name in _abi.SIGNATURES and name in _abi.ADDED_IN_7
