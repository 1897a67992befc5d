"""The BVH refit's host statement (nori_scene_bvh_refit, nori_amd.bvh_refit) against an
independent numpy statement (refit_util.numpy_refit), bit for bit; no GPU.

The kernels of nori_gpu_update_vertices are tested against the host statement in
test_gpu_refit.py, so this file is what ties them to the refit's definition in nori_gpu.h:
topology kept, records rebuilt from the vertices, leaf boxes from the vertex positions, inner
boxes from the child node's used slots, unused (NaN) slots never written.
"""
import numpy as np
import pytest

import nori_amd
import refit_util as ru
from nori_amd import _abi


@pytest.fixture(scope="module")
def scenes(built, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("refit"))
    got = {}
    for which in ru.SCENES:
        s = ru.load(which, out)
        got[which] = (s, nori_amd.bvh_refit(s))
    return got


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_the_scenes_are_the_cases_they_stand_for(scenes):
    info = {k: nori_amd.bvh_info(s) for k, (s, _) in scenes.items()}
    assert info["hf"]["num_prims"] == 2 * 48 * 48 + 12 and info["hf"]["device_nodes"] > 256
    assert info["nest"]["depth"] == 26
    assert info["pile"]["num_prims"] == 200 and info["pile"]["device_nodes"] >= 2   # one leaf of 200 split up
    assert scenes["pile"][0].desc.num_vertices == 202                                  # two vertices shared by all
    assert info["cbox"]["num_prims"] == 14
    nodes, prims, _ = scenes["cbox"][1]
    refs = nodes.view(np.uint32)[:, 24:28]
    used = ~np.isnan(nodes[:, 0:4])
    assert (~used).any() and (prims.view(np.uint32)[:, 7] == 1).sum() == 2
    # a leaf at record 0, and unused slots whose ref is the leaf bit alone ...
    assert ((refs[used] & 0x81FFFFFF) == ru.LEAF_BIT).any() and (refs[~used] == ru.LEAF_BIT).all()
    # ... which in `apart` is also the ref of a USED slot: the one-primitive leaf at record 0
    nodes, _, _ = scenes["apart"][1]
    refs, used = nodes.view(np.uint32)[:, 24:28], ~np.isnan(nodes[:, 0:4])
    assert (refs[used] == ru.LEAF_BIT).sum() == 1 and (refs[~used] == ru.LEAF_BIT).any()
    for k, (s, (nodes, prims, _)) in scenes.items():
        assert nodes.shape == (info[k]["device_nodes"], 32) and prims.shape == (info[k]["num_prims"], 12)


@pytest.mark.parametrize("pset", ru.SETS)
@pytest.mark.parametrize("which", ru.SCENES)
def test_host_statement_equals_the_numpy_statement(scenes, which, pset):
    s, (nodes0, prims0, box0) = scenes[which]
    P = ru.position_set(s, pset)
    nodes, prims, box = nori_amd.bvh_refit(s, P)
    want_nodes, want_prims, want_root, want_all = ru.numpy_refit(s, nodes0, prims0, P)
    assert ru.same_bits(prims, want_prims)
    assert ru.same_bits(nodes, want_nodes)
    # topology, refs, the unused words and every w word are as built
    assert np.array_equal(_bits(nodes)[:, 24:32], _bits(nodes0)[:, 24:32])
    assert np.array_equal(np.isnan(nodes[:, :24]), np.isnan(nodes0[:, :24]))
    assert np.array_equal(_bits(prims)[:, [3, 7, 11]], _bits(prims0)[:, [3, 7, 11]])
    # the root box: the root node's used slots = the min / max over all primitives
    assert np.array_equal(_bits(box), _bits(want_root)) and np.array_equal(_bits(box), _bits(want_all))
    if pset == "a":   # the builder's boxes are the exact unions already: a refit to the same positions is the identity
        assert ru.same_bits(nodes, nodes0) and ru.same_bits(prims, prims0) and np.array_equal(_bits(box), _bits(box0))
    if pset == "c":   # the root box grows
        assert (box[:3] < box0[:3]).all() and (box[3:] > box0[3:]).all()
    if pset == "d":   # both zeros occur, and a collapsed triangle has zero edges
        assert (_bits(P) == 0x80000000).any()
        tri = prims.view(np.uint32)[:, 7] != 1
        assert (np.abs(prims[tri][:, [4, 5, 6, 8, 9, 10]]).max(axis=1) == 0).any()


@pytest.mark.parametrize("which", ru.SCENES)
def test_the_statement_has_no_memory(scenes, which):
    s, _ = scenes[which]
    P1, P2 = ru.position_set(s, "c"), ru.position_set(s, "b")
    nori_amd.bvh_refit(s, P1)
    a = nori_amd.bvh_refit(s, P2)
    b = nori_amd.bvh_refit(s, P2)
    assert all(ru.same_bits(x, y) for x, y in zip(a, b))
    # ... and it leaves the scene as loaded
    c = nori_amd.bvh_refit(s)
    assert all(ru.same_bits(x, y) for x, y in zip(c, scenes[which][1]))


def test_ordered_zeros():
    """The numpy statement's key orders -0 below +0 and round-trips every float."""
    x = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, 1e-45, -1e-45], np.float32)
    k = ru._key(x)
    assert k[1] < k[0] and k[7] < k[1] and k[0] < k[6] and k[5] == k.min() and k[4] == k.max()
    assert np.array_equal(_bits(ru._unkey(k)), _bits(x))


def test_arguments(scenes):
    s, (nodes0, _, _) = scenes["cbox"]
    P = s.positions()
    P[3, 1] = np.nan
    with pytest.raises(nori_amd.NoriError) as e:
        nori_amd.bvh_refit(s, P)
    assert e.value.code == _abi.NORI_ERR_INVALID
    with pytest.raises(ValueError):
        nori_amd.bvh_refit(s, P[:-1])
    assert nori_amd.lib().nori_scene_bvh_refit(None, None, None, None, None) == _abi.NORI_ERR_INVALID
    # every output is optional
    assert nori_amd.lib().nori_scene_bvh_refit(s.desc_ptr, None, None, None, None) == _abi.NORI_OK


def test_new_struct_layouts_match_c(built, tmp_path):
    """As test_abi.test_struct_layout_matches_c, for the two structs this call adds."""
    import ctypes as C
    import os
    import subprocess

    from conftest import ROOT

    structs = {"nori_gpu_update_desc": _abi.UpdateDesc, "nori_gpu_update_stats": _abi.UpdateStats}
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
    for name in ("nori_gpu_update_vertices", "nori_gpu_bvh_read", "nori_scene_bvh_refit"):
        assert name in _abi.SIGNATURES and name in _abi.ADDED_IN_7
