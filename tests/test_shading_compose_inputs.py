"""The inputs of the composition test (tests/test_gpu_shading_queries.py, test 3) on the CPU: that
test leaves out the samples the renderer dropped as invalid (count 0 in the statistics) and caps
them at 1 %.  Here the oracle renders the same scenes, passes and size and reports no invalid
sample at all, so a sample missing on the GPU would be a finding, not an input property."""
import pytest

import nori_amd
import pyoracle
import shading_compose
from conftest import scene_path


def _no_invalid_sample(scene):
    assert (scene.width, scene.height) == (32, 32)
    oracle = pyoracle.OracleScene(scene)
    for k in shading_compose.PASSES:
        oracle.render(passes=1, pass_begin=k, rng="wave")
        st = oracle.last_stats
        assert st["samples"] == 32 * 32 and st["invalid_samples"] == 0, (k, st)


@pytest.mark.parametrize("parts", shading_compose.DIRECT_SCENES, ids=[p[-1][:-4] for p in shading_compose.DIRECT_SCENES])
def test_composed_scenes_have_no_invalid_sample(built, parts):
    scene = nori_amd.load_scene(scene_path(*parts), 32, 32, 1)
    assert scene.integrator in ("direct_ems", "direct_mats", "direct_mis")
    _no_invalid_sample(scene)


def test_envmap_scene_has_no_invalid_sample(built, tmp_path):
    _no_invalid_sample(nori_amd.load_scene(shading_compose.envmap_direct_mis(str(tmp_path))))
