"""bench.py's multi-GPU launch plan (CPU only): `bench.py --gpus N` without a
launcher starts torch.distributed.run with N processes itself, a rank of such
a job runs in place, and inconsistent requests are refused before any GPU
call."""
import importlib.util
import os
import sys

import pytest

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_single_gpu_runs_in_place():
    b = _bench()
    assert b.launch_plan(1, {}, 1, []) is None
    assert b.launch_plan(1, {}, 8, ["--steps", "3"]) is None


def test_n_gpus_without_launcher_spawns_torchrun():
    b = _bench()
    argv = ["--gpus", "4", "--steps", "7"]
    plan = b.launch_plan(4, {}, 8, argv, port=29555)
    assert plan[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in plan and "--nnodes=1" in plan
    assert "--master-addr=127.0.0.1" in plan and "--master-port=29555" in plan
    i = plan.index(os.path.join(ROOT, "bench.py"))
    assert plan[i + 1:] == argv  # the ranks see the same arguments (and WORLD_SIZE=4)


def test_rank_of_a_launched_job_runs_in_place():
    b = _bench()
    env = {"WORLD_SIZE": "8", "LOCAL_WORLD_SIZE": "8", "RANK": "3", "LOCAL_RANK": "3"}
    assert b.launch_plan(8, env, 8, []) is None


def test_dump_outputs_writes_float32_within_the_limit(tmp_path):
    """--dump-outputs: DIR/<name>.npy in float32 (float64 stays); an array over
    its share of the byte limit becomes the same seeded sample in every run."""
    import numpy as np

    b = _bench()
    assert b.DUMP_LIMIT == 64 << 20
    film = np.arange(8 * 8 * 4, dtype=np.float32).reshape(8, 8, 4)
    big = np.arange(1000, dtype=np.float64)
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), {"film": film, "big": big, "ints": np.arange(5)}, limit=3 * 2048)
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("film", "big", "ints")}
    assert got["film"].dtype == np.float32 and np.array_equal(got["film"], film)
    assert got["ints"].dtype == np.float32 and np.array_equal(got["ints"], np.arange(5))
    assert got["big"].dtype == np.float64 and got["big"].nbytes <= 2048
    assert np.all(np.diff(got["big"]) > 0) and np.isin(got["big"], big).all()  # distinct values of the array
    assert np.array_equal(got["big"], np.load(tmp_path / "b" / "big.npy"))
    assert sum(a.nbytes for a in got.values()) <= 3 * 2048


@pytest.mark.parametrize("gpus,env,devices", [
    (2, {"WORLD_SIZE": "4"}, 8),   # --gpus disagrees with the launcher
    (4, {"WORLD_SIZE": "4", "LOCAL_WORLD_SIZE": "4"}, 2),  # more local ranks than GPUs
    (8, {}, 1),                     # more GPUs than the node has
    (0, {}, 8),
])
def test_inconsistent_requests_are_refused(gpus, env, devices):
    b = _bench()
    with pytest.raises(SystemExit):
        b.launch_plan(gpus, env, devices, [])
