"""The tail finisher's path numbering (csrc/tail_index.h: tail_prefix_per,
tail_paths_per_wave, tail_grid, tail_first, tail_segment, tail_slot -- the
functions k_tail_prefix, k_finish and finish_dispatch number the queued paths
with), compiled for the host with g++ (tests/tail_index_check.cpp), once per
NORI_FINISH_WAVES setting the project has used: the prefix's total is the
path count, the waves the grid launches cover every queued path exactly once
after the whole-work-group and whole-wave exits, no lane looks a path up in
an empty or neighbouring segment, and every queue index lies inside its
segment's count -- over segment counts G on both sides of the point where the
2 * G grid overtakes kFinishWaves / wpb and path totals on both sides of
every step of K."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "tail_index_check.cpp")
INC = os.path.join(ROOT, "nori-ray-tracer_amd", "csrc")


def _build_and_run(exe, waves, extra=()):
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", *extra, f"-DNORI_FINISH_WAVES={waves}", "-I", INC, SRC,
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert f"(NORI_FINISH_WAVES={waves})" in r.stdout, r.stdout
    assert " 0 failures" in r.stdout, r.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("waves", [0, 1024, 2048, 4096])
def test_tail_index_covers_every_path_once(tmp_path, waves):
    _build_and_run(tmp_path / f"tail_index_check_{waves}", waves)


def _has_sanitizers(tmp_path):
    """Can this g++ link a program with the address and undefined-behaviour sanitizers?"""
    if shutil.which("g++") is None:
        return False
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", "-fsanitize=address,undefined", str(src), "-o", str(tmp_path / "probe")],
                       capture_output=True)
    return r.returncode == 0


def test_tail_index_under_sanitizers(tmp_path):
    """The same stand-alone program (default NORI_FINISH_WAVES) with
    -fsanitize=address,undefined: an index past the prefix, the counts or the
    coverage tables of the check itself aborts it."""
    if not _has_sanitizers(tmp_path):
        pytest.skip("g++ has no sanitizer runtimes")
    _build_and_run(tmp_path / "tail_index_check_asan", 1024,
                   ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))
