"""The radiance query's ABI on the CPU: nori_gpu_li_desc's ctypes mirror against the C layout
(compiled with gcc, as tests/test_shading_abi.py does), the entry point in the library, the header
and the mirror, csrc/kernels_li.hip cross-compiled for gfx950, and the call's device-free checks
(csrc/li_prep.cpp) run under the address and undefined-behaviour sanitizers as a program of their
own (tests/li_prep_check.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from nori_amd import _abi

HEADER = os.path.join(ROOT, "include", "nori_gpu.h")
PKG = os.path.join(ROOT, "nori-ray-tracer_amd")


def test_li_desc_layout_matches_c(tmp_path):
    py = _abi.LiDesc
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             'printf("size %zu\\n", sizeof(nori_gpu_li_desc));']
    for fname, _ in py._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(nori_gpu_li_desc, {fname}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(py) == 32
    assert [f for f, _ in py._fields_] == ["n", "on_device", "seed", "stream_base", "first_draw", "reserved"]
    assert [int(out[f]) for f, _ in py._fields_] == [0, 4, 8, 16, 24, 28]
    for fname, _ in py._fields_:
        assert int(out[fname]) == getattr(py, fname).offset, fname


def test_library_exports_the_radiance_query(built):
    lib = C.CDLL(_abi.LIB_PATH)
    assert hasattr(lib, "nori_gpu_li")
    assert "nori_gpu_li" in _abi.SIGNATURES and "nori_gpu_li" in _abi.ADDED_IN_7
    assert _abi.ABI_VERSION == 7  # added without an ABI bump
    text = open(HEADER).read()
    assert "int nori_gpu_li(nori_gpu_ctx *ctx, const nori_gpu_li_desc *desc, const float *rays," in text
    assert "#define NORI_GPU_ABI_VERSION 7" in text
    assert "nori_gpu_li           <- Integrator::Li include/nori/integrator.h:55" in text
    res, args = _abi.SIGNATURES["nori_gpu_li"]
    assert res is C.c_int and len(args) == 6 and args[1] == C.POINTER(_abi.LiDesc) and args[5] == C.POINTER(_abi.Stats)


def test_kernels_li_cross_compiles_for_gfx950(tmp_path):
    hipcc = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    assert hipcc, "hipcc not found"
    obj = tmp_path / "kernels_li.o"
    subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-slp-vectorize",
                    "-Wall", "-Werror", "-c", os.path.join(PKG, "csrc", "kernels_li.hip"), "-o", str(obj)], check=True)
    assert obj.stat().st_size > 0
    # the device code object holds k_li<STACK, INTEG, LDS, FULL>: the path integrators with the
    # basic and the full plugin set and staged in LDS, a one-bounce integrator, the deepest stack
    syms = subprocess.run(["strings", "-a", str(obj)], capture_output=True, text=True, check=True).stdout
    for k in ("k_liILi0ELi1ELb1ELb0E", "k_liILi0ELi1ELb0ELb1E", "k_liILi64ELi0ELb0ELb1E", "k_liILi8ELi2ELb0ELb0E",
              "k_liILi32ELi8ELb0ELb1E", "k_liILi0ELi9ELb0ELb1E"):
        assert k in syms, k


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_li_prep_sanitized(tmp_path):
    exe = tmp_path / "li_prep_check"
    # the sanitizer runtime is linked into the program: with the shared one ASan refuses to start
    # wherever the environment preloads any other library
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-I", os.path.join(PKG, "csrc"),
                    os.path.join(ROOT, "tests", "li_prep_check.cpp"), os.path.join(PKG, "csrc", "li_prep.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == "ok" and r.stderr == "", (r.stdout, r.stderr[-4000:])
