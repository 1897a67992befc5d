"""The shading queries' ABI on the CPU: nori_gpu_shading_desc's ctypes mirror against the C layout
(compiled with gcc, as tests/test_abi.py does for the other structures), the five entry points in
the library and the mirror, and csrc/kernels_shading.hip cross-compiled for gfx950."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from nori_amd import _abi

HEADER = os.path.join(ROOT, "include", "nori_gpu.h")
PKG = os.path.join(ROOT, "nori-ray-tracer_amd")
CALLS = ("nori_gpu_bsdf_eval", "nori_gpu_bsdf_sample", "nori_gpu_emitter_sample", "nori_gpu_emitter_eval",
         "nori_gpu_sample_uniforms")


def test_shading_desc_layout_matches_c(tmp_path):
    py = _abi.ShadingDesc
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             'printf("size %zu\\n", sizeof(nori_gpu_shading_desc));']
    for fname, _ in py._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(nori_gpu_shading_desc, {fname}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(py) == 16
    assert [f for f, _ in py._fields_] == ["n", "on_device", "emitter", "reserved"]
    for fname, _ in py._fields_:
        assert int(out[fname]) == getattr(py, fname).offset, fname


def test_library_exports_the_shading_queries(built):
    lib = C.CDLL(_abi.LIB_PATH)
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in _abi.SIGNATURES and name in _abi.ADDED_IN_7, name
    assert _abi.ABI_VERSION == 7  # added without an ABI bump
    text = open(HEADER).read()
    for name in CALLS:
        assert f"int {name}(nori_gpu_ctx *ctx" in text, name


def test_kernels_shading_cross_compiles_for_gfx950(tmp_path):
    hipcc = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    assert hipcc, "hipcc not found"
    obj = tmp_path / "kernels_shading.o"
    subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-slp-vectorize",
                    "-Wall", "-Werror", "-c", os.path.join(PKG, "csrc", "kernels_shading.hip"), "-o", str(obj)], check=True)
    assert obj.stat().st_size > 0
    # the device code object holds the kernels of both record reads
    syms = subprocess.run(["strings", "-a", str(obj)], capture_output=True, text=True, check=True).stdout
    for k in ("k_bsdf_evalILb0", "k_bsdf_evalILb1", "k_bsdf_sampleILb0", "k_emitter_sample", "k_emitter_evalILb1",
              "k_sample_uniforms"):
        assert k in syms, k
