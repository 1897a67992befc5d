"""Timings of nori_gpu_film_splat / nori_gpu_film_splat_passes on an MI355X.

    python tools/splat_bench.py [OUTDIR]     -> OUTDIR/splat_bench_<library>.json

cbox_path_mis at 512 x 512, 8 passes, device arrays (torch); ms_splat is the HIP-event time of the
kernels (nori_gpu_stats).  3 warm-up calls, then 15 timed ones: the median, and min / max as the
spread of repeating the same call.  Inputs:
  passes     the renderer's own positions (pixel + draws 0, 1 of sample_uniforms) in pass layout,
             through film_splat_passes (k_splat_pos)
  scattered  the same samples through film_splat (k_splat_scatter)
  permuted   ... after a random permutation
  one_block  2M samples all inside one 32 x 32 block
  builtin    ms_splat of a timing=True render of the same scene and passes with NORI_JIT_CODE=0:
             k_splat<B, false>, the same arithmetic with the jitter recomputed instead of loaded
The scattered figures also come as atomic bytes n K^2 16 over kernel time, as a share of the
1.3 TB/s chip-wide float-atomic rate.  NORI_GPU_LIB selects another build of the library (the
scattered kernel's other form is a compile-time choice, NORI_SCATTER_ROWS): run the tool once per
library, alternating, to compare them."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "nori-ray-tracer_amd")]
import nori_amd  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "bench_out")
os.makedirs(OUT, exist_ok=True)
REPS, WARM = 15, 3
W = H = 512
PASSES = 8
ATOMIC_RATE = 1.3e12  # bytes / s, chip-wide float atomics


def med(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "n": len(v)}


def main():
    import torch
    dev = torch.device("cuda", 0)
    lib = os.path.basename(os.environ.get("NORI_GPU_LIB", "libnori_gpu.so"))
    scene_xml = os.path.join(ROOT, "scenes/pa4/cbox/cbox_path_mis.xml")
    s = nori_amd.load_scene(scene_xml, W, H, PASSES)
    b = s.film_shape()[0] - H >> 1
    K = 2 * b + 1
    res = {"lib": lib, "width": W, "height": H, "passes": PASSES, "border": b}
    g = torch.Generator(device=dev).manual_seed(1)
    with nori_amd.GpuRenderer(s, 0) as r:
        n = PASSES * H * W
        u = torch.zeros((PASSES, H, W, 2), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        r.sample_uniforms(0, 2, passes=PASSES, out=u)
        ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
        pos = (torch.stack([xs, ys], -1).float()[None] + u).contiguous()
        val = (2.0 * torch.rand((PASSES, H, W, 3), generator=g, device=dev)).contiguous()
        perm = torch.randperm(n, generator=g, device=dev)
        pos_p, val_p = pos.reshape(-1, 2)[perm].contiguous(), val.reshape(-1, 3)[perm].contiguous()
        n1 = 2 * 1024 * 1024
        pos_1 = (torch.tensor([224.0, 288.0], device=dev) + 32.0 * torch.rand((n1, 2), generator=g, device=dev)).clamp(
            max=319.99).contiguous()
        pos_1[:, 0].clamp_(max=255.99)
        val_1 = (2.0 * torch.rand((n1, 3), generator=g, device=dev)).contiguous()
        film = torch.zeros(s.film_shape(), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        cases = {
            "passes": lambda: r.film_splat_passes(pos, val, passes=PASSES, out=film),
            "scattered": lambda: r.film_splat(pos.reshape(-1, 2), val.reshape(-1, 3), out=film),
            "permuted": lambda: r.film_splat(pos_p, val_p, out=film),
            "one_block": lambda: r.film_splat(pos_1, val_1, out=film),
        }
        times = {k: [] for k in cases}
        for i in range(REPS + WARM):
            for k, call in cases.items():  # the inputs alternate
                call()
                assert r.last_stats["invalid_samples"] == 0, (k, r.last_stats)
                if i >= WARM:
                    times[k].append(r.last_stats["ms_splat"])
        for k, v in times.items():
            e = {"ms_splat": med(v), "samples": n1 if k == "one_block" else n}
            if k != "passes":
                rate = e["samples"] * K * K * 16 / (e["ms_splat"]["median"] * 1e-3)
                e["atomic_TBps"] = rate / 1e12
                e["share_of_atomic_rate"] = rate / ATOMIC_RATE
            res[k] = e
            print(lib, k, json.dumps(e), flush=True)
    # the built-in kernel on the same scene and passes, the jitter recomputed from pcg32
    os.environ["NORI_JIT_CODE"] = "0"
    try:
        with nori_amd.GpuRenderer(s, 0) as r:
            film = torch.zeros(s.film_shape(), dtype=torch.float32, device=dev)
            torch.cuda.synchronize(dev)
            v = []
            for i in range(REPS + WARM):
                r.render(passes=PASSES, device_ptr=film.data_ptr(), timing=True)
                if i >= WARM:
                    v.append(r.last_stats["ms_splat"])
            res["builtin"] = {"ms_splat": med(v), "samples": n}
            print(lib, "builtin", json.dumps(res["builtin"]), flush=True)
    finally:
        os.environ.pop("NORI_JIT_CODE")
    res["passes_over_builtin"] = res["passes"]["ms_splat"]["median"] / res["builtin"]["ms_splat"]["median"]
    print(lib, "passes / builtin", res["passes_over_builtin"], flush=True)
    with open(os.path.join(OUT, f"splat_bench_{lib.replace('.so', '')}.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
