"""Timings of nori_gpu_film_gather / nori_gpu_film_gather_passes on an MI355X,
beside the forward splat of the same inputs.

    python tools/gather_bench.py [OUTDIR]     -> OUTDIR/gather_bench_<library>.json

The scene and the inputs of tools/splat_bench.py: cbox_path_mis at 512 x 512, 8 passes, device
arrays (torch); ms_splat is the HIP-event time of the kernels (nori_gpu_stats).  3 warm-up calls,
then 15 timed ones: the median, and min / max as the spread of repeating the same call.  Inputs:
  passes     the renderer's own positions (pixel + draws 0, 1 of sample_uniforms) in pass layout,
             through film_gather_passes (k_gather_pos)
  passes64   ... at 64 passes; also (32 n + film bytes) / time as a share of 8 TB/s
  scattered  the 8 passes' samples through film_gather (k_gather_scatter)
  permuted   ... after a random permutation
  one_block  2M samples all inside one 32 x 32 block
Every input's forward splat (film_splat_passes / film_splat into a device film) is timed in the
same run, alternating with its gather.  NORI_GPU_LIB selects another build of the library."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "nori-ray-tracer_amd")]
import nori_amd  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "bench_out")
os.makedirs(OUT, exist_ok=True)
REPS, WARM = 15, 3
W = H = 512
PASSES, PASSES_LONG = 8, 64
HBM_RATE = 8e12  # bytes / s, the roofline figure of DESIGN.md


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
    film_bytes = 16 * s.film_shape()[0] * s.film_shape()[1]
    res = {"lib": lib, "width": W, "height": H, "passes": PASSES, "passes_long": PASSES_LONG, "border": b}
    g = torch.Generator(device=dev).manual_seed(1)
    with nori_amd.GpuRenderer(s, 0) as r:
        n = PASSES * H * W
        u = torch.zeros((PASSES_LONG, H, W, 2), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        r.sample_uniforms(0, 2, passes=PASSES_LONG, out=u)
        ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
        pos64 = (torch.stack([xs, ys], -1).float()[None] + u).contiguous()
        val64 = (2.0 * torch.rand((PASSES_LONG, H, W, 3), generator=g, device=dev)).contiguous()
        pos, val = pos64[:PASSES].contiguous(), val64[:PASSES].contiguous()
        perm = torch.randperm(n, generator=g, device=dev)
        pos_p, val_p = pos.reshape(-1, 2)[perm].contiguous(), val.reshape(-1, 3)[perm].contiguous()
        n1 = 2 * 1024 * 1024
        pos_1 = (torch.tensor([224.0, 288.0], device=dev) + 32.0 * torch.rand((n1, 2), generator=g, device=dev)).clamp(
            max=319.99).contiguous()
        pos_1[:, 0].clamp_(max=255.99)
        val_1 = (2.0 * torch.rand((n1, 3), generator=g, device=dev)).contiguous()
        film = torch.zeros(s.film_shape(), dtype=torch.float32, device=dev)
        grad = torch.randn(s.film_shape(), generator=g, dtype=torch.float32, device=dev)
        rows = torch.zeros((PASSES_LONG * H * W, 3), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        cases = {  # name: (samples, the gather, the forward splat)
            "passes": (n, lambda: r.film_gather_passes(pos, grad, val, passes=PASSES, out=rows),
                       lambda: r.film_splat_passes(pos, val, passes=PASSES, out=film)),
            "passes64": (PASSES_LONG * H * W, lambda: r.film_gather_passes(pos64, grad, val64, passes=PASSES_LONG, out=rows),
                         lambda: r.film_splat_passes(pos64, val64, passes=PASSES_LONG, out=film)),
            "scattered": (n, lambda: r.film_gather(pos.reshape(-1, 2), grad, val.reshape(-1, 3), out=rows),
                          lambda: r.film_splat(pos.reshape(-1, 2), val.reshape(-1, 3), out=film)),
            "permuted": (n, lambda: r.film_gather(pos_p, grad, val_p, out=rows), lambda: r.film_splat(pos_p, val_p, out=film)),
            "one_block": (n1, lambda: r.film_gather(pos_1, grad, val_1, out=rows), lambda: r.film_splat(pos_1, val_1, out=film)),
        }
        times = {k: {"gather": [], "splat": []} for k in cases}
        for i in range(REPS + WARM):
            for k, (_, gather, splat) in cases.items():  # the inputs and the two directions alternate
                for what, call in (("gather", gather), ("splat", splat)):
                    call()
                    assert r.last_stats["invalid_samples"] == 0, (k, what, r.last_stats)
                    if i >= WARM:
                        times[k][what].append(r.last_stats["ms_splat"])
        for k, v in times.items():
            e = {"samples": cases[k][0], "gather_ms": med(v["gather"]), "splat_ms": med(v["splat"])}
            e["gather_over_splat"] = e["gather_ms"]["median"] / e["splat_ms"]["median"]
            rate = (32 * e["samples"] + film_bytes) / (e["gather_ms"]["median"] * 1e-3)
            e["TBps"] = rate / 1e12
            e["share_of_hbm_rate"] = rate / HBM_RATE
            res[k] = e
            print(lib, k, json.dumps(e), flush=True)
    with open(os.path.join(OUT, f"gather_bench_{lib.replace('.so', '')}.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
