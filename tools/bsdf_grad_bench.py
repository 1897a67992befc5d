"""Timings of nori_gpu_bsdf_grad on an MI355X, beside the forward it differentiates
and what a user has without it.

    python tools/bsdf_grad_bench.py [OUTDIR]     -> OUTDIR/bsdf_grad_bench.json

1M camera-ray hit records each (1024 x 1024, one pass; misses stay in), wo towards a sample of the
scene's first light from the hit, a random gradient row, device arrays (torch).  Inputs: cbox
(cbox_path_mis: diffuse), veach (veach_ems: the microfacet plates), disney (the Disney box); each
in pixel order and randomly permuted.  ms_shade is the HIP-event time of k_bsdf_grad +
k_bsdf_grad_sum (nori_gpu_stats); the forward nori_gpu_bsdf_eval on the same inputs and the torch
formulation are timed with torch's events around the (blocking) call, and so is the adjoint's
whole call (grad_call_ms), which is what compares with them.  3 warm-up calls, then 15 timed ones:
the median, and min / max as the spread of repeating the same call; the adjoint, the forward and
the torch formulation alternate in the same run.
torch_ms (cbox only): what a user has today for a diffuse scene, index_add_ of g_rgb / pi of the
lit elements into a zero (num_bsdfs, 3) tensor.  atomic_ms: the same call with
NORI_BSDF_GRAD_TABLE=0 (the wave groups' first lanes add with float atomics)."""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "nori-ray-tracer_amd")]
import nori_amd  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "bench_out")
os.makedirs(OUT, exist_ok=True)
REPS, WARM = 15, 3
W = H = 1024
SCENES = {"cbox": "scenes/pa4/cbox/cbox_path_mis.xml", "veach": "scenes/pa3/veach_mi/veach_ems.xml",
          "disney": "scenes/project/disney/cbox_path_mis.xml"}


def med(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "n": len(v)}


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    import torch

    dev = torch.device("cuda", 0)
    results = {}
    for name, path in SCENES.items():
        scene = nori_amd.load_scene(os.path.join(ROOT, path), W, H, 1)
        n, nb = W * H, scene.desc.num_bsdfs
        with nori_amd.GpuRenderer(scene, 0) as r:
            def buf(cols):
                return torch.zeros((n, cols), dtype=torch.float32, device=dev)

            rays, surf, es, out = buf(8), buf(16), buf(12), buf(8)
            torch.cuda.synchronize()
            r.camera_rays(passes=1, out=rays.data_ptr())
            r.query(rays.data_ptr(), n=n, surf_out=surf.data_ptr())
            u = torch.rand((n, 2), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
            p = surf[:, 0:3].contiguous()
            torch.cuda.synchronize()
            r.emitter_sample(p, u, emitter=0, n=n, out=es)
            wi = (-rays[:, 4:7]).contiguous()
            wo = es[:, 0:3].contiguous()
            g = torch.randn((n, 8), device=dev, generator=torch.Generator(device=dev).manual_seed(2))
            shape = surf[:, 11].view(torch.int32)
            sb = torch.tensor([scene.desc.shapes[s].bsdf for s in range(scene.desc.num_shapes)] + [0], device=dev)
            for order in ("pixel", "permuted"):
                if order == "permuted":
                    perm = torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
                    surf, wi, wo, g = (a[perm].contiguous() for a in (surf, wi, wo, g))
                    shape = surf[:, 11].view(torch.int32)
                gm = torch.zeros((nb, 16), dtype=torch.float32, device=dev)
                torch.cuda.synchronize()
                r.bsdf_eval(surf, wi, wo, n=n, out=out)
                bid = sb[shape.long()]  # (a miss, -1, indexes the trailing entry; its terms are masked)
                lit = (shape >= 0) & (out[:, 4] > 0) & (out[:, 5] > 0)

                def torch_form():
                    t = torch.where(lit[:, None], g[:, 0:3] * (1.0 / math.pi), torch.zeros_like(g[:, 0:3]))
                    return torch.zeros((nb, 3), device=dev).index_add_(0, bid, t)

                grad, gcall, fwd, tch, atm = [], [], [], [], []
                for it in range(WARM + REPS):
                    gw = timed(torch, lambda: r.bsdf_grad(surf, wi, wo, g, grad_materials=gm, n=n))
                    a = r.last_stats["ms_shade"]
                    f = timed(torch, lambda: r.bsdf_eval(surf, wi, wo, n=n, out=out))
                    t = timed(torch, torch_form) if name == "cbox" else 0.0
                    os.environ["NORI_BSDF_GRAD_TABLE"] = "0"
                    r.bsdf_grad(surf, wi, wo, g, grad_materials=gm, n=n)
                    os.environ.pop("NORI_BSDF_GRAD_TABLE")
                    if it >= WARM:
                        grad.append(a), gcall.append(gw), fwd.append(f), tch.append(t), atm.append(r.last_stats["ms_shade"])
                key = f"{name}_{order}"
                results[key] = {"n": n, "num_bsdfs": nb, "hits": int((shape >= 0).sum()), "grad_ms": med(grad), "grad_call_ms": med(gcall),
                                "forward_call_ms": med(fwd), "atomic_ms": med(atm)}
                if name == "cbox":
                    results[key]["torch_ms"] = med(tch)
                print(key, json.dumps(results[key]), flush=True)
    with open(os.path.join(OUT, "bsdf_grad_bench.json"), "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
