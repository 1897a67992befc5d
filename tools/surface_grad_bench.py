"""Timings of nori_gpu_surface_grad on an MI355X, beside what a user has without it:
the same terms formed in torch from pos[tri[prim]] and scattered with index_add_.

    python tools/surface_grad_bench.py [OUTDIR]     -> OUTDIR/surface_grad_bench_<library>.json

1M camera rays each (1024 x 1024, one pass), device arrays (torch), a random record gradient;
ms_shade is the HIP-event time of k_surface_grad (nori_gpu_stats), the torch formulation is timed
with torch's events.  3 warm-up calls, then 15 timed ones: the median, and min / max as the spread
of repeating the same call.  Each library call alternates with the comparison in the same run.
Inputs:
  mesh      the 524,288-triangle height field of bench config C3: about two hits per triangle,
            nothing to merge
  cbox      cbox_path_mis: a few dozen triangles (and two spheres, which contribute nothing):
            everything merges
  permuted  the same Cornell box hits in a random order: the wave merge finds little, the atomics
            contend
torch_ms: the whole backward (gather pos[tri[prim]], the nine position terms of the header in
float32, three index_add_ into a zero (V, 3) tensor); torch_scatter_ms: the index_add_ calls alone.
Neither scene has vertex normals, so both sides form the nine position terms.  added_TBps: the
terms' bytes (36 per contributing hit) over the kernel's time, against the 1.3 TB/s of
chip-wide float atomics.  NORI_GPU_LIB selects another build of the library."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "nori-ray-tracer_amd")]
import nori_amd  # noqa: E402
from nori_amd import configs  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "bench_out")
os.makedirs(OUT, exist_ok=True)
REPS, WARM = 15, 3
W = H = 1024
ATOMIC_RATE = 1.3e12  # bytes / s of added floats, chip-wide


def med(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "n": len(v)}


def prim_tables(scene, torch, dev):
    """(vertex ids (P, 3) int64, mesh flag (P,)) by global primitive id."""
    import numpy as np
    idx = scene.indices().astype(np.int64)
    vid, mesh = [], []
    for sh in scene.shapes():
        if sh.type == nori_amd._abi.SHAPE_SPHERE:
            vid.append(np.zeros((1, 3), np.int64))
            mesh.append(np.zeros(1, bool))
        else:
            vid.append(idx[sh.tri_offset:sh.tri_offset + sh.tri_count])
            mesh.append(np.ones(sh.tri_count, bool))
    return torch.from_numpy(np.concatenate(vid)).to(dev), torch.from_numpy(np.concatenate(mesh)).to(dev)


def torch_terms(torch, pos, vid, mesh, rays, hits, grad):
    """The header's nine position terms per hit in torch float32 (meshes without vertex normals:
    g' = g_ng + g_ns), zero rows where the hit contributes nothing; and the vertex ids."""
    prim = hits[:, 1].view(torch.int32).long()
    live = prim >= 0
    k = torch.where(live, prim, torch.zeros_like(prim))
    live = live & mesh[k]
    f = vid[k]
    p0, p1, p2 = pos[f[:, 0]], pos[f[:, 1]], pos[f[:, 2]]
    t, u, v = hits[:, 0:1], hits[:, 2:3], hits[:, 3:4]
    o, d = rays[:, 0:3], rays[:, 4:7]
    g_p, g_t, gq = grad[:, 0:3], grad[:, 3:4], grad[:, 4:7] + grad[:, 8:11]
    b = 1 - (u + v)
    e1, e2 = p1 - p0, p2 - p0
    N = torch.linalg.cross(e1, e2)
    ln = N.norm(dim=1, keepdim=True)
    D = (N * d).sum(1, keepdim=True)
    live = live & (ln[:, 0] > 0) & (D[:, 0] != 0)
    ng = N / ln
    gN = (gq - ng * (ng * gq).sum(1, keepdim=True)) / ln
    s = g_t / D
    gN = gN + (p0 - (o + d * t)) * s
    ge1, ge2 = torch.linalg.cross(e2, gN), torch.linalg.cross(gN, e1)
    zero = torch.zeros_like(g_p)
    m = live[:, None]
    t0 = torch.where(m, (g_p * b + N * s) - (ge1 + ge2), zero)
    t1 = torch.where(m, g_p * u + ge1, zero)
    t2 = torch.where(m, g_p * v + ge2, zero)
    return (t0, t1, t2), f, live


def main():
    import tempfile

    import torch
    dev = torch.device("cuda", 0)
    lib = os.path.basename(os.environ.get("NORI_GPU_LIB", "libnori_gpu.so"))
    res = {"lib": lib, "width": W, "height": H}
    g = torch.Generator(device=dev).manual_seed(1)
    n = W * H
    inputs = {}
    keep = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, xml in (("mesh", configs.config_scene("c3", tmp, W, H, 1)[0]),
                          ("cbox", os.path.join(ROOT, "scenes/pa4/cbox/cbox_path_mis.xml"))):
            s = nori_amd.load_scene(xml, W, H, 1)
            r = nori_amd.GpuRenderer(s, 0)
            keep.append(r)
            rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
            hits = torch.empty((n, 4), dtype=torch.float32, device=dev)
            torch.cuda.synchronize(dev)
            r.camera_rays(passes=1, out=rays.data_ptr())
            r.query(rays.data_ptr(), n=n, hits_out=hits.data_ptr())
            grad = torch.randn((n, 16), generator=g, dtype=torch.float32, device=dev)
            pos = torch.from_numpy(s.positions()).to(dev)
            vid, mesh = prim_tables(s, torch, dev)
            inputs[name] = (r, s, rays, hits, grad, pos, vid, mesh)
            if name == "cbox":
                perm = torch.randperm(n, generator=g, device=dev)
                inputs["permuted"] = (r, s, rays[perm].contiguous(), hits[perm].contiguous(), grad[perm].contiguous(), pos, vid, mesh)
    times = {k: {"lib": [], "torch": [], "scatter": []} for k in inputs}
    live = {}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for i in range(REPS + WARM):
        for k, (r, s, rays, hits, grad, pos, vid, mesh) in inputs.items():
            V = s.desc.num_vertices
            gp = torch.zeros((V, 3), dtype=torch.float32, device=dev)
            torch.cuda.synchronize(dev)
            r.surface_grad(rays, hits, grad, gp, None)
            t_lib = r.last_stats["ms_shade"]
            out = torch.zeros((V, 3), dtype=torch.float32, device=dev)
            torch.cuda.synchronize(dev)
            ev[0].record()
            terms, f, alive = torch_terms(torch, pos, vid, mesh, rays, hits, grad)
            ev[1].record()
            for j in range(3):
                out.index_add_(0, f[:, j], terms[j])
            ev[2].record()
            torch.cuda.synchronize(dev)
            live[k] = int(alive.sum())
            if i == 0:  # the two formulations agree (float32 sums in different orders)
                scale = float(out.abs().max())
                res.setdefault("max_abs_difference_over_max", {})[k] = float((out - gp).abs().max()) / scale
            if i >= WARM:
                times[k]["lib"].append(t_lib)
                times[k]["torch"].append(ev[0].elapsed_time(ev[2]))
                times[k]["scatter"].append(ev[1].elapsed_time(ev[2]))
    for k, v in times.items():
        e = {"hits": n, "contributing": live[k], "lib_ms": med(v["lib"]), "torch_ms": med(v["torch"]),
             "torch_scatter_ms": med(v["scatter"])}
        e["torch_over_lib"] = e["torch_ms"]["median"] / e["lib_ms"]["median"]
        e["torch_scatter_over_lib"] = e["torch_scatter_ms"]["median"] / e["lib_ms"]["median"]
        rate = 36 * live[k] / (e["lib_ms"]["median"] * 1e-3)
        e["added_TBps"] = rate / 1e12
        e["share_of_atomic_rate"] = rate / ATOMIC_RATE
        res[k] = e
        print(lib, k, json.dumps(e), flush=True)
    with open(os.path.join(OUT, f"surface_grad_bench_{lib.replace('.so', '')}.json"), "w") as f:
        json.dump(res, f, indent=1)
    for r in keep:
        r.close()


if __name__ == "__main__":
    main()
