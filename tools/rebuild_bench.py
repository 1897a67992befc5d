"""Timings of nori_gpu_rebuild_bvh on an MI355X (DESIGN_LOG.md, dynamic geometry).

    python tools/rebuild_bench.py [OUTDIR]   -> OUTDIR/rebuild_bench.json

The C3 mesh (the 512-grid height field, 524,300 triangles) at 1024 x 1024, refit_bench.py's protocol:
  rebuild  rebuild_bvh() on the moved mesh against what the same tree quality cost before it,
           load_scene + GpuRenderer on the moved mesh, alternating: wall time of the blocking call
           and the HIP-event time from its first launch to its last
  trace    1M camera rays on (i) a context created fresh on the positions (the SAH tree), (ii) the
           refitted tree, (iii) the rebuilt tree, alternating, after a displacement of about one
           cell, after one the size of the mesh's relief (0.15; and at 0.02 and 0.05 between them), and at refit_util's position set c (every
           vertex at a random point of a box three times the scene's: no tree helps there and a ray
           costs a large share of the 524,300 triangles, so that row traces RAYS_C rays)
  leaf     the rebuild and the trace at the large displacement for leaf_max 2, 4 and 8
3 warm-up calls, then REPS timed ones; the sides of every comparison alternate in one process.
"""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "nori-ray-tracer_amd")]
import nori_amd  # noqa: E402
from nori_amd import configs  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "bench_out")
os.makedirs(OUT, exist_ok=True)
REPS, N, RES = 15, 512, 1024
RAYS_C, REPS_C = 4096, 5


def med(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "n": len(v)}


def displaced(scene, amplitude):
    """The height field's vertices lifted by a wave of the given amplitude (the walls and the light stay)."""
    P = scene.positions()
    big = max(scene.shapes(), key=lambda sh: sh.tri_count)
    v = slice(big.vtx_offset, big.vtx_offset + big.vtx_count)
    P[v, 1] += (amplitude * np.sin(9.0 * P[v, 0] + 0.4) * np.cos(7.0 * P[v, 2] - 0.2)).astype(np.float32)
    return P


def set_c(scene, seed=5):
    """refit_util.position_set(scene, "c")."""
    P = scene.positions()
    used = P[np.unique(scene.indices())].astype(np.float64)
    lo, hi = used.min(0), used.max(0)
    mid, half = 0.5 * (lo + hi), 1.5 * (hi - lo)
    return np.random.default_rng(seed).uniform(mid - half, mid + half, size=P.shape).astype(np.float32)


def fresh(xml, P):
    s = nori_amd.load_scene(xml)
    np.ctypeslib.as_array(s.desc.positions, shape=(len(P), 3))[:] = P
    return s


def main():
    tmp = tempfile.mkdtemp()
    xml = configs.heightfield_scene(tmp, n=N, width=RES, height=RES, spp=1)
    scene = nori_amd.load_scene(xml)
    cell = 1.6 / N
    sets = {"one cell": displaced(scene, cell), "0.02": displaced(scene, 0.02), "0.05": displaced(scene, 0.05),
            "relief": displaced(scene, 0.15), "set c": set_c(scene)}
    res = {"triangles": int(scene.desc.num_triangles), "vertices": int(scene.desc.num_vertices)}
    dev = torch.device("cuda", 0)
    n = RES * RES
    rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
    hits = {k: torch.empty((n, 4), dtype=torch.float32, device=dev) for k in ("fresh", "refit", "rebuilt")}
    torch.cuda.synchronize()
    with nori_amd.GpuRenderer(scene, 0) as A, nori_amd.GpuRenderer(scene, 0) as Cx:
        # ---- rebuild against load + create on the moved mesh, alternating
        P = sets["relief"]
        A.update_vertices(P)
        Cx.update_vertices(P)
        wall, kern, create = [], [], []
        for k in range(3 + REPS):
            t0 = time.perf_counter()
            st = Cx.rebuild_bvh()
            t1 = time.perf_counter()
            with nori_amd.GpuRenderer(fresh(xml, P), 0):
                t2 = time.perf_counter()
            if k >= 3:
                wall.append(1e3 * (t1 - t0))
                kern.append(st["ms_device"])
                create.append(1e3 * (t2 - t1))
        res["rebuild"] = {"wall_ms": med(wall), "device_ms": med(kern), "fresh_create_ms": med(create),
                          "slowest_rebuild_beats_fastest_create": max(wall) < min(create),
                          **{k: st[k] for k in ("nodes", "depth", "stack", "levels", "launches")}}
        print(json.dumps(res["rebuild"]), flush=True)
        # ---- trace: fresh (SAH) / refitted / rebuilt
        res["trace"] = {}
        for name, Q in sets.items():
            few = name == "set c"
            m, reps = (RAYS_C, REPS_C) if few else (n, REPS)
            A.update_vertices(Q)
            Cx.update_vertices(Q)
            Cx.rebuild_bvh()
            try:  # (the SAH builder's tree of set c is too deep for the traversal stack: no fresh side there)
                B = nori_amd.GpuRenderer(fresh(xml, Q), 0)
            except nori_amd.NoriError as e:
                B, refused = None, str(e)
            sides = [(k, r) for k, r in (("fresh", B), ("refit", A), ("rebuilt", Cx)) if r is not None]
            try:
                A.camera_rays(passes=1, out=rays.data_ptr())  # (the camera does not move: every context's rays)
                if few:  # a strided sample of the frame's rays, packed at the front
                    rays[:m] = rays[:: n // m][:m].clone()
                    torch.cuda.synchronize()
                t = {k: [] for k, _ in sides}
                for k in range((1 if few else 3) + reps):
                    for side, r in sides:
                        r.query(rays.data_ptr(), n=m, hits_out=hits[side].data_ptr())
                        if k >= (1 if few else 3):
                            t[side].append(r.last_stats["ms_extend"])
                same_t = all(bool(torch.equal(hits["refit"][:m, 0].view(torch.int32), hits[k][:m, 0].view(torch.int32)))
                             for k, _ in sides)
            finally:
                if B is not None:
                    B.close()
            md = {k: med(v) for k, v in t.items()}
            row = {"rays": m, **{f"{k}_ms": v for k, v in md.items()}, "t_bit_equal": same_t,
                   "rebuilt_over_refit": md["rebuilt"]["median"] / md["refit"]["median"]}
            if B is None:
                row["fresh_refused"] = refused
            else:
                row["refit_over_fresh"] = md["refit"]["median"] / md["fresh"]["median"]
                row["rebuilt_over_fresh"] = md["rebuilt"]["median"] / md["fresh"]["median"]
            res["trace"][name] = row
            print(name, json.dumps(row), flush=True)
        # ---- leaf_max 2, 4, 8 at the relief displacement
        Cx.update_vertices(sets["relief"])
        Cx.camera_rays(passes=1, out=rays.data_ptr())
        torch.cuda.synchronize()
        leaf = {L: {"wall": [], "trace": []} for L in (2, 4, 8)}
        for k in range(3 + REPS):
            for L in leaf:
                t0 = time.perf_counter()
                st = Cx.rebuild_bvh(L)
                dt = 1e3 * (time.perf_counter() - t0)
                Cx.query(rays.data_ptr(), n=n, hits_out=hits["rebuilt"].data_ptr())
                if k >= 3:
                    leaf[L]["wall"].append(dt)
                    leaf[L]["trace"].append(Cx.last_stats["ms_extend"])
                    leaf[L].update(nodes=st["nodes"], depth=st["depth"])
        res["leaf_max"] = {str(L): {"rebuild_wall_ms": med(v["wall"]), "trace_ms": med(v["trace"]), "nodes": v["nodes"],
                                    "depth": v["depth"]} for L, v in leaf.items()}
    with open(os.path.join(OUT, "rebuild_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
