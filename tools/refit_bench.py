"""Timings of nori_gpu_update_vertices on an MI355X (DESIGN_LOG.md, dynamic geometry).

    python tools/refit_bench.py [OUTDIR]   -> OUTDIR/refit_bench.json

The C3 mesh (the 512-grid height field, 524,288 triangles) at 1024 x 1024:
  update   update_vertices from a device tensor and from a host array, alternating: wall time of the
           blocking call and the HIP-event time of its vertex / record / refit launches
  rebuild  what the same result costs without it: load_scene + GpuRenderer on the moved mesh
  trace    1M camera rays on the refitted context against a context created fresh on the same
           positions, alternating, after a displacement of about one cell and after a large one
3 warm-up calls, then REPS timed ones; the two sides of every comparison alternate in one process.
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


def main():
    tmp = tempfile.mkdtemp()
    xml = configs.heightfield_scene(tmp, n=N, width=RES, height=RES, spp=1)
    t0 = time.perf_counter()
    scene = nori_amd.load_scene(xml)
    load_s = time.perf_counter() - t0
    cell = 1.6 / N
    sets = {"one cell": displaced(scene, cell), "large": displaced(scene, 0.15)}
    res = {"triangles": int(scene.desc.num_triangles), "vertices": int(scene.desc.num_vertices), "load_scene_s": load_s}
    dev = torch.device("cuda", 0)
    n = RES * RES
    with nori_amd.GpuRenderer(scene, 0) as A:
        # ---- update: device tensor / host array, alternating
        P = sets["one cell"]
        d = torch.from_numpy(P).to(dev)
        torch.cuda.synchronize()
        for _ in range(3):
            A.update_vertices(d)
            A.update_vertices(P)
        wall = {"device": [], "host": []}
        kern = {"device": [], "host": []}
        for _ in range(REPS):
            for name, arg in (("device", d), ("host", P)):
                t0 = time.perf_counter()
                st = A.update_vertices(arg)
                wall[name].append(1e3 * (time.perf_counter() - t0))
                kern[name].append(st["ms_device"])
        nodes, prims = A.bvh_nodes()
        res["update"] = {k: {"wall_ms": med(wall[k]), "kernels_ms": med(kern[k])} for k in wall}
        res["update"]["launches"] = st["launches"]
        res["update"]["levels"] = st["levels"]
        res["update"]["nodes"] = st["nodes"]
        # positions in + pos read-modify-write + records (gather 48 B, read 48 B, write 48 B) + nodes read and written
        res["update"]["bytes_touched"] = int(12 * len(P) + 32 * len(P) + 144 * len(prims) + 2 * 128 * len(nodes))
        # ---- rebuild: load + create on the moved mesh (the positions are overwritten after the load)
        reb = []
        for _ in range(3):
            t0 = time.perf_counter()
            s2 = nori_amd.load_scene(xml)
            np.ctypeslib.as_array(s2.desc.positions, shape=(len(P), 3))[:] = P
            with nori_amd.GpuRenderer(s2, 0):
                reb.append(1e3 * (time.perf_counter() - t0))
        res["rebuild_ms"] = med(reb)
        # ---- trace: refitted against fresh, 1M camera rays on device buffers
        rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
        hits = torch.empty((n, 4), dtype=torch.float32, device=dev)
        hits_b = torch.empty((n, 4), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        res["trace"] = {}
        for name, Q in sets.items():
            A.update_vertices(Q)
            s2 = nori_amd.load_scene(xml)
            np.ctypeslib.as_array(s2.desc.positions, shape=(len(Q), 3))[:] = Q
            with nori_amd.GpuRenderer(s2, 0) as B:
                B.camera_rays(passes=1, out=rays.data_ptr())
                t = {"refit": [], "fresh": []}
                for k in range(3 + REPS):
                    for side, r, h in (("refit", A, hits), ("fresh", B, hits_b)):
                        r.query(rays.data_ptr(), n=n, hits_out=h.data_ptr())
                        if k >= 3:
                            t[side].append(r.last_stats["ms_extend"])
                same_t = bool(torch.equal(hits[:, 0].view(torch.int32), hits_b[:, 0].view(torch.int32)))
                res["trace"][name] = {"refit_ms": med(t["refit"]), "fresh_ms": med(t["fresh"]),
                                      "ratio": med(t["refit"])["median"] / med(t["fresh"])["median"],
                                      "t_bit_equal": same_t, "hit_share": float((hits[:, 1].view(torch.int32) >= 0).float().mean())}
    with open(os.path.join(OUT, "refit_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
