"""Timings of nori_gpu_query / nori_gpu_camera_rays on an MI355X (DESIGN_LOG.md, ray queries).

    python tools/query_bench.py [OUTDIR]          device buffers (torch): camera rays of cbox and of the
                                                  512-grid height field at 1M and 4M rays; k_surface with both
                                                  store variants alternating (NORI_SURFACE_STORE), the trace
                                                  kernel, the whole blocking call -> OUTDIR/query_bench.json
    python tools/query_bench.py host [OUTDIR]     host buffers, 1M camera rays of cbox: wall time of trace() and
                                                  query(); with NORI_GPU_LIB=<a library without nori_gpu_query>
                                                  trace() alone, on the rays the first form saved in OUTDIR

3 warm-up calls, then 15 (host: 7) timed ones; kernel times are the HIP-event times of
nori_gpu_stats (ms_extend: trace, ms_shade: k_surface), wall times a host clock around the blocking call."""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "nori-ray-tracer_amd")]
import nori_amd  # noqa: E402
from nori_amd import configs  # noqa: E402

ARGS = [a for a in sys.argv[1:] if a != "host"]
OUT = ARGS[0] if ARGS else os.path.join(ROOT, "bench_out")
os.makedirs(OUT, exist_ok=True)
REPS = 15


def med(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "n": len(v)}


def host_only():
    """wall time of trace() (and query() where the library has it) on host buffers, 1M camera rays of cbox"""
    s = nori_amd.load_scene(os.path.join(ROOT, "scenes/pa4/cbox/cbox_path_mis.xml"), 1024, 1024, 1)
    res = {"lib": os.environ.get("NORI_GPU_LIB", "default")}
    with nori_amd.GpuRenderer(s, 0) as r:
        has_q = hasattr(nori_amd.lib(), "nori_gpu_query")
        if has_q:
            rays = r.camera_rays(passes=1).reshape(-1, 8)
            np.save(os.path.join(OUT, "rays_1m.npy"), rays)
        else:
            rays = np.load(os.path.join(OUT, "rays_1m.npy"))
        n = rays.shape[0]
        for _ in range(3):
            r.trace(rays)
        tt, tq, tqs = [], [], []
        for _ in range(7):
            t0 = time.perf_counter(); r.trace(rays); tt.append(1e3 * (time.perf_counter() - t0))
            if has_q:
                t0 = time.perf_counter(); r.query(rays, surface=False); tq.append(1e3 * (time.perf_counter() - t0))
                t0 = time.perf_counter(); r.query(rays); tqs.append(1e3 * (time.perf_counter() - t0))
        res["n"] = n
        res["trace_ms"] = med(tt)
        if has_q:
            res["query_hits_ms"], res["query_surf_ms"] = med(tq), med(tqs)
    print(json.dumps(res))
    with open(os.path.join(OUT, f"query_host_{res['lib'].split('/')[-1]}.json"), "w") as f:
        json.dump(res, f)


def device():
    import torch
    tmp = tempfile.mkdtemp()
    scenes = {
        "cbox": nori_amd.load_scene(os.path.join(ROOT, "scenes/pa4/cbox/cbox_path_mis.xml"), 1024, 1024, 4),
        "heightfield": nori_amd.load_scene(configs.heightfield_scene(tmp, n=512, width=1024, height=1024, spp=4)),
    }
    res = {}
    for name, s in scenes.items():
        with nori_amd.GpuRenderer(s, 0) as r:
            for passes in (1, 4):
                n = passes * 1024 * 1024
                rays = torch.zeros((n, 8), dtype=torch.float32, device="cuda:0")
                hits = torch.zeros((n, 4), dtype=torch.float32, device="cuda:0")
                surf = {v: torch.zeros((n, 16), dtype=torch.float32, device="cuda:0") for v in ("direct", "lds")}
                torch.cuda.synchronize()
                cam = []
                for i in range(REPS + 3):
                    t0 = time.perf_counter()
                    r.camera_rays(passes=passes, out=rays.data_ptr())
                    if i >= 3:
                        cam.append(1e3 * (time.perf_counter() - t0))
                tm = {v: {"wall": [], "trace": [], "surface": []} for v in surf}
                for i in range(REPS + 3):
                    for v in ("direct", "lds"):   # alternate the variants
                        os.environ["NORI_SURFACE_STORE"] = v
                        t0 = time.perf_counter()
                        r.query(rays.data_ptr(), n=n, hits_out=hits.data_ptr(), surf_out=surf[v].data_ptr())
                        w = 1e3 * (time.perf_counter() - t0)
                        if i >= 3:
                            tm[v]["wall"].append(w)
                            tm[v]["trace"].append(r.last_stats["ms_extend"])
                            tm[v]["surface"].append(r.last_stats["ms_shade"])
                os.environ.pop("NORI_SURFACE_STORE")
                same = bool(torch.equal(surf["direct"].view(torch.int32), surf["lds"].view(torch.int32)))
                hit_share = float((hits[:, 1].view(torch.int32) >= 0).float().mean())
                e = {"n": n, "hit_share": hit_share, "variants_bit_equal": same,
                     "camera_rays_wall_ms": med(cam)}
                for v in surf:
                    k = med(tm[v]["surface"])
                    e[v] = {"query_wall_ms": med(tm[v]["wall"]), "k_trace_ms": med(tm[v]["trace"]), "k_surface_ms": k,
                            "k_surface_TBps_112B": 112.0 * n / (k["median"] * 1e-3) / 1e12,
                            "k_surface_share_of_8TBps": 112.0 * n / (k["median"] * 1e-3) / 8e12}
                res[f"{name}_{passes}M"] = e
                print(name, passes, json.dumps(e), flush=True)
                del rays, hits, surf
    with open(os.path.join(OUT, "query_bench.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    host_only() if "host" in sys.argv[1:] else device()
