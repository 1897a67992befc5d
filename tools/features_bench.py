"""Timings of the first-hit feature pass and the guided denoiser on GPU 0; prints JSON lines.

  python tools/features_bench.py run [--reps N] [--size S] [--passes P]
      cbox_path_mis at SxS: GpuRenderer.features(P passes) into a device buffer, with the kernel
      time from HIP events (stats ms_shade), in the context's automatic traversal mode (scan for
      this scene) and with NORI_TRAVERSAL=bvh; then, on a 16-spp render of the same frame with its
      variance and features, denoise_guided with the defaults and at radius 8 / patch 3, and the
      NL-means kernel (denoise, radius 3, patch 3, textbook distance) for scale -- host wall time of
      the calls, host buffers (copies included).  Each after a warm-up, N timed runs.
  rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python tools/features_bench.py run
  python tools/features_bench.py trace DIR
      The kernels' own durations from that trace: per kernel and case of `run` (reps + 1 launches,
      in run's order) the median, minimum and maximum over the dispatches after the first (the warm-up).
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "nori-ray-tracer_amd")]

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["run", "trace"])
ap.add_argument("dir", nargs="?")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--passes", type=int, default=16)
a = ap.parse_args()


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}


def guided_lds_bytes(r, f):
    """guided_lds_bytes of denoise.hip: colour + variance on the 32x16 tile +- (r + f), 8 feature
    floats on the tile +- r, the colour-term plane on the tile +- f and its row sums.  A restatement
    (the library does not export the figure): keep it in step with denoise.hip.  The waves per CU
    below follow from it and the 160 KiB of LDS of an MI355X compute unit."""
    return 4 * (4 * (32 + 2 * (r + f)) * (16 + 2 * (r + f)) + 8 * (32 + 2 * r) * (16 + 2 * r)
                + (32 + 2 * f) * (16 + 2 * f) + (16 + 2 * f) * 32)


def run():
    import numpy as np
    import nori_amd
    import torch

    xml = os.path.join(ROOT, "scenes/pa4/cbox/cbox_path_mis.xml")
    s = nori_amd.load_scene(xml, a.size, a.size, 16)
    buf = torch.zeros((s.height, s.width, 8), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    for mode in (None, "bvh"):
        if mode:
            os.environ["NORI_TRAVERSAL"] = mode
        r = nori_amd.GpuRenderer(s, 0)
        os.environ.pop("NORI_TRAVERSAL", None)
        r.features(passes=a.passes, out=buf.data_ptr(), timing=True)
        kern, wall = [], []
        for _ in range(a.reps):
            t = time.perf_counter()
            r.features(passes=a.passes, out=buf.data_ptr(), timing=True)
            wall.append(1e3 * (time.perf_counter() - t))
            kern.append(r.last_stats["ms_shade"])
        print(json.dumps({"measurement": "k_features", "traversal": mode or "auto (scan)", "size": a.size,
                          "passes": a.passes, "bvh_nodes": r.last_stats["bvh_nodes"], "kernel_ms": spread(kern),
                          "call_ms": spread(wall),
                          "msamples_per_s": round(a.size * a.size * a.passes / statistics.median(kern) / 1e3, 1)}),
              flush=True)
        if mode is None:
            stats = np.zeros((s.height, s.width, 8), np.float32)
            img = nori_amd.develop(s, r.render(variance=stats))
            feat7 = nori_amd.film_features(s, r.features(passes=16))
            var = nori_amd.film_variance(s, stats).sum(axis=2)
        r.close()
    cases = [("k_guided defaults", lambda: nori_amd.denoise_guided(img, var, feat7), (5, 1)),
             ("k_guided r=8 f=3", lambda: nori_amd.denoise_guided(img, var, feat7, radius=8, patch=3), (8, 3)),
             ("k_nlmeans r=3 f=3", lambda: nori_amd.denoise(img, var, radius=3, patch=3, mode=1, script_scale=False), None)]
    for name, f, rf in cases:
        f()
        wall = []
        for _ in range(a.reps):
            t = time.perf_counter()
            f()
            wall.append(1e3 * (time.perf_counter() - t))
        out = {"measurement": name, "size": a.size, "call_ms_host_buffers": spread(wall)}
        if rf:
            lds = guided_lds_bytes(*rf)
            out.update({"lds_bytes": lds, "work_groups_per_cu": (160 * 1024) // lds,
                        "waves_per_cu": 4 * ((160 * 1024) // lds)})
        print(json.dumps(out), flush=True)


def trace():
    import re

    rows = []
    for path in glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(path)))
    groups = {}
    for row in sorted(rows, key=lambda r: int(r["Start_Timestamp"])):
        m = re.search(r"k_(features|guided|nlmeans)(<\d+>)?", row["Kernel_Name"])
        if m:
            groups.setdefault(m.group(0), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6)
    # `run` launches each case reps + 1 times (the first is its warm-up), case after case
    for name, v in groups.items():
        for i in range(0, len(v), a.reps + 1):
            c = v[i:i + a.reps + 1]
            print(json.dumps({"kernel": name, "case": i // (a.reps + 1), "dispatches": len(c), "first_ms": round(c[0], 4),
                              "ms_after_first": spread(c[1:]) if len(c) > 1 else None}))


{"run": run, "trace": trace}[a.what]()
