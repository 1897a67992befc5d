"""Measurements of the adaptive render (nori_gpu_render_adaptive) on GPU 0; prints JSON lines.

  python tools/adaptive_bench.py cost [--reps N] [--plain-only] [--pkg DIR]
      The cost of the round loop: render_adaptive at threshold 0 (every block with a non-zero
      error runs all rounds to the cap) against plain render() of the cap with statistics, both
      with the film and the statistics in device memory, alternating, after a warm-up of each;
      and the per-call time of GpuRenderer.block_error on device statistics.
      --plain-only times the plain render alone; with --pkg DIR (another build's package
      directory, e.g. the parent commit's) that is the same measurement on that build.
  python tools/adaptive_bench.py buys [--thresholds T,T,...] [--reps N]
      What it buys: for each threshold the samples taken, the wall time, the relMSE against a
      4096-spp uniform render (another seed) and the relMSE of the uniform render with the nearest
      equal sample count.

Scene: pa4/cbox/cbox_path_mis.xml at 512x512, min 32, cap 512 (--size, --min, --max).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["cost", "buys"])
ap.add_argument("--pkg", default=os.path.join(ROOT, "nori-ray-tracer_amd"))
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--min", type=int, default=32)
ap.add_argument("--max", type=int, default=512)
ap.add_argument("--ref-spp", type=int, default=4096)
ap.add_argument("--thresholds", default="0.01,0.015,0.02,0.03,0.04,0.05,0.065,0.08,0.1,0.13")
a = ap.parse_args()
sys.path[:0] = [os.path.abspath(a.pkg)]

import numpy as np  # noqa: E402
import nori_amd  # noqa: E402
import torch  # noqa: E402

s = nori_amd.load_scene(os.path.join(ROOT, "scenes/pa4/cbox/cbox_path_mis.xml"), a.size, a.size, a.max)
r = nori_amd.GpuRenderer(s, 0)
film = torch.zeros(s.film_shape(), dtype=torch.float32, device="cuda:0")
stat = torch.zeros((s.height, s.width, 8), dtype=torch.float32, device="cuda:0")
torch.cuda.synchronize()


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "n": len(v)}


def timed(f):
    """Host wall time (ms) of a blocking library call, and its result."""
    t = time.perf_counter()
    out = f()
    return 1e3 * (time.perf_counter() - t), out


def plain(passes=None):
    return r.render(passes=passes, device_ptr=film.data_ptr(), variance=stat.data_ptr())


def adaptive(thr):
    return r.render_adaptive(thr, min_passes=a.min, max_passes=a.max, device_ptr=film.data_ptr(),
                             variance=stat.data_ptr())


def cost():
    plain()  # warm-up of each shape the timed window uses
    if not a.plain_only:
        adaptive(0.0)
    tp, ta, tk = [], [], []
    for _ in range(a.reps):  # alternating
        tp.append(timed(plain)[0])
        if not a.plain_only:
            ms, (_, passes, _) = timed(lambda: adaptive(0.0))
            ta.append(ms)
    out = {"measurement": "cost", "package": os.path.relpath(os.path.abspath(a.pkg), ROOT), "size": a.size,
           "passes": a.max, "plain_samples": s.width * s.height * a.max, "plain_render_ms": spread(tp)}
    if not a.plain_only:
        # (a block whose error is exactly 0 -- every sample black -- stops even at threshold 0)
        out["adaptive_samples"] = r.last_stats["samples"]
        out["blocks_by_passes"] = {int(k): int((passes == k).sum()) for k in np.unique(passes)}
        for _ in range(10):
            r.block_error(stat.data_ptr())
        for _ in range(50):
            tk.append(timed(lambda: r.block_error(stat.data_ptr()))[0])
        rounds = 1
        while a.min << (rounds - 1) < a.max:
            rounds += 1
        out.update({"adaptive_threshold0_ms": spread(ta), "rounds": rounds,
                    "overhead_ms": round(statistics.median(ta) - statistics.median(tp), 3),
                    "overhead_percent": round(100 * (statistics.median(ta) / statistics.median(tp) - 1), 2),
                    "block_error_call_ms": spread(tk)})
    print(json.dumps(out), flush=True)


def rel_mse(img, ref):
    return float(np.mean((img.astype(np.float64) - ref) ** 2 / (ref ** 2 + 1e-2)))


def develop_device():
    return nori_amd.develop(s, film.cpu().numpy())


def buys():
    film.zero_()
    torch.cuda.synchronize()
    r.render(passes=a.ref_spp, seed=12345, device_ptr=film.data_ptr())
    ref = develop_device().astype(np.float64)
    adaptive(0.05)
    plain()
    npx = s.width * s.height
    for thr in [float(t) for t in a.thresholds.split(",")]:
        ta, tu = [], []
        for _ in range(a.reps):
            film.zero_()
            torch.cuda.synchronize()
            ms, (_, passes, _) = timed(lambda: adaptive(thr))
            ta.append(ms)
        taken = r.last_stats["samples"]
        img_a = develop_device()
        spp = max(1, int(round(taken / npx)))
        for _ in range(a.reps):
            film.zero_()
            torch.cuda.synchronize()
            tu.append(timed(lambda: plain(spp))[0])
        img_u = develop_device()
        counts = {int(k): int((passes == k).sum()) for k in np.unique(passes)}
        print(json.dumps({"measurement": "buys", "threshold": thr, "samples": taken,
                          "share_of_uniform": round(taken / (npx * a.max), 4), "blocks_by_passes": counts,
                          "adaptive_ms": spread(ta), "adaptive_relmse": rel_mse(img_a, ref),
                          "uniform_spp": spp, "uniform_ms": spread(tu), "uniform_relmse": rel_mse(img_u, ref)}),
              flush=True)


{"cost": cost, "buys": buys}[a.what]()
r.close()
