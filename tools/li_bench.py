"""Timings of nori_gpu_li against nori_gpu_render on an MI355X.

    python tools/li_bench.py [OUTDIR] [cbox c3]     -> OUTDIR/li_bench.json

Per scene -- cbox_path_mis (scan mode) and the C3 height field of nori_amd/configs.py (BVH mode),
both 512 x 512 -- the camera rays of 16 passes are made once in a device buffer (camera_rays);
then, alternating and repeated 5 times after one warm-up round, li on those rays (ms_shade, the
HIP-event time of k_li) and render of the same 16 passes into a device film (ms_total).  Reported:
the median, min and max of each, rays/s of li and the ratio li / render.  Then the knobs, each
value timed 3 times in alternation with the others: NORI_LI_REFILL 0 / 1 and NORI_LI_RANGE
128 / 256 / 1024."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "nori-ray-tracer_amd")]
import nori_amd  # noqa: E402
from nori_amd import configs  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "bench_out")
SCENES = sys.argv[2:] or ["cbox", "c3"]
W = H = 512
PASSES = 16
SEED = 3


def med(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "n": len(v)}


class env:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update({k: str(v) for k, v in self.kw.items()})

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def bench(name, xml, res):
    import torch
    dev = torch.device("cuda", 0)
    s = nori_amd.load_scene(xml, W, H, PASSES)
    n = PASSES * H * W
    with nori_amd.GpuRenderer(s, 0) as r:
        rays = torch.zeros((n, 8), dtype=torch.float32, device=dev)
        out = torch.zeros((n, 3), dtype=torch.float32, device=dev)
        film = torch.zeros(s.film_shape(), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        r.camera_rays(passes=PASSES, seed=SEED, out=rays.data_ptr())

        def li():
            r.li(rays, seed=SEED, stream_base=0, first_draw=4, n=n, out=out)
            return r.last_stats

        t_li, t_render = [], []
        for i in range(6):
            st = li()
            r.render(passes=PASSES, seed=SEED, device_ptr=film.data_ptr())
            if i:
                t_li.append(st["ms_shade"])
                t_render.append(r.last_stats["ms_total"])
        e = {"rays": n, "rays_closest": st["rays_closest"], "rays_shadow": st["rays_shadow"],
             "invalid": st["invalid_samples"], "li_ms": med(t_li), "render_ms": med(t_render)}
        e["li_Mrays_s"] = n / e["li_ms"]["median"] / 1e3
        e["li_over_render"] = e["li_ms"]["median"] / e["render_ms"]["median"]
        res[name] = e
        print(name, json.dumps(e), flush=True)
        knobs = [("NORI_LI_REFILL", (0, 1)), ("NORI_LI_RANGE", (128, 256, 1024))]
        for var, values in knobs:
            times = {v: [] for v in values}
            for _ in range(3):
                for v in values:
                    with env(**{var: v}):
                        times[v].append(li()["ms_shade"])
            e[var] = {str(v): med(t) for v, t in times.items()}
            print(name, var, json.dumps(e[var]), flush=True)


def main():
    os.makedirs(OUT, exist_ok=True)
    res = {"width": W, "height": H, "passes": PASSES}
    for name in SCENES:
        if name == "cbox":
            xml = os.path.join(ROOT, "scenes/pa4/cbox/cbox_path_mis.xml")
        else:
            xml = configs.config_scene("c3", os.path.join(OUT, "scenes"))[0]
        bench(name, xml, res)
    with open(os.path.join(OUT, "li_bench.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
