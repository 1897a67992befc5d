"""Command line mirror of `nori_euler <scene.xml>` (src/main_euler.cpp:24-60 ->
RenderThread::renderScene, render.cpp:135-280):

    python -m nori_amd scene.xml [--width W --height H --spp N] [--gpus G] [--png]
                                 [--adaptive T [--min-spp N]] [--features [N]] [--denoise]

Parses the scene, renders it on the GPU(s) and writes `<stem>.exr` and
`<stem>_variance.exr` next to the XML (render.cpp:158-169), plus `<stem>.png`
with --png (Bitmap::saveToLDR, the hdrToLdr tool).  With --gpus G > 1 one
context per device renders a slice of the sample passes on its own host
thread and the RGBW films are summed (ImageBlock::put(block), block.cpp:124-133).
With --adaptive T (one GPU) blocks stop once their error E_b is at most T
(GpuRenderer.render_adaptive; --spp or the XML's sampleCount is the cap,
--min-spp the first round) and `<stem>_samples.exr` holds each pixel's valid
sample count.
With --features [N] the first-hit features of N sample passes (default 16,
at most the spp; GpuRenderer.features) are written as `<stem>_albedo.exr`,
`<stem>_normal.exr` and `<stem>_depth.exr` (the depth in all three channels).
--denoise implies them and writes `<stem>_denoised.exr` (and `.png` with
--png): the feature-guided denoiser with its default parameters
(denoise_guided) on the image, its variance and the features.
"""
import argparse
import os
import sys
import threading
import time

import numpy as np

from . import (GpuRenderer, NoriError, denoise_guided, develop, device_count, film_features, film_variance, load_scene,
               write_exr, write_png)


def _features(a, scene, r):
    """--features / --denoise: the (H, W, 7) feature means taken on the render's context, else None."""
    if a.features is None and not a.denoise:
        return None
    n_feat = max(1, min(16 if a.features is None else a.features, scene.spp))
    return film_features(scene, r.features(passes=n_feat))


def _render_adaptive(a, scene):
    """--adaptive: (film, statistics, features) of one adaptive render on device 0."""
    stats = np.zeros((scene.height, scene.width, 8), np.float32)
    print("Rendering .. ", end="", flush=True)
    t0 = time.time()
    with GpuRenderer(scene, 0) as r:
        film, passes, _ = r.render_adaptive(a.adaptive, min_passes=a.min_spp, variance=stats)
        taken = r.last_stats["samples"]
        feat7 = _features(a, scene, r)
    print(f"done. (took {1e3 * (time.time() - t0):.1f}ms)")
    uniform = scene.width * scene.height * scene.spp
    print(f"Adaptive sampling: {taken} of {uniform} samples ({100.0 * taken / uniform:.1f} %), "
          f"{int(passes.min())} to {int(passes.max())} passes per block")
    return film, stats, feat7


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nori_amd", description=__doc__.split("\n\n")[0])
    ap.add_argument("scene")
    ap.add_argument("--width", type=int, default=0)
    ap.add_argument("--height", type=int, default=0)
    ap.add_argument("--spp", type=int, default=0)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--png", action="store_true", help="also write <stem>.png (sRGB, 8 bit)")
    ap.add_argument("--adaptive", type=float, default=None, metavar="T",
                    help="adaptive sampling: a 32x32 block stops once its error is at most T; "
                         "also writes <stem>_samples.exr")
    ap.add_argument("--min-spp", type=int, default=8, help="adaptive sampling: passes of the first round")
    ap.add_argument("--features", type=int, nargs="?", const=16, default=None, metavar="N",
                    help="write the first-hit features of N sample passes (default 16, at most the spp) as "
                         "<stem>_albedo.exr, <stem>_normal.exr and <stem>_depth.exr")
    ap.add_argument("--denoise", action="store_true",
                    help="feature-guided denoiser with its default parameters: writes <stem>_denoised.exr "
                         "(implies --features)")
    a = ap.parse_args(argv)
    if a.adaptive is not None and a.gpus > 1:
        print("Fatal error: adaptive rendering runs on one GPU (--gpus 1)", file=sys.stderr)
        return 1
    try:
        scene = load_scene(a.scene, a.width, a.height, a.spp)
        stem = os.path.splitext(a.scene)[0]
        if a.adaptive is not None:
            film, stat, feat7 = _render_adaptive(a, scene)
            image = develop(scene, film)
        else:
            n = max(1, min(a.gpus, device_count()))
            spp = scene.spp
            renderers = [GpuRenderer(scene, d) for d in range(n)]
            films = [np.zeros(scene.film_shape(), np.float32) for _ in range(n)]
            stats = [np.zeros((scene.height, scene.width, 8), np.float32) for _ in range(n)]
            errors = []

            def run(i):
                b, e = spp * i // n, spp * (i + 1) // n
                try:
                    if e > b:
                        renderers[i].render(passes=e - b, pass_begin=b, out=films[i], variance=stats[i])
                except NoriError as err:
                    errors.append(err)

            print("Rendering .. ", end="", flush=True)
            t0 = time.time()
            threads = [threading.Thread(target=run, args=(i,)) for i in range(n)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
            if errors:
                raise errors[0]
            print(f"done. (took {1e3 * (time.time() - t0):.1f}ms)")
            feat7 = _features(a, scene, renderers[0])
            for r in renderers:
                r.close()
            image = develop(scene, np.sum(films, axis=0))
            stat = np.sum(stats, axis=0)
        print(f"Writing a {scene.width}x{scene.height} OpenEXR file to \"{stem}.exr\"")
        write_exr(stem + ".exr", image)
        write_exr(stem + "_variance.exr", film_variance(scene, stat))
        if a.adaptive is not None:
            write_exr(stem + "_samples.exr", np.repeat(stat[..., 6:7], 3, axis=2))
        if a.png:
            print(f"Writing a {scene.width}x{scene.height} PNG file to \"{stem}.png\"")
            write_png(stem + ".png", image)
        if feat7 is not None:
            write_exr(stem + "_albedo.exr", feat7[..., 0:3])
            write_exr(stem + "_normal.exr", feat7[..., 3:6])
            write_exr(stem + "_depth.exr", np.repeat(feat7[..., 6:7], 3, axis=2))
            if a.denoise:
                print(f"Writing the denoised image to \"{stem}_denoised.exr\"")
                denoised = denoise_guided(image, film_variance(scene, stat).sum(axis=2), feat7)
                write_exr(stem + "_denoised.exr", denoised)
                if a.png:
                    write_png(stem + "_denoised.png", denoised)
    except NoriError as e:
        print(f"Fatal error: {e}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
