"""A lat-long (equirectangular) panorama from the scene camera's origin, through the radiance query.

    python examples/panorama_torch.py scenes/pa4/cbox/cbox_path_mis.xml out.png --spp 16 [--width 256 --height 128]

The library's cameras are perspective ones; this camera is written here, in torch, and the
scene's own integrator -- any of the ten -- runs along its rays through GpuRenderer.li:

  camera (torch) -> GpuRenderer.li -> GpuRenderer.film_splat_passes -> develop (torch)

Per pass, on tensors that never leave the GPU:
  1. the jittered directions: pixel (x, y) at position pos = (x + u0, y + u1), with u0, u1 the
     renderer's own jitter draws of sample (pass, pixel) (sample_uniforms draws 0, 1), looks along
     phi = 2 pi pos.x / W around the camera's up axis and theta = pi pos.y / H down from it;
  2. li with the streams of (pass, pixel) and first_draw = 4, the draw at which the built-in
     integrators start: each sample continues the stream its jitter came from;
  3. film_splat_passes at pos: the scene's reconstruction filter, as the renderer applies it;
  4. the film developed: rgb / weight.
The first host copy is the finished image.

The library runs on its own stream and its calls block, so the only synchronisation needed is
torch.cuda.synchronize() before a call that reads what torch has just written.
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nori-ray-tracer_amd"))
import nori_amd  # noqa: E402

EPS = 1e-4  # NORI_EPSILON


def camera_frame(scene, dev):
    """(origin, right, up, forward) of the scene's camera: the columns of cameraToWorld."""
    m = torch.tensor(list(scene.desc.camera.camera_to_world), dtype=torch.float32, device=dev).reshape(4, 4)
    unit = lambda v: v / v.norm()  # noqa: E731
    return m[0:3, 3].clone(), unit(m[0:3, 0]), unit(m[0:3, 1]), unit(m[0:3, 2])


def panorama_rays(scene, pos, dev):
    """(H * W, 8) rays for the sample positions pos (H, W, 2) in pixel units."""
    H, W = scene.height, scene.width
    o, right, up, fwd = camera_frame(scene, dev)
    phi = pos[..., 0] * (2.0 * math.pi / W) - math.pi  # the image centre looks forward
    theta = pos[..., 1] * (math.pi / H)
    st = torch.sin(theta)
    d = (st * torch.sin(phi))[..., None] * right + torch.cos(theta)[..., None] * up + (st * torch.cos(phi))[..., None] * fwd
    rays = torch.empty((H * W, 8), dtype=torch.float32, device=dev)
    rays[:, 0:3] = o
    rays[:, 3] = EPS
    rays[:, 4:7] = d.reshape(-1, 3)
    rays[:, 7] = float("inf")
    return rays


def develop(scene, film):
    """(H, W, 3): the film's rgb over its filter weight (ImageBlock::toBitmap), on the device."""
    b = scene.border
    core = film[b:film.shape[0] - b, b:film.shape[1] - b]
    w = core[..., 3:4]
    return torch.where(w != 0, core[..., 0:3] / w, torch.zeros_like(core[..., 0:3]))


def panorama(r, spp=4, seed=0, on_pass=None):
    """(H, W, 3) float32 cuda tensor: the panorama after spp passes.  on_pass(k, image) is called
    with the image developed after every pass (a progressive preview), if given."""
    scene = r.scene
    dev = torch.device("cuda", r.device)
    H, W = scene.height, scene.width
    n = H * W
    film = torch.zeros(scene.film_shape(), dtype=torch.float32, device=dev)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    pixel = torch.stack([xs, ys], -1).float()
    jitter = torch.zeros((1, H, W, 2), dtype=torch.float32, device=dev)
    val = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    image = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    for k in range(spp):
        torch.cuda.synchronize(dev)
        r.sample_uniforms(0, 2, passes=1, pass_begin=k, seed=seed, out=jitter)
        pos = (pixel + jitter[0]).contiguous()
        rays = panorama_rays(scene, pos, dev)
        torch.cuda.synchronize(dev)
        r.li(rays, seed=seed, stream_base=k * n, first_draw=4, n=n, out=val)
        r.film_splat_passes(pos, val, passes=1, out=film)
        image = develop(scene, film)
        if on_pass:
            on_pass(k, image)
    return image


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("scene")
    ap.add_argument("output", help="PNG file")
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--width", type=int, default=0)
    ap.add_argument("--height", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    scene = nori_amd.load_scene(a.scene, a.width, a.height, 1)
    with nori_amd.GpuRenderer(scene, a.device) as r:
        img = panorama(r, a.spp, a.seed).cpu().numpy()  # the first host copy
        invalid = r.last_stats["invalid_samples"]
    nori_amd.write_png(a.output, img)
    print(f"{a.output}: {scene.width}x{scene.height} lat-long, {scene.integrator}, "
          f"{a.spp} spp, mean {img.mean():.4f}, {invalid} samples dropped in the last pass")


if __name__ == "__main__":
    main()
