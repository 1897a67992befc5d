"""Ambient occlusion from torch tensors: a user-written integrator on the ray-query API.

    python examples/ao_torch.py scenes/pa4/cbox/cbox_path_mis.xml ao.png --width 256 --height 256

The flow a custom integrator takes -- every buffer is a torch tensor on the GPU and nothing is
copied to the host before the final image:

  1. GpuRenderer.camera_rays(out=tensor)      the renderer's own primary rays (any camera plugin)
  2. GpuRenderer.query(rays, surf_out=...)    closest hits with the full record (p, ng, ns, uv, ...)
  3. torch                                    cosine-weighted directions about the shading normal
  4. GpuRenderer.query(..., any_hit=True)     occlusion within `radius`

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


def _frame(n):
    """Tangent vectors (s, t) of unit normals n (N, 3): coordinateSystem of the reference (common.cpp:274-283)."""
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    zero = torch.zeros_like(x)
    big = x.abs() > y.abs()
    inv = torch.rsqrt(torch.where(big, x, y) ** 2 + z * z)
    t = torch.where(big[:, None], torch.stack([z * inv, zero, -x * inv], 1), torch.stack([zero, z * inv, -y * inv], 1))
    return torch.linalg.cross(t, n), t


def ao_image(renderer, directions=16, radius=1.0, seed=0, pass_begin=0):
    """(H, W) float32 cuda tensor: the share of `directions` cosine-weighted directions about the
    first hit's shading normal (turned towards the camera) that are unoccluded within `radius`;
    0 where the primary ray misses."""
    scene = renderer.scene
    H, W = scene.height, scene.width
    n = H * W
    dev = torch.device("cuda", renderer.device)
    gen = torch.Generator(device=dev).manual_seed(seed)

    rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
    surf = torch.empty((n, 16), dtype=torch.float32, device=dev)  # nori_gpu_surface: 64 bytes
    torch.cuda.synchronize(dev)
    renderer.camera_rays(passes=1, pass_begin=pass_begin, seed=seed, out=rays.data_ptr())
    renderer.query(rays.data_ptr(), n=n, surf_out=surf.data_ptr())

    hit = surf[:, 7].view(torch.int32) >= 0  # prim
    p, ns = surf[:, 0:3], surf[:, 8:11]
    facing = (ns * rays[:, 4:7]).sum(1) < 0
    nrm = torch.where(facing[:, None], ns, -ns)
    nrm = torch.where(hit[:, None], nrm, torch.tensor([0.0, 0.0, 1.0], device=dev))
    s, t = _frame(nrm)
    eps = 1e-4 * (1 + p.abs().amax(1))  # the reference's adaptive epsilon (bvh.cpp:404-462)

    shadow = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    occluded = torch.empty((n, 4), dtype=torch.float32, device=dev)  # nori_gpu_hit: 16 bytes
    free = torch.zeros(n, dtype=torch.float32, device=dev)
    for _ in range(directions):
        u = torch.rand((n, 2), generator=gen, device=dev)
        r, phi = u[:, 0].sqrt(), 2 * math.pi * u[:, 1]
        loc = torch.stack([r * phi.cos(), r * phi.sin(), (1 - u[:, 0]).clamp_min(0).sqrt()], 1)
        shadow[:, 0:3] = torch.where(hit[:, None], p, torch.zeros_like(p))
        shadow[:, 3] = eps
        shadow[:, 4:7] = s * loc[:, 0:1] + t * loc[:, 1:2] + nrm * loc[:, 2:3]
        shadow[:, 7] = torch.where(hit, torch.full_like(eps, radius), torch.full_like(eps, -1.0))  # maxt < mint: no hit
        torch.cuda.synchronize(dev)
        renderer.query(shadow.data_ptr(), n=n, any_hit=True, hits_out=occluded.data_ptr())
        free += (occluded[:, 1].view(torch.int32) < 0).float()
    ao = torch.where(hit, free / directions, torch.zeros_like(free))
    return ao.reshape(H, W)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("scene")
    ap.add_argument("output", help="PNG file")
    ap.add_argument("--width", type=int, default=0)
    ap.add_argument("--height", type=int, default=0)
    ap.add_argument("--directions", type=int, default=16)
    ap.add_argument("--radius", type=float, default=1.0)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    scene = nori_amd.load_scene(a.scene, a.width, a.height, 1)
    with nori_amd.GpuRenderer(scene, a.device) as r:
        ao = ao_image(r, a.directions, a.radius)
    img = ao.cpu().numpy()  # the first host copy
    nori_amd.write_png(a.output, img[..., None].repeat(3, -1))
    print(f"{a.output}: {scene.width}x{scene.height}, {a.directions} directions, mean {img.mean():.3f}")


if __name__ == "__main__":
    main()
