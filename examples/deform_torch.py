"""An animated mesh from torch tensors: the vertices move on the GPU, the BVH is refitted there.

    NORI_TRAVERSAL=bvh python examples/deform_torch.py scenes/pa4/cbox/cbox_path_mis.xml frame --frames 8

Per frame -- every buffer is a torch tensor on the GPU and nothing is copied to the host before a
frame is written:

  1. torch                                        the rest positions displaced by an expression of the time
  2. GpuRenderer.update_vertices(tensor)          pos / triangle records rewritten, boxes refitted (no rebuild)
     GpuRenderer.rebuild_bvh()                    with --rebuild-every N, every N-th frame: a new tree for the
                                                  positions as they are now, built on the GPU
  3. GpuRenderer.camera_rays(out=tensor)          the renderer's own primary rays
  4. GpuRenderer.query(rays, surf_out=...)        closest hits on the new geometry: a normals image

A context updates its vertices only if it walks a BVH: scenes of at most 64 primitives are
scanned by default (NORI_TRAVERSAL=bvh at creation switches them to the walk).  Spheres do not
move.  The library's calls block, and update_vertices waits for the work torch has queued on a
tensor it is given; camera_rays and query take raw addresses, so torch.cuda.synchronize() comes
before them (see ao_torch.py).
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nori-ray-tracer_amd"))
import nori_amd  # noqa: E402


def displaced(rest, time, amplitude):
    """A travelling wave along x that lifts y and shears z; `rest` is (V, 3)."""
    phase = 6.0 * rest[:, 0] + 2.0 * math.pi * time
    out = rest.clone()
    out[:, 1] += amplitude * torch.sin(phase)
    out[:, 2] += 0.5 * amplitude * torch.cos(phase + 3.0 * rest[:, 1])
    return out


def normals_image(renderer, rays, surf):
    """(H, W, 3) float32 cuda tensor: |shading normal| at the first hit, 0 on a miss (the `normals` integrator)."""
    scene = renderer.scene
    n = scene.height * scene.width
    renderer.camera_rays(passes=1, out=rays.data_ptr())
    renderer.query(rays.data_ptr(), n=n, surf_out=surf.data_ptr())
    hit = surf[:, 7].view(torch.int32) >= 0  # prim
    img = torch.where(hit[:, None], surf[:, 8:11].abs(), torch.zeros_like(surf[:, 8:11]))
    return img.reshape(scene.height, scene.width, 3)


def deform_frames(renderer, frames=8, amplitude=0.05, rebuild_every=0):
    """`frames` normals images of the scene under displaced(): a list of (H, W, 3) cuda tensors.
    rebuild_every = N > 0: the BVH is rebuilt on the device after the update of every N-th frame
    (a refit keeps the topology chosen for the positions as loaded); 0: refits only."""
    scene = renderer.scene
    dev = torch.device("cuda", renderer.device)
    rest = torch.from_numpy(scene.positions()).to(dev)  # the one upload: the geometry as loaded
    n = scene.height * scene.width
    rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
    surf = torch.empty((n, 16), dtype=torch.float32, device=dev)  # nori_gpu_surface: 64 bytes
    out = []
    for f in range(frames):
        renderer.update_vertices(displaced(rest, f / max(frames, 1), amplitude))
        if rebuild_every > 0 and (f + 1) % rebuild_every == 0:
            renderer.rebuild_bvh()
        torch.cuda.synchronize(dev)
        out.append(normals_image(renderer, rays, surf).clone())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("scene")
    ap.add_argument("output", help="stem of the PNG files: <stem>_000.png, ...")
    ap.add_argument("--width", type=int, default=0)
    ap.add_argument("--height", type=int, default=0)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--amplitude", type=float, default=0.05)
    ap.add_argument("--rebuild-every", type=int, default=0, metavar="N",
                    help="rebuild the BVH on the device every N-th frame (default 0: refit only)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    scene = nori_amd.load_scene(a.scene, a.width, a.height, 1)
    with nori_amd.GpuRenderer(scene, a.device) as r:
        imgs = deform_frames(r, a.frames, a.amplitude, a.rebuild_every)
    for i, img in enumerate(imgs):
        nori_amd.write_png(f"{a.output}_{i:03d}.png", img.cpu().numpy())  # the first host copy of a frame
    print(f"{a.output}_000.png .. {len(imgs) - 1:03d}.png: {scene.width}x{scene.height}")


if __name__ == "__main__":
    main()
