"""Fit a mesh to depth and normal images: gradients of hit records in the vertices, in torch.

    NORI_TRAVERSAL=bvh python examples/fit_mesh_torch.py [scene.xml] --steps 100

The scene's largest mesh (by default the height field of nori_amd.configs.heightfield_scene) is
displaced along y by a smooth expression; camera_rays + query on that copy give the target: a
depth image t and a geometric-normal image ng.  Starting from the rest positions, Adam minimises
the squared difference of t and ng over the pixels that hit the mesh in both images, moving the
mesh's y coordinates (--free xyz: all three):

  1. autograd.surface(r, rays, positions)      update_vertices + query; the records carry a graph
  2. torch                                      the loss on rec[:, 3] (t) and rec[:, 4:7] (ng)
  3. loss.backward()                            nori_gpu_surface_grad: the records' adjoint in the
                                                vertices, summed per triangle on chip before the atomics

Every buffer is a torch tensor on the GPU.  What the gradient sees: t along the fixed camera ray
and ng, on the triangles the rays hit now -- the hit set is held, so a silhouette does not pull,
and vertices no ray reaches do not move.  --rebuild-every k builds a new BVH every k-th step (a
refit keeps the tree chosen for the rest positions).  A context moves its vertices only if it
walks a BVH: NORI_TRAVERSAL=bvh for scenes of at most 64 primitives.
"""
import argparse
import os
import sys
import tempfile

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nori-ray-tracer_amd"))
import nori_amd  # noqa: E402
from nori_amd import autograd, configs  # noqa: E402


def largest_mesh(scene):
    """(shape index, vertex slice, first global primitive id, triangle count) of the mesh with the most vertices."""
    first, best = 0, None
    for i, sh in enumerate(scene.shapes()):
        sphere = sh.type == nori_amd._abi.SHAPE_SPHERE
        if not sphere and (best is None or sh.vtx_count > best[1].stop - best[1].start):
            best = (i, slice(sh.vtx_offset, sh.vtx_offset + sh.vtx_count), first, sh.tri_count)
        first += 1 if sphere else sh.tri_count
    if best is None:
        raise SystemExit("the scene has no mesh")
    return best


def displaced(rest, sl, amplitude):
    """The target geometry: the mesh's vertices lifted along y by a smooth function of x and z."""
    out = rest.clone()
    x, z = rest[sl, 0], rest[sl, 2]
    out[sl, 1] += amplitude * (torch.sin(4.0 * x + 0.5) * torch.cos(3.0 * z - 0.2) + 0.5 * torch.sin(2.0 * (x + z)))
    return out


def on_mesh(hits, first, count):
    prim = hits[:, 1].view(torch.int32)
    return (prim >= first) & (prim < first + count)


def fit(r, steps=100, amplitude=0.03, lr=None, rebuild_every=0, free="y", log=print):
    """Runs the fit on context `r`; returns (first loss, last loss, initial and final RMS vertex error).
    free: "y" -- the vertices move along y only, the axis of the displacement (one unknown per
    vertex); "xyz" -- all three coordinates (the images do not determine a vertex's slide within
    its surface, so the vertex error need not fall with the loss)."""
    scene = r.scene
    dev = torch.device("cuda", r.device)
    _, sl, first, count = largest_mesh(scene)
    rest = torch.from_numpy(scene.positions()).to(dev)
    goal = displaced(rest, sl, amplitude)
    n = scene.height * scene.width
    rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    r.camera_rays(passes=1, out=rays.data_ptr())
    with torch.no_grad():
        rec, hits = autograd.surface(r, rays, goal)
        tgt_t, tgt_ng, tgt_on = rec[:, 3].clone(), rec[:, 4:7].clone(), on_mesh(hits, first, count)
    param = rest[sl].clone().requires_grad_(True)
    axes = torch.tensor([0.0, 1.0, 0.0] if free == "y" else [1.0, 1.0, 1.0], device=dev)
    opt = torch.optim.Adam([param], lr=lr if lr is not None else amplitude / 15.0)
    losses = []
    rms = lambda: float((((rest[sl] + (param.detach() - rest[sl]) * axes) - goal[sl]) ** 2).sum(1).mean().sqrt())  # noqa: E731
    rms0 = rms()
    for step in range(steps):
        opt.zero_grad()
        pos = torch.cat([rest[:sl.start], rest[sl] + (param - rest[sl]) * axes, rest[sl.stop:]])
        rec, hits = autograd.surface(r, rays, pos)
        if rebuild_every > 0 and (step + 1) % rebuild_every == 0:
            # a new tree for the same vertices: the hits do not change, but the context's geometry
            # counter does, so the records are taken again on the rebuilt tree
            r.rebuild_bvh()
            rec, hits = autograd.surface(r, rays, pos)
        both = tgt_on & on_mesh(hits, first, count)
        k = max(int(both.sum()), 1)
        dt = torch.where(both, rec[:, 3] - tgt_t, torch.zeros_like(tgt_t))
        dn = torch.where(both[:, None], rec[:, 4:7] - tgt_ng, torch.zeros_like(tgt_ng))
        loss = ((dt * dt).sum() + (dn * dn).sum()) / k
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        log(f"step {step:4d}  loss {losses[-1]:.6e}  pixels {k}")
    log(f"RMS vertex error against the displaced copy: {rms0:.6e} -> {rms():.6e} "
        f"({sl.stop - sl.start} vertices, amplitude {amplitude:g})")
    return losses[0], losses[-1], rms0, rms()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("scene", nargs="?", help="default: a 32 x 32 cell height field in the Cornell box")
    ap.add_argument("--width", type=int, default=0)
    ap.add_argument("--height", type=int, default=0)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--amplitude", type=float, default=0.03)
    ap.add_argument("--lr", type=float, default=None, help="Adam's step (default amplitude / 15)")
    ap.add_argument("--rebuild-every", type=int, default=0, metavar="K", help="rebuild the BVH every K-th step")
    ap.add_argument("--free", choices=("y", "xyz"), default="y", help="the coordinates the fit may move (default y)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        if a.scene:
            scene = nori_amd.load_scene(a.scene, a.width, a.height, 1)
        else:
            scene = nori_amd.load_scene(configs.heightfield_scene(tmp, n=32, width=a.width or 128, height=a.height or 128, spp=1))
        print(f"{scene.width}x{scene.height}, {a.steps} steps of Adam")
        with nori_amd.GpuRenderer(scene, a.device) as r:
            return fit(r, a.steps, a.amplitude, a.lr, a.rebuild_every, a.free)


if __name__ == "__main__":
    main()
