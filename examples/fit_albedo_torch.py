"""Per-shape albedos of a scene fitted to an image through the library's own film, in torch.

    python examples/fit_albedo_torch.py scenes/pa4/cbox/cbox_path_mis.xml --spp 4 --steps 200

The integrator is direct_ems written on the query API, in the order of examples/direct_torch.py,
split so that the parameter stays in torch.  For a diffuse BSDF f = albedo / pi, so a sample's
radiance is

    val = base + lit * ratio[shape]

with base the emission term, lit the sum of the unshadowed (f cos) Li terms computed with the
scene's own albedo, shape the hit's shape id and ratio a (num_shapes, 3) tensor: the albedo
relative to the scene's own (held at 1 for shapes whose BSDF is not diffuse).  pos, base, lit and
shape are computed once (prepare); every optimisation step is then

    ratio -> val (torch) -> nori_amd.autograd.film_splat_passes -> autograd.develop -> loss

and loss.backward() carries the image's gradient back through the scene's reconstruction filter
(its border and the block-tile clipping of ImageBlock::put included) with the film gather, the
splat's adjoint.  The command line builds the target with ratio = 1, starts from
grey albedos, runs Adam with ratio clamped at 0 and prints the loss and the recovered ratios.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nori-ray-tracer_amd"))
import nori_amd  # noqa: E402
from nori_amd import _abi, autograd  # noqa: E402

EPS = 1e-4  # NORI_EPSILON


def _pass(r, k, seed):
    """(base, lit, shape) of pass k's sample of every pixel: (n, 3), (n, 3) float32 and (n,) int64
    (a miss has shape num_shapes).  direct_ems as direct_torch.sample_radiance computes it, with the
    emission term and the light terms kept apart."""
    scene = r.scene
    n = scene.height * scene.width
    dev = torch.device("cuda", r.device)
    n_em = len(scene.emitters())

    def buf(cols):
        return torch.zeros((n, cols), dtype=torch.float32, device=dev)

    rays, surf, U = buf(8), buf(16), buf(max(2 * n_em, 1))
    torch.cuda.synchronize(dev)
    r.camera_rays(passes=1, pass_begin=k, seed=seed, out=rays.data_ptr())
    if n_em:
        r.sample_uniforms(4, 2 * n_em, passes=1, pass_begin=k, seed=seed, out=U)
    r.query(rays.data_ptr(), n=n, surf_out=surf.data_ptr())
    shape = surf[:, 11].view(torch.int32)
    hit = shape >= 0
    o = rays[:, 0:3].contiguous()
    view = (-rays[:, 4:7]).contiguous()
    p = surf[:, 0:3].contiguous()
    ee, es, be, hits = buf(4), buf(12), buf(8), buf(4)
    torch.cuda.synchronize(dev)
    r.emitter_eval(surf, o, n=n, out=ee)  # a miss record gives zeros
    base = torch.where(hit[:, None], ee[:, 0:3], torch.zeros_like(ee[:, 0:3]))
    lit = torch.zeros_like(base)
    for i in range(n_em):
        s2 = U[:, 2 * i:2 * i + 2].contiguous()
        torch.cuda.synchronize(dev)
        r.emitter_sample(p, s2, emitter=i, n=n, out=es)
        wi, maxt, Li = es[:, 0:3].contiguous(), es[:, 3], es[:, 4:7]
        sh = buf(8)
        sh[:, 0:3], sh[:, 3], sh[:, 4:7] = p, EPS, wi
        sh[:, 7] = torch.where(hit, maxt, torch.full_like(maxt, -1.0))  # maxt < mint: no hit
        torch.cuda.synchronize(dev)
        r.query(sh.data_ptr(), n=n, any_hit=True, hits_out=hits.data_ptr())
        r.bsdf_eval(surf, view, wi, n=n, out=be)
        free = (hits[:, 1].view(torch.int32) < 0) & hit
        f, cos = be[:, 0:3], be[:, 4]
        lit = torch.where(free[:, None], lit + (f * cos[:, None]) * Li, lit)
    return base, lit, torch.where(hit, shape, torch.full_like(shape, len(scene.shapes()))).long()


def prepare(r, spp, seed=0):
    """The per-sample data of passes 0 .. spp-1, computed once without a graph: "pos" (spp, H, W, 2)
    = pixel + draws 0, 1, "base" and "lit" (spp, H, W, 3), "shape" (spp, H, W) int64, and "diffuse"
    (num_shapes,) bool: the shapes whose BSDF is diffuse -- the rows of ratio that are fitted."""
    scene = r.scene
    dev = torch.device("cuda", r.device)
    H, W = scene.height, scene.width
    with torch.no_grad():
        ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
        jitter = torch.zeros((spp, H, W, 2), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        r.sample_uniforms(0, 2, passes=spp, seed=seed, out=jitter)
        pos = (torch.stack([xs, ys], -1).float()[None] + jitter).contiguous()
        per_pass = [_pass(r, k, seed) for k in range(spp)]
        base, lit, shape = (torch.stack([q[j] for q in per_pass]) for j in range(3))
    bsdfs = scene.bsdfs()
    diffuse = torch.tensor([sh.bsdf >= 0 and bsdfs[sh.bsdf].type == _abi.BSDF_DIFFUSE for sh in scene.shapes()],
                           dtype=torch.bool, device=dev)
    return {"spp": spp, "pos": pos, "base": base.reshape(spp, H, W, 3), "lit": lit.reshape(spp, H, W, 3),
            "shape": shape.reshape(spp, H, W), "diffuse": diffuse}


def image(r, data, ratio):
    """(H, W, 3): the samples with the albedo ratios `ratio` (num_shapes, 3) through the library's
    film (autograd.film_splat_passes) and ImageBlock::toBitmap (autograd.develop)."""
    eff = torch.where(data["diffuse"][:, None], ratio, torch.ones_like(ratio))
    eff = torch.cat([eff, torch.ones_like(eff[:1])])  # the row of a miss
    val = data["base"] + data["lit"] * eff[data["shape"]]
    film = autograd.film_splat_passes(r, data["pos"], val, passes=data["spp"])
    return autograd.develop(r.scene, film)


def loss(r, data, ratio, target):
    """The squared differences to `target`, summed in float64."""
    return ((image(r, data, ratio) - target).double() ** 2).sum()


def grey_ratios(scene, device, grey=0.5):
    """The ratios of albedo `grey` in every channel: grey / the scene's own albedo for a diffuse
    shape with a constant non-zero albedo, else 1."""
    bsdfs = scene.bsdfs()
    rows = []
    for sh in scene.shapes():
        b = bsdfs[sh.bsdf] if sh.bsdf >= 0 else None
        if b is not None and b.type == _abi.BSDF_DIFFUSE and b.albedo_texture == _abi.TEXTURE_CONSTANT and b.albedo_image < 0:
            rows.append([grey / a if a > 0 else 1.0 for a in b.albedo])
        else:
            rows.append([1.0, 1.0, 1.0])
    return torch.tensor(rows, dtype=torch.float32, device=device)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("scene")
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--width", type=int, default=0)
    ap.add_argument("--height", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    scene = nori_amd.load_scene(a.scene, a.width, a.height, a.spp)
    dev = torch.device("cuda", a.device)
    with nori_amd.GpuRenderer(scene, a.device) as r:
        data = prepare(r, a.spp, a.seed)
        with torch.no_grad():
            target = image(r, data, torch.ones((len(scene.shapes()), 3), device=dev))
        ratio = grey_ratios(scene, dev).requires_grad_(True)
        opt = torch.optim.Adam([ratio], lr=a.lr)
        first = last = None
        for step in range(a.steps + 1):
            opt.zero_grad()
            l = loss(r, data, ratio, target)
            last = float(l.detach())
            first = last if first is None else first
            if step == a.steps:
                break
            l.backward()
            opt.step()
            with torch.no_grad():
                ratio.clamp_(min=0.0)
    print(f"{os.path.basename(a.scene)}: {scene.width}x{scene.height}, {a.spp} spp, {a.steps} steps of Adam: "
          f"loss {first:.6e} -> {last:.6e}")
    for i, (row, d) in enumerate(zip(ratio.detach().cpu().tolist(), data["diffuse"].cpu().tolist())):
        print(f"  shape {i}: ratio " + " ".join(f"{v:.4f}" for v in row) + ("" if d else "  (not diffuse: held at 1)"))
    return first, last


if __name__ == "__main__":
    main()
