"""BSDF parameters of a scene fitted to an image through the library's own shading and film, in torch.

    python examples/fit_material_torch.py --scene veach --spp 4 --steps 200
    python examples/fit_material_torch.py --scene disney

The integrator is direct_ems written on the query API, in the order of examples/direct_torch.py
(sample_radiance), with the BSDF evaluated by nori_amd.autograd.bsdf_eval: the material rows are a
torch tensor, the library evaluates f and the cosine for them, and loss.backward() reaches the
rows through nori_gpu_bsdf_grad.  Nothing of microfacet.cpp or disney.cpp is
restated here.  Everything that does not depend on the materials is computed once (prepare):
the camera rays, the hit records, the light samples, their shadow rays and the emission term.
Every optimisation step is then

    theta -> rows (torch) -> autograd.bsdf_eval (one call over all passes and lights)
          -> val = base + sum of the unshadowed (f cos) Li -> autograd.film_splat_passes
          -> autograd.develop -> loss

--scene veach: the four microfacet plates' alpha and kd of scenes/pa3/veach_mi/veach_ems.xml; the
target is the scene's own built-in render (its integrator is direct_ems, so the composition
reproduces it sample for sample at the scene's own values).  --scene disney: roughness and
base_color of the Disney sphere of scenes/project/disney/cbox_path_mis.xml; that scene's
integrator is path_mis, whose indirect light this composition does not model, so the target is
the composition itself at the scene's own values.  The fit starts from perturbed rows; the fitted
words are positive and parametrised as start * exp(theta), optimised with Adam.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nori-ray-tracer_amd"))
import nori_amd  # noqa: E402
from nori_amd import _abi, autograd  # noqa: E402

EPS = 1e-4  # NORI_EPSILON
SCENES = {"veach": ("scenes/pa3/veach_mi/veach_ems.xml", _abi.BSDF_MICROFACET, (0, 1, 2, 3)),   # kd, alpha
          "disney": ("scenes/project/disney/cbox_path_mis.xml", _abi.BSDF_DISNEY, (0, 1, 2, 6))}  # base_color, roughness


def prepare(r, spp, seed=0):
    """What a step needs and the materials do not change, for passes 0 .. spp-1 and every light:
    pos (spp, H, W, 2) sample positions; base (spp, n, 3) the emission term; and, concatenated over
    passes and lights, surf (m, 16), view (m, 3), wi (m, 3), Li (m, 3), lit (m,) bool (the surface
    is hit and the light sample is unshadowed), with m = spp * lights * n."""
    scene = r.scene
    H, W = scene.height, scene.width
    n = H * W
    dev = torch.device("cuda", r.device)
    n_em = len(scene.emitters())

    def buf(cols):
        return torch.zeros((n, cols), dtype=torch.float32, device=dev)

    ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    pixel = torch.stack([xs, ys], -1).float()
    pos, base, parts = [], [], []
    for k in range(spp):
        rays, surf, U, jit = buf(8), buf(16), buf(max(2 * n_em, 1)), torch.zeros((1, H, W, 2), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        r.camera_rays(passes=1, pass_begin=k, seed=seed, out=rays.data_ptr())
        r.sample_uniforms(0, 2, passes=1, pass_begin=k, seed=seed, out=jit)
        if n_em:
            r.sample_uniforms(4, 2 * n_em, passes=1, pass_begin=k, seed=seed, out=U)
        r.query(rays.data_ptr(), n=n, surf_out=surf.data_ptr())
        hit = surf[:, 11].view(torch.int32) >= 0
        o, view, p = rays[:, 0:3].contiguous(), (-rays[:, 4:7]).contiguous(), surf[:, 0:3].contiguous()
        ee, es, hits = buf(4), buf(12), buf(4)
        torch.cuda.synchronize(dev)
        r.emitter_eval(surf, o, n=n, out=ee)
        pos.append(pixel + jit[0])
        base.append(torch.where(hit[:, None], ee[:, 0:3], torch.zeros_like(ee[:, 0:3])))
        for i in range(n_em):
            s2 = U[:, 2 * i:2 * i + 2].contiguous()
            torch.cuda.synchronize(dev)
            r.emitter_sample(p, s2, emitter=i, n=n, out=es)
            wi, maxt, Li = es[:, 0:3].contiguous(), es[:, 3], es[:, 4:7].clone()
            sh = buf(8)
            sh[:, 0:3], sh[:, 3], sh[:, 4:7] = p, EPS, wi
            sh[:, 7] = torch.where(hit, maxt, torch.full_like(maxt, -1.0))  # maxt < mint: no hit
            torch.cuda.synchronize(dev)
            r.query(sh.data_ptr(), n=n, any_hit=True, hits_out=hits.data_ptr())
            free = hits[:, 1].view(torch.int32) < 0
            parts.append((surf, view, wi, Li, hit & free))
    cat = [torch.cat([q[j] for q in parts]).contiguous() for j in range(5)]
    return torch.stack(pos).contiguous(), torch.stack(base), cat, n_em


def image(r, rows, prep, spp):
    """The developed (H, W, 3) image of the composition at the material rows `rows`."""
    pos, base, (surf, view, wi, Li, lit), n_em = prep
    scene = r.scene
    n = scene.height * scene.width
    be = autograd.bsdf_eval(r, surf, view, wi, rows)
    term = (be[:, 0:3] * be[:, 4:5]) * Li
    term = torch.where(lit[:, None], term, torch.zeros_like(term))
    val = base + term.reshape(spp, max(n_em, 1), n, 3).sum(1) if n_em else base
    film = autograd.film_splat_passes(r, pos, val.reshape(spp, scene.height, scene.width, 3), passes=spp)
    return autograd.develop(scene, film)


def fit(r, which, spp=2, steps=100, lr=0.05, seed=0, log=None):
    """Fits the chosen words; returns (losses, start rows, fitted rows, the scene's rows) as numpy."""
    scene = r.scene
    dev = torch.device("cuda", r.device)
    _, bsdf_type, words = SCENES[which]
    own = torch.from_numpy(nori_amd.scene_materials(scene)).to(dev)
    mask = torch.zeros_like(own, dtype=torch.bool)
    for b in range(scene.desc.num_bsdfs):
        if scene.desc.bsdfs[b].type == bsdf_type:
            mask[b, list(words)] = True
    mask &= own > 0  # start * exp(theta) cannot leave 0
    prep = prepare(r, spp, seed)
    if which == "veach":  # the built-in direct_ems render of the same passes
        target = torch.from_numpy(nori_amd.develop(scene, r.render(passes=spp, seed=seed))).to(dev)
    else:
        with torch.no_grad():
            target = image(r, own, prep, spp)
    g = torch.Generator(device="cpu").manual_seed(7)
    factor = torch.exp(torch.empty(own.shape).uniform_(0.4, 0.9, generator=g) *
                       torch.where(torch.rand(own.shape, generator=g) < 0.5, -1.0, 1.0)).to(dev)
    start = torch.where(mask, own * factor, own)
    if which == "disney":
        start = torch.where(mask, start.clamp(max=0.95), start)
    theta = torch.zeros_like(own, requires_grad=True)
    opt = torch.optim.Adam([theta], lr=lr)
    losses = []
    for step in range(steps):
        opt.zero_grad()
        rows = torch.where(mask, start * torch.exp(theta), own)
        loss = ((image(r, rows, prep, spp) - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
        if log and (step % log == 0 or step == steps - 1):
            print(f"step {step:4d}  loss {losses[-1]:.6e}")
    with torch.no_grad():
        fitted = torch.where(mask, start * torch.exp(theta), own)
    return losses, start.cpu().numpy(), fitted.cpu().numpy(), own.cpu().numpy()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scene", choices=sorted(SCENES), default="veach")
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--width", type=int, default=192)
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    scene = nori_amd.load_scene(os.path.join(ROOT, SCENES[a.scene][0]), a.width, a.height, a.spp)
    with nori_amd.GpuRenderer(scene, a.device) as r:
        losses, start, fitted, own = fit(r, a.scene, a.spp, a.steps, a.lr, log=max(1, a.steps // 10))
    np.set_printoptions(precision=4, suppress=True)
    words = list(SCENES[a.scene][2])
    for b in range(own.shape[0]):
        if scene.desc.bsdfs[b].type == SCENES[a.scene][1]:
            print(f"bsdf {b}: start {start[b, words]}  fitted {fitted[b, words]}  scene {own[b, words]}")
    print(f"loss {losses[0]:.4e} -> {losses[-1]:.4e}")


if __name__ == "__main__":
    main()
