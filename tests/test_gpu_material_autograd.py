"""torch.autograd over the materials: nori_amd.autograd.bsdf_eval (forward update_materials +
bsdf_eval, backward nori_gpu_bsdf_grad) and examples/fit_material_torch.py.

1. out.backward(g) gives what GpuRenderer.bsdf_grad gives for g, bit for bit (the table path is
   reproducible); 2. the backward raises after a later update_materials; 3. central differences
   through autograd.bsdf_eval in float32: per BSDF, a random direction d over its words in use,
   fd = (<g, out(rows + h d)> - <g, out(rows - h d)>) with the two sums taken in float64 from the
   float32 outputs, against <grad, (rows + h d) - (rows - h d)>, in D20's measure
   e = |fd - an| / sum |terms| |d| per element.  The forward is float32 here: each of the two
   outputs carries a relative rounding of a few 2^-24 of its own size, and the difference of the
   two is h |d| |terms| ~ 2^-7 of that size or, where the lobe's value is large against its
   derivative (the microfacet lobe's flank), far less; so e is 1e-6 .. 1e-5 in the bulk and
   reaches 1e-3 in the worst element.  Observed on an MI355X (this file's print), largest e of
   4000 elements: microfacet 4.33e-03, disney 1.72e-04, diffuse 5.5e-06, checkerboard 4.3e-06
   (medians 1.6e-06 .. 6.0e-06).  Cap FD_CAP = 5e-2: the largest times ten, rounded up to one
   digit; a wrong or missing term shows as O(1).  (tests/test_bsdf_grad.py takes the same
   differences of the float64 forward on the CPU, where the cap is 1000 times tighter.)
4. 20 steps of examples/fit_material_torch.py at 32 x 32, 2 spp lower its loss: observed veach
   4.602e-04 -> 1.792e-05 (0.039 of the first), disney 2.748e-06 -> 1.437e-07 (0.052); asserted
   below 0.25 of the first for both."""
import importlib.util
import os

import numpy as np
import pytest

import material_util as M
import nori_amd
from conftest import ROOT

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
FD_CAP = 5e-2


@pytest.fixture(scope="module")
def zoo(built, tmp_path_factory):
    s = nori_amd.load_scene(M.zoo_xml(str(tmp_path_factory.mktemp("mauto"))), 32, 32, 1)
    with nori_amd.GpuRenderer(s, 0) as r:
        yield s, r


def elements(scene, n, seed):
    g = np.random.default_rng(seed)
    shape = np.where(np.arange(n) % 7 == 6, -1, g.integers(scene.desc.num_shapes, size=n))
    nsv = M.random_frames(n, seed)
    wi, wo = M.world_dirs(nsv, M.directions(n, seed + 1, 0.1, 0.95)), M.world_dirs(nsv, M.directions(n, seed + 2, 0.1, 0.95))
    return M.records(n, shape, ns=nsv, uv=g.uniform(-2, 2, (n, 2)).astype(f32)), wi, wo, shape


def test_backward_is_bsdf_grad_and_refuses_stale_materials(zoo):
    import torch
    from nori_amd import autograd

    scene, r = zoo
    n = 2000
    rec, wi, wo, _ = elements(scene, n, 1)
    rows = torch.from_numpy(nori_amd.scene_materials(scene)).cuda().requires_grad_(True)
    g = torch.from_numpy(np.random.default_rng(2).standard_normal((n, 8)).astype(f32)).cuda()
    surf = torch.from_numpy(rec.view(f32).reshape(n, 16)).cuda()
    out = autograd.bsdf_eval(r, surf, wi, wo, rows)
    assert np.array_equal(out.detach().cpu().numpy().view(np.uint32), r.bsdf_eval(rec, wi, wo).view(np.uint32))
    out.backward(g)
    want = r.bsdf_grad(rec, wi, wo, g.cpu().numpy())
    assert want.any() and np.array_equal(rows.grad.cpu().numpy().view(np.uint32), want.view(np.uint32))
    out2 = autograd.bsdf_eval(r, surf, wi, wo, rows)
    r.update_materials(nori_amd.scene_materials(scene))
    with pytest.raises(RuntimeError, match="materials have changed"):
        out2.backward(g)


def test_central_differences_through_autograd(zoo):
    import torch
    from nori_amd import autograd

    scene, r = zoo
    n, h = 4000, 2.0 ** -7
    rec, wi, wo, shape = elements(scene, n, 3)
    surf = torch.from_numpy(rec.view(f32).reshape(n, 16)).cuda()
    own = nori_amd.scene_materials(scene)
    rng = np.random.default_rng(4)
    g = np.zeros((n, 8), f32)
    g[:, :4] = rng.standard_normal((n, 4))
    gt = torch.from_numpy(g).cuda()
    sb, kinds = M.shape_bsdfs(scene), M.kinds(scene)
    d = np.zeros_like(own)
    for b, kind in enumerate(kinds):
        d[b, M.WORDS[kind]] = rng.uniform(0.5, 1.0, len(M.WORDS[kind])) * own[b, M.WORDS[kind]]  # relative steps
    plus, minus = (own + f32(h) * d).astype(f32), (own - f32(h) * d).astype(f32)

    def forward(rows):
        with torch.no_grad():
            o = autograd.bsdf_eval(r, surf, wi, wo, torch.from_numpy(rows).cuda())
        return (o.cpu().numpy().astype(f64)[:, :4] * g[:, :4]).sum(1)

    fd = forward(plus) - forward(minus)
    r.update_materials(own)
    _, terms = r.bsdf_grad(rec, wi, wo, g, terms=True)
    step = (plus.astype(f64) - minus.astype(f64))
    hit = shape >= 0
    per = np.zeros((n, 16))
    per[hit] = step[sb[shape[hit]]]
    an = (terms.astype(f64) * per).sum(1)
    den = (np.abs(terms.astype(f64)) * np.abs(per)).sum(1)
    live = den > 0
    e = np.abs(fd - an)[live] / den[live]
    assert np.all(fd[~live] == 0)
    kind = np.array(["miss" if s < 0 else kinds[sb[s]] for s in shape])[live]
    for k in sorted(set(kind)):
        print(f"{k}: {int((kind == k).sum())} elements, largest e {e[kind == k].max():.3e}, median {np.median(e[kind == k]):.3e}")
    assert e.max() <= FD_CAP, e.max()
    # the whole call through autograd: rows.grad . step against the summed difference
    rows = torch.from_numpy(own).cuda().requires_grad_(True)
    autograd.bsdf_eval(r, surf, wi, wo, rows).backward(gt)
    whole = float((rows.grad.cpu().numpy().astype(f64) * step).sum())
    assert abs(whole - fd.sum()) <= FD_CAP * den.sum()


@pytest.mark.parametrize("which,bar", (("veach", 0.25), ("disney", 0.25)))
def test_fit_material_example_lowers_its_loss(built, which, bar):
    spec = importlib.util.spec_from_file_location("fit_material_torch", os.path.join(ROOT, "examples", "fit_material_torch.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    scene = nori_amd.load_scene(os.path.join(ROOT, ex.SCENES[which][0]), 32, 32, 2)
    with nori_amd.GpuRenderer(scene, 0) as r:
        losses, start, fitted, own = ex.fit(r, which, spp=2, steps=20)
    print(f"{which}: loss {losses[0]:.4e} -> {losses[-1]:.4e} ({losses[-1] / losses[0]:.3f} of the first), min {min(losses):.4e}")
    assert np.isfinite(losses).all() and losses[0] > 0
    assert losses[-1] < bar * losses[0]
    assert not np.array_equal(start, fitted) and np.isfinite(fitted).all()
