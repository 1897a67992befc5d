"""The film as a differentiable torch operation.

    from nori_amd import autograd
    film = autograd.film_splat_passes(r, pos, val)      # val.requires_grad: the film carries a graph
    img = autograd.develop(r.scene, film)                # ImageBlock::toBitmap in torch
    ((img - target) ** 2).sum().backward()               # val.grad through the scene's own filter

The forward is GpuRenderer.film_splat / film_splat_passes into a new film; the splat is linear in
`val`, and the backward is its adjoint, GpuRenderer.film_gather / film_gather_passes: every sample
reads the incoming gradient over the window it was splatted into, with the same weights
(nori_film_gather in nori_gpu.h).  `pos` never receives a gradient: the tabulated filter is
piecewise constant in the position.  The library runs on its own stream and its calls block, so
each call is preceded by a synchronisation of torch's current stream on the context's device.

`surface` makes the hit record differentiable in the mesh vertices:

    rec, hits = autograd.surface(r, rays, positions)     # positions.requires_grad: rec carries a graph
    hit = hits[:, 1].view(torch.int32) >= 0
    ((rec[hit, 3] - target_t[hit]) ** 2).sum().backward()   # positions.grad, through nori_gpu_surface_grad

`bsdf_eval` makes the shading query differentiable in the material rows:

    out = autograd.bsdf_eval(r, surf, wi, wo, materials)  # materials.requires_grad: out carries a graph
    (out[:, 0:3] * weight).sum().backward()                 # materials.grad, through nori_gpu_bsdf_grad

This module alone imports torch; `import nori_amd` works without it."""
import torch
from torch.autograd.function import once_differentiable

__all__ = ["film_splat", "film_splat_passes", "develop", "surface", "bsdf_eval"]


def _device(r):
    return torch.device("cuda", r.device)


def _input(r, a):
    """`a` as a contiguous float32 tensor on the context's device (a tracked conversion)."""
    return torch.as_tensor(a).to(device=_device(r), dtype=torch.float32).contiguous()


def _ready(r):
    torch.cuda.current_stream(_device(r)).synchronize()


class _FilmSplat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, r, pos, val):
        film = torch.zeros(r.scene.film_shape(), dtype=torch.float32, device=_device(r))
        _ready(r)
        r.film_splat(pos, val, n=val.numel() // 3, out=film)
        ctx.r = r
        ctx.save_for_backward(pos, val)
        return film

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        pos, val = ctx.saved_tensors
        grad = grad.contiguous()
        grad_val = torch.zeros_like(val)
        _ready(ctx.r)
        ctx.r.film_gather(pos, grad, val, n=val.numel() // 3, out=grad_val)
        return None, None, grad_val


class _FilmSplatPasses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, r, pos, val, passes, blocks):
        film = torch.zeros(r.scene.film_shape(), dtype=torch.float32, device=_device(r))
        _ready(r)
        r.film_splat_passes(pos, val, passes=passes, blocks=blocks, out=film)
        ctx.r, ctx.passes, ctx.blocks = r, passes, blocks
        ctx.save_for_backward(pos, val)
        return film

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        pos, val = ctx.saved_tensors
        grad = grad.contiguous()
        grad_val = torch.zeros_like(val)  # zero: the rows of unselected blocks are not written
        _ready(ctx.r)
        ctx.r.film_gather_passes(pos, grad, val, passes=ctx.passes, blocks=ctx.blocks, out=grad_val)
        return None, None, grad_val, None, None


class _Surface(torch.autograd.Function):
    @staticmethod
    def forward(ctx, r, rays, positions, normals):
        n = rays.numel() // 8
        dev = _device(r)
        _ready(r)
        r.update_vertices(positions, normals)
        hits = torch.empty((n, 4), dtype=torch.float32, device=dev)
        rec = torch.empty((n, 16), dtype=torch.float32, device=dev)
        _ready(r)
        if n:
            r.query(rays.data_ptr(), n=n, hits_out=hits.data_ptr(), surf_out=rec.data_ptr())
        ctx.r, ctx.version, ctx.with_normals = r, r.geometry_version, normals is not None
        ctx.save_for_backward(rays, hits)
        ctx.mark_non_differentiable(hits)
        return rec, hits

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_rec, _grad_hits):
        r = ctx.r
        if r.geometry_version != ctx.version:
            raise RuntimeError("autograd.surface: the context's geometry has changed since this forward "
                               "(update_vertices / rebuild_bvh); the backward reads the context's current "
                               "vertices and would return the gradient at another geometry")
        rays, hits = ctx.saved_tensors
        V = r.scene.desc.num_vertices
        grad_rec = grad_rec.contiguous()
        gp = torch.zeros((V, 3), dtype=torch.float32, device=grad_rec.device)
        gn = torch.zeros_like(gp) if ctx.with_normals and ctx.needs_input_grad[3] else None
        _ready(r)
        if rays.numel():
            r.surface_grad(rays, hits, grad_rec, gp, gn, n=rays.numel() // 8)
        return None, None, gp, gn


def surface(r, rays, positions, normals=None):
    """The hit records of `rays` on the mesh at `positions`, differentiable in the vertices.

    rays (n, 8), positions and normals (num_vertices, 3; normals=None: the vertex normals stay).
    Forward: r.update_vertices(positions, normals), then r.query(rays) into new tensors.  Returns
    (rec, hits): the (n, 16) float32 records in nori_gpu_surface's layout -- p 0:3, t 3, ng 4:7,
    ns 8:11, uv 12:14, bary 14:16; columns 7 and 11 hold the int32 prim and shape as bits -- and the
    (n, 4) hits (t, prim as bits, u, v; no gradient).  rec carries a graph when positions or
    normals requires grad; its backward is r.surface_grad (nori_gpu_surface_grad).

    The context's geometry moves to `positions` as a side effect: that is the design, every later
    call of `r` sees it.  The backward reads the context's vertices, so it raises if
    update_vertices or rebuild_bvh ran on `r` after this forward.  The context must be able to
    move its vertices (NORI_TRAVERSAL=bvh for small scenes): update_vertices' NoriError passes
    through.

    What is differentiated: p and ns at fixed barycentrics, t as the distance at which the fixed
    ray meets the moving triangle's plane, ng; the hit set is held (no silhouette terms), uv and
    bary have no gradient, a normal-mapped shape's ns none, spheres none.  For the point where the
    fixed ray meets the moving surface use rays[:, 0:3] + rec[:, 3:4] * rays[:, 4:7] instead of
    rec[:, 0:3] (equivalently: fold d . g_p into g_t and pass g_p = 0).  A miss has t = +inf: mask
    it out of the loss."""
    rays = _input(r, rays).detach().reshape(-1, 8)
    positions = _input(r, positions)
    if normals is not None:
        normals = _input(r, normals)
    return _Surface.apply(r, rays, positions, normals)


class _BsdfEval(torch.autograd.Function):
    @staticmethod
    def forward(ctx, r, surf, wi, wo, materials):
        n = wi.numel() // 3
        _ready(r)
        r.update_materials(materials)
        out = torch.empty((n, 8), dtype=torch.float32, device=_device(r))
        if n:
            r.bsdf_eval(surf, wi, wo, n=n, out=out)
        ctx.r, ctx.version = r, r.materials_version
        ctx.save_for_backward(surf, wi, wo)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        r = ctx.r
        if r.materials_version != ctx.version:
            raise RuntimeError("autograd.bsdf_eval: the context's materials have changed since this forward "
                               "(update_materials); the backward reads the context's current materials and "
                               "would return the gradient at other values")
        surf, wi, wo = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        gm = torch.zeros((r.scene.desc.num_bsdfs, 16), dtype=torch.float32, device=grad_out.device)
        _ready(r)
        if wi.numel():
            r.bsdf_grad(surf, wi, wo, grad_out, grad_materials=gm, n=wi.numel() // 3)
        return None, None, None, None, gm


def bsdf_eval(r, surf, wi, wo, materials):
    """GpuRenderer.bsdf_eval at the material rows `materials`, differentiable in them.

    surf (n, 16) float32 records (query()'s, as a tensor), wi and wo (n, 3), materials (num_bsdfs,
    16) in scene_materials' layout.  Forward: r.update_materials(materials), then r.bsdf_eval into
    a new (n, 8) tensor (eval rgb, pdf, wo_local.z, wi_local.z, 0, 0).  Backward: r.bsdf_grad
    (nori_gpu_bsdf_grad) into a zero (num_bsdfs, 16) tensor; words a BSDF's type does not use,
    and the reserved ones, receive 0.

    The context's materials move to `materials` as a side effect: that is the design, every later
    render and query of `r` sees them.  The backward reads the context's materials, so it raises
    if update_materials ran on `r` after this forward.  There is no gradient in surf, wi or wo (they
    are detached), none in the IORs, textures' layout or image texels; the cosines in columns 4-5
    do not depend on the materials."""
    surf = _input(r, surf).detach().reshape(-1, 16)
    wi = _input(r, wi).detach().reshape(-1, 3)
    wo = _input(r, wo).detach().reshape(-1, 3)
    return _BsdfEval.apply(r, surf, wi, wo, _input(r, materials))


def film_splat(r, pos, val):
    """GpuRenderer.film_splat(pos, val) into a new film tensor (H+2b, W+2b, 4), differentiable in
    val: pos (n, 2), val (n, 3)."""
    return _FilmSplat.apply(r, _input(r, pos).detach(), _input(r, val))


def film_splat_passes(r, pos, val, passes=None, blocks=None):
    """GpuRenderer.film_splat_passes(pos, val, passes, blocks) into a new film tensor,
    differentiable in val: pos (passes, H, W, 2), val (passes, H, W, 3); passes=None is the
    scene's sampleCount.  The samples of unselected blocks get a zero gradient."""
    pos, val = _input(r, pos).detach(), _input(r, val)
    W, H = r.scene.width, r.scene.height
    if passes is None:
        passes = int(r.scene.spp)
    if val.numel() != 3 * passes * H * W or pos.numel() != 2 * passes * H * W:
        raise ValueError(f"film_splat_passes: pos {tuple(pos.shape)} and val {tuple(val.shape)}, expected "
                         f"{(passes, H, W, 2)} and {(passes, H, W, 3)}")
    return _FilmSplatPasses.apply(r, pos, val, passes, None if blocks is None else [int(b) for b in blocks])


def develop(scene, film):
    """ImageBlock::toBitmap (nori_amd.develop) in differentiable torch operations: the border
    cropped, rgb / w where w != 0, else 0 -- (H, W, 3).  The denominator of a w == 0 cell is
    replaced by 1 before the division, so no NaN gradient appears; the quotient of the two floats
    is taken in float64 and rounded to float32, which is the correctly rounded float32 quotient
    (53 >= 2 * 24 + 2 bits): the values equal nori_amd.develop's bit for bit, whatever torch's
    float32 division does."""
    if tuple(film.shape) != tuple(scene.film_shape()):
        raise ValueError(f"film shape {tuple(film.shape)} != {scene.film_shape()}")
    b, H, W = scene.border, scene.height, scene.width
    crop = film[b:H + b, b:W + b]
    rgb, w = crop[..., 0:3], crop[..., 3:4]
    nz = w != 0
    safe = torch.where(nz, w, torch.ones_like(w))
    q = (rgb.double() / safe.double()).float()
    return torch.where(nz, q, torch.zeros_like(q))
