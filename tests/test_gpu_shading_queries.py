"""The shading queries on the GPU: nori_gpu_bsdf_eval / _bsdf_sample / _emitter_sample /
_emitter_eval / _sample_uniforms (csrc/kernels_shading.hip), stated in include/nori_gpu.h.

1. BSDFs at real hit records against the CPU oracle, compared as tests/test_gpu_device_units.py
   compares the device-unit shim;
2. the image-texture albedo against the feature pass (an independent kernel);
3. the direct_* integrators composed in numpy from the queries (tests/shading_compose.py) against
   the built-in ones, sample for sample;
4. device buffers (torch) against host arrays; 5. sample_uniforms; 6. dynamic geometry;
7. refusals; 8. examples/direct_torch.py.

Equality is of 32-bit patterns, NaN against NaN counting as equal."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import bsdf_ref64 as R
import device_unit_inputs as I
import nori_amd
import pyoracle
import refit_util
import shading_compose
import synth
from conftest import ROOT, scene_path
from nori_amd import _abi
from test_gpu_device_units import DIR_TOL, EXPF_TOL, _nonfinite_pattern_equal, _only_underflow, assert_same_bits, same_bits
from test_gpu_query import COUNTS, THINLENS, _bits, _chunked, _renderer
from test_query import CBOX, NMAP, scene_rays

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
VEACH = ("pa3", "veach_mi", "veach_mis.xml")
TEXTURED = ("project", "textured", "cbox_path_mis.xml")
SCAN_MAX_PRIMS = 64  # scene_prep.h kScanMaxPrims: contexts of larger scenes traverse the BVH


def local32(ns, v):
    """to_local(frame_from(ns), v) in float32: ((n, 9) frame rows s, t, n; (n, 3) local v)."""
    F = R.frame32(np.ascontiguousarray(ns, f32))
    v = np.ascontiguousarray(v, f32)
    return F, np.stack([R.dot32(v, F[:, 0:3]), R.dot32(v, F[:, 3:6]), R.dot32(v, F[:, 6:9])], 1).astype(f32)


def world32(F, v):
    """to_world(frame, v) = (s v.x + t v.y) + n v.z in float32."""
    with np.errstate(all="ignore"):
        return ((F[:, 0:3] * v[:, 0:1] + F[:, 3:6] * v[:, 1:2]) + F[:, 6:9] * v[:, 2:3]).astype(f32)


_E_VAL_MEASURED = {}


def e_val_for(desc):
    """E_val of a scene's BSDF: the largest relative difference of eval, pdf and weight luminance
    between the oracle and the float64 model on the well-conditioned subset.  Diffuse is the table's
    entry (device_unit_inputs.E_VAL).  The table has no entry for a scene's microfacet plates
    (veach_mis: alpha 0.005, 0.02, 0.05, 0.1), so theirs is measured here, on the CPU and from the
    reference alone, by the procedure that produced the table -- test_values_match_the_model of
    tests/test_bsdf_ref64.py on device_unit_inputs' input sets for that descriptor (0.4 s each):
    1.1e-2, 6.9e-4, 1.2e-4 and 2.8e-5 for the four plates (the table's alpha = 0.1 entry is 2.87e-5)."""
    if desc.type == _abi.BSDF_DIFFUSE:
        return I.E_VAL["diffuse"]
    assert desc.type == _abi.BSDF_MICROFACET
    key = bytes(desc)
    if key not in _E_VAL_MEASURED:
        wi_s, u, uv_s = I.sample_inputs(desc)
        o = pyoracle.bsdf_sample_uv(desc, wi_s, u, uv_s)
        wi, wo, uv = I.eval_inputs(desc, o[:, :3])
        ep = pyoracle.bsdf_eval_pdf_uv(desc, wi, wo, uv)
        ev64, pdf64 = R.eval_pdf64(desc, wi, wo, uv)
        well = I.well_conditioned(wi, wo)
        ws = I.well_conditioned(wi_s, o[:, :3]) & (o[:, 6] != 0)
        assert well.sum() > 1000 and ws.sum() > 1000
        e = max(float(I.rel_diff(ep[well, :3], ev64[well]).max()), float(I.rel_diff(ep[well, 3], pdf64[well]).max()),
                float(I.rel_diff(o[ws, 6], R.weight_lum64(desc, wi_s[ws], o[ws, :3], uv_s[ws])).max()))
        assert np.isfinite(e) and e < 0.05, e  # (a bound near 1 could not fail)
        _E_VAL_MEASURED[key] = e
    return _E_VAL_MEASURED[key]


# nori_gpu_bsdf_sample returns the sampled direction in the world only, so the local direction at
# which the oracle is asked for its pdf and weight is to_local(to_world(wo)), not the device's wo.
# to_world rounds each component 5 times (3 products, 2 sums of values <= 1: at most 6 * 2^-24), to_local
# carries that over with |s_i| + |t_i| + |n_i| <= sqrt(3) and rounds 5 times itself: 16 * 2^-24 per component.
# Observed on the MI355X: the microfacet plates stay inside 4 E_val alone (pdf 9.5e-3 / 6.0e-4 / 9.7e-5 /
# 2.4e-5 against 4.6e-2 / 2.8e-3 / 4.6e-4 / 1.1e-4, weight luminance at most 4.2e-6); the cosine lobe's pdf,
# kInvPi * wo.z, reaches 6.0e-7 against 4 E_val = 4.0e-7 on a few rows near the horizon, where the trip
# explains up to 1.7e-5.
TRIP = 16 * 2.0 ** -24


def lum32(c):
    return ((c[:, 0] * f32(0.212671) + c[:, 1] * f32(0.715160)) + c[:, 2] * f32(0.072169)).astype(f32)


def oracle_pdf_and_weight(desc, wi_l, wo_l, uv):
    """(pdf, weight luminance) of the oracle at the pair: the weight formed as Microfacet::sample forms it."""
    wo_l = np.ascontiguousarray(wo_l, f32)
    ep = pyoracle.bsdf_eval_pdf_uv(desc, wi_l, wo_l, uv)
    with np.errstate(all="ignore"):
        w = ((ep[:, :3] * wo_l[:, 2:3]) / ep[:, 3:4]).astype(f32)
    return ep[:, 3], lum32(w)


def trip_allowance(desc, wi_l, wo_l, uv):
    """Per row: how far the oracle's own pdf and weight luminance move (relative) when the direction moves
    by TRIP along an axis -- the part of a difference that the world-and-back trip can explain."""
    base = oracle_pdf_and_weight(desc, wi_l, wo_l, uv)
    out = [np.zeros(len(wo_l)), np.zeros(len(wo_l))]
    for k in range(3):
        for sgn in (-1, 1):
            moved = np.array(wo_l, f32)
            moved[:, k] += f32(sgn * TRIP)
            for j, q in enumerate(oracle_pdf_and_weight(desc, wi_l, moved, uv)):
                out[j] = np.maximum(out[j], np.nan_to_num(I.rel_diff(q, base[j]), nan=np.inf))
    return base, out


def untextured(desc):
    """A copy of an image-textured diffuse desc with the constant albedo 1: the oracle's
    descriptor-only entry points have no image table (test 2 checks the texel)."""
    d = _abi.BsdfDesc.from_buffer_copy(desc)
    d.albedo_texture, d.albedo_image = _abi.TEXTURE_CONSTANT, -1
    d.albedo[:] = [1, 1, 1]
    return d


# ---------------------------------------------------------------- 1. BSDFs against the oracle
@pytest.fixture(scope="module", params=["cbox", "nmap", "veach"])
def records(request, built):
    """Real records of a scene at 32 x 32 with the directions and samples of tests 1 and 4 and the
    host reference (the frames and local directions in float32): computed once, read-only."""
    which = request.param
    scene = nori_amd.load_scene(scene_path(*{"cbox": CBOX, "nmap": NMAP, "veach": VEACH}[which]), 32, 32, 1)
    with nori_amd.GpuRenderer(scene, 0) as r:
        rays = r.camera_rays(passes=1).reshape(-1, 8)[:1000] if which == "veach" else scene_rays(which, scene, 1000)
        rays = np.ascontiguousarray(rays)
        surf = r.query(rays)["surf"]
    n = surf.shape[0]
    rng = np.random.default_rng(31)
    wi = np.ascontiguousarray(-rays[:, 4:7])
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    # seven in eight on wi's side of the shading normal, where the lobes are
    side = np.sign((v * surf["ns"]).sum(1) * (wi * surf["ns"]).sum(1))
    flip = (side < 0) & (np.arange(n) % 8 != 0)
    wo = np.where(flip[:, None], -v, v).astype(f32)
    u = rng.random((n, 2), dtype=f32)
    F, wi_l = local32(surf["ns"], wi)
    _, wo_l = local32(surf["ns"], wo)
    out = dict(which=which, scene=scene, surf=surf, wi=wi, wo=wo, u=u, F=F, wi_l=wi_l, wo_l=wo_l)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def test_bsdfs_at_hit_records_against_oracle(records):
    o = records
    scene, surf, n = o["scene"], o["surf"], o["surf"].shape[0]
    shapes, bsdfs = scene.shapes(), scene.bsdfs()
    hit = surf["shape"] >= 0
    bsdf_of = np.array([sh.bsdf for sh in shapes] + [-1])[surf["shape"]]
    types = {b.type for b in (bsdfs[sh.bsdf] for sh in shapes)}
    # the input: at least half the records are hits, every BSDF type of the scene by at least 1 %
    assert hit.mean() >= 0.5, hit.mean()
    type_of = np.array([b.type for b in bsdfs] + [-1])[bsdf_of]
    for t in types:
        assert (type_of == t).mean() >= 0.01, (t, (type_of == t).mean())
    with nori_amd.GpuRenderer(scene, 0) as r:
        ev, sm = {}, {}
        for m in COUNTS:
            with _chunked(m):
                ev[m] = r.bsdf_eval(surf[:m], o["wi"][:m], o["wo"][:m])
                sm[m] = r.bsdf_sample(surf[:m], o["wi"][:m], o["u"][:m])
    for m in COUNTS:  # every count is the prefix of the largest
        assert_same_bits(ev[m], ev[1000][:m], f"bsdf_eval n = {m}")
        assert_same_bits(sm[m], sm[1000][:m], f"bsdf_sample n = {m}")
    ev, sm = ev[1000], sm[1000]
    assert not ev[~hit].view(u32).any() and not sm[~hit].view(u32).any(), "a miss record gives zeros"
    # the cosines are the host's to_local, bit for bit
    assert_same_bits(ev[hit, 4], o["wo_l"][hit, 2], "wo_local.z")
    assert_same_bits(ev[hit, 5], o["wi_l"][hit, 2], "wi_local.z")
    assert not ev[:, 6:8].any()
    for b in sorted(set(bsdf_of[hit])):
        d, rows = bsdfs[b], np.flatnonzero(bsdf_of == b)
        textured = d.type == _abi.BSDF_DIFFUSE and d.albedo_texture == _abi.TEXTURE_IMAGE
        od = untextured(d) if textured else d
        wi_l, wo_l, uv = (np.ascontiguousarray(a[rows]) for a in (o["wi_l"], o["wo_l"], surf["uv"]))
        name = f"{o['which']} bsdf {b} (type {d.type})"
        # ---- eval / pdf
        ref, got = pyoracle.bsdf_eval_pdf_uv(od, wi_l, wo_l, uv), ev[rows, 0:4]
        if textured:  # the albedo factor is test 2's: the pdf and the zero pattern here
            assert_same_bits(got[:, 3], ref[:, 3], f"{name}: pdf")
            assert np.array_equal((got[:, 0:3] == 0).all(1), (ref[:, 0:3] == 0).all(1)), name
        elif I.exact_eval(d):
            assert_same_bits(got, ref, f"{name}: eval / pdf")
        else:
            _nonfinite_pattern_equal(got, ref, name)
            num = np.isfinite(ref).all(1)
            assert np.array_equal(got[num] < 0, ref[num] < 0)
            assert np.array_equal(got[num] == 0, ref[num] == 0) or _only_underflow(got[num], ref[num]), "zero pattern"
            well = I.well_conditioned(wi_l, wo_l) & num
            e = float(I.rel_diff(got[well], ref[well]).max()) if well.any() else 0.0
            print(f"{name}: eval / pdf error {e:.3e} over {int(well.sum())} pairs")
            assert e <= 4 * e_val_for(d) and e <= EXPF_TOL
        # ---- sample
        u = np.ascontiguousarray(o["u"][rows])
        ref, got = pyoracle.bsdf_sample_uv(od, wi_l, u, uv), sm[rows]
        Fr = o["F"][rows]
        zero_ref, zero_got = (ref[:, 3:6] == 0).all(1), (got[:, 4:7] == 0).all(1)
        assert not got[zero_got].view(u32).any(), f"{name}: a zero weight gives a zero row"
        ref_dir = np.where(zero_ref[:, None], f32(0), world32(Fr, ref[:, 0:3])).astype(f32)
        live = ~zero_ref & ~zero_got
        assert np.array_equal(got[live, 7], ref[live, 7]), f"{name}: measure"
        assert not (got[:, 4:7] < 0).any(), "negative weight"
        if I.exact(d):
            assert np.array_equal(zero_ref, zero_got)
            assert_same_bits(got[:, 0:3], ref_dir, f"{name}: direction")
            assert_same_bits(got[live, 4:7], ref[live, 3:6], f"{name}: weight")
            assert not got[:, 3].any(), f"{name}: the pdf of a discrete lobe is 0"
            continue
        # the zero / non-zero pattern of the weight, except next to the horizon
        differs, horizon = zero_ref != zero_got, np.abs(ref[:, 2]) < 1e-5
        assert not (differs & ~horizon).any(), f"{name}: a weight is zero where the oracle's is not"
        assert (differs & horizon).sum() <= max(1, 1e-3 * rows.size)
        if d.type == _abi.BSDF_DIFFUSE and not textured:
            assert_same_bits(got[live, 4:7], ref[live, 3:6], f"{name}: weight (the albedo)")
        e_dir = float(np.abs(got[live, 0:3] - ref_dir[live]).max()) if live.any() else 0.0
        # the device's pdf and weight against the oracle's at the device's own direction, as
        # test_bsdf_sample_against_oracle of tests/test_gpu_device_units.py: 4 E_val on the
        # well-conditioned subset, plus what the trip to the world and back can explain (TRIP)
        if not live.any():  # (e.g. a light's few hits, all seen from behind)
            continue
        _, wo_dev = local32(surf["ns"][rows], got[:, 0:3])
        assert np.abs(wo_dev[live] - ref[live, 0:3]).max() <= DIR_TOL + TRIP, f"{name}: the local direction"
        (pdf_ref, w_ref), (allow_pdf, allow_w) = trip_allowance(od, wi_l, wo_dev, uv)
        well = I.well_conditioned(wi_l, wo_dev) & live
        assert well.any(), name
        e_val = e_val_for(d)
        d_pdf = I.rel_diff(got[well, 3], pdf_ref[well])
        # (an image texture's weight is its texel, test 2's subject: the oracle here has albedo 1)
        d_w = np.zeros(int(well.sum())) if textured else I.rel_diff(lum32(got[:, 4:7])[well], w_ref[well])
        print(f"{name}: {rows.size} samples, {int(well.sum())} well conditioned, direction error {e_dir:.3e} (bound "
              f"{DIR_TOL:.3e}); pdf error {float(d_pdf.max()):.3e}, weight luminance error {float(d_w.max()):.3e} "
              f"(4 E_val = {4 * e_val:.3e}; the trip allows up to {float(allow_pdf[well].max()):.3e} / "
              f"{float(allow_w[well].max()):.3e} more on its rows)")
        assert e_dir <= DIR_TOL
        assert (d_pdf <= 4 * e_val + allow_pdf[well]).all(), f"{name}: pdf"
        assert (d_w <= 4 * e_val + allow_w[well]).all(), f"{name}: weight"


# ---------------------------------------------------------------- 2. image-texture albedo against the feature pass
def test_image_texture_albedo_equals_feature_pass(built):
    """f * pi of a diffuse hit at wi = wo = ns against the albedo of features(passes=1).

    f = fl(albedo * kInvPi), and fl(f * pi32) is not albedo exactly: the two roundings are 2^-24
    each relative, and pi32 * kInvPi differs from 1 by the two constants' own roundings, 2^-24
    each: |f pi - albedo| <= 4 * 2^-24 * albedo = 2.4e-7 albedo.  Observed on the MI355X: 586 diffuse
    hits, the largest |f pi - albedo| / albedo is 8.4e-8, and every channel rounds to the same byte."""
    s = nori_amd.load_scene(scene_path(*TEXTURED), 32, 32, 1)
    assert any(b.albedo_texture == _abi.TEXTURE_IMAGE for b in s.bsdfs())
    with nori_amd.GpuRenderer(s, 0) as r:
        feat = r.features(passes=1).reshape(-1, 8)
        rays = r.camera_rays(passes=1).reshape(-1, 8)
        surf = r.query(rays)["surf"]
        ns = np.ascontiguousarray(surf["ns"])
        ev = r.bsdf_eval(surf, ns, ns)
    bsdf = np.array([s.bsdfs()[sh.bsdf].type for sh in s.shapes()] + [-1])[surf["shape"]]
    tex = np.array([s.bsdfs()[sh.bsdf].albedo_texture for sh in s.shapes()] + [-1])[surf["shape"]]
    diffuse = bsdf == _abi.BSDF_DIFFUSE
    assert (diffuse & (tex == _abi.TEXTURE_IMAGE)).mean() >= 0.05, "too few image-textured hits"
    fpi = (ev[diffuse, 0:3] * f32(np.pi)).astype(f32)
    alb = feat[diffuse, 0:3]
    err = np.abs(fpi.astype(np.float64) - alb)
    print(f"albedo: {int(diffuse.sum())} diffuse hits, max |f pi - albedo| / albedo = "
          f"{float((err / np.maximum(alb, 1e-30)).max()):.3e}")
    assert (err <= 4 * 2.0 ** -24 * alb).all()
    # ... and the texel bytes are the same
    assert np.array_equal(np.rint(fpi * 255), np.rint(alb * 255))


# ---------------------------------------------------------------- 3. the composed integrator is the built-in one
DIRECT = shading_compose.DIRECT_SCENES  # (tests/test_shading_compose_inputs.py: no invalid sample on the CPU)


def _modes(scene):
    prims = sum(1 if sh.type == _abi.SHAPE_SPHERE else sh.tri_count for sh in scene.shapes())
    return ["scan", "bvh"] if prims <= SCAN_MAX_PRIMS else ["bvh"]


def _composed_equals_builtin(scene, label):
    """Bit equality of L per sample: the statistics of a 1-pass render hold 0 + L in channels 0-2
    and the count in channel 6; a sample the renderer dropped as invalid (count 0) is left out.
    Observed maximum difference on the MI355X: 0 on each of the 1024 samples of every scene, mode
    and pass, none left out (every operation on the host is one IEEE float32 operation that the
    device performs too; no operation had to be bounded)."""
    H, W = scene.height, scene.width
    for mode in _modes(scene):
        with _renderer(scene, mode) as r:
            for k in shading_compose.PASSES:
                var = np.zeros((H, W, 8), f32)
                r.render(passes=1, pass_begin=k, variance=var)
                L, hit = shading_compose.direct_li(r, scene, scene.integrator, k)
                count = var[..., 6]
                assert np.isin(count, (0, 1)).all()
                keep = count == 1  # no pixel with count 1 is left out
                assert (~keep).mean() <= 0.01, f"{label} {mode} pass {k}: {(~keep).sum()} invalid samples"
                want = var[..., 0:3][keep]
                got = (L[keep] + f32(0)).astype(f32)  # the statistics are 0 + L
                bad = ~same_bits(got, want).all(1)
                diff = float(np.nanmax(np.abs(got.astype(np.float64) - want))) if keep.any() else 0.0
                print(f"{label} {mode} pass {k}: {int(keep.sum())} samples, {int(hit.sum())} hits, "
                      f"mean L {float(want.mean()):.4f}, max |difference| {diff:.3e}")
                assert hit.mean() > 0.1 and want.max() > 0
                assert not bad.any(), (f"{label} {mode} pass {k}: {int(bad.sum())} samples differ, first "
                                       f"{got[bad][0]!r} against {want[bad][0]!r}")


@pytest.mark.parametrize("parts", DIRECT, ids=[p[-1][:-4] for p in DIRECT])
def test_composed_direct_integrator_equals_builtin(built, parts):
    scene = nori_amd.load_scene(scene_path(*parts), 32, 32, 1)
    assert scene.integrator in ("direct_ems", "direct_mats", "direct_mis")
    _composed_equals_builtin(scene, parts[-1])


def test_composed_direct_mis_with_an_environment_map(built, tmp_path):
    """The envmap scene of tests/test_gpu_parity.py with direct_mis: Disney and diffuse surfaces
    under an environment-mapped sky sphere (the one-bounce kernel renders environment maps).  Also:
    emitter_sample's pdf_em is emitter_eval's pdf at the sky sphere along the sampled direction."""
    scene = nori_amd.load_scene(shading_compose.envmap_direct_mis(str(tmp_path)))
    assert any(e.type == _abi.EMITTER_ENVMAP for e in scene.emitters())
    _composed_equals_builtin(scene, "envmap direct_mis")
    env = [i for i, e in enumerate(scene.emitters()) if e.type == _abi.EMITTER_ENVMAP][0]
    sky = scene.emitters()[env].shape
    n = 1000
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, (n, 3)).astype(f32)
    u = rng.random((n, 2), dtype=f32)
    with nori_amd.GpuRenderer(scene, 0) as r:
        es = r.emitter_sample(x, u, emitter=env)
        # the sky sphere's hit along the sampled wi, seen from the origin: p - from = wi exactly
        rec = np.zeros(n, nori_amd.SURFACE_DTYPE)
        rec["p"], rec["ns"], rec["shape"], rec["t"] = es[:, 0:3], -es[:, 0:3], sky, 1
        ee = r.emitter_eval(rec, np.zeros((n, 3), f32))
    # emitter_eval normalises p - from once more; where that leaves the sampled direction as it is
    # (normalize is float32 numpy's, tests/test_gpu_device_units.py) both sides look up one direction
    with np.errstate(all="ignore"):
        same_dir = same_bits(R.normalize32(np.ascontiguousarray(es[:, 0:3])), es[:, 0:3]).all(1)
    print(f"envmap: {int(same_dir.sum())} of {n} sampled directions are fixed points of normalize")
    assert same_dir.sum() >= 16 and (es[same_dir, 7] > 0).any()
    assert_same_bits(ee[same_dir, 3], es[same_dir, 7], "emitter_eval pdf against emitter_sample pdf_em")


# ---------------------------------------------------------------- 4. device buffers
def test_device_buffers_equal_host_arrays(records):
    torch = pytest.importorskip("torch")
    o = records
    scene, surf = o["scene"], o["surf"]
    n_em = len(scene.emitters())
    ids = (np.arange(1000) % n_em).astype(np.int32)
    x = np.ascontiguousarray(surf["p"])

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(f32 if a.dtype != np.int32 else np.int32).copy()).to("cuda:0")

    with nori_amd.GpuRenderer(scene, 0) as r:
        for n in (1000, 129):
            s_h = surf[:n]
            s_d = dev(s_h.view(f32).reshape(n, 16))
            host = [r.bsdf_eval(s_h, o["wi"][:n], o["wo"][:n]), r.bsdf_sample(s_h, o["wi"][:n], o["u"][:n]),
                    r.emitter_sample(x[:n], o["u"][:n], ids=ids[:n]), r.emitter_sample(x[:n], o["u"][:n], emitter=n_em - 1),
                    r.emitter_eval(s_h, o["wi"][:n])]
            outs = [torch.full((n, c), 7.0, dtype=torch.float32, device="cuda:0") for c in (8, 8, 12, 12, 4)]
            wi_d, wo_d, u_d, x_d, ids_d = dev(o["wi"][:n]), dev(o["wo"][:n]), dev(o["u"][:n]), dev(x[:n]), dev(ids[:n])
            torch.cuda.synchronize()
            assert r.bsdf_eval(s_d, wi_d, wo_d, n=n, out=outs[0]) is None
            r.bsdf_sample(s_d.data_ptr(), wi_d.data_ptr(), u_d.data_ptr(), n=n, out=outs[1].data_ptr())
            r.emitter_sample(x_d, u_d, ids=ids_d, n=n, out=outs[2])
            r.emitter_sample(x_d, u_d, emitter=n_em - 1, n=n, out=outs[3])
            r.emitter_eval(s_d, wi_d, n=n, out=outs[4])
            for k, (h, d) in enumerate(zip(host, outs)):
                assert_same_bits(d.cpu().numpy(), h, f"call {k}, n = {n}")
        # both record reads give the same bits
        os.environ["NORI_SHADING_LOAD"] = "lds"
        try:
            lds = [r.bsdf_eval(surf[:m], o["wi"][:m], o["wo"][:m]) for m in COUNTS]
            lds_s = r.bsdf_sample(surf, o["wi"], o["u"])
            lds_e = r.emitter_eval(surf, o["wi"])
        finally:
            os.environ["NORI_SHADING_LOAD"] = "direct"
        try:
            direct = [r.bsdf_eval(surf[:m], o["wi"][:m], o["wo"][:m]) for m in COUNTS]
            direct_s = r.bsdf_sample(surf, o["wi"], o["u"])
            direct_e = r.emitter_eval(surf, o["wi"])
        finally:
            os.environ.pop("NORI_SHADING_LOAD")
        for a, b, m in zip(lds, direct, COUNTS):
            assert_same_bits(a, b, f"record read through LDS against per lane, n = {m}")
        assert_same_bits(lds_s, direct_s, "bsdf_sample, LDS against per lane")
        assert_same_bits(lds_e, direct_e, "emitter_eval, LDS against per lane")


def test_chain_on_the_device_without_a_host_copy(built):
    """camera_rays -> query -> emitter_sample -> query(any_hit) -> bsdf_eval on torch tensors."""
    torch = pytest.importorskip("torch")
    s = nori_amd.load_scene(scene_path(*CBOX), 32, 32, 1)
    n = 32 * 32
    with nori_amd.GpuRenderer(s, 0) as r:
        z = lambda c: torch.zeros((n, c), dtype=torch.float32, device="cuda:0")  # noqa: E731
        rays, surf, U, es, sh, occ, be = z(8), z(16), z(2), z(12), z(8), z(4), z(8)
        torch.cuda.synchronize()
        r.camera_rays(passes=1, out=rays.data_ptr())
        r.sample_uniforms(4, 2, passes=1, out=U)
        r.query(rays.data_ptr(), n=n, surf_out=surf.data_ptr())
        p = surf[:, 0:3].contiguous()
        torch.cuda.synchronize()
        r.emitter_sample(p, U, emitter=0, n=n, out=es)
        hit = surf[:, 11].view(torch.int32) >= 0
        sh[:, 0:3], sh[:, 3], sh[:, 4:7] = p, 1e-4, es[:, 0:3]
        sh[:, 7] = torch.where(hit, es[:, 3], torch.full_like(es[:, 3], -1.0))
        wi, view = es[:, 0:3].contiguous(), (-rays[:, 4:7]).contiguous()
        torch.cuda.synchronize()
        r.query(sh.data_ptr(), n=n, any_hit=True, hits_out=occ.data_ptr())
        r.bsdf_eval(surf, view, wi, n=n, out=be)
        # the same chain on host arrays
        h_rays = r.camera_rays(passes=1).reshape(-1, 8)
        h_surf = r.query(h_rays)["surf"]
        h_U = r.sample_uniforms(4, 2, passes=1).reshape(-1, 2)
        h_es = r.emitter_sample(np.ascontiguousarray(h_surf["p"]), h_U, emitter=0)
        h_be = r.bsdf_eval(h_surf, -h_rays[:, 4:7], np.ascontiguousarray(h_es[:, 0:3]))
    assert_same_bits(U.cpu().numpy(), h_U, "sample_uniforms")
    assert_same_bits(es.cpu().numpy(), h_es, "emitter_sample")
    assert_same_bits(be.cpu().numpy(), h_be, "bsdf_eval")
    free = (occ[:, 1].view(torch.int32) < 0) & hit
    assert 0.05 < float(free.float().mean()) < 1.0 and float(be[:, 0:3].max()) > 0


# ---------------------------------------------------------------- 5. sample_uniforms
def test_sample_uniforms_are_the_renderers(built):
    s = nori_amd.load_scene(scene_path(*CBOX), 96, 72, 8)  # 3 x 3 blocks
    H, W = 72, 96
    with nori_amd.GpuRenderer(s, 0) as r:
        whole = r.sample_uniforms(0, 7, passes=5, pass_begin=0, seed=7)
        assert whole.shape == (5, H, W, 7) and whole.dtype == f32
        assert (whole >= 0).all() and (whole < 1).all()
        # a pass range split over two calls; a draw range split over two calls
        part = r.sample_uniforms(0, 7, passes=3, pass_begin=2, seed=7)
        assert np.array_equal(_bits(part), _bits(whole[2:5]))
        tail = r.sample_uniforms(4, 3, passes=5, seed=7)
        assert np.array_equal(_bits(tail), _bits(whole[..., 4:7]))
        far = r.sample_uniforms(1000003, 2, passes=1, seed=7)
        assert not np.array_equal(whole[0, ..., 0:2], far[0]) and (far >= 0).all() and (far < 1).all()
        assert not np.array_equal(whole, r.sample_uniforms(0, 7, passes=5, seed=8))
        assert r.sample_uniforms(0, 1, passes=0).shape == (8, H, W, 1)  # pass_count 0: the scene's sampleCount
        # rendered per block, and unselected pixels untouched
        sentinel = f32(-12345.0)
        out = np.full((5, H, W, 7), sentinel, f32)
        assert r.sample_uniforms(0, 7, passes=5, seed=7, blocks=[1, 4], out=out) is out
        inside = np.zeros((H, W), bool)
        for b in (1, 4):
            by, bx = divmod(b, 3)
            inside[32 * by:32 * by + 32, 32 * bx:32 * bx + 32] = True
        assert (out[:, ~inside] == sentinel).all()
        assert np.array_equal(_bits(out[:, inside]), _bits(whole[:, inside]))
        rest = [b for b in range(s.num_blocks()) if b not in (1, 4)]
        r.sample_uniforms(0, 7, passes=5, seed=7, blocks=rest, out=out)
        assert np.array_equal(_bits(out), _bits(whole))
        rays = r.camera_rays(passes=5, seed=7)
    # draws 0-1 are the jitter of the oracle's stream of the same sample (its film position)
    k = 2
    ys, xs = np.mgrid[0:H, 0:W]
    ids = (k * H * W + ys * W + xs).ravel()
    ws = pyoracle.OracleScene(s).wave_samples(ids, seed=7)
    pos = np.stack([xs.ravel().astype(f32) + whole[k, ..., 0].ravel(), ys.ravel().astype(f32) + whole[k, ..., 1].ravel()], 1)
    assert np.array_equal(_bits(pos.astype(f32)), _bits(ws[:, 0:2]))
    # ... and they reproduce camera_rays: the perspective camera's ray through that film position
    cam = s.desc.camera
    m = np.array(list(cam.sample_to_camera), np.float64).reshape(4, 4)
    c2w = np.array(list(cam.camera_to_world), np.float64).reshape(4, 4)
    q = np.stack([pos[:, 0] / W, pos[:, 1] / H, np.zeros(len(pos)), np.ones(len(pos))], 1) @ m.T
    near = q[:, 0:3] / q[:, 3:4]
    dl = near / np.linalg.norm(near, axis=1, keepdims=True)
    dw = dl @ c2w[0:3, 0:3].T
    assert np.abs(dw - rays[k].reshape(-1, 8)[:, 4:7]).max() < 1e-5


def test_aperture_draws_reproduce_thin_lens_origins(built, tmp_path):
    """Draws 2-3 are the aperture sample: the thin-lens camera's ray origin is cameraToWorld of
    lensRadius * squareToConcentricDisk(draws 2-3) (thinlens.cpp:120-147), here in float64.
    The device forms it in float32 with at most 16 roundings of values no larger than the origin's
    largest coordinate m (the disk warp with cosf / sinf, the product by the radius, a row of the
    matrix, the division by w): |difference| <= 16 * 2^-24 * m."""
    s = nori_amd.load_scene(synth.cbox_variant(str(tmp_path), "t", integrator="path_mis", width=32, height=32,
                                               camera_type="thinlens", camera_props=THINLENS), 0, 0, 1)
    cam = s.desc.camera
    assert cam.camera_type == _abi.CAMERA_THINLENS and cam.lens_radius > 0
    with nori_amd.GpuRenderer(s, 0) as r:
        rays = r.camera_rays(passes=2, pass_begin=1, seed=5).reshape(-1, 8)
        ap = r.sample_uniforms(2, 2, passes=2, pass_begin=1, seed=5).reshape(-1, 2).astype(np.float64)
    ox, oy = 2 * ap[:, 0] - 1, 2 * ap[:, 1] - 1
    wide = np.abs(ox) > np.abs(oy)
    with np.errstate(all="ignore"):
        rad = np.where(wide, ox, oy)
        theta = np.where(wide, np.pi / 4 * (oy / ox), np.pi / 2 - np.pi / 4 * (ox / oy))
    zero = (ox == 0) & (oy == 0)
    px = np.where(zero, 0.0, rad * np.cos(theta)) * cam.lens_radius
    py = np.where(zero, 0.0, rad * np.sin(theta)) * cam.lens_radius
    c2w = np.array(list(cam.camera_to_world), np.float64).reshape(4, 4)
    h = np.stack([px, py, np.zeros_like(px), np.ones_like(px)], 1) @ c2w.T
    want = h[:, 0:3] / h[:, 3:4]
    err = float(np.abs(rays[:, 0:3] - want).max())
    m = float(np.abs(want).max())
    spread = float(np.ptp(rays[:, 0:3], axis=0).max())
    print(f"thin lens: {len(want)} origins, max |difference| {err:.3e} (bound {16 * 2.0 ** -24 * m:.3e}), lens spread {spread:.3f}")
    assert spread > cam.lens_radius  # the origins do move over the lens
    assert err <= 16 * 2.0 ** -24 * m


# ---------------------------------------------------------------- 6. dynamic geometry
def test_emitter_sample_follows_update_vertices(built, tmp_path):
    base = refit_util.load("cbox", str(tmp_path))
    P = refit_util.position_set(base, "b")
    assert not np.array_equal(P, base.positions())
    light = [i for i, sh in enumerate(base.shapes()) if sh.emitter >= 0][0]
    sh = base.shapes()[light]
    assert not np.array_equal(P[sh.vtx_offset:sh.vtx_offset + sh.vtx_count],
                              base.positions()[sh.vtx_offset:sh.vtx_offset + sh.vtx_count]), "the light's mesh moves"
    rng = np.random.default_rng(9)
    x = rng.uniform(-1, 1, (1000, 3)).astype(f32)
    u = rng.random((1000, 2), dtype=f32)
    with _renderer(base, "bvh") as r:
        before = r.emitter_sample(x, u, emitter=0)
        r.update_vertices(P)
        moved = r.emitter_sample(x, u, emitter=0)
        surf = r.query(scene_rays("cbox", base, 257))["surf"]
        ee_moved = r.emitter_eval(surf, np.zeros((257, 3), f32))
    fresh_scene = refit_util.load("cbox", str(tmp_path), positions=P)
    with _renderer(fresh_scene, "bvh") as r:
        fresh = r.emitter_sample(x, u, emitter=0)
        ee_fresh = r.emitter_eval(surf, np.zeros((257, 3), f32))  # (the same records)
    assert not np.array_equal(_bits(before), _bits(moved))
    assert_same_bits(moved, fresh, "emitter_sample after update_vertices against a fresh context")
    assert_same_bits(ee_moved, ee_fresh, "emitter_eval after update_vertices against a fresh context")


# ---------------------------------------------------------------- 7. refusals
def test_refusals_leave_the_context_usable(built):
    torch = pytest.importorskip("torch")
    s = nori_amd.load_scene(scene_path(*CBOX), 32, 32, 2)
    rays = scene_rays("cbox", s, 64)
    L, INV, n = nori_amd.lib(), _abi.NORI_ERR_INVALID, 64
    num_shapes, num_em = len(s.shapes()), len(s.emitters())
    with nori_amd.GpuRenderer(s, 0) as r:
        ref = r.query(rays)
        surf = ref["surf"].copy()
        wi = np.ascontiguousarray(-rays[:, 4:7])
        u = np.random.default_rng(1).random((n, 2), dtype=f32)
        x = np.ascontiguousarray(surf["p"])
        ids = np.zeros(n, np.int32)
        out = np.zeros((n, 12), f32)
        P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        sd = _abi.ShadingDesc(n, 0, 0, 0)
        calls = {
            "bsdf_eval": (L.nori_gpu_bsdf_eval, [P(surf), P(wi), P(wi)]),
            "bsdf_sample": (L.nori_gpu_bsdf_sample, [P(surf), P(wi), P(u)]),
            "emitter_sample": (L.nori_gpu_emitter_sample, [P(ids), P(x), P(u)]),
            "emitter_eval": (L.nori_gpu_emitter_eval, [P(surf), P(wi)]),
        }
        for name, (fn, args) in calls.items():
            assert fn(r._h, C.byref(sd), *args, P(out)) == _abi.NORI_OK, name
            assert fn(None, C.byref(sd), *args, P(out)) == INV, name
            assert fn(r._h, None, *args, P(out)) == INV, name
            assert fn(r._h, C.byref(sd), *args, None) == INV, name
            for k in range(len(args)):
                if name == "emitter_sample" and k == 0:
                    continue  # ids may be NULL
                bad = list(args)
                bad[k] = None
                assert fn(r._h, C.byref(sd), *bad, P(out)) == INV, (name, k)
            assert fn(r._h, C.byref(_abi.ShadingDesc(n, 0, 0, 1)), *args, P(out)) == INV, name  # reserved
            out[:] = 5
            assert fn(r._h, C.byref(_abi.ShadingDesc(0, 0, 0, 0)), *args, P(out)) == _abi.NORI_OK  # n == 0: a no-op
            assert (out == 5).all()
            # on_device with host pointers: not device memory
            assert fn(r._h, C.byref(_abi.ShadingDesc(n, 1, 0, 0)), *args, P(out)) == INV, name
        # host arrays: a shape index or an emitter id out of range
        for bad_shape in (num_shapes, -2):
            bad = surf.copy()
            bad["shape"][3] = bad_shape
            for name in ("bsdf_eval", "bsdf_sample", "emitter_eval"):
                fn, args = calls[name]
                assert fn(r._h, C.byref(sd), P(bad), *args[1:], P(out)) == INV, (name, bad_shape)
        for bad_id in (num_em, -1):
            bid = ids.copy()
            bid[5] = bad_id
            assert L.nori_gpu_emitter_sample(r._h, C.byref(sd), P(bid), P(x), P(u), P(out)) == INV
            assert L.nori_gpu_emitter_sample(r._h, C.byref(_abi.ShadingDesc(n, 0, bad_id, 0)), None, P(x), P(u), P(out)) == INV
        # device arrays: misaligned pointers
        d_surf = torch.from_numpy(surf.view(f32).reshape(n, 16).copy()).to("cuda:0")
        d_wi, d_u, d_out = (torch.from_numpy(a.copy()).to("cuda:0") for a in (wi, u, out))
        torch.cuda.synchronize()
        dd = _abi.ShadingDesc(n - 1, 1, 0, 0)
        V = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
        assert L.nori_gpu_bsdf_eval(r._h, C.byref(dd), V(d_surf), V(d_wi), V(d_wi), V(d_out)) == _abi.NORI_OK
        assert L.nori_gpu_bsdf_eval(r._h, C.byref(dd), V(d_surf, 4), V(d_wi), V(d_wi), V(d_out)) == INV
        assert L.nori_gpu_bsdf_eval(r._h, C.byref(dd), V(d_surf), V(d_wi, 2), V(d_wi), V(d_out)) == INV
        assert L.nori_gpu_bsdf_eval(r._h, C.byref(dd), V(d_surf), V(d_wi), V(d_wi), V(d_out, 4)) == INV
        assert L.nori_gpu_bsdf_eval(r._h, C.byref(dd), V(d_surf), V(d_wi, 4), V(d_wi), V(d_out)) == _abi.NORI_OK  # 4-byte aligned
        # sample_uniforms
        rd = _abi.RenderDesc()
        rd.pass_count = 1
        big = np.zeros((1, 32, 32, 4), f32)
        f = L.nori_gpu_sample_uniforms
        assert f(r._h, C.byref(rd), 0, 0, P(big)) == INV                     # count == 0
        assert f(r._h, C.byref(rd), 0xFFFFFFFF, 2, P(big)) == INV            # first + count overflows
        assert f(r._h, C.byref(rd), 0, 4, None) == INV and f(None, C.byref(rd), 0, 4, P(big)) == INV
        rd.variance_out = big.ctypes.data
        assert f(r._h, C.byref(rd), 0, 4, P(big)) == INV
        assert not big.any()
        rd.variance_out = None
        rd.num_blocks = 1                                                    # blocks without ids
        assert f(r._h, C.byref(rd), 0, 4, P(big)) == INV
        rd.num_blocks = 0
        d_big = torch.full((1, 32, 32, 4), 3.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        rd.output_on_device = 1
        assert f(r._h, C.byref(rd), 0, 4, V(d_big, 2)) == INV                # misaligned device buffer
        assert f(r._h, C.byref(rd), 0, 4, P(big)) == INV                     # not device memory
        assert (d_big == 3.0).all() and not big.any()
        assert f(r._h, C.byref(rd), 0, 4, V(d_big)) == _abi.NORI_OK
        assert float(d_big.max()) < 1.0
        rd.output_on_device = 0
        assert f(r._h, C.byref(rd), 0xFFFFFFFE, 1, P(big)) == _abi.NORI_OK   # the last draw that exists
        # device mode: the kernels' own range guards give zeros, the neighbours are unaffected
        good = r.bsdf_eval(surf, wi, wi)
        good_es = r.emitter_sample(x, u, ids=ids)
        hits = np.flatnonzero(surf["shape"] >= 0)
        a, b = int(hits[1]), int(hits[2])
        edited = surf.copy()
        edited["shape"][a], edited["shape"][b] = num_shapes, -1
        bid = ids.copy()
        bid[7] = num_em
        d_bad = torch.from_numpy(edited.view(f32).reshape(n, 16).copy()).to("cuda:0")
        d_ids = torch.from_numpy(bid).to("cuda:0")
        d_x = torch.from_numpy(x.copy()).to("cuda:0")
        o8 = torch.full((n, 8), 7.0, dtype=torch.float32, device="cuda:0")
        o12 = torch.full((n, 12), 7.0, dtype=torch.float32, device="cuda:0")
        o4 = torch.full((n, 4), 7.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        r.bsdf_eval(d_bad, d_wi, d_wi, n=n, out=o8)
        got = o8.cpu().numpy()
        r.bsdf_sample(d_bad, d_wi, d_u, n=n, out=o8)
        got_s = o8.cpu().numpy()
        r.emitter_eval(d_bad, d_wi, n=n, out=o4)
        got_e = o4.cpu().numpy()
        r.emitter_sample(d_x, d_u, ids=d_ids, n=n, out=o12)
        got_es = o12.cpu().numpy()
        others = np.ones(n, bool)
        others[[a, b]] = False
        assert good[[a, b]].any(), "the edited records were hits with a non-zero answer"
        for g in (got, got_s, got_e):
            assert not g[[a, b]].view(u32).any()
        assert_same_bits(got[others], good[others], "neighbours of the edited records")
        assert not got_es[7].view(u32).any() and good_es[7].any()
        r.emitter_sample(d_x, d_u, emitter=num_em, n=n, out=o12)             # desc->emitter, device mode: zeros too
        assert not o12.cpu().numpy().view(u32).any()
        others = np.arange(n) != 7
        assert_same_bits(got_es[others], good_es[others], "neighbours of the edited id")
        # the context works afterwards
        again = r.query(rays)
        assert np.array_equal(_bits(again["hits"]), _bits(ref["hits"]))
        assert np.array_equal(_bits(again["surf"]), _bits(ref["surf"]))


# ---------------------------------------------------------------- 8. the example
def test_direct_torch_example(built):
    """examples/direct_torch.py at 2 spp against sum L / n of the built-in render's statistics, bit for bit."""
    torch = pytest.importorskip("torch")
    spec = importlib.util.spec_from_file_location("direct_torch", os.path.join(ROOT, "examples", "direct_torch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    s = nori_amd.load_scene(scene_path("pa3", "odyssey", "odyssey_mis.xml"), 32, 32, 2)
    with nori_amd.GpuRenderer(s, 0) as r:
        img = mod.direct_image(r, "mis", spp=2)
        var = np.zeros((32, 32, 8), f32)
        r.render(passes=2, variance=var)
    assert img.is_cuda and img.shape == (32, 32, 3) and img.dtype == torch.float32
    keep = var[..., 6] == 2
    assert (~keep).mean() <= 0.01
    want = (var[..., 0:3] / f32(2)).astype(f32)
    assert want.max() > 0
    assert_same_bits(img.cpu().numpy()[keep], want[keep], "the example's image against the statistics' mean")


@pytest.mark.parametrize("integrator", ["ems", "mats"])
def test_direct_torch_command_line(built, tmp_path, monkeypatch, capsys, integrator):
    """main(): the arguments, --width / --height, the ems and mats branches and the PNG (run in this process)."""
    pytest.importorskip("torch")
    spec = importlib.util.spec_from_file_location("direct_torch", os.path.join(ROOT, "examples", "direct_torch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    png = str(tmp_path / f"{integrator}.png")
    monkeypatch.setattr("sys.argv", ["direct_torch.py", scene_path("pa3", "odyssey", f"odyssey_{integrator}.xml"), png,
                                     "--spp", "2", "--integrator", integrator, "--width", "48", "--height", "32"])
    mod.main()
    assert f"48x32, direct_{integrator}, 2 spp" in capsys.readouterr().out
    img = nori_amd.read_image(png)
    assert img.shape == (32, 48, 3) and img.max() > 0
    # ... and the image is the built-in integrator's per-sample mean (8-bit: compared as bytes)
    s = nori_amd.load_scene(scene_path("pa3", "odyssey", f"odyssey_{integrator}.xml"), 48, 32, 2)
    with nori_amd.GpuRenderer(s, 0) as r:
        var = np.zeros((32, 48, 8), f32)
        r.render(passes=2, variance=var)
    assert (var[..., 6] == 2).all()
    assert np.array_equal(img, nori_amd.ldr_bytes((var[..., 0:3] / f32(2)).astype(f32)))
