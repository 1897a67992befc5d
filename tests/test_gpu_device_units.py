"""Unit tests of the device code of device_math.h and shading.h, run on the GPU
through libnori_devtest.so (csrc/devtest.hip, tests/devtest_util.py) -- the
routines the image-parity tests only see through whole renders.  The library
also covers the tail finisher's pieces (k_tail_prefix's body, the path
lookup of tail_index.h, coop_scan) and the primitive tests of scan.h
(tri_hit*, sphere_hit*, box_test): tests/test_gpu_finish_tail.py.

a. the fast-math forms (sqrt_rn, rcp_rn, rcp_full and the FAST variants of
   fsqrt, normalize, frame_from, fresnel) against IEEE, bit for bit, and
   pcg_skip3 against three steps;
b. bsdf_sample / bsdf_eval / bsdf_pdf / dielectric_wo against the oracle on the
   input sets of device_unit_inputs.py: bit-equal where the path has no
   transcendental, within the tolerances measured by test_bsdf_ref64.py
   (E_dir, E_val) where it has;
c. the chi^2 test of tests/test_chi2.py with the device's microfacet sampling
   and pdf;
d. glass_step against glass_bounce + chord_hit, bit for bit.

Equality is of 32-bit patterns, NaN against NaN counting as equal.
"""
import numpy as np
import pytest
from scipy import special

import bsdf_ref64 as R
import device_unit_inputs as I
import devtest_util as D
import nori_amd
import pyoracle
from test_chi2 import _bsdfs as chi2_bsdfs
from test_chi2 import chi2_test

pytestmark = pytest.mark.gpu
A = nori_amd._abi
f32, u32 = np.float32, np.uint32


def same_bits(a, b):
    """Elementwise: equal bit patterns, or NaN on both sides."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return (a.view(u32) == b.view(u32)) | (np.isnan(a) & np.isnan(b))


def assert_same_bits(a, b, what, inputs=None):
    ok = same_bits(a, b)
    if not ok.all():
        i = np.argwhere(~ok)[0]
        row = tuple(i)
        where = f" at input {inputs[row[0]]!r}" if inputs is not None else ""
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} differ, first at {row}{where}: "
                             f"{np.asarray(a)[row]!r} ({np.asarray(a, f32).view(u32)[row]:#x}) against "
                             f"{np.asarray(b)[row]!r} ({np.asarray(b, f32).view(u32)[row]:#x})")


# ---------------------------------------------------------------- a. fast math
@pytest.fixture(scope="module")
def floats(built):
    x = I.math_inputs()
    x.setflags(write=False)
    return x


def test_sqrt_rn_is_ieee(floats):
    with np.errstate(all="ignore"):
        ref = np.sqrt(floats)
    assert_same_bits(D.math(D.SQRT_RN, floats), ref, "sqrt_rn", floats)
    fast, ieee = D.math(D.FSQRT_FAST, floats), D.math(D.FSQRT_IEEE, floats)
    assert_same_bits(ieee, ref, "fsqrt<false>", floats)
    assert_same_bits(fast, ieee, "fsqrt<true> against fsqrt<false>", floats)


def test_rcp_full_is_ieee(floats):
    with np.errstate(all="ignore"):
        ref = f32(1) / floats
    got = D.math(D.RCP_FULL, floats)
    assert_same_bits(got, ref, "rcp_full", floats)
    zero = floats == 0
    assert np.isinf(got[zero]).all() and (np.signbit(got[zero]) == np.signbit(floats[zero])).all()


def test_rcp_rn_is_ieee_on_its_domain(floats):
    """|x| >= 2^-125, up to and including inf, and NaN (device_math.h rcp_rn)."""
    dom = ~(np.abs(floats) < f32(2.0 ** -125))
    x = floats[dom]
    assert (np.abs(x) > f32(2.0 ** 125)).sum() > 1000 and np.isnan(x).any() and np.isinf(x).any()
    with np.errstate(all="ignore"):
        ref = f32(1) / x
    assert_same_bits(D.math(D.RCP_RN, x), ref, "rcp_rn", x)


@pytest.fixture(scope="module")
def vectors(built):
    v = I.vector_inputs()
    v.setflags(write=False)
    return v


def test_normalize_fast_is_ieee(vectors):
    fast, ieee = D.math(D.NORMALIZE_FAST, vectors), D.math(D.NORMALIZE_IEEE, vectors)
    assert_same_bits(ieee, R.normalize32(vectors), "normalize<false> against numpy float32", vectors)
    assert_same_bits(fast, ieee, "normalize<true> against normalize<false>", vectors)


def test_frame_from_fast_is_ieee(vectors):
    fast, ieee = D.math(D.FRAME_FAST, vectors), D.math(D.FRAME_IEEE, vectors)
    assert_same_bits(ieee, R.frame32(vectors), "frame_from<false> against numpy float32", vectors)
    assert_same_bits(fast, ieee, "frame_from<true> against frame_from<false>", vectors)
    assert (np.abs(vectors[:, 0]) == np.abs(vectors[:, 1])).sum() > 1000  # the tie of the branch


@pytest.mark.parametrize("int_ior,ext_ior", I.DIELECTRIC_IORS)
def test_fresnel_fast_is_ieee(built, int_ior, ext_ior):
    c = I.cosine_inputs((ext_ior, int_ior))
    fast = D.math(D.FRESNEL_FAST, c, ext_ior, int_ior)
    ieee = D.math(D.FRESNEL_IEEE, c, ext_ior, int_ior)
    ref = R.fresnel32(c, ext_ior, int_ior)
    assert_same_bits(ieee, ref, "fresnel<false> against numpy float32", c)
    assert_same_bits(fast, ieee, "fresnel<true> against fresnel<false>", c)
    if int_ior != ext_ior:  # both sides of the critical angle are in the set
        assert (ref == 1).sum() > 1000 and ((ref > 0) & (ref < 1)).sum() > 1000


def test_tan_theta(vectors):
    v = vectors
    with np.errstate(all="ignore"):
        t = f32(1) - v[:, 2] * v[:, 2]
        ref = np.where(t <= 0, f32(0), np.sqrt(t) / v[:, 2]).astype(f32)
    assert_same_bits(D.math(D.TAN_THETA, v), ref, "tan_theta", v)


def test_pcg_skip3_is_three_steps(built):
    rng = np.random.default_rng(11)
    n = 1 << 20
    state = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    inc = rng.integers(0, 1 << 64, n, dtype=np.uint64) | np.uint64(1)
    state[:4] = [0, 1, (1 << 64) - 1, 1 << 63]
    inc[:4] = [1, (1 << 64) - 1, (1 << 64) - 1, 1]
    skip, three = D.pcg_skip3(state, inc)
    ref = state.copy()
    with np.errstate(over="ignore"):
        for _ in range(3):  # ext/pcg32/pcg32.h: state * 0x5851f42d4c957f2d + inc, mod 2^64
            ref = ref * np.uint64(0x5851F42D4C957F2D) + inc
    assert np.array_equal(three, ref), "three pcg_skip(r, 1) against the generator's recurrence"
    assert np.array_equal(skip, three), "pcg_skip3 against three steps"


# ---------------------------------------------------------------- b. BSDFs against the oracle
CONFIGS = I.configs()
DIR_TOL = max(4 * I.E_DIR, 8 * 2.0 ** -24)


@pytest.fixture(scope="module")
def oracle(built):
    """name -> the inputs and the oracle's outputs, computed once and read-only."""
    cache = {}

    def get(name):
        if name not in cache:
            d = dict(CONFIGS)[name]
            wi, u, uv = I.sample_inputs(d)
            smp = pyoracle.bsdf_sample_uv(d, wi, u, uv)
            ewi, ewo, euv = I.eval_inputs(d, smp[:, :3])
            ep = pyoracle.bsdf_eval_pdf_uv(d, ewi, ewo, euv)
            cache[name] = dict(wi=wi, u=u, uv=uv, smp=smp, ewi=ewi, ewo=ewo, euv=euv, ep=ep)
            for a in cache[name].values():
                a.setflags(write=False)
        return cache[name]

    return get


def _nonfinite_pattern_equal(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN where the oracle has none, or the reverse"
    assert np.array_equal(np.isinf(got), np.isinf(ref)), f"{what}: infinite where the oracle is finite, or the reverse"


@pytest.mark.parametrize("name", [n for n, _ in CONFIGS])
def test_bsdf_sample_against_oracle(oracle, name):
    d, o = dict(CONFIGS)[name], oracle(name)
    wi, u, uv, ref = o["wi"], o["u"], o["uv"], o["smp"]
    got = D.bsdf_sample(d, wi, u, uv)
    n = wi.shape[0]
    rows = np.concatenate([wi, u], 1)
    # measure, and the luminance of the weight as luminance() of its components
    assert np.array_equal(got[:, 7], ref[:, 7]), "measure"
    lum = (got[:, 3] * f32(0.212671) + got[:, 4] * f32(0.715160)) + got[:, 5] * f32(0.072169)
    assert_same_bits(got[:, 6], lum, "luminance(weight)")
    _nonfinite_pattern_equal(got[:, :7], ref[:, :7], name)
    w, wr = got[:, 3:7], ref[:, 3:7]
    assert not (w < 0).any(), "negative weight"
    if I.exact(d) or d.type == A.BSDF_DIFFUSE:
        # no transcendental on the path (mirror, dielectric) or in the weight (diffuse: the albedo)
        assert_same_bits(w, wr, f"{name}: weight", rows)
    if I.exact(d):
        assert_same_bits(got[:, :3], ref[:, :3], f"{name}: wo", rows)
        return
    # directions: |difference| <= max(4 E_dir, 8 * 2^-24) wherever they are numbers
    num = ~np.isnan(ref[:, :3]).any(1)
    e_dir = float(np.abs(got[num, :3] - ref[num, :3]).max())
    # the zero / non-zero pattern of the weight, except next to the horizon
    differs = ((w[:, 3] == 0) != (wr[:, 3] == 0))
    horizon = np.abs(ref[:, 2]) < 1e-5
    exceptions = int((differs & horizon).sum())
    # The weight on the well-conditioned subset.  The device's direction is
    # up to DIR_TOL away from the oracle's, and a narrow lobe turns that into a
    # larger relative change of eval * cos / pdf than E_val (measured at one
    # direction) allows: 1.1e-5 against 4 * 2.5e-6 for alpha = 0.1.  So the
    # oracle is asked for eval and pdf at the device's own direction, and its
    # weight is formed as Microfacet::sample / Disney::sample form it.
    e_w, n_w = 0.0, 0
    if d.type != A.BSDF_DIFFUSE:
        wo = np.ascontiguousarray(got[:, :3])
        ep = pyoracle.bsdf_eval_pdf_uv(d, wi, wo, uv)
        with np.errstate(all="ignore"):
            wo_w = (ep[:, :3] * wo[:, 2:3]) / ep[:, 3:4]
            wo_l = (wo_w[:, 0] * f32(0.212671) + wo_w[:, 1] * f32(0.715160)) + wo_w[:, 2] * f32(0.072169)
        well = I.well_conditioned(wi, wo) & (w[:, 3] != 0)
        e_w, n_w = float(I.rel_diff(w[well, 3], wo_l[well]).max()), int(well.sum())
        assert n_w > 1000
    print(f"{name}: {n} samples, direction error {e_dir:.3e} (bound {DIR_TOL:.3e}), weight luminance error "
          f"{e_w:.3e} over {n_w} (bound {4 * I.E_VAL[name]:.3e}), {exceptions} horizon exceptions")
    assert e_dir <= DIR_TOL
    assert not (differs & ~horizon).any(), "a weight is zero where the oracle's is not, away from the horizon"
    assert exceptions <= 1e-3 * n
    assert e_w <= 4 * I.E_VAL[name]


@pytest.mark.parametrize("name", [n for n, _ in CONFIGS])
def test_bsdf_eval_pdf_against_oracle(oracle, name):
    d, o = dict(CONFIGS)[name], oracle(name)
    wi, wo, uv, ref = o["ewi"], o["ewo"], o["euv"], o["ep"]
    got = D.bsdf_eval_pdf(d, wi, wo, uv)
    rows = np.concatenate([wi, wo], 1)
    if I.exact_eval(d):  # sqrt, division and double products only
        assert_same_bits(got, ref, f"{name}: eval / pdf", rows)
        return
    _nonfinite_pattern_equal(got, ref, name)
    num = np.isfinite(ref).all(1)
    assert np.array_equal(got[num] < 0, ref[num] < 0)  # (eval is negative below the horizon in the reference too)
    assert np.array_equal(got[num] == 0, ref[num] == 0) or _only_underflow(got[num], ref[num]), "zero pattern"
    well = I.well_conditioned(wi, wo) & num
    e = float(I.rel_diff(got[well], ref[well]).max())
    print(f"{name}: eval / pdf error {e:.3e} over {int(well.sum())} pairs "
          f"(bounds {4 * I.E_VAL[name]:.3e} and {EXPF_TOL:.3e})")
    assert e <= 4 * I.E_VAL[name]
    assert e <= EXPF_TOL


# Microfacet eval and pdf on the same (wi, wo): the two sides differ only in
# expf -- glibc's is within 1 ulp, the ROCm device library documents 1 ulp --
# so the factor differs by at most 2 ulp, and each of the at most six float
# operations that follow (/ (pi alpha^2 cos^4), * ks, * F, * G, / den, + kd/pi;
# or * cos, / (4 |n.wo|), * ks, + the diffuse term) rounds the two slightly
# different values apart by at most one more: 8 ulp = 8 * 2^-23.
EXPF_TOL = 8 * 2.0 ** -23


def _only_underflow(got, ref):
    """The zero patterns differ only where the other side is below TINY."""
    d = (got == 0) != (ref == 0)
    return bool((np.maximum(np.abs(got[d]), np.abs(ref[d])) < I.TINY).all())


@pytest.mark.parametrize("name", [n for n, d in CONFIGS if I.basic(d)])
def test_basic_plugin_set_equals_full(oracle, name):
    """bsdf_*<false> is bsdf_*<true> for constant-albedo diffuse, mirror and dielectric."""
    d, o = dict(CONFIGS)[name], oracle(name)
    full = D.bsdf_sample(d, o["wi"], o["u"], o["uv"], full=True)
    lite = D.bsdf_sample(d, o["wi"], o["u"], o["uv"], full=False)
    assert_same_bits(lite, full, f"{name}: bsdf_sample<false>")
    full = D.bsdf_eval_pdf(d, o["ewi"], o["ewo"], o["euv"], full=True)
    lite = D.bsdf_eval_pdf(d, o["ewi"], o["ewo"], o["euv"], full=False)
    assert_same_bits(lite, full, f"{name}: bsdf_eval / bsdf_pdf<false>")


# ---------------------------------------------------------------- c. chi^2 of the device's sampling
def test_device_microfacet_chi2(built):
    """tests/test_chi2.py's procedure with the device's bsdf_sample and bsdf_pdf."""
    res_t, res_p, n, tests_per_bsdf = 10, 20, 10 * 20 * 5000, 5
    bsdfs = chi2_bsdfs()
    assert len(bsdfs) == 3
    rng = np.random.default_rng(2024)
    gx, gw = special.roots_legendre(24)
    # the quadrature points of all 200 cells: one bsdf_pdf call per incident direction
    pts, wts = [], []
    for i in range(res_t):
        c0, c1 = -1 + i * 2 / res_t, -1 + (i + 1) * 2 / res_t
        cs = 0.5 * (c1 - c0) * gx + 0.5 * (c1 + c0)
        for j in range(res_p):
            p0, p1 = j * 2 * np.pi / res_p, (j + 1) * 2 * np.pi / res_p
            phs = 0.5 * (p1 - p0) * gx + 0.5 * (p1 + p0)
            C, P = np.meshgrid(cs, phs, indexing="ij")
            S = np.sqrt(1 - C * C)
            pts.append(np.stack([S * np.cos(P), S * np.sin(P), C], -1).reshape(-1, 3).astype(f32))
            wts.append((np.outer(gw, gw) * 0.25 * (c1 - c0) * (p1 - p0)).ravel())
    pts, wts = np.concatenate(pts), np.stack(wts)
    fails = []
    for b in bsdfs:
        for _ in range(tests_per_bsdf):
            ct = rng.random()
            st, ph = np.sqrt(max(0.0, 1 - ct * ct)), 2 * np.pi * rng.random()
            wi = np.array([np.cos(ph) * st, np.sin(ph) * st, ct], f32)
            smp = D.bsdf_sample(b, np.tile(wi, (n, 1)), rng.random((n, 2), dtype=f32))
            wo = smp[smp[:, 6] != 0, :3]
            tb = np.clip(np.floor((wo[:, 2] * 0.5 + 0.5) * res_t).astype(int), 0, res_t - 1)
            sp = np.arctan2(wo[:, 1], wo[:, 0]) * (1 / (2 * np.pi))
            sp = np.where(sp < 0, sp + 1, sp)
            pb = np.clip(np.floor(sp * res_p).astype(int), 0, res_p - 1)
            obs = np.bincount(tb * res_p + pb, minlength=res_t * res_p).astype(np.float64)
            pdf = D.bsdf_eval_pdf(b, np.tile(wi, (pts.shape[0], 1)), pts)[:, 3].astype(np.float64)
            exp = (pdf.reshape(res_t * res_p, -1) * wts).sum(1) * n
            ok, msg = chi2_test(obs, exp, n, 5, 0.01, tests_per_bsdf * len(bsdfs))
            print(f"alpha {b.alpha}: {msg}")
            if not ok:
                fails.append((b.alpha, msg))
    assert not fails, fails


# ---------------------------------------------------------------- d. glass chain
GLASS_LANES = 1 << 18
GLASS_EDGE_LANES = 1 << 15


@pytest.mark.parametrize("integrator", [A.INTEGRATOR_PATH_MIS, A.INTEGRATOR_PATH_MATS], ids=["path_mis", "path_mats"])
def test_glass_step_equals_bounce_and_chord(built, integrator):
    mis = integrator == A.INTEGRATOR_PATH_MIS
    glass = I._desc(A.BSDF_DIELECTRIC)  # the defaults of dielectric.cpp: 1.5046 / 1.000277
    total = dict(lanes=0, chord=0, step=0, refracted=0, roulette=0, other=0)
    finite_total = dict(step=0, refracted=0, roulette=0, other=0)  # the same over the lanes of finite beta
    for k, (name, center, radius) in enumerate(I.GLASS_SPHERES):
        n = GLASS_LANES // 3 + (GLASS_LANES % 3 if k == 0 else 0)
        main = I.glass_inputs(center, radius, n, 100 + k)
        edge = I.glass_inputs(center, radius, GLASS_EDGE_LANES, 200 + k, *I.GLASS_EDGE_COS[name])
        o, d, beta = (np.concatenate([a, b]) for a, b in zip(main, edge))
        r = D.glass(integrator, center, radius, glass, 0x5EED + k, o, d, beta)
        fl, inp, step, bnc = r["flags"], r["input"], r["step"], r["bounce"]
        chord = (fl & D.GLASS_CHORD) != 0
        taken = (fl & D.GLASS_STEP) != 0
        alive = (fl & D.GLASS_ALIVE) != 0
        hit = (fl & D.GLASS_HIT) != 0
        assert not (taken & ~chord).any()

        def same_state(a, b):
            fa, fb = a[:, :12].view(f32), b[:, :12].view(f32)
            ta, tb = a[:, 14].view(f32), b[:, 14].view(f32)
            return (same_bits(fa, fb).all(1) & (a[:, 12] == b[:, 12]) & (a[:, 13] == b[:, 13]) & same_bits(ta, tb))

        # the input state is what was asked for
        assert np.array_equal(inp[:, 0:3].view(f32), o) and np.array_equal(inp[:, 3:6].view(f32), d)
        assert same_bits(inp[:, 8:11].view(f32), beta).all()
        # glass_step taken: route B survived, hit the sphere again, and every word agrees
        assert (alive & hit)[taken].all(), f"{name}: glass_step went on where glass_bounce / chord_hit did not"
        eq = same_state(step, bnc)
        assert eq[taken].all(), (f"{name}: {int((taken & ~eq).sum())} lanes differ between the routes, first "
                                 f"{step[taken & ~eq][0].tolist()} against {bnc[taken & ~eq][0].tolist()}")
        # not taken: nothing changed
        assert same_state(step, inp)[~taken].all(), f"{name}: glass_step changed the state of a lane it handed back"
        # the other direction: wherever route B stays on the sphere with a skippable NEE, the step is taken
        fin = np.isfinite(bnc[:, 8:11].view(f32)).all(1)
        should = chord & alive & hit & (fin if mis else True)
        pb = bnc[:, 0:3].view(f32).astype(np.float64)
        outward = ((pb - np.array(center, np.float64)) * bnc[:, 3:6].view(f32)).sum(1) > 0
        reflected = should & ~outward
        assert (taken | ~reflected).all(), f"{name}: a reflected lane with a next chord was handed back"
        if mis:
            nonfinite = ~np.isfinite(beta).all(1)
            assert not (taken & nonfinite).any(), "path_mis: a non-finite throughput must hand back"
            assert (bnc[alive, 11].view(f32) == -1).all() and (step[taken, 11].view(f32) == -1).all()
        else:
            assert (step[:, 11].view(f32) == f32(0.5)).all()  # path_mats never touches prev
        outcome = dict(step=taken, refracted=chord & alive & ~taken & outward, roulette=chord & ~alive,
                       other=chord & alive & ~taken & ~outward)
        c = dict(lanes=fl.size, chord=int(chord.sum()), **{key: int(m.sum()) for key, m in outcome.items()})
        finite_beta = np.isfinite(beta).all(1)
        for key, m in outcome.items():
            finite_total[key] += int((m & finite_beta).sum())
        print(f"{'path_mis' if mis else 'path_mats'} {name}: {c}")
        assert c["chord"] == c["step"] + c["refracted"] + c["roulette"] + c["other"]
        for key, v in c.items():
            total[key] += v
    print(f"{'path_mis' if mis else 'path_mats'} total: {total}")
    # the inputs reach every outcome: step taken, refracted out, ended by
    # Russian roulette, no next chord or handed back
    for key in ("step", "refracted", "roulette", "other"):
        assert total[key] >= 1000, (key, total)
    # about 3/4 of the cosines are beyond the critical angle: among the lanes
    # that may step (path_mis hands every non-finite beta back) most do
    print(f"finite beta: {finite_total}")
    assert finite_total["step"] > max(finite_total["refracted"], finite_total["roulette"], finite_total["other"])
