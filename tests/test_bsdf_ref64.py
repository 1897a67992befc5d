"""The oracle's BSDFs against the float64 / correctly-rounded-libm model of
tests/bsdf_ref64.py, on exactly the input sets of the device unit tests
(tests/device_unit_inputs.py).  No GPU needed.

This validates the model, and it measures the tolerances that
tests/test_gpu_device_units.py gives the device:

E_dir  largest |difference| of a component of a sampled direction between
       pyoracle.bsdf_sample_uv and bsdf_ref64.sample_dir.
       Measured 4.62e-7 (Disney, metallic 1, roughness 0.5 and 1; 1.19e-7 for
       the cosine lobe, at most 2.98e-7 for the microfacet configurations).
E_val  largest relative difference of eval, pdf and weight luminance between
       the oracle and bsdf_ref64.eval_pdf64 on the well-conditioned subset
       (wi.z, wo.z and the half-vector's z all >= 0.05; nothing inside it is
       left out; values below 2^-83 are compared absolutely,
       device_unit_inputs.rel_diff).  Measured per configuration:
       1.0e-7 diffuse and microfacet with ks = 0; 1.1e-6 .. 2.9e-5 the other
       microfacet BSDFs with alpha >= 0.05; 4.6e-7 .. 7.4e-6 Disney with
       roughness >= 0.5; and 0.15 .. 0.32 for the narrow lobes (microfacet
       alpha = 1e-3, Disney roughness 0 and 0.02), whose float32 formulas
       are ill-conditioned at the peak whatever the directions' z.  So the
       single E_val of all configurations is 0.317; the GPU tests use each
       configuration's own value, which is never larger.

Both are recorded in device_unit_inputs.E_DIR / E_VAL and asserted here with a
2x margin, so a drift of the oracle shows.
"""
import numpy as np
import pytest

import bsdf_ref64 as R
import device_unit_inputs as I
import pyoracle

A = I.A
MODELLED = [(n, d) for n, d in I.configs() if d.type in (A.BSDF_DIFFUSE, A.BSDF_MICROFACET, A.BSDF_DISNEY)]


@pytest.fixture(scope="module")
def oracle_samples(built):
    """name -> (wi, u, uv, oracle sample rows (n, 8)); computed once, read-only."""
    out = {}
    for name, d in I.configs():
        wi, u, uv = I.sample_inputs(d)
        o = pyoracle.bsdf_sample_uv(d, wi, u, uv)
        for a in (wi, u, uv, o):
            a.setflags(write=False)
        out[name] = (wi, u, uv, o)
    return out


def test_sampled_directions_match_the_model(oracle_samples):
    worst = 0.0
    for name, d in MODELLED:
        wi, u, _, o = oracle_samples[name]
        m = R.sample_dir(d, wi, u)
        assert np.array_equal(np.isnan(o[:, :3]), np.isnan(m)), name
        e = float(np.nanmax(np.abs(o[:, :3] - m)))
        print(f"{name}: E_dir {e:.3e} over {wi.shape[0]} samples")
        worst = max(worst, e)
    print(f"E_dir = {worst:.3e} (recorded {I.E_DIR:.3e})")
    assert worst <= 2 * I.E_DIR


def test_values_match_the_model(oracle_samples):
    measured = {}
    for name, d in MODELLED:
        wi_s, _, uv_s, o = oracle_samples[name]
        wi, wo, uv = I.eval_inputs(d, o[:, :3])
        ep = pyoracle.bsdf_eval_pdf_uv(d, wi, wo, uv)
        ev64, pdf64 = R.eval_pdf64(d, wi, wo, uv)
        well = I.well_conditioned(wi, wo)
        assert well.sum() > 1000, name
        e_eval = float(I.rel_diff(ep[well, :3], ev64[well]).max())
        e_pdf = float(I.rel_diff(ep[well, 3], pdf64[well]).max())
        # the weight, at the direction the oracle sampled
        ws = I.well_conditioned(wi_s, o[:, :3]) & (o[:, 6] != 0)
        assert ws.sum() > 1000, name
        e_w = float(I.rel_diff(o[ws, 6], R.weight_lum64(d, wi_s[ws], o[ws, :3], uv_s[ws])).max())
        print(f"{name}: eval {e_eval:.3e} pdf {e_pdf:.3e} weight {e_w:.3e} "
              f"({int(well.sum())} pairs, {int(ws.sum())} samples)")
        assert np.isfinite([e_eval, e_pdf, e_w]).all(), name
        measured[name] = max(e_eval, e_pdf, e_w)
    print("E_VAL = {" + ", ".join(f'"{k}": {v:.3g}' for k, v in measured.items()) + "}")
    print(f"E_val = {max(measured.values()):.3e} (recorded {max(I.E_VAL.values()):.3e})")
    for name, e in measured.items():
        assert e <= 2 * I.E_VAL[name], (name, e, I.E_VAL[name])


def test_horizon_samples_stay_under_the_cap(oracle_samples):
    """The GPU tests let the zero / non-zero pattern of a weight differ where
    the oracle's |wo.z| < 1e-5, for at most 0.1 % of a configuration's
    samples: the inputs must leave room for that.  (Mirror and dielectric are
    bit-equal on the device and get no such allowance.)"""
    for name, _ in MODELLED:
        o = oracle_samples[name][3]
        near = int((np.abs(o[:, 2]) < 1e-5).sum() - (o[:, :3] == 0).all(1).sum())
        print(f"{name}: {near} of {o.shape[0]} sampled directions within 1e-5 of the horizon")
        assert near <= 1e-3 * o.shape[0], name
