// bsdf_desc.h -- nori_bsdf_desc -> DevBsdf on the host: the desc values and
// the constants derived from them once per scene (the IOR quotients, ks,
// Disney's alpha).  Shared by the scene plan (scene_plan.cpp) and the
// test-only device library (devtest.hip), so the unit tests run the product's
// derived constants.  Host code; compiled with -ffp-contract=off like the
// rest, so every quotient rounds as the reference's per-call division does.
#pragma once
#include <cstring>

#include "../../include/nori_gpu.h"
#include "dev_records.h"
#include "material_row.h"

namespace nori {

// Everything but the image texture (img, img_w, img_h, img_wrap stay zero:
// the caller owns the texel storage) and the range checks of the upload.
inline void dev_bsdf_from_desc(const nori_bsdf_desc &b, DevBsdf &o) {
    std::memset(&o, 0, sizeof(o));
    o.type = b.type;
    for (int k = 0; k < 3; ++k) o.albedo[k] = b.albedo[k], o.kd[k] = b.kd[k], o.base[k] = b.base_color[k];
    o.int_ior = b.int_ior;
    o.ext_ior = b.ext_ior;
    o.eta_ei = b.ext_ior / b.int_ior;  // the divisions of common.cpp:296 / dielectric.cpp:57-60, done once
    o.eta_ie = b.int_ior / b.ext_ior;
    o.inv_eta_ei = 1 / o.eta_ei;
    o.alpha = b.alpha;
    o.metallic = b.metallic;
    o.specular = b.specular;
    o.roughness = b.roughness;
    o.sheen = b.sheen;
    o.sheen_tint = b.sheen_tint;
    o.spec_tint = b.specular_tint;
    bsdf_derived(o);  // ks and d_alpha (material_row.h: nori_gpu_update_materials recomputes them with it)
    o.tex = b.albedo_texture;
    for (int k = 0; k < 3; ++k) o.tex_v2[k] = b.tex_value2[k];
    for (int k = 0; k < 2; ++k) o.tex_delta[k] = b.tex_delta[k], o.tex_scale[k] = b.tex_scale[k];
}

}  // namespace nori
