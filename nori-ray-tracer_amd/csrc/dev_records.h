// dev_records.h -- the three plain records of a scene's device tables:
// DevShape, DevBsdf and DevEmitter.  Only <stdint.h>, so the host compiler
// takes it (scene_plan.h builds the tables without a device) as well as hipcc
// and hipRTC (dev_scene.h and device_math.h include it).
#pragma once
#include <stdint.h>

namespace nori {

struct DevShape {
    int32_t type, bsdf, emitter, has_normals;
    uint32_t prim_offset, prim_count, cdf_offset, has_uvs;
    float center[3], radius;
    float area_norm;     // DiscretePDF::getNormalization (mesh) or sphere pdf
    int32_t nm_w, nm_h, nm_wrap;  // NormalMap (meshes with normals, mesh.cpp:147-155)
    // sphere only: no other primitive meets the closed ball (host-checked with
    // a margin, and the ball lies inside the scene box): a ray from a point of
    // this sphere that hits it again hits nothing before (the chord is inside
    // the ball), so the tail finisher takes that hit without a scene scan
    int32_t solitary;
    const uint32_t *nmap;         // RGBX8 texels in global memory, or null
};

// 128 B.  Area: radiance.  Envmap (envmap.cpp): R x C texels (R = Bitmap rows,
// the reference's m_width), tables at float offsets into DevScene::env:
// rgb R*C*3, pdf R*C, cdf R*(C+1), marginal pdf R, marginal cdf R+1.
// Point (pointlight.cpp): position, power.  Spot (spotlight.cpp): position,
// power (= "color"), direction, cosines of falloffStart and totalWidth.
struct DevEmitter {
    int32_t type, shape;
    float radiance[3];
    float weight;
    int32_t R, C;
    uint32_t rgb_off, pdf_off, cdf_off, pmarg_off, cmarg_off;
    float position[3], power[3], direction[3], cos_fs, cos_tw;
    uint32_t pad[8];
};
static_assert(sizeof(DevEmitter) == 128, "DevEmitter layout");

// Device BSDF record: desc values plus derived constants.
struct DevBsdf {
    int32_t type;
    float albedo[3];
    float int_ior, ext_ior, alpha, ks;
    float kd[3];
    float base[3];
    float metallic, specular, roughness, sheen, sheen_tint, spec_tint, d_alpha;
    int32_t tex;  // diffuse albedo: NORI_TEXTURE_CONSTANT (albedo), _CHECKERBOARD (albedo = value1) or _IMAGE
    float tex_v2[3], tex_delta[2], tex_scale[2];
    int32_t img_w, img_h, img_wrap;  // NORI_TEXTURE_IMAGE: RGBX8 texels in global memory
    const uint32_t *img;
    // the IOR quotients fresnel() and Dielectric::sample compute per call,
    // computed once on the host with the same float divisions:
    // ext/int, int/ext and 1.0f / (ext/int)
    float eta_ei, eta_ie, inv_eta_ei;
};

}  // namespace nori
