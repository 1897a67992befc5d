// material_row.h -- the material row of nori_gpu.h (NORI_MATERIAL_FLOATS
// floats per BSDF) against the DevBsdf record: which words a BSDF uses, the
// row of a record, a row set into a record, and the constants derived from
// the parameters.  One definition for the host (the scene plan through
// bsdf_desc.h, the host statements) and the device (k_materials_set), so a
// context updated to some values holds the bits a context created with them
// holds.  Only dev_records.h and the ABI's constants: the host compiler takes it.
#pragma once
#include "dev_records.h"

#ifdef __HIPCC_RTC__
#include "nori_gpu.h"
#else
#include "../../include/nori_gpu.h"
#endif

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
#define NORI_ROW_FN __host__ __device__ inline
#else
#define NORI_ROW_FN inline
#endif

namespace nori {

// Bit w: word w of the row is in use for this BSDF.
NORI_ROW_FN uint32_t material_words(int32_t type, int32_t tex) {
    switch (type) {
    case NORI_BSDF_DIFFUSE:
        return tex == NORI_TEXTURE_CONSTANT ? 0x0007u : tex == NORI_TEXTURE_CHECKERBOARD ? 0x1C07u : 0u;
    case NORI_BSDF_MICROFACET: return 0x000Fu;
    case NORI_BSDF_DISNEY: return 0x03F7u;
    default: return 0u;
    }
}

// The constants derived from the parameters, with the operations of the
// reference's constructors: ks (microfacet.cpp:45), Disney's pdf alpha
// (disney.cpp:59, the square taken in double).
NORI_ROW_FN void bsdf_derived(DevBsdf &o) {
    float mk = o.kd[0] < o.kd[1] ? o.kd[1] : o.kd[0];
    mk = mk < o.kd[2] ? o.kd[2] : mk;
    o.ks = 1 - mk;
    const double r2 = (double)o.roughness * (double)o.roughness;
    o.d_alpha = (float)(r2 > 1e-3 ? r2 : 1e-3);
}

// The record's row: the words in use, zeros elsewhere.
NORI_ROW_FN void material_row_get(const DevBsdf &b, float row[NORI_MATERIAL_FLOATS]) {
    const uint32_t used = material_words(b.type, b.tex);
    const float *col = b.type == NORI_BSDF_MICROFACET ? b.kd : b.type == NORI_BSDF_DISNEY ? b.base : b.albedo;
    const float all[NORI_MATERIAL_FLOATS] = {col[0],   col[1],       col[2],      b.alpha,     b.metallic,  b.specular,
                                             b.roughness, b.sheen,   b.sheen_tint, b.spec_tint, b.tex_v2[0], b.tex_v2[1],
                                             b.tex_v2[2], 0.0f,      0.0f,        0.0f};
    for (int w = 0; w < NORI_MATERIAL_FLOATS; ++w) row[w] = (used >> w & 1u) ? all[w] : 0.0f;
}

// The row's words in use set into the record, the derived constants after them.
NORI_ROW_FN void material_row_set(DevBsdf &b, const float row[NORI_MATERIAL_FLOATS]) {
    const uint32_t used = material_words(b.type, b.tex);
    if (!used) return;
    float *col = b.type == NORI_BSDF_MICROFACET ? b.kd : b.type == NORI_BSDF_DISNEY ? b.base : b.albedo;
    for (int k = 0; k < 3; ++k) col[k] = row[k];
    if (used & 0x0008u) b.alpha = row[3];
    if (used & 0x0010u) {
        b.metallic = row[4], b.specular = row[5], b.roughness = row[6];
        b.sheen = row[7], b.sheen_tint = row[8], b.spec_tint = row[9];
    }
    if (used & 0x0400u)
        for (int k = 0; k < 3; ++k) b.tex_v2[k] = row[10 + k];
    bsdf_derived(b);
}

}  // namespace nori
