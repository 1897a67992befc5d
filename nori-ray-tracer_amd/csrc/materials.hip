// materials.hip -- differentiable materials: the material rows of a scene and
// of a context (nori_scene_materials, nori_gpu_update_materials,
// nori_gpu_materials) and bsdf_eval's adjoint in them, its host statement and
// its device call (nori_scene_bsdf_grad, nori_gpu_bsdf_grad).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "bsdf_desc.h"
#include "bsdf_grad.h"
#include "ctx.h"

namespace nori {
namespace {

// nori_gpu_update_materials (stated in nori_gpu.h): validate, then on the
// context's stream count the non-finite words in use (nothing is modified
// before that count is back) and set the rows into both copies of the table.
int update_materials(nori_gpu_ctx &c, const nori_gpu_materials_desc &md, const float *rows) {
    const char *name = "nori_gpu_update_materials";
    if (c.S.integrator == NORI_INTEGRATOR_PHOTONMAPPER)
        throw NoriException(NORI_ERR_UNSUPPORTED,
                            std::string(name) + ": a photonmapper context (its photon map was traced at creation)");
    if (md.num_bsdfs != c.num_bsdfs)
        throw NoriException(NORI_ERR_INVALID, std::string(name) + ": num_bsdfs " + std::to_string(md.num_bsdfs) +
                                                  " is not the scene's " + std::to_string(c.num_bsdfs));
    for (uint32_t r : md.reserved)
        if (r != 0) throw NoriException(NORI_ERR_INVALID, std::string(name) + ": reserved must be 0");
    if (md.on_device && (uintptr_t)rows % 4)
        throw NoriException(NORI_ERR_INVALID, std::string(name) + ": the device pointer must be 4-byte aligned");
    HIP_TRY(hipSetDevice(c.device));
    if (md.on_device) require_device_ptr(rows, std::string(name) + ": on_device with a pointer that is not device memory");
    const uint32_t nb = c.num_bsdfs;
    if (nb == 0) return NORI_OK;
    const size_t bytes = sizeof(float) * NORI_MATERIAL_FLOATS * (size_t)nb;
    const float *dr = rows;
    if (!md.on_device) {
        c.mat_rows.ensure(bytes);
        HIP_TRY(hipMemcpyAsync(c.mat_rows.p, rows, bytes, hipMemcpyHostToDevice, c.stream));
        dr = c.mat_rows.as<float>();
    }
    // ---- a pass of its own: nothing is modified before its count is back
    c.upd_count.ensure(4);
    HIP_TRY(hipMemsetAsync(c.upd_count.p, 0, 4, c.stream));
    HIP_TRY(launch_materials_count(c.bsdfs.as<DevBsdf>(), dr, nb, c.upd_count.as<uint32_t>(), c.stream));
    uint32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, c.upd_count.p, 4, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    if (bad)
        throw NoriException(NORI_ERR_INVALID, std::string(name) + ": " + std::to_string(bad) +
                                                  " non-finite values in words in use; nothing was changed");
    // ---- the table, and the blob's copy of it (the tail finisher and k_shade stage the blob in LDS)
    DevBsdf *blob = c.S.blob ? reinterpret_cast<DevBsdf *>(c.blob.as<char>() + c.S.off_bsdfs) : nullptr;
    HIP_TRY(launch_materials_set(c.bsdfs.as<DevBsdf>(), blob, dr, nb, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    ++c.materials_version;
    return NORI_OK;
}

int read_materials(nori_gpu_ctx &c, float *rows, uint64_t *version) {
    if (version) *version = c.materials_version;
    if (!rows || c.num_bsdfs == 0) return NORI_OK;
    HIP_TRY(hipSetDevice(c.device));
    HIP_TRY(hipStreamSynchronize(c.stream));
    std::vector<DevBsdf> h(c.num_bsdfs);
    HIP_TRY(hipMemcpy(h.data(), c.bsdfs.p, h.size() * sizeof(DevBsdf), hipMemcpyDeviceToHost));
    for (uint32_t b = 0; b < c.num_bsdfs; ++b) material_row_get(h[b], rows + NORI_MATERIAL_FLOATS * (size_t)b);
    return NORI_OK;
}

// nori_gpu_bsdf_grad: k_bsdf_grad over the caller's elements, for the BSDF
// table as it is now.  Device arrays are checked and used in place; host
// inputs pass through q_surf / sh_in / bg_gout (and the terms back through
// bg_terms) in chunks of whole tiles, at most NORI_QUERY_CHUNK elements where
// that is a tile or more, and the sums are added into the zeroed mat_rows and
// from there to the caller's array at the end.  On the table path the chunks
// continue one set of slabs, so the chunking does not show in the bits.
int bsdf_grad(nori_gpu_ctx &c, const nori_gpu_bsdf_grad_desc &gd, const nori_gpu_surface *surf, const float *wi,
              const float *wo, const float *grad_out, float *grad_materials, float *terms, nori_gpu_stats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    const char *name = "nori_gpu_bsdf_grad";
    HIP_TRY(hipSetDevice(c.device));
    const uint32_t n = gd.n, nb = c.num_bsdfs, ns = (uint32_t)c.hshapes.size();
    if (gd.on_device) {
        const void *all[6] = {surf, wi, wo, grad_out, grad_materials, terms};
        for (const void *p : all)
            if (p) require_device_ptr(p, std::string(name) + ": on_device with a pointer that is not device memory");
    } else {
        for (uint32_t i = 0; i < n; ++i)
            if (surf[i].shape < -1 || surf[i].shape >= (int32_t)ns)
                throw NoriException(NORI_ERR_INVALID, std::string(name) + ": record " + std::to_string(i) +
                                                          " names shape " + std::to_string(surf[i].shape) + " of " +
                                                          std::to_string(ns));
    }
    if (nb == 0) return NORI_OK;
    const uint32_t G = bsdf_grad_slabs(n);
    const size_t row_bytes = sizeof(float) * NORI_MATERIAL_FLOATS * (size_t)nb;
    if (bsdf_grad_table(nb)) c.bg_slabs.ensure(row_bytes * G);
    float *slabs = c.bg_slabs.as<float>();
    c.clock.reset(stats != nullptr);
    auto run = [&](const void *s, const void *a, const void *b, const void *g, uint32_t m, uint32_t first, float *gm,
                   void *tm) {
        c.clock.span(c.stream, kKindShade, [&] {
            return launch_bsdf_grad(c.S, ns, nb, (const float4 *)s, (const float *)a, (const float *)b, (const float4 *)g,
                                    m, first, G, gm, (float4 *)tm, slabs, c.stream);
        });
    };
    auto sum = [&](float *gm) {
        c.clock.span(c.stream, kKindShade, [&] { return launch_bsdf_grad_sum(nb, slabs, G, gm, c.stream); });
    };
    if (gd.on_device) {
        run(surf, wi, wo, grad_out, n, 0, grad_materials, terms);
        sum(grad_materials);
        HIP_TRY(hipStreamSynchronize(c.stream));
        c.clock.collect();
    } else {
        c.mat_rows.ensure(row_bytes);
        HIP_TRY(hipMemsetAsync(c.mat_rows.p, 0, row_bytes, c.stream));
        const uint32_t tile = bsdf_grad_tile();
        uint32_t chunk = query_chunk(std::getenv("NORI_QUERY_CHUNK"));
        chunk = std::max(tile, chunk / tile * tile);  // whole tiles
        chunk = std::min(chunk, (n + tile - 1) / tile * tile);
        c.q_surf.ensure(64 * (size_t)chunk);
        c.sh_in[0].ensure(12 * (size_t)chunk);
        c.sh_in[1].ensure(12 * (size_t)chunk);
        c.bg_gout.ensure(32 * (size_t)chunk);
        if (terms) c.bg_terms.ensure(64 * (size_t)chunk);
        for (uint64_t i0 = 0; i0 < n; i0 += chunk) {
            const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, n - i0);
            HIP_TRY(hipMemcpyAsync(c.q_surf.p, surf + i0, 64 * (size_t)m, hipMemcpyHostToDevice, c.stream));
            HIP_TRY(hipMemcpyAsync(c.sh_in[0].p, wi + 3 * i0, 12 * (size_t)m, hipMemcpyHostToDevice, c.stream));
            HIP_TRY(hipMemcpyAsync(c.sh_in[1].p, wo + 3 * i0, 12 * (size_t)m, hipMemcpyHostToDevice, c.stream));
            HIP_TRY(hipMemcpyAsync(c.bg_gout.p, grad_out + 8 * i0, 32 * (size_t)m, hipMemcpyHostToDevice, c.stream));
            run(c.q_surf.p, c.sh_in[0].p, c.sh_in[1].p, c.bg_gout.p, m, (uint32_t)i0, c.mat_rows.as<float>(),
                terms ? c.bg_terms.p : nullptr);
            if (terms)
                HIP_TRY(hipMemcpyAsync(terms + NORI_MATERIAL_FLOATS * i0, c.bg_terms.p, 64 * (size_t)m,
                                       hipMemcpyDeviceToHost, c.stream));
            HIP_TRY(hipStreamSynchronize(c.stream));
            c.clock.collect();
        }
        sum(c.mat_rows.as<float>());
        std::vector<float> h(NORI_MATERIAL_FLOATS * (size_t)nb);
        HIP_TRY(hipMemcpyAsync(h.data(), c.mat_rows.p, row_bytes, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
        c.clock.collect();
        for (size_t k = 0; k < h.size(); ++k)
            if (h[k] != 0.0f) grad_materials[k] += h[k];
    }
    if (begin_stats(c, t0, stats)) stats->ms_shade = c.clock.ms[kKindShade];  // k_bsdf_grad, k_bsdf_grad_sum
    return NORI_OK;
}

// The scene's BSDF records as nori_gpu_create forms them (image pointers
// aside: an image-textured BSDF has no row), with `materials` set into them.
std::vector<DevBsdf> host_bsdfs(const nori_scene_desc &d, const float *materials) {
    std::vector<DevBsdf> out(d.num_bsdfs);
    for (uint32_t b = 0; b < d.num_bsdfs; ++b) {
        dev_bsdf_from_desc(d.bsdfs[b], out[b]);
        if (materials) material_row_set(out[b], materials + NORI_MATERIAL_FLOATS * (size_t)b);
    }
    return out;
}

}  // namespace
}  // namespace nori

extern "C" {

int nori_scene_materials(const nori_scene_desc *d, float *rows) {
    return guarded([&] {
        if (!d || !rows || (d->num_bsdfs && !d->bsdfs)) return fail(NORI_ERR_INVALID, "null argument");
        const std::vector<DevBsdf> B = host_bsdfs(*d, nullptr);
        for (uint32_t b = 0; b < d->num_bsdfs; ++b) material_row_get(B[b], rows + NORI_MATERIAL_FLOATS * (size_t)b);
        return NORI_OK;
    });
}

// bsdf_eval's adjoint, its statement (nori_gpu.h): the rows are bsdf_grad.h's,
// which k_bsdf_grad compiles too; the sums are float64 per destination, in
// element order.  Everything is formed before anything is written, so a
// refusal leaves the caller's arrays alone.
int nori_scene_bsdf_grad(const nori_scene_desc *d, const float *materials, uint32_t n, const nori_gpu_surface *surf,
                         const float *wi, const float *wo, const float *grad_out, float *grad_materials, float *terms) {
    return guarded([&] {
        if (!d || !surf || !wi || !wo || !grad_out || !grad_materials) return fail(NORI_ERR_INVALID, "null argument");
        for (uint32_t i = 0; i < n; ++i)
            if (surf[i].shape < -1 || surf[i].shape >= (int32_t)d->num_shapes)
                return fail(NORI_ERR_INVALID, "nori_scene_bsdf_grad: record " + std::to_string(i) + " names shape " +
                                                  std::to_string(surf[i].shape) + " of " + std::to_string(d->num_shapes));
        for (uint32_t s = 0; s < d->num_shapes; ++s)
            if (d->shapes[s].bsdf < 0 || (uint32_t)d->shapes[s].bsdf >= d->num_bsdfs)
                return fail(NORI_ERR_INVALID, "shape without a valid bsdf");
        const std::vector<DevBsdf> B = host_bsdfs(*d, materials);
        const size_t nfl = NORI_MATERIAL_FLOATS * (size_t)d->num_bsdfs;
        std::vector<float> tm(NORI_MATERIAL_FLOATS * (size_t)n, 0.0f);
        std::vector<double> acc(nfl, 0.0);
        std::vector<uint8_t> has(nfl, 0);
        for (uint32_t i = 0; i < n; ++i) {
            const nori_gpu_surface &r = surf[i];
            if (r.shape < 0) continue;
            const uint32_t b = (uint32_t)d->shapes[r.shape].bsdf;
            float t[NORI_MATERIAL_FLOATS];
            const float *a = wi + 3 * (size_t)i, *o = wo + 3 * (size_t)i, *g = grad_out + 8 * (size_t)i;
            if (!bsdf_grad_element(B[b], V3{r.ns[0], r.ns[1], r.ns[2]}, r.uv[0], r.uv[1], V3{a[0], a[1], a[2]},
                                   V3{o[0], o[1], o[2]}, g[0], g[1], g[2], g[3], t))
                continue;
            for (int w = 0; w < NORI_MATERIAL_FLOATS; ++w) {
                tm[NORI_MATERIAL_FLOATS * (size_t)i + w] = t[w];
                if (t[w] == 0.0f) continue;
                acc[NORI_MATERIAL_FLOATS * (size_t)b + w] += (double)t[w];
                has[NORI_MATERIAL_FLOATS * (size_t)b + w] = 1;
            }
        }
        for (size_t k = 0; k < nfl; ++k)
            if (has[k]) grad_materials[k] = (float)((double)grad_materials[k] + acc[k]);
        if (terms) std::memcpy(terms, tm.data(), tm.size() * sizeof(float));
        return NORI_OK;
    });
}

int nori_gpu_update_materials(nori_gpu_ctx *c, const nori_gpu_materials_desc *md, const float *rows) {
    return guarded([&] {
        if (!c || !md || !rows) return fail(NORI_ERR_INVALID, "null argument");
        return update_materials(*c, *md, rows);
    });
}

int nori_gpu_materials(nori_gpu_ctx *c, float *rows, uint64_t *version) {
    return guarded([&] {
        if (!c) return fail(NORI_ERR_INVALID, "null argument");
        return read_materials(*c, rows, version);
    });
}

int nori_gpu_bsdf_grad(nori_gpu_ctx *c, const nori_gpu_bsdf_grad_desc *gd, const nori_gpu_surface *surf, const float *wi,
                       const float *wo, const float *grad_out, float *grad_materials, float *terms,
                       nori_gpu_stats *stats) {
    return guarded([&] {
        const char *name = "nori_gpu_bsdf_grad";
        if (!c || !gd || !surf || !wi || !wo || !grad_out || !grad_materials) return fail(NORI_ERR_INVALID, "null argument");
        if (gd->reserved[0] != 0 || gd->reserved[1] != 0) return fail(NORI_ERR_INVALID, std::string(name) + ": reserved must be 0");
        if (gd->on_device && ((uintptr_t)surf % 16 || (uintptr_t)grad_out % 16 || (uintptr_t)grad_materials % 16 ||
                              (uintptr_t)terms % 16))
            return fail(NORI_ERR_INVALID,
                        std::string(name) + ": device surf, grad_out, grad_materials and terms must be 16-byte aligned");
        if (gd->on_device && ((uintptr_t)wi % 4 || (uintptr_t)wo % 4))
            return fail(NORI_ERR_INVALID, std::string(name) + ": device wi and wo must be 4-byte aligned");
        if (gd->n == 0) return NORI_OK;
        return bsdf_grad(*c, *gd, surf, wi, wo, grad_out, grad_materials, terms, stats);
    });
}

}  // extern "C"
