// kernels_surface_grad.hip -- the hit record's adjoint in the vertex positions
// and normals: k_surface_grad and its launcher (nori_gpu_surface_grad, stated
// at nori_scene_surface_grad in nori_gpu.h; the terms are surface_grad.h's).
#include "kernels.h"
#include "surface_grad.h"

namespace nori {

// One lane per hit: the 16-byte hit is read directly (a wave's 1 KiB is
// contiguous), the 32-byte ray and the 64-byte gradient record come through
// LDS -- every load instruction of a wave reads one contiguous 1 KiB, and the
// lanes then take their rows, padded to three and five float4 so that the
// 16-byte reads spread over the banks (k_surface<true>'s layout, reversed).
//
// The adds.  Float atomics onto one address serialise (about 200 ns each,
// DESIGN.md D20), and this renderer's usual input lands a million hits on a
// few dozen triangles, so everything that shares a destination is summed on
// chip before an atomic leaves the CU, in two steps.
// In the wave: the loop takes the first remaining contributing lane's
// primitive id, made uniform, ballots the lanes that carry it, and -- where
// there is more than one -- reduces their terms over the wave (a butterfly in
// which the other lanes hold zeros); the first lane of the group keeps the
// sums.  A group of one costs a ballot and no reduction.
// In the work-group: the groups' first lanes append (id, vertex ids, sums) to
// a list in the LDS the rows have left; where the list is short (at most
// kGradMergeMax entries: the waves found much to merge, so the work-group
// will too), entry j's thread sums the later entries with its id unless an
// earlier one carries it, and adds.  A long list means mostly different
// triangles: each first lane adds its own sums, in one pass of atomics, so a
// wave of 64 different triangles issues each atomic instruction once.
constexpr int kGradBlock = 512;
constexpr int kGradRayRow = 3;   // float4 per ray row in LDS (2 + 1 padding)
constexpr int kGradRecRow = 5;   // float4 per record row in LDS (4 + 1 padding)
constexpr uint32_t kGradMergeMax = 128;  // list entries up to which the work-group merges

ND float wave_sum(float x) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) x += __shfl_xor(x, s, 64);
    return x;
}

ND void add3(float *dst, uint32_t vtx, V3 g) {
    float *d = dst + 3 * (size_t)vtx;
    atomicAdd(d, g.x);
    atomicAdd(d + 1, g.y);
    atomicAdd(d + 2, g.z);
}

template <bool NORM>
__global__ __launch_bounds__(kGradBlock) void k_surface_grad(DevScene S, uint32_t V, const float4 *rays, const float4 *hits,
                                                             const float4 *grec, uint32_t n, float *gpos, float *gnrm) {
    __shared__ float4 lds[kGradBlock * (kGradRayRow + kGradRecRow)];
    __shared__ uint32_t count;
    float4 *ray_rows = lds, *rec_rows = lds + kGradBlock * kGradRayRow;
    if (threadIdx.x == 0) count = 0;
    const uint32_t base = blockIdx.x * kGradBlock;  // first hit of the block
    const uint32_t q = base + threadIdx.x;
    const uint32_t left = n - base < (uint32_t)kGradBlock ? n - base : (uint32_t)kGradBlock;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const uint32_t i = j * kGradBlock + threadIdx.x;
        if (i < 2 * left) ray_rows[(i >> 1) * kGradRayRow + (i & 1)] = rays[2 * (size_t)base + i];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t i = j * kGradBlock + threadIdx.x;
        if (i < 4 * left) rec_rows[(i >> 2) * kGradRecRow + (i & 3)] = grec[4 * (size_t)base + i];
    }
    __syncthreads();

    bool live = false;      // the lane holds terms to add
    bool with_n = false;    // ... and normal terms among them
    uint32_t prim = 0xFFFFFFFFu, i0 = 0, i1 = 0, i2 = 0;
    V3 tp[3] = {}, tn[3] = {};
    if (q < n) {
        const float4 hit = hits[q];
        prim = __float_as_uint(hit.y);
        if (prim < S.num_prims) {
            const DevShape &sh = S.shapes[S.prim_shape[prim]];
            if (sh.type != NORI_SHAPE_SPHERE) {
                const uint32_t *f = S.tri_vidx + 3 * (size_t)prim;
                i0 = f[0], i1 = f[1], i2 = f[2];
                if (i0 < V && i1 < V && i2 < V) {
                    const float4 ro = ray_rows[threadIdx.x * kGradRayRow], rd = ray_rows[threadIdx.x * kGradRayRow + 1];
                    const float4 *g = rec_rows + threadIdx.x * kGradRecRow;
                    const float4 ga = g[0], gb = g[1], gc = g[2];
                    const V3 g_ng = ld3(gb), g_ns = ld3(gc);
                    live = surface_grad_positions(ld3(S.pos[i0]), ld3(S.pos[i1]), ld3(S.pos[i2]), ld3(ro), ld3(rd), hit.x,
                                                  hit.z, hit.w, ld3(ga), ga.w, sh.has_normals ? g_ng : g_ng + g_ns, tp);
                    if constexpr (NORM)
                        if (live && sh.has_normals && !sh.nmap)
                            with_n = surface_grad_normals(ld3(S.nrm[i0]), ld3(S.nrm[i1]), ld3(S.nrm[i2]), hit.z, hit.w, g_ns, tn);
                }
            }
        }
    }
    if (!live) tp[0] = tp[1] = tp[2] = V3{0.0f, 0.0f, 0.0f};
    if (!with_n) tn[0] = tn[1] = tn[2] = V3{0.0f, 0.0f, 0.0f};

    // ---- the wave merge: one group per distinct primitive id among the live lanes
    const uint32_t lane = threadIdx.x & 63u;
    bool emit = false;  // the first lane of its group: adds the group's sums
    unsigned long long rem = __ballot(live);
    while (rem) {  // (uniform: rem is the same in every lane)
        const int first = __ffsll((long long)rem) - 1;
        const uint32_t key = (uint32_t)__shfl((int)prim, first, 64);
        const bool mine = live && prim == key;
        const unsigned long long grp = __ballot(mine);
        rem &= ~grp;
        if (__popcll(grp) > 1) {  // (uniform)
            // every lane takes part in the butterfly; lanes outside the group hold zeros
            V3 sp[3], sn[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                sp[k].x = wave_sum(mine ? tp[k].x : 0.0f);
                sp[k].y = wave_sum(mine ? tp[k].y : 0.0f);
                sp[k].z = wave_sum(mine ? tp[k].z : 0.0f);
            }
            bool any_n = false;
            if constexpr (NORM) {
                any_n = __ballot(mine && with_n) != 0ull;  // (uniform)
                if (any_n) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        sn[k].x = wave_sum(mine ? tn[k].x : 0.0f);
                        sn[k].y = wave_sum(mine ? tn[k].y : 0.0f);
                        sn[k].z = wave_sum(mine ? tn[k].z : 0.0f);
                    }
                }
            }
            if ((int)lane == first) {
#pragma unroll
                for (int k = 0; k < 3; ++k) tp[k] = sp[k];
                if constexpr (NORM)
                    if (any_n) {
#pragma unroll
                        for (int k = 0; k < 3; ++k) tn[k] = sn[k];
                        with_n = true;
                    }
            }
        }
        if ((int)lane == first) emit = true;
    }
    // ---- the work-group merge: the rows are read, their LDS becomes the list
    constexpr int kEnt = NORM ? 23 : 13;  // words per entry: id, three vertex ids, 9 (+ 9) sums (+ flag); odd: no bank pattern
    static_assert(kGradBlock * kEnt * 4 <= (int)sizeof(lds), "the list fits the rows' LDS");
    uint32_t *ent = reinterpret_cast<uint32_t *>(lds);
    __syncthreads();
    if (emit) {
        uint32_t *e = ent + atomicAdd(&count, 1u) * kEnt;
        e[0] = prim, e[1] = i0, e[2] = i1, e[3] = i2;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            e[4 + 3 * k] = __float_as_uint(tp[k].x), e[5 + 3 * k] = __float_as_uint(tp[k].y), e[6 + 3 * k] = __float_as_uint(tp[k].z);
            if constexpr (NORM)
                e[13 + 3 * k] = __float_as_uint(tn[k].x), e[14 + 3 * k] = __float_as_uint(tn[k].y), e[15 + 3 * k] = __float_as_uint(tn[k].z);
        }
        if constexpr (NORM) e[22] = with_n ? 1u : 0u;
    }
    __syncthreads();
    const uint32_t cnt = count;
    if (cnt <= kGradMergeMax) {  // (uniform)
        const uint32_t j = threadIdx.x;
        if (j >= cnt) return;
        const uint32_t *e = ent + j * kEnt;
        const uint32_t key = e[0];
        for (uint32_t k = 0; k < j; ++k)
            if (ent[k * kEnt] == key) return;  // an earlier entry adds this triangle
        float sum[kEnt - 4];
#pragma unroll
        for (int w = 0; w < kEnt - 4; ++w) sum[w] = __uint_as_float(e[4 + w]);
        uint32_t any_n = NORM ? e[kEnt - 1] : 0u;
        for (uint32_t k = j + 1; k < cnt; ++k) {
            const uint32_t *o = ent + k * kEnt;
            if (o[0] != key) continue;
#pragma unroll
            for (int w = 0; w < (NORM ? 18 : 9); ++w) sum[w] += __uint_as_float(o[4 + w]);
            if constexpr (NORM) any_n |= o[22];
        }
        i0 = e[1], i1 = e[2], i2 = e[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            tp[k] = V3{sum[3 * k], sum[3 * k + 1], sum[3 * k + 2]};
            if constexpr (NORM) tn[k] = V3{sum[9 + 3 * k], sum[10 + 3 * k], sum[11 + 3 * k]};
        }
        with_n = any_n != 0u;
    } else if (!emit) {
        return;
    }
    add3(gpos, i0, tp[0]);
    add3(gpos, i1, tp[1]);
    add3(gpos, i2, tp[2]);
    if constexpr (NORM) {
        if (with_n) {
            add3(gnrm, i0, tn[0]);
            add3(gnrm, i1, tn[1]);
            add3(gnrm, i2, tn[2]);
        }
    }
}

hipError_t launch_surface_grad(const DevScene &S, uint32_t num_vertices, const float4 *rays, const float4 *hits,
                               const float4 *grad_surf, uint32_t n, float *grad_positions, float *grad_normals,
                               hipStream_t st) {
    if (n == 0) return hipSuccess;
    const dim3 g((n + kGradBlock - 1) / kGradBlock), b(kGradBlock);
    if (grad_normals)
        hipLaunchKernelGGL(k_surface_grad<true>, g, b, 0, st, S, num_vertices, rays, hits, grad_surf, n, grad_positions,
                           grad_normals);
    else
        hipLaunchKernelGGL(k_surface_grad<false>, g, b, 0, st, S, num_vertices, rays, hits, grad_surf, n, grad_positions,
                           (float *)nullptr);
    return hipGetLastError();
}

}  // namespace nori
