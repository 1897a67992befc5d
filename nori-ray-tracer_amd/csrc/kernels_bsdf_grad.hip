// kernels_bsdf_grad.hip -- differentiable materials on the device: bsdf_eval's
// adjoint in the material rows (k_bsdf_grad, k_bsdf_grad_sum; stated at
// nori_scene_bsdf_grad in nori_gpu.h, the terms are bsdf_grad.h's) and the
// kernels of nori_gpu_update_materials (k_materials_count, k_materials_set).
#include <cstdlib>

#include "bsdf_grad.h"
#include "kernels.h"

namespace nori {

// The reduction.  A million elements land on a few dozen rows of 16 floats, and
// float atomics onto one address serialise (about 200 ns each),
// so the table path issues none: partial sums travel through LDS, registers
// and one slab of global memory per work-group, each written by one thread.
// The elements are cut into tiles of 256 (tile t = elements 256 t ..), and
// work-group j of G takes the tiles t = j (mod G) in ascending order:
//   lane        one element of the tile: its row of 16 terms
//   wave        the ballot loop of k_surface_grad over the BSDF id, made
//               uniform: the group of the first remaining lane's id is summed
//               over the wave (a butterfly in which the other lanes hold
//               zeros; only the words that BSDF uses: 3, 6, 4 or 9), and the
//               group's first lane adds the sums into the wave's own table in
//               LDS.  Groups of one skip the butterfly.
//   work-group  after each tile the waves' tables are summed in wave order,
//               ((W0 + W1) + W2) + W3, and added to the work-group's running
//               sums, which thread i holds for floats 4 i .. 4 i + 3 of the
//               num_bsdfs x 16; at the end they are written as the work-group's
//               slab with plain 16-byte stores
//   grid        k_bsdf_grad_sum: one thread per destination float sums the
//               slabs in slab order and adds the sum to grad_materials once
// Every step's order is a function of the element order and of G alone, and
// G is a function of n alone, so the same inputs give the same bits on every
// call.  A caller's array that arrives in chunks (host arrays) gives those
// bits too: chunks are whole tiles, a chunk's launch is told its first tile
// and G of the whole array, and the work-groups load their running sums from
// the slabs (`carry`) instead of starting at zero.
//
// LDS per work-group of 256: the records' rows 256 x 5 float4 = 20 KiB (as
// load_record<true>: each load instruction of a wave reads one contiguous
// 1 KiB), the packed wi and wo 2 x 3 KiB (three contiguous 1 KiB loads per
// array and tile), and the four waves' tables 4 x K x 64 B.  K =
// NORI_BSDF_GRAD_MAX_TABLE = 64 makes the tables 16 KiB and the whole 42 KiB:
// three work-groups, twelve waves, per CU of 160 KiB -- and the running sums
// one float4 per thread.  Doubling K would take the CU to two work-groups for
// scenes that this renderer does not have (its largest scene has 30 BSDFs);
// above K the atomic form below serves.
constexpr int kBgBlock = 256;
constexpr int kBgWaves = kBgBlock / 64;
constexpr int kBgRecRow = 5;   // float4 per record row in LDS (4 + 1 padding)
constexpr int kBgMaxGrid = 512;
constexpr int kBgTable = NORI_BSDF_GRAD_MAX_TABLE;
static_assert(kBgTable * NORI_MATERIAL_FLOATS / 4 <= kBgBlock, "one float4 of the running sums per thread");

ND float bg_wave_sum(float x) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) x += __shfl_xor(x, s, 64);
    return x;
}

// Elements [0, n) of the arrays are tiles tile0 .. of the caller's whole
// array; gridDim.x = G.  TABLE: the reproducible path (num_bsdfs <= kBgTable;
// `dst` is the slab buffer, G slabs; carry: they hold the earlier chunks'
// sums).  Otherwise `dst` is grad_materials itself and each wave group's
// first lane adds its sums with float atomics.
template <bool TABLE>
__global__ __launch_bounds__(kBgBlock) void k_bsdf_grad(DevScene S, uint32_t num_shapes, uint32_t num_bsdfs,
                                                        const float4 *surf, const float *wi, const float *wo,
                                                        const float4 *gout, uint32_t n, uint32_t tile0, int carry,
                                                        float *dst, float4 *terms) {
    __shared__ float4 rows[kBgBlock * kBgRecRow];
    __shared__ float dirs[2][3 * kBgBlock];
    __shared__ float4 table[TABLE ? kBgWaves * kBgTable * NORI_MATERIAL_FLOATS / 4 : 1];
    constexpr uint32_t kTab4 = kBgTable * NORI_MATERIAL_FLOATS / 4;  // float4 per wave table
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t row4 = num_bsdfs * (NORI_MATERIAL_FLOATS / 4);  // float4 in use of a table, of a slab
    float *mine_tab = reinterpret_cast<float *>(table + (TABLE ? wave * kTab4 : 0));
    float4 *slab = reinterpret_cast<float4 *>(dst) + (size_t)blockIdx.x * row4;
    float4 acc = make_float4(0, 0, 0, 0);
    if constexpr (TABLE) {
        if (carry && tid < row4) acc = slab[tid];
        for (uint32_t i = lane; i < row4; i += 64) table[wave * kTab4 + i] = make_float4(0, 0, 0, 0);
    }
    const uint32_t G = gridDim.x, tiles = (n + kBgBlock - 1) / kBgBlock;
    // the first tile of this launch that is blockIdx.x (mod G), as a local tile index
    for (uint32_t lt = (blockIdx.x + G - tile0 % G) % G; lt < tiles; lt += G) {  // (uniform in the work-group)
        const uint32_t base = lt * kBgBlock;
        const uint32_t left = n - base < (uint32_t)kBgBlock ? n - base : (uint32_t)kBgBlock;
        __syncthreads();  // the last tile's rows are read, the tables zeroed
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t i = j * kBgBlock + tid;
            if (i < 4 * left) rows[(i >> 2) * kBgRecRow + (i & 3)] = surf[4 * (size_t)base + i];
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const uint32_t i = j * kBgBlock + tid;
            if (i < 3 * left) {
                dirs[0][i] = wi[3 * (size_t)base + i];
                dirs[1][i] = wo[3 * (size_t)base + i];
            }
        }
        __syncthreads();

        const uint32_t q = base + tid;
        float t[NORI_MATERIAL_FLOATS];
#pragma unroll
        for (int w = 0; w < NORI_MATERIAL_FLOATS; ++w) t[w] = 0.0f;
        bool live = false;
        uint32_t bid = 0xFFFFFFFFu, words = 0;
        if (q < n) {
            const float4 r2 = rows[tid * kBgRecRow + 2], r3 = rows[tid * kBgRecRow + 3];
            const uint32_t shape = __float_as_uint(r2.w);
            if (shape < num_shapes) {
                const uint32_t b = (uint32_t)S.shapes[shape].bsdf;
                if (b < num_bsdfs) {
                    const DevBsdf &B = S.bsdfs[b];
                    const float4 g = gout[2 * (size_t)q];  // the row's first float4; words 4-7 are never loaded
                    const V3 vi = V3{dirs[0][3 * tid], dirs[0][3 * tid + 1], dirs[0][3 * tid + 2]};
                    const V3 vo = V3{dirs[1][3 * tid], dirs[1][3 * tid + 1], dirs[1][3 * tid + 2]};
                    live = bsdf_grad_element(B, ld3(r2), r3.x, r3.y, vi, vo, g.x, g.y, g.z, g.w, t);
                    bid = b;
                    words = material_words(B.type, B.tex);
                }
            }
            if (terms) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    terms[4 * (size_t)q + j] = make_float4(t[4 * j], t[4 * j + 1], t[4 * j + 2], t[4 * j + 3]);
            }
        }

        // ---- the wave merge: one group per distinct BSDF id among the live lanes
        unsigned long long rem = __ballot(live);
        while (rem) {  // (uniform: rem is the same in every lane)
            const int first = __ffsll((long long)rem) - 1;
            const uint32_t key = (uint32_t)__shfl((int)bid, first, 64);
            const uint32_t use = (uint32_t)__shfl((int)words, first, 64);
            const bool mine = live && bid == key;
            const unsigned long long grp = __ballot(mine);
            rem &= ~grp;
            const bool many = __popcll(grp) > 1;  // (uniform)
            float *out = TABLE ? mine_tab + key * NORI_MATERIAL_FLOATS : dst + (size_t)key * NORI_MATERIAL_FLOATS;
#pragma unroll
            for (int w = 0; w < 13; ++w) {  // (words 13-15 are reserved)
                if (!(use >> w & 1u)) continue;  // (uniform)
                float s = mine ? t[w] : 0.0f;
                if (many) s = bg_wave_sum(s);  // every lane takes part; lanes outside the group hold zeros
                if ((int)lane == first) {
                    if constexpr (TABLE) out[w] += s;
                    else atomicAdd(out + w, s);
                }
            }
        }

        // ---- the work-group merge: the tile's four tables in wave order onto the running sums
        if constexpr (TABLE) {
            __syncthreads();
            if (tid < row4) {
                float4 s = table[tid];
#pragma unroll
                for (int wv = 1; wv < kBgWaves; ++wv) {
                    const float4 a = table[wv * kTab4 + tid];
                    s.x += a.x, s.y += a.y, s.z += a.z, s.w += a.w;
                }
                acc.x += s.x, acc.y += s.y, acc.z += s.z, acc.w += s.w;
#pragma unroll
                for (int wv = 0; wv < kBgWaves; ++wv) table[wv * kTab4 + tid] = make_float4(0, 0, 0, 0);
            }
        }
    }
    if constexpr (TABLE)
        if (tid < row4) slab[tid] = acc;
}

// One thread per destination float: the slabs in slab order, added once.
__global__ __launch_bounds__(kBgBlock) void k_bsdf_grad_sum(const float *slabs, uint32_t num_slabs, uint32_t row_floats,
                                                            float *grad_materials) {
    const uint32_t i = blockIdx.x * kBgBlock + threadIdx.x;
    if (i >= row_floats) return;
    float s = slabs[i];
    for (uint32_t k = 1; k < num_slabs; ++k) s += slabs[(size_t)k * row_floats + i];
    if (s != 0.0f) grad_materials[i] += s;
}

uint32_t bsdf_grad_slabs(uint32_t n) {
    const uint32_t g = (n + kBgBlock - 1) / kBgBlock;
    return g < (uint32_t)kBgMaxGrid ? g : (uint32_t)kBgMaxGrid;
}

bool bsdf_grad_table(uint32_t num_bsdfs) {
    const char *e = std::getenv("NORI_BSDF_GRAD_TABLE");
    return num_bsdfs <= (uint32_t)kBgTable && !(e && e[0] == '0');
}

hipError_t launch_bsdf_grad(const DevScene &S, uint32_t num_shapes, uint32_t num_bsdfs, const float4 *surf,
                            const float *wi, const float *wo, const float4 *grad_out, uint32_t n, uint32_t first,
                            uint32_t slabs_n, float *grad_materials, float4 *terms, float *slabs, hipStream_t st) {
    if (n == 0 || num_bsdfs == 0 || slabs_n == 0) return hipSuccess;
    if (first % kBgBlock) return hipErrorInvalidValue;  // (chunks are whole tiles)
    if (bsdf_grad_table(num_bsdfs))
        hipLaunchKernelGGL(k_bsdf_grad<true>, dim3(slabs_n), dim3(kBgBlock), 0, st, S, num_shapes, num_bsdfs, surf, wi, wo,
                           grad_out, n, first / kBgBlock, first != 0 ? 1 : 0, slabs, terms);
    else
        hipLaunchKernelGGL(k_bsdf_grad<false>, dim3(slabs_n), dim3(kBgBlock), 0, st, S, num_shapes, num_bsdfs, surf, wi,
                           wo, grad_out, n, first / kBgBlock, 0, grad_materials, terms);
    return hipGetLastError();
}
hipError_t launch_bsdf_grad_sum(uint32_t num_bsdfs, const float *slabs, uint32_t slabs_n, float *grad_materials,
                                hipStream_t st) {
    if (num_bsdfs == 0 || slabs_n == 0 || !bsdf_grad_table(num_bsdfs)) return hipSuccess;
    const uint32_t row_floats = num_bsdfs * NORI_MATERIAL_FLOATS;
    hipLaunchKernelGGL(k_bsdf_grad_sum, dim3((row_floats + kBgBlock - 1) / kBgBlock), dim3(kBgBlock), 0, st, slabs, slabs_n,
                       row_floats, grad_materials);
    return hipGetLastError();
}
uint32_t bsdf_grad_tile() { return kBgBlock; }

// ---- nori_gpu_update_materials
// The non-finite floats among the rows' words in use (nothing is modified before this count is back).
__global__ __launch_bounds__(kBgBlock) void k_materials_count(const DevBsdf *bsdfs, const float *rows, uint32_t num_bsdfs,
                                                              uint32_t *count) {
    const uint32_t i = blockIdx.x * kBgBlock + threadIdx.x;
    if (i >= num_bsdfs * NORI_MATERIAL_FLOATS) return;
    const DevBsdf &B = bsdfs[i / NORI_MATERIAL_FLOATS];
    const float x = rows[i];
    if ((material_words(B.type, B.tex) >> (i % NORI_MATERIAL_FLOATS) & 1u) && !(x - x == 0.0f)) atomicAdd(count, 1u);
}
// One thread per BSDF: the row set into the record (material_row_set: the
// host's own routine), written to the table and, where the scene has one, to
// the blob's copy.
__global__ __launch_bounds__(kBgBlock) void k_materials_set(DevBsdf *bsdfs, DevBsdf *blob_bsdfs, const float *rows,
                                                            uint32_t num_bsdfs) {
    const uint32_t b = blockIdx.x * kBgBlock + threadIdx.x;
    if (b >= num_bsdfs) return;
    DevBsdf B = bsdfs[b];
    float row[NORI_MATERIAL_FLOATS];
    for (int w = 0; w < NORI_MATERIAL_FLOATS; ++w) row[w] = rows[(size_t)b * NORI_MATERIAL_FLOATS + w];
    material_row_set(B, row);
    bsdfs[b] = B;
    if (blob_bsdfs) blob_bsdfs[b] = B;
}

hipError_t launch_materials_count(const DevBsdf *bsdfs, const float *rows, uint32_t num_bsdfs, uint32_t *count,
                                  hipStream_t st) {
    if (num_bsdfs == 0) return hipSuccess;
    const uint32_t m = num_bsdfs * NORI_MATERIAL_FLOATS;
    hipLaunchKernelGGL(k_materials_count, dim3((m + kBgBlock - 1) / kBgBlock), dim3(kBgBlock), 0, st, bsdfs, rows,
                       num_bsdfs, count);
    return hipGetLastError();
}
hipError_t launch_materials_set(DevBsdf *bsdfs, DevBsdf *blob_bsdfs, const float *rows, uint32_t num_bsdfs,
                                hipStream_t st) {
    if (num_bsdfs == 0) return hipSuccess;
    hipLaunchKernelGGL(k_materials_set, dim3((num_bsdfs + kBgBlock - 1) / kBgBlock), dim3(kBgBlock), 0, st, bsdfs,
                       blob_bsdfs, rows, num_bsdfs);
    return hipGetLastError();
}

}  // namespace nori
