// kernel_config.h -- the constants and wave helpers that device code shares
// with the launchers, free of host headers: kernels.h (the launch API) and the
// device headers include it, and so does the hipRTC program of the shade
// kernel (shade_kernel.h), which cannot see <string> or <vector>.
#pragma once
#include "dev_scene.h"

namespace nori {

constexpr int kShadeBlock = 256;   // shade / regen work-group size
#ifndef NORI_SHADE_LDS_MAX
#define NORI_SHADE_LDS_MAX 16384
#endif
constexpr uint32_t kShadeLdsMax = NORI_SHADE_LDS_MAX;  // largest scene blob the shade kernel stages in LDS
// The shade kernels of the full plugin set are compiled without the inline
// shadow rays (S.nee_inline only for basic scenes): with them, C4 3964 and
// C5 4162 against 4000 / 4308 Msamples/s, queue mode both (one box, 2 reps).
// NORI_NEE_FULL=1 compiles them in (NORI_NEE_INLINE=1 then applies there too).
#ifndef NORI_NEE_FULL
#define NORI_NEE_FULL 0
#endif
constexpr bool kNeeFull = NORI_NEE_FULL;

// ------------------------------------------------------------------ wave helpers
ND uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
ND uint32_t rank_in(uint64_t mask) {  // set lanes of `mask` below this lane
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

}  // namespace nori
