// kernels_shade.hip -- the ahead-of-time instantiations of k_shade
// (shade_kernel.h) and launch_shade, which launches the scene's own
// compilation of the kernel (rtc.hip) where the context holds one.
#include <algorithm>

#include "kernels.h"
#include "shade_kernel.h"

namespace nori {

template <int INTEG, int VAR>
static void shade_dispatch(const DevScene &S, const PathQueue &in, const PathQueue &out, const ShadowQueue &sq,
                           const SegState &seg, int in_sel, const WorkDesc &wd, float4 *rec, Counters *C,
                           uint32_t lds, uint32_t nseg, hipStream_t st) {
    dim3 g(nseg), b(kShadeBlock);  // nseg segments from wd.b0 (wd.G counts the whole pool)
    // the shadow-ray slots overlay the blob, dead once the vertices are shaded
    const uint32_t dyn = S.nee_inline ? std::max(lds, kNeeSlotBytes) : lds;
    const ShadeArgs a{S, in, out, sq, seg, in_sel, wd, rec, C, lds};
    if (lds) hipLaunchKernelGGL((k_shade<INTEG, true, VAR>), g, b, dyn, st, a);
    else hipLaunchKernelGGL((k_shade<INTEG, false, VAR>), g, b, dyn, st, a);
}
template <int INTEG>
static void shade_dispatch(const DevScene &S, const PathQueue &in, const PathQueue &out, const ShadowQueue &sq,
                           const SegState &seg, int in_sel, const WorkDesc &wd, float4 *rec, Counters *C,
                           uint32_t lds, uint32_t nseg, hipStream_t st) {
    if (S.basic) shade_dispatch<INTEG, 0>(S, in, out, sq, seg, in_sel, wd, rec, C, lds, nseg, st);
    else if (S.chroma) shade_dispatch<INTEG, 2>(S, in, out, sq, seg, in_sel, wd, rec, C, lds, nseg, st);
    else shade_dispatch<INTEG, 1>(S, in, out, sq, seg, in_sel, wd, rec, C, lds, nseg, st);
}
// rtc: the scene's own compilation of its kernel (rtc.hip), launched in place
// of the instantiation below when it is the one this launch would pick -- the
// same grid, block, dynamic LDS and argument block as shade_dispatch.
hipError_t launch_shade(const DevScene &S, const PathQueue &in, const PathQueue &out, const ShadowQueue &sq,
                        const SegState &seg, int in_sel, const WorkDesc &wd, float4 *rec, Counters *C,
                        uint32_t nseg, hipStream_t st, const ShadeRtc *rtc) {
    if (nseg == 0 || wd.b0 + nseg > wd.G) return hipErrorInvalidValue;
    const uint32_t lds = shade_lds_bytes(S.blob_bytes);
    if (rtc && rtc->shade && S.basic && rtc->integrator == shade_integrator(S.integrator) && rtc->lds == (lds != 0)) {
        const uint32_t dyn = S.nee_inline ? std::max(lds, kNeeSlotBytes) : lds;
        ShadeArgs a{S, in, out, sq, seg, in_sel, wd, rec, C, lds};
        void *params[] = {&a};
        return hipModuleLaunchKernel(rtc->shade, nseg, 1, 1, kShadeBlock, 1, 1, dyn, st, params, nullptr);
    }
    switch (S.integrator) {
    case NORI_INTEGRATOR_PATH_MATS:
        shade_dispatch<NORI_INTEGRATOR_PATH_MATS>(S, in, out, sq, seg, in_sel, wd, rec, C, lds, nseg, st);
        break;
    case NORI_INTEGRATOR_VOLUMETRIC:
        shade_dispatch<NORI_INTEGRATOR_VOLUMETRIC>(S, in, out, sq, seg, in_sel, wd, rec, C, lds, nseg, st);
        break;
    default: shade_dispatch<NORI_INTEGRATOR_PATH_MIS>(S, in, out, sq, seg, in_sel, wd, rec, C, lds, nseg, st); break;
    }
    return hipGetLastError();
}

}  // namespace nori
