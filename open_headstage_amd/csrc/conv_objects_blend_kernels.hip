// conv_objects_blend_kernels.hip -- k_conv_p1_objects_blend: K moving sources per stream, each between TWO directions with a weight
// (ohs_scene2_process_blended, include/ohs_scene2.h; kernels.h: ConvObjectsBlendArgs with four planes).
// The text is conv_objects_body.hpp's, instantiated for two directions; the translation unit is this kernel's own because a kernel
// beside it could change how hipcc allocates it.  What the build gives (hipcc, gfx950; libohs_hip.resources.json, DESIGN.md section
// 4.5i): all 168 VGPRs that three waves per SIMD leave, 102 SGPRs, no scratch.
#include "conv_objects_body.hpp"

namespace ohs {

static_assert(kObjLdsPlanFits, "k_conv_p1_objects_blend: LDS plan");

__global__ __launch_bounds__(64 * kObjWaves, kObjWavesPerSimd) void k_conv_p1_objects_blend(const ConvP1Args A, const ConvObjectsBlendArgs L)
{
    objects_block_loop<2>(A, L);
}

hipError_t launch_conv_p1_objects_blend(const ConvP1Args &args, const ConvObjectsBlendArgs &l, hipStream_t st)
{
    return launch_objects_kernel(k_conv_p1_objects_blend, args, l, st);
}

}  // namespace ohs
