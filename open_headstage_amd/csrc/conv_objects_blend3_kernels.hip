// conv_objects_blend3_kernels.hip -- k_conv_p1_objects_blend3: K moving sources per stream, each inside a triangle of THREE
// directions with two weights (ohs_scene3_process_blended3, include/ohs_scene3.h; kernels.h: ConvObjectsBlendArgs with six planes).
// The text is conv_objects_body.hpp's, instantiated for three directions; the translation unit is this kernel's own because a
// kernel beside it could change how hipcc allocates its 168 VGPRs.  What the build gives is in libohs_hip.resources.json and
// no scratch, no AGPRs, three waves per SIMD.
#include "conv_objects_body.hpp"

namespace ohs {

static_assert(kObjLdsPlanFits, "k_conv_p1_objects_blend3: LDS plan");

__global__ __launch_bounds__(64 * kObjWaves, kObjWavesPerSimd) void k_conv_p1_objects_blend3(const ConvP1Args A, const ConvObjectsBlendArgs L)
{
    objects_block_loop<3>(A, L);
}

hipError_t launch_conv_p1_objects_blend3(const ConvP1Args &args, const ConvObjectsBlendArgs &l, hipStream_t st)
{
    return launch_objects_kernel(k_conv_p1_objects_blend3, args, l, st);
}

}  // namespace ohs
