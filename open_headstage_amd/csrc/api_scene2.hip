// api_scene2.hip -- ohs_scene2_* (include/ohs_scene2.h): the scene surface's bodies (api_scene_bodies.inc) under the second library's
// names, plus the blended call and the launch record with its fourth figure.  Linked into libohs_scene2.so only.
#include "../../include/ohs_hip.h"
#include "../../include/ohs_scene2.h"
#include "host_internal.h"

static_assert(OHS_SCENE2_OK == OHS_OK && OHS_SCENE2_ERR_INVALID_ARG == OHS_ERR_INVALID_ARG && OHS_SCENE2_ERR_NO_DEVICE == OHS_ERR_NO_DEVICE &&
              OHS_SCENE2_ERR_HIP == OHS_ERR_HIP && OHS_SCENE2_ERR_ALLOC == OHS_ERR_ALLOC, "ohs_scene2.h restates ohs_hip.h's status codes");

#define OHS_SCENE_T ohs_scene2
#define OHS_SCENE_FN(name) ohs_scene2_##name
#define OHS_SCENE_OWN_LAST_LAUNCH 1
#include "api_scene_bodies.inc"

extern "C" {

int ohs_scene2_process_blended(ohs_scene2 *sc, const float *d_in, float *d_out, size_t n_blocks, size_t in_stream_stride,
                               size_t in_channel_stride, size_t out_stream_stride, size_t out_channel_stride, size_t n_objects,
                               size_t seg_blocks, const unsigned *dir_idx, const float *obj_gain, size_t idx_stride,
                               const unsigned *prev_idx, const float *prev_gain, int switch_mode, void *hip_stream,
                               const unsigned *dir_idx1, const float *weight, const unsigned *prev_idx1, const float *prev_weight)
{
    if (!sc) return scene_null("scene is NULL");
    return ohsint_batch_process_objects_blend(sc->b, d_in, d_out, n_blocks, in_stream_stride, in_channel_stride, out_stream_stride,
                                              out_channel_stride, n_objects, seg_blocks, dir_idx, obj_gain, idx_stride, prev_idx, prev_gain,
                                              switch_mode, hip_stream, dir_idx1, weight, prev_idx1, prev_weight);
}

int ohs_scene2_last_launch(const ohs_scene2 *sc, int *n_pairs, int *ranges_per_stream, unsigned long long *fading_passes,
                           unsigned long long *blended_passes)
{
    if (!sc) return scene_null("scene is NULL");
    return ohsint_batch_last_objects_blend_launch(sc->b, n_pairs, ranges_per_stream, fading_passes, blended_passes);
}

}  // extern "C"
