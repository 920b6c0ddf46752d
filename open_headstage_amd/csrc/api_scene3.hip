// api_scene3.hip -- ohs_scene3_* (include/ohs_scene3.h): the scene surface's bodies (api_scene_bodies.inc) under the third library's
// names, plus the two- and the three-direction call and the launch record with its fifth figure.  Linked into libohs_scene3.so only.
#include "../../include/ohs_hip.h"
#include "../../include/ohs_scene3.h"
#include "host_internal.h"

static_assert(OHS_SCENE3_OK == OHS_OK && OHS_SCENE3_ERR_INVALID_ARG == OHS_ERR_INVALID_ARG && OHS_SCENE3_ERR_NO_DEVICE == OHS_ERR_NO_DEVICE &&
              OHS_SCENE3_ERR_HIP == OHS_ERR_HIP && OHS_SCENE3_ERR_ALLOC == OHS_ERR_ALLOC, "ohs_scene3.h restates ohs_hip.h's status codes");

#define OHS_SCENE_T ohs_scene3
#define OHS_SCENE_FN(name) ohs_scene3_##name
#define OHS_SCENE_OWN_LAST_LAUNCH 1
#include "api_scene_bodies.inc"

extern "C" {

int ohs_scene3_process_blended(ohs_scene3 *sc, const float *d_in, float *d_out, size_t n_blocks, size_t in_stream_stride,
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

int ohs_scene3_process_blended3(ohs_scene3 *sc, const float *d_in, float *d_out, size_t n_blocks, size_t in_stream_stride,
                                size_t in_channel_stride, size_t out_stream_stride, size_t out_channel_stride, size_t n_objects,
                                size_t seg_blocks, const unsigned *dir_idx, const float *obj_gain, size_t idx_stride,
                                const unsigned *prev_idx, const float *prev_gain, int switch_mode, void *hip_stream,
                                const unsigned *dir_idx1, const float *weight, const unsigned *prev_idx1, const float *prev_weight,
                                const unsigned *dir_idx2, const float *weight2, const unsigned *prev_idx2, const float *prev_weight2)
{
    if (!sc) return scene_null("scene is NULL");
    return ohsint_batch_process_objects_blend3(sc->b, d_in, d_out, n_blocks, in_stream_stride, in_channel_stride, out_stream_stride,
                                               out_channel_stride, n_objects, seg_blocks, dir_idx, obj_gain, idx_stride, prev_idx, prev_gain,
                                               switch_mode, hip_stream, dir_idx1, weight, prev_idx1, prev_weight, dir_idx2, weight2,
                                               prev_idx2, prev_weight2);
}

int ohs_scene3_last_launch(const ohs_scene3 *sc, int *n_pairs, int *ranges_per_stream, unsigned long long *fading_passes,
                           unsigned long long *blended_passes, unsigned long long *blended3_passes)
{
    if (!sc) return scene_null("scene is NULL");
    return ohsint_batch_last_objects_blend3_launch(sc->b, n_pairs, ranges_per_stream, fading_passes, blended_passes, blended3_passes);
}

}  // extern "C"
