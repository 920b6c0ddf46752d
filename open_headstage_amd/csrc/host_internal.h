// host_internal.h -- host-side helpers shared between the translation units of libohs_hip.so (not part
// of the public header).
#pragma once

#include <stddef.h>

#include <vector>

extern "C" void ohsint_set_error(const char *msg);     // api_core.hip: feeds ohs_last_error()
struct ohs_batch;
struct ohs_sofa;
// api_batch.hip: ohs_batch_set_ir with the impulse response already in memory of the batch's device
extern "C" int ohsint_batch_set_ir_device(ohs_batch *b, int path, const float *d_ir, size_t len);
// api_batch.hip: what libohs_scene.so's entries (api_scene.hip, include/ohs_scene.h) call on the batch object a scene owns -- the
// direction table, the scene call (K moving sources per stream -> two ears, then the layout call's epilogue) and its launch record
extern "C" int ohsint_batch_set_object_dirs(ohs_batch *b, size_t n_dirs, const float *irs, size_t len);
extern "C" int ohsint_batch_process_objects(ohs_batch *b, const float *d_in, float *d_out, size_t n_blocks, size_t in_stream_stride,
                                            size_t in_channel_stride, size_t out_stream_stride, size_t out_channel_stride,
                                            size_t n_objects, size_t seg_blocks, const unsigned *dir_idx, const float *obj_gain,
                                            size_t idx_stride, const unsigned *prev_idx, const float *prev_gain, int switch_mode,
                                            void *hip_stream);
extern "C" int ohsint_batch_last_objects_launch(const ohs_batch *b, int *n_pairs, int *ranges_per_stream,
                                                unsigned long long *fading_passes);
// api_batch.hip: what libohs_scene2.so adds (api_scene2.hip, include/ohs_scene2.h) -- the scene call with a second direction and a
// weight per object (dir_idx1 and weight both NULL: ohsint_batch_process_objects), and the launch record with its blended passes
extern "C" int ohsint_batch_process_objects_blend(ohs_batch *b, const float *d_in, float *d_out, size_t n_blocks, size_t in_stream_stride,
                                                  size_t in_channel_stride, size_t out_stream_stride, size_t out_channel_stride,
                                                  size_t n_objects, size_t seg_blocks, const unsigned *dir_idx, const float *obj_gain,
                                                  size_t idx_stride, const unsigned *prev_idx, const float *prev_gain, int switch_mode,
                                                  void *hip_stream, const unsigned *dir_idx1, const float *weight,
                                                  const unsigned *prev_idx1, const float *prev_weight);
extern "C" int ohsint_batch_last_objects_blend_launch(const ohs_batch *b, int *n_pairs, int *ranges_per_stream,
                                                      unsigned long long *fading_passes, unsigned long long *blended_passes);
// api_batch.hip: what libohs_scene3.so adds (api_scene3.hip, include/ohs_scene3.h) -- the scene call with a third direction and a
// second weight per object (dir_idx2 and weight2 both NULL: ohsint_batch_process_objects_blend), and the launch record with its
// six-row passes
extern "C" int ohsint_batch_process_objects_blend3(ohs_batch *b, const float *d_in, float *d_out, size_t n_blocks, size_t in_stream_stride,
                                                   size_t in_channel_stride, size_t out_stream_stride, size_t out_channel_stride,
                                                   size_t n_objects, size_t seg_blocks, const unsigned *dir_idx, const float *obj_gain,
                                                   size_t idx_stride, const unsigned *prev_idx, const float *prev_gain, int switch_mode,
                                                   void *hip_stream, const unsigned *dir_idx1, const float *weight,
                                                   const unsigned *prev_idx1, const float *prev_weight, const unsigned *dir_idx2,
                                                   const float *weight2, const unsigned *prev_idx2, const float *prev_weight2);
extern "C" int ohsint_batch_last_objects_blend3_launch(const ohs_batch *b, int *n_pairs, int *ranges_per_stream,
                                                       unsigned long long *fading_passes, unsigned long long *blended_passes,
                                                       unsigned long long *blended3_passes);

namespace ohs_host {

// biquad 0.4.2 Coefficients::<f32>::from_params restated; out = {b0, b1, b2, a1, a2} / a0.
// Returns an OHS_* status (OHS_ERR_OUTSIDE_NYQUIST, OHS_ERR_NEGATIVE_Q, OHS_ERR_INVALID_ARG).
int rbj(int type, float fs, float fc, float q, float gain_db, float out[5]);

// speakers.cpp: the four impulse responses [Lsl, Lsr, Rsl, Rsr] of two virtual speakers at the plugin's angles
// (degrees, azimuth positive to the right), optionally resampled to fs
int speaker_irs(const struct ::ohs_sofa *sofa, float az_l, float el_l, float az_r, float el_r, float radius_m, float fs,
                std::vector<float> out[4]);

}  // namespace ohs_host
