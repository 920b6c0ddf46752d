/* ohs_scene3.h -- C ABI of libohs_scene3.so: object scenes whose objects stand INSIDE a triangle of three measured directions
 * (k_conv_p1_objects_blend3; DESIGN.md section 4.5k, SCENES.md).
 *
 * A superset of ohs_scene2.h in a library of its own: the older headers and libraries are frozen, and nothing here adds to
 * them.  libohs_scene3.so carries its own copy of the product's code and exports the ohs_scene3_* names below and nothing
 * else.  Fourteen of the fifteen entries are ohs_scene2.h's under the new prefix, with identical contracts -- compiled from the
 * same source --, except that the launch record has a fifth figure; the fifteenth is the three-direction call.  Handles of the
 * libraries do not mix.
 *
 * Conventions are ohs_scene.h's: every function returns a status (0 = ok), the last-error entry gives the thread-local
 * detail of the last failure in THIS library, audio buffers are DEVICE pointers, planar f32, `irs` and every row are HOST
 * pointers that are free again when the call returns.  A handle is used from one thread at a time.  Blocks are 512 frames.
 * Asynchrony is THE STREAM CONTRACT beside ohs_batch_process in ohs_hip.h, for the four calls here that take a hip_stream.
 *
 * Out of scope (none of it is built): four or more directions per object; rows (indices and weights) found on the device
 * -- the caller computes them, e.g. with open_headstage_amd.scene3.triangle_directions, which defines them --; per-sample
 * weight ramps other than the one-block fade; responses beyond one partition (512 taps); in-place calls; a node twin over
 * several GPUs; and the rest of ohs_scene.h's list -- a session-renderer mode over scenes, fades other than one block. */
#ifndef OHS_SCENE3_H
#define OHS_SCENE3_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OHS_SCENE3_OK              0
#define OHS_SCENE3_ERR_INVALID_ARG 1
#define OHS_SCENE3_ERR_NO_DEVICE   2
#define OHS_SCENE3_ERR_HIP         3
#define OHS_SCENE3_ERR_ALLOC       6

#define OHS_SCENE3_MAX_OBJECTS     64
#define OHS_SCENE3_MAX_DIRECTIONS  65536
#define OHS_SCENE3_SWITCH_RING_OUT  0   /* a change takes effect at the segment's first frame; the old response's tail rings out */
#define OHS_SCENE3_SWITCH_CROSSFADE 1   /* ... is faded in over the segment's first block */

typedef struct ohs_scene3 ohs_scene3;

/* ---- the thirteen entries of ohs_scene.h: see that header for each contract ---- */
int ohs_scene3_create(int device, size_t n_streams, size_t num_bands, ohs_scene3 **out);
void ohs_scene3_destroy(ohs_scene3 *sc);
const char *ohs_scene3_status_string(int status);
const char *ohs_scene3_last_error(void);
int ohs_scene3_set_direction_irs(ohs_scene3 *sc, size_t n_dirs, const float *irs, size_t len);
/* one direction per object: ohs_scene.h's process call, bit for bit */
int ohs_scene3_process(ohs_scene3 *sc, const float *d_in, float *d_out, size_t n_blocks, size_t in_stream_stride,
                       size_t in_channel_stride, size_t out_stream_stride, size_t out_channel_stride, size_t n_objects,
                       size_t seg_blocks, const unsigned *dir_idx, const float *obj_gain, size_t idx_stride,
                       const unsigned *prev_idx, const float *prev_gain, int switch_mode, void *hip_stream);
int ohs_scene3_set_gain(ohs_scene3 *sc, float gain);
int ohs_scene3_set_eq_band_coeffs(ohs_scene3 *sc, size_t band, const float coeffs[5], int enabled);
int ohs_scene3_set_eq_enabled(ohs_scene3 *sc, int eq_enable);
int ohs_scene3_set_flush_denormals(ohs_scene3 *sc, int mode);
int ohs_scene3_reset(ohs_scene3 *sc);
int ohs_scene3_sync(ohs_scene3 *sc, void *hip_stream);
/* the most recent launch: ohs_scene.h's three figures; blended_passes -- the passes that loaded FOUR table rows (a pair in
 * which a w1 is not +0.0 and both w2 are); and blended3_passes -- the passes that loaded SIX (a pair in which a w2 is not
 * +0.0).  Passes through old directions are included, each counted by the old entries; both are summed over streams and
 * blocks.  Both 0 behind a call of the one-direction entry, blended3_passes 0 behind the two-direction entry.  Zeros before
 * the first launch.  Refuses any NULL. */
int ohs_scene3_last_launch(const ohs_scene3 *sc, int *n_pairs, int *ranges_per_stream, unsigned long long *fading_passes,
                           unsigned long long *blended_passes, unsigned long long *blended3_passes);

/* ---- two directions per object: ohs_scene2.h's blended call, bit for bit (see that header for the contract) ---- */
int ohs_scene3_process_blended(ohs_scene3 *sc, const float *d_in, float *d_out, size_t n_blocks, size_t in_stream_stride,
                               size_t in_channel_stride, size_t out_stream_stride, size_t out_channel_stride, size_t n_objects,
                               size_t seg_blocks, const unsigned *dir_idx, const float *obj_gain, size_t idx_stride,
                               const unsigned *prev_idx, const float *prev_gain, int switch_mode, void *hip_stream,
                               const unsigned *dir_idx1, const float *weight, const unsigned *prev_idx1, const float *prev_weight);

/* ---- the three-direction call ----
 * The blended call with a third direction index and a second weight per object, stream and segment:
 *   result = EQ(gain * sum over objects c of conv(u(c) h[dir(c)][e] + w1(c) h[dir1(c)][e] + w2(c) h[dir2(c)][e], x[c] * obj_gain(c))),
 *   u = (1.0f - w1) - w2.
 * The twenty-one leading arguments are the blended call's, with its contract (`weight` is w1).  dir_idx2 and weight2 have the
 * shape and the stride rule of dir_idx1 and weight; prev_idx2 and prev_weight2 those of prev_idx1 and prev_weight.
 * dir_idx2 and weight2 are both NULL or both given.  Both NULL: this IS the blended call (prev_idx2, prev_weight2 ignored).
 * Given, they need dir_idx1 and weight.  prev_idx2 / prev_weight2 NULL: the first segment's own entries (read under CROSSFADE
 * only).  w1 >= 0, w2 >= 0 and w1 + w2 <= 1 with the sum formed in f32; -0.0 is accepted (and is not +0.0 below).
 * Arithmetic: per pass u = (1 - w1) - w2 once in f32, then every component of the object's table row as
 *   (u * A[dir] + w1 * A[dir1]) + w2 * A[dir2],
 * three multiplications and two additions, each rounded by itself, in that order.
 * The pass rule -- one choice per pass (a pair of objects; the absent partner of an odd last object counts as +0.0 everywhere):
 *   both objects' w1 and w2 have the bits of +0.0:  the one-direction call's pass, operation for operation (two table rows);
 *   otherwise both w2 have the bits of +0.0:        the blended call's pass, operation for operation (four rows; dir2 is not read);
 *   otherwise:                                      six rows, the arithmetic above for both objects.
 * So a scene whose w2 are all +0.0 has the blended call's bits whatever dir_idx2 and prev_idx2 name and however they move, one
 * whose w1 are +0.0 too has the one-direction call's, and a scene pays for three directions in the pairs that use them only.
 * Everything else is within the project's FFT bar (1e-6 relative RMS) of the rule above.
 * The change rule under CROSSFADE: an object CHANGES when any of these differs from the entry in front: dir; the bits of w1,
 * of w2 or of the gain; dir1, beside a w1 that is not +0.0 on both sides; dir2, beside a w2 that is not +0.0 on both sides.
 * The pair rule, the pass order and the ramps are the one-direction call's; the old half of a fade goes through the old
 * (dir, dir1, dir2, w1, w2, gain).
 * The bits do not depend on where a signal is cut into calls, given prev_* naming what stood in front of each cut, nor on
 * how the library cuts a call into ranges.
 * Refused, each before anything is queued, with nothing written and the handle left as it was: everything the blended call
 * refuses; one of dir_idx2 / weight2 NULL and the other not; dir_idx2 without dir_idx1; an entry of dir_idx2 that would be
 * read, or of prev_idx2, >= n_dirs; a pair (w1, w2) that would be read, or the pair in front of the call, that fails
 * w1 >= 0 && w2 >= 0 && w1 + w2 <= 1 (NaN fails); 6 * n_streams * segments * n_objects > 0x7fffffff. */
int ohs_scene3_process_blended3(ohs_scene3 *sc, const float *d_in, float *d_out, size_t n_blocks, size_t in_stream_stride,
                                size_t in_channel_stride, size_t out_stream_stride, size_t out_channel_stride, size_t n_objects,
                                size_t seg_blocks, const unsigned *dir_idx, const float *obj_gain, size_t idx_stride,
                                const unsigned *prev_idx, const float *prev_gain, int switch_mode, void *hip_stream,
                                const unsigned *dir_idx1, const float *weight, const unsigned *prev_idx1, const float *prev_weight,
                                const unsigned *dir_idx2, const float *weight2, const unsigned *prev_idx2, const float *prev_weight2);

#ifdef __cplusplus
}
#endif
#endif
