/* ohs_scene2.h -- C ABI of libohs_scene2.so: object scenes whose objects stand BETWEEN two measured directions
 * (k_conv_p1_objects_blend; DESIGN.md section 4.5i, SCENES.md).
 *
 * A superset of ohs_scene.h in a library of its own: include/ohs_scene.h and libohs_scene.so are frozen as ohs_hip.h and
 * libohs_hip.so are, and nothing here adds to them.  libohs_scene2.so carries its own copy of the product's code and exports
 * the ohs_scene2_* names below and nothing else.  Thirteen of the fourteen entries are ohs_scene.h's under the new prefix, with
 * identical contracts -- compiled from the same source --, except that the launch record has a fourth figure; the fourteenth is
 * the blended call.  Handles of the three libraries do not mix.
 *
 * Conventions are ohs_scene.h's: every function returns a status (0 = ok), the last-error entry gives the thread-local
 * detail of the last failure in THIS library, audio buffers are DEVICE pointers, planar f32, `irs` and every row are HOST
 * pointers that are free again when the call returns.  A handle is used from one thread at a time.  Blocks are 512 frames.
 * Asynchrony is THE STREAM CONTRACT beside ohs_batch_process in ohs_hip.h, for the three calls here that take a hip_stream.
 *
 * Out of scope (none of it is built): three or more directions per object; per-sample weight ramps other than the
 * one-block fade; and the rest of ohs_scene.h's list -- a session-renderer mode over scenes, responses beyond one partition
 * (512 taps), in-place calls, a node twin over several GPUs, fades other than one block. */
#ifndef OHS_SCENE2_H
#define OHS_SCENE2_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OHS_SCENE2_OK              0
#define OHS_SCENE2_ERR_INVALID_ARG 1
#define OHS_SCENE2_ERR_NO_DEVICE   2
#define OHS_SCENE2_ERR_HIP         3
#define OHS_SCENE2_ERR_ALLOC       6

#define OHS_SCENE2_MAX_OBJECTS     64
#define OHS_SCENE2_MAX_DIRECTIONS  65536
#define OHS_SCENE2_SWITCH_RING_OUT  0   /* a change takes effect at the segment's first frame; the old response's tail rings out */
#define OHS_SCENE2_SWITCH_CROSSFADE 1   /* ... is faded in over the segment's first block */

typedef struct ohs_scene2 ohs_scene2;

/* ---- the thirteen entries of ohs_scene.h: see that header for each contract ---- */
int ohs_scene2_create(int device, size_t n_streams, size_t num_bands, ohs_scene2 **out);
void ohs_scene2_destroy(ohs_scene2 *sc);
const char *ohs_scene2_status_string(int status);
const char *ohs_scene2_last_error(void);
int ohs_scene2_set_direction_irs(ohs_scene2 *sc, size_t n_dirs, const float *irs, size_t len);
/* one direction per object: ohs_scene.h's process call, bit for bit */
int ohs_scene2_process(ohs_scene2 *sc, const float *d_in, float *d_out, size_t n_blocks, size_t in_stream_stride,
                       size_t in_channel_stride, size_t out_stream_stride, size_t out_channel_stride, size_t n_objects,
                       size_t seg_blocks, const unsigned *dir_idx, const float *obj_gain, size_t idx_stride,
                       const unsigned *prev_idx, const float *prev_gain, int switch_mode, void *hip_stream);
int ohs_scene2_set_gain(ohs_scene2 *sc, float gain);
int ohs_scene2_set_eq_band_coeffs(ohs_scene2 *sc, size_t band, const float coeffs[5], int enabled);
int ohs_scene2_set_eq_enabled(ohs_scene2 *sc, int eq_enable);
int ohs_scene2_set_flush_denormals(ohs_scene2 *sc, int mode);
int ohs_scene2_reset(ohs_scene2 *sc);
int ohs_scene2_sync(ohs_scene2 *sc, void *hip_stream);
/* the most recent launch: ohs_scene.h's three figures, and blended_passes -- the passes that loaded FOUR table rows (a pair in
 * which a weight is not +0.0), passes through old directions included, summed over streams and blocks.  0 behind a call of
 * the one-direction entry.  Zeros before the first launch.  Refuses any NULL. */
int ohs_scene2_last_launch(const ohs_scene2 *sc, int *n_pairs, int *ranges_per_stream, unsigned long long *fading_passes,
                           unsigned long long *blended_passes);

/* ---- the blended call ----
 * The one-direction call with a second direction index and a weight per object, stream and segment:
 *   result = EQ(gain * sum over objects c of conv((1 - w(c)) h[dir(c)][e] + w(c) h[dir1(c)][e], x[c] * obj_gain(c))).
 * The seventeen leading arguments are the one-direction call's, with its contract.  dir_idx1 and weight have the shape and
 * the stride rule of dir_idx and obj_gain (entry [(s * idx_stride + k) * n_objects + c]); prev_idx1 and prev_weight those of
 * prev_idx and prev_gain.
 * dir_idx1 and weight are both NULL or both given.  Both NULL: this IS the one-direction call (prev_idx1, prev_weight ignored).
 * prev_idx1 / prev_weight NULL: the first segment's own entries, i.e. the call's start is no boundary for them (read under
 * CROSSFADE only).  0 <= w <= 1; -0.0 is accepted (and blends: it is not +0.0).
 * CROSSFADE: an object CHANGES when its index, its weight's bits or its gain's bits differ from the entry in front, or when
 * its second index does and its weight is not +0.0 on both sides.  (A second index beside a weight of +0.0 in the entry in
 * front AND in the current one is never read, so it changes nothing: an object that is not blended fades exactly where the
 * one-direction call fades it.)  The pair rule, the pass order and the ramps are the one-direction call's; the old half of
 * a fade goes through the old (dir, dir1, w, gain).
 * Arithmetic: per pass u = 1 - w once in f32, then every component of the object's table row as u * A[dir] + w * A[dir1],
 * two multiplications and one addition, each rounded by itself: w = 0 gives A[dir] and w = 1 gives A[dir1] exactly.
 * Bits: a pair of objects whose weights are all +0.0 (old and current ones in a fading block) has the bits the one-direction
 * call gives on dir_idx, whatever dir_idx1 and prev_idx1 name and however they move (the change rule above) -- a scene that
 * blends nothing has that call's bits and its fading_passes, one that blends some of its pairs pays for those only.  Everything else is within the project's FFT bar (1e-6 relative RMS) of the rule above.
 * The bits do not depend on where a signal is cut into calls, given prev_* naming what stood in front of each cut, nor on
 * how the library cuts a call into ranges.
 * Refused, each before anything is queued and with the handle left as it was: everything the one-direction call refuses;
 * one of dir_idx1 / weight NULL and the other not; an entry of dir_idx1 that would be read, or of prev_idx1, >= n_dirs; a
 * weight that would be read, or an entry of prev_weight, outside [0, 1] or NaN. */
int ohs_scene2_process_blended(ohs_scene2 *sc, const float *d_in, float *d_out, size_t n_blocks, size_t in_stream_stride,
                               size_t in_channel_stride, size_t out_stream_stride, size_t out_channel_stride, size_t n_objects,
                               size_t seg_blocks, const unsigned *dir_idx, const float *obj_gain, size_t idx_stride,
                               const unsigned *prev_idx, const float *prev_gain, int switch_mode, void *hip_stream,
                               const unsigned *dir_idx1, const float *weight, const unsigned *prev_idx1, const float *prev_weight);

#ifdef __cplusplus
}
#endif
#endif
