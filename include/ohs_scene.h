/* ohs_scene.h -- C ABI of libohs_scene.so: object scenes, K independently moving sources per stream rendered to two ears
 * in one kernel (k_conv_p1_objects; DESIGN.md section 4.5h, SCENES.md).
 *
 * A library of its own beside libohs_hip.so, with a handle type of its own: include/ohs_hip.h and the exported surface of
 * libohs_hip.so are frozen, and nothing here adds to them.  libohs_scene.so carries its own copy of the product's code and
 * exports the ohs_scene_* names below and nothing else; an ohs_scene owns a batch object of that copy, which is never
 * handed out.  Handles of the two libraries do not mix.
 *
 * Conventions are ohs_hip.h's: every function returns a status (0 = ok; the values are ohs_hip.h's OHS_* codes, restated
 * below), ohs_scene_last_error() is the thread-local detail of the last failure in THIS library, audio buffers are DEVICE
 * pointers, planar f32, `irs` and every row are HOST pointers that are free again when the call returns.  A handle is used
 * from one thread at a time.  Blocks are 512 frames.  What "asynchronous on hip_stream" promises -- input produced on the stream,
 * buffers reusable on the stream and rows on return, which calls may wait on the host (the fifth call in flight) -- is THE STREAM
 * CONTRACT beside ohs_batch_process in ohs_hip.h; tests/test_gpu_stream_order.py holds this library's calls to it.
 *
 * Out of scope (none of it is built): a session-renderer mode over scenes; interpolation between two directions per
 * object (an object takes the table's entry it names); responses beyond one partition (512 taps); in-place calls; a
 * node twin over several GPUs; fades other than one block. */
#ifndef OHS_SCENE_H
#define OHS_SCENE_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OHS_SCENE_OK              0
#define OHS_SCENE_ERR_INVALID_ARG 1
#define OHS_SCENE_ERR_NO_DEVICE   2
#define OHS_SCENE_ERR_HIP         3
#define OHS_SCENE_ERR_ALLOC       6

#define OHS_SCENE_MAX_OBJECTS     64
#define OHS_SCENE_MAX_DIRECTIONS  65536
#define OHS_SCENE_SWITCH_RING_OUT  0    /* a change of direction or gain takes effect at the segment's first frame; the old response's tail rings out */
#define OHS_SCENE_SWITCH_CROSSFADE 1    /* ... is faded in over the segment's first block */

typedef struct ohs_scene ohs_scene;

/* n_streams listeners (1 .. 2^20) on `device`, an EQ of num_bands bands (<= 64; all disabled) behind the renderer, gain 1.
 * Refuses out == NULL; OHS_SCENE_ERR_NO_DEVICE when no GPU is usable.  *out is NULL after a failure. */
int ohs_scene_create(int device, size_t n_streams, size_t num_bands, ohs_scene **out);
/* NULL is allowed.  The caller has waited for the handle's work (ohs_scene_sync). */
void ohs_scene_destroy(ohs_scene *sc);
const char *ohs_scene_status_string(int status);
const char *ohs_scene_last_error(void);

/* The direction table: irs[n_dirs][2][len], direction d -> left ear irs[d][0], right ear irs[d][1]; 1 <= len <= 512,
 * 1 <= n_dirs <= 65536 (8 KiB of device memory per direction).  Replaces any earlier table and zeroes every stream's overlap;
 * n_dirs == 0 frees the table (irs, len ignored).  Waits for the device.  Refuses sc == NULL, irs == NULL, len 0 or > 512,
 * n_dirs > 65536: the handle keeps the table and the overlap it had.
 * Bits: a pair of objects on directions (a, b) is convolved with the table entries a layout of ohs_hip.h builds for the same
 * four responses, bit for bit, as long as the spectra stay in f32's normal range. */
int ohs_scene_set_direction_irs(ohs_scene *sc, size_t n_dirs, const float *irs, size_t len);

/* n_blocks * 512 frames of every stream's n_objects input channels -> two ears, out of place:
 *   in  (s, c, i) at d_in [s * in_stream_stride  + c * in_channel_stride  + i], c < n_objects (further channels are never read)
 *   out (s, e, i) at d_out[s * out_stream_stride + e * out_channel_stride + i], e = 0 left, 1 right
 *   result = EQ(gain * sum over objects c of conv(h[dir(c)][e], x[c] * obj_gain(c))), the EQ if it is enabled.
 * Segment k = blocks [k seg_blocks, (k + 1) seg_blocks) of the call (seg_blocks is clamped to n_blocks); n_segs of them.
 * dir_idx and obj_gain hold [stream][segment][n_objects] 32-bit entries: object c of stream s in segment k reads entry
 * [(s * idx_stride + k) * n_objects + c].  idx_stride == 0: one row [segment][n_objects] for all streams, and prev_* hold
 * n_objects entries; else idx_stride >= n_segs, and prev_* hold [n_streams][n_objects].  obj_gain == NULL: 1.0 everywhere.
 * prev_idx / prev_gain: what stood in front of the call's first block (read under CROSSFADE only); NULL: the first segment's
 * own entries, i.e. the call's start is no boundary for the indices / the gains.
 * CROSSFADE: an object CHANGES in the first block of a segment when its index, or its gain's bits, differ from the entry in
 * front; a PAIR of objects (2 p, 2 p + 1) fades when either changes.  In that block a fading pair's frames go
 * (x * gain_old) * g[n] through the old two directions and (x * gain_cur) * f[n] through the current ones, f[n] = n / 512,
 * g[n] = (512 - n) / 512; every other pair's frames go x * gain_cur through the current directions.  RING_OUT: nothing fades.
 * State: the 512-frame overlap per stream (and the EQ's), nothing else -- the bits do not depend on where a signal is cut
 * into calls, given prev_* naming what stood in front of each cut, nor on how the library cuts a call into ranges.
 * Bits: with no change anywhere and obj_gain NULL or 1.0 a block has the bits of ohs_batch_process_layout on
 * irs[c] = directions[dir(c)]; a block in which EVERY pair fades, gains 1.0, has the bits of the fading block of
 * ohs_batch_process_layout_scheduled.  Elsewhere the result is within the project's FFT bar (1e-6 relative RMS) of the rule
 * above.  Asynchronous on hip_stream (NULL: the default stream); obeys the handle's flush-denormals mode.
 * n_blocks == 0: a no-op (after the argument checks).  Refused, each before anything is queued and with the handle left as
 * it was: a NULL sc, d_in, d_out or dir_idx; n_objects 0 or > 64; seg_blocks 0; a switch_mode other than the two; no table;
 * n_blocks > 2^24; idx_stride in 1 .. n_segs - 1; an entry of dir_idx that would be read, or of prev_idx, >= n_dirs; strides
 * smaller than the processed region; input and output regions that overlap.  A HIP failure marks the handle failed: every
 * later call returns OHS_SCENE_ERR_HIP until ohs_scene_reset. */
int ohs_scene_process(ohs_scene *sc, const float *d_in, float *d_out, size_t n_blocks, size_t in_stream_stride,
                      size_t in_channel_stride, size_t out_stream_stride, size_t out_channel_stride, size_t n_objects,
                      size_t seg_blocks, const unsigned *dir_idx, const float *obj_gain, size_t idx_stride,
                      const unsigned *prev_idx, const float *prev_gain, int switch_mode, void *hip_stream);

/* the output gain (applied at the kernel's store, in front of the EQ).  Refuses sc == NULL. */
int ohs_scene_set_gain(ohs_scene *sc, float gain);
/* band `band` (< num_bands) of the EQ behind the renderer: coeffs = {b0, b1, b2, a1, a2} / a0.  Refuses NULL, band out of range. */
int ohs_scene_set_eq_band_coeffs(ohs_scene *sc, size_t band, const float coeffs[5], int enabled);
int ohs_scene_set_eq_enabled(ohs_scene *sc, int eq_enable);
/* 0: IEEE denormals, 1: flush (renderer and EQ alike; see ohs_engine_set_flush_denormals).  Refuses NULL, other modes. */
int ohs_scene_set_flush_denormals(ohs_scene *sc, int mode);
/* zeroes every stream's overlap and EQ state (table, EQ bands, gain kept): the next call has a new handle's bits.  Also the
 * way back from a failed handle. */
int ohs_scene_reset(ohs_scene *sc);
/* waits (host side) for everything queued on hip_stream */
int ohs_scene_sync(ohs_scene *sc, void *hip_stream);
/* the most recent launch: pairs of objects, block ranges per stream (1, 2, 4, 8 or 16; every range but the first runs one dry
 * block in front), and the passes through OLD directions summed over streams and segments.  Zeros before the first launch.
 * Refuses any NULL. */
int ohs_scene_last_launch(const ohs_scene *sc, int *n_pairs, int *ranges_per_stream, unsigned long long *fading_passes);

#ifdef __cplusplus
}
#endif
#endif
