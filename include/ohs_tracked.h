/* ohs_tracked.h -- C ABI of libohs_tracked.so: the three-direction scene call with its rows FOUND, SEALED AND RENDERED ON THE DEVICE, on
 * one stream -- sources and head poses in, two ears out (k_lookup_tri_cells, k_lookup_tri_rest, k_scene_rows_seal,
 * k_conv_p1_objects_blend3; DESIGN.md section 4.5n, SCENES.md).
 *
 * A library of its own: the older headers and libraries are frozen, and nothing here adds to them.  libohs_tracked.so carries its
 * own copy of the product's code and of the pruned lookup's kernels and exports the ohs_tracked_* names below and nothing else.
 * Handles of the libraries do not mix.
 *
 * THE RESULT IS DEFINED BY COMPOSITION.  ohs_tracked_process has, bit for bit, the output of
 *     ohs_lookup3p_rows(src, rot ...)  ->  (idx0, idx1, idx2, w1, w2)                                     (include/ohs_lookup3p.h)
 *     ohs_scene3_process_blended3(..., those rows, obj_gain, prev_* = the previous call's last segment)   (include/ohs_scene3.h)
 * on handles with the same table, mesh, EQ, gain and flush mode.  What differs is where the rows live: they never leave the
 * device.  The lookup writes the five row planes where the convolution kernel reads them; k_scene_rows_seal, the device form of
 * the scene call's host scan, builds the planes in front of the call, gathers the call's last segment for the next call and counts
 * the launch record's passes.
 *
 * Conventions are ohs_scene3.h's: every function returns a status (0 = ok; ohs_hip.h's OHS_* codes, restated below), the last-error
 * entry gives the thread-local detail of the last failure in THIS library, audio buffers are DEVICE pointers, planar f32, every
 * other array is a HOST pointer that is free again when the call returns.  A handle is used from one thread at a time.  Blocks
 * are 512 frames.  Asynchrony is THE STREAM CONTRACT beside ohs_batch_process in ohs_hip.h for ohs_tracked_process and
 * ohs_tracked_sync; one handle serves one signal, so consecutive calls go to one stream, or to streams the caller has ordered.
 *
 * Out of scope (none of it is built): tracked forms of the one- and two-direction calls; rows supplied by the caller as device
 * pointers; one row for all streams (ohs_scene3.h's idx_stride = 0); a session renderer over scenes; a node twin over several
 * GPUs; and the rest of ohs_scene3.h's and ohs_lookup3p.h's lists. */
#ifndef OHS_TRACKED_H
#define OHS_TRACKED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OHS_TRACKED_OK              0
#define OHS_TRACKED_ERR_INVALID_ARG 1
#define OHS_TRACKED_ERR_NO_DEVICE   2
#define OHS_TRACKED_ERR_HIP         3
#define OHS_TRACKED_ERR_ALLOC       6

#define OHS_TRACKED_MAX_OBJECTS     64
#define OHS_TRACKED_MAX_DIRECTIONS  65536
#define OHS_TRACKED_MAX_TRIANGLES   131072
#define OHS_TRACKED_MAX_MAGNITUDE   1e15   /* of any source coordinate or matrix element, as in ohs_lookup3p.h */
#define OHS_TRACKED_MAX_GRID        256
#define OHS_TRACKED_SWITCH_RING_OUT  0     /* ohs_scene3.h's switch modes */
#define OHS_TRACKED_SWITCH_CROSSFADE 1
#define OHS_TRACKED_FRESH            0     /* no boundary at the call's start: ohs_scene3.h's prev_* == NULL */
#define OHS_TRACKED_CARRY            1     /* in front of the call stands the last segment of the handle's previous call */

typedef struct ohs_tracked ohs_tracked;

/* ohs_scene3_create's handle (device, n_streams, num_bands) and ohs_lookup3p_create's table and mesh (n_dirs, xyz, n_tris, tris,
 * grid) in one.  The triangles' inverses, the certificate's bound and the cube-map index are computed here, on the host, exactly
 * as ohs_lookup3p_create computes them, and go to the device once.  Refuses what either of the two refuses, the singular
 * triangle in ohs_lookup3p_create's words.  *out is NULL after a failure. */
int ohs_tracked_create(int device, size_t n_streams, size_t num_bands, size_t n_dirs, const float *xyz, size_t n_tris,
                       const uint32_t *tris, unsigned grid, ohs_tracked **out);
/* NULL is allowed.  Waits for what the handle has queued. */
void ohs_tracked_destroy(ohs_tracked *tr);
const char *ohs_tracked_status_string(int status);
const char *ohs_tracked_last_error(void);

/* ---- ohs_scene3.h's entries of the same names, with their contracts ---- */
/* The direction table; the call needs one with at least the mesh's n_dirs rows (row i is measurement i of xyz). */
int ohs_tracked_set_direction_irs(ohs_tracked *tr, size_t n_dirs, const float *irs, size_t len);
int ohs_tracked_set_gain(ohs_tracked *tr, float gain);
int ohs_tracked_set_eq_band_coeffs(ohs_tracked *tr, size_t band, const float coeffs[5], int enabled);
int ohs_tracked_set_eq_enabled(ohs_tracked *tr, int eq_enable);
int ohs_tracked_set_flush_denormals(ohs_tracked *tr, int mode);
/* ohs_scene3_reset, and the carried rows are dropped: the next call is OHS_TRACKED_FRESH. */
int ohs_tracked_reset(ohs_tracked *tr);
int ohs_tracked_sync(ohs_tracked *tr, void *hip_stream);

/* ---- the call ----
 * d_in [stream][n_objects][n_blocks * 512] and d_out [stream][2][n_blocks * 512] with their strides, seg_blocks and switch_mode:
 * ohs_scene3_process_blended3's.  src, src_stream_stride, src_seg_stride, rot, rot_stream_stride: ohs_lookup3p_rows', with its
 * layout and stride rules (src f64 [..][n_objects][3], a stride of 0 shares the entry; rot f64 3 x 3 per stream and segment, or
 * NULL: no rotation), over the call's segments = ceil(n_blocks / seg_blocks).  obj_gain: f32 [stream][segment][n_objects], packed,
 * or NULL: 1.0.  carry: OHS_TRACKED_CARRY or OHS_TRACKED_FRESH.
 * Asynchronous on hip_stream.  On return src, rot and obj_gain have been checked and copied to pinned staging and are the
 * caller's again; d_in and d_out are ordered on the stream.  Staging goes through a ring of four slots guarded by events: with
 * four calls of a handle in flight the fifth waits, on the host, for the first.  Device and pinned memory grow to the largest call
 * seen and are then reused (growing waits for the device).
 * On the stream, in order: sources, poses and gains up (the gains straight into the gain plane); per chunk of 2^18 queries the
 * lookup's two passes, writing into the five row planes at the chunk's offset, with a fallback counter per chunk; k_scene_rows_seal;
 * k_conv_p1_objects_blend3 on the planes; the EQ.  Rows are per stream.
 * k_scene_rows_seal: the planes in front of the call [6][stream][n_objects] (idx0, idx1, idx2, w1, w2, gain) are the carried rows
 * under CARRY and the first segment's own entries under FRESH, the gain plane reading 1.0 where obj_gain is NULL; this call's last
 * segment is gathered into the handle's OTHER carry buffer (the convolution still reads the old one); and the launch record is
 * counted by ohs_scene3.h's rules -- under CROSSFADE an object changes on idx0, on the bits of w1, w2 or the gain, on idx1 beside
 * a w1 that is not +0.0 on both sides, on idx2 beside such a w2; a pair fades when either object changes; blended_passes and
 * blended3_passes count the segment's blocks per current pass and one per fading old pass.
 * n_blocks == 0: nothing is queued, the carried rows stay.
 * Refused, each before anything is queued, with nothing written and the handle left as it was: a NULL handle, d_in, d_out or src;
 * n_objects outside 1 .. 64; seg_blocks == 0; a switch_mode or carry that is neither of its two values; n_blocks > 2^24; strides
 * smaller than the processed regions, or regions that overlap; a coordinate or matrix element that is not finite or above 1e15 in
 * magnitude; src_stream_stride neither 0 nor >= (segments - 1) * src_seg_stride + 1; rot_stream_stride neither 0 nor >= segments;
 * 6 * n_streams * segments * n_objects > 0x7fffffff; no direction table, or one with fewer rows than the mesh's n_dirs (the
 * convolution kernel trusts its indices: this is what keeps a lookup result inside the table); OHS_TRACKED_CARRY with no carried
 * rows, or with carried rows of another n_objects; a handle that failed in the middle of an earlier call (ohs_tracked_reset). */
int ohs_tracked_process(ohs_tracked *tr, const float *d_in, float *d_out, size_t n_blocks, size_t in_stream_stride,
                        size_t in_channel_stride, size_t out_stream_stride, size_t out_channel_stride, size_t n_objects,
                        size_t seg_blocks, const double *src, size_t src_stream_stride, size_t src_seg_stride, const double *rot,
                        size_t rot_stream_stride, const float *obj_gain, int switch_mode, int carry, void *hip_stream);

/* The most recent call that queued work: ohs_scene3_last_launch's five figures and, sixth, how many of the call's queries the
 * lookup's pass 2 answered (ohs_lookup3p_last_launch's fallback_queries).  Waits for that call if it has not finished, then
 * reads the device's counters.  Zeros before the first call.  Refuses any NULL. */
int ohs_tracked_last_launch(ohs_tracked *tr, int *n_pairs, int *ranges_per_stream, unsigned long long *fading_passes,
                            unsigned long long *blended_passes, unsigned long long *blended3_passes,
                            unsigned long long *fallback_queries);

/* The five row planes of the most recent call that queued work, copied to host arrays [stream][segment][n_objects] each: what was
 * rendered.  SYNCHRONOUS: waits for that call.  Refuses any NULL, and a handle that has made no such call. */
int ohs_tracked_rows(ohs_tracked *tr, uint32_t *idx0, uint32_t *idx1, uint32_t *idx2, float *w1, float *w2);

#ifdef __cplusplus
}
#endif
#endif
