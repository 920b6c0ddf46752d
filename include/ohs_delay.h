/* ohs_delay.h -- C ABI of libohs_delay.so: OBJECT DISTANCE.  A propagation delay and a gain per object, stream and segment, both moving
 * linearly per sample inside a segment (that is what makes Doppler), applied on the device in front of a scene call (k_object_delay,
 * k_delay_history; DESIGN.md section 4.5o, SCENES.md).
 *
 * A library of its own: it links none of the product's code, exports the ohs_delay_* names below and nothing else, and its handle
 * mixes with no other library's.  The stage is linear and acts per object, so it composes with every scene entry and with
 * ohs_tracked_process: ohs_delay_process writes [stream][K][frames], a scene call on the same stream takes that buffer as its d_in.
 * Nothing of the older headers and libraries changes.
 *
 * Conventions: every function returns a status (0 = ok; the values are ohs_hip.h's OHS_* codes, restated below),
 * ohs_delay_last_error() is the thread-local detail of the last failure in THIS library.  Audio buffers are DEVICE pointers, planar
 * f32; every other array is a HOST pointer that is the caller's again when the call returns.  Blocks are 512 frames.  A handle is
 * used from one thread at a time.  Asynchrony is THE STREAM CONTRACT beside ohs_batch_process in ohs_hip.h for ohs_delay_process and
 * ohs_delay_sync; one handle serves one signal, so consecutive calls go to one stream, or to streams the caller has ordered.
 *
 * THE ARITHMETIC.  Every operation is rounded by itself (no fused multiply-add), in the order written.  A call is cut into segments
 * of seg_blocks * 512 frames; the last one may be short, and L is the frames it has.  A segment's row (D, G) is the delay in frames
 * and the gain REACHED AT ITS LAST FRAME; (D', G') is what stands in front of it: the previous segment's row, or for the first
 * segment what `carry` says.  For frame j (0 .. L - 1) of a segment, frame n of the stream:
 *   f64:  a  = (double)(j + 1) / (double)L
 *         d  = D' + (D - D') * a ;   d = min(max(d, 1), max_delay)
 *         i  = floor(d) ;            f = (float)(d - i)
 *         gd = (double)G' + ((double)G - (double)G') * a ;   g = (float)gd
 *   f32:  fm1 = f - 1 ;  fm2 = f - 2 ;  fp1 = f + 1
 *         c_-1 = ((f   * fm1) * fm2) * (-1/6 as the nearest f32, -0x1.555556p-3)
 *         c_0  = ((fp1 * fm1) * fm2) *  0.5f
 *         c_1  = ((fp1 * f  ) * fm2) * -0.5f
 *         c_2  = ((fp1 * f  ) * fm1) * ( 1/6 as the nearest f32)
 *         y[n] = g * (((c_-1 * x[n-i+1] + c_0 * x[n-i]) + c_1 * x[n-i-1]) + c_2 * x[n-i-2])
 * Four-point Lagrange interpolation on the nodes -1, 0, 1, 2.  The minimum delay is one frame, so the tap x[n-i+1] is causal.
 * Frames in front of the stream's start read as 0.  f may round to 1.0f (d just below a whole number): c_1 is then exactly 1 and
 * the others are zeros, which picks x[n-i-1], the next tap, exactly.  At f = 0 it is c_0 that is 1: a delay of exactly 1 with a gain
 * of 1 gives a finite input one frame late, value for value (a zero sample may leave with the other sign: the three zero products
 * are added to it).  Behind a call, what stands in front of the next one is the last row's (D, G) as GIVEN, not the d and g computed
 * at its last frame.  There is no flush mode: subnormals pass as IEEE 754 has them, and a NaN or an infinity in the input makes the
 * four outputs that read it NaN or infinite (0 * inf is NaN).
 *
 * Out of scope (none of it is built): the stage fused into the scene kernels; air absorption or any other filter that depends on
 * distance; delays below one frame; interpolators other than this cubic; a session-renderer mode. */
#ifndef OHS_DELAY_H
#define OHS_DELAY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OHS_DELAY_OK              0
#define OHS_DELAY_ERR_INVALID_ARG 1
#define OHS_DELAY_ERR_NO_DEVICE   2
#define OHS_DELAY_ERR_HIP         3
#define OHS_DELAY_ERR_ALLOC       6

#define OHS_DELAY_MAX_OBJECTS     64
#define OHS_DELAY_MAX_DELAY       65536
#define OHS_DELAY_MAX_STREAMS     65535
#define OHS_DELAY_FRESH           0     /* in front of the call: its first row's own values (no ramp) over a silent history */
#define OHS_DELAY_CARRY           1     /* in front of the call: the (D, G) and the input history the previous call left */

typedef struct ohs_delay ohs_delay;

/* n_streams of 1 .. 65535, max_objects of 1 .. 64, max_delay of 1 .. 65536 frames.  Per stream and object the handle keeps the last
 * max_delay + 2 input frames (a ring, [n_streams][max_objects][max_delay + 2] f32, allocated HERE and zeroed) and the last (D, G).
 * OHS_DELAY_ERR_NO_DEVICE when no GPU is usable.  *out is NULL after a failure. */
int ohs_delay_create(int device, size_t n_streams, size_t max_objects, size_t max_delay, ohs_delay **out);
/* NULL is allowed.  Waits for what the handle has queued. */
void ohs_delay_destroy(ohs_delay *dl);
const char *ohs_delay_status_string(int status);
const char *ohs_delay_last_error(void);

/* ---- the call ----
 * d_in [stream][n_objects][n_blocks * 512] at d_in[s * in_stream_stride + c * in_channel_stride + n], as the scene calls read it;
 * d_out in the same shape with its own two strides (in floats).  The segments are ceil(n_blocks / seg_blocks).
 * delay: f64, frames, 1 <= delay <= max_delay, at delay[(s * row_stream_stride + k) * n_objects + c] for stream s, segment k, object c;
 * row_stream_stride is in segments: >= the call's segments, or 0 -- one row [segment][n_objects] for all streams.  gain: f32 in the
 * same layout, or NULL: 1.0.  carry: OHS_DELAY_CARRY or OHS_DELAY_FRESH.
 * Asynchronous on hip_stream.  On return delay and gain have been checked and copied to pinned staging and are the caller's again;
 * d_in and d_out are ordered on the stream.  Staging goes through a ring of four slots guarded by events: with four calls of a
 * handle in flight the fifth waits, on the host, for the first.  A slot holds 16 segments' rows from the start (8 MiB at the most) and grows
 * to the largest call seen (growing waits for the device).
 * On the stream, in order: the rows up; k_object_delay; k_delay_history, which moves the call's last max_delay + 2 frames (all of
 * them, if it has fewer) into the ring -- a launch of its own behind the kernel that reads the ring, so calls shorter than the
 * history chain as long ones do.
 * n_blocks == 0: nothing is queued, history and carry stay.
 * Refused with OHS_DELAY_ERR_INVALID_ARG, each before anything is queued, with nothing written and the handle left as it was: a NULL
 * handle, d_in, d_out or delay; d_out == d_in, or the two regions overlapping anywhere; n_objects of 0 or above max_objects;
 * seg_blocks == 0; n_blocks > 2^24; a carry that is neither of its two values; OHS_DELAY_CARRY on a handle that carries nothing
 * (none yet, or ohs_delay_reset), or whose previous call had another n_objects; strides smaller than the processed regions;
 * row_stream_stride neither 0 nor >= the segments; a delay that is not finite or outside [1, max_delay]; a gain that is not finite;
 * a handle that failed in the middle of an earlier call (ohs_delay_reset). */
int ohs_delay_process(ohs_delay *dl, const float *d_in, float *d_out, size_t n_blocks, size_t in_stream_stride,
                      size_t in_channel_stride, size_t out_stream_stride, size_t out_channel_stride, size_t n_objects,
                      size_t seg_blocks, const double *delay, const float *gain, size_t row_stream_stride, int carry,
                      void *hip_stream);

/* Zeroes the history and drops the carry: the stream starts again from silence.  Waits for the whole device first. */
int ohs_delay_reset(ohs_delay *dl);
/* Waits for everything queued on hip_stream. */
int ohs_delay_sync(ohs_delay *dl, void *hip_stream);

/* The most recent call that queued work: the frames of a tile, the widest input window a tile stages in LDS, and the tiles that
 * took each form -- staged in LDS, or their four taps gathered from global memory.  Waits for that call if it has not finished, then
 * reads the device's counters.  Zero tiles before the first call.  Refuses any NULL. */
int ohs_delay_last_launch(ohs_delay *dl, unsigned *tile_frames, unsigned *lds_window, unsigned long long *lds_tiles,
                          unsigned long long *gather_tiles);

/* What the handle holds as (D', G') for an OHS_DELAY_CARRY call: delay[n_streams][n_objects] and gain likewise, n_objects the
 * previous call's, written to *n_objects (0, and nothing else written, when nothing is carried).  Host state: it waits for
 * nothing.  Refuses any NULL. */
int ohs_delay_carried(const ohs_delay *dl, size_t *n_objects, double *delay, float *gain);

#ifdef __cplusplus
}
#endif
#endif
