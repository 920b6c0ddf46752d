/* ohs_delay2.h -- C ABI of libohs_delay2.so: OBJECT DISTANCE WITH AIR ABSORPTION.  ohs_delay.h's stage -- a propagation delay and a gain
 * per object, stream and segment, both moving linearly per sample inside a segment -- and, fused into it, a short symmetric FIR per
 * object, stream and segment whose taps move per sample in the same way: the dulling of the treble by which the ear judges distance
 * (k_object_delay2, k_delay2_history; DESIGN.md section 4.5p, SCENES.md).  The taps come from the caller: the library carries no
 * acoustics (open_headstage_amd.air_absorption_taps supplies the atmospheric law).
 *
 * A library of its own: it links none of the product's code and none of libohs_delay.so's, exports the ohs_delay2_* names below and
 * nothing else, and its handle mixes with no other library's.  It composes with the scene calls as ohs_delay.h says of its own.
 * Nothing of the older headers and libraries changes.
 *
 * Conventions: ohs_delay.h's.  Every function returns a status (0 = ok; ohs_hip.h's OHS_* codes, restated below),
 * ohs_delay2_last_error() is the thread-local detail of the last failure in THIS library.  Audio buffers are DEVICE pointers, planar
 * f32; every other array is a HOST pointer that is the caller's again when the call returns.  Blocks are 512 frames.  A handle is
 * used from one thread at a time.  Asynchrony is THE STREAM CONTRACT beside ohs_batch_process in ohs_hip.h for the two process calls
 * and ohs_delay2_sync; one handle serves one signal.
 *
 * THE ARITHMETIC.  Every operation is rounded by itself (no fused multiply-add), in the order written.  A call is cut into segments
 * of seg_blocks * 512 frames; the last one may be short, and L is the frames it has.  A segment's row (D, G, H_0 .. H_4) is the delay
 * in frames, the gain and the FIR's taps REACHED AT ITS LAST FRAME; (D', G', H'_0 .. H'_4) is what stands in front of it: the previous
 * segment's row, or for the first segment what `carry` says.  H_0 is the centre and H_1 .. H_4 one side of a symmetric filter of
 * 2 R + 1 = 9 taps, R = OHS_DELAY2_FIR_RADIUS = 4.
 *
 * THE PASS is chosen per segment row (stream, segment, object), so it is the same for every frame of the row.
 *   PLAIN, when H' and H are both the identity (1.0f, +0, +0, +0, +0) by their bits -- and throughout ohs_delay2_process --: frame by
 *   frame ohs_delay.h's arithmetic, with its clamp of d at 1 and its bits.  A non-finite input spreads to the four outputs that read
 *   it, as ohs_delay.h says.
 *   FILTERED, every other row.  For frame j (0 .. L - 1) of the segment, frame n of the stream:
 *   f64:  a  = (double)(j + 1) / (double)L
 *         d  = D' + (D - D') * a ;   d = min(max(d, 1 + R), max_delay)         (the lower clamp is 5, not 1: D' + (D - D') * a can
 *                                                                               round one ulp below both ends)
 *         i  = floor(d) ;            f = (float)(d - i)
 *         gd = (double)G' + ((double)G - (double)G') * a ;   g = (float)gd
 *         h_r = (float)((double)H'_r + ((double)H_r - (double)H'_r) * a)        for r = 0 .. 4
 *   f32:  fm1 = f - 1 ;  fm2 = f - 2 ;  fp1 = f + 1
 *         c_-1 = ((f   * fm1) * fm2) * (-1/6 as the nearest f32, -0x1.555556p-3)
 *         c_0  = ((fp1 * fm1) * fm2) *  0.5f
 *         c_1  = ((fp1 * f  ) * fm2) * -0.5f
 *         c_2  = ((fp1 * f  ) * fm1) * ( 1/6 as the nearest f32)
 *         m = n - i + 1, and for each node t of m, m - 1, m - 2, m - 3:
 *         v(t) = ((((h_0 * x[t] + h_1 * (x[t-1] + x[t+1])) + h_2 * (x[t-2] + x[t+2])) + h_3 * (x[t-3] + x[t+3])) + h_4 * (x[t-4] + x[t+4]))
 *         y[n] = g * (((c_-1 * v(m) + c_0 * v(m-1)) + c_1 * v(m-2)) + c_2 * v(m-3))
 * The filter first, on the four nodes, then ohs_delay.h's four-point Lagrange interpolation between them.  The newest sample read is
 * x[n-i+5], causal because i >= 5; the oldest is x[n-i-6]: twelve distinct inputs, x[m-7 .. m+4], per output, and a history of
 * max_delay + 2 + R frames.  Frames in front of the stream's start read as 0.  A non-finite input makes the twelve outputs that read
 * it non-finite.  Behind a call, what stands in front of the next one is the last row's (D, G, H) as GIVEN; behind ohs_delay2_process
 * the taps in front of the next call are the identity.  There is no flush mode.
 *
 * Out of scope (none of it is built): taps beyond radius 4; IIR absorption; filtering below 5 frames of delay; the stage fused into
 * the scene kernels; interpolators other than the cubic; a session-renderer mode. */
#ifndef OHS_DELAY2_H
#define OHS_DELAY2_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OHS_DELAY2_OK              0
#define OHS_DELAY2_ERR_INVALID_ARG 1
#define OHS_DELAY2_ERR_NO_DEVICE   2
#define OHS_DELAY2_ERR_HIP         3
#define OHS_DELAY2_ERR_ALLOC       6

#define OHS_DELAY2_MAX_OBJECTS     64
#define OHS_DELAY2_MAX_DELAY       65536
#define OHS_DELAY2_MAX_STREAMS     65535
#define OHS_DELAY2_FIR_RADIUS      4     /* R: a row has R + 1 = 5 taps, the centre and one side of 2 R + 1 */
#define OHS_DELAY2_FRESH           0     /* in front of the call: its first row's own values, taps included (no ramp), over a silent history */
#define OHS_DELAY2_CARRY           1     /* in front of the call: the (D, G, H) and the input history the previous call left */

typedef struct ohs_delay2 ohs_delay2;

/* n_streams of 1 .. 65535, max_objects of 1 .. 64, max_delay of 1 .. 65536 frames.  Per stream and object the handle keeps the last
 * max_delay + 2 + R input frames (a ring, [n_streams][max_objects][max_delay + 6] f32, allocated HERE and zeroed) and the last
 * (D, G, H[5]).  OHS_DELAY2_ERR_NO_DEVICE when no GPU is usable.  *out is NULL after a failure. */
int ohs_delay2_create(int device, size_t n_streams, size_t max_objects, size_t max_delay, ohs_delay2 **out);
/* NULL is allowed.  Waits for what the handle has queued. */
void ohs_delay2_destroy(ohs_delay2 *dl);
const char *ohs_delay2_status_string(int status);
const char *ohs_delay2_last_error(void);

/* ---- the unfiltered call ----
 * ohs_delay_process (ohs_delay.h) argument for argument, refusal for refusal and bit for bit: every tile takes the PLAIN pass.  The
 * handle then carries the identity as its taps. */
int ohs_delay2_process(ohs_delay2 *dl, const float *d_in, float *d_out, size_t n_blocks, size_t in_stream_stride,
                       size_t in_channel_stride, size_t out_stream_stride, size_t out_channel_stride, size_t n_objects,
                       size_t seg_blocks, const double *delay, const float *gain, size_t row_stream_stride, int carry,
                       void *hip_stream);

/* ---- the filtered call ----
 * The same arguments, and fir: f32, five per object, stream and segment, H_0 .. H_4 at
 * fir[((s * row_stream_stride + k) * n_objects + c) * 5 + j], in the layout of delay and gain.  fir == NULL makes the call
 * ohs_delay2_process.
 * On the stream, in order: the rows up; k_object_delay2; k_delay2_history, which moves the call's last max_delay + 6 frames into the
 * ring.  A tile is 256 frames of one object inside one segment; it stages its input window in LDS when that is at most 2 048 frames
 * wide and gathers its inputs from global memory otherwise (four loads per lane in the plain pass, twelve in the filtered one).  A
 * filtered tile's window is R frames wider on each side than a plain one's.
 * Refused with OHS_DELAY2_ERR_INVALID_ARG, each before anything is queued, with nothing written and the handle left as it was:
 * everything ohs_delay_process refuses, and with fir non-NULL a tap that is not finite, and any delay below 1 + R = 5 frames (3.6 cm
 * at 48 kHz) -- among the rows given and, under OHS_DELAY2_CARRY, among the delays the handle carries. */
int ohs_delay2_process_filtered(ohs_delay2 *dl, const float *d_in, float *d_out, size_t n_blocks, size_t in_stream_stride,
                                size_t in_channel_stride, size_t out_stream_stride, size_t out_channel_stride, size_t n_objects,
                                size_t seg_blocks, const double *delay, const float *gain, const float *fir,
                                size_t row_stream_stride, int carry, void *hip_stream);

/* Zeroes the history and drops the carry: the stream starts again from silence.  Waits for the whole device first. */
int ohs_delay2_reset(ohs_delay2 *dl);
/* Waits for everything queued on hip_stream. */
int ohs_delay2_sync(ohs_delay2 *dl, void *hip_stream);

/* The most recent call that queued work: the frames of a tile, the widest input window a tile stages in LDS, the tiles that took each
 * form -- staged in LDS, or gathered from global memory -- and, among all of them, the tiles that took the FILTERED pass (counted on
 * the host from the rows: the pass depends on nothing else).  Waits for that call if it has not finished, then reads the device's
 * counters.  Zero tiles before the first call.  Refuses any NULL. */
int ohs_delay2_last_launch(ohs_delay2 *dl, unsigned *tile_frames, unsigned *lds_window, unsigned long long *lds_tiles,
                           unsigned long long *gather_tiles, unsigned long long *filtered_tiles);

/* What the handle holds as (D', G', H') for an OHS_DELAY2_CARRY call: delay[n_streams][n_objects], gain likewise and
 * fir[n_streams][n_objects][5], n_objects the previous call's, written to *n_objects (0, and nothing else written, when nothing is
 * carried).  Host state: it waits for nothing.  Refuses any NULL. */
int ohs_delay2_carried(const ohs_delay2 *dl, size_t *n_objects, double *delay, float *gain, float *fir);

#ifdef __cplusplus
}
#endif
#endif
