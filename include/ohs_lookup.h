/* ohs_lookup.h -- C ABI of libohs_lookup.so: the rows the scene calls read -- a direction index per object, stream and segment, and
 * for ohs_scene2_process_blended a second index and a weight -- found on the device (k_lookup; DESIGN.md section 4.5j, SCENES.md).
 *
 * A library of its own: it links none of the product's code, exports the ohs_lookup_* names below and nothing else, and its handle
 * mixes with no other library's.  What it computes is what the host helpers of open_headstage_amd (scene.nearest_directions,
 * scene2.bracket_directions) define, as the arithmetic written out below; tests/lookup_model.py restates it and the device is held
 * to that model's bits.
 *
 * Conventions: every function returns a status (0 = ok; the values are ohs_hip.h's OHS_* codes, restated below),
 * ohs_lookup_last_error() is the thread-local detail of the last failure in THIS library.  EVERY pointer is a HOST pointer.  EVERY
 * call is SYNCHRONOUS: the answers are in the caller's arrays on return.  The handle works on a non-blocking stream of its own, so
 * that a scene call queued from another thread is not serialised behind it.  A handle is used from one thread at a time.
 *
 * THE ARITHMETIC.  Everything is f64, every operation is rounded by itself (no fused multiply-add), sums are taken in the order
 * written.  P[m] is the table's f32 coordinate widened to f64.
 *   pose (rows only)   q[i] = (R[0][i] v[0] + R[1][i] v[1]) + R[2][i] v[2]   (q = R^T v; rot == NULL: q = v)
 *   stage 1            d = P[m] - q;  D(m) = (d0 d0 + d1 d1) + d2 d2;  idx0 = the smallest m at which D is minimal
 *   stage 2 (idx1, w)  qr = q rounded to f32 and widened again;  p0 = P[idx0];  for every m:
 *                        c = P[m] - p0;  L = (c0 c0 + c1 c1) + c2 c2;  m is skipped unless L > 0
 *                        e = qr - p0;  t = ((c0 e0 + c1 e1) + c2 e2) / L;  t = min(max(t, 0), 1)
 *                        o = (p0 + t c) - qr;  O(m) = (o0 o0 + o1 o1) + o2 o2
 *                      idx1 = the smallest m at which O is minimal, w = (float)t at that m, a zero written as +0.0;
 *                      no m survives (every point is a copy of P[idx0]): idx1 = idx0, w = +0.0
 * There is no trigonometry here: angles become coordinates on the caller's side.
 *
 * Out of scope (none of it is built): rows handed to the scene calls on the device (their ABI takes host rows); the three
 * directions and two weights per object that libohs_scene3.so renders (ohs_scene3.h: the caller computes those rows); a session
 * renderer over scenes. */
#ifndef OHS_LOOKUP_H
#define OHS_LOOKUP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OHS_LOOKUP_OK              0
#define OHS_LOOKUP_ERR_INVALID_ARG 1
#define OHS_LOOKUP_ERR_NO_DEVICE   2
#define OHS_LOOKUP_ERR_HIP         3
#define OHS_LOOKUP_ERR_ALLOC       6

#define OHS_LOOKUP_MAX_OBJECTS     64
#define OHS_LOOKUP_MAX_DIRECTIONS  65536
#define OHS_LOOKUP_MAX_MAGNITUDE   1e100    /* of any query, source or matrix element */

typedef struct ohs_lookup ohs_lookup;

/* A table of n_dirs points (1 .. 65536), xyz[n_dirs][3] Cartesian f32, on `device`.  The table is fixed for the handle's life.
 * Refuses out == NULL, xyz == NULL, n_dirs out of range, a coordinate that is not finite; OHS_LOOKUP_ERR_NO_DEVICE when no GPU
 * is usable.  *out is NULL after a failure. */
int ohs_lookup_create(int device, size_t n_dirs, const float *xyz, ohs_lookup **out);
/* NULL is allowed. */
void ohs_lookup_destroy(ohs_lookup *lk);
const char *ohs_lookup_status_string(int status);
const char *ohs_lookup_last_error(void);

/* n free-standing queries q[n][3] (f64, the table's Cartesian frame) -> idx0[n], and idx1[n], w[n].
 * idx1 and w are both NULL or both given; both NULL: nearest only, stage 2 does not run and nothing but idx0 is written.
 * n == 0 is OK and touches nothing.  Queries of any count are cut into chunks inside the call; device and pinned memory grow to the
 * largest chunk seen and are then reused.
 * Refused with OHS_LOOKUP_ERR_INVALID_ARG, the handle as it was and the outputs untouched: lk, q or idx0 NULL; one of idx1 / w NULL
 * and the other not; a coordinate that is not finite or above 1e100 in magnitude. */
int ohs_lookup_points(ohs_lookup *lk, size_t n, const double *q, uint32_t *idx0, uint32_t *idx1, float *w);

/* Rows for a scene call: out[(s * n_segs + k) * n_objects + c], i.e. idx_stride = n_segs of ohs_scene*_process.
 *   source c of stream s in segment k: src[((s * src_stream_stride + k * src_seg_stride) * n_objects + c) * 3 ..]  (a stride of 0 shares)
 *   pose of stream s in segment k:     rot[(s * rot_stream_stride + k) * 9 ..], row-major 3 x 3; rot == NULL: the identity
 * The query of (s, k, c) is the pose applied to the source (THE ARITHMETIC above), then ohs_lookup_points' rule.
 * n_streams == 0 or n_segs == 0 is OK and touches nothing.
 * Refused with OHS_LOOKUP_ERR_INVALID_ARG, the handle as it was and the outputs untouched: everything ohs_lookup_points refuses
 * (src in q's place); n_objects of 0 or above 64; src_stream_stride neither 0 nor >= (n_segs - 1) * src_seg_stride + 1;
 * rot_stream_stride neither 0 nor >= n_segs; a source or matrix element that would be read and is not finite or above 1e100. */
int ohs_lookup_rows(ohs_lookup *lk, size_t n_streams, size_t n_segs, size_t n_objects,
                    const double *src, size_t src_stream_stride, size_t src_seg_stride,
                    const double *rot, size_t rot_stream_stride,
                    uint32_t *idx0, uint32_t *idx1, float *w);

/* The most recent successful call: the table points the kernel stages at a time, the queries per chunk, and the chunks the call was
 * cut into (0 before the first call and behind a call of no queries).  Refuses any NULL. */
int ohs_lookup_last_launch(const ohs_lookup *lk, unsigned *tile_points, size_t *chunk_queries, size_t *chunks);

#ifdef __cplusplus
}
#endif
#endif
