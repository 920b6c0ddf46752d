"""The arithmetic of include/ohs_lookup.h in elementwise numpy: every product and every sum is its own numpy operation on f64 arrays,
in the order the header writes them.  There is no einsum and no sum here -- numpy promises no order for those -- so what this file
gives is one definite set of bits, and the device (tests/test_gpu_lookup.py) and lookup_body.hpp compiled for the host
(tests/test_cpu_lookup.py) are held to them."""
import numpy as np

SLICE = 1 << 21         # table points x queries evaluated at a time


def widen(xyz32):
    """the table as the kernel walks it: f32 coordinates widened to f64, [M][3]"""
    return np.ascontiguousarray(xyz32, np.float32).reshape(-1, 3).astype(np.float64)


def pose(R, v):
    """q = R^T v: q[i] = (R[0][i] v[0] + R[1][i] v[1]) + R[2][i] v[2]; R [..][3][3], v [..][3], broadcasting"""
    R, v = np.asarray(R, np.float64), np.asarray(v, np.float64)
    return np.stack([(R[..., 0, i] * v[..., 0] + R[..., 1, i] * v[..., 1]) + R[..., 2, i] * v[..., 2] for i in range(3)], -1)


def rows_queries(v, src_stream_stride, src_seg_stride, R, rot_stream_stride, S, n_segs, K):
    """the queries of ohs_lookup_rows, [S][n_segs][K][3], from what open_headstage_amd.lookup.rows_host_half returns"""
    v = np.asarray(v, np.float64).reshape((S if src_stream_stride else 1, n_segs if src_seg_stride else 1, K, 3))
    v = np.broadcast_to(v, (S, n_segs, K, 3))
    if R is None:
        return v.copy()
    R = np.asarray(R, np.float64).reshape((S if rot_stream_stride else 1, n_segs, 1, 3, 3))
    return pose(np.broadcast_to(R, (S, n_segs, K, 3, 3)), v)


def _sq(a0, a1, a2):
    return (a0 * a0 + a1 * a1) + a2 * a2


def _best_and_runner_up(A):
    """per row: the first index of the minimum, the minimum, and the smallest value at any other index (inf: none)"""
    rows = np.arange(A.shape[0])
    j = np.argmin(A, axis=1)
    best = A[rows, j]
    B = A.copy()
    B[rows, j] = np.inf
    return j, best, B.min(axis=1)


def chord_terms(P, p0, qr, m=None):
    """stage 2 for queries qr [n][3] with nearest points p0 [n][3] against table points P [M][3] (m None: all, -> [n][M]) or one
    point each, P[m] (m [n], -> [n]): (t clamped, O, ok)"""
    c = [(P[None, :, i] - p0[:, None, i]) if m is None else (P[m, i] - p0[:, i]) for i in range(3)]
    x = (lambda a: a[:, None]) if m is None else (lambda a: a)
    L = _sq(*c)
    ok = L > 0.0
    e = [x(qr[:, i] - p0[:, i]) for i in range(3)]
    with np.errstate(invalid="ignore", over="ignore"):
        t = ((c[0] * e[0] + c[1] * e[1]) + c[2] * e[2]) / np.where(ok, L, 1.0)
        t = np.where(t < 0.0, 0.0, t)
        t = np.where(t > 1.0, 1.0, t)
        o = [(x(p0[:, i]) + t * c[i]) - x(qr[:, i]) for i in range(3)]
        O = np.where(ok, _sq(*o), np.inf)
    return t, O, ok


def lookup(xyz32, q, blend=True):
    """-> dict(idx0, idx1, w, d_best, d_next, o_best, o_next) for queries q [n][3] f64 against the table xyz32 [M][3]; without blend
    the stage-2 entries are None.  d_next / o_next: the runner-up, inf where there is none."""
    P = widen(xyz32)
    q = np.ascontiguousarray(q, np.float64).reshape(-1, 3)
    n, M = q.shape[0], P.shape[0]
    out = dict(idx0=np.empty(n, np.uint32), d_best=np.empty(n), d_next=np.empty(n), idx1=None, w=None, o_best=None, o_next=None)
    if blend:
        out.update(idx1=np.empty(n, np.uint32), w=np.empty(n, np.float32), o_best=np.empty(n), o_next=np.empty(n))
    step = max(1, SLICE // M)
    for lo in range(0, n, step):
        s = slice(lo, lo + step)
        qs = q[s]
        d = [P[None, :, i] - qs[:, None, i] for i in range(3)]
        i0, out["d_best"][s], out["d_next"][s] = _best_and_runner_up(_sq(*d))
        out["idx0"][s] = i0
        if not blend:
            continue
        with np.errstate(over="ignore"):
            qr = qs.astype(np.float32).astype(np.float64)
        t, O, _ = chord_terms(P, P[i0], qr)
        j, ob, on = _best_and_runner_up(O)
        found = np.isfinite(ob)
        out["idx1"][s] = np.where(found, j, i0)
        w = np.where(found, t[np.arange(len(j)), j], 0.0).astype(np.float32)
        out["w"][s] = np.where(w == 0, np.float32(0.0), w)          # (a zero of either sign: +0.0)
        out["o_best"][s], out["o_next"][s] = ob, on
    return out


def chord_offset(xyz32, q, idx0, idx1):
    """O of the chord (idx0, idx1) per query, by the same arithmetic (inf where idx1 is a copy of idx0: no chord)"""
    P = widen(xyz32)
    q = np.ascontiguousarray(q, np.float64).reshape(-1, 3)
    qr = q.astype(np.float32).astype(np.float64)
    i0, i1 = np.asarray(idx0).reshape(-1).astype(np.int64), np.asarray(idx1).reshape(-1).astype(np.int64)
    return chord_terms(P, P[i0], qr, i1)[1]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
