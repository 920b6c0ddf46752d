"""The arithmetic of include/ohs_lookup3.h in elementwise numpy: every product, quotient and sum is its own numpy operation on f64
arrays, in the order the header writes them -- scene3.triangle_directions' steps, restated over Cartesian queries.  The device
(tests/test_gpu_lookup3.py) and lookup3_body.hpp compiled for the host (tests/test_cpu_lookup3.py) are held to these bits, and
these to the helper's."""
import numpy as np

from tests.lookup_model import bits, pose, rows_queries, widen  # noqa: F401  (shared with the two-direction model)

SLICE = 1 << 20         # triangles x queries evaluated at a time


def _cross(u, v):
    return [u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]]


def _norm(u):
    return np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])


def inverses(xyz32, tris):
    """-> (inv [T][3][3], singular [T] bool): the cofactor inverses of the header, and which triangles ohs_lookup3_create refuses"""
    P, tri = widen(xyz32), np.asarray(tris, np.int64).reshape(-1, 3)
    a, b, c = P[tri[:, 0]], P[tri[:, 1]], P[tri[:, 2]]
    rows = (_cross(b, c), _cross(c, a), _cross(a, b))
    det = (a[:, 0] * rows[0][0] + a[:, 1] * rows[0][1]) + a[:, 2] * rows[0][2]
    singular = ~(np.abs(det) > 1e-9 * ((_norm(a) * _norm(b)) * _norm(c)))
    inv = np.empty((len(tri), 3, 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(3):
            for j in range(3):
                inv[:, i, j] = rows[i][j] / det
    return inv, singular


def lookup3(xyz32, tris, q):
    """-> dict(idx0, idx1, idx2 uint32, w1, w2 float32, tri uint32, m_best, m_next f64) for queries q [n][3] f64 over the mesh tris
    [T][3] of the table xyz32 [M][3].  m_best: the winner's min(g); m_next: the largest min(g) at any other triangle (-inf: none)."""
    tri = np.asarray(tris, np.int64).reshape(-1, 3)
    inv, singular = inverses(xyz32, tri)
    assert not singular.any(), f"triangle {int(np.flatnonzero(singular)[0])} is singular"
    q = np.ascontiguousarray(q, np.float64).reshape(-1, 3)
    with np.errstate(over="ignore"):
        q = q.astype(np.float32).astype(np.float64)
    n, T = q.shape[0], tri.shape[0]
    out = dict(idx0=np.empty(n, np.uint32), idx1=np.empty(n, np.uint32), idx2=np.empty(n, np.uint32), w1=np.empty(n, np.float32),
               w2=np.empty(n, np.float32), tri=np.empty(n, np.uint32), m_best=np.empty(n), m_next=np.empty(n))
    step = max(1, SLICE // T)
    for lo in range(0, n, step):
        s = slice(lo, lo + step)
        qs = q[s]
        rows = np.arange(qs.shape[0])
        q0, q1, q2 = qs[:, None, 0], qs[:, None, 1], qs[:, None, 2]
        g = [(inv[None, :, i, 0] * q0 + inv[None, :, i, 1] * q1) + inv[None, :, i, 2] * q2 for i in range(3)]      # [n][T] x 3
        m = np.minimum(np.minimum(g[0], g[1]), g[2])
        t = np.argmax(m, axis=1)                                    # (the first of equals)
        out["tri"][s], out["m_best"][s] = t, m[rows, t]
        m[rows, t] = -np.inf
        out["m_next"][s] = m.max(axis=1)
        gt = np.stack([g[i][rows, t] for i in range(3)], -1)        # [n][3]
        top = np.maximum(np.maximum(gt[:, 0], gt[:, 1]), gt[:, 2])
        k = np.where(gt > (top * 2.0 ** -20)[:, None], gt, 0.0)
        k = np.where(k < 0.0, 0.0, k)
        ssum = (k[:, 0] + k[:, 1]) + k[:, 2]
        none = ~(ssum > 0.0)
        at = np.where(gt[:, 0] == top, 0, np.where(gt[:, 1] == top, 1, 2))
        k = np.where(none[:, None], (np.arange(3)[None, :] == at[:, None]).astype(np.float64), k)
        ssum = np.where(none, 1.0, ssum)
        w = k / ssum[:, None]
        v = tri[t]
        order = np.lexsort((v, -w), axis=1)                         # by descending weight, then by ascending index
        v, w = np.take_along_axis(v, order, 1), np.take_along_axis(w, order, 1)
        out["idx0"][s], out["idx1"][s], out["idx2"][s] = v[:, 0], v[:, 1], v[:, 2]
        for name, col in (("w1", 1), ("w2", 2)):
            w32 = w[:, col].astype(np.float32)
            out[name][s] = np.where(w32 == 0, np.float32(0.0), w32)     # (a zero of either sign: +0.0)
    return out


def random_soup(M, T, seed):
    """a random unit table of M points (M >= 3) and T random non-singular triples of it -> (xyz32 [M][3], tris [T][3] uint32): the
    triangles overlap, so that several contain a query and the walk has a real contest"""
    rng = np.random.default_rng(seed)
    xyz = rng.standard_normal((M, 3))
    xyz = (xyz / np.linalg.norm(xyz, axis=1, keepdims=True)).astype(np.float32)
    tris = np.empty((0, 3), np.uint32)
    while len(tris) < T:
        cand = rng.integers(0, M, (2 * T + 8, 3)).astype(np.uint32)
        P = xyz.astype(np.float64)
        a, b, c = P[cand[:, 0]], P[cand[:, 1]], P[cand[:, 2]]
        vol = np.abs(np.einsum("ij,ij->i", a, np.cross(b, c)))      # (well away from create's 1e-9 line: no case sits on it)
        tris = np.concatenate([tris, cand[vol > 1e-3]])
    return xyz, np.ascontiguousarray(tris[:T])


def soup_queries(xyz32, tris, n, seed):
    """about n queries [.][3] f64 for a mesh: random directions at radii 0.5 / 1 / 3, on points, on edge midpoints, on centroids, and
    the origin"""
    rng = np.random.default_rng(seed)
    P, tri = widen(xyz32), np.asarray(tris, np.int64)
    r = rng.standard_normal((n // 2, 3))
    r = r / np.linalg.norm(r, axis=1, keepdims=True) * rng.choice([0.5, 1.0, 3.0], (n // 2, 1))
    t = tri[rng.integers(0, len(tri), n // 6)]
    on_points = P[t[:, 0]]
    mid = (P[t[:, 0]] + P[t[:, 1]]) / 2
    cen = ((P[t[:, 0]] + P[t[:, 1]]) + P[t[:, 2]]) / 3
    return np.ascontiguousarray(np.concatenate([r, on_points, mid, cen, np.zeros((1, 3))]))


FIELDS = ("idx0", "idx1", "idx2", "w1", "w2")


def same_rows(got, m):
    """the five outputs `got` (in FIELDS' order) against the model's: indices equal, weights equal in their bits"""
    ok = np.ones(len(m["idx0"]), bool)
    for name, g in zip(FIELDS, got):
        g = np.asarray(g).reshape(-1)
        ok &= (bits(g) == bits(m[name])) if name.startswith("w") else (g == m[name])
    return ok
