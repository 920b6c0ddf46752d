"""What include/ohs_lookup3p.h adds to include/ohs_lookup3.h, in elementwise numpy: the certificate's threshold, which queries pass 2
answers, and the cube-map cell of a query.  The rows themselves are tests/lookup3_model.lookup3's -- the pruned lookup returns the
unpruned one's bits -- and are not restated here.  The device (tests/test_gpu_lookup3p.py) and lookup3p_body.hpp compiled for the host
(tests/test_cpu_lookup3p.py) are held to these."""
import numpy as np

from tests.lookup3_model import inverses, lookup3


def _round(q):
    q = np.ascontiguousarray(q, np.float64).reshape(-1, 3)
    with np.errstate(over="ignore"):
        return q.astype(np.float32).astype(np.float64)


def bound(xyz32, tris):
    """B: the largest (|inv[t][i][0]| + |inv[t][i][1]|) + |inv[t][i][2]|"""
    a = np.abs(inverses(xyz32, tris)[0])
    return ((a[:, :, 0] + a[:, :, 1]) + a[:, :, 2]).max()


def tau(xyz32, tris, q):
    """the certificate's threshold per query: (2^-40 B) ((|q0| + |q1|) + |q2|) on the query as the walk sees it"""
    a = np.abs(_round(q))
    return (2.0 ** -40 * bound(xyz32, tris)) * ((a[:, 0] + a[:, 1]) + a[:, 2])


def falls_back(xyz32, tris, q, m=None):
    """which queries pass 2 answers: those whose best min(g) over EVERY triangle does not exceed tau -- whatever the grid"""
    m = lookup3(xyz32, tris, q) if m is None else m
    return ~(m["m_best"] > tau(xyz32, tris, q))


def choose_grid(n_tris):
    """grid == 0: the smallest G with 6 G^2 >= n_tris, at most 256"""
    G = 1
    while G < 256 and 6 * G * G < n_tris:
        G += 1
    return G


def cell(q, G):
    """the header's cell assignment: face = 2 axis + (q[axis] < 0), axis the coordinate of largest magnitude (x before y before z among
    equals); u, v the two next coordinates (cyclically) over |q[axis]|; floor((u + 1) (G / 2)) clamped; the origin -> 0"""
    q = _round(q)
    a = np.abs(q)
    axis = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), 0, np.where(a[:, 1] >= a[:, 2], 1, 2))
    rows = np.arange(len(q))
    M, major = a[rows, axis], q[rows, axis]
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = q[rows, (axis + 1) % 3] / M, q[rows, (axis + 2) % 3] / M
        iu = np.clip(np.floor((u + 1.0) * (0.5 * G)), 0, G - 1)
        iv = np.clip(np.floor((v + 1.0) * (0.5 * G)), 0, G - 1)
    face = 2 * axis + (major < 0)
    out = (face * G + np.nan_to_num(iu).astype(np.int64)) * G + np.nan_to_num(iv).astype(np.int64)
    return np.where(M > 0, out, 0).astype(np.uint32)
