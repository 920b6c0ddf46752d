"""How the three lookup libraries cut a *_rows call into chunks and what they stage for each, restated in numpy from the headers and
api_lookup.hip / api_lookup3.hip / api_lookup3p.hip (RowSource::range, the memcpy loops, the kernels' index expression), and the
shapes, the checker and the one-handle sequence that tests/test_gpu_lookup_chunks.py runs on the device.  Pure numpy: no GPU, no
library.  tests/test_cpu_lookup_chunks.py holds all of it to what it names.

A call of n = S * segs * K queries is cut every CHUNK queries.  A chunk that covers (s_lo, k_lo) .. (s_hi, k_hi) stages the packed
entries [lo, hi] that RowSource::range names -- five branches, BRANCHES below -- and hands the kernel g0 = at, src_base = lo of the
sources and rot_base = lo of the poses; the kernel rebuilds (s, k, c) from g0 + i and reads entry s a + k b - base.

THE PALETTE.  Sources come from a palette of P points and poses from a palette of R matrices, so a call of 540 000 queries has at
most P (R + 1) distinct (source, pose) PAIRS; the pose is a per-query function, so the model computed once per pair and indexed out is
exact.  Every array that goes to a library has a twin of the same layout that holds the palette's indices instead of coordinates:
staged through the same code it names the pair each query must be, and the numpy libraries below (NumpyLibrary) work on it alone.

AN ADAPTER is what the checkers drive -- a device library or a NumpyLibrary:
    Q, dtypes (one per output plane), optional (the planes that may be NULL together),
    rows(case, arrays) -> status, points(q, pair, arrays) -> status, launch() -> (chunks, fallback or None),
    want (the model's planes per pair, as uint32 bits), rest (per pair: answered by pass 2; None where the library has no pass 2),
    existing(got, pair, what): the library's existing checker on the same answers (a NumpyLibrary has none)."""
import numpy as np

from tests.lookup_model import pose, rows_queries, widen

CHUNK = 1 << 18
BRANCHES = ("stream and segment", "stream", "segment, one stream", "segment, every stream", "shared")
SENT_U, SENT_F = np.uint32(0xDEADBEEF), np.float32(-7.25)
GAP = -2.0              # the indices' twin of an unreadable gap
INV = 1                 # OHS_ERR_INVALID_ARG
FAULTS = ("src base", "rot base", "segment zero", "g0", "last fallback", "first cap")


# ---- the cut and the ranges ------------------------------------------------------------------------------------------------------
def _ab(stream_stride, seg_stride, segs):
    """RowSource::a, ::b: the packed entry of (s, k) is s a + k b"""
    return ((segs if seg_stride else 1) if stream_stride else 0), (1 if seg_stride else 0)


def _range(stream_stride, seg_stride, segs, s_lo, k_lo, s_hi, k_hi):
    """RowSource::range -> (lo, hi, branch)"""
    if stream_stride and seg_stride:
        return s_lo * segs + k_lo, s_hi * segs + k_hi, BRANCHES[0]
    if stream_stride:
        return s_lo, s_hi, BRANCHES[1]
    if seg_stride:
        return (k_lo, k_hi, BRANCHES[2]) if s_lo == s_hi else (0, segs - 1, BRANCHES[3])
    return 0, 0, BRANCHES[4]


def _entry(j, stream_stride, seg_stride, segs):
    """RowSource::entry: where packed entry j lies in the caller's array, in entries"""
    if stream_stride and seg_stride:
        return (j // segs) * stream_stride + (j % segs) * seg_stride
    return j * stream_stride if stream_stride else j * seg_stride


def chunk_plan(S, segs, K, sss, sks, rss, has_rot, Q=CHUNK):
    """-> per chunk dict(at, nq, lo (s, k), hi (s, k), src (lo, hi, branch), rot (lo, hi, branch) or None, c)"""
    n, plan = S * segs * K, []
    for at in range(0, n, Q):
        nq = min(Q, n - at)
        sk_lo, sk_hi = at // K, (at + nq - 1) // K
        lo, hi = (sk_lo // segs, sk_lo % segs), (sk_hi // segs, sk_hi % segs)
        plan.append(dict(at=at, nq=nq, lo=lo, hi=hi, src=_range(sss, sks, segs, *lo, *hi), rot=_range(rss, 1, segs, *lo, *hi) if has_rot else None,
                         c=at % K))
    return plan


def _gather(arr, eu, stream_stride, seg_stride, segs, span, e, sub, unit, first, base, exact, what):
    """pack entries [lo, hi] of arr (eu values each) as the memcpy loop does -- from `first` on -- and read `unit` values at
    ((e - base) * (eu // unit) + sub) * unit, as the kernel does.  exact: every read inside the packed bytes and off every gap, or
    an AssertionError; else a read outside gives -1"""
    lo, hi = span
    j = np.arange(hi - lo + 1, dtype=np.int64) + first
    packed = arr[_entry(j, stream_stride, seg_stride, segs)[:, None] * eu + np.arange(eu)].reshape(-1)
    at = ((e - base) * (eu // unit) + sub) * unit
    ok = (at >= 0) & (at + unit <= packed.size)
    if exact:
        assert ok.all(), f"{what}: {int((~ok).sum())} reads outside the {packed.size} packed values, the first at query {int(np.argmin(ok))}"
        assert np.isfinite(packed).all() and (packed != GAP).all(), f"{what}: a gap was packed"
    out = packed[np.where(ok, at, 0)[:, None] + np.arange(unit)]
    return np.where(ok[:, None], out, -1.0)


def staged_queries(src, rot, S, segs, K, sss, sks, rss, Q=CHUNK, unit=3, rot_unit=9, fault=None):
    """-> (v [n][unit], r [n][rot_unit] or None): what each query reads through the staging.  src holds K * unit values per entry, rot
    rot_unit.  fault: one of FAULTS[:4], a library wrong in that way"""
    assert fault in (None,) + FAULTS[:4]
    src = np.asarray(src, np.float64).reshape(-1)
    rot = None if rot is None else np.asarray(rot, np.float64).reshape(-1)
    a, b = _ab(sss, sks, segs)
    ra, _ = _ab(rss, 1, segs)
    vs, rs = [], []
    for ci, ch in enumerate(chunk_plan(S, segs, K, sss, sks, rss, rot is not None, Q)):
        g = (0 if fault == "g0" else ch["at"]) + np.arange(ch["nq"], dtype=np.int64)
        sk = g // K
        c, s = g - sk * K, sk // segs
        k = sk - s * segs
        lo, hi, branch = ch["src"]
        first = 0 if fault == "segment zero" and branch == BRANCHES[2] else lo
        base = 0 if fault == "src base" and ci > 0 else lo
        vs.append(_gather(src, K * unit, sss, sks, segs, (lo, hi), s * a + k * b, c, unit, first, base, fault is None, f"sources of chunk {ci}"))
        if rot is not None:
            rlo, rhi, branch = ch["rot"]
            first = 0 if fault == "segment zero" and branch == BRANCHES[2] else rlo
            base = lo if fault == "rot base" else rlo
            rs.append(_gather(rot, rot_unit, rss, 1, segs, (rlo, rhi), s * ra + k, 0, rot_unit, first, base, fault is None, f"poses of chunk {ci}"))
    return np.concatenate(vs), (np.concatenate(rs) if rs else None)


# ---- the palette and the cases -------------------------------------------------------------------------------------------------------
def palette(xyz32, tris=None, n_points=24, n_poses=6, seed=0):
    """-> (points [P][3] f64, poses [R][3][3] f64, n_meas): the first n_meas points ARE measurements (f32 values widened), then edge
    midpoints and centroids (of the mesh, or of random pairs and triples of the table), then random directions at radii 0.5, 1, 3;
    poses[0] is the identity -- R^T v is then v itself, a query exactly on a corner -- the others random orthonormal matrices"""
    rng = np.random.default_rng(seed)
    T = widen(xyz32)
    tri = np.asarray(tris, np.int64) if tris is not None else np.stack([rng.permutation(len(T))[:3] for _ in range(16)])
    n_meas = n_points // 3
    t = tri[rng.integers(0, len(tri), n_points)]
    mid, cen = (T[t[:, 0]] + T[t[:, 1]]) / 2, ((T[t[:, 0]] + T[t[:, 1]]) + T[t[:, 2]]) / 3
    r = rng.standard_normal((n_points, 3))
    r = r / np.linalg.norm(r, axis=1, keepdims=True) * rng.choice([0.5, 1.0, 3.0], (n_points, 1))
    n_each = (n_points - n_meas) // 3
    points = np.concatenate([T[rng.choice(len(T), n_meas, replace=False)], mid[:n_each], cen[:n_each], r])[:n_points]
    poses = np.concatenate([np.eye(3)[None], np.linalg.qr(rng.standard_normal((n_poses - 1, 3, 3)))[0]])
    return np.ascontiguousarray(points), np.ascontiguousarray(poses), n_meas


def pair_queries(points, poses):
    """the query of every pair [P (R + 1)][3]: pair p (R + 1) is the source p without a pose, p (R + 1) + 1 + r the source under pose r
    (lookup_model.pose's operations, the kernels')"""
    return np.ascontiguousarray(np.concatenate([points[:, None], pose(poses[None, :], points[:, None])], axis=1).reshape(-1, 3))


# form -> (sources: per stream, per segment; poses: None, or per stream; wide strides)
FORMS = {"a": (True, True, True, False), "b": (False, True, True, False), "c": (True, True, False, False), "d": (True, False, None, False),
         "e": (True, True, True, True), "f": (True, False, True, False), "g": (False, False, False, False)}


def rows_case(pal, S, segs, K, form, seed):
    """one *_rows call from the palette -> dict(S, segs, K, sss, sks, rss, src, rot, src_id, rot_id, pair [n], v, R, form): src / rot
    what the library is given (gaps NaN / Inf), src_id / rot_id their twins of indices, pair the pair of every query by the direct
    formula, v / R the dense arrays lookup_model.rows_queries takes.  With K >= 2 object 0 of every entry is a measurement and object 1
    is not, and a third of the poses are the identity: both kinds of query wherever a chunk lies."""
    points, poses, n_meas = pal
    per_s, per_k, rot_s, wide = FORMS[form]
    rng = np.random.default_rng(seed)
    P, R = len(points), len(poses)
    ds, dk = (S if per_s else 1), (segs if per_k else 1)
    sid = rng.integers(0, P, (ds, dk, K))
    if K >= 2:
        sid[..., 0], sid[..., 1] = rng.integers(0, n_meas, (ds, dk)), rng.integers(n_meas, P, (ds, dk))
    sks = (2 if wide else 1) if per_k else 0
    sss = ((segs - 1) * sks + 1 + (3 if wide else 0)) if per_s else 0
    off = (np.arange(ds)[:, None] * sss + np.arange(dk)[None, :] * sks).reshape(-1)
    src = np.full((int(off.max()) + 1, K, 3), np.nan)
    src_id = np.full((int(off.max()) + 1, K), GAP)
    src[off], src_id[off] = points[sid].reshape(-1, K, 3), sid.reshape(-1, K)
    case = dict(S=S, segs=segs, K=K, sss=sss, sks=sks, rss=0, src=src, src_id=src_id, rot=None, rot_id=None, v=points[sid], R=None, form=form)
    pair = np.broadcast_to(sid, (S, segs, K)) * (R + 1)
    if rot_s is not None:
        dr = S if rot_s else 1
        rid = np.where(rng.random((dr, segs)) < 1 / 3, 0, rng.integers(1, R, (dr, segs)))
        rss = (segs + (2 if wide else 0)) if rot_s else 0
        off = (np.arange(dr)[:, None] * rss + np.arange(segs)[None, :]).reshape(-1)
        rot = np.full((int(off.max()) + 1, 3, 3), np.inf)
        rot_id = np.full(int(off.max()) + 1, GAP)
        rot[off], rot_id[off] = poses[rid].reshape(-1, 3, 3), rid.reshape(-1)
        case.update(rss=rss, rot=rot, rot_id=rot_id, R=poses[rid])
        pair = pair + (np.broadcast_to(rid, (S, segs)) + 1)[:, :, None]
    case["pair"] = np.ascontiguousarray(pair.reshape(-1))
    return case


def case_queries(case):
    """lookup_model.rows_queries on the case's dense arrays [n][3]: the direct formula"""
    c = case
    return rows_queries(c["v"], c["sss"], c["sks"], c["R"], c["rss"], c["S"], c["segs"], c["K"]).reshape(-1, 3)


def staged_pairs(case, n_poses, Q=CHUNK, fault=None):
    """the pair of every query as the staging delivers it (-1: a read outside the packed bytes)"""
    c = case
    v, r = staged_queries(c["src_id"], c["rot_id"], c["S"], c["segs"], c["K"], c["sss"], c["sks"], c["rss"], Q, 1, 1, fault)
    v = v[:, 0].astype(np.int64)
    r = np.zeros_like(v) if r is None else r[:, 0].astype(np.int64) + 1
    return np.where((v < 0) | (r < 0), -1, v * (n_poses + 1) + r)


def shape_a(pal, form, seed=1):
    return rows_case(pal, 3, 30000, 6, form, seed)


def shape_b(pal, Q=CHUNK, seed=2):
    return rows_case(pal, Q // 64 + 3, 1, 64, "f", seed)


def shape_c(pal, Q=CHUNK, seed=3):
    return rows_case(pal, Q + 5, 1, 1, "f", seed)


def big_rows(pal, Q=CHUNK, seed=4):
    """K = 1 with a pose per stream and segment: 96 bytes of input per query, a chunk and some"""
    return rows_case(pal, Q // 1000 + 2, 1000, 1, "a", seed)


# ---- the checker ---------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def new_arrays(dtypes, n, extra=5):
    return [np.full(n + extra, SENT_F if d == np.float32 else SENT_U, d) for d in dtypes]


def untouched(arrays, lo=0):
    return all(a is None or (bits(a[lo:]) == bits(np.array([SENT_F if a.dtype == np.float32 else SENT_U], a.dtype))).all() for a in arrays)


def first_bad(got, want, pair, Q, segs=1, K=1):
    """got: the output arrays (None: not asked for), want: the model's planes per pair, pair [n] -> None, or the first wrong answer as
    dict(query, chunk, stream, segment, object, planes)"""
    n = len(pair)
    bad = np.zeros(n, bool)
    for g, w in zip(got, want):
        if g is not None:
            bad |= bits(g[:n]) != w[pair]
    if not bad.any():
        return None
    i = int(np.argmax(bad))
    return dict(query=i, chunk=i // Q, stream=i // K // segs, segment=i // K % segs, object=i % K, wrong=int(bad.sum()),
                planes=[j for j, (g, w) in enumerate(zip(got, want)) if g is not None and bits(g[i:i + 1])[0] != w[pair[i]]])


def model_planes(m, fields):
    """the model's fields as planes of uint32 bits"""
    return [bits(m[f]) for f in fields]


def hold_answers(ad, got, pair, what, segs=1, K=1):
    """every answer bit for bit, every word behind n the sentinel, a zero weight +0.0"""
    bad = first_bad(got, ad.want, pair, ad.Q, segs, K)
    assert bad is None, (f"{what}: {bad['wrong']} wrong answers, the first at query {bad['query']}: chunk {bad['chunk']}, stream {bad['stream']}, "
                         f"segment {bad['segment']}, object {bad['object']} (planes {bad['planes']})")
    assert untouched(got, len(pair)), f"{what}: a word behind the {len(pair)} answers was written"
    assert all(g is None or g.dtype != np.float32 or (bits(g[:len(pair)]) != 0x80000000).all() for g in got), f"{what}: a weight of -0.0"


def hold_launch(ad, pair, what):
    """the record of the call: the chunks, and the queries pass 2 answered summed over them"""
    n = len(pair)
    chunks = -(-n // ad.Q)
    per_chunk = None if ad.rest is None else [int(ad.rest[pair[at:at + ad.Q]].sum()) for at in range(0, n, ad.Q)]
    want = (chunks, None if per_chunk is None else sum(per_chunk))
    assert ad.launch() == want, f"{what}: the launch record {ad.launch()} against {want}; pass 2's share chunk by chunk: {per_chunk}"
    return per_chunk


def hold_rows(ad, case, what, null=False):
    """one rows call on the adapter: status, answers, tails, record -> the arrays"""
    arrays = new_arrays(ad.dtypes, len(case["pair"]))
    given = [None if null and j in ad.optional else a for j, a in enumerate(arrays)]
    assert ad.rows(case, given) == 0, f"{what}: refused"
    hold_answers(ad, given, case["pair"], what, case["segs"], case["K"])
    ad.existing(given, case["pair"], what)
    assert untouched([a for a, g in zip(arrays, given) if g is None]), f"{what}: an output that was not asked for was written"
    hold_launch(ad, case["pair"], what)
    return arrays


def hold_points(ad, pal_q, pair, what, null=False):
    arrays = new_arrays(ad.dtypes, len(pair))
    given = [None if null and j in ad.optional else a for j, a in enumerate(arrays)]
    assert ad.points(np.ascontiguousarray(pal_q[pair]), pair, given) == 0, f"{what}: refused"
    hold_answers(ad, given, pair, what)
    ad.existing(given, pair, what)
    assert untouched([a for a, g in zip(arrays, given) if g is None]), f"{what}: an output that was not asked for was written"
    hold_launch(ad, pair, what)
    return arrays


# ---- one handle, many calls ---------------------------------------------------------------------------------------------------------
SMALL_N, SMALL_K, SMALL_FORMS = (1, 64, 65, 300), (1, 6, 64), "abcdeg"


def draw_sequence(seed):
    """16 operations for ONE handle.  Fixed places: 'big rows' (K = 1, a pose per stream and segment: 96 input bytes per query, more than
    a chunk) at 1, BEFORE the first 'points' of Q + 1 at 4 -- the input staging grows while the output staging is still small --, shape
    B at 7, and the reverse order later: 'points' of Q + 1 at 10, 'big rows' at 12.  A small served call stands right behind each of
    the five (2, 5, 8, 11, 13): small points, small rows of S = 3, segs = 5 in a random stride form, and one of them with the optional
    outputs NULL.  Place 0 holds a small served call too, so that the output staging starts small.  The other places (3, 6, 9, 14, 15)
    hold, shuffled: an empty call of each entry, a refused call of each kind (a NaN coordinate, a short stride), and a small call."""
    rng = np.random.default_rng(52000 + seed)

    def small(null=False):
        if rng.integers(0, 2):
            return ("points", int(rng.choice(SMALL_N)), null, int(rng.integers(1 << 30)))
        return ("rows", int(rng.choice(SMALL_K)), SMALL_FORMS[int(rng.integers(len(SMALL_FORMS)))], null, int(rng.integers(1 << 30)))
    ops = [None] * 16
    ops[1], ops[4], ops[7], ops[10], ops[12] = ("big rows",), ("points", "Q + 1", False, 41), ("shape b",), ("points", "Q + 1", False, 42), ("big rows",)
    behind = [small(null=j == 0) for j in range(5)]
    for at, j in zip((2, 5, 8, 11, 13), rng.permutation(5)):
        ops[at] = behind[j]
    ops[0] = small()
    other = [("empty", "points"), ("empty", "rows"), ("refused", "nan"), ("refused", "stride"), small()]
    for at, j in zip((3, 6, 9, 14, 15), rng.permutation(5)):
        ops[at] = other[j]
    return ops


def is_large(op):
    return op[0] in ("big rows", "shape b") or (op[0] == "points" and op[1] == "Q + 1")


def is_small_served(op):
    return op[0] in ("points", "rows") and not is_large(op)


def run_sequence(ad, pal, ops):
    """every operation on the one adapter; after each: the answers bit for bit, the tails, the launch record (unchanged by a refusal,
    no chunks after an empty call).  A failure prints the sequence so far."""
    pal_q = pair_queries(pal[0], pal[1])
    done, record = [], ad.launch()
    for op in ops:
        done.append(" ".join(str(v) for v in op))
        where = f"operation {len(done) - 1}: {done[-1]}; the sequence so far:\n  " + "\n  ".join(done)
        try:
            if op[0] == "points":
                n = ad.Q + 1 if op[1] == "Q + 1" else op[1]
                hold_points(ad, pal_q, np.random.default_rng(op[3]).integers(0, len(pal_q), n), "points", op[2])
            elif op[0] == "rows":
                hold_rows(ad, rows_case(pal, 3, 5, op[1], op[2], op[4]), "small rows", op[3])
            elif op[0] == "big rows":
                hold_rows(ad, big_rows(pal, ad.Q), "big rows")
            elif op[0] == "shape b":
                hold_rows(ad, shape_b(pal, ad.Q), "shape b")
            elif op[0] == "empty":
                arrays = new_arrays(ad.dtypes, 8)
                if op[1] == "points":
                    assert ad.points(np.zeros((0, 3)), np.zeros(0, np.int64), arrays) == 0
                else:
                    assert ad.rows(dict(rows_case(pal, 3, 5, 6, "a", 7), S=0), arrays) == 0
                assert untouched(arrays), "an empty call wrote"
                assert ad.launch() == (0, None if ad.rest is None else 0), f"the record behind an empty call: {ad.launch()}"
            elif op[0] == "refused":
                case = rows_case(pal, 3, 5, 6, "a", 8)
                if op[1] == "nan":
                    case["src"] = case["src"].copy()
                    case["src"][7, 3, 1] = np.nan
                else:
                    case["sss"] = case["segs"] - 1
                arrays = new_arrays(ad.dtypes, len(case["pair"]))
                assert ad.rows(case, arrays) == INV, "not refused"
                assert untouched(arrays), "a refused call wrote"
                assert ad.launch() == record, f"the record behind a refused call: {ad.launch()}, before it {record}"
            else:
                raise ValueError(op)
        except AssertionError as e:
            raise AssertionError(f"{where}\n{e}") from e
        record = ad.launch()
    return len(done)


# ---- the libraries in numpy, right or wrong in one way -------------------------------------------------------------------------------
class NumpyLibrary:
    """A handle of any of the three libraries over the palette's indices: the cut, the staging (staged_pairs), the output planes `cap`
    apart in a staging that grows and never shrinks, the copies to `at`, the fallback count.  fault: None, or one of FAULTS."""

    def __init__(self, want, rest, dtypes, optional, n_poses, Q=CHUNK, fault=None):
        assert fault is None or fault in FAULTS
        self.want, self.rest, self.dtypes, self.optional, self.n_poses, self.Q, self.fault = want, rest, dtypes, optional, n_poses, Q, fault
        self.cap = self.first_cap = 0
        self.d_out = np.zeros(0, np.uint32)
        self.last = (0, 0)

    def existing(self, got, pair, what):
        pass

    def launch(self):
        return (self.last[0], None if self.rest is None else self.last[1])

    def _serve(self, pair, arrays):
        if arrays[0] is None or any((arrays[j] is None) != (arrays[self.optional[0]] is None) for j in self.optional):
            return INV
        if any(a is None for j, a in enumerate(arrays) if j not in self.optional):
            return INV
        chunks = fallback = 0
        for at in range(0, len(pair), self.Q):
            p = pair[at:at + self.Q]
            if len(p) > self.cap:
                self.cap, self.d_out = len(p), np.full(len(self.dtypes) * len(p), 0xCDCDCDCD, np.uint32)
                self.first_cap = self.first_cap or self.cap
            for j, w in enumerate(self.want):
                self.d_out[j * self.cap:j * self.cap + len(p)] = np.where(p >= 0, w[np.maximum(p, 0)], 0x0BADBAD0)
            down = self.first_cap if self.fault == "first cap" else self.cap
            for j, a in enumerate(arrays):
                if a is not None:
                    bits(a)[at:at + len(p)] = self.d_out[j * down:j * down + len(p)]
            count = 0 if self.rest is None else int(((p < 0) | self.rest[np.maximum(p, 0)]).sum())
            fallback = count if self.fault == "last fallback" else fallback + count
            chunks += 1
        self.last = (chunks, fallback)
        return 0

    def points(self, q, pair, arrays):
        return self._serve(np.asarray(pair, np.int64), arrays)

    def rows(self, case, arrays):
        c = case
        if c["S"] == 0:
            self.last = (0, 0)
            return 0
        if c["sss"] and c["sss"] < (c["segs"] - 1) * c["sks"] + 1:
            return INV
        if c["rot"] is not None and c["rss"] and c["rss"] < c["segs"]:
            return INV
        if not np.isfinite(c["src"][c["src_id"][:, 0] != GAP]).all() or (c["rot"] is not None and not np.isfinite(c["rot"][c["rot_id"] != GAP]).all()):
            return INV              # (every entry the strides name, before the first chunk runs)
        return self._serve(staged_pairs(c, self.n_poses, self.Q, self.fault if self.fault in FAULTS[:4] else None), arrays)
