"""numpy reference of the streamed retrieval kernels (csrc/retrieval_stream.hip) -- plain helper module, no tests of its own.

Two families of inputs, each with the statement that can be made about it:

* EXACT GRID.  Feature entries are k/8, k in -4..4, d <= 512: every product is a multiple of 1/64, every partial sum a multiple of
  1/64 below 2^13 units (512 * 16), so an fp32 sum of them is exact in ANY order.  ``grid_scores`` takes them in int64; counts, top-k
  values and indices have to be met exactly.  Low d and duplicated rows give dense genuine ties.
* REAL-VALUED BAND.  Unit-norm float32 rows around a common centre (``real_inputs``); scores in fp64.  delta = d 2^-24 max|q_i||g_j|
  bounds the error of an fp32 dot product in any summation order, so a candidate is certainly above the label when its fp64 score
  exceeds the label's by more than 2 delta, and cannot be above or equal when it lies more than 2 delta below (``band``).  For the
  dual-softmax re-rank the margin is per element, eps |x| (``dsl_band``), eps = 4 x the largest relative deviation from fp64 of a
  numpy-float32 restatement of dsl_rerank_kernel's formula on the same inputs (``dsl_restated_f32``, ``dsl_epsilon``).
  ``check_band`` holds counts to the band and returns the share of queries the band does not pin to one value."""
import functools

import numpy as np

GRID = 8                                   # feature entries are multiples of 1 / GRID


# ------------------------------------------------------------------------------------------------------------------ exact grid
def grid_inputs(nq, ng, d, seed, dup_q=(), dup_g=()):
    """(q, g) float32 with entries k/8, k in -4..4; ``dup_g`` / ``dup_q``: (dst, src) pairs -- row dst becomes a copy of row src"""
    assert d <= 512
    rng = np.random.default_rng(seed)
    q = rng.integers(-4, 5, size=(nq, d)).astype(np.float32) / GRID
    g = rng.integers(-4, 5, size=(ng, d)).astype(np.float32) / GRID
    for dst, src in dup_q:
        q[dst] = q[src]
    for dst, src in dup_g:
        g[dst] = g[src]
    return q, g


def grid_scores(q, g):
    """int64 [nq, ng]: the scores in units of 1/64 (exact); score = units / 64 is exact in fp32"""
    qi, gi = np.rint(q.astype(np.float64) * GRID).astype(np.int64), np.rint(g.astype(np.float64) * GRID).astype(np.int64)
    assert np.array_equal(qi / GRID, q) and np.array_equal(gi / GRID, g) and max(np.abs(qi).max(), np.abs(gi).max()) <= 4
    return qi @ gi.T


def counts(x, labels=None):
    """(greater, equal) per ROW of x against the labelled entry (default: the diagonal); int64"""
    n = x.shape[0]
    lab = np.arange(n) if labels is None else np.asarray(labels)
    v = x[np.arange(n), lab][:, None]
    return (x > v).sum(1), (x == v).sum(1)


def topk(x, k, index_base=0):
    """(values [n, k], indices [n, k]): value descending, ties to the lowest index"""
    order = np.argsort(-x, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(x, order, 1), order + index_base


def ranks_from_counts(greater, equal):
    """every sorted position that ties the label -- what oracle.retrieval_oracle.ranks lists"""
    return np.concatenate([np.arange(g, g + e) for g, e in zip(greater, equal)])


# ------------------------------------------------------------------------------------------------------------ real-valued band
def _normalise(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def real_inputs(nq, ng, d, seed):
    """unit-norm float32 rows normalise(c + 0.35 noise / sqrt d) around one centre c; q[i] += 0.5 (g[i] - c) for the paired rows
    i < min(nq, ng), so that the diagonal is a meaningful label.  (Fully random rows leave 7 % of the queries ambiguous.)"""
    rng = np.random.default_rng(seed)
    c = _normalise(rng.standard_normal((1, d)))
    g = c + 0.35 * rng.standard_normal((ng, d)) / np.sqrt(d)
    q = c + 0.35 * rng.standard_normal((nq, d)) / np.sqrt(d)
    n = min(nq, ng)
    q[:n] += 0.5 * (g[:n] - c)
    return _normalise(q).astype(np.float32), _normalise(g).astype(np.float32)


def scores64(q, g):
    return q.astype(np.float64) @ g.astype(np.float64).T


def delta(q, g):
    """the worst error of an fp32 dot product of a row of q with a row of g, in any summation order"""
    q, g = q.astype(np.float64), g.astype(np.float64)
    return q.shape[1] * 2.0 ** -24 * np.linalg.norm(q, axis=1).max() * np.linalg.norm(g, axis=1).max()


def band(x, labels, margin):
    """per ROW of the fp64 matrix x: lo = #{x > x_label + 2 margin}, hi = #{x >= x_label - 2 margin}"""
    n = x.shape[0]
    lab = np.arange(n) if labels is None else np.asarray(labels)
    v = x[np.arange(n), lab][:, None]
    return (x > v + 2 * margin).sum(1), (x >= v - 2 * margin).sum(1)


def dsl64(s, theta):
    """s * softmax(theta s, axis 0) in fp64"""
    y = s * theta
    e = np.exp(y - y.max(0, keepdims=True))
    return s * (e / e.sum(0, keepdims=True))


def dsl_restated_f32(q, g, theta):
    """dsl_rerank_kernel's formula (csrc/retrieval.hip) in numpy float32 on the float32 product of the same features:
    mx = max_i s theta; sum = sum_i exp(s theta - mx); x = s * (exp(s theta - mx) / sum)"""
    s = (q @ g.T).astype(np.float32)
    th = np.float32(theta)
    mx = (s * th).max(0, keepdims=True)
    e = np.exp(s * th - mx, dtype=np.float32)
    return s * (e / e.sum(0, keepdims=True, dtype=np.float32))


def dsl_epsilon(q, g, theta):
    """(eps, deviation): deviation = the largest relative deviation of the float32 restatement from fp64; eps = 4 x that"""
    x64, x32 = dsl64(scores64(q, g), theta), dsl_restated_f32(q, g, theta).astype(np.float64)
    dev = float(np.max(np.abs(x32 - x64) / np.abs(x64)))
    return 4.0 * dev, dev


def dsl_band(x, labels, eps):
    """``band`` with the per-element margin eps |x|: lo = #{x - eps|x| > x_l + eps|x_l|}, hi = #{x + eps|x| >= x_l - eps|x_l|}"""
    n = x.shape[0]
    lab = np.arange(n) if labels is None else np.asarray(labels)
    v = x[np.arange(n), lab][:, None]
    m, mv = eps * np.abs(x), eps * np.abs(v)
    return (x - m > v + mv).sum(1), (x + m >= v - mv).sum(1)


def check_band(tag, greater, equal, lo, hi):
    """lo <= greater, greater + equal <= hi, equal >= 1; where hi - lo == 1 the counts are pinned: greater == lo, equal == 1.
    Returns the share of queries with hi - lo > 1 (held to the band alone)."""
    greater, equal = np.asarray(greater, np.int64), np.asarray(equal, np.int64)
    assert greater.shape == lo.shape == hi.shape == equal.shape, tag
    bad = np.nonzero((greater < lo) | (greater + equal > hi) | (equal < 1))[0]
    assert bad.size == 0, f"{tag}: {bad.size} queries outside the band, first {bad[0]}: greater {greater[bad[0]]} equal " \
                          f"{equal[bad[0]]} band [{lo[bad[0]]}, {hi[bad[0]]}]"
    pinned = hi - lo == 1
    assert np.array_equal(greater[pinned], lo[pinned]) and (equal[pinned] == 1).all(), f"{tag}: a pinned query is off"
    return float((~pinned).mean())


BAND_SHAPES = [(257, 1031, 96), (515, 130, 40), (130, 515, 40)]        # (nq, ng, d)
AMBIGUOUS_CAP = 0.10                                                   # the share of queries the band may leave open, per case


@functools.lru_cache(maxsize=None)
def band_case(nq, ng, d, theta=100.0):
    """one real-valued case, computed once and shared (read-only) by the tests: inputs, labels (the diagonal where every query has
    one, i mod the other extent otherwise), delta, eps, and the (lo, hi) bands of both directions, simple and DSL"""
    q, g = real_inputs(nq, ng, d, seed=nq + ng)
    lab_q = None if nq <= ng else np.arange(nq) % ng
    lab_g = None if ng <= nq else np.arange(ng) % nq
    s = scores64(q, g)
    dl = delta(q, g)
    eps, dev = dsl_epsilon(q, g, theta)
    x = dsl64(s, theta)
    y = s * theta
    return dict(q=q, g=g, lab_q=lab_q, lab_g=lab_g, delta=dl, eps=eps, dev=dev, spread=float((y.max(0) - y.min(0)).max()),
                simple=(band(s, lab_q, dl), band(s.T, lab_g, dl)), dsl=(dsl_band(x, lab_q, eps), dsl_band(x.T, lab_g, eps)))


def tile_edges(n, tile):
    """the first and the last position of every tile of an extent (tiles are what the device's plan splits into runs)"""
    return sorted({p for t in range(0, n, tile) for p in (t, min(t + tile, n) - 1)})
