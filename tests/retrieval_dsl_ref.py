"""numpy reference of DSL-weighted top-k search (csrc/retrieval_stream.hip: xp_retrieval_dsl_stats, xp_retrieval_topk_dsl) -- plain
helper module, no tests of its own.  Built on tests/retrieval_stream_ref.py (``R``), which stays as it is.

The re-ranked score of query i and gallery row j is x_ij = s_ij exp(theta s_ij - mx) / sum, s = q g^T, in one of two modes:

* ``"gallery"`` (the reference's t2v): (mx, sum) belong to gallery row j and run over all queries -- x = R.dsl64(s): the rows of
  ``sim * np_softmax(sim * theta, axis=0)``, sim = cal_cossim(queries, gallery);
* ``"queries"`` (the reference's v2t): (mx, sum) belong to query i and run over the whole gallery -- x = R.dsl64(s^T)^T: the rows of
  the transpose of the same expression with sim = cal_cossim(gallery, queries).

REAL-VALUED LISTS.  A device value may differ from fp64 by eps |x| (eps = 4 x the largest relative deviation from fp64 of a numpy
float32 restatement of the formula on the same inputs -- R.dsl_epsilon's rule; ``epsilon`` is that function with entries that are
exactly zero on both sides left out, and with the statistics of a shard-by-shard fold where the test folds).  ``check_list`` holds a
device list to everything fp64 decides under those margins and returns the share of positions it leaves open."""
import functools

import numpy as np

from tests import retrieval_stream_ref as R

MODES = ("gallery", "queries")


# ------------------------------------------------------------------------------------------------------------------------ fp64
def stats64(over, of, theta):
    """(mx, sum) per row of ``of`` over the rows of ``over``, fp64"""
    y = theta * R.scores64(over, of)
    mx = y.max(0)
    return mx, np.exp(y - mx).sum(0)


def x64(q, g, theta, dsl_of):
    """[nq, ng] fp64: the re-ranked score of every (query, gallery row) pair"""
    s = R.scores64(q, g)
    return R.dsl64(s, theta) if dsl_of == "gallery" else R.dsl64(s.T, theta).T


def topk64(q, g, theta, dsl_of, k, index_base=0):
    return R.topk(x64(q, g, theta, dsl_of), k, index_base)


# ------------------------------------------------------------------------------------------------------- float32 restatements
def stat_merge32(m, s, m2, s2):
    """(m, s) + (m2, s2) in float32, the first operand first: (max, s e^(m - max) + s2 e^(m2 - max))"""
    mm = np.maximum(m, m2)
    return mm, (s * np.exp(m - mm, dtype=np.float32) + s2 * np.exp(m2 - mm, dtype=np.float32)).astype(np.float32)


def stats32(over_shards, of, theta):
    """float32 (mx, sum) per row of ``of``, the rows of ``over`` arriving as a list of shards that are folded in order -- one shard:
    dsl_rerank_kernel's two sweeps (R.dsl_restated_f32's statistics); several: an accumulated fold"""
    th, m, sm = np.float32(theta), None, None
    for shard in over_shards:
        y = (shard @ of.T).astype(np.float32) * th
        m2 = y.max(0)
        s2 = np.exp(y - m2, dtype=np.float32).sum(0, dtype=np.float32)
        m, sm = (m2, s2) if m is None else stat_merge32(m, sm, m2, s2)
    return m, sm


def x32(q, g, theta, dsl_of, mx, sm):
    """float32 s * (exp(s theta - mx) / sum) on the float32 product of the features, with the given float32 statistics"""
    s = (q @ g.T).astype(np.float32)
    mx, sm = (mx[None, :], sm[None, :]) if dsl_of == "gallery" else (mx[:, None], sm[:, None])
    return s * (np.exp(s * np.float32(theta) - mx, dtype=np.float32) / sm)


def epsilon(q, g, theta, dsl_of, gallery_shards=None):
    """(eps, deviation) of mode ``dsl_of``: deviation = the largest relative deviation from fp64 of the float32 restatement, eps =
    4 x that.  ``gallery_shards`` (mode "queries" only): the (first, last + 1) row ranges in which the gallery is folded into the
    per-query statistics.  Entries where fp64 and float32 are both exactly zero (a zero score) are left out"""
    if dsl_of == "gallery":
        assert gallery_shards is None
        st = stats32([q], g, theta)
    else:
        st = stats32([g[a:b] for a, b in (gallery_shards or [(0, g.shape[0])])], q, theta)
    want, got = x64(q, g, theta, dsl_of), x32(q, g, theta, dsl_of, *st).astype(np.float64)
    live = (want != 0) | (got != 0)
    dev = float(np.max(np.abs(got[live] - want[live]) / np.abs(want[live]))) if live.any() else 0.0
    return 4.0 * dev, dev


# ------------------------------------------------------------------------------------------------------------- the list check
def open_positions(x, k, eps):
    """[n, k] bool: position p of the fp64 order of row i is OPEN unless the margins separate its entry from both fp64 neighbours
    (position k, the best excluded candidate, is a neighbour of position k - 1).  x - eps|x| and x + eps|x| both grow with x, so a
    separated entry has exactly p candidates certainly above it and every other certainly below: the device holds it at p"""
    n, m = x.shape
    order = np.argsort(-x, axis=1, kind="stable")[:, :min(k + 1, m)]
    v = np.take_along_axis(x, order, 1)
    lo, hi = v - eps * np.abs(v), v + eps * np.abs(v)
    apart = lo[:, :-1] > hi[:, 1:]                       # entry p certainly above entry p + 1
    above = np.concatenate([np.ones((n, 1), bool), apart], 1)[:, :k]
    below = np.concatenate([apart, np.ones((n, 1), bool)], 1)[:, :k]     # (m == k: nothing follows the last position)
    return ~(above & below)


def check_list(tag, vals, idx, x, eps, index_base=0):
    """a device list (vals [n, k] float32, idx [n, k] int64) against the fp64 matrix x [n, m].  Per query: indices distinct and in
    range; values descending, equal values by ascending index; |v_p - x[i_p]| <= eps |x[i_p]|; no excluded candidate's lower bound
    x - eps|x| above an included one's upper bound x + eps|x| (the device ranks every included entry at or above every excluded
    one); every position that is not open holds the fp64 index.  Returns the share of open positions"""
    vals, idx = np.asarray(vals, np.float64), np.asarray(idx, np.int64) - index_base
    n, m = x.shape
    k = vals.shape[1]
    assert vals.shape == idx.shape == (n, k) and k <= m, f"{tag}: shapes {vals.shape} {idx.shape} for x {x.shape}"
    assert ((idx >= 0) & (idx < m)).all(), f"{tag}: an index out of range"
    assert (np.diff(np.sort(idx, axis=1), axis=1) > 0).all(), f"{tag}: an index listed twice"
    dv, di = np.diff(vals, axis=1), np.diff(idx, axis=1)
    assert ((dv < 0) | ((dv == 0) & (di > 0))).all(), f"{tag}: the list is not in order (value descending, ties by index)"
    xi = np.take_along_axis(x, idx, 1)
    bad = np.abs(vals - xi) > eps * np.abs(xi)
    assert not bad.any(), f"{tag}: {bad.sum()} values beyond eps = {eps:.2e} of fp64, worst " \
                          f"{np.max(np.abs(vals - xi)[bad] / np.abs(xi)[bad]):.2e}"
    if k < m:
        inside = np.zeros((n, m), bool)
        np.put_along_axis(inside, idx, True, 1)
        best_out = np.where(inside, -np.inf, x - eps * np.abs(x)).max(1)
        worst_in = (xi + eps * np.abs(xi)).min(1)
        assert (best_out <= worst_in).all(), f"{tag}: {(best_out > worst_in).sum()} queries miss a better candidate"
    is_open = open_positions(x, k, eps)
    want = np.argsort(-x, axis=1, kind="stable")[:, :k]
    wrong = ~is_open & (idx != want)
    assert not wrong.any(), f"{tag}: {wrong.sum()} decided positions hold another index than fp64's"
    return float(is_open.mean())


# ---------------------------------------------------------------------------------------------------------------------- cases
GRID_THETA = 0.25
GRID_SHAPES = [(1, 130, 40), (130, 1, 40), (257, 1031, 40), (515, 130, 40)]          # exact grid, d = 40


@functools.lru_cache(maxsize=None)
def grid_case(nq, ng, d=40):
    """exact-grid inputs (entries k/8: scores are multiples of 1/64 within +-10) whose gallery rows on the first and last position of
    every 128-row tile are copies of one row; the int64 scores; computed once, read-only"""
    eg = R.tile_edges(ng, 128)
    q, g = R.grid_inputs(nq, ng, d, seed=7000 + 10 * nq + ng, dup_g=[(p, eg[0]) for p in eg[1:]])
    return dict(q=q, g=g, units=R.grid_scores(q, g))


@functools.lru_cache(maxsize=None)
def band_x64(nq, ng, d, dsl_of, theta=100.0):
    """(x64, eps, deviation) of R.band_case(nq, ng, d) in mode ``dsl_of``; computed once, read-only"""
    c = R.band_case(nq, ng, d, theta)
    return (x64(c["q"], c["g"], theta, dsl_of), *epsilon(c["q"], c["g"], theta, dsl_of))
