"""Retrieval metrics on the device (reference: ``src/utils/metrics.py`` and ``validate`` in
``src/tasks/run_video_retrieval.py:123-203``).

Same function names and return tuples as the reference -- ``cal_cossim``, ``np_softmax`` (axis 0 only, the one DSL
uses), ``compute_metrics``, ``compute_metrics_multi`` -- but they take and keep GPU tensors: the similarity GEMM, the
dual-softmax re-rank and the rank counting run as HIP kernels; only two int32 vectors of length n_queries come back to
the host for the final recall / median / mean arithmetic.  There is no CPU path.
"""
import numpy as np
import torch

from .. import _lib as L
from .. import hip_ops as H


def _f32(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor (xpretrain_amd has no CPU path)")
    return t.contiguous().float()


def cal_cossim(feats1: torch.Tensor, feats2: torch.Tensor) -> torch.Tensor:
    """sim[i][j] = feats1[i] . feats2[j]   (metrics.py:3-5)"""
    return H.sim_matrix(_f32(feats1, "feats1"), _f32(feats2, "feats2"))


def _col_softmax(sim: torch.Tensor, theta: float, multiply: bool) -> torch.Tensor:
    out = _f32(sim, "sim").clone()
    L.check(L.lib().xp_dsl_rerank(H._p(out), out.shape[0], out.shape[1], float(theta), int(multiply), H._stream()),
            "xp_dsl_rerank")
    return out


def dsl_rerank(sim: torch.Tensor, theta: float = 100.0) -> torch.Tensor:
    """``sim * np_softmax(sim * theta, axis=0)`` (run_video_retrieval.py:170-171); returns a new tensor."""
    return _col_softmax(sim, theta, True)


def np_softmax(X: torch.Tensor, theta: float = 1.0, axis=0) -> torch.Tensor:
    """metrics.py:7-39 for the one case the path uses: softmax over axis 0 of a 2-D matrix."""
    if axis != 0 or X.dim() != 2:
        raise NotImplementedError("np_softmax: only axis=0 of a 2-D matrix (the DSL use) is on the HIP path")
    return _col_softmax(X, theta, False)


def _rank_counts(x: torch.Tensor, labels=None, transpose=False):
    x = _f32(x, "sim")
    n, m = x.shape
    q = m if transpose else n
    lab = None
    if labels is not None:
        lab = torch.as_tensor(labels, dtype=torch.int64, device=x.device).contiguous()
        if lab.numel() != q:
            raise ValueError("labels must have one entry per query")
    greater = torch.empty(q, dtype=torch.int32, device=x.device)
    equal = torch.empty(q, dtype=torch.int32, device=x.device)
    L.check(L.lib().xp_retrieval_ranks(H._p(x), H._p(lab) if lab is not None else None, n, m, int(transpose),
                                       H._p(greater), H._p(equal), H._stream()), "xp_retrieval_ranks")
    return greater.cpu().numpy(), equal.cpu().numpy()


def _summarise(greater, equal):
    # np.where(sorted - label == 0) lists EVERY sorted position that ties the label (metrics.py:45-47)
    ind = np.concatenate([np.arange(g, g + e) for g, e in zip(greater, equal)]) if (equal != 1).any() else greater
    r1 = float(np.sum(ind == 0)) / len(ind)
    r5 = float(np.sum(ind < 5)) / len(ind)
    r10 = float(np.sum(ind < 10)) / len(ind)
    return r1, r5, r10, np.median(ind) + 1, np.mean(ind) + 1


def compute_metrics(x: torch.Tensor):
    """(R@1, R@5, R@10, median rank, mean rank) of the diagonal entries of each ROW (metrics.py:41-53)."""
    return _summarise(*_rank_counts(x))


def compute_metrics_multi(x: torch.Tensor, t2v_labels_list):
    return _summarise(*_rank_counts(x, labels=t2v_labels_list))


def retrieval_metrics(text_feats: torch.Tensor, vis_feats: torch.Tensor):
    """The body of ``validate`` (run_video_retrieval.py:163-188): returns {setting: {direction: metrics}} for the
    'simple' and 'DSL' settings; the v2t direction ranks the columns of the same matrix (no transposed copy)."""
    sim = cal_cossim(text_feats, vis_feats)
    out = {}
    for setting in ("simple", "DSL"):
        if setting == "DSL":
            sim = dsl_rerank(sim, 100.0)
        out[setting] = {"v2t": _summarise(*_rank_counts(sim, transpose=True)), "t2v": _summarise(*_rank_counts(sim))}
    return out


# ---- retrieval at gallery scale: the same evaluation, and top-k search, without the [queries, gallery] matrix -----------------
def _feats(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor (xpretrain_amd has no CPU path)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: expected float32 features, got {t.dtype} (ranks turn on differences of 1e-6)")
    return t.contiguous()


def rank_counts_streamed(text_feats, vis_feats, labels=None, v2t_labels=None, dsl_theta=None):
    """((greater, equal) of the t2v direction, (greater, equal) of the v2t direction) as numpy int32 vectors -- what
    ``_rank_counts`` gives for the rows and for the columns of ``cal_cossim(text_feats, vis_feats)`` (re-ranked with
    ``dsl_rerank(sim, dsl_theta)`` when ``dsl_theta`` is given), computed tile by tile from the features in one pass.
    ``labels`` [n_text]: each text's video (default: the diagonal); ``v2t_labels`` [n_video]: each video's text."""
    q, g = _feats(text_feats, "text_feats"), _feats(vis_feats, "vis_feats")
    gq, eq, gg, eg = H.retrieval_ranks_streamed(q, g, labels, v2t_labels, dsl=dsl_theta is not None,
                                                theta=100.0 if dsl_theta is None else float(dsl_theta))
    return (gq.cpu().numpy(), eq.cpu().numpy()), (gg.cpu().numpy(), eg.cpu().numpy())


def retrieval_metrics_streamed(text_feats, vis_feats, labels=None, v2t_labels=None, theta=100.0):
    """``retrieval_metrics`` without the matrix: the same {setting: {direction: (R@1, R@5, R@10, median, mean)}}, memory and
    traffic O(n_text + n_video).  Two calls: 'simple', then 'DSL'."""
    out = {}
    for setting, th in (("simple", None), ("DSL", theta)):
        t2v, v2t = rank_counts_streamed(text_feats, vis_feats, labels, v2t_labels, dsl_theta=th)
        out[setting] = {"v2t": _summarise(*v2t), "t2v": _summarise(*t2v)}
    return out


def dsl_stats(over_feats, of_feats, theta=100.0, out=None):
    """(mx, sum), fp32 GPU vectors with one entry per row of ``of_feats``: the dual softmax's statistics over the rows of
    ``over_feats`` -- ``mx[j] = max_i theta s_ij``, ``sum[j] = sum_i exp(theta s_ij - mx[j])`` with ``s = cal_cossim(over_feats,
    of_feats)``, i.e. ``np_softmax(s * theta, axis=0) = exp(theta s - mx) / sum``.  ``out`` = (mx, sum) of an earlier call over other
    rows of ``over_feats``: they lead the fold and the pair is updated in place, so an ``over`` set can arrive in shards."""
    return H.retrieval_dsl_stats(_feats(over_feats, "over_feats"), _feats(of_feats, "of_feats"), theta, out)


def topk(query_feats, gallery_feats, k, index_base=0, out=None, dsl=None, dsl_of="gallery", theta=100.0):
    """(values [n_query, k] fp32, indices [n_query, k] int64): each query's k best gallery rows by dot product, best first, ties to
    the lowest index; ``index_base`` is added to every index.  ``out`` = (values, indices) of an earlier call: its entries compete
    with this gallery's and the pair is updated in place -- shard by shard gives exactly the one-shot result.

    ``dsl`` = (mx, sum) from ``dsl_stats``: rank by the DSL setting of ``validate`` instead (run_video_retrieval.py:157-171), exact
    given those statistics.
    ``dsl_of="gallery"`` (t2v, queries = texts; statistics of length n_gallery from ``dsl_stats(query_feats, gallery_feats)``): the
    rows of ``sim * np_softmax(sim*theta, axis=0)`` with ``sim = cal_cossim(query_feats, gallery_feats)``.
    ``dsl_of="queries"`` (v2t, queries = videos; statistics of length n_query from ``dsl_stats(gallery_feats, query_feats)`` over
    the WHOLE gallery): the rows of the transpose of that expression with ``sim = cal_cossim(gallery_feats, query_feats)``."""
    return H.retrieval_topk(_feats(query_feats, "query_feats"), _feats(gallery_feats, "gallery_feats"), k, index_base, out, dsl=dsl,
                            dsl_of=dsl_of, theta=theta)


def search(query_feats, shards, k, dsl_of=None, theta=100.0):
    """``topk`` over a gallery that arrives as an iterable of [rows, d] shards; indices count rows across the shards.  Every shard
    needs at least k rows (a shard's own best k are what it can contribute).

    ``dsl_of="gallery"``: the rows of ``sim * np_softmax(sim*theta, axis=0)`` with ``sim = cal_cossim(query_feats, gallery)`` (the
    reference's t2v).  One walk: a gallery row's statistics need the queries only, so each shard gets its own from ``dsl_stats``.
    ``dsl_of="queries"``: the rows of the transpose of that expression with ``sim = cal_cossim(gallery, query_feats)`` (the
    reference's v2t).  Two walks: a query's statistics run over the whole gallery and must be complete before any candidate can be
    ranked, so ``shards`` must be re-iterable -- a sequence, or a zero-argument callable that returns a fresh iterator."""
    if dsl_of not in (None, "gallery", "queries"):
        raise ValueError(f"search: dsl_of must be None, 'gallery' or 'queries', got {dsl_of!r}")
    walk = shards if callable(shards) else (lambda: shards)
    if dsl_of == "queries" and not callable(shards) and iter(shards) is shards:
        raise TypeError("search: dsl_of='queries' walks the gallery twice (each query's statistics over the whole gallery, then the "
                        "ranking) and a one-shot iterator cannot be rewound: pass a sequence, or a zero-argument callable that returns "
                        "a fresh iterator")
    stats = None
    if dsl_of == "queries":
        for shard in walk():
            stats = dsl_stats(shard, query_feats, theta, out=stats)
        if stats is None:
            raise ValueError("search: no gallery shards")
    out, base = None, 0
    for shard in walk():
        if dsl_of is None:
            out = topk(query_feats, shard, k, index_base=base, out=out)
        else:
            st = stats if dsl_of == "queries" else dsl_stats(query_feats, shard, theta)
            out = topk(query_feats, shard, k, index_base=base, out=out, dsl=st, dsl_of=dsl_of, theta=theta)
        base += shard.shape[0]
    if out is None:
        raise ValueError("search: no gallery shards")
    return out
