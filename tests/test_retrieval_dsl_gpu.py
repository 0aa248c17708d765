"""GPU: DSL-weighted top-k search (csrc/retrieval_stream.hip: xp_retrieval_dsl_stats, xp_retrieval_topk_dsl; utils/metrics.py:
dsl_stats, topk(dsl=...), search(dsl_of=...)) against tests/retrieval_dsl_ref.py.

    [x] neutral element     dsl = (0, 1), theta = 0 is the plain call bit for bit, both modes: the mode changes nothing but the value
    [x] the rank counts     lists and xp_retrieval_ranks_streamed's (greater, equal) agree position by position, both directions:
                            the statistics entry forms the rank call's internal bits, and x is dsl_x
    [x] shards              one statistics vector: shards == one shot bit for bit; search == its manual composition
    [x] exact grid          per-query statistics keep the order of s: indices exact; per-gallery: the list check
    [x] real-valued lists   both modes, k = 1, 10, 128: everything fp64 decides under eps; the two-walk search over three shards
    [x] the contract        guarded workspaces, outputs and statistics; accumulate; a side stream; run to run; refusals; fp32 / GPU only
"""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import retrieval_dsl_ref as D
from tests import retrieval_stream_ref as R
from tests.gpu_util import report
from tests.guarded import Guarded, GuardedWorkspaces

pytestmark = pytest.mark.gpu

TILE = 128
KS = (1, 10, 128)
# the smallest call | one query row | one gallery row | d % 4 != 0 | several tiles both ways | 5 statistic runs: the combine kernel |
# 16 gallery splits: topk_merge_kernel | ng == k at k = 128
SHAPES = [(1, 1, 1), (1, 130, 40), (130, 1, 40), (33, 257, 3), (257, 1031, 96), (515, 130, 40), (64, 2048, 512), (33, 128, 96)]


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _np(t):
    return None if t is None else t.cpu().numpy()


def _bits(t):
    a = t if isinstance(t, np.ndarray) else _np(t)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(a, b):
    """two (values, indices) or (mx, sum) pairs, bit for bit"""
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def case(kind, nq, ng, d):
    """inputs and labels of one shape, computed once and read-only.  "grid": exact-grid rows, those on the first and last position
    of every tile copies of one row (in q and in g), labels that walk those positions; "real": R.real_inputs, labels i mod the
    other extent.  theta: 0.25 on the grid (no underflow), 100 on real values"""
    if kind == "grid":
        eq, eg = R.tile_edges(nq, TILE), R.tile_edges(ng, TILE)
        q, g = R.grid_inputs(nq, ng, d, seed=31 * nq + ng + d, dup_q=[(p, eq[0]) for p in eq[1:]], dup_g=[(p, eg[0]) for p in eg[1:]])
        lab_q = np.array([eg[i % len(eg)] for i in range(nq)], dtype=np.int64)
        lab_g = np.array([eq[j % len(eq)] for j in range(ng)], dtype=np.int64)
        theta = D.GRID_THETA
    else:
        q, g = R.real_inputs(nq, ng, d, seed=nq + ng + d)
        lab_q, lab_g, theta = np.arange(nq) % ng, np.arange(ng) % nq, 100.0
    return dict(q=q, g=g, lab_q=lab_q, lab_g=lab_g, theta=theta)


def _cuts(ng, k):
    """shard borders just before, on and just behind tile borders in turn, every shard at least k rows"""
    assert {c % TILE for c in R.tile_edges(4 * TILE, TILE)} == {0, TILE - 1}
    cuts, prev = [], 0
    for c in (t * TILE + o for t, o in zip(range(1, ng // TILE + 1), itertools.cycle((-1, 0, 1)))):
        if c - prev >= k and ng - c >= k:
            cuts.append(c)
            prev = c
    return list(zip([0] + cuts, cuts + [ng]))


# ------------------------------------------------------------------------------------------------------- 1. the neutral element
@pytest.mark.parametrize("kind", ["grid", "real"])
@pytest.mark.parametrize("nq,ng,d", SHAPES)
def test_neutral_statistics_give_the_plain_call(nq, ng, d, kind):
    """theta = 0, mx = 0, sum = 1: fmaf(s, 0, -0) = +-0, expf(+-0) = 1, s * (1 / 1) = s"""
    from xpretrain_amd.utils import metrics
    c = case(kind, nq, ng, d)
    q, g = _dev(c["q"]), _dev(c["g"])
    for k in KS:
        if k > ng:
            continue
        plain = metrics.topk(q, g, k, index_base=3)
        for mode, n in (("gallery", ng), ("queries", nq)):
            st = (torch.zeros(n, device="cuda"), torch.ones(n, device="cuda"))
            got = metrics.topk(q, g, k, index_base=3, dsl=st, dsl_of=mode, theta=0.0)
            assert _same(got, plain), (mode, k)


# ---------------------------------------------------------------------------------------------------------- 2. the rank counts
def _agrees_with_counts(tag, vals, idx, greater, equal, labels):
    vals, idx = _bits(vals), _np(idx)
    k = vals.shape[1]
    fv = vals.view(np.float32)
    seen_ties = 0
    for i, (G, E, lab) in enumerate(zip(greater.tolist(), equal.tolist(), labels.tolist())):
        assert E >= 1, (tag, i)
        if G >= k:
            assert lab not in idx[i], (tag, i, "the label is listed although k candidates are above it")
            continue
        end = min(k, G + E)
        assert (vals[i, G:end] == vals[i, G]).all(), (tag, i, "the label's ties differ in bits")
        if G + E <= k:
            assert lab in idx[i, G:end], (tag, i, "the label is not among its ties")
        assert G == 0 or fv[i, G - 1] > fv[i, G], (tag, i, "the entry in front of the label's ties is not above them")
        assert G + E >= k or fv[i, G + E] < fv[i, G], (tag, i, "the entry behind the label's ties is not below them")
        seen_ties += E > 1
    return seen_ties


@pytest.mark.parametrize("kind", ["grid", "real"])
@pytest.mark.parametrize("nq,ng,d", SHAPES)
def test_lists_agree_with_the_rank_counts(nq, ng, d, kind):
    from xpretrain_amd.utils import metrics
    c = case(kind, nq, ng, d)
    q, g, th = _dev(c["q"]), _dev(c["g"]), c["theta"]
    st = metrics.dsl_stats(q, g, th)
    (gq, eq), (gg, eg) = metrics.rank_counts_streamed(q, g, c["lab_q"], c["lab_g"], dsl_theta=th)
    t2v = metrics.topk(q, g, min(128, ng), dsl=st, dsl_of="gallery", theta=th)
    v2t = metrics.topk(g, q, min(128, nq), dsl=st, dsl_of="queries", theta=th)
    ties = _agrees_with_counts(f"{kind} {nq}x{ng}x{d} t2v", *t2v, gq, eq, c["lab_q"])
    ties += _agrees_with_counts(f"{kind} {nq}x{ng}x{d} v2t", *v2t, gg, eg, c["lab_g"])
    if kind == "grid" and max(nq, ng) > TILE:
        assert ties > 0                                  # the planted duplicates: equal > 1 occurs


# ------------------------------------------------------------------------------------------------------------------- 3. shards
@pytest.mark.parametrize("nq,ng,d,k", [(257, 1031, 96, 10), (257, 1031, 96, 128), (64, 2048, 512, 128), (33, 257, 3, 10)])
def test_shards_equal_one_shot_given_the_statistics(nq, ng, d, k):
    from xpretrain_amd.utils import metrics
    c = case("real", nq, ng, d)
    q, g, th = _dev(c["q"]), _dev(c["g"]), c["theta"]
    cuts = _cuts(ng, k)
    assert len(cuts) >= 2 and all(b - a >= k for a, b in cuts)
    per_gallery, per_query = metrics.dsl_stats(q, g, th), metrics.dsl_stats(g, q, th)
    for mode, st in (("gallery", per_gallery), ("queries", per_query)):
        one = metrics.topk(q, g, k, dsl=st, dsl_of=mode, theta=th)
        for order in (cuts, cuts[::-1]):
            out = None
            for a, b in order:
                part = (st[0][a:b], st[1][a:b]) if mode == "gallery" else st
                out = metrics.topk(q, g[a:b], k, index_base=a, out=out, dsl=part, dsl_of=mode, theta=th)
            assert _same(out, one), (mode, order[0])


@pytest.mark.parametrize("nq,ng,d,k", [(257, 1031, 96, 10), (33, 257, 3, 10)])
def test_search_is_its_manual_composition(nq, ng, d, k):
    from xpretrain_amd.utils import metrics
    c = case("real", nq, ng, d)
    q, g, th = _dev(c["q"]), _dev(c["g"]), c["theta"]
    cuts = _cuts(ng, k)
    shards = [g[a:b] for a, b in cuts]
    out = None
    for (a, b), shard in zip(cuts, shards):                 # one walk: each shard's own statistics over the queries
        out = metrics.topk(q, shard, k, index_base=a, out=out, dsl=metrics.dsl_stats(q, shard, th), dsl_of="gallery", theta=th)
    assert _same(metrics.search(q, shards, k, dsl_of="gallery", theta=th), out)
    assert _same(metrics.search(q, lambda: iter(shards), k, dsl_of="gallery", theta=th), out)
    st = None
    for shard in shards:                                    # two walks: the queries' statistics over all shards, then the ranking
        st = metrics.dsl_stats(shard, q, th, out=st)
    out = None
    for (a, b), shard in zip(cuts, shards):
        out = metrics.topk(q, shard, k, index_base=a, out=out, dsl=st, dsl_of="queries", theta=th)
    assert _same(metrics.search(q, shards, k, dsl_of="queries", theta=th), out)
    assert _same(metrics.search(q, lambda: iter(shards), k, dsl_of="queries", theta=th), out)
    with pytest.raises(TypeError, match="one-shot iterator"):
        metrics.search(q, iter(shards), k, dsl_of="queries", theta=th)
    assert _same(metrics.search(q, iter(shards), k), metrics.topk(q, g, k))          # the plain walk takes what it always took


# --------------------------------------------------------------------------------------------------------------- 4. exact grid
@pytest.mark.parametrize("nq,ng,d", D.GRID_SHAPES)
def test_exact_grid(nq, ng, d):
    from xpretrain_amd.utils import metrics
    c = D.grid_case(nq, ng, d)
    q, g, th = _dev(c["q"]), _dev(c["g"]), D.GRID_THETA
    per_gallery, per_query = metrics.dsl_stats(q, g, th), metrics.dsl_stats(g, q, th)
    for k in KS:
        if k > ng:
            continue
        # per-query statistics: x grows with s, so the list is the stable sort of the exact scores
        x = D.x64(c["q"], c["g"], th, "queries")
        eps, _ = D.epsilon(c["q"], c["g"], th, "queries")
        vals, idx = metrics.topk(q, g, k, dsl=per_query, dsl_of="queries", theta=th)
        want_i = R.topk(c["units"], k)[1]
        assert np.array_equal(_np(idx), want_i)
        xi = np.take_along_axis(x, want_i, 1)
        assert (np.abs(_np(vals).astype(np.float64) - xi) <= eps * np.abs(xi)).all()
        # per-gallery statistics: duplicates still tie exactly, everything else is held to what fp64 decides
        x = D.x64(c["q"], c["g"], th, "gallery")
        eps, _ = D.epsilon(c["q"], c["g"], th, "gallery")
        vals, idx = metrics.topk(q, g, k, dsl=per_gallery, dsl_of="gallery", theta=th)
        share = D.check_list(f"grid {nq}x{ng}x{d} gallery k={k}", _np(vals), _np(idx), x, eps)
        print(f"dsl top-k grid {nq}x{ng}x{d} gallery k={k}: open share {share:.4f}, eps {eps:.2e}")


# --------------------------------------------------------------------------------------------------------- 5. real-valued lists
@pytest.mark.parametrize("mode", D.MODES)
@pytest.mark.parametrize("nq,ng,d", R.BAND_SHAPES)
def test_real_valued_lists(nq, ng, d, mode):
    from xpretrain_amd.utils import metrics
    c = R.band_case(nq, ng, d)
    x, eps, dev = D.band_x64(nq, ng, d, mode)
    q, g = _dev(c["q"]), _dev(c["g"])
    st = metrics.dsl_stats(q, g, 100.0) if mode == "gallery" else metrics.dsl_stats(g, q, 100.0)
    for k in KS:
        if k > ng:
            continue
        vals, idx = metrics.topk(q, g, k, dsl=st, dsl_of=mode, theta=100.0)
        tag = f"dsl top-k {nq}x{ng}x{d} {mode} k={k}"
        report(f"{tag}: values / fp64 (tol = eps = 4 x the float32 restatement's {dev:.2e})",
               vals.double().cpu() / torch.from_numpy(np.take_along_axis(x, _np(idx), 1)), torch.ones(nq, k, dtype=torch.float64), eps)
        share = D.check_list(tag, _np(vals), _np(idx), x, eps)
        report(f"{tag}: 1 + the share of positions fp64 leaves open (tol = the cap)", torch.tensor([1.0 + share]), torch.ones(1),
               R.AMBIGUOUS_CAP)
        assert share <= R.AMBIGUOUS_CAP


@pytest.mark.parametrize("nq,ng,d", R.BAND_SHAPES)
def test_two_walk_search_over_three_shards(nq, ng, d):
    """eps from the float32 restatement of the SAME fold: the gallery folded into the queries' statistics in these three shards"""
    from xpretrain_amd.utils import metrics
    c = R.band_case(nq, ng, d)
    k = 10
    cuts = [(0, ng // 3 + 1), (ng // 3 + 1, 2 * ng // 3 + 3), (2 * ng // 3 + 3, ng)]
    assert all(b - a >= k for a, b in cuts)
    eps, dev = D.epsilon(c["q"], c["g"], 100.0, "queries", cuts)
    x = D.band_x64(nq, ng, d, "queries")[0]
    q, g = _dev(c["q"]), _dev(c["g"])
    vals, idx = metrics.search(q, [g[a:b] for a, b in cuts], k, dsl_of="queries", theta=100.0)
    tag = f"dsl search {nq}x{ng}x{d} queries, three shards, k={k}"
    report(f"{tag}: values / fp64 (tol = eps = 4 x the folded float32 restatement's {dev:.2e})",
           vals.double().cpu() / torch.from_numpy(np.take_along_axis(x, _np(idx), 1)), torch.ones(nq, k, dtype=torch.float64), eps)
    share = D.check_list(tag, _np(vals), _np(idx), x, eps)
    report(f"{tag}: 1 + the share of positions fp64 leaves open (tol = the cap)", torch.tensor([1.0 + share]), torch.ones(1), R.AMBIGUOUS_CAP)
    assert share <= R.AMBIGUOUS_CAP


# ------------------------------------------------------------------------------------------------------------- 6. the contract
def _c_stats(L, H, over, of, theta, acc, mx, sm, ws, nbytes):
    return L.lib().xp_retrieval_dsl_stats(H._p(over), H._p(of), over.shape[0], of.shape[0], over.shape[1], theta, acc, H._p(mx), H._p(sm),
                                          H._p(ws), nbytes, H._stream())


@pytest.mark.parametrize("n_over,n_of,d", [(515, 130, 40), (257, 1031, 96), (100, 130, 40), (33, 257, 3)])
def test_stats_in_guarded_buffers(n_over, n_of, d):
    """the C entry with the workspace at exactly its stated size between poisoned guards, the statistics in guard buffers; a fresh
    call, then an accumulating one (one split and several: both go through the partials and the combine kernel)"""
    from xpretrain_amd import _lib as L, hip_ops as H
    c = case("real", n_over, n_of, d)
    over, of = _dev(c["q"]), _dev(c["g"])
    want = H.retrieval_dsl_stats(over, of, 100.0)
    half = n_over // 2
    want_acc = H.retrieval_dsl_stats(over[half:], of, 100.0, out=H.retrieval_dsl_stats(over[:half], of, 100.0))
    gm, gs = Guarded(1, n_of, torch.float32), Guarded(1, n_of, torch.float32)
    am, asum = Guarded(1, n_of, torch.float32), Guarded(1, n_of, torch.float32)
    with GuardedWorkspaces() as gw:
        for rows, acc, (m, s) in ((over, 0, (gm, gs)), (over[:half], 0, (am, asum)), (over[half:], 1, (am, asum))):
            need = L.lib().xp_retrieval_dsl_stats_workspace_bytes(rows.shape[0], n_of, d)
            ws = H.workspace(need, of.device, "retrieval_dsl_stats")
            assert ws.numel() == need
            L.check(_c_stats(L, H, rows, of, 100.0, acc, m.mat, s.mat, ws, need), "xp_retrieval_dsl_stats")
        gw.check()
        again = H.retrieval_dsl_stats(over, of, 100.0)                    # the wrapper asks for the same bytes
        gw.check()
    assert gw.records[-1][1] == gw.records[0][1] and [r[0] for r in gw.records] == ["retrieval_dsl_stats"] * 4
    for guard in (gm, gs, am, asum):
        guard.check(f"dsl stats {n_over}x{n_of}x{d}", 1, n_of)
    assert _same((gm.mat.view(-1), gs.mat.view(-1)), want) and _same(again, want)
    assert _same((am.mat.view(-1), asum.mat.view(-1)), want_acc)
    # accumulated: the maximum is exact; the sum is the same n_over positive terms in another order and rescaled once more --
    # within (n - 1) 2^-24 of the exact sum each, plus a few roundings of the rescaling
    assert np.array_equal(_bits(am.mat.view(-1)), _bits(want[0]))
    one, acc = _np(want[1]).astype(np.float64), _np(asum.mat.view(-1)).astype(np.float64)
    tol = (2 * n_over + 16) * 2.0 ** -24
    report(f"dsl stats {n_over}x{n_of}x{d}: accumulated sum / one-shot sum", torch.from_numpy(acc / one), torch.ones(n_of, dtype=torch.float64), tol)
    assert (np.abs(acc - one) <= tol * one).all() and np.isfinite(one).all() and (one >= 1).all()


@pytest.mark.parametrize("mode", D.MODES)
@pytest.mark.parametrize("nq,ng,d,k", [(64, 2048, 512, 128), (257, 1031, 96, 10)])
def test_topk_dsl_in_guarded_buffers(nq, ng, d, k, mode):
    from xpretrain_amd import _lib as L, hip_ops as H
    c = case("real", nq, ng, d)
    q, g = _dev(c["q"]), _dev(c["g"])
    st = H.retrieval_dsl_stats(q, g, 100.0) if mode == "gallery" else H.retrieval_dsl_stats(g, q, 100.0)
    want = H.retrieval_topk(q, g, k, dsl=st, dsl_of=mode)
    n = st[0].numel()
    gm, gs = Guarded(1, n, torch.float32), Guarded(1, n, torch.float32)        # the statistics end where the guard begins
    gm.mat.view(-1).copy_(st[0])
    gs.mat.view(-1).copy_(st[1])
    gv, gi = Guarded(nq, k, torch.float32), Guarded(nq, 2 * k, torch.float32)
    idx = gi.mat.view(torch.int64)
    with GuardedWorkspaces() as gw:
        need = L.lib().xp_retrieval_topk_workspace_bytes(nq, ng, d, k)
        ws = H.workspace(need, q.device, "retrieval_topk")
        assert ws.numel() == need
        L.check(L.lib().xp_retrieval_topk_dsl(H._p(q), H._p(g), nq, ng, d, k, 0, 0, 100.0, H.DSL_OF[mode], H._p(gm.mat), H._p(gs.mat),
                                              H._p(gv.mat), H._p(idx), H._p(ws), need, H._stream()), "xp_retrieval_topk_dsl")
        gw.check()
        again = H.retrieval_topk(q, g, k, dsl=st, dsl_of=mode)
        gw.check()
    assert [r[1] for r in gw.records] == [need, need]
    gv.check("topk dsl vals", nq, k)
    gi.check("topk dsl idx", nq, 2 * k)
    assert _same((gv.mat, idx), want) and _same(again, want) and not torch.isnan(gv.mat).any()


def test_refusals_leave_the_outputs_untouched():
    from xpretrain_amd import _lib as L, hip_ops as H
    nq, ng, d, k = 33, 257, 3, 10
    c = case("real", nq, ng, d)
    q, g = _dev(c["q"]), _dev(c["g"])
    st = H.retrieval_dsl_stats(q, g, 100.0)
    ws = H.workspace(1 << 20, q.device, "retrieval_topk")
    gv, gi = Guarded(nq, k, torch.float32), Guarded(nq, 2 * k, torch.float32)
    gm, gs = Guarded(1, ng, torch.float32), Guarded(1, ng, torch.float32)
    GAL = L.XP_DSL_OF_GALLERY

    def topk(theta=100.0, of=GAL, mx=st[0], sm=st[1], k=k, ng=ng, nbytes=1 << 20):
        return L.lib().xp_retrieval_topk_dsl(H._p(q), H._p(g), nq, ng, d, k, 0, 0, theta, of, H._p(mx), H._p(sm), H._p(gv.mat),
                                             H._p(gi.mat), H._p(ws), nbytes, H._stream())

    def stats(theta=100.0, n_over=nq, mx=gm.mat, nbytes=1 << 20):
        return L.lib().xp_retrieval_dsl_stats(H._p(q), H._p(g), n_over, ng, d, theta, 0, H._p(mx), H._p(gs.mat), H._p(ws), nbytes, H._stream())
    for rc in (topk(theta=float("inf")), topk(theta=float("nan")), topk(of=0), topk(of=3), topk(mx=None), topk(sm=None), topk(k=0),
               topk(k=129), topk(k=11, ng=10), topk(nbytes=0), stats(theta=float("inf")), stats(n_over=0), stats(mx=None), stats(nbytes=0)):
        assert rc == -1, L.lib().xp_last_error().decode()
    torch.cuda.synchronize()
    for guard, cols in ((gv, k), (gi, 2 * k), (gm, ng), (gs, ng)):
        guard.check("refused", 0, cols)                              # not one element written


def test_side_stream_and_run_to_run():
    from xpretrain_amd.utils import metrics
    c = R.band_case(515, 130, 40)
    q, g = _dev(c["q"]), _dev(c["g"])

    def run():
        out = []
        for mode, st in (("gallery", metrics.dsl_stats(q, g)), ("queries", metrics.dsl_stats(g, q))):
            out += [*st, *metrics.topk(q, g, 100, dsl=st, dsl_of=mode)]
        return out + [*metrics.search(q, [g[:70], g[70:]], 10, dsl_of="queries")]
    first = run()
    for _ in range(2):
        assert _same(run(), first)
    torch.cuda.synchronize()
    # torch hands out its 32 pooled side streams round robin: taking all 32 leaves the pool where it was, so this test does not
    # change which pooled stream any later test of the session is given
    s = [torch.cuda.Stream() for _ in range(32)][0]
    with torch.cuda.stream(s):
        side = run()
    s.synchronize()
    assert _same(side, first)


def test_only_fp32_gpu_inputs():
    from xpretrain_amd.utils import metrics
    q, g = torch.zeros(4, 8, device="cuda"), torch.zeros(16, 8, device="cuda")
    st = metrics.dsl_stats(q, g)
    for bad in (q.bfloat16(), q.double(), q.cpu()):
        for f in (lambda: metrics.topk(bad, g, 2, dsl=st), lambda: metrics.dsl_stats(bad, g), lambda: metrics.dsl_stats(g, bad),
                  lambda: metrics.search(bad, [g], 2, dsl_of="gallery"), lambda: metrics.search(bad, [g], 2, dsl_of="queries")):
            with pytest.raises(RuntimeError, match="float32|no CPU path"):
                f()
    with pytest.raises(ValueError, match="k=17"):
        metrics.topk(q, g, 17, dsl=st)
    for bad in ((st[0][:4], st[1][:4]), (st[0], st[1][:4]), st[0], (st[0].double(), st[1]), (st[0].cpu(), st[1]), (st[0][::2], st[1][::2])):
        with pytest.raises((ValueError, TypeError), match="length 16"):
            metrics.topk(q, g, 2, dsl=bad, dsl_of="gallery")
    with pytest.raises(ValueError, match="length 4"):
        metrics.topk(q, g, 2, dsl=st, dsl_of="queries")
    with pytest.raises(ValueError, match="gallery.*queries"):
        metrics.topk(q, g, 2, dsl=st, dsl_of="rows")
    with pytest.raises((ValueError, TypeError), match="length 16"):
        metrics.dsl_stats(q, g, out=(st[0][:4], st[1]))
