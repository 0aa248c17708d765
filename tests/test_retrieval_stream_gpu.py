"""GPU: the streamed retrieval kernels (csrc/retrieval_stream.hip: xp_retrieval_ranks_streamed, xp_retrieval_topk) and their Python
surface (utils/metrics.py) against tests/retrieval_stream_ref.py.

    [x] exact grid        counts in both directions (diagonal and explicit labels) and top-k (k = 1, 10, 128; ng == k; index_base;
                          a three-shard accumulate chain against the one-shot call) met EXACTLY; duplicate rows and the labels'
                          columns sit on the first and last position of every tile of the device's plan
    [x] real-valued band  simple and DSL, both directions, at the three shapes of the reference; eps printed
    [x] the fixture       retrieval_metrics_streamed under the acceptance rule of test_metrics_against_reference_fixture
    [x] position independence, run-to-run bit equality, guarded workspaces and outputs, a non-default stream, a gallery beyond 4 GiB
"""
import functools

import numpy as np
import pytest
import torch

from tests import retrieval_stream_ref as R
from tests.gpu_util import report
from tests.guarded import Guarded, GuardedWorkspaces

pytestmark = pytest.mark.gpu

TILE = 128
GRID_SHAPES = [(1, 1, 1), (1, 130, 40), (130, 1, 40), (33, 257, 96), (257, 1031, 96), (515, 130, 40), (64, 2048, 512), (33, 257, 3),
               (33, 257, 33)]
TOPK_SHAPES = GRID_SHAPES + [(33, 128, 96), (5, 10, 3)]               # ... and ng == k for k = 128 and k = 10


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _np(t):
    return None if t is None else t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def grid_case(nq, ng, d):
    """exact-grid inputs whose rows on the first and last position of every tile are copies of one row (they tie exactly with each
    other wherever they lie), explicit labels that walk those positions, and the int64 scores; computed once, read-only"""
    eq, eg = R.tile_edges(nq, TILE), R.tile_edges(ng, TILE)
    q, g = R.grid_inputs(nq, ng, d, seed=1000 * nq + ng + d, dup_q=[(p, eq[0]) for p in eq[1:]], dup_g=[(p, eg[0]) for p in eg[1:]])
    lab_q = np.array([eg[i % len(eg)] for i in range(nq)], dtype=np.int64)
    lab_g = np.array([eq[j % len(eq)] for j in range(ng)], dtype=np.int64)
    return dict(q=q, g=g, lab_q=lab_q, lab_g=lab_g, units=R.grid_scores(q, g))


def _ranks(q, g, lab_q=None, lab_g=None, **kw):
    from xpretrain_amd import hip_ops as H
    return tuple(_np(t) for t in H.retrieval_ranks_streamed(_dev(q), _dev(g), lab_q, lab_g, **kw))


# ------------------------------------------------------------------------------------------------------------------ exact grid
@pytest.mark.parametrize("labels", ["diagonal", "explicit"])
@pytest.mark.parametrize("nq,ng,d", GRID_SHAPES)
def test_grid_counts(nq, ng, d, labels):
    c = grid_case(nq, ng, d)
    u = c["units"]
    if labels == "explicit":
        gq, eq, gg, eg = _ranks(c["q"], c["g"], c["lab_q"], c["lab_g"])
        want_q, want_g = R.counts(u, c["lab_q"]), R.counts(u.T, c["lab_g"])
    else:
        rows, cols = nq <= ng, ng <= nq
        gq, eq, gg, eg = _ranks(c["q"], c["g"], rows=rows, cols=cols)
        want_q, want_g = (R.counts(u) if rows else None), (R.counts(u.T) if cols else None)
        assert (gq is None) == (not rows) and (gg is None) == (not cols)
    if want_q is not None:
        assert np.array_equal(gq, want_q[0]) and np.array_equal(eq, want_q[1]) and (eq >= 1).all()
    if want_g is not None:
        assert np.array_equal(gg, want_g[0]) and np.array_equal(eg, want_g[1]) and (eg >= 1).all()


def test_grid_counts_one_direction_equals_both():
    c = grid_case(257, 1031, 96)
    both = _ranks(c["q"], c["g"], c["lab_q"], c["lab_g"])
    rows = _ranks(c["q"], c["g"], c["lab_q"], None, cols=False)
    cols = _ranks(c["q"], c["g"], None, c["lab_g"], rows=False)
    assert np.array_equal(rows[0], both[0]) and np.array_equal(rows[1], both[1]) and rows[2] is None
    assert np.array_equal(cols[2], both[2]) and np.array_equal(cols[3], both[3]) and cols[0] is None


def _shards(ng, k):
    """three shards of at least k rows whose borders are no tile borders"""
    a, b = max(k, ng // 3 + 1), max(2 * k, 2 * ng // 3 + 3)
    return [(0, a), (a, b), (b, ng)] if ng - b >= k else None


@pytest.mark.parametrize("nq,ng,d,k", [(*s, k) for s in TOPK_SHAPES for k in (1, 10, 128) if k <= s[1]])      # (k > ng is refused)
def test_grid_topk(nq, ng, d, k):
    from xpretrain_amd.utils import metrics
    c = grid_case(nq, ng, d)
    q, g = _dev(c["q"]), _dev(c["g"])
    want_v, want_i = R.topk(c["units"], k)
    vals, idx = metrics.topk(q, g, k)
    assert np.array_equal(_np(vals), (want_v / 64.0).astype(np.float32)) and np.array_equal(_np(idx), want_i)
    vals, idx = metrics.topk(q, g, k, index_base=(1 << 33) + 5)
    assert np.array_equal(_np(vals), (want_v / 64.0).astype(np.float32)) and np.array_equal(_np(idx), want_i + (1 << 33) + 5)
    sh = _shards(ng, k)
    if sh is not None:
        sv, si = metrics.search(q, [g[a:b] for a, b in sh], k)
        assert torch.equal(sv, vals) and np.array_equal(_np(si), want_i)
        out = None                                      # the shards in another order: indices by index_base, the same result
        for a, b in (sh[2], sh[0], sh[1]):
            out = metrics.topk(q, g[a:b], k, index_base=a, out=out)
        assert torch.equal(out[0], vals) and np.array_equal(_np(out[1]), want_i)


# ------------------------------------------------------------------------------------------------------------ real-valued bands
@pytest.mark.parametrize("setting", ["simple", "dsl"])
@pytest.mark.parametrize("nq,ng,d", R.BAND_SHAPES)
def test_real_valued_bands(nq, ng, d, setting):
    c = R.band_case(nq, ng, d)
    gq, eq, gg, eg = _ranks(c["q"], c["g"], c["lab_q"], c["lab_g"], dsl=setting == "dsl", theta=100.0)
    if setting == "dsl":
        x64 = R.dsl64(R.scores64(c["q"], c["g"]), 100.0)
        ratio = torch.from_numpy(R.dsl_restated_f32(c["q"], c["g"], 100.0).astype(np.float64) / x64)
        report(f"retrieval stream {nq}x{ng}x{d}: float32 restatement of dsl_rerank_kernel / fp64 (tol = eps = 4 x this)", ratio,
               torch.ones_like(ratio), c["eps"])
    for direction, (lo, hi), got_g, got_e in (("t2v", c[setting][0], gq, eq), ("v2t", c[setting][1], gg, eg)):
        share = R.check_band(f"{nq}x{ng}x{d} {setting} {direction}", got_g, got_e, lo, hi)
        print(f"retrieval stream {nq}x{ng}x{d} {setting} {direction}: ambiguous share {share:.4f}, delta {c['delta']:.2e}, eps {c['eps']:.2e}")
        assert share <= R.AMBIGUOUS_CAP


def test_streamed_metrics_against_reference_fixture(golden):
    """the acceptance rule of tests/test_retrieval_gpu.py::test_metrics_against_reference_fixture, on the streamed path"""
    from xpretrain_amd.utils import metrics
    fx = golden("retrieval.pt")
    for ci, c in enumerate(fx["cases"]):
        txt, vis = c["txt"].cuda(), c["vis"].cuda()
        got = metrics.retrieval_metrics_streamed(txt, vis)
        n = txt.shape[0]
        for setting in ("simple", "DSL"):
            for direction in ("v2t", "t2v"):
                g, r = got[setting][direction], c["results"][setting][direction]
                tol = 0.0 if setting == "simple" else 1.5 / n
                assert all(abs(a - b) <= tol * max(1.0, abs(b)) + (0 if setting == "simple" else 0.51) * (i >= 3)
                           for i, (a, b) in enumerate(zip(g, r))), (ci, setting, direction, g, r)
        t2v, _ = metrics.rank_counts_streamed(txt, vis, labels=c["labels"].tolist())
        assert metrics._summarise(*t2v) == pytest.approx(c["multi"], rel=1e-12)


# ------------------------------------------------------------------------------------------------------- the contract's properties
def test_position_independence():
    """permuting the gallery rows permutes idx and leaves vals, greater and equal bit-equal"""
    from xpretrain_amd.utils import metrics
    c = R.band_case(257, 1031, 96)
    perm = np.random.default_rng(11).permutation(1031)
    q, g, g2 = _dev(c["q"]), _dev(c["g"]), _dev(c["g"][perm])
    lab_q = np.arange(257)
    inv = np.argsort(perm)                                              # row j of g is row inv[j] of g2
    for k in (1, 10, 128):
        (v1, i1), (v2, i2) = metrics.topk(q, g, k), metrics.topk(q, g2, k)
        assert torch.equal(v1, v2)
        # two rows whose fp32 scores tie are listed lowest index first, in either numbering: order ties by the original index, and
        # leave out the entries that tie with the k-th (which member of such a tie is listed depends on the numbering as well)
        v, a, b = _np(v1), _np(i1), perm[_np(i2)]
        b = np.take_along_axis(b, np.lexsort((b, -v)), 1)
        inside = v > v[:, -1:]
        assert np.array_equal(a[inside], b[inside]) and (k == 128 or inside.sum() >= 257 * (k - 1))
    for dsl in (False, True):
        a = _ranks(c["q"], c["g"], lab_q, c["lab_g"], dsl=dsl)
        b = _ranks(c["q"], c["g"][perm], inv[lab_q], c["lab_g"][perm], dsl=dsl)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(a[2], b[2][inv]) and np.array_equal(a[3], b[3][inv])
    # tie-heavy: values and counts (indices of tied entries follow the new positions)
    t = grid_case(257, 1031, 96)
    v1, _ = metrics.topk(_dev(t["q"]), _dev(t["g"]), 128)
    v2, _ = metrics.topk(_dev(t["q"]), _dev(t["g"][perm]), 128)
    assert torch.equal(v1, v2)
    a, b = _ranks(t["q"], t["g"], t["lab_q"], t["lab_g"]), _ranks(t["q"], t["g"][perm], inv[t["lab_q"]], t["lab_g"][perm])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2][inv]) and np.array_equal(a[3], b[3][inv])


def test_run_to_run_bit_equality():
    from xpretrain_amd.utils import metrics
    c = R.band_case(515, 130, 40)
    q, g = _dev(c["q"]), _dev(c["g"])
    first = None
    for _ in range(3):
        got = [*_ranks(c["q"], c["g"], c["lab_q"], c["lab_g"], dsl=True), *(_np(t) for t in metrics.topk(q, g, 100))]
        first = first or got
        assert all(np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a, b.view(np.int32) if b.dtype == np.float32 else b)
                   for a, b in zip(first, got))


def _int_out(n):
    g = Guarded(1, n, torch.float32)                       # the pattern 0x7FA5A5A5 reads as a large positive int32
    return g, g.mat.view(torch.int32).view(-1)


@pytest.mark.parametrize("dsl", [0, 1])
def test_ranks_in_guarded_buffers(dsl):
    """the C entry point with the workspace at exactly its stated size between poisoned guards and every output in a guard buffer"""
    from xpretrain_amd import _lib as L, hip_ops as H
    nq, ng, d = 257, 1031, 96
    c = R.band_case(nq, ng, d)
    q, g = _dev(c["q"]), _dev(c["g"])
    want = _ranks(c["q"], c["g"], c["lab_q"], c["lab_g"], dsl=bool(dsl))
    outs = [_int_out(n) for n in (nq, nq, ng, ng)]
    lab_g = _dev(c["lab_g"])
    with GuardedWorkspaces() as gw:
        need = L.lib().xp_retrieval_ranks_streamed_workspace_bytes(nq, ng, d, dsl)
        ws = H.workspace(need, q.device, "retrieval_ranks")
        assert ws.numel() == need
        L.check(L.lib().xp_retrieval_ranks_streamed(H._p(q), H._p(g), None, H._p(lab_g), nq, ng, d, dsl, 100.0, *(H._p(o[1]) for o in outs),
                                                    H._p(ws), need, H._stream()), "xp_retrieval_ranks_streamed")
        gw.check()
        again = H.retrieval_ranks_streamed(q, g, None, lab_g, dsl=bool(dsl))         # the wrapper asks for the same bytes
        gw.check()
    assert [r[1] for r in gw.records] == [need, need]
    for (guard, view), w, a, n in zip(outs, want, again, (nq, nq, ng, ng)):
        guard.check(f"ranks dsl={dsl}", 1, n)
        assert np.array_equal(_np(view), w) and np.array_equal(_np(a), w)


@pytest.mark.parametrize("nq,ng,d,k", [(64, 2048, 512, 128), (257, 1031, 96, 10)])
def test_topk_in_guarded_buffers(nq, ng, d, k):
    from xpretrain_amd import _lib as L, hip_ops as H
    c = grid_case(nq, ng, d)
    q, g = _dev(c["q"]), _dev(c["g"])
    want_v, want_i = R.topk(c["units"], k)
    gv, gi = Guarded(nq, k, torch.float32), Guarded(nq, 2 * k, torch.float32)
    idx = gi.mat.view(torch.int64)
    with GuardedWorkspaces() as gw:
        need = L.lib().xp_retrieval_topk_workspace_bytes(nq, ng, d, k)
        ws = H.workspace(need, q.device, "retrieval_topk")
        L.check(L.lib().xp_retrieval_topk(H._p(q), H._p(g), nq, ng, d, k, 0, 0, H._p(gv.mat), H._p(idx), H._p(ws), need, H._stream()),
                "xp_retrieval_topk")
        gw.check()
    gv.check("topk vals", nq, k)
    gi.check("topk idx", nq, 2 * k)
    assert np.array_equal(_np(gv.mat), (want_v / 64.0).astype(np.float32)) and np.array_equal(_np(idx), want_i)


def test_on_a_side_stream():
    from xpretrain_amd.utils import metrics
    c = R.band_case(130, 515, 40)
    q, g = _dev(c["q"]), _dev(c["g"])
    want = [*_ranks(c["q"], c["g"], c["lab_q"], c["lab_g"], dsl=True), *(_np(t) for t in metrics.topk(q, g, 10))]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = [*_ranks(c["q"], c["g"], c["lab_q"], c["lab_g"], dsl=True), *(_np(t) for t in metrics.topk(q, g, 10))]
    s.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(want, got))


def test_gallery_beyond_4_gib():
    """ng = 2^21 + 64 rows of 512: a zero gallery with exact-grid rows on both sides of byte offsets 2^31 and 2^32 and in the last
    row; top-k and the row direction's counts against the reference (the planted rows' scores, zero everywhere else)"""
    from xpretrain_amd import hip_ops as H
    from xpretrain_amd.utils import metrics
    nq, ng, d, k = 4, (1 << 21) + 64, 512, 10
    free, _ = torch.cuda.mem_get_info()
    if free < 6 << 30:
        pytest.skip("needs 6 GiB of free device memory")
    row_bytes = d * 4
    planted = np.array([(1 << 31) // row_bytes - 1, (1 << 31) // row_bytes, (1 << 32) // row_bytes - 1, (1 << 32) // row_bytes, ng - 1])
    assert ng * row_bytes > 1 << 32
    q, rows = R.grid_inputs(nq, len(planted), d, seed=77)
    rows[1], rows[3] = rows[0], rows[2]                      # the rows on either side of a boundary tie exactly
    units = np.zeros((nq, ng), dtype=np.int64)
    units[:, planted] = R.grid_scores(q, rows)
    gallery = torch.zeros((ng, d), dtype=torch.float32, device="cuda")
    gallery[torch.from_numpy(planted).cuda()] = _dev(rows)
    qd = _dev(q)
    want_v, want_i = R.topk(units, k)
    vals, idx = metrics.topk(qd, gallery, k)
    assert np.array_equal(_np(vals), (want_v / 64.0).astype(np.float32)) and np.array_equal(_np(idx), want_i)
    lab = planted[[1, 2, 3, 4]]
    gq, eq, _, _ = H.retrieval_ranks_streamed(qd, gallery, lab, None, cols=False)
    want_g, want_e = R.counts(units, lab)
    assert np.array_equal(_np(gq), want_g) and np.array_equal(_np(eq), want_e)
    del gallery
    torch.cuda.empty_cache()


def test_only_fp32_gpu_features():
    from xpretrain_amd.utils import metrics
    q, g = torch.zeros(4, 8, device="cuda"), torch.zeros(16, 8, device="cuda")
    for bad in (q.bfloat16(), q.double(), q.cpu()):
        for f in (lambda: metrics.topk(bad, g, 2), lambda: metrics.rank_counts_streamed(bad, g), lambda: metrics.search(bad, [g], 2),
                  lambda: metrics.retrieval_metrics_streamed(bad, g)):
            with pytest.raises(RuntimeError, match="float32|no CPU path"):
                f()
    with pytest.raises(ValueError, match="k=17"):
        metrics.topk(q, g, 17)                                            # k > ng, refused by the library's sizing call
