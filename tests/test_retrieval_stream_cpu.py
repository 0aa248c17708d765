"""CPU: the reference of the streamed retrieval kernels (tests/retrieval_stream_ref.py) against oracle/retrieval_oracle.py and
tests/golden/retrieval.pt; how much the real-valued bands leave open; and the host side of the C ABI -- workspace sizes and every
refusal, none of which launches anything."""
import ctypes as C

import numpy as np
import pytest

from oracle import retrieval_oracle as RO
from tests import retrieval_stream_ref as R
from xpretrain_amd import _lib as L

XP_ERR_ARG = -1
FAKE = C.c_void_p(4096)                  # a non-null pointer no refused call may touch


def _labels(n, limit, seed):
    return np.random.default_rng(seed).integers(0, limit, size=n)


# ------------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("nq,ng,d", [(33, 257, 3), (64, 64, 1), (130, 40, 8)])
def test_grid_counts_are_the_oracles_ranks(nq, ng, d):
    q, g = R.grid_inputs(nq, ng, d, seed=nq + d, dup_g=[(ng - 1, 0), (1, 0)])
    units = R.grid_scores(q, g)
    x = units / 64.0
    assert np.array_equal(x.astype(np.float32), (q.astype(np.float64) @ g.astype(np.float64).T))     # exact in fp32
    lab = _labels(nq, ng, 5)
    assert np.array_equal(R.ranks_from_counts(*R.counts(units, lab)), RO.ranks(x, lab))
    lab_g = _labels(ng, nq, 6)
    assert np.array_equal(R.ranks_from_counts(*R.counts(units.T, lab_g)), RO.ranks(x.T, lab_g))
    if nq <= ng:
        assert np.array_equal(R.ranks_from_counts(*R.counts(units)), RO.ranks(x))
    vals, idx = R.topk(units, min(10, ng), index_base=7)
    for i in (0, nq - 1):
        pairs = sorted(((-int(v), j + 7) for j, v in enumerate(units[i])))[:min(10, ng)]
        assert [p[1] for p in pairs] == idx[i].tolist() and [-p[0] for p in pairs] == vals[i].tolist()


def test_reference_validate_is_the_oracles():
    q, g = R.real_inputs(96, 96, 32, seed=2)
    q, g = q.astype(np.float64), g.astype(np.float64)
    want = RO.validate(q, g)
    s = q @ g.T
    for setting, x in (("simple", s), ("DSL", R.dsl64(s, 100))):
        assert RO.summarise(R.ranks_from_counts(*R.counts(x))) == pytest.approx(want[setting]["t2v"], rel=1e-12)
        assert RO.summarise(R.ranks_from_counts(*R.counts(x.T))) == pytest.approx(want[setting]["v2t"], rel=1e-12)


def test_reference_against_the_reference_fixture(golden):
    fx = golden("retrieval.pt")
    for c in fx["cases"]:
        txt, vis = c["txt"].numpy(), c["vis"].numpy()
        sim = RO.cal_cossim(txt, vis)
        assert RO.summarise(R.ranks_from_counts(*R.counts(sim))) == pytest.approx(c["results"]["simple"]["t2v"], rel=1e-12)
        assert RO.summarise(R.ranks_from_counts(*R.counts(sim.T))) == pytest.approx(c["results"]["simple"]["v2t"], rel=1e-12)
        assert RO.summarise(R.ranks_from_counts(*R.counts(sim, c["labels"].numpy()))) == pytest.approx(c["multi"], rel=1e-12)
        dsl = sim * RO.col_softmax(sim, 100)
        assert RO.summarise(R.ranks_from_counts(*R.counts(dsl))) == pytest.approx(c["results"]["DSL"]["t2v"], rel=1e-12)


@pytest.mark.parametrize("nq,ng,d", R.BAND_SHAPES)
def test_the_bands_pin_nine_queries_in_ten(nq, ng, d):
    c = R.band_case(nq, ng, d)
    assert c["spread"] <= 20.0                      # theta * (column score range): far from fp32 underflow
    for setting in ("simple", "dsl"):
        for direction, (lo, hi) in zip(("t2v", "v2t"), c[setting]):
            share = float((hi - lo > 1).mean())
            print(f"{nq}x{ng}x{d} {setting} {direction}: ambiguous share {share:.4f} (delta {c['delta']:.2e}, deviation {c['dev']:.2e})")
            assert (hi - lo >= 1).all() and share <= R.AMBIGUOUS_CAP


# ------------------------------------------------------------------------------------------------------------ workspace sizes
def _ws_ranks(nq, ng, d, dsl):
    return L.lib().xp_retrieval_ranks_streamed_workspace_bytes(nq, ng, d, dsl)


def _ws_topk(nq, ng, d, k):
    return L.lib().xp_retrieval_topk_workspace_bytes(nq, ng, d, k)


@pytest.mark.parametrize("nq,ng", [(1, 1), (130, 515), (1000, 1000), (4096, 16384), (8192, 1 << 20), (100000, 1000000), (1 << 20, 3000)])
def test_workspaces_grow_at_most_linearly(nq, ng):
    """doubling both extents at most doubles the workspace, plus a constant: the padding of the carved regions, and what a launch
    that splits its streamed dimension keeps per split -- the statistics of at most 512 workgroups of 128 columns (8 bytes each),
    the lists of at most 512 workgroups of 128 queries (12 k bytes each); a dimension large enough to fill the GPU is not split"""
    pad = 64 << 10
    for d in (40, 512):
        for dsl in (0, 1):
            a, b = _ws_ranks(nq, ng, d, dsl), _ws_ranks(2 * nq, 2 * ng, d, dsl)
            assert 0 < a and b <= 2 * a + pad + 512 * 128 * 8, (nq, ng, d, dsl, a, b)
        for k in (1, 10, 128):
            if k <= ng:
                a, b = _ws_topk(nq, ng, d, k), _ws_topk(2 * nq, 2 * ng, d, k)
                assert 0 < a and b <= 2 * a + pad + 512 * 128 * 12 * k, (nq, ng, d, k, a, b)


def test_workspaces_at_gallery_scale():
    assert _ws_ranks(100000, 1000000, 512, 1) < 64 << 20 and _ws_ranks(100000, 1000000, 512, 0) < 64 << 20
    for k in (1, 10, 128):
        assert _ws_topk(100000, 1000000, 512, k) < 64 << 20
    # never a queries x gallery term: 2^20 x 2^20 scores would be 4 TiB
    assert _ws_ranks(1 << 20, 1 << 20, 512, 1) < 64 << 20 and _ws_topk(1 << 20, 1 << 20, 512, 128) < 64 << 20


# ------------------------------------------------------------------------------------------------------------------ refusals
def _refused(rc, fn):
    msg = L.lib().xp_last_error().decode()
    assert rc == XP_ERR_ARG and msg.startswith(fn + ":"), (rc, msg)
    return msg


def _ranks(q=FAKE, g=FAKE, lq=None, lg=None, nq=4, ng=4, d=8, dsl=0, theta=100.0, gq=FAKE, eq=FAKE, gg=FAKE, eg=FAKE, ws=FAKE,
           ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = max(_ws_ranks(nq, ng, d, dsl), 1) if min(nq, ng, d) > 0 else 1 << 20
    return L.lib().xp_retrieval_ranks_streamed(q, g, lq, lg, nq, ng, d, dsl, theta, gq, eq, gg, eg, ws, ws_bytes, None)


def _topk(q=FAKE, g=FAKE, nq=4, ng=16, d=8, k=4, base=0, acc=0, vals=FAKE, idx=FAKE, ws=FAKE, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = 1 << 20
    return L.lib().xp_retrieval_topk(q, g, nq, ng, d, k, base, acc, vals, idx, ws, ws_bytes, None)


@pytest.mark.parametrize("kw", [dict(q=None), dict(g=None), dict(nq=0), dict(ng=0), dict(d=0), dict(nq=-3), dict(gq=None), dict(eg=None),
                                dict(gq=None, eq=None, gg=None, eg=None), dict(ws=None), dict(ws_bytes=0),
                                dict(nq=5, ng=4), dict(nq=4, ng=5), dict(nq=1 << 31), dict(dsl=1, theta=float("inf"))],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_ranks_refusals(kw):
    _refused(_ranks(**kw), "xp_retrieval_ranks_streamed")


def test_ranks_refuses_a_short_workspace():
    for dsl in (0, 1):
        need = _ws_ranks(257, 1031, 96, dsl)
        msg = _refused(_ranks(nq=257, ng=1031, d=96, dsl=dsl, gg=None, eg=None, lq=None, ws_bytes=need - 1), "xp_retrieval_ranks_streamed")
        assert str(need) in msg


def test_ranks_one_direction_lifts_the_other_directions_label_rule():
    """nq > ng without labels_q is refused only when the row direction is asked for: the next refusal here is the labels'"""
    bad = np.array([0, 1, 2, 9], dtype=np.int64)
    msg = _refused(_ranks(nq=5, ng=4, gq=None, eq=None, lg=bad.ctypes.data_as(C.c_void_p)), "xp_retrieval_ranks_streamed")
    assert "labels_g[3] = 9" in msg


@pytest.mark.parametrize("which,n,limit", [("lq", 6, 4), ("lg", 4, 6)])
@pytest.mark.parametrize("value", [-1, "limit"])
def test_ranks_refuses_host_labels_out_of_range(which, n, limit, value):
    lab = np.zeros(n, dtype=np.int64)
    lab[n - 2] = limit if value == "limit" else value
    nq, ng = (6, 4) if which == "lq" else (6, 4)
    kw = {which: lab.ctypes.data_as(C.c_void_p)}
    if which == "lq":
        kw.update(gg=None, eg=None)
    else:
        kw.update(gq=None, eq=None)
    msg = _refused(_ranks(nq=nq, ng=ng, **kw), "xp_retrieval_ranks_streamed")
    assert f"[{n - 2}]" in msg and "labels_" + which[1] in msg


@pytest.mark.parametrize("kw", [dict(q=None), dict(g=None), dict(vals=None), dict(idx=None), dict(nq=0), dict(ng=0), dict(d=0), dict(k=0),
                                dict(k=-1), dict(k=129, ng=4096), dict(k=17, ng=16), dict(ws=None), dict(ws_bytes=0), dict(base=-1),
                                dict(ng=1 << 31, k=1)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_topk_refusals(kw):
    _refused(_topk(**kw), "xp_retrieval_topk")


def test_topk_refuses_a_short_workspace():
    need = _ws_topk(64, 2048, 512, 128)
    assert need > 256                                  # this shape splits the gallery: the lists of the further splits
    msg = _refused(_topk(nq=64, ng=2048, d=512, k=128, ws_bytes=need - 1), "xp_retrieval_topk")
    assert str(need) in msg


def test_workspace_functions_refuse_with_zero():
    lib = L.lib()
    for args in ((0, 4, 8, 0), (4, 0, 8, 1), (4, 4, 0, 0), (1 << 31, 4, 8, 0)):
        assert _ws_ranks(*args) == 0 and lib.xp_last_error().decode().startswith("xp_retrieval_ranks_streamed_workspace_bytes:")
    for args in ((0, 4, 8, 1), (4, 4, 8, 0), (4, 4, 8, 5), (4, 4096, 8, 129)):
        assert _ws_topk(*args) == 0 and lib.xp_last_error().decode().startswith("xp_retrieval_topk_workspace_bytes:")


def test_plan_names_the_tile_and_the_splits():
    from xpretrain_amd import hip_ops as H
    p = H.retrieval_stream_plan(64, 2048, 10)
    assert p["tile"] == 128 and p["topk_tiles_per_split"] == 1 and p["stat_tiles_per_split"] == 1
    p = H.retrieval_stream_plan(515, 130, 1)
    assert p["stat_tiles_per_split"] == 1 and p["topk_tiles_per_split"] == 1     # 5 query tiles: 5 statistic splits
    p = H.retrieval_stream_plan(100000, 1000000, 10)
    assert p["topk_tiles_per_split"] == 7813 and p["stat_tiles_per_split"] == 782      # neither dimension is split at this size


def test_streamed_metrics_have_no_cpu_path():
    import torch
    from xpretrain_amd.utils import metrics
    z = torch.zeros(2, 4)
    for f in (lambda: metrics.rank_counts_streamed(z, z), lambda: metrics.retrieval_metrics_streamed(z, z), lambda: metrics.topk(z, z, 1),
              lambda: metrics.search(z, [z], 1)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            f()
