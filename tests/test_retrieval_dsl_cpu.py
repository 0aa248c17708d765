"""CPU: DSL-weighted top-k search -- the C ABI's new entries as the header declares and ``_lib`` binds them, every refusal (none
launches anything), the reference's list check (tests/retrieval_dsl_ref.py) on lists it must accept and must reject, how much
that check leaves open on the real-valued cases, and what the exact-grid cases promise."""
import ctypes as C

import numpy as np
import pytest

from tests import retrieval_dsl_ref as D
from tests import retrieval_stream_ref as R
from xpretrain_amd import _lib as L

XP_ERR_ARG = -1
FAKE = C.c_void_p(4096)                  # a non-null pointer no refused call may touch
KS = (1, 10, 128)


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_header_declares_and_lib_binds_the_entries():
    with open(L.HEADER_PATH) as f:
        abi = L.parse_header(f.read(), L.HEADER_PATH)
    constants, signatures = abi.constants, abi.signatures
    assert constants["XP_DSL_OF_GALLERY"] != constants["XP_DSL_OF_QUERIES"]
    assert (L.XP_DSL_OF_GALLERY, L.XP_DSL_OF_QUERIES) == (constants["XP_DSL_OF_GALLERY"], constants["XP_DSL_OF_QUERIES"])
    i64, i32, f32, ptr, sz = C.c_int64, C.c_int32, C.c_float, C.c_void_p, C.c_size_t
    want = {"xp_retrieval_dsl_stats_workspace_bytes": (sz, [i64, i64, i64]),
            "xp_retrieval_dsl_stats": (i32, [ptr, ptr, i64, i64, i64, f32, i32, ptr, ptr, ptr, sz, ptr]),
            "xp_retrieval_topk_dsl": (i32, [ptr, ptr, i64, i64, i64, i32, i64, i32, f32, i32, ptr, ptr, ptr, ptr, ptr, sz, ptr])}
    for name, (res, args) in want.items():
        assert signatures[name] == (res, args) and L.SIGNATURES[name] == (res, args), (name, signatures[name])
        fn = getattr(L.lib(), name)                                 # the shared library exports it and the binding typed it
        assert fn.restype is res and list(fn.argtypes) == args


# ------------------------------------------------------------------------------------------------------------------ refusals
def _refused(rc, fn):
    msg = L.lib().xp_last_error().decode()
    assert rc == XP_ERR_ARG and msg.startswith(fn + ":"), (rc, msg)
    return msg


def _topk_dsl(q=FAKE, g=FAKE, nq=4, ng=16, d=8, k=4, base=0, acc=0, theta=100.0, of=None, mx=FAKE, sm=FAKE, vals=FAKE, idx=FAKE, ws=FAKE,
              ws_bytes=1 << 20):
    of = L.XP_DSL_OF_GALLERY if of is None else of
    return L.lib().xp_retrieval_topk_dsl(q, g, nq, ng, d, k, base, acc, theta, of, mx, sm, vals, idx, ws, ws_bytes, None)


def _stats(over=FAKE, of=FAKE, n_over=4, n_of=16, d=8, theta=100.0, acc=0, mx=FAKE, sm=FAKE, ws=FAKE, ws_bytes=1 << 20):
    return L.lib().xp_retrieval_dsl_stats(over, of, n_over, n_of, d, theta, acc, mx, sm, ws, ws_bytes, None)


@pytest.mark.parametrize("kw", [dict(mx=None), dict(sm=None), dict(theta=float("inf")), dict(theta=float("nan")), dict(of=0), dict(of=3),
                                dict(of=-1),
                                # ... and everything xp_retrieval_topk refuses (tests/test_retrieval_stream_cpu.py::test_topk_refusals)
                                dict(q=None), dict(g=None), dict(vals=None), dict(idx=None), dict(nq=0), dict(ng=0), dict(d=0), dict(k=0),
                                dict(k=-1), dict(k=129, ng=4096), dict(k=17, ng=16), dict(ws=None), dict(ws_bytes=0), dict(base=-1),
                                dict(ng=1 << 31, k=1)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_topk_dsl_refusals(kw):
    for of in ((kw["of"],) if "of" in kw else (L.XP_DSL_OF_GALLERY, L.XP_DSL_OF_QUERIES)):
        _refused(_topk_dsl(**{**kw, "of": of}), "xp_retrieval_topk_dsl")


def test_topk_dsl_refuses_a_short_workspace():
    need = L.lib().xp_retrieval_topk_workspace_bytes(64, 2048, 512, 128)
    msg = _refused(_topk_dsl(nq=64, ng=2048, d=512, k=128, ws_bytes=need - 1), "xp_retrieval_topk_dsl")
    assert str(need) in msg


@pytest.mark.parametrize("kw", [dict(over=None), dict(of=None), dict(mx=None), dict(sm=None), dict(n_over=0), dict(n_of=0), dict(d=0),
                                dict(n_over=-3), dict(n_of=1 << 31), dict(theta=float("inf")), dict(theta=float("nan")), dict(ws=None),
                                dict(ws_bytes=0), dict(acc=1, mx=None)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_stats_refusals(kw):
    _refused(_stats(**kw), "xp_retrieval_dsl_stats")


def test_stats_workspace():
    ws = L.lib().xp_retrieval_dsl_stats_workspace_bytes
    for args in ((0, 4, 8), (4, 0, 8), (4, 4, 0), (1 << 31, 4, 8)):
        assert ws(*args) == 0 and L.lib().xp_last_error().decode().startswith("xp_retrieval_dsl_stats_workspace_bytes:")
    # the per-split partials of the rank call's plan: 5 runs of query tiles at 515 x 130; nothing but padding once the gallery fills
    # the GPU; never an n_over * n_of term
    pad = lambda n: (n + 255) & ~255
    assert ws(515, 130, 40) == 2 * pad(5 * 130 * 4)
    assert ws(130, 515, 40) == 2 * pad(2 * 515 * 4)
    assert 0 < ws(8192, 1 << 20, 512) <= 2 * pad(4 << 20) and ws(1 << 20, 1 << 20, 512) <= 2 * pad(4 << 20)
    need = ws(515, 130, 40)
    msg = _refused(_stats(n_over=515, n_of=130, d=40, ws_bytes=need - 1), "xp_retrieval_dsl_stats")
    assert str(need) in msg


def test_python_surface_refuses_before_the_library():
    import torch
    from xpretrain_amd.utils import metrics
    z = torch.zeros(4, 8)
    for f in (lambda: metrics.dsl_stats(z, z), lambda: metrics.topk(z, z, 1, dsl=(z[:, 0], z[:, 0])),
              lambda: metrics.search(z, [z], 1, dsl_of="gallery"), lambda: metrics.search(z, [z], 1, dsl_of="queries")):
        with pytest.raises(RuntimeError, match="no CPU path"):
            f()
    with pytest.raises(TypeError, match="one-shot iterator"):
        metrics.search(z, iter([z]), 1, dsl_of="queries")             # refused before the features are looked at
    with pytest.raises(ValueError, match="dsl_of"):
        metrics.search(z, [z], 1, dsl_of="rows")


# ------------------------------------------------------------------------------------------------------ the reference itself
def test_reference_modes_are_the_reference_expressions():
    """"gallery": rows of sim * softmax(theta sim, axis 0), sim = queries x gallery; "queries": rows of the transpose of the same
    expression with sim = gallery x queries; the statistics are that softmax's max and denominator"""
    q, g = R.real_inputs(33, 57, 16, seed=3)
    q64, g64 = q.astype(np.float64), g.astype(np.float64)

    def expr(a, b):
        sim = a @ b.T
        e = np.exp(sim * 100.0 - (sim * 100.0).max(0, keepdims=True))
        return sim * (e / e.sum(0, keepdims=True))
    assert np.allclose(D.x64(q, g, 100.0, "gallery"), expr(q64, g64), rtol=1e-13, atol=0)
    assert np.allclose(D.x64(q, g, 100.0, "queries"), expr(g64, q64).T, rtol=1e-13, atol=0)
    for over, of, mode in ((q, g, "gallery"), (g, q, "queries")):
        mx, sm = D.stats64(over, of, 100.0)
        s = R.scores64(over, of)
        x = s * np.exp(100.0 * s - mx) / sm
        assert np.allclose(x if mode == "gallery" else x.T, D.x64(q, g, 100.0, mode), rtol=1e-13, atol=0)


@pytest.mark.parametrize("nq,ng,d", R.BAND_SHAPES)
def test_epsilon_is_the_projects_rule(nq, ng, d):
    """mode "gallery": R.dsl_epsilon itself; mode "queries": R.dsl_epsilon of the transposed problem; a fold over three shards stays
    within a few ulp of the one-shot restatement"""
    c = R.band_case(nq, ng, d)
    assert D.epsilon(c["q"], c["g"], 100.0, "gallery") == R.dsl_epsilon(c["q"], c["g"], 100.0) == (c["eps"], c["dev"])
    assert D.epsilon(c["q"], c["g"], 100.0, "queries") == R.dsl_epsilon(c["g"], c["q"], 100.0)
    cuts = [(0, ng // 3 + 1), (ng // 3 + 1, 2 * ng // 3 + 3), (2 * ng // 3 + 3, ng)]
    one, folded = D.epsilon(c["q"], c["g"], 100.0, "queries"), D.epsilon(c["q"], c["g"], 100.0, "queries", cuts)
    assert abs(folded[1] - one[1]) <= 1e-6 and folded[1] > 0
    m1, s1 = D.stats32([c["g"]], c["q"], 100.0)
    m3, s3 = D.stats32([c["g"][a:b] for a, b in cuts], c["q"], 100.0)
    # the maximum is exact; the sum is reordered (n positive terms in any order: within (n - 1) 2^-24 of the exact sum, twice that
    # between two orders) and each shard's terms are rescaled once (three roundings and two exp, a few 2^-24 more)
    assert np.array_equal(m1, m3) and np.allclose(s1, s3, rtol=(2 * ng + 16) * 2.0 ** -24, atol=0)


def _case(k=10):
    c = R.band_case(257, 1031, 96)
    x, eps, _ = D.band_x64(257, 1031, 96, "gallery")
    vals, idx = R.topk(x, k)
    return x, eps, vals.copy(), idx.copy()


def test_list_check_accepts_the_fp64_list():
    for mode in D.MODES:
        x, eps, _ = D.band_x64(257, 1031, 96, mode)
        for k in KS:
            vals, idx = R.topk(x, k, index_base=5)
            assert D.check_list("fp64", vals, idx, x, eps, index_base=5) <= R.AMBIGUOUS_CAP
            assert D.check_list("fp32", vals.astype(np.float32), idx, x, eps, index_base=5) <= R.AMBIGUOUS_CAP


def _clear_pair(x, eps, k):
    """(query, position p < k - 1) where the margins separate positions p and p + 1"""
    o = D.open_positions(x, k, eps)
    i, p = np.argwhere(~o[:, :-1] & ~o[:, 1:])[0]
    return int(i), int(p)


def test_list_check_rejects_a_swap_across_a_clear_gap():
    x, eps, vals, idx = _case()
    i, p = _clear_pair(x, eps, 10)
    v2, i2 = vals.copy(), idx.copy()
    v2[i, [p, p + 1]], i2[i, [p, p + 1]] = vals[i, [p + 1, p]], idx[i, [p + 1, p]]
    with pytest.raises(AssertionError, match="not in order"):
        D.check_list("swapped", v2, i2, x, eps)
    i2 = idx.copy()
    i2[i, [p, p + 1]] = idx[i, [p + 1, p]]                          # the indices alone: the values no longer belong to them
    with pytest.raises(AssertionError, match="beyond eps"):
        D.check_list("swapped indices", vals, i2, x, eps)


def test_list_check_rejects_a_wrong_index():
    x, eps, vals, idx = _case()
    i, p = _clear_pair(x, eps, 10)
    far = int(np.argsort(-x[i], kind="stable")[500])
    i2 = idx.copy()
    i2[i, p] = far
    with pytest.raises(AssertionError, match="beyond eps"):
        D.check_list("wrong index", vals, i2, x, eps)
    i2 = idx.copy()
    i2[i, p] = idx[i, p + 1]
    with pytest.raises(AssertionError, match="listed twice"):
        D.check_list("duplicate", vals, i2, x, eps)
    i2[i, p] = x.shape[1]
    with pytest.raises(AssertionError, match="out of range"):
        D.check_list("out of range", vals, i2, x, eps)


def test_list_check_rejects_a_missing_better_candidate():
    x, eps, _, _ = _case()
    vals, idx = R.topk(x, 11)
    with pytest.raises(AssertionError, match="miss a better candidate"):
        D.check_list("best dropped", vals[:, 1:], idx[:, 1:], x, eps)


def test_list_check_rejects_a_value_beyond_eps():
    x, eps, vals, idx = _case()
    v2 = vals.copy()
    v2[3, -1] *= 1 - 3 * eps                                          # still in order
    with pytest.raises(AssertionError, match="beyond eps"):
        D.check_list("value off", v2, idx, x, eps)
    v2 = vals.copy()
    v2[3, -1] *= 1 - 0.5 * eps
    D.check_list("value inside", v2, idx, x, eps)


@pytest.mark.parametrize("mode", D.MODES)
@pytest.mark.parametrize("nq,ng,d", R.BAND_SHAPES)
def test_the_margins_decide_nine_positions_in_ten(nq, ng, d, mode):
    """a position counts as open when EITHER neighbour is within the margins (a close pair opens both of its positions).  Measured
    here: at most 0.094 open (257 x 1031 x 96, k = 128, per-query statistics; 0.089 per-gallery), at most 0.013 at k = 10, none at
    k = 1"""
    x, eps, dev = D.band_x64(nq, ng, d, mode)
    for k in KS:
        if k <= ng:
            share = float(D.open_positions(x, k, eps).mean())
            print(f"dsl top-k {nq}x{ng}x{d} {mode} k={k}: open share {share:.4f} (deviation {dev:.2e}, eps {eps:.2e})")
            assert share <= R.AMBIGUOUS_CAP


@pytest.mark.parametrize("nq,ng,d", D.GRID_SHAPES)
def test_exact_grid_has_no_underflow_and_no_foreign_tie(nq, ng, d):
    """theta = 0.25 on scores within +-10 in steps of 1/64: exp(theta s - mx) >= e^-5; every score lies above -1/theta, where
    s e^(theta s) grows with s (per-query statistics keep the order of s); two candidates of a query tie in x64 only where their
    scores tie"""
    c = D.grid_case(nq, ng, d)
    s = c["units"] / 64.0
    assert np.abs(s).max() <= 10 and s.min() > -3.75
    for mode in D.MODES:
        x = D.x64(c["q"], c["g"], D.GRID_THETA, mode)
        mx, sm = D.stats64(*((c["q"], c["g"]) if mode == "gallery" else (c["g"], c["q"])), D.GRID_THETA)
        y = D.GRID_THETA * (s if mode == "gallery" else s.T) - mx
        assert y.min() >= -5.0 and np.isfinite(x).all() and ((x == 0) == (s == 0)).all() and sm.min() >= 1.0
        order = np.argsort(-x, axis=1, kind="stable")
        xs, us = np.take_along_axis(x, order, 1), np.take_along_axis(c["units"], order, 1)
        assert ((np.diff(xs, axis=1) != 0) | (np.diff(us, axis=1) == 0)).all()
        if mode == "queries":
            assert np.array_equal(order, np.argsort(-c["units"], axis=1, kind="stable"))
