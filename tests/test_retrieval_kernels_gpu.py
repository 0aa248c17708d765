"""GPU: the three retrieval-evaluation kernels of csrc/small_gemm.hip and csrc/retrieval.hip, called through the C ABI with every output in a guard buffer, and
the functions of xpretrain_amd.utils.metrics built on them.

Covered:
    [x] xp_sim_matrix        fp64 product of unit-norm rows, 1e-5 of the tensor scale (the figure tests/test_retrieval_gpu.py uses for
                             cal_cossim); ragged tiles in all three extents
    [x] xp_dsl_rerank        in place; fp64 column softmax of the same fp32 input, 1e-4 of the tensor scale (the project's figure for
                             np_softmax(100x)); theta 1 / 100, multiply 0 / 1; row counts on both sides of the 64-lane stride; with
                             multiply = 0 every column sums to 1 within 1e-5; two runs give the same bits
    [x] xp_retrieval_ranks   integer-exact against (row > v).sum() / (row == v).sum() by torch on the very same fp32 matrix: candidate
                             counts 1, 5, 63, 64, 65, 200, both orientations, explicit and diagonal labels, generic matrices and
                             matrices quantised to multiples of 1/8 (ties everywhere, -0.0 beside +0.0); diagonal labels with more
                             queries than candidates are refused with nothing written
    [x] metrics.compute_metrics / compute_metrics_multi / retrieval_metrics on the tie-heavy matrices: equal to
                             oracle.retrieval_oracle.summarise(ranks(...)) on the same matrix on the host, exactly ('simple'); the
                             DSL setting keeps the allowance of tests/test_retrieval_gpu.py (a near-tie may swap after the fp32 softmax)
No label is out of range: the kernels do not check them."""
import numpy as np
import pytest
import torch

from oracle import retrieval_oracle as RO
from tests.gpu_util import report
from tests.guarded import Guarded

pytestmark = pytest.mark.gpu
F32 = torch.float32
XP_ERR_ARG = -1


def _H():
    from xpretrain_amd import hip_ops as H
    return H, H.L.lib()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ok(rc, lib):
    assert rc == 0, lib.xp_last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ xp_sim_matrix
@pytest.mark.parametrize("na,nb,d", [(1, 1, 1), (33, 65, 7), (64, 32, 96), (70, 200, 513)])
def test_sim_matrix(na, nb, d):
    H, lib = _H()
    g = _gen(na + nb + d)
    a = torch.nn.functional.normalize(torch.randn(na, d, generator=g), dim=-1)
    b = torch.nn.functional.normalize(torch.randn(nb, d, generator=g), dim=-1)
    out = Guarded(na, nb, F32)
    da, db = a.cuda(), b.cuda()
    _ok(lib.xp_sim_matrix(H._p(da), H._p(db), H._p(out.mat), na, nb, d, H._stream()), lib)
    out.check(f"sim_matrix {na}x{nb}x{d}", na, nb)
    ref = a.double() @ b.double().t()
    assert report(f"xp_sim_matrix {na}x{nb}x{d}", out.mat, ref, 1e-5) <= 1e-5


# ------------------------------------------------------------------------------------------------------------------ xp_dsl_rerank
def _rerank(x, theta, multiply):
    H, lib = _H()
    n, m = x.shape
    g = Guarded(n, m, F32)
    g.mat.copy_(x.cuda())
    _ok(lib.xp_dsl_rerank(H._p(g.mat), n, m, float(theta), multiply, H._stream()), lib)
    g.check(f"dsl_rerank {n}x{m}", n, m)
    return g.mat.cpu()


@pytest.mark.parametrize("multiply", [0, 1])
@pytest.mark.parametrize("theta", [1, 100])
@pytest.mark.parametrize("n,m", [(1, 1), (63, 5), (64, 64), (65, 3), (200, 130)])
def test_dsl_rerank(n, m, theta, multiply):
    x = torch.rand(n, m, generator=_gen(n + m)) * 2 - 1
    got = _rerank(x, theta, multiply)
    sm = torch.softmax(x.double() * theta, dim=0)
    ref = x.double() * sm if multiply else sm
    tag = f"xp_dsl_rerank {n}x{m} theta={theta} multiply={multiply}"
    assert report(tag, got, ref, 1e-4) <= 1e-4
    if not multiply:
        dev = (got.double().sum(0) - 1).abs().max().item()
        print(f"{tag}: max |column sum - 1| = {dev:.2e}")
        assert dev <= 1e-5
    again = _rerank(x, theta, multiply)
    assert torch.equal(again.view(torch.int32), got.view(torch.int32)), "second run differs"


# ------------------------------------------------------------------------------------------------------------------ xp_retrieval_ranks
def _matrix(n, m, family):
    g = _gen(17 * n + m)
    if family == "generic":
        return torch.randn(n, m, generator=g)
    x = torch.randint(-4, 5, (n, m), generator=g).float() / 8          # multiples of 1/8 in [-0.5, 0.5]: ties everywhere
    if family == "signed_zeros":
        flat = x.view(-1)
        zeros = (flat == 0).nonzero()[:, 0]
        flat[zeros[::2]] = -0.0                                         # every other zero is -0.0
    return x


def _ranks(x, labels, transpose):
    """-> (rc, greater, equal, their guards)"""
    H, lib = _H()
    n, m = x.shape
    q = m if transpose else n
    gg, ge = Guarded(1, q, F32), Guarded(1, q, F32)                     # int32 outputs in the fp32 guard buffer: same width
    d = x.cuda()
    lab = None if labels is None else labels.cuda()
    rc = lib.xp_retrieval_ranks(H._p(d), H._p(lab), n, m, int(transpose), H._p(gg.mat), H._p(ge.mat), H._stream())
    torch.cuda.synchronize()
    return rc, gg.mat[0].view(torch.int32).cpu(), ge.mat[0].view(torch.int32).cpu(), (gg, ge)


def _ranks_ref(x, labels, transpose):
    M = x.t() if transpose else x
    q = M.shape[0]
    lab = torch.arange(q) if labels is None else labels
    v = M[torch.arange(q), lab][:, None]
    return (M > v).sum(1).to(torch.int32), (M == v).sum(1).to(torch.int32)


SHAPES = [(1, 1), (5, 63), (64, 64), (65, 200), (200, 65)]


@pytest.mark.parametrize("family", ["generic", "eighths", "signed_zeros"])
@pytest.mark.parametrize("labels", ["explicit", "diagonal"])
@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("n,m", SHAPES)
def test_retrieval_ranks(n, m, transpose, labels, family):
    H, lib = _H()
    q, cnt = (m, n) if transpose else (n, m)
    x = _matrix(n, m, family)
    if family == "signed_zeros" and n * m > 1:
        bits = x.view(torch.int32)
        assert bool((bits == 0).any()) and bool((bits == -(1 << 31)).any())
    if labels == "diagonal" and q > cnt:
        rc, g, e, guards = _ranks(x, None, transpose)                   # more queries than candidates: no diagonal, refused
        assert rc == XP_ERR_ARG and lib.xp_last_error().decode().startswith("xp_retrieval_ranks:")
        for gd in guards:
            gd.check(f"retrieval_ranks {n}x{m} refused", 0, 0)
        return
    lab = torch.randint(0, cnt, (q,), generator=_gen(n + 3 * m + transpose)) if labels == "explicit" else None
    rc, g, e, guards = _ranks(x, lab, transpose)
    assert rc == 0, lib.xp_last_error()
    for gd in guards:
        gd.check(f"retrieval_ranks {n}x{m}", 1, q)
    rg, re_ = _ranks_ref(x, lab, transpose)
    assert torch.equal(g, rg) and torch.equal(e, re_)
    assert int(e.min()) >= 1
    if family != "generic" and cnt >= 63:
        assert int(e.max()) > 1 and int(g.max()) > 0                    # the ties are really there


# ------------------------------------------------------------------------------------------------------------------ metrics
@pytest.mark.parametrize("family", ["eighths", "signed_zeros"])
@pytest.mark.parametrize("n,m", [(5, 63), (64, 64), (65, 200)])
def test_compute_metrics_on_tie_heavy_matrices(n, m, family):
    from xpretrain_amd.utils import metrics
    x = _matrix(n, m, family)
    d, xn = x.cuda(), x.numpy()
    ind = RO.ranks(xn)
    assert len(ind) > n                                                  # ties: more listed positions than queries
    assert metrics.compute_metrics(d) == RO.summarise(ind)
    lab = torch.randint(0, m, (n,), generator=_gen(n + m)).tolist()
    assert metrics.compute_metrics_multi(d, lab) == RO.summarise(RO.ranks(xn, lab))
    greater, equal = metrics._rank_counts(d)
    assert np.array_equal(np.concatenate([np.arange(a, a + b) for a, b in zip(greater, equal)]), ind)


@pytest.mark.parametrize("n", [64, 130])
def test_retrieval_metrics_on_a_tie_heavy_matrix(n):
    """text features = the quantised matrix, video features = the identity: the similarity matrix IS the quantised matrix (sums of
    one product and zeros are exact).  'simple' equals the oracle exactly, t2v on the matrix and v2t on its transposed copy; DSL keeps
    the allowance of tests/test_retrieval_gpu.py::test_metrics_against_reference_fixture."""
    from xpretrain_amd.utils import metrics
    x = _matrix(n, n, "eighths")
    got = metrics.retrieval_metrics(x.cuda(), torch.eye(n).cuda())
    assert torch.equal(metrics.cal_cossim(x.cuda(), torch.eye(n).cuda()).cpu(), x)
    xn = x.numpy()
    assert got["simple"]["t2v"] == RO.summarise(RO.ranks(xn))
    assert got["simple"]["v2t"] == RO.summarise(RO.ranks(np.ascontiguousarray(xn.T)))
    ref = RO.validate(xn, np.eye(n, dtype=np.float32))
    assert got["simple"]["t2v"] == ref["simple"]["t2v"] and got["simple"]["v2t"] == ref["simple"]["v2t"]
    for direction in ("v2t", "t2v"):
        gd, rd = got["DSL"][direction], ref["DSL"][direction]
        print(f"retrieval_metrics DSL {direction} n={n}: {gd} | oracle {rd}")
        assert all(abs(a - b) <= 1.5 / n * max(1.0, abs(b)) + 0.51 * (i >= 3) for i, (a, b) in enumerate(zip(gd, rd))), (direction, gd, rd)
