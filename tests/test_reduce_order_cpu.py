"""CPU: tests/reduce_emulation.py restates SUMS (each order agrees with an fp64 sum to the 2e-6 the GPU tests of these kernels use),
and the orders it restates are distinguishable bit for bit -- so the torch.equal of tests/test_reduce_gpu.py pins an order, not
merely a value."""
import pytest
import torch

from tests import reduce_emulation as E

TOL = 2e-6        # relative to the tensor scale: the bound of tests/test_layernorm_gpu.py / test_gemm_plans_gpu.py on these kernels


def _rel(a, ref):
    return ((a.double() - ref).abs().max() / ref.abs().max()).item()


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("nrows", [1, 4, 5, 8, 9, 13, 33, 64, 65, 589, 1025])
def test_trees_and_batch_partition_are_sums(nrows):
    x = _randn(nrows, 72, seed=nrows)
    ref = x.double().sum(0)
    assert _rel(E.tree_a(x), ref) <= TOL
    assert _rel(E.tree_b(x), ref) <= TOL
    assert _rel(E.batch_segment(x), ref) <= TOL
    out = torch.full((72,), 3.0)
    assert _rel(E.batch_segment(x, out, True), ref + 3.0) <= TOL
    assert torch.equal(E.tree_a(x, 0, nrows), E.tree_a(x))
    if nrows > 5:         # a row window: nothing outside [r0, r1) enters
        assert _rel(E.tree_a(x, 3, nrows - 2), x[3:nrows - 2].double().sum(0)) <= TOL


@pytest.mark.parametrize("rows,cols", [(1, 4), (7, 64), (33, 200), (1056, 256), (2048, 256), (2356, 768)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_colsum_partitions_are_sums(rows, cols, dtype):
    X = _randn(rows, cols, seed=rows + cols).to(dtype)
    ref = X.double().sum(0)
    assert E.colsum_partials(X).shape == (E.cdiv(rows, E.cs_rows(rows, cols)), cols)
    assert _rel(E.colsum(X), ref) <= TOL
    assert _rel(E.colsum_deferred(X), ref) <= TOL
    out = torch.full((cols,), 3.0)
    assert _rel(E.colsum(X, out, True), ref + 3.0) <= TOL


def test_cs_rows():
    """32 / 64 / 128 rows per chunk as rows * ceil(cols / 256) crosses 64 * 2048 and 128 * 2048"""
    assert [E.cs_rows(r, c) for r, c in [(1, 4), (2356, 768), (10922, 3072), (10923, 3072), (21845, 3072), (21846, 3072)]] == \
           [32, 32, 32, 64, 64, 128]
    assert [E.cs_rows(131071, 256), E.cs_rows(131072, 256), E.cs_rows(131072, 257)] == [32, 64, 128]


@pytest.mark.parametrize("splits", [1, 2, 3, 4, 5, 7, 8, 9])
def test_splitk_order_is_a_sum(splits):
    slabs = _randn(splits, 1200, seed=splits)
    ref = slabs.double().sum(0)
    assert _rel(E.splitk_reduce(slabs), ref) <= TOL
    out = torch.full((1200,), 3.0)
    assert _rel(E.splitk_reduce(slabs, out, True), ref + 3.0) <= TOL
    assert torch.equal(out, torch.full((1200,), 3.0))          # the caller's tensor is not modified


@pytest.mark.parametrize("blocks,cols", [(1, 192), (9, 192), (38, 768), (295, 192)])
def test_ln_param_reduce_is_a_sum(blocks, cols):
    part = _randn(blocks, 2 * cols, seed=blocks)
    ref = part.double().sum(0)
    dg, db = E.ln_param_reduce(part, cols)
    assert _rel(dg, ref[:cols]) <= TOL and _rel(db, ref[cols:]) <= TOL
    assert [E.ln_bwd_blocks(r) for r in (1, 16, 17, 144, 4712, 8192, 100000)] == [1, 1, 2, 9, 295, 512, 512]


def test_orders_differ_bitwise():
    """on a seeded 64x256 input tree A, tree B and torch.sum give different bits: a kernel that summed in another of these orders
    would fail the GPU test's torch.equal"""
    x = _randn(64, 256, seed=0)
    a, b, t = E.tree_a(x), E.tree_b(x), x.sum(0)
    assert not torch.equal(a, t)
    assert not torch.equal(a, b)
    assert not torch.equal(b, t)
    for o in (a, b, t):
        assert _rel(o, x.double().sum(0)) <= TOL


def test_partitions_differ_only_between_33_and_64_partial_rows():
    """xp_colsum's partition of the chunk partials and the batch path's give the same tree up to 32 rows and from 65 on; for 33..64
    the batch path sums directly and xp_colsum sums pairs first"""
    for n in (1, 7, 32, 65, 74, 171):
        p = _randn(n, 256, seed=n)
        assert torch.equal(E.tree_a(E.groups_a(p, E.cdiv(n, 32))), E.batch_segment(p)), n
    for n in (33, 64):
        p = _randn(n, 256, seed=n)
        assert not torch.equal(E.tree_a(E.groups_a(p, E.cdiv(n, 32))), E.batch_segment(p)), n
