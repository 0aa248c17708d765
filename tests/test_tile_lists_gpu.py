"""GPU: tile lists in the 256-wide GEMM family (XpGemmDesc::m_tiles / k_tiles) and the last video layer's backward over them
(xp_encoder_layer_bwd_listed, functional._dx3_support).  A listed launch is planned as the dense problem and walks only the listed
tiles; over operands that are zero outside those tiles every skipped term is acc + (+-0), so everything here is held to
``torch.equal`` with the dense launch -- no tolerance."""
import pytest
import torch

import xpretrain_amd.functional as XF
from xpretrain_amd import _lib as L
from xpretrain_amd import hip_ops as H

pytestmark = pytest.mark.gpu

SENTINEL = 123.0


class _Partials:
    """stands where a DeferredReduce stands in hip_ops.gemm: hands out one buffer for the fused column sums' partial rows, pre-filled
    with the sentinel, and reduces nothing"""

    def __init__(self):
        self.part = None

    def slot(self, nbytes, name):
        self.part = torch.full((nbytes // 4,), SENTINEL, device="cuda")
        return self.part

    def add(self, *a, **k):
        pass


# ---------------------------------------------------------------------------------------------------------------- dX form
# N = 768 is three tile columns: the default family rule (>= 96 workgroups) then needs 32 row tiles, so M = 31 * 256 + 40 is the
# smallest M with a 256-wide dense plan, more than 3 row tiles and a partial last one.
DX_M, DX_N, DX_K = 31 * 256 + 40, 768, 256
DX_LISTS = {"first": [0], "last-partial": [31], "two-adjacent": [4, 5], "all": list(range(32))}


@pytest.fixture(scope="module")
def dx_operands():
    torch.manual_seed(11)
    A = torch.randn(DX_M, DX_K, device="cuda").bfloat16()
    W = (torch.randn(DX_K, DX_N, device="cuda") * 0.1).bfloat16()          # B k-strided: [K, N]
    resid = torch.randn(DX_M, DX_N, device="cuda").bfloat16()
    return A, W, resid


def _dx(A, W, resid, epi, tiles=None):
    parts = _Partials()
    out = torch.full((DX_M, DX_N), SENTINEL, device="cuda", dtype=torch.bfloat16)
    H.gemm(A, W, DX_M, DX_N, DX_K, b_kstrided=True, epilogue=epi, resid=resid if epi != L.EPI_NONE else None, out=out,
           colsum_defer=parts, m_tiles=tiles)
    torch.cuda.synchronize()
    assert parts.part is not None, "the fused column sums are part of this plan"
    return out, parts.part.view(-1, DX_N)


@pytest.mark.parametrize("epi", [L.EPI_NONE, L.EPI_GELU_BWD], ids=["none", "gelu_bwd"])
@pytest.mark.parametrize("which", list(DX_LISTS))
def test_row_tile_list_equals_the_dense_launch_on_its_tiles_and_writes_nothing_else(dx_operands, which, epi):
    A, W, resid = dx_operands
    tiles = DX_LISTS[which]
    plan = H.gemm_plan(DX_M, DX_N, DX_K, torch.bfloat16, b_kstrided=True, epilogue=epi, colsum=True)
    assert plan["family"] == L.GEMM_FAMILY_256 and plan["tiles_m"] == 32 and plan["colsum_rows"] == 64
    row_tile = torch.arange(DX_M, device="cuda") // 256
    listed_rows = torch.isin(row_tile, torch.tensor(tiles, device="cuda"))
    Az = torch.where(listed_rows[:, None], A, torch.zeros_like(A))
    dense, dense_cs = _dx(Az, W, resid, epi)
    got, got_cs = _dx(Az, W, resid, epi, tiles)
    assert not (dense == SENTINEL).all(1).any(), "the dense launch writes every row"
    assert torch.equal(got[listed_rows], dense[listed_rows])
    assert (got[~listed_rows] == SENTINEL).all(), "a row outside the listed tiles was written"
    cs_rows = torch.isin(torch.arange(64, device="cuda") // 2, torch.tensor(tiles, device="cuda"))      # two partial rows per tile
    assert torch.equal(got_cs[cs_rows], dense_cs[cs_rows])
    assert (got_cs[~cs_rows] == SENTINEL).all(), "a partial row of an unlisted tile was written"


# ---------------------------------------------------------------------------------------------------------------- dW form
# dW[3072, 768] over K = 750 token rows, split 3: slabs of 256, 256 and 238 rows = k-tiles 0-3, 4-7, 8-11 (tile 11: the partial K
# tail, 46 rows).  dY is non-zero in k-tiles 5 and 11 only: slab 0 lists nothing of its own (two padding tiles), slab 1 exactly one
# (+ one padding tile), slab 2 the partial tail (+ one padding tile).
DW_M, DW_N, DW_K, DW_SPLIT = 3072, 768, 750, 3
DW_TILES, DW_BEGIN = [0, 1, 4, 5, 8, 11], [0, 2, 4, 6]


@pytest.fixture(scope="module")
def dw_operands():
    torch.manual_seed(12)
    dY = torch.randn(DW_K, DW_M, device="cuda").bfloat16()
    kt = torch.arange(DW_K, device="cuda") // 64
    dY = torch.where(((kt == 5) | (kt == 11))[:, None], dY, torch.zeros_like(dY))
    X = torch.randn(DW_K, DW_N, device="cuda").bfloat16()
    return dY, X


def _dw(dY, X, **lists):
    slabs = torch.full((DW_SPLIT, DW_M, DW_N), SENTINEL, device="cuda")
    H.gemm(dY, X, DW_M, DW_N, DW_K, a_kstrided=True, b_kstrided=True, out=slabs, split_k=DW_SPLIT, **lists)
    dw = H.splitk_reduce(slabs, torch.empty(DW_M, DW_N, device="cuda"), splits=DW_SPLIT)
    torch.cuda.synchronize()
    return slabs, dw


def test_k_tile_lists_equal_the_dense_split_k_launch(dw_operands):
    dY, X = dw_operands
    plan = H.gemm_plan(DW_M, DW_N, DW_K, torch.bfloat16, a_kstrided=True, b_kstrided=True, split_k=DW_SPLIT)
    assert plan["family"] == L.GEMM_FAMILY_256 and plan["split"] == 3 and plan["k_per_split"] == 256
    assert XF.dx3_tile_lists(1, DW_K, 5 * 64, [(3, 256)])[1][0][0][:4] == DW_TILES[:4]      # (the builder pads the same way)
    dense_slabs, dense = _dw(dY, X)
    slabs, dw = _dw(dY, X, k_tiles=DW_TILES, k_tile_begin=DW_BEGIN)
    assert not (slabs == SENTINEL).any(), "every slab writes its output slab"
    assert torch.equal(slabs, dense_slabs) and torch.equal(dw, dense)
    assert (dense_slabs[0] == 0).all() and dense_slabs[1].abs().max() > 0 and dense_slabs[2].abs().max() > 0


def test_lists_are_refused_where_they_do_not_apply(dx_operands, dw_operands):
    A, W, resid = dx_operands
    dY, X = dw_operands
    dx = lambda M=DX_M, **kw: H.gemm(A, W, M, DX_N, DX_K, b_kstrided=True, **kw)
    dw = lambda **kw: H.gemm(dY, X, DW_M, DW_N, DW_K, a_kstrided=True, b_kstrided=True, split_k=DW_SPLIT, **kw)
    with pytest.raises(RuntimeError, match="256-wide-family plan"):
        dx(M=1024, m_tiles=[0])                                         # 4 x 3 tiles: the 128-row family's plan
    with pytest.raises(RuntimeError, match="256-wide-family plan"):
        H.gemm(A.float(), W.float(), DX_M, DX_N, DX_K, b_kstrided=True, m_tiles=[0])      # fp32 never plans 256-wide
    with pytest.raises(RuntimeError, match="256-wide-family plan|row remap"):
        dx(m_tiles=[0], c_remap=(DX_M, DX_M, 0), out_rows=DX_M)         # (a remapped problem is not planned 256-wide to begin with)
    with pytest.raises(RuntimeError, match="256-wide-family plan|row remap"):
        dx(m_tiles=[0], a_remap=(DX_M, DX_M, 0))
    with pytest.raises(RuntimeError, match="entries"):
        dx(m_tiles=list(range(33)))
    with pytest.raises(RuntimeError, match="dX form"):
        dw(m_tiles=[0])
    with pytest.raises(RuntimeError, match="dW form"):
        dx(k_tiles=[0, 1], k_tile_begin=[0, 2])
    with pytest.raises(RuntimeError, match="needs 2"):
        dw(k_tiles=[0, 1, 5, 8, 11], k_tile_begin=[0, 2, 3, 5])         # slab 1 below the pipeline depth
    with pytest.raises(RuntimeError, match="needs 2"):
        dw(k_tiles=list(range(12)) + [11], k_tile_begin=[0, 4, 8, 13])  # slab 2 lists more tiles than it has
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- the layer
# ViT-B's layer over B = 2 samples of S = 4 + 21 * 196 = 4120 tokens: 8240 rows is the smallest such shape whose three dX GEMMs plan
# 256-wide (33 x 3 tiles >= 96); the weight-gradient stream runs (rows >= 4096); S is no multiple of 64, the last row tile is
# partial, and the split-3 weight gradients have a slab without any gradient row.
LAYER = dict(B=2, S=4120, size=(4, 21, 196), D=768, heads=12, Dff=3072)


@pytest.fixture(scope="module")
def layer_case():
    from tests.layer_paths import layer_params
    params = layer_params(LAYER["D"], LAYER["Dff"])
    torch.manual_seed(5)
    x = torch.randn(LAYER["B"] * LAYER["S"], LAYER["D"], device="cuda")
    w = torch.randn(LAYER["B"], LAYER["D"], device="cuda")
    return x, params, w


def _layer_run(layer_case, dtype, native, sparse, loss=None, hook=None):
    """forward of EncoderLayerFn and GatherRowsFn(token 0), backward of ``loss(x3, pooled)`` (default: sum(pooled * w)) with the two
    switches set; returns (dx, the sixteen gradients, listed native backward calls)"""
    from tests.layer_paths import PARAMS
    x, params, w = layer_case
    B, S, size, D, heads = (LAYER[k] for k in ("B", "S", "size", "D", "heads"))
    xin = x.to(dtype, copy=True).requires_grad_()          # (a leaf of its own: the fixture stays as it is)
    side = x.view(B, S, D)[:, :size[0]].reshape(B * size[0], D).contiguous() if dtype == torch.bfloat16 else None
    for p in params:
        p.grad = None
    old = XF.LAYER_CALLS, XF.SPARSE_LAST_BWD, XF.sparse_last_bwd_calls
    XF.LAYER_CALLS, XF.SPARSE_LAST_BWD = native, sparse
    try:
        out = XF.EncoderLayerFn.apply(xin, *params, B, S, heads, size, None, True, side)
        x3 = out[0] if isinstance(out, tuple) else out
        assert x3.grad_fn.native == native
        if hook is not None:
            x3.register_hook(hook)
        pooled = XF.GatherRowsFn.apply(x3, None, B, S)
        (loss(x3, pooled) if loss else (pooled.float() * w).sum()).backward()
        torch.cuda.synchronize()
        calls = XF.sparse_last_bwd_calls - old[2]
    finally:
        XF.LAYER_CALLS, XF.SPARSE_LAST_BWD = old[:2]
    return xin.grad, {n: p.grad for n, p in zip(PARAMS, params)}, calls


def _same(a, b, what):
    assert torch.equal(a[0], b[0]), f"dx differs: {what}"
    for n in a[1]:
        assert torch.equal(a[1][n], b[1][n]), f"{n} differs: {what}"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_last_layer_backward_over_lists_returns_the_dense_bits(layer_case, dtype):
    listed = _layer_run(layer_case, dtype, native=True, sparse=True)
    dense = _layer_run(layer_case, dtype, native=True, sparse=False)
    ops = _layer_run(layer_case, dtype, native=False, sparse=True)
    # bf16: the claim is honoured with lists; fp32 never plans 256-wide: the claim is honoured by the dense call
    assert (listed[2], dense[2], ops[2]) == (int(dtype == torch.bfloat16), 0, 0)
    assert listed[0].abs().max() > 0 and all(g.abs().max() > 0 for n, g in listed[1].items() if n != "bk")
    _same(listed, dense, "lists against the switch off")
    _same(listed, ops, "lists against the op-by-op path")


def test_a_second_consumer_or_a_write_loses_the_claim(layer_case):
    w = layer_case[2]
    # the last hidden state has a second consumer: autograd sums two gradients, the sum carries no claim
    both = lambda x3, pooled: (pooled.float() * w).sum() + x3[1::997].float().sum() * 0.25
    got = _layer_run(layer_case, torch.bfloat16, native=True, sparse=True, loss=both)
    ref = _layer_run(layer_case, torch.bfloat16, native=False, sparse=True, loss=both)
    assert got[2] == 0
    _same(got, ref, "second consumer")
    # a hook writes to the scattered gradient in place (a row no list names): the version moves, the claim is gone
    def hook(g):
        g[4000].add_(0.5)
    got = _layer_run(layer_case, torch.bfloat16, native=True, sparse=True, hook=hook)
    ref = _layer_run(layer_case, torch.bfloat16, native=False, sparse=True, hook=hook)
    assert got[2] == 0
    _same(got, ref, "in-place write")
    plain = _layer_run(layer_case, torch.bfloat16, native=True, sparse=True)
    assert plain[2] == 1 and not torch.equal(plain[0], got[0]), "the written row reaches dx only on the dense path"
