"""CPU: tests/embed_ref.py is right, and its case tables can tell a wrong kernel from a right one.

    * the index maps equal torch's view / permute / F.embedding / indexing formulations;
    * the ordered sums equal fp64 autograd of the formulas they are the gradients of (oracle.clipvip_oracle.vip_embeddings, and the
      token + position gather that opens oracle.clipvip_oracle.text_tower) to 1e-5 of the tensor scale, the figure of
      tests/test_embed_loss_gpu.py; the accumulate forms equal that plus the old contents;
    * the integer bf16 rounding equals torch's CPU Tensor.to(bfloat16) on the special-value tables and on a million random patterns;
    * the constructed ids have the properties tests/test_embed_contract_gpu.py relies on;
    * each wrong variant -- swapped grid, reversed / pairwise sums, a chunk boundary off by one, last maximum, truncation -- changes the
      result on at least one case of its table: the torch.equal of the GPU file pins what it is meant to pin."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import clipvip_oracle as O
from tests import embed_ref as R

TOL = 1e-5


def _rel(a, ref):
    return ((a.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-30)).item()


# ------------------------------------------------------------------------------------------------------------------ index maps
@pytest.mark.parametrize("case", R.IM2COL_CASES, ids=str)
def test_im2col_is_the_unfold(case):
    BT, H, W, P = case
    gh, gw = H // P, W // P
    v = R.frames_f32(case)
    ref = v.view(BT, 3, gh, P, gw, P).permute(0, 2, 4, 1, 3, 5).reshape(BT * gh * gw, 3 * P * P)
    assert torch.equal(R.im2col(v, P), ref)
    conv = F.unfold(v, kernel_size=P, stride=P).transpose(1, 2).reshape(BT * gh * gw, 3 * P * P)            # the conv's own patches
    assert torch.equal(R.im2col(v, P), conv)
    u = R.frames_u8(case)
    assert torch.equal(R.im2col(u, P), u.view(BT, 3, gh, P, gw, P).permute(0, 2, 4, 1, 3, 5).reshape(BT * gh * gw, 3 * P * P))


def test_im2col_table_sees_a_swapped_grid():
    changed = [c for c in R.IM2COL_CASES if not torch.equal(R.im2col(R.frames_f32(c), c[3], swap_grid=True), R.im2col(R.frames_f32(c), c[3]))]
    assert changed and all(c[1] != c[2] for c in changed)                       # only non-square frames can tell
    assert [c for c in R.IM2COL_CASES if c[1] != c[2]] == changed               # and each of them does
    for c in changed:
        u = R.frames_u8(c)
        assert not torch.equal(R.im2col(u, c[3], swap_grid=True), R.im2col(u, c[3]))


@pytest.mark.parametrize("norm", list(R.NORMS))
def test_image_norm_u8_is_the_oracle_arithmetic(norm):
    from oracle import retrieval_oracle as RO
    mean, std = R.NORMS[norm]
    assert len(set(mean)) == 3 and len(set(std)) == 3
    u = R.frames_u8((2, 32, 48, 16))
    got = R.image_norm_u8(u, mean, std)
    assert got.dtype == torch.float32 and torch.equal(got, torch.from_numpy(RO.image_norm(u.numpy(), mean, std)))
    assert _rel(got, (u.double() / 255 - torch.tensor(mean, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(std, dtype=torch.float64).view(1, 3, 1, 1)) <= 1e-6


@pytest.mark.parametrize("case", R.PROXY_CASES, ids=str)
def test_proxy_rows(case):
    B, S, M, D = case
    cls, added, pos = R.proxy_inputs(case)
    ref = torch.zeros(B, M, D)
    ref[:, 0] = cls + pos[0]
    if M > 1:
        ref[:, 1:] = added + pos[0]
    assert torch.equal(R.proxy_rows(cls, added, pos, B, M), ref)


@pytest.mark.parametrize("case", R.TEXT_CASES, ids=str)
def test_text_embed_is_the_embedding_lookup(case):
    B, Lt, D, V = case
    inp = R.text_inputs(case, torch.float32)
    ref = F.embedding(inp["ids"], inp["tok"]) + inp["pos"][:Lt][None]
    assert torch.equal(R.text_embed(inp["ids"], inp["tok"], inp["pos"]), ref)
    assert inp["npos"] > Lt


@pytest.mark.parametrize("case", R.GATHER_CASES, ids=str)
def test_gather_and_scatter(case):
    B, S, D = case
    x, dout, idx = R.gather_inputs(case, torch.float32)
    assert 0 in idx.tolist() and (B < 3 or (idx.tolist().count(S - 1) >= 2))
    assert torch.equal(R.gather_rows(x, idx), x[torch.arange(B), idx])
    assert torch.equal(R.gather_rows(x, None), x[:, 0])
    for i in (idx, None):
        exp = torch.zeros(B, S, D)
        exp[torch.arange(B), idx if i is not None else torch.zeros(B, dtype=torch.int64)] = dout
        assert torch.equal(R.scatter_rows(dout, i, S), exp)
        assert int((R.scatter_rows(dout, i, S) != 0).any(-1).sum()) == B


def test_argmax_is_the_first_maximum_and_the_table_sees_the_last():
    changed = 0
    for case in R.ARGMAX_CASES:
        ids = R.argmax_ids(case)
        got = R.argmax_rows(ids)
        ref = torch.tensor([row.index(max(row)) for row in ids.tolist()])
        assert torch.equal(got, ref)
        changed += int((R.argmax_rows(ids, last=True) != got).sum())
    ids = R.argmax_ids((65, 77))
    got = R.argmax_rows(ids)
    assert got[0] == 0 and got[1] == 76 and got[2] == 10 and got[3] == 9 and got[64] == 5
    assert int(ids.max()) > 1 << 32
    assert int(R.argmax_rows(ids & 0xFFFFFFFF)[3]) != 9                         # a 32-bit compare answers differently
    assert changed >= 3


# ------------------------------------------------------------------------------------------------------------------ ordered sums
def _vip_autograd(case, dx, old=None):
    """fp64 gradients of oracle.clipvip_oracle.vip_embeddings' tables under the incoming gradient dx (patch size 1, zero frames)"""
    B, M, T, L, D = case
    gh = 1 if L in (1, 7, 17) else 2 if L == 8 else 3
    gw = L // gh
    p = {"vision_model.embeddings.patch_embedding.weight": torch.zeros(D, 3, 1, 1, dtype=torch.float64),
         "vision_model.embeddings.position_embedding.weight": torch.zeros(1 + L, D, dtype=torch.float64, requires_grad=True),
         "vision_model.embeddings.temporal_embedding": torch.zeros(1, T, D, dtype=torch.float64, requires_grad=True),
         "vision_model.embeddings.class_embedding": torch.zeros(D, dtype=torch.float64, requires_grad=True),
         "vision_model.embeddings.added_cls": torch.zeros(M - 1, D, dtype=torch.float64, requires_grad=True)}
    x, size = O.vip_embeddings(torch.zeros(B, T, 3, gh, gw, dtype=torch.float64), p, SimpleNamespace(patch=1, use_temporal_embed=True))
    assert size == (M, T, L)
    x.backward(dx.double())
    return {"d_class": p["vision_model.embeddings.class_embedding"].grad, "d_added": p["vision_model.embeddings.added_cls"].grad,
            "d_pos": p["vision_model.embeddings.position_embedding.weight"].grad,
            "d_time": p["vision_model.embeddings.temporal_embedding"].grad[0]}


@pytest.mark.parametrize("dtype", R.DTYPES, ids=str)
@pytest.mark.parametrize("case", R.VIP_BWD_CASES, ids=str)
def test_vip_embed_bwd_is_the_gradient(case, dtype):
    B, M, T, L, D = case
    dx, old = R.vip_bwd_inputs(case, dtype)
    ref = _vip_autograd(case, dx)
    got, acc = R.vip_embed_bwd(dx, M, T, L), R.vip_embed_bwd(dx, M, T, L, old=old)
    for k in ref:
        assert got[k].shape == ref[k].shape and got[k].dtype == torch.float32
        if ref[k].numel():
            assert _rel(got[k], ref[k]) <= TOL, k
            assert _rel(acc[k], ref[k] + old[k].double()) <= TOL, k
    for order in ("reversed", "pairwise"):                      # other orders are the same sum
        alt = R.vip_embed_bwd(dx, M, T, L, order=order)
        assert all(_rel(alt[k], ref[k]) <= TOL for k in ref if ref[k].numel())


@pytest.mark.parametrize("dtype", R.DTYPES, ids=str)
@pytest.mark.parametrize("case", R.TEXT_CASES, ids=str)
def test_text_embed_bwd_is_the_gradient(case, dtype):
    B, Lt, D, V = case
    inp = R.text_inputs(case, dtype)
    ids, dx = inp["ids"], inp["dx"]
    tok = inp["tok"].double().requires_grad_()
    pos = inp["pos"].double().requires_grad_()
    (tok[ids] + pos[:Lt][None]).backward(dx.double())            # oracle.clipvip_oracle.text_tower's embedding line
    d_tok, d_pos = R.text_embed_bwd(ids, dx, V)
    assert _rel(d_tok, tok.grad) <= TOL and _rel(d_pos, pos.grad[:Lt]) <= TOL and d_pos.shape == (Lt, D)
    absent = torch.tensor([i not in set(ids.view(-1).tolist()) for i in range(V)])
    assert bool((d_tok[absent].view(torch.int32) == 0).all())                                   # zero BITS
    a_tok, a_pos = R.text_embed_bwd(ids, dx, V, old_tok=inp["old_tok"], old_pos=inp["old_pos"])
    assert _rel(a_tok, tok.grad + inp["old_tok"].double()) <= TOL and _rel(a_pos, pos.grad + inp["old_pos"].double()) <= TOL
    assert torch.equal(a_tok[absent], inp["old_tok"][absent]) and torch.equal(a_pos[Lt:], inp["old_pos"][Lt:])
    ref64 = torch.zeros(V, D, dtype=torch.float64).index_add_(0, ids.view(-1), dx.double().view(-1, D))
    assert _rel(d_tok, ref64) <= TOL


def test_ordered_sum_orders():
    x = R.randn(37, 64, seed=1)
    ref = x.double().sum(0)
    outs = [R.ordered_sum(x, o) for o in ("forward", "reversed", "pairwise")]
    assert all(_rel(o, ref) <= TOL for o in outs)
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
    seq = torch.zeros(64)
    for r in x:
        seq = seq + r
    assert torch.equal(outs[0], seq)
    assert torch.equal(R.ordered_sum(x, from_zero=False), outs[0])                # 0 + x[0] == x[0] for every value but -0.0
    z = torch.tensor([[-0.0]])
    assert R.ordered_sum(z).view(torch.int32).item() == 0 and R.ordered_sum(z, from_zero=False).view(torch.int32).item() != 0


@pytest.mark.parametrize("order", ["reversed", "pairwise"])
def test_tables_see_another_summation_order(order):
    """every ordered sum, in some case of its table, gives other bits when summed in another order"""
    seen = set()
    for case in R.VIP_BWD_CASES:
        B, M, T, L, D = case
        for dtype in R.DTYPES:
            dx, _ = R.vip_bwd_inputs(case, dtype)
            a, b = R.vip_embed_bwd(dx, M, T, L), R.vip_embed_bwd(dx, M, T, L, order=order)
            seen |= {k for k in a if not torch.equal(a[k], b[k])}
            pos_rows = not torch.equal(a["d_pos"][1:], b["d_pos"][1:]), not torch.equal(a["d_pos"][0], b["d_pos"][0])
            seen |= {n for n, hit in zip(("d_pos[1:]", "d_pos[0]"), pos_rows) if hit}
    assert seen >= {"d_class", "d_added", "d_pos[1:]", "d_pos[0]", "d_time"}
    seen = set()
    for case in R.TEXT_CASES:
        inp = R.text_inputs(case, torch.float32)
        a, b = R.text_embed_bwd(inp["ids"], inp["dx"], case[3]), R.text_embed_bwd(inp["ids"], inp["dx"], case[3], order=order)
        seen |= {n for n, x, y in zip(("d_tok", "d_pos"), a, b) if not torch.equal(x, y)}
    assert seen == {"d_tok", "d_pos"}


def test_splitk_order_of_d_time_is_seen():
    """d_time goes through xp_splitk_reduce's (a+b)+(c+d) grouping: with four or more slabs it differs from the running sum"""
    hit = False
    for case in R.VIP_BWD_CASES:
        B, M, T, L, D = case
        dx, _ = R.vip_bwd_inputs(case, torch.float32)
        fr = dx[:, M:].reshape(B, T, L, D)
        part = R.ordered_sum(fr.permute(2, 0, 1, 3).contiguous())
        hit |= not torch.equal(R.vip_embed_bwd(dx, M, T, L)["d_time"], R.ordered_sum(part))
    assert hit


@pytest.mark.parametrize("chunk", [(255, 256), (256, 255), (257, 256)], ids=str)
def test_constructed_ids_see_a_chunk_boundary_off_by_one(chunk):
    """a ballot round that looks at one row too few (drops offset 255), rounds one row too close or one row too wide (count a row twice)"""
    case = R.CONSTRUCTED
    inp = R.text_inputs(case, torch.float32)
    good, _ = R.text_embed_bwd(inp["ids"], inp["dx"], case[3])
    bad, _ = R.text_embed_bwd(inp["ids"], inp["dx"], case[3], chunk=chunk)
    assert not torch.equal(good[0], bad[0])
    assert torch.equal(good[1], bad[1]) and torch.equal(good[2], bad[2])          # ids that occur once are not affected


def test_constructed_ids_have_their_properties():
    B, Lt, D, V = R.CONSTRUCTED
    ids = R.constructed_ids()
    flat, rows, r0 = ids.view(-1).tolist(), B * Lt, R.CONSTRUCTED_R0
    assert ids.shape == (B, Lt) and rows == 288 and min(flat) >= 0 and max(flat) < V
    occ = {i: [r for r, v in enumerate(flat) if v == i] for i in range(V)}
    assert occ[0] == [r0, r0 + 255, r0 + 256, r0 + 257]
    # chunks behind the first occurrence r are rows r+1 .. r+256, r+257 .. r+512: offsets 254 and 255 of the first, 0 of the second
    assert [(q - r0 - 1) // 256 for q in occ[0][1:]] == [0, 0, 1] and [(q - r0 - 1) % 256 for q in occ[0][1:]] == [254, 255, 0]
    assert occ[1] == [0] and occ[2] == [rows - 1]
    assert len(occ[3]) == 2 and (occ[3][1] - occ[3][0] - 1) // 256 == 1          # the only repeat lies in the second chunk
    assert occ[39] == [] and sum(1 for i in range(V) if not occ[i]) >= 1
    assert any(len(o) > 2 and (o[-1] - o[0] - 1) // 256 == 1 for i, o in occ.items() if i >= 4)      # ordinary ids repeat across chunks too
    for case in R.TEXT_CASES[1:]:
        assert len(set(R.text_ids(case).view(-1).tolist())) < case[3]             # every table case but the 1-token one has an absent id


# ------------------------------------------------------------------------------------------------------------------ bf16
def _torch_bf16_bits(u32):
    return R.from_f32_bits(u32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("name", ["SPECIAL", "SUBNORMAL"])
def test_bf16_tables(name):
    table = getattr(R, name)
    src = np.array([a for a, _ in table], dtype=np.uint32)
    want = np.array([b for _, b in table], dtype=np.uint16)
    got = R.bf16_bits(src)
    assert got.tolist() == want.tolist()
    nan = np.isnan(R.from_f32_bits(src).numpy())
    assert got[~nan].tolist() == _torch_bf16_bits(src)[~nan].tolist()             # (the NaN compares as a NaN two lines below)
    t = R.table_f32(table)
    assert R.same(R.to_bf16(t), t.to(torch.bfloat16))
    if name == "SPECIAL":
        f = t.tolist()
        assert any(np.isnan(v) for v in f) and float("inf") in f and float("-inf") in f
        assert {0x00000000, 0x80000000} <= set(src.tolist())
        big = R.to_bf16(t).float()
        assert big[src.tolist().index(0x7F7F7FFF)].item() == torch.finfo(torch.bfloat16).max and torch.isinf(big[src.tolist().index(0x7F7F8000)])
        assert big[src.tolist().index(0x3FFF8000)].item() == 2.0
    else:
        assert all(0 < (a & 0x7FFFFFFF) < 0x00800000 for a, _ in table) and {a >> 31 for a, _ in table} == {0, 1}


def test_bf16_rounding_equals_torch_on_a_million_patterns():
    rng = np.random.default_rng(20)
    u = rng.integers(0, 1 << 32, size=1_000_000, dtype=np.uint64).astype(np.uint32)
    got, ref = R.bf16_bits(u), _torch_bf16_bits(u)
    nan = np.isnan(R.from_f32_bits(u).numpy())
    assert nan.sum() > 1000                                                      # (about 0.4 % of all patterns are NaNs)
    assert np.array_equal(got[~nan], ref[~nan])
    gn, rn = got[nan], ref[nan]
    assert bool(((gn & 0x7F80) == 0x7F80).all() and ((gn & 0x7F) != 0).all() and ((rn & 0x7F80) == 0x7F80).all() and ((rn & 0x7F) != 0).all())


def test_tables_see_truncation():
    src = np.array([a for a, _ in R.SPECIAL], dtype=np.uint32)
    assert (R.bf16_bits(src, "truncate") != R.bf16_bits(src)).sum() >= 6
    for n in R.CAST_N:
        x = R.cast_input(n)
        assert x.numel() == n
        assert not R.same(R.to_bf16(x, "truncate"), R.to_bf16(x))
    x = R.frames_f32(R.IM2COL_CASES[0])
    assert not R.same(R.to_bf16(x, "truncate"), R.to_bf16(x))


def test_same_compares_bits():
    a = torch.tensor([0.0, 1.0, float("nan")])
    assert R.same(a, a.clone()) and not R.same(a, torch.tensor([-0.0, 1.0, float("nan")])) and not R.same(a, torch.tensor([0.0, 1.0, 2.0]))
    assert R.same(R.store(a, torch.bfloat16), a.to(torch.bfloat16))


# ------------------------------------------------------------------------------------------------------------------ l2norm, cast_back
@pytest.mark.parametrize("case", R.L2NORM_CASES, ids=str)
def test_l2norm_reference_is_autograd(case):
    x, dy = R.l2norm_inputs(case, torch.float32)
    xd = x.double().requires_grad_()
    yr = xd / xd.norm(dim=-1, keepdim=True)
    yr.backward(dy.double())
    y, inv = R.l2norm_fwd64(x)
    assert _rel(y, yr.detach()) <= 1e-12 and _rel(R.l2norm_bwd64(dy, y, inv), xd.grad) <= 1e-12


def test_l2norm_zero_row_is_nan_like_the_reference():
    x, _ = R.l2norm_inputs(R.L2NORM_ZERO_ROW, torch.float32, zero_row=True)
    y, inv = R.l2norm_fwd64(x)
    assert bool(torch.isnan(y[1]).all()) and torch.isinf(inv[1]) and bool(torch.isfinite(y[[0, 2, 3]]).all())
    assert bool(torch.isnan((x / x.norm(dim=-1, keepdim=True))[1]).all())


def test_cast_back_reference():
    src = R.randn(12, seed=3).to(torch.bfloat16)
    old = R.randn(12, seed=4)
    assert torch.equal(R.cast_back(src), src.float()) and torch.equal(R.cast_back(src, old), src.float() + old)
