"""GPU: the single-query proxy attention kernels (csrc/attention_pooled.hip: token 0 of every sample against all S keys, the
pooled last layer of the video tower) against an fp64 computation of the same formulas -- plain softmax over all keys of query 0
-- forward and backward, in both compute dtypes; run-to-run bit identity; the fused column sums of dkv; and a cross-check against
row b*S of the dense kernels (xp_attn_fwd / xp_attn_bwd with dout zero elsewhere).

Geometries (B, H, S): configs[1] at the bench batch, the 448^2 configs' 6276 keys, M=4 N=1 L=784, the T = 1 image pass, and two
small odd ones (S not a multiple of anything, fewer problems than CUs); (8, 12, 2356) has more workgroups than CUs.
Tolerances: the project's own for attention against fp64 (tests/test_attention_gpu.py): 1.2e-2 / 2e-2 of the tensor scale in
bf16, 2e-5 / 1e-4 in fp32."""
import pytest
import torch

from tests.gpu_util import report

pytestmark = pytest.mark.gpu

# (B, H, S) -> an (M, N, L) with M + N*L == S for the dense cross-check
GEOMS = {(8, 12, 2356): (4, 12, 196), (2, 12, 6276): (4, 8, 784), (2, 12, 788): (4, 1, 784), (8, 12, 200): (4, 1, 196),
         (1, 2, 9): (1, 2, 4), (3, 5, 201): (1, 4, 50)}
DTYPES = [torch.bfloat16, torch.float32]
Q_SCALE = 0.125


def _tols(dtype):
    return (1.2e-2, 2e-2) if dtype == torch.bfloat16 else (2e-5, 1e-4)


def _inputs(B, H, S, dtype, seed):
    torch.manual_seed(seed)
    q = torch.randn(B, H * 64, device="cuda").to(dtype)
    kv = torch.randn(B * S, 2 * H * 64, device="cuda").to(dtype)
    dout = torch.randn(B, H * 64, device="cuda").to(dtype)
    return q, kv, dout


def _reference(q, kv, dout, B, H, S):
    """fp64 on the kernels' own inputs: out, dq (of the scaled q), dk, dv"""
    qd = q.double().view(B, H, 64).requires_grad_()
    k, v = [t.requires_grad_() for t in kv.double().view(B, S, 2, H, 64).unbind(2)]           # [B, S, H, 64]
    p = torch.softmax(torch.einsum("bhd,bshd->bhs", qd, k), dim=-1)
    out = torch.einsum("bhs,bshd->bhd", p, v).reshape(B, H * 64)
    out.backward(dout.double())
    return out.detach(), qd.grad.reshape(B, H * 64), k.grad, v.grad


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("B,H,S", list(GEOMS))
def test_pooled_attention_against_fp64(B, H, S, dtype):
    from xpretrain_amd import hip_ops as Hh
    tf, tb = _tols(dtype)
    q, kv, dout = _inputs(B, H, S, dtype, seed=S)
    out, stats = Hh.attn_pooled_fwd(q, kv, B, S, H)
    ref_o, ref_dq, ref_dk, ref_dv = _reference(q, kv, dout, B, H, S)
    tag = f"attn_pooled {str(dtype)[6:]} B{B} H{H} S{S}"
    errs = [report(tag + " fwd", out, ref_o, tf)]
    # statistics: (row max, log row sum) of the scores, as xp_attn_fwd defines them
    sc = torch.einsum("bhd,bshd->bhs", q.double().view(B, H, 64), kv.double().view(B, S, 2, H, 64)[:, :, 0])
    lse = stats[..., 0].double() + stats[..., 1].double()
    e_lse = (lse - torch.logsumexp(sc, -1)).abs().max().item()
    print(f"{tag} lse: max|d|={e_lse:.3e}")
    assert e_lse <= 1e-3
    d = Hh.DeferredReduce(q.device)
    dq, dkv, cs = Hh.attn_pooled_bwd(q, kv, out, dout, stats, B, S, H, q_scale=Q_SCALE, colsum_defer=d)
    d.flush()
    dk, dv = dkv.view(B, S, 2, H, 64).unbind(2)
    errs.append(report(tag + " dq", dq, ref_dq * Q_SCALE, tb))
    errs.append(report(tag + " dk", dk, ref_dk, tb))
    errs.append(report(tag + " dv", dv, ref_dv, tb))
    e_cs = report(tag + " fused colsum vs stored", cs, dkv.double().sum(0), 1e-5, scale_floor=1e-3)
    for t in (out, stats, dq, dkv, cs):
        assert torch.isfinite(t.float()).all(), tag
    assert errs[0] <= tf and max(errs[1:]) <= tb and e_cs <= 1e-5, tag
    # run to run: bit-identical (fixed-order combines, no atomics)
    out2, stats2 = Hh.attn_pooled_fwd(q, kv, B, S, H)
    d2 = Hh.DeferredReduce(q.device)
    dq2, dkv2, cs2 = Hh.attn_pooled_bwd(q, kv, out2, dout, stats2, B, S, H, q_scale=Q_SCALE, colsum_defer=d2)
    d2.flush()
    for a, b in ((out, out2), (stats, stats2), (dq, dq2), (dkv, dkv2), (cs, cs2)):
        assert torch.equal(a, b), tag + ": two runs differ"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("B,H,S", list(GEOMS))
def test_pooled_attention_against_dense_row(B, H, S, dtype):
    """row b*S of the dense kernels on qkv = [q scattered into row b*S | kv], dout zero outside those rows"""
    from xpretrain_amd import hip_ops as Hh
    tf, tb = _tols(dtype)
    size = GEOMS[(B, H, S)]
    D = H * 64
    q, kv, dout = _inputs(B, H, S, dtype, seed=S + 1)
    qkv = torch.empty(B * S, 3 * D, device="cuda", dtype=dtype)
    qkv[:, :D] = torch.randn(B * S, D, device="cuda").to(dtype)
    qkv.view(B, S, 3 * D)[:, 0, :D] = q
    qkv[:, D:] = kv
    dense_o, dense_stats = Hh.attn_fwd(qkv, B, S, H, size=size)
    out, stats = Hh.attn_pooled_fwd(q, qkv[:, D:], B, S, H)          # (kv read in place, row pitch 3D)
    tag = f"attn_pooled vs dense {str(dtype)[6:]} B{B} H{H} S{S}"
    e = [report(tag + " fwd", out, dense_o.view(B, S, D)[:, 0], tf)]
    dd = torch.zeros(B * S, D, device="cuda", dtype=dtype)
    dd.view(B, S, D)[:, 0] = dout
    dense_dqkv = Hh.attn_bwd(qkv, dense_o, dd, dense_stats, B, S, H, size=size, q_scale=Q_SCALE)
    dq, dkv = Hh.attn_pooled_bwd(q, qkv[:, D:], out, dout, stats, B, S, H, q_scale=Q_SCALE)
    e.append(report(tag + " dq", dq, dense_dqkv.view(B, S, 3 * D)[:, 0, :D], tb))
    e.append(report(tag + " dk", dkv[:, :D], dense_dqkv[:, D:2 * D], tb))
    e.append(report(tag + " dv", dkv[:, D:], dense_dqkv[:, 2 * D:], tb))
    assert e[0] <= tf and max(e[1:]) <= tb, tag


def test_pooled_attention_strided_outputs_and_rejects():
    """dq / dkv written into a [rows, 3D] gradient buffer (the layer's layout) equal the contiguous outputs bit for bit; bad
    arguments are errors, not launches"""
    from xpretrain_amd import hip_ops as Hh
    B, H, S = 3, 5, 201
    D = H * 64
    q, kv, dout = _inputs(B, H, S, torch.bfloat16, seed=3)
    out, stats = Hh.attn_pooled_fwd(q, kv, B, S, H)
    dq, dkv = Hh.attn_pooled_bwd(q, kv, out, dout, stats, B, S, H, q_scale=Q_SCALE)
    dqkv = torch.zeros(B * S, 3 * D, device="cuda", dtype=torch.bfloat16)
    Hh.attn_pooled_bwd(q, kv, out, dout, stats, B, S, H, q_scale=Q_SCALE, dq=dqkv.view(B, S * 3 * D)[:, :D], dkv=dqkv[:, D:])
    assert torch.equal(dqkv.view(B, S, 3 * D)[:, 0, :D], dq) and torch.equal(dqkv[:, D:], dkv)
    assert not dqkv.view(B, S, 3 * D)[:, 1:, :D].any()              # nothing else is touched
    with pytest.raises(RuntimeError, match="row stride"):
        Hh.L.check(Hh.L.lib().xp_attn_pooled_fwd(q.data_ptr(), kv.data_ptr(), D, out.data_ptr(), stats.data_ptr(), B, H, S, 0,
                                                 stats.data_ptr(), 1 << 20, None), "xp_attn_pooled_fwd")
