"""GPU: the attention-weights kernel (csrc/attention_probs.hip, ``hip_ops.attn_probs``) against the fp64 restatement on the kernel's
own inputs.  Inputs as in tests/test_attention_gpu.py::_run -- randn qkv in the storage dtype, ``stats`` from ``attn_fwd`` on them
-- so the row sums also check the statistics the fused forward kernels leave behind, which nothing else reads directly.

Gates (every case): the deviation bound tol = 2e-5 + 3 * 64 * 2^-24 * A with A = max over the visible (query, key) pairs of
sum_d |q_d k_d| in fp64 -- 2e-5 is the fp32 forward gate of test_attention_gpu.py, the second term the worst-case fp32 error of two
64-term dot products plus the statistics, each entering the exponent once; a bound, not a measurement.  Row sums within tol of 1.
Exact zeros above the causal diagonal and at padded keys; the all-padded sample uniform.  Guard buffers around the outputs, every
element written.  P @ V in fp64 against ``attn_fwd``'s own output at that file's gates.  Two calls bit-identical."""
import pytest
import torch

from tests import attn_probs_ref as R
from tests.gpu_util import report
from tests.guarded import Guarded, _SENT

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
PROXY_CASES = [((1, 3, 5), 2, 1), ((4, 2, 49), 2, 2), ((4, 3, 70), 1, 3), ((4, 5, 208), 1, 2), ((20, 3, 49), 1, 2),
               ((4, 12, 196), 1, 2), ((4, 2, 784), 1, 1)]
PROXY_PARAMS = [(c, BF) for c in PROXY_CASES] + [(PROXY_CASES[i], F32) for i in (0, 1, -1)]
SPIKE_CASE = ((4, 3, 196), 1, 2)          # test_proxy_attention_rescale_and_qscale: scale 2.0, one late key dominates one row
CAUSAL_CASES = [(3, 12, 2, "ragged"), (2, 7, 1, "none"), (2, 77, 2, "ragged"), (2, 16, 2, "allpad"), (1, 130, 1, "ragged")]
OUT_GATE = {BF: 1.2e-2, F32: 2e-5}        # attn_fwd's output against fp64 (tf in test_attention_gpu.py)


def _split(qkv, B, S, H):
    q, k, v = qkv.view(B, S, 3, H, 64).double().unbind(2)
    return [t.transpose(1, 2) for t in (q, k, v)]                  # [B,H,S,64]


def _inputs(B, S, H, size, pad_mask, seed, dtype, scale=1.0, spike=False):
    from xpretrain_amd import hip_ops as Hh
    torch.manual_seed(seed)
    qkv = (torch.randn(B * S, 3 * H * 64, device="cuda") * scale).to(dtype)
    if spike:
        v = qkv.view(B, S, 3, H, 64)
        v[0, S - 1, 1, 0] = v[0, S // 2, 0, 0] * 6.0
    out, stats = Hh.attn_fwd(qkv, B, S, H, size=size, pad_mask=pad_mask)
    return qkv, out, stats


def _tol(score_mats):
    """2e-5 + 3 * 64 * 2^-24 * A, A over the |q|.|k| matrices in the layout of the weights (visible pairs only)"""
    A = max(m.max().item() for m in score_mats)
    return 2e-5 + 3 * 64 * 2.0 ** -24 * A, A


def _guarded(shape):
    cols = shape[-1]
    g = Guarded(int(torch.Size(shape).numel()) // cols, cols, F32)
    return g


def _all_written(tag, g):
    g.check(tag, g.rows, g.cols)
    itype, sent = _SENT[F32]
    assert not (g.mat.view(itype) == sent).any().item(), f"{tag}: elements of the output still hold the sentinel"


def _gates(tag, P, P64, tol):
    dev = report(tag, P, P64, tol, scale_floor=1.0)               # weights are <= 1: the absolute deviation
    rows = (P.double().sum(-1) - 1).abs().max().item()
    print(f"{tag}: max |row sum - 1| = {rows:.3e} tol={tol:.1e}")
    assert (P.double() - P64).abs().max().item() <= tol, tag
    assert rows <= tol, tag + " row sums"
    return dev


def _run_proxy(size, B, H, dtype, seed, scale=1.0, spike=False):
    from xpretrain_amd import hip_ops as Hh
    M, N, L = size
    S = M + N * L
    qkv, out, stats = _inputs(B, S, H, size, None, seed, dtype, scale, spike)
    q, k, v = _split(qkv, B, S, H)
    proxy64, frame64 = R.proxy_probs(q, k, size)
    qa, ka = q.abs(), k.abs()
    kk = torch.cat([ka[:, :, :M].unsqueeze(2).expand(B, H, N, M, 64), ka[:, :, M:].reshape(B, H, N, L, 64)], dim=3)
    tol, A = _tol([qa[:, :, :M] @ ka.transpose(-1, -2), qa[:, :, M:].reshape(B, H, N, L, 64) @ kk.transpose(-1, -2)])
    gp, gf = _guarded((B, H, M, S)), _guarded((B, H, N, L, M + L))
    assert (gp.rows, gp.cols, gf.rows, gf.cols) == (B * H * M, S, B * H * N * L, M + L)
    proxy, frame = Hh.attn_probs(qkv, stats, B, S, H, size=size, out=(gp.mat, gf.mat))
    assert proxy.shape == (B, H, M, S) and frame.shape == (B, H, N, L, M + L) and proxy.dtype == frame.dtype == F32
    assert proxy.data_ptr() == gp.mat.data_ptr() and frame.data_ptr() == gf.mat.data_ptr()
    tag = f"attn_probs {str(dtype)[6:]} B{B} H{H} size{size} A={A:.1f}"
    _all_written(tag + " proxy", gp); _all_written(tag + " frame", gf)
    _gates(tag + " proxy", proxy, proxy64, tol)
    _gates(tag + " frame", frame, frame64, tol)
    if not spike:
        o = R.proxy_pv(proxy.double(), frame.double(), v, size).transpose(1, 2).reshape(B * S, H * 64)
        assert report(tag + " P@V vs attn_fwd", out, o, OUT_GATE[dtype]) <= OUT_GATE[dtype], tag
    again = Hh.attn_probs(qkv, stats, B, S, H, size=size)
    assert torch.equal(again[0], proxy) and torch.equal(again[1], frame), tag + ": two calls differ"


@pytest.mark.parametrize("case,dtype", PROXY_PARAMS)
def test_proxy_attention_weights(case, dtype):
    (M, N, L), B, H = case
    _run_proxy((M, N, L), B, H, dtype, seed=M + N + L)


def test_proxy_attention_weights_spike():
    (M, N, L), B, H = SPIKE_CASE
    _run_proxy((M, N, L), B, H, BF, seed=5, scale=2.0, spike=True)


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("B,S,H,mode", CAUSAL_CASES)
def test_causal_attention_weights(B, S, H, mode, dtype):
    from xpretrain_amd import hip_ops as Hh
    torch.manual_seed(S)
    mask = None
    if mode != "none":
        lens = torch.randint(1, S + 1, (B,)); lens[0] = S
        mask = (torch.arange(S)[None] < lens[:, None]).long()
        if mode == "allpad":
            mask[1] = 0
        mask = mask.cuda()
    qkv, out, stats = _inputs(B, S, H, None, mask, S + 1, dtype)
    q, k, v = _split(qkv, B, S, H)
    P64 = R.causal_probs(q, k, mask)
    tol, A = _tol([(q.abs() @ k.abs().transpose(-1, -2)).tril()])
    g = _guarded((B, H, S, S))
    assert (g.rows, g.cols) == (B * H * S, S)
    P = Hh.attn_probs(qkv, stats, B, S, H, pad_mask=mask, out=g.mat)
    assert P.shape == (B, H, S, S) and P.dtype == F32 and P.data_ptr() == g.mat.data_ptr()
    tag = f"attn_probs {str(dtype)[6:]} causal B{B} S{S} H{H} {mode} A={A:.1f}"
    _all_written(tag, g)                                            # the upper triangle included: it is written
    _gates(tag, P, P64, tol)
    assert torch.equal(P.triu(1), torch.zeros_like(P)), tag + ": upper triangle"
    if mask is not None:
        sees_kept = (mask[:, None, :].expand(B, S, S).tril().sum(-1) > 0)[:, None, :, None]         # [B,1,S,1] by query row
        dead = (sees_kept & (mask == 0)[:, None, None, :]).expand_as(P)
        assert torch.equal(P[dead], torch.zeros(int(dead.sum()), device="cuda")), tag + ": padded keys"
    if mode == "allpad":
        want = (1.0 / torch.arange(1, S + 1, dtype=torch.float64, device="cuda"))[:, None].expand(S, S).tril()
        assert (P[1].double() - want).abs().max().item() <= tol, tag + ": the all-padded sample is not uniform"
    o = R.causal_pv(P.double(), v).transpose(1, 2).reshape(B * S, H * 64)
    assert report(tag + " P@V vs attn_fwd", out, o, OUT_GATE[dtype]) <= OUT_GATE[dtype], tag
    assert torch.equal(Hh.attn_probs(qkv, stats, B, S, H, pad_mask=mask), P), tag + ": two calls differ"


def test_attn_probs_refusals():
    from xpretrain_amd import hip_ops as Hh
    B, S, H = 3, 10, 1
    qkv = torch.zeros(B * S, 3 * 64, dtype=BF, device="cuda")
    stats = torch.zeros(B, H, S, 2, device="cuda")
    with pytest.raises(RuntimeError, match="no CPU path"):
        Hh.attn_probs(qkv.cpu(), stats, B, S, H)
    with pytest.raises(RuntimeError, match="no CPU path"):
        Hh.attn_probs(qkv, stats.cpu(), B, S, H)
    with pytest.raises(TypeError):
        Hh.attn_probs(qkv, stats.to(BF), B, S, H)
    with pytest.raises(TypeError):
        Hh.attn_probs(qkv.half(), stats, B, S, H)
    with pytest.raises(RuntimeError, match="M\\+N\\*L"):
        Hh.attn_probs(qkv, stats, B, S, H, size=(4, 2, 2))
    with pytest.raises(RuntimeError):
        Hh.attn_probs(qkv, stats, B, S, H, size=(2, 2, 4), pad_mask=torch.ones(B, S, dtype=torch.int64, device="cuda"))
