"""A CPU restatement of the attention kernels' arithmetic, for deriving per-row-class error bounds without a GPU (plain helper
module): the cases and seeded inputs that tests/test_attention_guarded_gpu.py runs, the fp64 reference (the oracle's cores with
autograd), and ``emulate``: dense masked attention in a working precision with the kernels' storage roundings --

    O  = rnd( rnd(e) V / l ),  e = exp(S - m) unnormalised, l = rowsum(e)        (forward: P enters the matrix product rounded)
    dV = rnd( rnd(P)^T dO ),   P = e / l
    dS = rnd( P o (dO V^T - delta) ),  delta = rowsum(dO o O) from the STORED output
    dQ = rnd( q_scale dS K ),  dK = rnd( dS^T Q )

With ``work = float64, rnd = bf16`` that is what correct bf16-storage arithmetic gives against fp64 (the bf16 bounds); with ``work =
float32, rnd = identity`` it is the same formulas in fp32 (the fp32-mode bounds).  Nothing here is measured on a GPU."""
import functools

import torch

from oracle import clipvip_oracle as O

Q_SCALE = 0.125
REGIMES = {"peaked": 1.0, "flat": 0.125}       # q as drawn (scores of standard deviation 8: near one-hot rows) / q * 0.125

# ---- the cases: (name, size (M, N, L) or None, B, H, S, causal mask mode or None)
PROXY = [((1, 3, 5), 2, 1), ((4, 12, 196), 1, 2), ((4, 3, 70), 1, 3), ((4, 3, 300), 2, 2), ((4, 5, 208), 1, 2), ((17, 2, 180), 1, 1),
         ((20, 3, 49), 1, 2), ((4, 2, 49), 2, 2)]
CAUSAL = [(2, 77, 2, "ragged"), (2, 16, 2, "allpad"), (1, 130, 1, "none")]


def case_id(size, B, H, S, mode):
    return (f"proxy{size[0]}x{size[1]}x{size[2]}" if size is not None else f"causal{S}{mode}") + f"-B{B}H{H}"


CASES = {}
for _size, _B, _H in PROXY:
    CASES[case_id(_size, _B, _H, _size[0] + _size[1] * _size[2], None)] = (_size, _B, _H, _size[0] + _size[1] * _size[2], None)
for _B, _S, _H, _mode in CAUSAL:
    CASES[case_id(None, _B, _H, _S, _mode)] = (None, _B, _H, _S, _mode)


def pad_mask_of(B, S, mode):
    """the padding masks of tests/test_attention_gpu.py: ragged lengths (sample 0 full), `allpad`: sample 1 entirely padded"""
    if mode in (None, "none"):
        return None
    g = torch.Generator().manual_seed(S)
    lens = torch.randint(1, S + 1, (B,), generator=g)
    lens[0] = S
    mask = (torch.arange(S)[None] < lens[:, None]).long()
    if mode == "allpad":
        mask[1] = 0
    return mask


@functools.lru_cache(maxsize=None)
def inputs(case, regime, dtype):
    """(qkv [B*S, 3*H*64], dout [B*S, H*64], pad mask or None) on the CPU, rounded to `dtype`, from a seeded CPU generator: the GPU
    test and the CPU bounds test see the same numbers.  Shared: never modify."""
    size, B, H, S, mode = CASES[case]
    g = torch.Generator().manual_seed(1000 + 7 * S + H)
    qkv = torch.randn(B * S, 3, H * 64, generator=g)
    qkv[:, 0] *= REGIMES[regime]
    dout = torch.randn(B * S, H * 64, generator=g)
    return qkv.view(B * S, 3 * H * 64).to(dtype), dout.to(dtype), pad_mask_of(B, S, mode)


def split_heads(qkv, B, S, H):
    """[B*S, 3*H*64] -> q, k, v as fp64 [B, H, S, 64]"""
    q, k, v = qkv.view(B, S, 3, H, 64).double().unbind(2)
    return [t.transpose(1, 2) for t in (q, k, v)]


def additive_mask(size, S, pad, dtype, device="cpu"):
    """the additive score mask [1 or B, 1, S, S]: -inf outside the proxy pattern / above the diagonal, finfo.min on padded keys"""
    if size is not None:
        M, N, L = size
        frame = torch.full((S,), -1, dtype=torch.long, device=device)
        frame[M:] = torch.arange(N, device=device).repeat_interleave(L)
        allow = (frame[:, None] == frame[None, :]) | (frame[None, :] < 0) | (frame[:, None] < 0)
        return torch.zeros((S, S), dtype=dtype, device=device).masked_fill(~allow, float("-inf"))[None, None]
    add = torch.full((S, S), float("-inf"), dtype=dtype, device=device).triu(1)[None, None]
    if pad is not None:
        inv = 1.0 - pad.to(device=device, dtype=dtype)[:, None, None, :]
        add = add + inv.masked_fill(inv.bool(), torch.finfo(dtype).min)
    return add


def reference(q, k, v, dout, size, pad, q_scale=Q_SCALE):
    """the oracle's fp64 cores and autograd on [B, H, S, 64] fp64 operands (any device), as tests/test_attention_gpu.py::_run:
    out, dq (times q_scale), dk, dv as [B, H, S, 64] and the row logsumexp of the masked scores [B, H, S]"""
    q, k, v = [t.detach().clone().requires_grad_() for t in (q, k, v)]
    pad = None if pad is None else pad.to(q.device)
    ref = O.proxy_attention_core(q, k, v, size) if size is not None else O.masked_attention_core(q, k, v, pad)
    ref.backward(dout)
    B, H, S, _ = q.shape
    lse = torch.empty(B, H, S, dtype=q.dtype, device=q.device)
    add = additive_mask(size, S, pad, q.dtype, q.device)
    for b in range(B):            # (one sample at a time: S x S scores per head)
        lse[b] = torch.logsumexp(q[b].detach() @ k[b].detach().transpose(-1, -2) + add[min(b, add.shape[0] - 1)], -1)
    return {"out": ref.detach(), "dq": q.grad * q_scale, "dk": k.grad, "dv": v.grad, "lse": lse}


def emulate(q, k, v, dout, size, pad, *, work=torch.float64, store=torch.bfloat16, q_scale=Q_SCALE):
    """the restatement (module docstring) on [B, H, S, 64] operands: out, dq, dk, dv, lse in `work` precision"""
    rnd = (lambda t: t) if store is None else (lambda t: t.to(store).to(work))
    q, k, v, dout = [t.to(work) for t in (q, k, v, dout)]
    B, H, S, _ = q.shape
    add = additive_mask(size, S, pad, work)
    res = {n: torch.empty_like(q) for n in ("out", "dq", "dk", "dv")}
    res["lse"] = torch.empty(B, H, S, dtype=work)
    for b in range(B):
        s = q[b] @ k[b].transpose(-1, -2) + add[min(b, add.shape[0] - 1)]
        m = s.max(-1, keepdim=True).values
        e = torch.exp(s - m)
        l = e.sum(-1, keepdim=True)
        o = rnd((rnd(e) @ v[b]) / l)
        p = e / l
        delta = (dout[b] * o).sum(-1, keepdim=True)
        ds = rnd(p * (dout[b] @ v[b].transpose(-1, -2) - delta))
        res["out"][b], res["lse"][b] = o, (m + torch.log(l)).squeeze(-1)
        res["dv"][b] = rnd(rnd(p).transpose(-1, -2) @ dout[b])
        res["dq"][b] = rnd((ds @ k[b]) * q_scale)
        res["dk"][b] = rnd(ds.transpose(-1, -2) @ q[b])
    return res


def row_classes(size, B, S, pad):
    """{class name: bool [B, S]} -- the row classes held to their own scale: proxy / frame rows of a proxy problem, kept / padded
    positions of a causal problem with a padding mask, everything otherwise"""
    if size is not None:
        proxy = torch.zeros(B, S, dtype=torch.bool)
        proxy[:, :size[0]] = True
        return {"proxy": proxy, "frame": ~proxy}
    if pad is not None:
        return {"kept": pad.bool().cpu(), "padded": ~pad.bool().cpu()}
    return {"all": torch.ones(B, S, dtype=torch.bool)}


def class_error(a, ref, rows):
    """max|a - ref| over the rows of the class / max|ref| over them; a class whose reference is exactly zero (the dk / dv of padded
    keys) must be reproduced exactly: 0 -> 0.0, anything else -> inf.  a, ref [B, H, S, 64]; rows bool [B, S]."""
    a, ref = a.double().cpu().transpose(1, 2)[rows], ref.double().cpu().transpose(1, 2)[rows]
    if a.numel() == 0:
        return 0.0
    d, sc = (a - ref).abs().max().item(), ref.abs().max().item()
    return d / sc if sc > 0 else (0.0 if d == 0 else float("inf"))


def restated_class_errors(case, regime, dtype):
    """{(quantity, class): error} of the restatement against the fp64 reference on the case's inputs: bf16 -> fp64 arithmetic with
    bf16 storage roundings, float32 -> the same formulas evaluated in float32"""
    size, B, H, S, mode = CASES[case]
    qkv, dout, pad = inputs(case, regime, dtype)
    q, k, v = split_heads(qkv, B, S, H)
    do = dout.view(B, S, H, 64).double().transpose(1, 2)
    ref = reference(q, k, v, do, size, pad)
    if dtype == torch.bfloat16:
        emu = emulate(q, k, v, do, size, pad)
    else:
        emu = emulate(q, k, v, do, size, pad, work=torch.float32, store=None)
    cls = row_classes(size, B, S, pad)
    return {(n, c): class_error(emu[n], ref[n], rows) for n in ("out", "dq", "dk", "dv") for c, rows in cls.items()}
