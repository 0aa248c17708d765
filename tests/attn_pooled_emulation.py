"""A CPU restatement of the single-query proxy attention kernels (csrc/attention_pooled.hip), for deriving per-class error bounds
without a GPU (plain helper module): the cases and seeded inputs that tests/test_attention_pooled_guarded_gpu.py runs, the fp64
reference (plain softmax over all S keys of one query, with autograd), and ``emulate``: the kernels' formulas in a working precision
with their STORAGE roundings only --

    out = rnd( sum_j e_j v_j / l ),  e_j = exp(s_j - m), l = sum_j e_j             (lse = m + log l: what ``stats`` holds)
    p_j = exp((s_j - m) - log l)                                                     (P is NOT rounded before the products: the kernel
    delta = dO . out  from the STORED output                                           keeps it in fp32; tests/attn_emulation.py, the dense
    dV_j = rnd( p_j dO ),  dS_j = p_j (dO . v_j - delta),  dK_j = rnd( dS_j q )        kernels' restatement, rounds it as an MFMA operand)
    dq   = rnd( q_scale sum_j dS_j k_j )

With ``work = float64, store = bfloat16`` that is what correct bf16-storage arithmetic gives against fp64 (the bf16 bounds); with
``work = float32, store = None`` it is the same formulas in fp32 (the fp32-mode bounds).  Nothing here is measured on a GPU.

Classes, each held to max|a - ref| over the class / max|ref| over the class (``class_errors``; one worst value per class kind):
``out`` / ``dq`` / ``dk`` / ``dv`` per problem (b, h) in both regimes, and in the flat regime ``dk`` / ``dv`` also per (b, h, block of
32 consecutive keys).  32 is CHUNK_ALIGN: every chunk any device's plan can cut is a union of such blocks, so the classes need no
knowledge of the device.  In the peaked regime a block's reference is down to 1e-7 of the tensor's and the correct restatement
itself is off by a large fraction of such a block's scale, so blocks are not classes there.  A class whose reference is exactly zero
must be reproduced exactly (tests/attn_emulation.py::class_error): 0 -> 0.0, anything else -> inf."""
import functools
import math

import torch

from tests.attn_emulation import Q_SCALE, REGIMES          # peaked: q as drawn (scores of standard deviation 8); flat: q * 0.125

BLOCK = 32                                                  # CHUNK_ALIGN of csrc/attention_pooled.hip
DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
# (B, H, S) -> (chunks, chunk_keys) of plan_pooled on a 256-CU device (tests/test_attention_pooled_class_bounds_cpu.py asserts it)
GEOMS = {
    (2, 2, 1): (1, 32),         # a single key
    (1, 2, 9): (1, 32),         # fewer keys than one wave step: most lane groups stay empty (m = -inf merges)
    (2, 2, 33): (1, 64),        # the second 32-key block holds one key
    (2, 2, 65): (2, 64),        # the last chunk holds one key
    (1, 1, 129): (3, 64),       # one problem only; the last chunk holds one key
    (3, 5, 201): (4, 64),       # the last chunk holds 9 keys
    (2, 2, 904): (15, 64),      # the last chunk holds 8 keys
    (1, 2, 4096): (64, 64),     # MAX_CHUNKS, exact fit
    (4, 16, 1100): (7, 160),    # more than one workgroup step per chunk (bf16 128 + 32, fp32 64 + 64 + 32); the last chunk holds 140
}


def case_id(B, H, S):
    return f"B{B}H{H}S{S}"


CASES = {case_id(*g): g for g in GEOMS}
QUANTITIES = ("out", "dq", "dk", "dv")


def lse_bound(S):
    """absolute bound on stats[..., 0] + stats[..., 1]: the existing 1e-3, and an eighth of what one key of uniform weight moves the
    logsumexp by (log S - log(S - 1) ~ 1 / S): a condition, not a measurement"""
    return min(1e-3, 1.0 / (8 * S))


def uniform_dv_bound(dt, S):
    """relative bound on dv = dout / S under uniform weights (q = 0), per element.  bf16: one rounding of the storage type, 2^-8
    (the fp32 arithmetic underneath, ~1e-6, is 2^-8 of the slack a bf16 rounding leaves below 2^-8).  fp32: one rounding, u = 2^-24,
    is NOT attainable by any float32 evaluation of p = exp(-log l) with log l stored as a float32, which is what ``stats`` holds --
    the stored log S alone is off by u log S, and torch's float32 restatement on the CPU is off by up to 5.3 u
    (tests/test_attention_pooled_class_bounds_cpu.py).  So the operations' own errors are added to the one rounding, in u relative
    to p: log l rounded to float32 (log S) and __logf's documented 1 ulp on it (2 log S); __expf(x) = exp2(x log2 e), whose rounded
    product moves the result by |x| = log S, and exp2's documented 1 ulp (2); the product p dO (the one rounding): (4 log S + 3) u.
    That is 36 u = 2.2e-6 at S = 4096, where a dropped key is worth 1 / S = 2.4e-4."""
    return 2.0 ** -8 if dt == "bf16" else (4 * math.log(S) + 3) * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def inputs(case, regime, dtype):
    """(q [B, H*64], kv [B*S, 2*H*64] = [k | v] rows, dout [B, H*64]) on the CPU, rounded to `dtype`, from a seeded CPU generator:
    the GPU test and the CPU bounds test see the same numbers.  Shared: never modify."""
    B, H, S = CASES[case]
    g = torch.Generator().manual_seed(2000 + 7 * S + H)
    q = torch.randn(B, H * 64, generator=g) * REGIMES[regime]
    kv = torch.randn(B * S, 2 * H * 64, generator=g)
    dout = torch.randn(B, H * 64, generator=g)
    return q.to(dtype), kv.to(dtype), dout.to(dtype)


def split(q, kv, dout, B, H, S):
    """-> fp64 q, dout [B, H, 64] and k, v [B, S, H, 64]"""
    k, v = kv.double().view(B, S, 2, H, 64).unbind(2)
    return q.double().view(B, H, 64), k, v, dout.double().view(B, H, 64)


def forward_reference(q, k, v):
    """fp64 out [B, H, 64] and lse [B, H] of plain softmax attention of one query per (b, h) over the keys given"""
    s = torch.einsum("bhd,bshd->bhs", q, k)
    return torch.einsum("bhs,bshd->bhd", torch.softmax(s, -1), v), torch.logsumexp(s, -1)


def reference(q, k, v, dout, q_scale=Q_SCALE):
    """fp64 softmax over all keys with autograd: out, dq (times q_scale) [B, H, 64], dk, dv [B, S, H, 64], lse [B, H]"""
    q, k, v = [t.detach().clone().requires_grad_() for t in (q, k, v)]
    out, lse = forward_reference(q, k, v)
    out.backward(dout)
    return {"out": out.detach(), "dq": q.grad * q_scale, "dk": k.grad, "dv": v.grad, "lse": lse.detach()}


def emulate(q, k, v, dout, *, work=torch.float64, store=torch.bfloat16, q_scale=Q_SCALE):
    """the restatement (module docstring) in `work` precision.  dO . v_j and delta = dO . out are the same expression (a product and
    a sum over the 64 elements), as in the kernel: with one key, where out == v, they cancel exactly."""
    rnd = (lambda t: t) if store is None else (lambda t: t.to(store).to(work))
    q, k, v, dout = [t.to(work) for t in (q, k, v, dout)]
    s = torch.einsum("bhd,bshd->bhs", q, k)
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    out = rnd(torch.einsum("bhs,bshd->bhd", e, v) / l)
    p = torch.exp((s - m) - torch.log(l)).transpose(1, 2)                   # [B, S, H]
    delta = (dout * out).sum(-1)                                            # [B, H]
    ds = p * ((dout[:, None] * v).sum(-1) - delta[:, None])
    return {"out": out, "lse": (m + torch.log(l)).squeeze(-1), "dv": rnd(p[..., None] * dout[:, None]),
            "dk": rnd(ds[..., None] * q[:, None]), "dq": rnd(torch.einsum("bsh,bshd->bhd", ds, k) * q_scale)}


def _ratio(d, sc):
    """per-class max|a - ref| / max|ref|, worst class; an exactly-zero reference must be reproduced exactly"""
    r = torch.where(sc > 0, d / sc.clamp_min(1e-300), torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, math.inf)))
    return r.max().item()


def class_errors(got, ref, regime):
    """{"quantity/class kind": worst class error}: out, dq, dk, dv per problem (b, h); in the flat regime dk and dv also per
    (b, h, block of 32 consecutive keys).  got / ref: out, dq [B, H, 64], dk, dv [B, S, H, 64]."""
    errs = {}
    for n in QUANTITIES:
        d, r = (got[n].double().cpu() - ref[n].double().cpu()).abs(), ref[n].double().cpu().abs()
        if n in ("out", "dq"):
            errs[f"{n}/problem"] = _ratio(d.amax(-1), r.amax(-1))
            continue
        d, r = d.amax(-1), r.amax(-1)                                        # [B, S, H]
        errs[f"{n}/problem"] = _ratio(d.amax(1), r.amax(1))
        if regime == "flat":
            S = d.shape[1]
            pad = (-S) % BLOCK                                               # (a zero row changes no maximum of absolute values)
            d, r = [torch.nn.functional.pad(t, (0, 0, 0, pad)).view(t.shape[0], -1, BLOCK, t.shape[2]) for t in (d, r)]
            errs[f"{n}/block"] = _ratio(d.amax(2), r.amax(2))
    return errs


def class_kinds(regime):
    return [f"{n}/problem" for n in QUANTITIES] + ([f"{n}/block" for n in ("dk", "dv")] if regime == "flat" else [])


@functools.lru_cache(maxsize=None)
def case_reference(case, regime, dtype):
    """the fp64 reference on the case's rounded inputs, computed once and shared (never modify)"""
    return reference(*split(*inputs(case, regime, dtype), *CASES[case]))


def restated(case, regime, dtype):
    """the restatement on the case's inputs: bf16 -> fp64 arithmetic with bf16 storage roundings, float32 -> the formulas in float32"""
    ops = split(*inputs(case, regime, dtype), *CASES[case])
    if dtype == torch.bfloat16:
        return emulate(*ops)
    threads = torch.get_num_threads()           # a float32 sum split over threads has another order: the recorded errors are those
    try:                                        # of one thread, whatever the machine offers (2 threads: up to 1.9 x in a small class)
        torch.set_num_threads(1)
        return emulate(*ops, work=torch.float32, store=None)
    finally:
        torch.set_num_threads(threads)


def restated_class_errors(case, regime, dtype):
    """({"quantity/class kind": error}, max|lse - ref|) of the restatement against the fp64 reference"""
    ref, emu = case_reference(case, regime, dtype), restated(case, regime, dtype)
    return class_errors(emu, ref, regime), (emu["lse"].double() - ref["lse"]).abs().max().item()


# ---- wrong results: what the classes must notice.  Each is applied to a CORRECT (fp64) result.
MUTANTS = ("last_block_dkv_zero", "last_key_dropped", "last_key_doubled")


def mutate(name, ref, q, k, v, dout):
    """a copy of the fp64 result `ref` with one mistake: dk and dv of the last 32-key block written as zero; the last key of the
    sequence left out of the forward; the last key counted twice (the clamp min(j, k1 - 1) without its `valid` test, once)"""
    res = {n: t.clone() for n, t in ref.items()}
    S = k.shape[1]
    if name == "last_block_dkv_zero":
        first = (S - 1) // BLOCK * BLOCK
        res["dk"][:, first:] = 0
        res["dv"][:, first:] = 0
    elif name == "last_key_dropped":
        res["out"], res["lse"] = forward_reference(q, k[:, :-1], v[:, :-1])
    elif name == "last_key_doubled":
        res["out"], res["lse"] = forward_reference(q, torch.cat([k, k[:, -1:]], 1), torch.cat([v, v[:, -1:]], 1))
    else:
        raise KeyError(name)
    return res
