#!/usr/bin/env python
"""Micro-benchmarks of the individual HIP kernels at BASELINE cfg #2 shapes (B=8, T=12, 224^2, ViT-B/16).
Run on the GPU box:  python tools/bench_kernels.py [gemm|gemmfwd|ln|attn|all]  -> prints one line per kernel.
`python tools/bench_kernels.py loss [n] [d]`: each kind of xp_contrastive_loss back to back, loss + all gradients per call, at n = m pairs of width d (default 64 x 512: 8 GPUs x 8 pairs).
`python tools/bench_kernels.py act [rounds]`: the two GEMMs that carry the MLP activation (fc1 forward with both outputs, dpre with
fused column sums), quick_gelu (epilogue kinds 3 / 5) against erf GELU (kinds 8 / 9), interleaved.
`python tools/bench_kernels.py probs`: xp_attn_probs (the attention weights of one layer, output_attentions) at cfg #2, bf16 and fp32
storage: the median of individually timed launches after a warm-up, against the time its stores alone need.
`python tools/bench_kernels.py optim [rounds]`: one optimizer step over the parameters of the cfg #2 model (ViT-B/16 + text tower) with
AdamW, Adam and Adamax, alternating within one process; the median of `rounds` (>= 3) rounds and AdamW's own round-to-round spread."""
import sys

import torch

sys.path.insert(0, ".")
from xpretrain_amd import hip_ops as H  # noqa: E402
from xpretrain_amd import _lib as L  # noqa: E402


def timeit(fn, iters=200, warmup=300):     # (sustained clocks: a cold GPU ramps for the first few hundred launches, tools/power_probe.py)
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.record()
    for _ in range(iters):
        fn()
    en.record()
    torch.cuda.synchronize()
    return st.elapsed_time(en) / iters * 1e3   # us


def bench_gemm(fwd_only=False):
    M = 8 * 2356
    bf = torch.bfloat16
    for name, N, K, kw in [("qkv", 2304, 768, dict(epilogue=L.EPI_BIAS_QSCALE, scale=0.125, scale_cols=768)),
                           ("out", 768, 768, dict(epilogue=L.EPI_BIAS_RESID)),
                           ("fc1", 3072, 768, dict(epilogue=L.EPI_BIAS_GELU)),
                           ("fc2", 768, 3072, dict(epilogue=L.EPI_BIAS_RESID))]:
        A = torch.randn(M, K, device="cuda").to(bf)
        W = (torch.randn(N, K, device="cuda") * 0.02).to(bf)
        bias = torch.zeros(N, device="cuda")
        out = torch.empty(M, N, dtype=bf, device="cuda")
        if kw["epilogue"] == L.EPI_BIAS_RESID:
            kw["resid"] = torch.randn(M, N, device="cuda").to(bf)
        if kw["epilogue"] == L.EPI_BIAS_GELU:
            kw["aux"] = torch.empty(M, N, dtype=bf, device="cuda")
        us = timeit(lambda: H.gemm(A, W, M, N, K, out=out, bias=bias, **kw))
        print(f"gemm fwd {name:4s} M={M} N={N} K={K}: {us:8.1f} us  {2*M*N*K/us/1e6:7.1f} TFLOP/s")
        if fwd_only:
            continue
        # dX: dY[M,N] . W[N,K]
        dY = torch.randn(M, N, device="cuda").to(bf)
        dX = torch.empty(M, K, dtype=bf, device="cuda")
        us = timeit(lambda: H.gemm(dY, W, M, K, N, b_kstrided=True, out=dX))
        print(f"gemm dX  {name:4s}: {us:8.1f} us  {2*M*N*K/us/1e6:7.1f} TFLOP/s")
        # dW[N,K] = dY^T X: the production path (functional._wgrad: split-K chosen by xp_gemm_auto_split + deterministic reduce)
        from xpretrain_amd.functional import _wgrad, _split_for
        split = _split_for(N, K, M, bf, (0, 0, 0))        # (the general plan; fc2 / fc1 / out_proj run the "slack" plan inside a layer's backward)
        us = timeit(lambda: _wgrad(dY, A, M, N, K))
        print(f"gemm dW  {name:4s} split={split:2d} (auto): {us:8.1f} us  {2*M*N*K/us/1e6:7.1f} TFLOP/s")
        us = timeit(lambda: H.colsum(dY, M, N))
        print(f"colsum   {name:4s}: {us:8.1f} us  {M*N*2/us/1e3:7.1f} GB/s")


def bench_act(rounds=3):
    """fc1 forward [18848 x 3072 x 768] (+bias, activation, pre-activation kept) and dpre = (dx3 . W2) * act'(pre) with fc1's bias
    gradient fused, per activation; `rounds` interleaved rounds (one GPU drifts by more than the difference between two launches)"""
    M, N, K = 8 * 2356, 3072, 768
    bf = torch.bfloat16
    h2 = torch.randn(M, K, device="cuda").to(bf)
    W1 = (torch.randn(N, K, device="cuda") * 0.02).to(bf)
    b1 = torch.randn(N, device="cuda") * 0.02
    act, pre = (torch.empty(M, N, dtype=bf, device="cuda") for _ in range(2))
    dx3 = torch.randn(M, K, device="cuda").to(bf)
    W2 = (torch.randn(K, N, device="cuda") * 0.02).to(bf)          # fc2's weight [D, Dff], read k-strided
    dpre = torch.empty(M, N, dtype=bf, device="cuda")
    defer = H.DeferredReduce(h2.device)

    def bwd(epi):           # (a fresh DeferredReduce per launch: the launch under test is the GEMM, the second-level reduce is not run)
        H.gemm(dx3, W2, M, N, K, b_kstrided=True, epilogue=epi, resid=pre, out=dpre, colsum_defer=H.DeferredReduce(h2.device))
    H.gemm(h2, W1, M, N, K, out=act, bias=b1, epilogue=L.EPI_BIAS_GELU, aux=pre)
    for r in range(rounds):
        for name, fwd_epi, bwd_epi in (("quick_gelu", L.EPI_BIAS_GELU, L.EPI_GELU_BWD), ("gelu", L.EPI_BIAS_GELU_ERF, L.EPI_GELU_ERF_BWD)):
            plan = H.gemm(dx3, W2, M, N, K, b_kstrided=True, epilogue=bwd_epi, resid=pre, out=dpre, colsum_defer=defer, plan_only=True)
            assert plan["colsum_rows"] > 0, plan
            uf = timeit(lambda: H.gemm(h2, W1, M, N, K, out=act, bias=b1, epilogue=fwd_epi, aux=pre))
            ub = timeit(lambda: bwd(bwd_epi))
            print(f"round {r} {name:10s} fc1 fwd (kind {fwd_epi}): {uf:7.1f} us {2*M*N*K/uf/1e6:6.1f} TFLOP/s | "
                  f"dpre + column sums (kind {bwd_epi}): {ub:7.1f} us {2*M*N*K/ub/1e6:6.1f} TFLOP/s")


def bench_ln():
    M, D = 8 * 2356, 768
    x = torch.randn(M, D, device="cuda").to(torch.bfloat16)
    g, b = torch.ones(D, device="cuda"), torch.zeros(D, device="cuda")
    us = timeit(lambda: H.layernorm_fwd(x, g, b, M, D))
    print(f"layernorm fwd {M}x{D}: {us:7.1f} us  {M*D*4/us/1e3:7.1f} GB/s")
    y, mean, rstd = H.layernorm_fwd(x, g, b, M, D)
    dy = torch.randn_like(x)
    us = timeit(lambda: H.layernorm_bwd(dy, x, g, mean, rstd, M, D, dres=dy))
    print(f"layernorm bwd {M}x{D}: {us:7.1f} us  {M*D*8/us/1e3:7.1f} GB/s")


def bench_attn():
    B, Hh, M, N, Lp = 8, 12, 4, 12, 196
    S = M + N * Lp
    qkv = torch.randn(B * S, 3 * Hh * 64, device="cuda").to(torch.bfloat16)
    us = timeit(lambda: H.attn_fwd(qkv, B, S, Hh, size=(M, N, Lp)))
    flops = 4 * N * Lp * (M + Lp) * 64 * Hh * B + 4 * M * S * 64 * Hh * B
    print(f"attn fwd  B{B} H{Hh} (4,12,196): {us:7.1f} us  {flops/us/1e6:6.1f} TFLOP/s  {4*B*S*Hh*64*2/us/1e3:7.1f} GB/s")
    out, stats = H.attn_fwd(qkv, B, S, Hh, size=(M, N, Lp))
    dout = torch.randn_like(out)
    us = timeit(lambda: H.attn_bwd(qkv, out, dout, stats, B, S, Hh, size=(M, N, Lp), q_scale=0.125))
    print(f"attn bwd  B{B} H{Hh} (4,12,196): {us:7.1f} us  {2.5*flops/us/1e6:6.1f} TFLOP/s")
    ids_mask = torch.ones(8, 32, dtype=torch.int64, device="cuda")
    q2 = torch.randn(8 * 32, 3 * 8 * 64, device="cuda").to(torch.bfloat16)
    us = timeit(lambda: H.attn_fwd(q2, 8, 32, 8, pad_mask=ids_mask))
    print(f"attn fwd  text B8 H8 S32: {us:7.1f} us")


def bench_probs(launches=200, warmup=300):
    """one layer's attention weights at cfg #2: 8 * 12 * (12 * 196 * 200 + 4 * 2356) fp32 = 184.2 MB written, 87 MB of bf16 qkv read"""
    B, Hh, M, N, Lp = 8, 12, 4, 12, 196
    S = M + N * Lp
    for dt in (torch.bfloat16, torch.float32):
        qkv = torch.randn(B * S, 3 * Hh * 64, device="cuda").to(dt)
        _, stats = H.attn_fwd(qkv, B, S, Hh, size=(M, N, Lp))
        out = H.attn_probs(qkv, stats, B, S, Hh, size=(M, N, Lp))
        for _ in range(warmup):
            H.attn_probs(qkv, stats, B, S, Hh, size=(M, N, Lp), out=out)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
        for st, en in ev:
            st.record()
            H.attn_probs(qkv, stats, B, S, Hh, size=(M, N, Lp), out=out)
            en.record()
        torch.cuda.synchronize()
        us = sorted(st.elapsed_time(en) * 1e3 for st, en in ev)
        nbytes = 4 * (out[0].numel() + out[1].numel())
        print(f"attn_probs {str(dt)[6:]:8s} B{B} H{Hh} (4,12,196): median {us[len(us) // 2]:7.1f} us (min {us[0]:.1f}, max {us[-1]:.1f}; both launches)  "
              f"{nbytes / 1e6:.1f} MB written: {nbytes / us[len(us) // 2] / 1e6:5.2f} TB/s of stores, floor {nbytes / 8e6:.1f} us at 8 TB/s")


def bench_loss(n=64, d=512):
    feats = [torch.nn.functional.normalize(torch.randn(n, d, device="cuda"), dim=-1) for _ in range(4)]
    ls = torch.tensor(4.6, device="cuda")
    kinds = ("NCE", "VSC_FC", "DSL", "VS_VC", "VS_VC_FC", "VSC", "VIDIMG", "VIDIMG_DIVIDE")
    runs = [(f"xp_contrastive_loss {k}", lambda k=k: H.contrastive_loss(getattr(L, "XP_LOSS_" + k), *feats, log_scale=ls)) for k in kinds]
    for name, fn in runs:
        print(f"loss n={n} d={d} {name:36s} {timeit(fn):8.1f} us per call (launches back to back, host call included)")


def bench_optim(rounds=3):
    """The update launch alone (`step()`) and with the fused clip (`clip_and_step`: the norm pass in front) per optimizer, on the cfg #2
    parameter set in the reference's four groups, every matrix with its bf16 copy in the weight cache (rewritten in the same pass).
    The three optimizers step the SAME parameter, gradient and state buffers (the state tensors are handed to each under its own
    names): with buffers of their own, the same kernel ran 12 % apart on the three sets on one box and level on another."""
    from xpretrain_amd import optimization as XO
    from xpretrain_amd.functional import WEIGHTS
    from xpretrain_amd.modeling import VidCLIP
    from xpretrain_amd.workload import ModelArgs, vit_b_config
    rounds = max(3, rounds)
    named = [(n, tuple(p.shape)) for n, p in VidCLIP(ModelArgs(vit_b_config())).named_parameters() if p.requires_grad]
    params = [torch.nn.Parameter(torch.randn(s, device="cuda") * 0.02) for _, s in named]
    state = [(torch.zeros_like(p), torch.zeros_like(p)) for p in params]
    for p in params:
        p.grad = torch.randn_like(p) * 0.01
        if p.ndim >= 2:
            WEIGHTS.get(p, torch.bfloat16)
    runs = {}
    for name, cls, keys in (("adamw", XO.AdamW, ("exp_avg", "exp_avg_sq")), ("adam", XO.Adam, ("exp_avg", "exp_avg_sq")),
                            ("adamax", XO.Adamax, ("exp_avg", "exp_inf"))):
        groups = XO.build_e2e_optimizer_w_lr_mul([(n, p) for (n, _), p in zip(named, params)], 1e-6, 0.2, lr_mul=1, lr_mul_prefix="")
        runs[name] = cls([g for g in groups if g["params"]], lr=1e-6, betas=(0.9, 0.98))
        for p, (a, b) in zip(params, state):
            runs[name].state[p] = {"step": 0, keys[0]: a, keys[1]: b}
    numel = sum(p.numel() for g in runs["adamw"].param_groups for p in g["params"])
    print(f"optimizer step, cfg #2 parameter set: {len(named)} tensors, {numel / 1e6:.1f} M elements, {numel * 30 / 1e9:.2f} GB per update pass")
    times = {k: ([], []) for k in runs}
    for r in range(rounds):
        for name, opt in runs.items():
            times[name][0].append(timeit(opt.step))
            times[name][1].append(timeit(lambda: opt.clip_and_step(1.0)))
            print(f"round {r} {name:6s} update {times[name][0][-1]:7.1f} us | norm + clipped update {times[name][1][-1]:7.1f} us")
    med = {k: [sorted(v)[len(v) // 2] for v in t] for k, t in times.items()}
    for i, what in enumerate(("update", "norm + clipped update")):
        base = times["adamw"][i]
        print(f"{what}: adamw median {med['adamw'][i]:.1f} us ({numel * 30 / med['adamw'][i] / 1e6:.2f} TB/s), round-to-round spread "
              f"{(max(base) - min(base)) / med['adamw'][i] * 100:.2f} % | "
              + " | ".join(f"{k} median {med[k][i]:.1f} us = {(med[k][i] / med['adamw'][i] - 1) * 100:+.2f} % of adamw" for k in ("adam", "adamax")))


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    if what in ("gemm", "all"):
        bench_gemm()
    if what == "gemmfwd":
        bench_gemm(fwd_only=True)
    if what == "act":
        bench_act(int(sys.argv[2]) if len(sys.argv) > 2 else 3)
    if what == "loss":
        bench_loss(*(int(a) for a in sys.argv[2:4]))
    if what == "probs":
        bench_probs()
    if what == "optim":
        bench_optim(int(sys.argv[2]) if len(sys.argv) > 2 else 3)
    if what in ("ln", "all"):
        bench_ln()
    if what in ("attn", "all"):
        bench_attn()
