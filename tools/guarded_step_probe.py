#!/usr/bin/env python
"""What the step guard (``skip_nonfinite=True``) costs the optimizer step, measured against the unguarded step in the same process.

Run on the GPU box:  python tools/guarded_step_probe.py [rounds]   (>= 5 rounds; prints the table profiles/guarded_step_probe.txt holds)

The cfg #2 parameter set (ViT-B/16 + text tower) in the reference's four groups, every matrix with its bf16 copy in the weight cache, the
optimizer alone: no forward, no backward.  A guarded and an unguarded AdamW step the SAME parameter, gradient and state buffers
(tools/bench_kernels.py optim: buffers matter more than kernels here), alternating within every round, timed with device events over
back-to-back steps after a warm-up.  Per round:
  clip on    unguarded: partials + update                 guarded: partials + verdict + guarded update     (the guard adds one launch)
  clip off   unguarded: update                            guarded: partials + verdict + guarded update     (the guard adds the norm pass)
  verdict    xp_step_verdict alone, back to back, over this plan's partials
The guarded optimizer's next step() waits for the previous step's verdict on the host; in training a forward and a backward lie between
the two, here nothing does, so the columns above drop that wait (the probe forgets the pending verdict after every step; all gradients are
finite) and the last column keeps it, to show what back-to-back guarded steps with nothing between them pay."""
import ctypes as C
import sys

import torch

sys.path.insert(0, ".")
from xpretrain_amd import _lib as L  # noqa: E402
from xpretrain_amd import hip_ops as H  # noqa: E402


def timeit(fn, iters=100, warmup=200):
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


def main(rounds):
    from xpretrain_amd import optimization as XO
    from xpretrain_amd.functional import WEIGHTS
    from xpretrain_amd.modeling import VidCLIP
    from xpretrain_amd.workload import ModelArgs, vit_b_config
    named = [(n, tuple(p.shape)) for n, p in VidCLIP(ModelArgs(vit_b_config())).named_parameters() if p.requires_grad]
    params = [torch.nn.Parameter(torch.randn(s, device="cuda") * 0.02) for _, s in named]
    state = [(torch.zeros_like(p), torch.zeros_like(p)) for p in params]
    for p in params:
        p.grad = torch.randn_like(p) * 0.01
        if p.ndim >= 2:
            WEIGHTS.get(p, torch.bfloat16)
    opts = {}
    for guard in (False, True):
        groups = XO.build_e2e_optimizer_w_lr_mul([(n, p) for (n, _), p in zip(named, params)], 1e-6, 0.2, lr_mul=1, lr_mul_prefix="")
        opts[guard] = XO.AdamW([g for g in groups if g["params"]], lr=1e-6, betas=(0.9, 0.98), skip_nonfinite=guard)
        for p, (a, b) in zip(params, state):
            opts[guard].state[p] = {"step": 0, "exp_avg": a, "exp_avg_sq": b}
    plain, guarded = opts[False], opts[True]
    numel = sum(p.numel() for p in params)

    def g_step(clip, wait):
        def fn():
            guarded.step(max_grad_norm=clip)
            if not wait:
                guarded._pending = None             # (probe only: do not wait for this verdict on the host at the next step)
        return fn
    guarded.step()
    torch.cuda.synchronize()
    plan = guarded._plan
    verdict = C.cast(guarded._verdict.data_ptr(), C.POINTER(L.XpStepVerdict))
    lib, partials, n = L.lib(), plan["partials"].data_ptr(), plan["n_chunks"]
    print(f"cfg #2 parameter set: {len(named)} tensors, {numel / 1e6:.1f} M elements, {n} chunks in {len(plan['launches'])} launch tables; "
          f"AdamW; {rounds} rounds of 100 back-to-back steps after 200; microseconds per step")
    cols = ("clip on: unguarded", "clip on: guarded", "clip off: unguarded", "clip off: guarded", "verdict alone", "clip on: guarded + host wait")
    rows = []
    for r in range(rounds):
        row = [timeit(lambda: plain.step(max_grad_norm=1.0)), timeit(g_step(1.0, False)), timeit(plain.step), timeit(g_step(None, False)),
               timeit(lambda: lib.xp_step_verdict(partials, n, verdict, H._stream())), timeit(g_step(1.0, True))]
        rows.append(row)
        print(f"round {r}: " + " | ".join(f"{c} {v:7.1f}" for c, v in zip(cols, row)))
    assert guarded.skipped_steps == 0
    med = [sorted(col)[len(col) // 2] for col in zip(*rows)]
    span = [max(col) - min(col) for col in zip(*rows)]
    print("median (max - min over the rounds): " + " | ".join(f"{c} {m:7.1f} ({s:.1f})" for c, m, s in zip(cols, med, span)))
    per_round = [row[1] - row[0] for row in rows]
    print(f"clip on: guarded - unguarded {med[1] - med[0]:+.1f} us ({(med[1] / med[0] - 1) * 100:+.2f} %), per round "
          f"{', '.join(f'{d:+.1f}' for d in per_round)}; the unguarded step's own rounds span {span[0]:.1f} us ({span[0] / med[0] * 100:.2f} %)")
    print(f"clip off: guarded / unguarded = {med[3] / med[2]:.3f} ({med[3] - med[2]:+.1f} us: the norm pass, one more read of the gradients, and "
          f"the verdict); the unguarded step's own rounds span {span[2]:.1f} us ({span[2] / med[2] * 100:.2f} %)")
    print(f"xp_step_verdict alone, back to back: {med[4]:.1f} us per launch")
    print(f"guarded steps with nothing between them (each waits for the verdict before it): {med[5]:.1f} us per step, {med[5] - med[1]:+.1f} us")


if __name__ == "__main__":
    main(max(5, int(sys.argv[1]) if len(sys.argv) > 1 else 5))
