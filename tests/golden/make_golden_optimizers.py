#!/usr/bin/env python
"""Generate tests/golden/optim_adam_adamax.pt from the UNMODIFIED reference: ``setup_e2e_optimizer(model, opts)`` of
src/optimization/utils.py:96-121 with ``opts.optim`` = "adam" and "adamax" (torch.optim.Adam / torch.optim.Adamax of the torch this
runs under; the version is stored), stepped as the training loops step it (tasks/run_video_retrieval.py:377-392).

Run in the build container (where the reference tree exists), beside make_golden.py:

    python tests/golden/make_golden_optimizers.py

A small module whose parameter names populate all four groups of build_e2e_optimizer_w_lr_mul (names containing ``bias``,
``LayerNorm.weight``, ``logit_scale``, and the lr_mul_prefix ``text_model``); 6 steps with the warm-up cosine schedule, the lr_mul of
the first two groups, ``clip_grad_norm_(params, 5.0)`` (active on the even steps only) and a weight decay of 0.2.  Every 7th
gradient element is exactly 0.  Both kinds see the same initial parameters, gradients and learning rates.
Stored: names, initial parameters, per-step gradients / learning rates / norms, and per kind the final parameters, both state tensors,
``state["step"]`` and the group indices.  Tensors and plain numbers, nothing else (tests/gpu_util.py::save_golden).
Read by tests/test_optim_family_cpu.py and tests/test_optim_family_gpu.py.
"""
import importlib
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402
from tests.gpu_util import save_golden  # noqa: E402

STATE = {"adam": ("exp_avg", "exp_avg_sq"), "adamax": ("exp_avg", "exp_inf")}


class _Tower(torch.nn.Module):
    def __init__(self, d_in, d):
        super().__init__()
        self.fc = torch.nn.Linear(d_in, d)
        self.LayerNorm = torch.nn.LayerNorm(d)


class _Clip(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.vision_model = _Tower(33, 24)
        self.text_model = _Tower(16, 20)
        self.logit_scale = torch.nn.Parameter(torch.tensor(4.6))


class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.clipmodel = _Clip()


def optimizers(ref):
    utils = importlib.import_module("src.optimization.utils")
    sched = importlib.import_module("src.optimization.sched")
    lr0, wd, lr_mul, prefix, betas, steps, total, max_norm = 1e-3, 0.2, 0.1, "text_model", (0.9, 0.98), 6, 20, 5.0
    torch.manual_seed(78)
    model = _Model()
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "logit_scale" not in n:
                p.copy_(torch.randn(p.shape) * 0.05 + (1.0 if n.endswith("LayerNorm.weight") else 0.0))
    names = [n for n, _ in model.named_parameters()]
    init = [p.detach().clone() for p in model.parameters()]
    grads = []
    for t in range(steps):
        gs = [torch.randn(p.shape) * (4.0 if t % 2 == 0 else 0.03) for p in init]
        for g in gs:
            g.view(-1)[::7] = 0.0
        grads.append(gs)
    lrs = [sched.get_lr_sched(t, "cosine", lr0, total, warmup_ratio=0.2) for t in range(steps)]
    out = dict(torch_version=torch.__version__, names=names, init=init, grads=grads, lrs=lrs, lr_mul=lr_mul, lr_mul_prefix=prefix,
               weight_decay=wd, betas=betas, learning_rate=lr0, max_norm=max_norm, kinds={})
    for kind in ("adam", "adamax"):
        with torch.no_grad():
            for p, p0 in zip(model.parameters(), init):
                p.copy_(p0)
        opts = ref.AttrDict(learning_rate=lr0, weight_decay=wd, lr_mul=lr_mul, lr_mul_prefix=prefix, optim=kind, betas=betas)
        opt = utils.setup_e2e_optimizer(model, opts)
        assert type(opt) is {"adam": torch.optim.Adam, "adamax": torch.optim.Adamax}[kind]
        params = list(model.parameters())
        group_idx = [[[id(p) for p in params].index(id(q)) for q in g["params"]] for g in opt.param_groups]
        assert all(group_idx), group_idx
        norms = []
        for t in range(steps):
            for gi, g in enumerate(opt.param_groups):                 # run_video_retrieval.py:377-383
                g["lr"] = lr_mul * lrs[t] if gi in (0, 1) else lrs[t]
            for p, g in zip(params, grads[t]):
                p.grad = g.clone()
            norms.append(torch.nn.utils.clip_grad_norm_(params, max_norm).clone())
            opt.step()
        sa, sb = STATE[kind]
        out["kinds"][kind] = dict(group_idx=group_idx, norms=norms, final=[p.detach().clone() for p in params],
                                  state_a=[opt.state[p][sa].clone() for p in params],
                                  state_b=[opt.state[p][sb].clone() for p in params],
                                  step=[int(opt.state[p]["step"]) for p in params],
                                  eps=opt.defaults["eps"])
        print(kind, "norms", [round(float(n), 3) for n in norms], "groups", group_idx)
    files = save_golden(out, "optim_adam_adamax.pt")
    print("optim_adam_adamax:", [os.path.basename(f) for f in files], sum(os.path.getsize(f) for f in files), "bytes")


if __name__ == "__main__":
    optimizers(ref_import.load())
