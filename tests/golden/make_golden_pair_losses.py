#!/usr/bin/env python
"""Generate tests/golden/pair_losses.pt from the UNMODIFIED reference: the four two-argument, fixed-temperature losses of
src/optimization/loss.py -- TripletContrastiveLoss, NCEContrastiveLoss, HardNegLoss, MILNCEContrastiveLoss.

Run in the build container (where the reference tree exists), beside make_golden_losses.py:

    python tests/golden/make_golden_pair_losses.py

Each case: the kind as its XpPairLossKind number, seeded unit-norm fp32 features vis [n, d] and txt [n * bag, d] (tests/pair_loss_ref.py::unit_feats, rounded to fp32),
the parameters, and the reference's fp32 loss and torch.autograd.grad with respect to both feature matrices.  Shapes: n = 1 (no
negatives at all), 2, 5 (odd), 16, 64 (a full wave), 70 (past the 64-lane stride).  Configurations: pair_loss_ref.configs(n).
Three of the losses select, so every shape takes the first seed at or above 1000 + n + d whose draw keeps
pair_loss_ref.MIN_MARGIN from every switch of every configuration (pair_loss_ref.decision_margin); the seed is stored.
Tensors and plain numbers, nothing else (tests/gpu_util.py::save_golden).
Read by tests/test_pair_loss_cpu.py and tests/test_pair_loss_gpu.py.

Also prints the reference's own fp32 rounding on these inputs: its classes run in fp64 against the stored fp32 outputs.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402
from tests import pair_loss_ref as R  # noqa: E402
from tests.gpu_util import maxrel, save_golden  # noqa: E402

SHAPES = [(1, 32), (2, 64), (5, 32), (16, 128), (64, 32), (70, 32)]


def reference_module(ref, kind, p):
    cfg = ref.AttrDict(margin=p["margin"], measure="order" if p["order_measure"] else "cosine",
                       max_violation=bool(p["max_violation"]), temp=p["temp"], hard_negative_num=p["hard_negative_num"])
    return getattr(ref.loss, R.KINDS[kind])(cfg)


def pair_losses(ref):
    cases = []
    worst = {"loss": 0.0, "grad": 0.0}
    for n, d in SHAPES:
        seed = 1000 + n + d
        while R.joint_margin(n, d, seed) < R.MIN_MARGIN:
            seed += 1
        print(f"n={n} d={d}: seed {seed} (base {1000 + n + d}), joint margin {R.joint_margin(n, d, seed):.3e}")
        drawn = {}                                       # one tensor object per draw: torch.save stores shared storage once
        for kind, params in R.configs(n):
            p = dict(R.DEFAULTS, **params)
            if p["bag"] not in drawn:
                drawn[p["bag"]] = [f.float() for f in R.unit_feats(n, d, seed, bag=p["bag"])]
            feats = drawn[p["bag"]]
            assert R.decision_margin(kind, p, feats) >= R.MIN_MARGIN
            fn = reference_module(ref, kind, p)
            out = {}
            for dtype in (torch.float32, torch.float64):
                fs = [f.to(dtype).requires_grad_() for f in feats]
                loss = fn(*fs)
                out[dtype] = (loss.detach(), [g.clone() for g in torch.autograd.grad(loss, fs)])
            loss, grads = out[torch.float32]
            assert torch.isfinite(loss) and all(torch.isfinite(g).all() for g in grads), (kind, n, p)
            l64, g64 = out[torch.float64]
            worst["loss"] = max(worst["loss"], abs(loss.item() - l64.item()) / max(1.0, abs(l64.item())))
            floor = R.grad_scale_floor(R.grad_scale(kind, p))
            worst["grad"] = max([worst["grad"]] + [maxrel(a, b, floor) for a, b in zip(grads, g64)])
            cases.append(dict(kind=R.KIND_IDS[kind], n=n, d=d, seed=seed, params=p, feats=feats, loss=loss, grads=grads))
    files = save_golden(cases, "pair_losses.pt")
    print("pair_losses:", len(cases), "cases ->", [os.path.basename(f) for f in files],
          sum(os.path.getsize(f) for f in files), "bytes")
    print("reference fp32 against reference fp64 on these inputs:", worst)


if __name__ == "__main__":
    pair_losses(ref_import.load())
