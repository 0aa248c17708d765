#!/usr/bin/env python
"""Generate tests/golden/loss_family.pt from the UNMODIFIED reference: the six learnable-temperature losses of
src/optimization/loss.py that loss.pt (make_golden.py) does not cover -- NCELearnableTempDSLLoss, NCELearnableTempLoss_vs_vc,
NCELearnableTempLoss_vs_vc_fc, NCELearnableTempLoss_vsc, VidImgNCELearnableTempLoss, VidImgDivideNCELearnableTempLoss.

Run in the build container (where the reference tree exists), beside make_golden.py:

    python tests/golden/make_golden_losses.py

Each case: seeded unit-norm features vis/txt [n, d] and img/cap [m, d], one log_scale of {0, 4.6, ln 200}, and per class the
reference's fp32 loss and torch.autograd.grad with respect to the features that class reads and the temperature.  Shapes:
n = 1 (no negatives at all), 2, 5 (odd), 16, 64 (a full wave), 70 (past the 64-lane stride); m != n for the two VidImg* classes
only, the others take square logits.  Tensors and plain numbers, nothing else (tests/gpu_util.py::save_golden).
Read by tests/test_loss_family_cpu.py and tests/test_loss_family_gpu.py.
"""
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402
from tests.gpu_util import save_golden  # noqa: E402

# class name -> (reads img, reads cap, accepts m != n)
CLASSES = {
    "NCELearnableTempDSLLoss": (False, False, False),
    "NCELearnableTempLoss_vs_vc": (False, True, False),
    "NCELearnableTempLoss_vs_vc_fc": (True, True, False),
    "NCELearnableTempLoss_vsc": (False, True, False),
    "VidImgNCELearnableTempLoss": (True, True, True),
    "VidImgDivideNCELearnableTempLoss": (True, True, True),
}
SHAPES = [(1, 1, 32), (2, 2, 64), (5, 5, 32), (16, 16, 128), (64, 64, 32), (70, 70, 32), (5, 10, 32), (3, 1, 64)]


def loss_family(ref):
    torch.manual_seed(23)
    cases = []
    for n, m, d in SHAPES:
        for ls in (0.0, 4.6, math.log(200.0)):
            feats = [torch.nn.functional.normalize(torch.randn(r, d), dim=-1).requires_grad_() for r in (n, n, m, m)]
            t = torch.tensor(ls, requires_grad=True)
            case = dict(n=n, m=m, d=d, log_scale=ls, feats=[f.detach() for f in feats], losses={}, grads={})
            for name, (use_img, use_cap, rect) in CLASSES.items():
                if m != n and not rect:
                    continue
                fn = getattr(ref.loss, name)(None)
                out = fn(feats[0], feats[1], t) if name == "NCELearnableTempDSLLoss" else fn(*feats, t)
                used = [0, 1] + ([2] if use_img else []) + ([3] if use_cap else [])
                g = torch.autograd.grad(out, [feats[i] for i in used] + [t])
                case["losses"][name] = out.detach()
                # [d vis, d txt, d img | None, d cap | None, d log_scale]
                case["grads"][name] = [g[used.index(i)].clone() if i in used else None for i in range(4)] + [g[-1].clone()]
            cases.append(case)
    files = save_golden(cases, "loss_family.pt")
    print("loss_family:", len(cases), "cases ->", [os.path.basename(f) for f in files],
          sum(os.path.getsize(f) for f in files), "bytes")


if __name__ == "__main__":
    loss_family(ref_import.load())
