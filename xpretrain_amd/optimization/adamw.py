"""AdamW with the reference's semantics, executed as ONE multi-tensor HIP launch (plus one for the gradient norm).

Mirrors ``src/optimization/adamw.py:11-103`` (``AdamW(params, lr, betas, eps=1e-6, weight_decay, correct_bias)``,
``.step(closure)``; state keys ``step`` / ``exp_avg`` / ``exp_avg_sq`` as ``E2E_TrainingRestorer`` checkpoints them,
``utils/load_save.py:306-314``).  On top of the reference surface, the fused clip (``step(max_grad_norm=...)`` / ``clip_and_step``), the rewritten compute-dtype weight copies,
``overlap_next_forward`` and the opt-in step guard (``skip_nonfinite=True``: a step with a non-finite gradient norm changes nothing) come
from ``multi_tensor.MultiTensorOptimizer``, which ``Adam`` and ``Adamax`` (``adam.py``) share.

There is no eager fallback: without the HIP library the step raises.
"""
import math

from .. import _lib as L
from .multi_tensor import MultiTensorOptimizer


class AdamW(MultiTensorOptimizer):
    _STATE = ("exp_avg", "exp_avg_sq")
    _ENTRY = ("xp_adamw_step", "xp_adamw_step_guarded")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, correct_bias=True, skip_nonfinite=False):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {} - should be >= 0.0".format(lr))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter: {} - should be in [0.0, 1.0[".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter: {} - should be in [0.0, 1.0[".format(betas[1]))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {} - should be >= 0.0".format(eps))
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, correct_bias=correct_bias),
                         skip_nonfinite=skip_nonfinite)

    def _group_struct(self, group, step):
        b1, b2 = group["betas"]
        step_size = group["lr"]
        if group["correct_bias"]:
            step_size = step_size * math.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step)
        return L.XpAdamGroup(group["lr"], b1, b2, group["eps"], group["weight_decay"], step_size)
