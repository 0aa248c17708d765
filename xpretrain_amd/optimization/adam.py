"""``Adam`` and ``Adamax`` with ``torch.optim``'s semantics, each executed as ONE multi-tensor HIP launch.

The reference's ``setup_e2e_optimizer`` (``src/optimization/utils.py:111-120``) builds ``torch.optim.Adam`` / ``torch.optim.Adamax``
for ``optim == "adam"`` / ``"adamax"`` with the four parameter groups, ``lr`` and ``betas``.  These classes take the same
arguments, run torch's own argument checks, and keep torch's state keys (``step``, ``exp_avg``, ``exp_avg_sq`` resp. ``step``,
``exp_avg``, ``exp_inf``), so ``E2E_TrainingRestorer`` checkpoints (``utils/load_save.py:306-314``) go either way; ``step`` is a
Python int here.  The arithmetic is torch's single-tensor path with ``amsgrad = maximize = False`` (include/xpretrain_hip.h,
``xp_optim_step``): coupled L2 weight decay on the clipped gradient, bias corrections where torch applies them.

The fused clip, the rewritten compute-dtype weight copies, ``overlap_next_forward`` and the opt-in step guard (``skip_nonfinite=True``,
``xp_optim_step_guarded``) come from ``multi_tensor.MultiTensorOptimizer``, as for ``AdamW``.  There is no eager fallback: without the HIP library the step raises.
"""
import math

import torch

from .. import _lib as L
from .multi_tensor import MultiTensorOptimizer


def _checked(cls, **kw):
    """torch's own argument checks, with its messages: ``cls`` is built once on a throwaway parameter"""
    cls([torch.nn.Parameter(torch.empty(0))], **kw)
    return kw


class _TorchFamily(MultiTensorOptimizer):
    _ENTRY = ("xp_optim_step", "xp_optim_step_guarded")      # (_KIND: XP_OPT_ADAM or XP_OPT_ADAMAX, by the subclass)

    def _group_struct(self, group, step):
        if group.get("amsgrad") or group.get("maximize"):       # (a loaded torch checkpoint brings its param groups along)
            raise NotImplementedError(f"xpretrain_amd {type(self).__name__}: amsgrad / maximize are not implemented")
        b1, b2 = group["betas"]
        lr = float(group["lr"])
        return L.XpOptGroup(lr, b1, b2, group["eps"], group["weight_decay"], lr / (1.0 - b1 ** step),
                            math.sqrt(1.0 - b2 ** step), 1.0 - b1)


class Adam(_TorchFamily):
    _STATE = ("exp_avg", "exp_avg_sq")
    _KIND = L.XP_OPT_ADAM

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, skip_nonfinite=False):
        if amsgrad:
            raise NotImplementedError("xpretrain_amd Adam: amsgrad=True is not implemented")
        super().__init__(params, _checked(torch.optim.Adam, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False),
                         skip_nonfinite=skip_nonfinite)


class Adamax(_TorchFamily):
    _STATE = ("exp_avg", "exp_inf")
    _KIND = L.XP_OPT_ADAMAX

    def __init__(self, params, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, skip_nonfinite=False):
        super().__init__(params, _checked(torch.optim.Adamax, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay),
                         skip_nonfinite=skip_nonfinite)
