"""The definition of a guarded optimizer run (``skip_nonfinite=True``) on plain tensors, in any dtype (a helper, not a test).

It is ``tests/optim_family_ref`` (Adam, Adamax) and ``oracle.optim_oracle.adamw_step`` (AdamW) with ONE rule added: a step whose fp32
gradient norm, as the kernels sum it, is not finite is the identity on (p, m, v, step).  The step count ``t`` of the bias corrections is
the number of APPLIED steps; a learning rate given per step is indexed by the step of the loop, skipped or not (the schedule is the
caller's and goes on).

``norm_is_finite``: the kernels sum the squares in fp32, per chunk of 64 Ki elements and then over the chunks.  Whether that sum is
finite does not depend on the order as long as no single reordering decides it: every term is >= 0 (or NaN), so the sum is not finite
iff a term is NaN / inf, a square overflows, or the running total passes FLT_MAX.  Only a total within rounding of FLT_MAX could come
out differently in another order; the tests stay a factor 1.3 away from it (2 x 2.25e38 against 3.4e38).
"""
import torch

from oracle.optim_oracle import adamw_step, clip_coef
from tests import optim_family_ref as R

KINDS = ("adamw",) + R.KINDS
STATE = dict(R.STATE, adamw=("exp_avg", "exp_avg_sq"))
CHUNK = 65536                                   # XP_OPT_CHUNK


def _adamw(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0):
    return adamw_step(p, g, m, v, step, lr, betas, eps, weight_decay, True)


STEP = dict(R.STEP, adamw=_adamw)


def norm_is_finite(grads):
    """the rule's condition: the fp32 sum of squares over chunks, then over the chunk sums, is finite"""
    partials = [(c * c).sum(dtype=torch.float32) for g in grads for c in g.detach().float().reshape(-1).split(CHUNK)]
    return bool(torch.isfinite(torch.stack(partials).sum(dtype=torch.float32)))


def first_bad(grads):
    """index of the first tensor holding a chunk whose own fp32 sum of squares is not finite, or None"""
    for i, g in enumerate(grads):
        if any(not torch.isfinite((c * c).sum(dtype=torch.float32)) for c in g.detach().float().reshape(-1).split(CHUNK)):
            return i
    return None


def train_steps(kind, params, grads_per_step, groups, max_norm=None, dtype=torch.float64):
    """optim_family_ref.train_steps with the rule.  Returns (params, first state tensors, second state tensors, applied step count of
    every parameter, one bool per step: skipped)."""
    ps = [p.to(dtype) for p in params]
    ms = [torch.zeros_like(p) for p in ps]
    ss = [torch.zeros_like(p) for p in ps]
    t, skipped = 0, []
    for k, grads in enumerate(grads_per_step):
        skipped.append(not norm_is_finite(grads))
        if skipped[-1]:
            continue                                                     # the identity on (p, m, v, step)
        t += 1
        gs = [g.to(dtype) for g in grads]
        if max_norm is not None:
            coef = clip_coef(gs, max_norm)[1].to(dtype)
            gs = [g * coef for g in gs]
        for grp in groups:
            lr = grp["lr"][k] if isinstance(grp["lr"], (list, tuple)) else grp["lr"]
            kw = {key: grp[key] for key in ("betas", "eps", "weight_decay") if key in grp}
            for i in grp["idx"]:
                ps[i], ms[i], ss[i] = STEP[kind](ps[i], gs[i], ms[i], ss[i], t, lr, **kw)
    return ps, ms, ss, [t] * len(ps), skipped
