"""``torch.optim.Adam`` / ``torch.optim.Adamax`` (single-tensor path, amsgrad = maximize = False) restated on plain tensors, in any
dtype (a helper, not a test).

Written from the formulas in include/xpretrain_hip.h (xp_optim_step); tests/test_optim_family_cpu.py pins them to the unmodified
reference's ``setup_e2e_optimizer(optim="adam" | "adamax")`` run (tests/golden/optim_adam_adamax.pt).  The clip is
``oracle.optim_oracle.clip_coef``: the coefficient multiplies the gradient BEFORE the coupled weight decay is added to it.
"""
import torch

from oracle.optim_oracle import clip_coef

KINDS = ("adam", "adamax")                       # XpOptKind's order
STATE = {"adam": ("exp_avg", "exp_avg_sq"), "adamax": ("exp_avg", "exp_inf")}
FIXTURE = "optim_adam_adamax.pt"                # tests/golden/make_golden_optimizers.py
DEFAULTS = {"adam": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0),
            "adamax": dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0)}


def adam_step(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """One Adam step on one tensor; ``g`` is the clipped gradient, ``step`` the count AFTER the increment.  Returns (p, m, v)."""
    b1, b2 = betas
    if weight_decay != 0:
        g = g + weight_decay * p
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    p = p - (lr / (1.0 - b1 ** step)) * m / (v.sqrt() / (1.0 - b2 ** step) ** 0.5 + eps)
    return p, m, v


def adamax_step(p, g, m, u, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """One Adamax step on one tensor; as adam_step.  Returns (p, m, u) with u = exp_inf."""
    b1, b2 = betas
    if weight_decay != 0:
        g = g + weight_decay * p
    m = b1 * m + (1.0 - b1) * g
    u = torch.maximum(b2 * u, g.abs() + eps)
    p = p - (lr / (1.0 - b1 ** step)) * m / u
    return p, m, u


def fixture_groups(fx, kind):
    """the fixture's four groups as optim_family_ref.train_steps takes them"""
    k = fx["kinds"][kind]
    return [dict(idx=idx, lr=[(fx["lr_mul"] if gi < 2 else 1.0) * lr for lr in fx["lrs"]], betas=tuple(fx["betas"]), eps=k["eps"],
                 weight_decay=fx["weight_decay"] if gi % 2 == 0 else 0.0) for gi, idx in enumerate(k["group_idx"])]


STEP = {"adam": adam_step, "adamax": adamax_step}


def train_steps(kind, params, grads_per_step, groups, max_norm=None, dtype=torch.float64):
    """Run len(grads_per_step) steps of ``kind``.  ``groups``: dicts(idx=[param indices], lr=float or one per step, and optionally
    betas, eps, weight_decay).  Returns (params, first state tensors, second state tensors, gradient norms)."""
    ps = [p.to(dtype) for p in params]
    ms = [torch.zeros_like(p) for p in ps]
    ss = [torch.zeros_like(p) for p in ps]
    norms = []
    for t, grads in enumerate(grads_per_step, start=1):
        gs = [g.to(dtype) for g in grads]
        if max_norm is not None:
            n, c = clip_coef(gs, max_norm)
            norms.append(n)
            gs = [g * c.to(dtype) for g in gs]
        for grp in groups:
            lr = grp["lr"][t - 1] if isinstance(grp["lr"], (list, tuple)) else grp["lr"]
            kw = {k: grp[k] for k in ("betas", "eps", "weight_decay") if k in grp}
            for i in grp["idx"]:
                ps[i], ms[i], ss[i] = STEP[kind](ps[i], gs[i], ms[i], ss[i], t, lr, **kw)
    return ps, ms, ss, norms
