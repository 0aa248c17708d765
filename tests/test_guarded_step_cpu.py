"""CPU: the definition of a guarded run (tests/guarded_step_ref.py) against live ``torch.optim.Adam`` / ``Adamax`` and the AdamW
restatement of oracle/optim_oracle.py, each driven by a loop that skips the non-finite steps by hand; the switch's default and where
``setup_e2e_optimizer`` reads it; the reconciliation bookkeeping (``multi_tensor.take_back``) as a pure function."""
import inspect
from types import SimpleNamespace

import pytest
import torch

from oracle import optim_oracle as OO
from tests import guarded_step_ref as G
from tests import optim_family_ref as R

SHAPES = [(5, 3), (7,), (), (G.CHUNK + 3,)]
BETAS, STEPS = (0.8, 0.95), 6
BAD = {1: (0, float("inf")), 2: (3, float("nan")), 4: (1, float("-inf"))}       # step -> (tensor, planted value)
LRS = [1e-2 * (1.0 - 0.1 * k) for k in range(STEPS)]                            # a schedule that goes on over skipped steps


def inputs():
    gen = torch.Generator().manual_seed(3)
    init = [torch.randn(s, generator=gen, dtype=torch.float64) * 0.1 for s in SHAPES]
    grads = [[torch.randn(s, generator=gen, dtype=torch.float64) * 0.05 for s in SHAPES] for _ in range(STEPS)]
    for k, (i, x) in BAD.items():
        grads[k][i].view(-1)[-1] = x
    return init, grads


def groups(kind):
    eps = 1e-6 if kind == "adamw" else 1e-8
    return [dict(idx=[0, 3], lr=LRS, betas=BETAS, eps=eps, weight_decay=0.1), dict(idx=[1, 2], lr=[0.5 * x for x in LRS], betas=BETAS, eps=eps)]


def test_the_rule_sees_what_the_kernels_see():
    init, grads = inputs()
    assert [G.norm_is_finite(gs) for gs in grads] == [k not in BAD for k in range(STEPS)]
    assert [G.first_bad(gs) for gs in grads] == [BAD[k][0] if k in BAD else None for k in range(STEPS)]
    # finite elements whose squares overflow fp32; and finite partials whose sum overflows (no chunk of its own to blame)
    assert not G.norm_is_finite([torch.tensor([1e30])]) and G.first_bad([torch.tensor([1e30])]) == 0
    two = [torch.tensor([1.5e19]), torch.tensor([1.5e19])]
    assert not G.norm_is_finite(two) and G.first_bad(two) is None
    assert G.norm_is_finite([torch.tensor([1.5e19])])


@pytest.mark.parametrize("clip", [None, 0.05])
@pytest.mark.parametrize("kind", R.KINDS)
def test_definition_against_live_torch_skipping_by_hand(kind, clip):
    init, grads = inputs()
    ps, ms, ss, steps, skipped = G.train_steps(kind, init, grads, groups(kind), max_norm=clip)
    assert skipped == [k in BAD for k in range(STEPS)] and steps == [STEPS - len(BAD)] * len(SHAPES)
    params = [torch.nn.Parameter(p.clone()) for p in init]
    cls = {"adam": torch.optim.Adam, "adamax": torch.optim.Adamax}[kind]
    opt = cls([dict(params=[params[i] for i in g["idx"]], weight_decay=g.get("weight_decay", 0)) for g in groups(kind)],
              betas=BETAS, eps=1e-8, foreach=False)
    for k, gs in enumerate(grads):
        for g, grp in zip(opt.param_groups, groups(kind)):
            g["lr"] = grp["lr"][k]                                       # the schedule goes on
        for p, g in zip(params, gs):
            p.grad = g.clone()
        if not all(torch.isfinite(g).all() for g in gs):                 # apex: a skipped optimizer.step() is a no-op
            continue
        if clip:
            torch.nn.utils.clip_grad_norm_(params, clip, foreach=False)
        opt.step()
    for i, p in enumerate(params):
        torch.testing.assert_close(ps[i], p.detach(), rtol=1e-12, atol=1e-15)
        torch.testing.assert_close(ms[i], opt.state[p][R.STATE[kind][0]], rtol=1e-12, atol=1e-15)
        torch.testing.assert_close(ss[i], opt.state[p][R.STATE[kind][1]], rtol=1e-12, atol=1e-15)
        assert int(opt.state[p]["step"]) == steps[i]


@pytest.mark.parametrize("clip", [None, 0.05])
def test_definition_against_the_adamw_restatement_skipping_by_hand(clip):
    init, grads = inputs()
    ps, _, _, steps, skipped = G.train_steps("adamw", init, grads, groups("adamw"), max_norm=clip)
    kept = [k for k in range(STEPS) if k not in BAD]
    ref, _ = OO.train_steps(init, [grads[k] for k in kept], [dict(g, lr=[g["lr"][k] for k in kept]) for g in groups("adamw")], max_norm=clip)
    assert steps == [len(kept)] * len(SHAPES)
    for a, b in zip(ps, ref):
        assert torch.equal(a, b)                                          # the same arithmetic on the same steps
    assert all(torch.isfinite(p).all() for p in ps)


def test_the_guard_is_off_unless_asked_for():
    from xpretrain_amd import optimization as XO
    from xpretrain_amd.optimization.multi_tensor import MultiTensorOptimizer
    for cls in (MultiTensorOptimizer, XO.AdamW, XO.Adam, XO.Adamax):
        assert inspect.signature(cls.__init__).parameters["skip_nonfinite"].default is False
    for cls in (XO.AdamW, XO.Adam, XO.Adamax):
        p = torch.nn.Parameter(torch.zeros(3))
        assert cls([p]).skip_nonfinite is False and cls([p], skip_nonfinite=True).skip_nonfinite is True
        opt = cls([p], skip_nonfinite=True)
        assert (opt.skipped_steps, opt.last_step_skipped, opt.last_nonfinite_param, opt.last_nonfinite_name) == (0, False, None, None)
        assert set(opt.state_dict()) == {"state", "param_groups"}
        assert "skip_nonfinite" not in opt.state_dict()["param_groups"][0]          # the keys stay torch's


@pytest.mark.parametrize("optim", ["adamw", "adam", "adamax"])
def test_setup_e2e_optimizer_reads_the_key(optim):
    from xpretrain_amd.optimization import setup_e2e_optimizer
    model = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.LayerNorm(3))
    opts = dict(learning_rate=1e-4, weight_decay=0.05, lr_mul=1, lr_mul_prefix="", betas=[0.9, 0.98], optim=optim)
    assert setup_e2e_optimizer(model, SimpleNamespace(**opts)).skip_nonfinite is False
    assert setup_e2e_optimizer(model, SimpleNamespace(**opts, skip_nonfinite_steps=0)).skip_nonfinite is False
    opt = setup_e2e_optimizer(model, SimpleNamespace(**opts, skip_nonfinite_steps=1))
    assert opt.skip_nonfinite is True
    assert opt.param_names == {id(p): n for n, p in model.named_parameters()}


def test_take_back_is_exact_bookkeeping():
    from xpretrain_amd.optimization.multi_tensor import take_back
    a, b, c = object(), object(), object()
    chunk_params = [a, a, b, c]
    stepped, other = [dict(step=3), dict(step=1)], dict(step=7)
    assert take_back(stepped, True, -1, chunk_params) is None and [s["step"] for s in stepped] == [3, 1]      # applied: nothing moves
    assert take_back(stepped, False, 2, chunk_params) is b
    assert [s["step"] for s in stepped] == [2, 0] and other["step"] == 7                                       # exactly the stepped ones
    assert take_back(stepped, False, 1, chunk_params) is a and take_back([], False, -1, chunk_params) is None  # only the sum overflowed
    assert [s["step"] for s in stepped] == [1, -1]


def test_a_guarded_step_under_stream_capture_raises(monkeypatch):
    """a replayed graph cannot take a step count back: refused before anything is enqueued; the unguarded step is not asked"""
    from xpretrain_amd.optimization import AdamW
    p = torch.nn.Parameter(torch.zeros(3))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="skip_nonfinite cannot run under stream capture"):
        AdamW([p], skip_nonfinite=True).step()
    assert AdamW([p]).step() is None                                     # no gradient, nothing to do: returns before any device call
