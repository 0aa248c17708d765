"""CPU: optim "adam" / "adamax" -- the restatement (tests/optim_family_ref.py) against the unmodified reference's run
(tests/golden/optim_adam_adamax.pt), the dispatch of setup_e2e_optimizer, the grouping, the constructors and the C ABI's text."""
import os
import re
import types

import pytest
import torch

from tests import optim_family_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = R.FIXTURE


def named_module(fx):
    """a module whose named_parameters() are the fixture's names and initial values, in the fixture's order"""
    root = torch.nn.Module()
    for name, p0 in zip(fx["names"], fx["init"]):
        mod, parts = root, name.split(".")
        for part in parts[:-1]:
            if not hasattr(mod, part):
                mod.add_module(part, torch.nn.Module())
            mod = getattr(mod, part)
        mod.register_parameter(parts[-1], torch.nn.Parameter(p0.clone()))
    assert [n for n, _ in root.named_parameters()] == fx["names"]
    return root


def fixture_opts(fx, optim):
    return types.SimpleNamespace(learning_rate=fx["learning_rate"], weight_decay=fx["weight_decay"], lr_mul=fx["lr_mul"],
                                 lr_mul_prefix=fx["lr_mul_prefix"], betas=fx["betas"], optim=optim)


@pytest.mark.parametrize("kind", R.KINDS)
def test_restatement_reproduces_the_reference_run_in_fp64(golden, kind):
    """The reference ran torch's fp32 optimizer; the fp64 restatement on the same inputs differs from it by fp32 rounding alone:
    a few 2^-24 relative per step on the parameters and exp_avg.  exp_avg_sq squares a gradient that the fp32 clip coefficient
    (relative error <= 2^-23 after the norm's sum and square root) scaled, so it gets twice that."""
    fx = golden(FIXTURE)
    k = fx["kinds"][kind]
    ps, ms, ss, norms = R.train_steps(kind, fx["init"], fx["grads"], R.fixture_groups(fx, kind), max_norm=fx["max_norm"])
    assert k["step"] == [len(fx["grads"])] * len(fx["names"])
    for n, ref in zip(norms, k["norms"]):
        assert abs(float(n) - float(ref)) <= 1e-6 * float(ref)
    assert any(float(n) > fx["max_norm"] for n in norms) and any(float(n) < fx["max_norm"] for n in norms)
    for got, ref, floor, tol in ((ps, k["final"], 1e-3, 2e-6), (ms, k["state_a"], 1e-6, 2e-6), (ss, k["state_b"], 1e-9, 4e-6)):
        for name, a, b in zip(fx["names"], got, ref):
            d = ((a - b.double()).abs().max() / max(b.abs().max().item(), floor)).item()
            assert d <= tol, (kind, name, d)
    for b in k["state_b"]:
        assert torch.isfinite(b).all()
    assert any((g.view(-1)[::7] == 0).all() and g.numel() > 7 for g in fx["grads"][0])       # the zero gradients are in there


def test_fixture_records_its_torch_version(golden):
    assert re.match(r"\d+\.\d+", golden(FIXTURE)["torch_version"])


@pytest.mark.parametrize("optim", ("adam", "adamax", "adamw"))
def test_setup_e2e_optimizer_dispatches_and_groups(golden, optim):
    from xpretrain_amd import optimization as XO
    fx = golden(FIXTURE)
    model = named_module(fx)
    opt = XO.setup_e2e_optimizer(model, fixture_opts(fx, optim))
    assert type(opt) is {"adam": XO.Adam, "adamax": XO.Adamax, "adamw": XO.AdamW}[optim]
    params = list(model.parameters())
    idx = [[[id(p) for p in params].index(id(q)) for q in g["params"]] for g in opt.param_groups]
    for kind in R.KINDS:
        assert idx == fx["kinds"][kind]["group_idx"] and all(idx)
    lr, wd = fx["learning_rate"], fx["weight_decay"]
    assert [g["lr"] for g in opt.param_groups] == [fx["lr_mul"] * lr, fx["lr_mul"] * lr, lr, lr]
    assert [g["weight_decay"] for g in opt.param_groups] == [wd, 0.0, wd, 0.0]
    assert all(tuple(g["betas"]) == tuple(fx["betas"]) for g in opt.param_groups)


@pytest.mark.parametrize("optim", ("sgd", "Adam", "", None))
def test_unknown_optimizer_names_are_refused(golden, optim):
    from xpretrain_amd.optimization import setup_e2e_optimizer
    fx = golden(FIXTURE)
    with pytest.raises(ValueError, match="invalid optimizer"):
        setup_e2e_optimizer(named_module(fx), fixture_opts(fx, optim))


@pytest.mark.parametrize("optim", ("adam", "adamax", "adamw"))
def test_setup_training_builds_each_optimizer_from_a_config(tmp_path, optim):
    """configs.setup_training (run_pretrain.py:222) on the shipped pre-training config with ``optim`` set, tiny towers"""
    import json
    from xpretrain_amd import configs as CF, optimization as XO, workload
    d = tmp_path / "clip-vit-tiny"
    d.mkdir()
    json.dump(workload.hf_config_dict(128, 2, 2, 256, 16, 32, 128, 2, 2, 256, 120, 16, 64), open(d / "config.json", "w"))
    base = json.load(open(os.path.join(ROOT, "tests", "golden", "pretrain_vip_base_16.json")))
    cfg = CF.load_config(dict(base, clip_config=str(d), clip_weights="", fp16=0, optim=optim,
                              clip_vision_additional_config=dict(base["clip_vision_additional_config"], temporal_size=3)))
    tr = CF.setup_training(cfg, CF.setup_model(cfg), 100)
    assert type(tr.optimizer) is {"adam": XO.Adam, "adamax": XO.Adamax, "adamw": XO.AdamW}[optim]
    assert len(tr.optimizer.param_groups) == 4 and tuple(tr.optimizer.param_groups[2]["betas"]) == tuple(cfg.betas)


@pytest.mark.parametrize("kind", R.KINDS)
def test_defaults_and_state_names(kind):
    from xpretrain_amd import optimization as XO
    cls = {"adam": XO.Adam, "adamax": XO.Adamax}[kind]
    opt = cls([torch.nn.Parameter(torch.zeros(3))])
    for key, val in R.DEFAULTS[kind].items():
        assert opt.defaults[key] == val and opt.param_groups[0][key] == val
    assert cls._STATE == R.STATE[kind]
    assert opt.last_grad_norm is None


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("bad", (dict(lr=-1.0), dict(eps=-1e-8), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)), dict(weight_decay=-0.1)))
def test_torchs_argument_checks(kind, bad):
    from xpretrain_amd import optimization as XO
    ours, theirs = {"adam": (XO.Adam, torch.optim.Adam), "adamax": (XO.Adamax, torch.optim.Adamax)}[kind]
    with pytest.raises(ValueError) as want:
        theirs([torch.nn.Parameter(torch.zeros(3))], **bad)
    with pytest.raises(ValueError) as got:
        ours([torch.nn.Parameter(torch.zeros(3))], **bad)
    assert str(got.value) == str(want.value)


def test_amsgrad_is_refused():
    from xpretrain_amd.optimization import Adam
    with pytest.raises(NotImplementedError):
        Adam([torch.nn.Parameter(torch.zeros(3))], amsgrad=True)
    assert Adam([torch.nn.Parameter(torch.zeros(3))], amsgrad=False).defaults["amsgrad"] is False


@pytest.mark.parametrize("kind", R.KINDS)
def test_step_without_gradients_returns_none(kind):
    from xpretrain_amd import optimization as XO
    p = torch.nn.Parameter(torch.ones(3))
    opt = {"adam": XO.Adam, "adamax": XO.Adamax}[kind]([p])
    assert opt.step() is None and opt.clip_and_step(1.0) is None
    assert len(opt.state) == 0 and torch.equal(p.detach(), torch.ones(3))
    assert opt.step(closure=lambda: 7.0) == 7.0


@pytest.mark.parametrize("kind", R.KINDS)
def test_load_state_dict_takes_torchs_tensor_step(kind):
    """torch.optim keeps ``step`` as a scalar tensor; loaded here it is a Python int, and the state tensors keep torch's names"""
    from xpretrain_amd import optimization as XO
    ours, theirs = {"adam": (XO.Adam, torch.optim.Adam), "adamax": (XO.Adamax, torch.optim.Adamax)}[kind]
    p = torch.nn.Parameter(torch.ones(5))
    t = theirs([p], lr=1e-2)
    for _ in range(3):
        p.grad = torch.full((5,), 0.5)
        t.step()
    sd = t.state_dict()
    assert torch.is_tensor(sd["state"][0]["step"])
    q = torch.nn.Parameter(p.detach().clone())
    o = ours([q], lr=1e-2)
    o.load_state_dict(sd)
    st = o.state[q]
    assert st["step"] == 3 and type(st["step"]) is int
    assert set(st) == {"step"} | set(R.STATE[kind])
    for name in R.STATE[kind]:
        assert torch.equal(st[name], t.state[p][name])


def test_header_declares_the_entry_and_keeps_the_abi_version():
    src = open(os.path.join(ROOT, "include", "xpretrain_hip.h")).read()
    assert re.search(r"^#define XP_ABI_VERSION 1$", src, flags=re.M)
    assert re.search(r"\bint xp_optim_step\(int32_t kind,", src)
    assert re.search(r"enum XpOptKind \{ XP_OPT_ADAM, XP_OPT_ADAMAX \};", src)
    assert re.search(r"\bint xp_adamw_step\(", src)
    from xpretrain_amd import _lib
    assert "xp_optim_step" in _lib.SIGNATURES and (_lib.XP_OPT_ADAM, _lib.XP_OPT_ADAMAX) == (0, 1)
    import ctypes
    assert ctypes.sizeof(_lib.XpOptGroup) == 32 and ctypes.sizeof(_lib.XpAdamGroup) == 24
