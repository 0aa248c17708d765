"""CPU: the public surface of the four fixed-temperature losses (factory names, C-ABI binding) and the pin of
tests/pair_loss_ref.py -- the fp64 yardstick of the GPU tests -- to the reference's own outputs (tests/golden/pair_losses.pt)."""
import os
import re
import types

import pytest
import torch

from tests import loss_family_ref as F
from tests import pair_loss_ref as R
from tests.gpu_util import maxrel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(R.KINDS.values())
CFG = dict(margin=0.2, measure="cosine", max_violation=True, temp=0.05, hard_negative_num=3)


@pytest.mark.parametrize("name", NAMES)
def test_build_loss_func_returns_every_named_class(name):
    import xpretrain_amd.optimization as opt
    from xpretrain_amd.optimization import build_loss_func
    cls = getattr(opt, name)                                     # exported under the reference's name
    assert type(build_loss_func(dict(CFG, loss_name=name))) is cls
    assert type(build_loss_func(types.SimpleNamespace(loss_name=name, **CFG))) is cls


def test_constructors_read_the_reference_fields():
    from xpretrain_amd import optimization as opt
    ns = types.SimpleNamespace(**dict(CFG, measure="order"))
    assert opt.TripletContrastiveLoss(ns).params == dict(margin=0.2, order_measure=True, max_violation=True)
    assert opt.TripletContrastiveLoss(CFG).params == dict(margin=0.2, order_measure=False, max_violation=True)
    assert opt.NCEContrastiveLoss(CFG).params == dict(temp=0.05)
    assert opt.HardNegLoss(ns).params == dict(hard_negative_num=3)
    assert opt.MILNCEContrastiveLoss(CFG).params == dict(temp=0.05)
    with pytest.raises(KeyError):
        opt.HardNegLoss({"temp": 1.0})
    with pytest.raises(AttributeError):
        opt.NCEContrastiveLoss(types.SimpleNamespace(margin=0.2))


def test_build_loss_func_refuses_other_names_and_lists_the_twelve():
    from xpretrain_amd.optimization import build_loss_func
    with pytest.raises(NotImplementedError) as e:
        build_loss_func({"loss_name": "NCEHardNegLoss"})
    listed = re.findall(r"'(\w+)'", str(e.value).split("available")[1])
    assert sorted(listed) == sorted(NAMES + [v[0] for v in F.KINDS.values()]) and len(listed) == 12


def test_binding_declares_the_entry_the_kinds_and_the_struct():
    import ctypes as C
    from xpretrain_amd import _lib as L
    from xpretrain_amd import optimization as opt
    assert len(L.SIGNATURES["xp_pair_loss"][1]) == 12 and len(L.SIGNATURES["xp_pair_loss_workspace_bytes"][1]) == 4
    ids = {k: getattr(L, "XP_PAIR_" + k.upper()) for k in R.KINDS}
    assert ids == R.KIND_IDS                                      # the header's enum order
    src = open(os.path.join(ROOT, "include", "xpretrain_hip.h")).read()
    enum = re.search(r"enum XpPairLossKind \{([^}]*)\}", src).group(1)
    assert [s.strip() for s in enum.split(",")] == ["XP_PAIR_" + k.upper() for k in R.KINDS]
    for k, name in R.KINDS.items():
        assert getattr(opt, name).kind == ids[k]
    fields = L.XpPairLossParams._fields_
    assert [f[0] for f in fields] == ["temp", "margin", "max_violation", "order_measure", "hard_negative_num", "bag"]
    assert [f[1] for f in fields] == [C.c_float] * 2 + [C.c_int32] * 4 and C.sizeof(L.XpPairLossParams) == 24
    struct = re.search(r"typedef struct \{([^}]*)\} XpPairLossParams;", src).group(1)
    assert re.findall(r"\b([a-z_]+)\s*[,;]", struct) == [f[0] for f in fields]


def test_cpu_tensors_are_rejected():
    from xpretrain_amd.optimization import NCEContrastiveLoss
    with pytest.raises(RuntimeError, match="no CPU path"):
        NCEContrastiveLoss(CFG)(torch.zeros(2, 8), torch.zeros(2, 8))


def test_fixture_cases_and_margins(golden):
    """every shape and configuration the generator is to write is there, and every case keeps MIN_MARGIN from every switch"""
    cases = golden("pair_losses.pt")
    seen = {(R.KIND_NAMES[c["kind"]], c["n"], c["d"], tuple(sorted(c["params"].items()))) for c in cases}
    want = set()
    for n, d in [(1, 32), (2, 64), (5, 32), (16, 128), (64, 32), (70, 32)]:
        for kind, p in R.configs(n):
            want.add((kind, n, d, tuple(sorted(dict(R.DEFAULTS, **p).items()))))
    assert seen == want and len(cases) == len(want) == 66
    for c in cases:
        assert c["feats"][0].shape == (c["n"], c["d"]) and c["feats"][1].shape == (c["n"] * c["params"]["bag"], c["d"])
        assert all(f.dtype == torch.float32 for f in c["feats"] + c["grads"])
        assert all(torch.equal(a, b.float()) for a, b in zip(c["feats"], R.unit_feats(c["n"], c["d"], c["seed"], c["params"]["bag"])))
        m = R.decision_margin(R.KIND_NAMES[c["kind"]], c["params"], c["feats"])
        assert m >= R.MIN_MARGIN, (c["kind"], c["n"], c["params"], m)
    # the shapes of the GPU tests' fp64 comparison, for every configuration jointly
    assert R.joint_margin(130, 96, 1529) >= R.MIN_MARGIN and R.joint_margin(9, 30, 1039) >= R.MIN_MARGIN


def test_decision_margin_sees_each_switch():
    """hand-made inputs one step from a switch: the margin is that step"""
    e = torch.eye(4, dtype=torch.float64)
    vis = e[:3]
    txt = torch.stack([e[0] + 0.1 * e[1] + 0.25 * e[2], e[1] + 0.3 * e[0], e[2] + (0.3 + 1e-6) * e[0]])
    # V T^T = [[1, .3, .3 + 1e-6], [.1, 1, 0], [.25, 0, 1]]: row 0 holds the only close pair
    inf = float("inf")
    assert R.decision_margin("nce", {}, [vis, txt]) == inf and R.decision_margin("milnce", {}, [vis, txt]) == inf
    assert abs(R.decision_margin("hardneg", dict(hard_negative_num=1), [vis, txt]) - 1e-6) < 1e-12
    assert R.decision_margin("hardneg", dict(hard_negative_num=2), [vis, txt]) > 9000       # the next entry is the lowered diagonal
    assert R.decision_margin("hardneg", dict(hard_negative_num=3), [vis, txt]) == inf       # no (k+1)-th entry
    assert R.decision_margin("triplet", dict(margin=0.7), [vis, txt]) < 1e-12               # hinge: 0.7 + 0.3 - 1 = 0
    assert abs(R.decision_margin("triplet", dict(margin=0.8), [vis, txt]) - 0.05) < 1e-9    # nearest hinge: 0.8 + 0.25 - 1
    assert abs(R.decision_margin("triplet", dict(margin=0.8, max_violation=1), [vis, txt]) - 1e-6) < 1e-12   # row 0: .1 and .1 + 1e-6
    assert R.decision_margin("triplet", dict(margin=0.2, max_violation=1), [vis[:1], txt[:1]]) == inf


def test_helper_matches_reference_fixtures(golden):
    """The fp64 helper against the reference's fp32 outputs, every case of pair_losses.pt, as max-norm relative errors (the loss
    relative to max(1, |ref|); gradients under R.grad_scale_floor).  The bound is 1e-5 unless the reference's own fp32 rounding
    is larger.  Measured, the reference's classes run in fp64 on the fixture's inputs against its stored fp32 outputs
    (tests/golden/make_golden_pair_losses.py prints it): loss 3.1e-7, feature gradients 8.7e-7 -- so both keep 1e-5."""
    worst = {"loss": 0.0, "grad": 0.0}
    for c in golden("pair_losses.pt"):
        kind = R.KIND_NAMES[c["kind"]]
        loss, grads = R.loss_and_grads(kind, c["feats"], **c["params"])
        ref = c["loss"].item()
        worst["loss"] = max(worst["loss"], abs(loss.item() - ref) / max(1.0, abs(ref)))
        floor = R.grad_scale_floor(R.grad_scale(kind, c["params"]))
        for g, r in zip(grads, c["grads"]):
            assert g.shape == r.shape
            worst["grad"] = max(worst["grad"], maxrel(r, g, floor))
    print("helper fp64 vs reference fp32:", worst)
    assert worst["loss"] <= 1e-5 and worst["grad"] <= 1e-5, worst
