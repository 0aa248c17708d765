"""CPU: the reference side of the non-finite tests (tests/nonfinite.py states the rule), for every (case, element, value) the GPU files
plant -- the same lists, tests/nonfinite_cases.py:
  (a) the fp64 reference run with the value planted is non-finite on all of D(e);
  (b) D(e) equals the structural set wherever the plant states one (an empty one for an element that must reach nothing);
  (c) the reference is bit-unchanged on I(e);
and a +-inf plant has the same non-finite set in the fp32 reference as in the fp64 one.  This is what makes the GPU tests non-vacuous:
they require of a kernel only what the reference alone already does.

The number of outputs required per family is pinned, so that it cannot shrink unnoticed.  The helper's own `check` is held against
constructed outputs at the end."""
import pytest
import torch

from tests import nonfinite as NF
from tests import nonfinite_cases as NC

FAMILIES = {
    "gemm": NC.gemm_cases, "layernorm": NC.layernorm_cases, "attention": NC.attention_cases, "pooled": NC.pooled_cases,
    "probs": NC.probs_cases,     "embed": NC.embed_cases, "loss": NC.loss_cases, "pair": NC.pair_cases,
}
# (cases, planted (element, value) pairs, outputs that must be non-finite) per family
REQUIRED = {
    "gemm": (26, 352, 90027), "layernorm": (41, 628, 889606), "attention": (10, 102, 2768218), "pooled": (2, 16, 53908), "probs": (4, 28, 770),
    "embed": (14, 78, 3738), "loss": (18, 96, 316012), "pair": (11, 22, 8124),
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_reference_carries_every_plant_the_gpu_tests_use(family):
    cases = FAMILIES[family]()
    total = sum(NF.verify_reference(c) for c in cases)
    got = (len(cases), sum(len(c.pairs()) for c in cases), total)
    print(f"{family}: {got[0]} cases, {got[1]} planted (element, value) pairs, {got[2]} outputs required to be non-finite")
    assert got == REQUIRED[family]


def test_selected_cases_are_the_ones_the_issue_names():
    ids = {c.name for c in NC.gemm_cases()}
    assert {"splitk-3-g256", "splitk-3-direct", "splitk-3-f32", "aremap-ks-split", "edge-ld-all", "edge-ld-gelu-aux", "edge-ld-tn"} <= ids
    fams = {(c.extra["case"]["expect"]["family"], c.extra["case"]["epi"]) for c in NC.gemm_cases()}
    for fam in ("g256", "direct", "staged"):
        assert {(fam, e) for e in ("bias", "gelu", "resid", "gelu_bwd", "qscale")} <= fams
    assert {("direct", "patch"), ("staged", "patch"), ("frames", "patch"), ("frames", "bias")} <= fams
    f, b = NC.layernorm_table()
    assert {(c.dtype, c.cols) for c in f} >= {(d, w) for d in ("bf16", "f32") for w in NC.LR.FWD_WIDTHS}
    assert {(c.dtype, c.cols) for c in b} >= {(d, w) for d in ("bf16", "f32") for w in NC.LR.BWD_WIDTHS}
    assert {c.side for c in f if c.side} == {s for _, s in NC.LR.SIDES}
    assert all(n in NC.AE.CASES for n, _, _ in NC.ATTN_RUNS)
    assert {c.extra["kind"] for c in NC.loss_cases()} == set(NC.LF.KINDS) and len(NC.pair_cases()) == len(NC.PL.configs(9))


def test_triplet_swallow_is_expressible():
    """the kernel fault the GPU test found: a triplet hinge that is false for NaN gives a finite loss -- `check` names it"""
    case = next(c for c in NC.pair_cases() if c.name == "triplet-margin=0.2")
    p = case.plants[0]
    clean = case.ref(case.inputs)
    req = case.required(p, NF.NAN)
    assert bool(req["loss"]) and req["d_txt"].any()
    with pytest.raises(AssertionError, match="loss: finite where it depends on the plant"):
        NF.check(clean, clean, req, None, "a kernel whose hinge drops the NaN")
    NF.check(case.ref(NF.plant(NF.as_double(case.inputs), p.which, p.index, NF.NAN)), clean, req, None, "the reference")


def test_check_names_every_violation_and_passes_a_clean_run():
    clean = {"y": torch.arange(6.0).view(2, 3), "s": torch.ones(2)}
    D = {"y": torch.tensor([[True, True, True], [False, False, False]]), "s": torch.tensor([True, False])}
    I = {k: ~m for k, m in D.items()}
    good = {"y": clean["y"].clone(), "s": clean["s"].clone()}
    good["y"][0], good["s"][0] = NF.NAN, NF.INF
    NF.check(good, clean, D, I, "good")
    bad = {"y": good["y"].clone(), "s": good["s"].clone()}
    bad["y"][0, 1] = 0.0                      # swallowed
    bad["y"][1, 2] = NF.NAN                   # leaked
    bad["s"][1] = 2.0                         # an independent problem moved
    with pytest.raises(AssertionError) as e:
        NF.check(bad, clean, D, I, "bad")
    msg = str(e.value)
    assert "y: finite where it depends" in msg and "y: non-finite in an independent" in msg and "s: an independent problem's bits moved" in msg
    NF.check_equal(good, {k: v.clone() for k, v in good.items()}, "equal, NaN included")
    with pytest.raises(AssertionError, match="never read"):
        NF.check_equal(good, clean, "differs")


def test_dependent_set_and_plant():
    ref = lambda inp, dtype=torch.float64: {"y": inp["a"].to(dtype) @ inp["b"].to(dtype).t()}
    inputs = {"a": torch.arange(6.0).view(2, 3), "b": torch.ones(4, 3)}
    D = NF.dependent_set(ref, inputs, "a", 4)
    assert torch.equal(D["y"], torch.tensor([[False] * 4, [True] * 4]))
    D = NF.dependent_set(ref, inputs, "b", 4)
    assert torch.equal(D["y"], torch.tensor([[False, True, False, False]] * 2))
    planted = NF.plant(inputs, "a", 4, NF.NAN)
    assert torch.isnan(planted["a"][1, 1]) and torch.isfinite(inputs["a"]).all() and planted["b"] is inputs["b"]
