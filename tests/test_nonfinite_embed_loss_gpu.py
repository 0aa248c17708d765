"""GPU: NaN and +-Inf planted in one input element of the embedding / pooling / normalise kernels and of every loss kernel -- none
swallowed, none leaked (tests/nonfinite.py states the rule; tests/test_nonfinite_cpu.py proves the reference side of every plant
used here).  No tolerance: an output that depends on the plant is non-finite, an independent one keeps its bits."""
import pytest
import torch

from tests import loss_family_ref as LF
from tests import nonfinite as NF
from tests import nonfinite_cases as NC
from tests import pair_loss_ref as PL

pytestmark = pytest.mark.gpu


def _cuda(inputs):
    return {k: v.cuda() for k, v in inputs.items()}


def _ids(cases):
    return [c.name for c in cases]


# ------------------------------------------------------------------------------------------------------------------ embedding
def _run_embed(case):
    from xpretrain_amd import hip_ops as H
    dtype, kind = case.extra["dtype"], case.name.split("-")[0]

    def run(inputs):
        d = _cuda(inputs)
        if kind == "text_fwd":
            B, Lt, D, V = NC.TEXT_CASE
            return {"x": H.text_embed_fwd(d["ids"], d["tok"], d["pos"], dtype).view(B, Lt, D)}
        if kind == "text_bwd":
            B, Lt, D, V = NC.TEXT_CASE
            d_tok, d_pos = H.text_embed_bwd(d["ids"], d["dx"], V, Lt)
            return {"d_tok": d_tok, "d_pos": d_pos}
        if kind == "vip_bwd":
            B, M, T, L, D = NC.VIP_BWD_CASE
            return dict(zip(("d_class", "d_added", "d_pos", "d_time"), H.vip_embed_bwd(d["dx"], B, M, T, L, D)))
        if kind == "gather":
            B, S, D = NC.GATHER_CASE
            return {"out": H.gather_rows(d["x"], d["idx"], B, S, D)}
        if kind == "scatter":
            B, S, D = NC.GATHER_CASE
            return {"dx": H.scatter_rows(d["dout"], d["idx"], B, S, D).view(B, S, D)}
        rows, cols = NC.L2NORM_CASE
        if kind == "l2norm_fwd":
            return dict(zip(("y", "inv"), H.l2norm_fwd(d["x"], rows, cols)))
        assert kind == "l2norm_bwd"
        return {"dx": H.l2norm_bwd(d["dy"], d["y"], d["inv"], rows, cols, dtype)}
    return run


@pytest.mark.parametrize("case", NC.embed_cases(), ids=_ids(NC.embed_cases()))
def test_embedding_kernels_carry_a_planted_value_and_nothing_else(case):
    """text embedding forward / backward, the ViP embedding backward, gather / scatter of the pooled row, l2norm forward / backward:
    the outputs that read the planted element are non-finite, every other row and column keeps its bits, and a plant in a table
    row no sample uses (an unused token, a position beyond Lt, a row that is not gathered) changes nothing."""
    n = NF.drive(case, _run_embed(case))
    print(f"{case.name}: {n} required outputs non-finite")


# ------------------------------------------------------------------------------------------------------------------ the loss family
_LOSS_OUT = ("loss", "d_vis", "d_txt", "d_img", "d_cap", "d_log_scale")


def _run_loss(case):
    from xpretrain_amd import hip_ops as H
    kind = case.extra["kind"]

    def run(inputs):
        d = _cuda(inputs)
        v, t, i, c = LF.operands(kind, [d[k] for k in ("vis", "txt", "img", "cap")])
        return dict(zip(_LOSS_OUT, H.contrastive_loss(LF.KIND_IDS[kind], v, t, i, c, log_scale=d["log_scale"])))
    return run


@pytest.mark.parametrize("case", NC.loss_cases(), ids=_ids(NC.loss_cases()))
def test_loss_family_carries_a_planted_value(case):
    """the eight kinds through hip_ops.contrastive_loss at tiled logits, the small-logits form and (VidImg) m != n: NaN in one element
    of every operand the kind reads, NaN and +inf in log_scale -> the loss, d log_scale and every gradient the element reaches"""
    n = NF.drive(case, _run_loss(case))
    print(f"{case.name}: {n} required outputs non-finite")


@pytest.mark.parametrize("kind", [k for k, (_, img, cap) in LF.KINDS.items() if not (img and cap)])
def test_loss_family_never_reads_an_operand_its_kind_does_not_have(kind):
    """xp_contrastive_loss itself with NaN-filled img / cap (and their gradient buffers) for a kind that reads neither or not img:
    every output bit-equal to the call that passes NULL there, and the unread gradient buffers untouched"""
    from xpretrain_amd import _lib as L
    from xpretrain_amd import hip_ops as H
    case = NC.loss_case(kind, NC.LOSS_SHAPES[0])
    n, m, d = case.extra["shape"]
    dev = _cuda(case.inputs)
    want = _run_loss(case)(case.inputs)
    reads = case.extra["reads"]
    ops = [dev["vis"], dev["txt"]] + [dev[k] if reads[k] else torch.full((m, d), NF.NAN, device="cuda") for k in ("img", "cap")]
    grads = [torch.full_like(t, NF.NAN) for t in ops]
    loss, dls = torch.empty((), device="cuda"), torch.empty((), device="cuda")
    ws = torch.empty(L.lib().xp_contrastive_loss_workspace_bytes(LF.KIND_IDS[kind], n, m, d), dtype=torch.uint8, device="cuda")
    rc = L.lib().xp_contrastive_loss(LF.KIND_IDS[kind], *[H._p(t) for t in ops], H._p(dev["log_scale"]), H._p(loss),
                                     *[H._p(g) for g in grads], H._p(dls), n, m, d, H._p(ws), ws.numel(), H._stream())
    assert rc == 0, L.lib().xp_last_error().decode()
    got = dict(zip(_LOSS_OUT, (loss, *[g if reads.get(k, True) else None for k, g in zip(("vis", "txt", "img", "cap"), grads)], dls)))
    NF.check_equal({k: v for k, v in got.items() if v is not None}, want, f"{kind} unread operands")
    for k, g in zip(("vis", "txt", "img", "cap"), grads):
        if not reads.get(k, True):
            assert torch.isnan(g).all(), f"{kind}: the gradient buffer of the unread {k} was written"


# ------------------------------------------------------------------------------------------------------------------ the pair losses
def _run_pair(case):
    from xpretrain_amd import hip_ops as H
    kind, p = case.extra["kind"], case.extra["params"]

    def run(inputs):
        return dict(zip(("loss", "d_vis", "d_txt"), H.pair_loss(PL.KIND_IDS[kind], inputs["vis"].cuda(), inputs["txt"].cuda(), **p)))
    return run


@pytest.mark.parametrize("case", NC.pair_cases(), ids=_ids(NC.pair_cases()))
def test_pair_losses_carry_a_planted_value(case):
    """every pair_loss_ref.configs(9) entry at (9, 30): NaN in one element of vis and of txt -> the loss and every gradient element
    the reference makes non-finite; the clean inputs keep MIN_MARGIN from every switch, as in tests/test_pair_loss_gpu.py"""
    margin = PL.decision_margin(case.extra["kind"], case.extra["params"], [case.inputs["vis"], case.inputs["txt"]])
    assert margin >= PL.MIN_MARGIN, margin
    n = NF.drive(case, _run_pair(case))
    print(f"{case.name}: {n} required outputs non-finite")
