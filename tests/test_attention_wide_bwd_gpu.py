"""GPU: the opt-in one-launch attention backward for key windows wider than one LDS group (attn_bwd6_kernel, plan name ``bwd6``,
XPRETRAIN_ATTN_BWD_WIDE=1 / hip_ops.set_attn_bwd_wide): against the fp64 oracle core with the gates of tests/test_attention_gpu.py,
against the dQ / dKV kernel pair on identical inputs with that file's fused-vs-split gate, its bias column sums, q_scale and a late
score spike, the configs[3]-shaped model against the reference fixture and the emulating oracle, and that the switch leaves the
shapes of attn_bwd5_kernel and the switch-off path bit-identical.  Every case asserts through hip_ops.attn_plan that it runs bwd6."""
import pytest
import torch

from oracle import clipvip_oracle as O
from tests import test_attention_gpu as AG
from tests.gpu_util import report, seeded_model

pytestmark = pytest.mark.gpu

# (size, B, H): the wide proxy shapes tests/test_attention_gpu.py runs through the kernel pair (2..6 key groups, 1..5 own blocks),
# M at its limit, and an odd tile count (15 tiles: one 32-row step of the last group reaches past R) with several heads
ORACLE_CASES = [((4, 2, 784), 1, 1), ((4, 3, 300), 2, 2), ((2, 2, 500), 1, 3), ((4, 5, 208), 1, 2), ((1, 2, 1023), 1, 1),
                ((4, 9, 784), 2, 3), ((16, 2, 400), 1, 2), ((3, 6, 230), 2, 5)]
# the pair on identical inputs: those, configs[3] at the bench batch (768 problems: three per CU), more problems than CUs with an odd
# tile count
PAIR_CASES = ORACLE_CASES + [((4, 8, 784), 8, 12), ((3, 40, 230), 3, 5)]


@pytest.fixture
def wide():
    """the switch on for one test, the previous state restored after"""
    from xpretrain_amd import hip_ops as H
    prev = H.get_attn_bwd_wide()
    H.set_attn_bwd_wide(True)
    try:
        yield
    finally:
        H.set_attn_bwd_wide(prev)


def _kernels(size, B, H):
    """(forward, backward) kernels of the case with the switch on: the forward is whatever the device plans, the backward must be bwd6"""
    from xpretrain_amd import hip_ops as Hh
    S = size[0] + size[1] * size[2]
    fwd = Hh.attn_plan(B, S, H, size=size)["kernel"]
    AG.check_kernels((fwd, "bwd6"), B, S, H, size=size)
    return fwd, "bwd6"


@pytest.mark.parametrize("size,B,H", ORACLE_CASES)
def test_wide_backward_against_the_fp64_oracle(size, B, H, wide):
    """tests/test_attention_gpu.py::_run itself (fp64 oracle core on the kernel's own bf16 inputs, 2e-2 of the tensor scale for dq, dk,
    dv, all finite), with the backward planned as bwd6"""
    M, N, L = size
    AG._run(B, H, size, M + N * L, None, seed=M + N + L, kernels=_kernels(size, B, H))


@pytest.mark.parametrize("size", [(4, 1, 300), (4, 3, 300)])
def test_wide_backward_rescale_and_qscale(size, wide):
    """q_scale != 1 and a late score spike at a wide shape, as test_proxy_attention_rescale_and_qscale: the last key of the sample
    is made to dominate the row of query S // 2 -- with one frame that is a frame query whose key sits in the LAST staged group,
    with three frames the key dominates the proxy rows' partials of the last frame"""
    B, H = 1, 2
    M, N, L = size
    AG._run(B, H, size, M + N * L, None, seed=5, kernels=_kernels(size, B, H), scale=2.0, spike=True, q_scale=0.125)


@pytest.mark.parametrize("size,B,Hh", PAIR_CASES)
def test_wide_backward_against_the_two_kernel_path(size, B, Hh):
    """bwd6 against the dQ / dKV kernel pair on identical inputs (switch off vs on): same operands, same rounding points, different
    summation order -- within 1e-2 of the tensor scale per q / k / v block (the gate of
    test_fused_backward_against_the_two_kernel_path; one bf16 ulp is 4e-3).  Two runs with the switch on are bit-identical (the
    counter decides only WHO computes a problem); the bias column sums equal a pass over dqkv as stored, and asking for them does
    not change dqkv."""
    from xpretrain_amd import hip_ops as H
    M, N, Lp = size
    S = M + N * Lp
    prev = H.get_attn_bwd_wide()
    torch.manual_seed(3)
    qkv = (torch.randn(B * S, 3 * Hh * 64, device="cuda") * 0.7).to(torch.bfloat16)
    out, stats = H.attn_fwd(qkv, B, S, Hh, size=size)
    dout = torch.randn_like(out)
    try:
        H.set_attn_bwd_wide(False)
        assert H.attn_plan(B, S, Hh, size=size, backward=True)["kernel"] == "bwd_pair"
        want = H.attn_bwd(qkv, out, dout, stats, B, S, Hh, size=size, q_scale=0.125)
        H.set_attn_bwd_wide(True)
        _kernels(size, B, Hh)
        d = H.DeferredReduce(qkv.device)
        got, cs = H.attn_bwd(qkv, out, dout, stats, B, S, Hh, size=size, q_scale=0.125, colsum_defer=d)
        assert len(d.segs) == 1                      # the fused path: one partial-row segment, no extra pass
        d.flush()
        again = H.attn_bwd(qkv, out, dout, stats, B, S, Hh, size=size, q_scale=0.125)
    finally:
        H.set_attn_bwd_wide(prev)
    assert torch.equal(got, again)
    assert torch.isfinite(got.float()).all()
    errs = []
    for j, name in enumerate("qkv"):
        a, b = [t.view(B * S, 3, Hh * 64)[:, j] for t in (got, want)]
        errs.append(report(f"attn bwd wide vs pair {size} B{B} H{Hh} d{name}", a, b, 1e-2))
    e_cs = report(f"attn bwd wide colsum vs stored {size} B{B} H{Hh}", cs, got.double().sum(0), 1e-5, scale_floor=1e-3)
    assert max(errs) <= 1e-2 and e_cs <= 1e-5


def test_switch_off_after_on_is_the_untouched_path():
    """no sticky state: the pair's output after the switch was on and off again is the output of a call made before it was set"""
    from xpretrain_amd import hip_ops as H
    size, B, Hh = (4, 3, 300), 2, 2
    S = size[0] + size[1] * size[2]
    prev = H.get_attn_bwd_wide()
    torch.manual_seed(8)
    qkv = (torch.randn(B * S, 3 * Hh * 64, device="cuda") * 0.7).to(torch.bfloat16)
    out, stats = H.attn_fwd(qkv, B, S, Hh, size=size)
    dout = torch.randn_like(out)
    try:
        H.set_attn_bwd_wide(False)
        before = H.attn_bwd(qkv, out, dout, stats, B, S, Hh, size=size, q_scale=0.125)
        H.set_attn_bwd_wide(True)
        _kernels(size, B, Hh)
        H.attn_bwd(qkv, out, dout, stats, B, S, Hh, size=size, q_scale=0.125)
        H.set_attn_bwd_wide(False)
        assert H.attn_plan(B, S, Hh, size=size, backward=True)["kernel"] == "bwd_pair"
        after = H.attn_bwd(qkv, out, dout, stats, B, S, Hh, size=size, q_scale=0.125)
    finally:
        H.set_attn_bwd_wide(prev)
    assert torch.equal(before, after)


def test_cfg3_shape_448_with_the_wide_backward(golden, wide):
    """configs[3]'s shape (8 frames of 448^2: R = 788 in every video layer) with the switch on, through the unchanged full-size
    yardstick: hidden states, features, loss and every gradient against the reference's fp32 fixture, every layer's backward
    teacher-forced against the bf16-emulating oracle -- the tolerances of tests/gpu_util.py::TOL, none overridden."""
    from tests.test_fullsize_parity_gpu import _run_case
    from xpretrain_amd import hip_ops as H
    fx = golden("full_cfg3.pt")
    Lp = (fx["res"] // fx["patch"]) ** 2
    size = (4, fx["frames"], Lp)
    assert H.attn_plan(fx["B"], 4 + fx["frames"] * Lp, 12, size=size, backward=True)["kernel"] == "bwd6"
    _run_case(golden, "full_cfg3.pt", emu_backward=True)


def test_switch_does_not_touch_the_one_group_shapes():
    """a two-layer ViT-B-width model at 224^2 (R = 200: attn_bwd5_kernel's shape): loss, features and every gradient are bit-identical
    with the switch on and off"""
    from xpretrain_amd import hip_ops as H
    from xpretrain_amd.optimization import NCELearnableTempLoss
    cfgd = O.vit_b_config(16, 224)
    cfgd["vision_config"]["num_hidden_layers"] = 2
    cfgd["text_config"]["num_hidden_layers"] = 2
    model = seeded_model(cfgd, 4).cuda().train()
    video, ids, mask = (t.cuda() for t in O.synthetic_inputs(2, 4, 224, 16))
    assert H.attn_plan(2, 4 + 4 * 196, 12, size=(4, 4, 196), backward=True)["kernel"] == "bwd5"
    prev = H.get_attn_bwd_wide()

    def step(on):
        H.set_attn_bwd_wide(on)
        assert H.attn_plan(2, 4 + 4 * 196, 12, size=(4, 4, 196), backward=True)["kernel"] == "bwd5"
        model.zero_grad(set_to_none=True)
        out = model(video, ids, mask)
        loss = NCELearnableTempLoss()(out["vis_features"], out["text_features"], model.clipmodel.logit_scale)
        loss.backward()
        return loss.detach().clone(), out["vis_features"].detach().clone(), out["text_features"].detach().clone(), \
            {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    try:
        off, on = step(False), step(True)
    finally:
        H.set_attn_bwd_wide(prev)
    assert all(torch.equal(a, b) for a, b in zip(off[:3], on[:3]))
    assert off[3].keys() == on[3].keys() and all(torch.equal(off[3][n], on[3][n]) for n in off[3])
