"""GPU: the learnable-temperature loss family behind xp_contrastive_loss -- the six kinds beside NCELearnableTempLoss and
NCELearnableTempLoss_vsc_fc -- against the reference's fixtures (tests/golden/loss_family.pt), against fp64 autograd of
tests/loss_family_ref.py, the library's operand table against the helper's, and through VidCLIP's backward."""
import functools

import pytest
import torch

from tests import loss_family_ref as R
from tests.gpu_util import ModelArgs, report

pytestmark = pytest.mark.gpu

NEW = R.NEW_KINDS
# (n, m, d, log_scale): more than one wave and one 32-tile, beyond the 128-row small-logits form; d % 4 != 0 (tiled logits at
# small n); img/cap with another row count (the two VidImg kinds only)
BIG, ODD_D, RECT = (200, 200, 96, 3.7), (9, 9, 30, 3.7), (200, 72, 96, 3.7)


def _module(kind):
    from xpretrain_amd.optimization import build_loss_func
    return build_loss_func({"loss_name": R.KINDS[kind][0]})


def _call(fn, kind, feats, ls):
    return fn(feats[0], feats[1], ls) if kind == "dsl" else fn(feats[0], feats[1], feats[2], feats[3], ls)


@functools.lru_cache(maxsize=None)
def _fp64(kind, n, m, d, ls):
    """(features, loss, grads, d log_scale) in fp64 on the CPU: computed once, shared, never modified"""
    feats = R.unit_feats(n, m, d, seed=1000 + n + m + d)
    return (feats, *R.loss_and_grads(kind, feats, ls))


def _run_kind(kind, feats, ls):
    from xpretrain_amd import hip_ops as H
    v, t, i, c = R.operands(kind, [f.float().cuda() for f in feats])
    return H.contrastive_loss(R.KIND_IDS[kind], v, t, i, c, log_scale=torch.tensor(ls, dtype=torch.float32, device="cuda"))


def _check_fp64(tag, out, ref, ls, tol=1e-4):
    _, rl, rg, rdls = ref
    assert abs(out[0].item() - rl.item()) <= tol * abs(rl.item()), tag
    for name, g, r in zip(("dV", "dT", "dI", "dC"), out[1:5], rg):
        assert (g is None) == (r is None), (tag, name)
        if g is not None:
            assert report(f"{tag} {name}", g, r, tol, scale_floor=R.grad_scale_floor(ls)) <= tol
    assert abs(out[5].item() - rdls.item()) <= tol * max(1.0, abs(rdls.item())), tag


@pytest.mark.parametrize("kind", NEW)
def test_family_against_reference_fixtures(golden, kind):
    """1. every case of loss_family.pt through the module surface and autograd, incoming scalar 2.0; the bounds of
    test_embed_loss_gpu.py (gradient errors relative to max(max|ref|, R.grad_scale_floor): the fixture holds saturated
    cases whose reference gradients are 1e-13, all rounding residue)."""
    name = R.KINDS[kind][0]
    fn = _module(kind)
    cases = [c for c in golden("loss_family.pt") if name in c["losses"]]
    assert len(cases) == (24 if kind.startswith("vidimg") else 18)
    for c in cases:
        feats = [f.cuda().requires_grad_() for f in c["feats"]]
        ls = torch.tensor(c["log_scale"], device="cuda", requires_grad=True)
        loss = _call(fn, kind, feats, ls)
        ref_l, ref_g = c["losses"][name].item(), c["grads"][name]
        used = [k for k in range(4) if ref_g[k] is not None]
        grads = torch.autograd.grad(loss * 2.0, [feats[k] for k in used] + [ls])
        tag = f"{kind} n={c['n']} m={c['m']} ls={c['log_scale']:.2f}"
        print(f"{tag}: loss {loss.item():.6f} ref {ref_l:.6f}")
        assert abs(loss.item() - ref_l) <= 1e-3 * max(1.0, abs(ref_l)), tag
        for k, g in zip(used, grads):
            assert report(f"{tag} d{'VTIC'[k]}", g / 2.0, ref_g[k], 1e-3, scale_floor=R.grad_scale_floor(c["log_scale"])) <= 1e-3
        r = ref_g[4].item()
        assert abs(grads[-1].item() / 2.0 - r) <= 1e-3 * max(1.0, abs(r)), tag


@pytest.mark.parametrize("kind,shape", [(k, s) for k in NEW for s in (BIG, ODD_D)] + [(k, RECT) for k in ("vidimg", "vidimg_divide")])
def test_family_against_fp64(kind, shape):
    """2. every new kind against fp64 autograd of the helper: loss within 1e-4 relative, gradients within 1e-4"""
    ref = _fp64(kind, *shape)
    out = _run_kind(kind, ref[0], shape[3])
    _check_fp64(f"{kind} fp64 n={shape[0]} m={shape[1]} d={shape[2]}", out, ref, shape[3])


def test_operands_query_is_the_kind_table():
    """3. which operands a kind reads is the library's to say (xp_contrastive_loss_operands): it agrees with the helper's table for
    every kind, refuses an unknown kind, and the wrapper hands out gradients for exactly those operands.  (The bits of every
    kind, nce and vsc_fc through their former entries included, are pinned by tests/test_loss_bits_gpu.py.)"""
    import ctypes as C
    from xpretrain_amd import hip_ops as H
    query = H.L.lib().xp_contrastive_loss_operands
    feats = [f.float().cuda() for f in R.unit_feats(6, 6, 32, seed=5)]
    for kind in list(R.KINDS) + [len(R.KINDS), -1, 1000]:
        img, cap = C.c_int32(-1), C.c_int32(-1)
        rc = query(R.KIND_IDS.get(kind, kind), C.byref(img), C.byref(cap))
        if kind in R.KINDS:
            use = R.KINDS[kind][1:]
            assert rc == 0 and (img.value, cap.value) == use and H.loss_operands(R.KIND_IDS[kind]) == use, kind
            out = H.contrastive_loss(R.KIND_IDS[kind], *feats, log_scale=torch.tensor(1.0, device="cuda"))
            assert [g is not None for g in out] == [True, True, True, *use, True], kind
        else:
            assert rc != 0 and (img.value, cap.value) == (-1, -1) and H.L.lib().xp_last_error().startswith(b"xp_contrastive_loss: unknown kind")
            with pytest.raises(RuntimeError, match=r"xp_contrastive_loss: unknown kind"):
                H.loss_operands(kind)
    assert query(0, None, None) != 0


@pytest.mark.parametrize("kind", NEW)
def test_family_is_deterministic(kind):
    """4. two runs, identical bits"""
    for n, d in ((70, 32), (200, 96)):
        feats = R.unit_feats(n, n, d, seed=7 * n + d)
        a, b = _run_kind(kind, feats, 4.6), _run_kind(kind, feats, 4.6)
        for x, y in zip(a, b):
            assert (x is None and y is None) or torch.equal(x, y)
        assert all(torch.isfinite(x).all() for x in a if x is not None)


@pytest.mark.parametrize("kind", ["vs_vc", "vsc"])
def test_unread_operand_gets_no_gradient(kind):
    """5. vs_vc / vsc take img_feat and do not read it: no gradient reaches it, the others match the fp64 yardstick"""
    ref = _fp64(kind, *BIG)
    feats = [f.float().cuda().requires_grad_() for f in ref[0]]
    ls = torch.tensor(BIG[3], dtype=torch.float32, device="cuda", requires_grad=True)
    loss = _call(_module(kind), kind, feats, ls)
    loss.backward()
    assert feats[2].grad is None
    got = (loss, feats[0].grad, feats[1].grad, None, feats[3].grad, ls.grad)
    assert all(torch.isfinite(g).all() for g in got if g is not None)
    _check_fp64(f"{kind} module n={BIG[0]}", got, ref, BIG[3])


def test_refusals():
    """6. what a kind rules out is refused by the library before any launch"""
    from xpretrain_amd import _lib as L
    from xpretrain_amd import hip_ops as H
    v, t, i, c = (f.float().cuda() for f in R.unit_feats(6, 4, 32, seed=3))
    c6 = R.unit_feats(6, 6, 32, seed=4)[3].float().cuda()
    ls = torch.tensor(1.0, device="cuda")
    for kind in (L.XP_LOSS_VS_VC, L.XP_LOSS_VSC, L.XP_LOSS_VS_VC_FC, L.XP_LOSS_VSC_FC):
        with pytest.raises(RuntimeError, match=r"xp_contrastive_loss.*m == n.*n=6 m=4"):
            H.contrastive_loss(kind, v, t, i, c, log_scale=ls)
    for kind, img, cap in ((L.XP_LOSS_VS_VC, None, None), (L.XP_LOSS_VSC, None, None), (L.XP_LOSS_VS_VC_FC, None, c6),
                           (L.XP_LOSS_VIDIMG, None, c), (L.XP_LOSS_VIDIMG_DIVIDE, i, None)):
        with pytest.raises(RuntimeError, match=r"xp_contrastive_loss.*null pointer"):
            H.contrastive_loss(kind, v, t, img, cap, log_scale=ls)
    for kind in (8, -1, 1000):
        with pytest.raises(RuntimeError, match=r"xp_contrastive_loss: unknown kind"):
            H.contrastive_loss(kind, v, t, log_scale=ls)
    with pytest.raises(AssertionError):                                       # loss.py:265, before the library is reached
        _module("vsc")(v, t, i, c, ls)


def _param_grads(model, loss):
    for p in model.parameters():
        p.grad = None
    loss.backward()
    return {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


def test_model_hand_off_vs_vc_fc_and_dsl():
    """7. the tiny seeded model and dual-pass inputs of test_pretrain_step_dual_pass_vsc_fc_against_oracle: VidCLIP.forward,
    the fused loss and backward against the same model with the loss restated in fp32 torch ops on the same features --
    every parameter gradient within that test's gradient bound (8e-2 under report())."""
    from oracle import clipvip_oracle as O
    from xpretrain_amd.modeling import VidCLIP
    torch.manual_seed(11)
    cfgd = O.hf_config_dict(128, 2, 2, 256, 16, 32, 128, 2, 2, 256, 120, 16, 64)
    model = VidCLIP(ModelArgs(cfgd, 4))
    with torch.no_grad():
        model.clipmodel.vision_model.embeddings.temporal_embedding.normal_(0, 0.1)
    B = 4
    video, ids, mask = O.synthetic_inputs(B, 4, 32, 8, vocab=120)
    _, cap_ids, cap_mask = O.synthetic_inputs(B, 1, 32, 8, vocab=120, seed=99)
    image = video[:, 1:2].contiguous()
    model.cuda().train()
    dual = dict(image=image.cuda(), caption_ids=cap_ids[:, None].cuda(), caption_masks=cap_mask[:, None].cuda())
    keys = ("vis_features", "text_features", "img_features", "cap_features")
    for kind, kw, nfeat in (("vs_vc_fc", dual, 4), ("dsl", {}, 2)):
        fn = _module(kind)
        got, want = {}, {}
        for store, fused in ((got, True), (want, False)):
            out = model(video.cuda(), ids.cuda(), mask.cuda(), **kw)
            feats = [out[k] for k in keys[:nfeat]]
            ls = model.clipmodel.logit_scale
            loss = fn(*feats, ls) if fused else R.loss(kind, *feats, log_scale=ls)
            store["loss"] = loss.item()
            store["grads"] = _param_grads(model, loss)
        print(f"hand-off {kind}: loss {got['loss']:.5f} torch ops {want['loss']:.5f}")
        assert abs(got["loss"] - want["loss"]) <= 1e-3 * max(1.0, abs(want["loss"]))
        assert set(got["grads"]) == set(want["grads"]) == {n for n, _ in model.named_parameters()}
        worst = 0.0
        for name, ref in want["grads"].items():
            if ref.abs().max() > 1e-5:
                worst = max(worst, report(f"hand-off {kind} grad {name}", got["grads"][name], ref, 8e-2))
        assert worst <= 8e-2
