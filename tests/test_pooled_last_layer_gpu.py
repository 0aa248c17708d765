"""GPU: the opt-in pooled last layer of the video tower (CLIPModel.pooled_last_layer / XPRETRAIN_POOLED_LAST=1): the last
encoder layer computes token 0 of every sample only (functional.PooledEncoderLayerFn, csrc/layer.hip:
xp_encoder_layer_pooled_fwd / _bwd, csrc/attention_pooled.hip).  It is the same mathematical function as the dense layer, so it
is held to the gates the dense step is held to -- the fp32 oracle in fp32 mode, the reference's fp32 results of the committed
full-size fixtures in bf16 (tests/gpu_util.py::TOL / TOL_B8, as tests/test_fullsize_parity_gpu.py applies them) -- and NOT to
bit-equality with the dense path in bf16 (the dense attention rounds P and dS to bf16 as matrix-core operands, the single-query
kernel keeps them in fp32).  Every case prints the dense run's deviations next to the pooled run's."""
import math

import pytest
import torch

from oracle import clipvip_oracle as O
from tests.gpu_util import LOGITS_VS_REFERENCE_BF16, TOL, TOL_B8, ModelArgs, loss_gate, report, seeded_model

pytestmark = pytest.mark.gpu


def _step(model, video, ids, mask, pooled, loss_fn=None, **extra):
    """one training step from the model's current weights with the switch set; returns (outputs, loss, gradients)"""
    from xpretrain_amd.optimization import NCELearnableTempLoss
    model.clipmodel.pooled_last_layer = pooled
    for p in model.parameters():
        p.grad = None
    out = model(video, ids, mask, **extra)
    if loss_fn is None:
        loss = NCELearnableTempLoss()(out["vis_features"], out["text_features"], model.clipmodel.logit_scale)
    else:
        loss = loss_fn(out)
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}
    return {k: v.detach().clone() for k, v in out.items()}, loss.detach().clone(), grads


def _tiny(seed=7, layers=4):
    from xpretrain_amd.modeling import VidCLIP
    torch.manual_seed(seed)
    cfgd = O.hf_config_dict(128, 2, layers, 256, 16, 32, 128, 2, 3, 256, 120, 16, 64)
    model = VidCLIP(ModelArgs(cfgd, 3)).cuda().train()
    with torch.no_grad():
        model.clipmodel.vision_model.embeddings.temporal_embedding.normal_(0, 0.02)
    return model, tuple(t.cuda() for t in O.synthetic_inputs(4, 3, 32, 12, vocab=120)), cfgd


# ------------------------------------------------------------------------------------------------ fp32 mode against the oracle
def test_pooled_fp32_mode_against_oracle_and_dense():
    """BASELINE config #1's architecture in fp32 compute mode (as test_fp32_compute_mode_against_oracle): the pooled step
    against the fp32 oracle -- features and loss within TOL["fp32_abs"], every parameter gradient within 5e-3 of its scale (same
    skips: reference gradients below 1e-6, and k_proj.bias, whose gradient is mathematically zero) -- and against the dense step
    of the same model, same bounds."""
    from xpretrain_amd.modeling import VidCLIP
    torch.manual_seed(1234)
    cfgd = O.vit_b_config(patch=32)
    model = VidCLIP(ModelArgs(cfgd, 12))
    with torch.no_grad():
        model.clipmodel.vision_model.embeddings.temporal_embedding.normal_(0, 0.02)
    video, ids, mask = O.synthetic_inputs(2, 2, 224, 16)
    cfg = O.OracleCfg.from_hf_dict(cfgd)
    sd = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in O.strip_prefix(model.state_dict()).items()}
    ref_loss, ref_vis, ref_txt = O.full_step(video, ids, mask, sd, cfg)
    ref_loss.backward()
    ref_g = {k: v.grad for k, v in sd.items() if v.grad is not None}
    model.cuda().train()
    model.clipmodel.set_compute_dtype(torch.float32)
    v, i, m = video.cuda(), ids.cuda(), mask.cuda()
    runs = {"dense": _step(model, v, i, m, False), "pooled": _step(model, v, i, m, True)}
    worst = {}
    for tag, (out, loss, grads) in runs.items():
        dv = (out["vis_features"].cpu() - ref_vis.detach()).abs().max().item()
        dt = (out["text_features"].cpu() - ref_txt.detach()).abs().max().item()
        dl = abs(loss.item() - ref_loss.item())
        w = 0.0
        for name, g in grads.items():
            key = name[len("clipmodel."):]
            if ref_g[key].abs().max() <= 1e-6 or name.endswith("k_proj.bias"):
                continue
            w = max(w, report(f"fp32 mode {tag} grad {name}", g, ref_g[key], 5e-3))
        worst[tag] = (dv, dt, dl, w)
        print(f"fp32 mode {tag}: |d vis| {dv:.2e} |d txt| {dt:.2e} |d loss| {dl:.2e} worst gradient {w:.2e}")
    dv, dt, dl, w = worst["pooled"]
    assert dv <= TOL["fp32_abs"] and dt <= TOL["fp32_abs"] and dl <= TOL["fp32_abs"] and w <= 5e-3
    # pooled against dense, same bounds
    (od, ld, gd), (op, lp, gp) = runs["dense"], runs["pooled"]
    assert (od["vis_features"] - op["vis_features"]).abs().max().item() <= TOL["fp32_abs"]
    assert abs(ld.item() - lp.item()) <= TOL["fp32_abs"]
    w = 0.0
    for name in gd:
        if gd[name].abs().max() <= 1e-6 or name.endswith("k_proj.bias"):
            continue
        w = max(w, report(f"fp32 mode pooled vs dense grad {name}", gp[name], gd[name], 5e-3))
    print(f"fp32 mode pooled vs dense: worst gradient {w:.2e}")
    assert w <= 5e-3


# ------------------------------------------------------------------------------------------------ bf16, full-size fixtures
def _reference_gates(name, tag, fx, model, out, loss, grads, tol):
    """the gates tests/test_fullsize_parity_gpu.py::_run_case applies to the dense step against the reference's fp32 run:
    features, cosines, logits vs the reference's own bf16 deviation, loss, 1-D and 2-D gradients.  Returns the measured figures
    and the list of failed gates."""
    vis, txt = out["vis_features"].cpu(), out["text_features"].cpu()
    fig = dict(dvis=(vis - fx["vis_features"]).abs().max().item(), dtxt=(txt - fx["text_features"]).abs().max().item(),
               dcos=(vis @ txt.t() - fx["vis_features"] @ fx["text_features"].t()).abs().max().item(),
               dloss=abs(loss.item() - fx["loss"].item()), grad_ref_1d=0.0, grad_ref_2d=0.0)
    bad = []
    if fig["dvis"] > tol["features_abs_full"] or fig["dtxt"] > tol["features_abs_full"]:
        bad.append("features")
    if fig["dcos"] > tol["cos_abs"]:
        bad.append("cosines")
    cal = fx.get("ref_bf16", {})
    if "dlogits" in cal:
        fig["dlogits"] = fig["dcos"] * math.exp(model.clipmodel.logit_scale.item())
        if fig["dlogits"] > LOGITS_VS_REFERENCE_BF16 * cal["dlogits"]:
            bad.append("logits")
    if not loss_gate(loss.item(), fx["loss"].item(), tol["loss_ref_abs"]):
        bad.append("loss")
    for key, ref in fx["grads"].items():
        if key.endswith("#rows"):
            pname = key[:-5]
            pick, ref = ref
            g = grads[pname].cpu()
            scale = g.abs().max().item()
            g = g.reshape(g.shape[0], -1)[pick]
        else:
            pname = key
            g = grads[pname].cpu()
            scale = ref.abs().max().item()
        if scale < 1e-7:
            continue
        err = (g.double() - ref.double()).abs().max().item() / scale
        kind = "grad_ref_2d" if grads[pname].dim() >= 2 else "grad_ref_1d"
        fig[kind] = max(fig[kind], err)
        if err > tol[kind]:
            bad.append(f"{pname}: {err:.3e} > {tol[kind]:.1e}")
    print(f"{name} {tag}: " + " ".join(f"{k}={v:.3e}" for k, v in fig.items()))
    return fig, bad


@pytest.mark.parametrize("name,b8", [("full_cfg2.pt", False), ("full_cfg2_b8.pt", True), ("full_cfg3.pt", False)])
def test_pooled_step_full_size_against_reference(golden, name, b8):
    """The committed full-size fixtures (configs[1] at batch 2 and 8; 8 frames of 448^2: 6276 keys for the pooled query): the
    switch-on step passes the dense step's gates against the reference's fp32 run.  No new tolerance."""
    fx = golden(name)
    tol = dict(TOL, **(TOL_B8 if b8 else {}))
    cfgd = O.vit_b_config(fx["patch"], fx["res"])
    model = seeded_model(cfgd, fx["temporal_size"]).cuda().train()
    video, ids, mask = (t.cuda() for t in O.synthetic_inputs(fx["B"], fx["frames"], fx["res"], fx["txt_len"]))
    out, loss, grads = _step(model, video, ids, mask, False)
    _reference_gates(name, "dense ", fx, model, out, loss, grads, tol)              # (reported; test_fullsize_parity_gpu.py gates it)
    del out, grads
    out, loss, grads = _step(model, video, ids, mask, True)
    fig, bad = _reference_gates(name, "pooled", fx, model, out, loss, grads, tol)
    assert all(g is not None and torch.isfinite(g).all() for g in grads.values())
    assert not bad, f"{name} pooled step vs the reference's fp32 run: {bad}"


# ------------------------------------------------------------------------------------------------ native == op by op
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_native_pooled_calls_equal_the_op_by_op_composition(dtype):
    """xp_encoder_layer_pooled_fwd / _bwd issue the same entry points with the same arguments as the op-by-op composition in
    functional.PooledEncoderLayerFn: features, loss and every gradient are BIT-identical, including a frozen subset (NULL
    gradient pointers) in the pooled layer."""
    import xpretrain_amd.functional as XF
    from xpretrain_amd.modeling import VidCLIP
    torch.manual_seed(9)
    cfgd = O.vit_b_config(16, 224)
    cfgd["vision_config"]["num_hidden_layers"] = 2
    cfgd["text_config"]["num_hidden_layers"] = 2
    model = VidCLIP(ModelArgs(cfgd, 4)).cuda().train()
    model.clipmodel.set_compute_dtype(dtype)
    with torch.no_grad():
        model.clipmodel.vision_model.embeddings.temporal_embedding.normal_(0, 0.02)
    video, ids, mask = (t.cuda() for t in O.synthetic_inputs(8 if dtype == torch.bfloat16 else 2, 4, 224, 16))

    def run(native):
        old, XF.LAYER_CALLS = XF.LAYER_CALLS, native
        try:
            return _step(model, video, ids, mask, True)
        finally:
            XF.LAYER_CALLS = old
    for frozen in ((), ("vision_model.encoder.layers.1.mlp.fc1", "vision_model.encoder.layers.1.layer_norm1",
                        "vision_model.encoder.layers.1.self_attn.k_proj.bias", "vision_model.encoder.layers.1.self_attn.out_proj.weight",
                        "vision_model.encoder.layers.0.layer_norm2")):
        for n, p in model.named_parameters():
            p.requires_grad = not any(f in n for f in frozen)
        (o1, l1, g1), (o0, l0, g0) = run(True), run(False)
        assert torch.equal(o1["vis_features"], o0["vis_features"]) and torch.equal(l1, l0)
        for n in g1:
            if any(f in n for f in frozen):
                assert g1[n] is None and g0[n] is None, n
            else:
                assert g1[n] is not None and torch.equal(g1[n], g0[n]), n


def test_pooled_op_by_op_backward_makes_every_layernorm_call_through_hip_ops(monkeypatch):
    """the op-by-op backward of one pooled layer (B 2, S 9 = 1 + 2*4, D 128, bf16 with side rows) reaches the library's LayerNorm
    backward through ``H.layernorm_bwd`` only -- LN2, LN1 over all rows, LN1 over the pooled rows (the pass whose parameter-gradient
    partial rows are dropped) -- where tools/determinism_hunt.py can wrap it; dx and all sixteen gradients equal the native call's
    bit for bit"""
    import xpretrain_amd.functional as XF
    from xpretrain_amd import hip_ops as H
    B, S, size, D, heads, Dff = 2, 9, (1, 2, 4), 128, 2, 512
    torch.manual_seed(3)
    g = lambda *shape, s=0.05: (torch.randn(*shape, device="cuda") * s).requires_grad_()
    params = [1 + g(D), g(D), g(D, D), g(D), g(D, D), g(D), g(D, D), g(D), g(D, D), g(D), 1 + g(D), g(D), g(Dff, D), g(Dff), g(D, Dff), g(D)]
    params = [p.detach().requires_grad_() for p in params]
    side = torch.randn(B * size[0], D, device="cuda")
    x = torch.randn(B * S, D, device="cuda").bfloat16()
    x.view(B, S, D)[:, :size[0]] = side.view(B, size[0], D).bfloat16()
    x.requires_grad_()
    w = torch.randn(B, D, device="cuda")
    calls = []
    real = H.layernorm_bwd

    def counted(*a, **k):
        calls.append((a[5], k.get("name")))
        return real(*a, **k)

    def run(native):
        monkeypatch.setattr(XF, "LAYER_CALLS", native)
        for t in [x] + params:
            t.grad = None
        x3, side_out = XF.PooledEncoderLayerFn.apply(x, *params, B, S, heads, size, True, side)
        assert side_out.shape == (B, D) and not side_out.requires_grad
        (x3.float() * w).sum().backward()
        torch.cuda.synchronize()
        return [t.grad.clone() for t in [x] + params]
    native = run(True)
    monkeypatch.setattr(H, "layernorm_bwd", counted)
    ops = run(False)
    assert calls == [(B, "ln2"), (B * S, "ln1"), (B, "ln1_pooled")]
    assert len(native) == len(ops) == 17
    for i, (a, b) in enumerate(zip(native, ops)):
        assert torch.equal(a, b), f"gradient {i} differs between the native call and the op-by-op path"


def _pooled_layer_case(dtype, sided):
    """PooledEncoderLayerFn's arguments at the one-layer shape: B 2, S 9 = 1 + 2*4, D 128, heads 2, Dff 512"""
    from tests.layer_paths import layer_input, layer_params
    B, S, size, D, heads, Dff = 2, 9, (1, 2, 4), 128, 2, 512
    params = layer_params(D, Dff)
    x, side = layer_input(B, S, D, dtype, size[0] if sided else 0)
    return x, params, (B, S, heads, size, True, side), torch.randn(B, D, device="cuda")


@pytest.mark.parametrize("dtype,sided", [(torch.bfloat16, True), (torch.float32, False)], ids=["bf16-side", "fp32"])
def test_one_pooled_layer_saves_and_returns_the_same_bits_on_either_path(dtype, sided):
    """PooledEncoderLayerFn applied directly with LAYER_CALLS on and off: both sequencers fill the same arena -- all sixteen saved
    pieces equal view by view -- and give the same x3, side_out, side_x2, dx and sixteen gradients; again with a frozen subset,
    whose gradients are None on both paths"""
    import xpretrain_amd.functional as XF
    from tests.layer_paths import FROZEN, both_paths
    x, params, tail, w = _pooled_layer_case(dtype, sided)
    for frozen in ((), FROZEN):
        got = both_paths(XF.PooledEncoderLayerFn, x, params, tail, w, frozen)
        assert len([n for n in got if n.startswith("piece:")]) == 16
        assert (got["side_out"] is not None) == (got["side_x2"] is not None) == sided


def test_pooled_op_by_op_backward_runs_under_the_fingerprinting_wrappers():
    """tools/determinism_hunt.install wraps every hip_ops entry (and replaces colsum_deferred): one pooled op-by-op pass at the
    one-layer shape completes under it -- the replacement forwards ``out=`` -- records fingerprints, and gives the native gradients"""
    import importlib.util
    import os
    import xpretrain_amd.functional as XF
    from xpretrain_amd import hip_ops as H
    from tests.layer_paths import assert_same, run_layer
    spec = importlib.util.spec_from_file_location(
        "determinism_hunt", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "determinism_hunt.py"))
    hunt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(hunt)
    x, params, tail, w = _pooled_layer_case(torch.bfloat16, True)
    native = run_layer(XF.PooledEncoderLayerFn, True, x, params, tail, w)
    for t in [x] + params:
        t.grad = None
    rec = hunt.Recorder("sum")
    saved, flush = dict(vars(H)), H.DeferredReduce.flush
    try:
        hunt.install(rec)
        ops = run_layer(XF.PooledEncoderLayerFn, False, x, params, tail, w)
    finally:
        for n, f in saved.items():
            setattr(H, n, f)
        H.DeferredReduce.flush = flush
    assert_same(native, ops)
    labels = [l for l, _ in rec.items]
    assert sum(l.startswith("colsum_deferred") for l in labels) == 2 and not rec.deferred      # db1 and dbq, finished by the flush
    assert any(l.startswith("attn_pooled_bwd") for l in labels) and sum(l.startswith("layernorm_bwd") for l in labels) >= 3


# ------------------------------------------------------------------------------------------------ where the switch applies
def test_switch_falls_back_to_dense_where_the_stream_is_read(monkeypatch):
    """output_hidden_states=True, the vision tower called directly, a forward hook on the last layer: torch.equal to the
    switch-off outputs (dense last layer).  Switch off: torch.equal to a model that never saw the attribute.  Switch on:
    vision_model_output.last_hidden_state is None, the features pass the bf16 feature gate against the dense ones."""
    from xpretrain_amd.modeling import CLIP_ViP
    monkeypatch.setattr(CLIP_ViP.CLIPModel, "pooled_last_layer", False)
    model, (video, ids, mask), _ = _tiny()
    fresh, _, _ = _tiny()                                  # same seed, attribute never set on the instance
    cm = model.clipmodel
    assert "pooled_last_layer" not in vars(fresh.clipmodel)
    o_never, l_never, g_never = _step_untouched(fresh, video, ids, mask)
    o_off, l_off, g_off = _step(model, video, ids, mask, False)
    assert torch.equal(o_off["vis_features"], o_never["vis_features"]) and torch.equal(l_off, l_never)
    assert all(torch.equal(g_off[n], g_never[n]) for n in g_off)

    def direct(pooled):
        cm.pooled_last_layer = pooled
        with torch.no_grad():
            hs = cm(input_ids=ids, pixel_values=video, attention_mask=mask, output_hidden_states=True)
            vo = cm.vision_model(pixel_values=video)
        return hs, vo
    hs0, vo0 = direct(False)
    hs1, vo1 = direct(True)
    assert torch.equal(hs1.image_embeds, hs0.image_embeds)
    assert hs1.vision_model_output.last_hidden_state is not None
    assert torch.equal(hs1.vision_model_output.last_hidden_state, hs0.vision_model_output.last_hidden_state)
    assert all(torch.equal(a, b) for a, b in zip(hs1.vision_model_output.hidden_states, hs0.vision_model_output.hidden_states))
    assert torch.equal(vo1.last_hidden_state, vo0.last_hidden_state) and torch.equal(vo1.pooler_output, vo0.pooler_output)
    # a forward hook on the last layer sees that layer's dense output
    seen = []
    h = cm.vision_model.encoder.layers[-1].register_forward_hook(lambda mod, args, out: seen.append(out))
    try:
        cm.pooled_last_layer = True
        with torch.no_grad():
            hooked = cm(input_ids=ids, pixel_values=video, attention_mask=mask)
    finally:
        h.remove()
    assert len(seen) == 1 and torch.equal(hooked.image_embeds, hs0.image_embeds)
    assert hooked.vision_model_output.last_hidden_state is not None
    # the switch itself
    with torch.no_grad():
        on = cm(input_ids=ids, pixel_values=video, attention_mask=mask)
        fv_on = model.forward_video(video)
        cm.pooled_last_layer = False
        fv_off = model.forward_video(video)
    assert on.vision_model_output.last_hidden_state is None and on.vision_model_output.pooler_output is not None
    assert torch.equal(fv_on, on.image_embeds) and torch.equal(fv_off, hs0.image_embeds)
    d = (fv_on - fv_off).abs().max().item()
    print(f"tiny model, forward_video pooled vs dense: max|d| = {d:.2e}")
    assert d <= TOL["features_abs_full"]


def _step_untouched(model, video, ids, mask):
    from xpretrain_amd.optimization import NCELearnableTempLoss
    out = model(video, ids, mask)
    loss = NCELearnableTempLoss()(out["vis_features"], out["text_features"], model.clipmodel.logit_scale)
    loss.backward()
    torch.cuda.synchronize()
    return ({k: v.detach().clone() for k, v in out.items()}, loss.detach().clone(),
            {n: p.grad.detach().clone() for n, p in model.named_parameters()})


def test_environment_switch_sets_the_class_default():
    """XPRETRAIN_POOLED_LAST=1 turns the class default on (a fresh interpreter reads it at import); unset or 0 is the dense step"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "from xpretrain_amd.modeling.CLIP_ViP import CLIPModel; print(int(CLIPModel.pooled_last_layer))"
    for val, want in ((None, "0"), ("0", "0"), ("1", "1")):
        env = {k: v for k, v in os.environ.items() if k != "XPRETRAIN_POOLED_LAST"}
        if val is not None:
            env["XPRETRAIN_POOLED_LAST"] = val
        got = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=300)
        assert got.returncode == 0 and got.stdout.strip() == want, (val, got.stdout, got.stderr[-500:])


# ------------------------------------------------------------------------------------------------ determinism, checkpointing
def test_pooled_step_repeats_and_checkpoints_bit_identically():
    """two pooled steps from the same state: every gradient torch.equal; gradient checkpointing on (the pooled layer is one more
    function to re-run): features, loss and gradients torch.equal to the non-checkpointed pooled run"""
    model, (video, ids, mask), _ = _tiny()
    o0, l0, g0 = _step(model, video, ids, mask, True)
    o1, l1, g1 = _step(model, video, ids, mask, True)
    assert torch.equal(o0["vis_features"], o1["vis_features"]) and torch.equal(l0, l1)
    assert not [n for n in g0 if not torch.equal(g0[n], g1[n])]
    model.clipmodel.gradient_checkpointing_enable()
    try:
        o2, l2, g2 = _step(model, video, ids, mask, True)
    finally:
        model.clipmodel.gradient_checkpointing_disable()
    assert torch.equal(o0["vis_features"], o2["vis_features"]) and torch.equal(l0, l2)
    bad = [n for n in g0 if not torch.equal(g0[n], g2[n])]
    assert not bad, bad[:5]
    # and a forward-only pass (no MLP pre-activation written) gives the same features bit for bit
    with torch.no_grad():
        assert torch.equal(model.forward_video(video), o0["vis_features"])


@pytest.mark.parametrize("shape", ["vit_b_2layers"])
def test_pooled_step_after_the_two_chain_forward_repeats(shape):
    """at a shape where layers 0..n-2 run as two half-batch chains on two streams: the pooled layer waits for both (join), the
    step is repeatable bit for bit and its features agree with the dense step within the bf16 feature gate"""
    from xpretrain_amd.modeling import VidCLIP
    torch.manual_seed(3)
    cfgd = O.vit_b_config(16, 224)
    cfgd["vision_config"]["num_hidden_layers"] = 3
    cfgd["text_config"]["num_hidden_layers"] = 2
    model = VidCLIP(ModelArgs(cfgd, 12)).cuda().train()
    video, ids, mask = (t.cuda() for t in O.synthetic_inputs(8, 12, 224, 16))
    od, ld, gd = _step(model, video, ids, mask, False)
    o0, l0, g0 = _step(model, video, ids, mask, True)
    o1, l1, g1 = _step(model, video, ids, mask, True)
    assert torch.equal(o0["vis_features"], o1["vis_features"]) and torch.equal(l0, l1)
    assert not [n for n in g0 if not torch.equal(g0[n], g1[n])]
    d = (o0["vis_features"] - od["vis_features"]).abs().max().item()
    print(f"3-layer ViT-B/16 batch 8: pooled vs dense features max|d| = {d:.2e}, loss {l0.item():.5f} vs {ld.item():.5f}")
    assert d <= TOL["features_abs_full"]


# ------------------------------------------------------------------------------------------------ the other step forms
def test_pooled_dual_pass_vsc_fc_step_against_oracle():
    """the pre-training step (video + subtitle pass, T = 1 image + caption pass: S = M + L for the pooled query;
    NCELearnableTempLoss_vsc_fc) with the switch on, against the fp32 oracle with the dense test's gates
    (tests/test_model_gpu.py::test_pretrain_step_dual_pass_vsc_fc_against_oracle); then with the text tower frozen"""
    from xpretrain_amd.modeling import VidCLIP
    from xpretrain_amd.optimization import build_loss_func
    torch.manual_seed(11)
    cfgd = O.hf_config_dict(128, 2, 2, 256, 16, 32, 128, 2, 2, 256, 120, 16, 64)
    model = VidCLIP(ModelArgs(cfgd, 4))
    with torch.no_grad():
        model.clipmodel.vision_model.embeddings.temporal_embedding.normal_(0, 0.1)
    B = 4
    video, ids, mask = O.synthetic_inputs(B, 4, 32, 8, vocab=120)
    _, cap_ids, cap_mask = O.synthetic_inputs(B, 1, 32, 8, vocab=120, seed=99)
    image = video[:, 1:2].contiguous()
    sd = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in O.strip_prefix(model.state_dict()).items()}
    cfg = O.OracleCfg.from_hf_dict(cfgd, temporal_size=4)
    rv, rt = O.clip_features(video, ids, mask, sd, cfg)
    ri, rc = O.clip_features(image, cap_ids, cap_mask, sd, cfg)
    ref_loss = O.nce_vsc_fc_loss(rv, rt, ri, rc, sd["logit_scale"])
    ref_loss.backward()
    model.cuda().train()
    fn = build_loss_func({"loss_name": "NCELearnableTempLoss_vsc_fc"})
    loss_fn = lambda o: fn(o["vis_features"], o["text_features"], o["img_features"], o["cap_features"], model.clipmodel.logit_scale)
    extra = dict(image=image.cuda(), caption_ids=cap_ids[:, None].cuda(), caption_masks=cap_mask[:, None].cuda())
    out, loss, grads = _step(model, video.cuda(), ids.cuda(), mask.cuda(), True, loss_fn, **extra)
    for k, r in (("vis_features", rv), ("text_features", rt), ("img_features", ri), ("cap_features", rc)):
        assert (out[k].cpu() - r.detach()).abs().max().item() < 2e-2, k
    print(f"pooled pretrain step: loss {loss.item():.5f} oracle {ref_loss.item():.5f}")
    assert abs(loss.item() - ref_loss.item()) < 2e-2 * max(1.0, abs(ref_loss.item()))
    worst = 0.0
    for name, g in grads.items():
        ref = sd[name[len("clipmodel."):]].grad
        assert g is not None and ref is not None, name
        if ref.abs().max() > 1e-5:
            worst = max(worst, report(f"pooled pretrain-step grad {name}", g, ref, 8e-2))
    assert worst <= 8e-2
    # frozen text tower: its gradients are absent, everything else is bit-identical to the unfrozen pooled step
    model.freeze_text_encoder(True)
    _, loss_f, grads_f = _step(model, video.cuda(), ids.cuda(), mask.cuda(), True, loss_fn, **extra)
    assert torch.equal(loss_f, loss)
    for n, g in grads_f.items():
        if ".text_model." in n or "text_projection" in n:
            assert g is None, n
        else:
            assert torch.equal(g, grads[n]), n
