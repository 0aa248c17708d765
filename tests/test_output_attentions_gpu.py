"""GPU: ``output_attentions=True`` through the model surface (modeling/CLIP_ViP.py), on the model of tests/golden/tiny_e2e.pt.

Text tower: the reference's own ``attentions`` (tests/golden/tiny_attentions.pt).  Video tower (a documented extension: the reference
returns None there): the fp64 layer-level restatement (tests/attn_probs_ref.py) fed the reference's hidden states.  In bf16 every
layer's entry is pinned bit for bit to ``hip_ops.attn_probs`` on the qkv / statistics recomputed from the model's own hidden states,
and the flag must move nothing else: features, hidden states, gradients -- under the text tower's side stream, the two half-batch
chains of the video tower, gradient checkpointing and the pooled last layer."""
import pytest
import torch

from oracle import clipvip_oracle as O
from tests import attn_probs_ref as R
from tests.gpu_util import LOGITS_VS_REFERENCE_BF16, TOL, ModelArgs

pytestmark = pytest.mark.gpu


def _tiny(golden, dtype=torch.bfloat16, train=False):
    from xpretrain_amd.modeling import VidCLIP
    fx = golden("tiny_e2e.pt")
    model = VidCLIP(ModelArgs(fx["config"], fx["temporal_size"], fx["add_cls_num"]))
    model.load_state_dict(fx["state_dict"], strict=True)
    model.cuda().train(train)
    model.clipmodel.set_compute_dtype(dtype)
    return model, fx, tuple(fx[k].cuda() for k in ("video", "ids", "mask"))


def _dev(tag, a, b):
    d = (a.double().cpu() - b.double().cpu()).abs().max().item()
    print(f"{tag}: max |d| = {d:.3e}")
    return d


def test_fp32_mode_text_attentions_against_the_reference(golden):
    model, fx, (video, ids, mask) = _tiny(golden, torch.float32)
    ref = golden("tiny_attentions.pt")["text_attentions"]
    with torch.no_grad():
        att = model.clipmodel.text_model(input_ids=ids, attention_mask=mask, output_attentions=True).attentions
    assert isinstance(att, tuple) and len(att) == len(ref) == 2
    for i, (a, b) in enumerate(zip(att, ref)):
        assert a.dtype == torch.float32 and tuple(a.shape) == tuple(b.shape) == (4, 2, 12, 12) and not a.requires_grad
        assert _dev(f"fp32 mode text attentions[{i}] vs reference", a, b) <= TOL["fp32_abs"]
        assert torch.equal(a.triu(1), torch.zeros_like(a))


def test_fp32_mode_video_attentions_against_the_restatement(golden):
    from xpretrain_amd.modeling.CLIP_ViP import ViPAttentions
    model, fx, (video, ids, mask) = _tiny(golden, torch.float32)
    sd = O.strip_prefix(fx["state_dict"])
    size, S = (4, 3, 16), 52
    with torch.no_grad():
        att = model.clipmodel.vision_model(pixel_values=video, output_attentions=True).attentions
    assert isinstance(att, tuple) and len(att) == 2
    for i, a in enumerate(att):
        assert isinstance(a, ViPAttentions) and a.proxy is a[0] and a.frame is a[1]
        assert tuple(a.proxy.shape) == (4, 2, 4, S) and tuple(a.frame.shape) == (4, 2, 3, 16, 20)
        assert a.proxy.dtype == a.frame.dtype == torch.float32 and not a.proxy.requires_grad and not a.frame.requires_grad
        proxy, frame = R.layer_probs(fx["vision_hidden"][i], sd, f"vision_model.encoder.layers.{i}.", 2, size=size)
        assert _dev(f"fp32 mode video attentions[{i}].proxy vs restatement", a.proxy, proxy) <= TOL["fp32_abs"]
        assert _dev(f"fp32 mode video attentions[{i}].frame vs restatement", a.frame, frame) <= TOL["fp32_abs"]


def _recomputed(layer, hidden, side, B, S, size, pad):
    """the layer's attention weights from its input, by the three hip_ops calls of EncoderLayerFn's op-by-op branch + attn_probs"""
    import xpretrain_amd.functional as XF
    from xpretrain_amd import _lib as L
    from xpretrain_amd import hip_ops as H
    a = layer.self_attn
    D, heads = hidden.shape[-1], layer.num_heads
    x = hidden.reshape(B * S, D).contiguous()
    Wqkv = XF.WEIGHTS.fused((a.q_proj.weight, a.k_proj.weight, a.v_proj.weight), x.dtype)
    bqkv = XF.WEIGHTS.fused((a.q_proj.bias, a.k_proj.bias, a.v_proj.bias), torch.float32)
    lns = None if side is None else ((S, size[0], size[0]) if size is not None else (1, 1, 1))
    xs = None if side is None else side.reshape(-1, D).contiguous()
    h1, _, _ = H.layernorm_fwd(x, layer.layer_norm1.weight.detach(), layer.layer_norm1.bias.detach(), B * S, D, x_side=xs, side=lns)
    qkv = H.gemm(h1, Wqkv, B * S, 3 * D, D, epilogue=L.EPI_BIAS_QSCALE, bias=bqkv, scale=64 ** -0.5, scale_cols=D)
    _, stats = H.attn_fwd(qkv, B, S, heads, size=size, pad_mask=pad)
    return H.attn_probs(qkv, stats, B, S, heads, size=size, pad_mask=pad)


def test_bf16_attentions_are_the_kernel_on_the_layers_own_inputs_and_near_the_reference(golden):
    """Teacher-forced, bit for bit: every layer's entry equals hip_ops.attn_probs on the qkv / stats recomputed from the model's own
    hidden_states[i] / hidden_side_rows[i] (pins the layer index, the side rows, the masks, the proxy / frame split).  And the text
    tower against the reference's fp32 attentions: at most LOGITS_VS_REFERENCE_BF16 = 2 x the reference's own bf16-autocast
    deviation (9.6e-3 / 2.3e-2 for layers 0 / 1).  Measured on MI355X: 7.7e-3 / 1.7e-2 (gates 1.9e-2 / 4.6e-2)."""
    model, fx, (video, ids, mask) = _tiny(golden)
    cm = model.clipmodel
    with torch.no_grad():
        to = cm.text_model(input_ids=ids, attention_mask=mask, output_attentions=True, output_hidden_states=True)
        vo = cm.vision_model(pixel_values=video, output_attentions=True, output_hidden_states=True)
        assert len(to.attentions) == len(vo.attentions) == 2 and to.hidden_side_rows is not None and vo.hidden_side_rows is not None
        for i, layer in enumerate(cm.text_model.encoder.layers):
            want = _recomputed(layer, to.hidden_states[i], to.hidden_side_rows[i], 4, 12, None, mask.to(torch.int64).contiguous())
            assert torch.equal(to.attentions[i], want), f"text layer {i}"
        for i, layer in enumerate(cm.vision_model.encoder.layers):
            proxy, frame = _recomputed(layer, vo.hidden_states[i], vo.hidden_side_rows[i], 4, 52, (4, 3, 16), None)
            assert torch.equal(vo.attentions[i].proxy, proxy) and torch.equal(vo.attentions[i].frame, frame), f"video layer {i}"
            assert vo.attentions[i].proxy.dtype == torch.float32 and tuple(vo.attentions[i].frame.shape) == (4, 2, 3, 16, 20)
    ref = golden("tiny_attentions.pt")
    for i, (a, b, dev) in enumerate(zip(to.attentions, ref["text_attentions"], ref["text_attentions_autocast_dev"])):
        d = _dev(f"bf16 text attentions[{i}] vs reference fp32 (reference's own autocast deviation {dev:.2e})", a, b)
        assert d <= LOGITS_VS_REFERENCE_BF16 * dev


def _step(cm, video, ids, mask, **kw):
    from xpretrain_amd.optimization import NCELearnableTempLoss
    for p in cm.parameters():
        p.grad = None
    out = cm(input_ids=ids, pixel_values=video, attention_mask=mask, output_hidden_states=True, **kw)
    loss = NCELearnableTempLoss()(out.image_embeds, out.text_embeds, cm.logit_scale)
    loss.backward()
    torch.cuda.synchronize()
    return out, loss.detach().clone(), {n: p.grad.clone() for n, p in cm.named_parameters()}


def _same_attentions(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, tuple):
            assert torch.equal(x.proxy, y.proxy) and torch.equal(x.frame, y.frame)
        else:
            assert torch.equal(x, y)


def _same_outputs(o1, l1, g1, o0, l0, g0):
    assert torch.equal(l1, l0) and torch.equal(o1.image_embeds, o0.image_embeds) and torch.equal(o1.text_embeds, o0.text_embeds)
    for t1, t0 in ((o1.vision_model_output, o0.vision_model_output), (o1.text_model_output, o0.text_model_output)):
        assert torch.equal(t1.pooler_output, t0.pooler_output) and torch.equal(t1.last_hidden_state, t0.last_hidden_state)
        assert len(t1.hidden_states) == len(t0.hidden_states) and all(torch.equal(a, b) for a, b in zip(t1.hidden_states, t0.hidden_states))
    bad = [n for n in g0 if not torch.equal(g0[n], g1[n])]
    assert not bad, bad[:5]


def test_the_flag_moves_nothing_else_and_the_text_stream_is_joined(golden):
    """train() mode, default settings, CLIPModel.forward (the text tower on its side stream): every other output and every gradient is
    bit-identical with and without the flag; the attentions read on the caller's stream equal those of direct tower calls"""
    model, fx, (video, ids, mask) = _tiny(golden, train=True)
    cm = model.clipmodel
    assert cm.overlap_text_tower and not cm.pooled_last_layer
    o0, l0, g0 = _step(cm, video, ids, mask)
    assert o0.vision_model_output.attentions is None and o0.text_model_output.attentions is None
    o1, l1, g1 = _step(cm, video, ids, mask, output_attentions=True)
    _same_outputs(o1, l1, g1, o0, l0, g0)
    ta, va = o1.text_model_output.attentions, o1.vision_model_output.attentions
    assert len(ta) == len(va) == 2 and not ta[0].requires_grad and not va[0].frame.requires_grad
    _same_attentions(ta, cm.text_model(input_ids=ids, attention_mask=mask, output_attentions=True).attentions)
    _same_attentions(va, cm.vision_model(pixel_values=video, output_attentions=True).attentions)
    assert o1.text_model_output.to_tuple()[-1] is ta
    # the features-only entry points accept the flag and return what they return without it
    assert torch.equal(cm.get_text_features(input_ids=ids, attention_mask=mask, output_attentions=True),
                       cm.get_text_features(input_ids=ids, attention_mask=mask))
    assert torch.equal(cm.get_image_features(pixel_values=video, output_attentions=True), cm.get_image_features(pixel_values=video))


def test_attentions_do_not_depend_on_the_forward_split(monkeypatch):
    """the "tiny" shape and switches of test_forward_as_two_half_batch_chains_is_bit_identical: the weights are computed behind the join
    of the two chains -- a race with the second chain would show as a run-to-run difference"""
    import xpretrain_amd.functional as XF
    from xpretrain_amd.modeling import VidCLIP
    torch.manual_seed(11)
    cfgd = O.hf_config_dict(128, 2, 4, 256, 16, 32, 128, 2, 3, 256, 120, 16, 64)
    model = VidCLIP(ModelArgs(cfgd, 3)).cuda().train()
    video, ids, mask = (t.cuda() for t in O.synthetic_inputs(4, 3, 32, 12, vocab=120))
    cm = model.clipmodel
    monkeypatch.setattr(XF, "FWD_SPLIT_MIN_ROWS", 0)
    made = []
    real = XF.ForwardSplit

    class Spy(real):
        def __init__(self, device):
            made.append(1)
            super().__init__(device)
    monkeypatch.setattr(XF, "ForwardSplit", Spy)

    def run(on, **kw):
        monkeypatch.setattr(XF, "FWD_SPLIT", on)
        out = cm(input_ids=ids, pixel_values=video, attention_mask=mask, **kw)
        torch.cuda.synchronize()
        return out
    base = run(False, output_attentions=True)
    assert not made and len(base.vision_model_output.attentions) == 4
    plain = run(True)
    assert len(made) == 1 and torch.equal(plain.image_embeds, base.image_embeds) and torch.equal(plain.text_embeds, base.text_embeds)
    for rep in range(3):
        out = run(True, output_attentions=True)
        assert len(made) == rep + 2
        _same_attentions(out.vision_model_output.attentions, base.vision_model_output.attentions)
        _same_attentions(out.text_model_output.attentions, base.text_model_output.attentions)
        assert torch.equal(out.image_embeds, plain.image_embeds) and torch.equal(out.text_embeds, plain.text_embeds)


def test_gradient_checkpointing_gives_the_same_attentions_and_gradients(golden):
    model, fx, (video, ids, mask) = _tiny(golden, train=True)
    cm = model.clipmodel
    o0, l0, g0 = _step(cm, video, ids, mask, output_attentions=True)
    cm.gradient_checkpointing_enable()
    assert all(m.gradient_checkpointing for m in cm.modules() if hasattr(m, "gradient_checkpointing"))
    o1, l1, g1 = _step(cm, video, ids, mask, output_attentions=True)
    _same_attentions(o1.text_model_output.attentions, o0.text_model_output.attentions)
    _same_attentions(o1.vision_model_output.attentions, o0.vision_model_output.attentions)
    _same_outputs(o1, l1, g1, o0, l0, g0)


def test_the_flag_keeps_the_pooled_last_layer_dense(golden):
    model, fx, (video, ids, mask) = _tiny(golden)
    cm = model.clipmodel
    cm.pooled_last_layer = True          # (an instance attribute: the class default stays off)
    with torch.no_grad():
        pooled = cm(input_ids=ids, pixel_values=video, attention_mask=mask)
        assert pooled.vision_model_output.last_hidden_state is None          # the switch works on this model ...
        out = cm(input_ids=ids, pixel_values=video, attention_mask=mask, output_attentions=True)
    vo = out.vision_model_output
    assert vo.last_hidden_state is not None and tuple(vo.last_hidden_state.shape) == (4, 52, 128)      # ... and the flag overrides it
    assert len(vo.attentions) == 2 and all(tuple(a.frame.shape) == (4, 2, 3, 16, 20) for a in vo.attentions)
