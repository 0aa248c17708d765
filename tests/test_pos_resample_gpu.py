"""GPU: xp_pos_resample_fwd / _bwd, functional.PosResampleFn, the ``interpolate_pos_encoding`` switch of the model classes and
``load_state_dict_with_mismatch(resize_embeddings=True)`` against the fp64 definition of tests/pos_resample_ref.py (which
tests/test_pos_resample_cpu.py holds against torch's float64 ``F.interpolate`` and transformers' ``interpolate_pos_encoding``).

The kernel gate is not a fixed number: for every case the largest deviation of torch's OWN float32 ``F.interpolate`` (forward) and of
its float32 autograd (backward) from the fp64 definition is computed on the CPU on the same inputs, and the kernel must stay within
4 x that -- room for another, equally valid fp32 summation order over at most 16 taps forward and a few dozen terms backward.  Where
torch's deviation is exactly 0 (7 -> 1 x 1: the one destination row sits on a source row) so must the kernel's be."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import clipvip_oracle as O
from tests import pos_resample_ref as R
from tests.gpu_util import OUT, TOL, ModelArgs, seeded_model
from tests.guarded import Guarded

pytestmark = pytest.mark.gpu

# the tiny configuration of tests/golden/make_golden.py
TINY = dict(vision_hidden=128, vision_heads=2, vision_layers=2, vision_inter=192, patch=8, image=32,
            text_hidden=128, text_heads=2, text_layers=2, text_inter=192, vocab=120, max_pos=16, proj=64)
POS = "clipmodel.vision_model.embeddings.position_embedding.weight"
TEMPORAL = "clipmodel.vision_model.embeddings.temporal_embedding"


def _torch_resample(pos, gh, gw):
    g0, D = R.grid_of(pos.shape[0]), pos.shape[1]
    grid = F.interpolate(pos[1:].view(1, g0, g0, D).permute(0, 3, 1, 2), size=(gh, gw), mode="bicubic", align_corners=False)
    return torch.cat([pos[:1], grid.permute(0, 2, 3, 1).reshape(gh * gw, D)])


def _gates(pos, cot, gh, gw):
    """(fp64 forward, fp64 transpose, forward gate, backward gate) of fp32 CPU tensors pos / cot: the gates are 4 x the deviation of
    torch's own float32 forward / autograd backward from the fp64 definition"""
    g0 = R.grid_of(pos.shape[0])
    ref_f, ref_b = R.forward(pos.numpy(), gh, gw), R.transpose(cot.numpy(), g0, gh, gw)
    p = pos.clone().requires_grad_()
    out = _torch_resample(p, gh, gw)
    out.backward(cot)
    dev_f = float(np.abs(out.detach().double().numpy() - ref_f).max())
    dev_b = float(np.abs(p.grad.double().numpy() - ref_b).max())
    return ref_f, ref_b, 4.0 * dev_f, 4.0 * dev_b


@functools.lru_cache(maxsize=None)
def _case(g0, gh, gw, D):
    """inputs, fp64 references and gates of one kernel case, computed once"""
    g = torch.Generator().manual_seed(1000 * g0 + 37 * gh + gw)
    pos = 0.02 * torch.randn(1 + g0 * g0, D, generator=g)
    cot = torch.randn(1 + gh * gw, D, generator=g)
    return (pos, cot) + _gates(pos, cot, gh, gw)


def _log(line):
    print(line)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "pos_resample_errors.txt"), "a") as f:
        f.write(line + "\n")


# ------------------------------------------------------------------------------------------------ kernel against the definition
@pytest.mark.parametrize("g0,gh,gw,D", R.KERNEL_CASES)
def test_kernel_forward_and_backward_against_fp64(g0, gh, gw, D):
    from xpretrain_amd import hip_ops as H
    pos, cot, ref_f, ref_b, gate_f, gate_b = _case(g0, gh, gw, D)
    out = H.pos_resample_fwd(pos.cuda(), gh, gw).cpu()
    d_pos = H.pos_resample_bwd(cot.cuda(), g0, gh, gw).cpu()
    assert out.shape == (1 + gh * gw, D) and d_pos.shape == (1 + g0 * g0, D)
    assert torch.isfinite(out).all() and torch.isfinite(d_pos).all()
    e_f = float(np.abs(out.double().numpy() - ref_f).max())
    e_b = float(np.abs(d_pos.double().numpy() - ref_b).max())
    _log(f"{g0} -> {gh} x {gw}, D {D}: forward |kernel - fp64| {e_f:.2e} (gate {gate_f:.2e} = 4 x torch fp32's {gate_f / 4:.2e}); "
         f"backward {e_b:.2e} (gate {gate_b:.2e} = 4 x torch fp32's {gate_b / 4:.2e})")
    assert torch.equal(out[0], pos[0]) and torch.equal(d_pos[0], cot[0])          # row 0: bit for bit, both ways
    assert e_f <= gate_f and e_b <= gate_b


# ------------------------------------------------------------------------------------------------ kernel contract
def test_two_calls_and_a_side_stream_give_the_same_bits():
    from xpretrain_amd import hip_ops as H
    for g0, gh, gw, D in [(7, 10, 13, 192), (14, 28, 28, 768)]:
        pos, cot = (t.cuda() for t in _case(g0, gh, gw, D)[:2])
        a, da = H.pos_resample_fwd(pos, gh, gw), H.pos_resample_bwd(cot, g0, gh, gw)
        b, db = H.pos_resample_fwd(pos, gh, gw), H.pos_resample_bwd(cot, g0, gh, gw)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            c, dc = H.pos_resample_fwd(pos, gh, gw), H.pos_resample_bwd(cot, g0, gh, gw)
        s.synchronize()
        assert torch.equal(a, b) and torch.equal(a, c)
        assert torch.equal(da, db) and torch.equal(da, dc)


@pytest.mark.parametrize("g0,gh,gw,D", [(7, 3, 5, 64), (7, 10, 13, 192), (2, 5, 3, 64), (7, 1, 1, 64)])
def test_outputs_between_poisoned_guards(g0, gh, gw, D):
    """(rows x D / 4 threads: 16 x 16, 131 x 48, 16 x 16 and 2 x 16 forward -- none a multiple of the 256-thread block but the first)"""
    from xpretrain_amd import hip_ops as H
    pos, cot, ref_f, ref_b, gate_f, gate_b = _case(g0, gh, gw, D)
    out, d_pos = Guarded(1 + gh * gw, D, torch.float32), Guarded(1 + g0 * g0, D, torch.float32)
    H.pos_resample_fwd(pos.cuda(), gh, gw, out=out.mat)
    H.pos_resample_bwd(cot.cuda(), g0, gh, gw, d_pos=d_pos.mat)
    torch.cuda.synchronize()
    out.check("pos_resample_fwd", 1 + gh * gw, D)
    d_pos.check("pos_resample_bwd", 1 + g0 * g0, D)
    assert torch.isfinite(out.mat).all() and torch.isfinite(d_pos.mat).all()          # ... and every element inside was written
    assert float(np.abs(out.mat.cpu().double().numpy() - ref_f).max()) <= gate_f
    assert float(np.abs(d_pos.mat.cpu().double().numpy() - ref_b).max()) <= gate_b


def test_bad_arguments_are_refused_without_a_launch():
    from xpretrain_amd import _lib as L
    lib = L.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    src = torch.zeros(1 + 49, 64, device="cuda")
    dst = Guarded(1 + 49, 64, torch.float32)
    ps, pd = C.c_void_p(src.data_ptr()), C.c_void_p(dst.mat.data_ptr())
    bad = [((ps, pd, 0, 7, 7, 64), "g0=0"), ((ps, pd, 7, 0, 7, 64), "gh=0"), ((ps, pd, 7, 7, -1, 64), "gw=-1"),
           ((ps, pd, 7, 7, 7, 0), "D=0"), ((ps, pd, 7, 7, 7, 62), "D=62"), ((ps, pd, 7, 7, 7, -4), "D=-4"),
           ((C.c_void_p(0), pd, 7, 7, 7, 64), "null"), ((ps, C.c_void_p(0), 7, 7, 7, 64), "null"),
           ((C.c_void_p(src.data_ptr() + 4), pd, 7, 7, 7, 60), "aligned")]
    for fn in ("xp_pos_resample_fwd", "xp_pos_resample_bwd"):
        for args, word in bad:
            rc = getattr(lib, fn)(*args, st)
            msg = lib.xp_last_error().decode()
            assert rc == -1 and fn in msg and word in msg, (fn, args[2:], rc, msg)
    torch.cuda.synchronize()
    dst.check("refused calls", 0, 0)                                                   # nothing was written anywhere
    from xpretrain_amd import hip_ops as H
    with pytest.raises(ValueError, match="square"):
        H.pos_resample_fwd(torch.zeros(18, 64, device="cuda"), 3, 3)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        H.pos_resample_fwd(torch.zeros(17, 6, device="cuda"), 3, 3)


def test_autograd_function_returns_the_parameters_shape():
    from xpretrain_amd import functional as XF
    pos, cot, ref_f, ref_b, gate_f, gate_b = _case(7, 10, 13, 192)
    w = pos.cuda().requires_grad_()
    out = XF.pos_table(w, 10, 13)
    out.backward(cot.cuda())
    assert out.shape == (131, 192) and w.grad.shape == w.shape
    assert float(np.abs(w.grad.cpu().double().numpy() - ref_b).max()) <= gate_b
    assert XF.pos_table(w, 7, 7) is w


# ------------------------------------------------------------------------------------------------ model
def _inputs(h=32, w=32, B=2, T=3):
    g = torch.Generator().manual_seed(4321)
    video = torch.randn(B, T, 3, h, w, generator=g)
    _, ids, mask = O.synthetic_inputs(B, T, 32, 12, vocab=TINY["vocab"])
    return video.cuda(), ids.cuda(), mask.cuda()


def _model(dtype=torch.bfloat16, **over):
    model = seeded_model(O.hf_config_dict(**{**TINY, **over}), 3).cuda().train()
    model.clipmodel.set_compute_dtype(dtype)
    return model


def _step(model, video, ids, mask, flag, **kw):
    """one training step through CLIPModel.forward; (outputs, loss, gradients by name)"""
    from xpretrain_amd.optimization import NCELearnableTempLoss
    cm = model.clipmodel
    for p in model.parameters():
        p.grad = None
    out = cm(input_ids=ids, pixel_values=video, attention_mask=mask, interpolate_pos_encoding=flag, **kw)
    loss = NCELearnableTempLoss()(out.image_embeds, out.text_embeds, cm.logit_scale)
    loss.backward()
    torch.cuda.synchronize()
    return out, loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def test_native_grid_with_the_flag_is_the_flag_off_step():
    model = _model()
    video, ids, mask = _inputs()
    o0, l0, g0 = _step(model, video, ids, mask, False)
    o1, l1, g1 = _step(model, video, ids, mask, True)
    assert torch.equal(o0.image_embeds, o1.image_embeds) and torch.equal(o0.text_embeds, o1.text_embeds) and torch.equal(l0, l1)
    assert sorted(g0) == sorted(g1) and POS in g0
    assert not [n for n in g0 if not torch.equal(g0[n], g1[n])]


def test_off_grid_frames_without_the_flag_are_still_refused():
    model = _model()
    video, ids, mask = _inputs(48, 40)
    with pytest.raises(ValueError, match="position_embedding has 17 rows but the frame has 30 patches"):
        model(video, ids, mask)
    with pytest.raises(ValueError, match="position_embedding has 17 rows"):
        model.clipmodel.get_image_features(pixel_values=video)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_flag_on_equals_a_model_that_holds_the_resampled_table(dtype):
    """48 x 40 frames (grid 6 x 5) with the flag on, against a second model with the same weights whose position_embedding IS the
    kernel's [31, 128] output, flag off: features, hidden states and loss bit-equal; every gradient but the table's bit-equal; the
    table's gradient is the transpose of the second model's table gradient (rows 1..16 within the kernel's backward gate on exactly
    these inputs, row 0 within 4 float32 ulps of its largest magnitude)."""
    from xpretrain_amd import hip_ops as H
    a = _model(dtype)
    video, ids, mask = _inputs(48, 40)
    table = H.pos_resample_fwd(a.state_dict()[POS].detach().contiguous(), 6, 5)
    b = _model(dtype)                                          # the same seeds: the same weights
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    emb = torch.nn.Embedding(31, 128).cuda()
    with torch.no_grad():
        emb.weight.copy_(table)
    b.clipmodel.vision_model.embeddings.position_embedding = emb
    oa, la, ga = _step(a, video, ids, mask, True, output_hidden_states=True)
    ob, lb, gb = _step(b, video, ids, mask, False, output_hidden_states=True)
    assert torch.equal(oa.image_embeds, ob.image_embeds) and torch.equal(oa.text_embeds, ob.text_embeds) and torch.equal(la, lb)
    ha, hb = oa.vision_model_output.hidden_states, ob.vision_model_output.hidden_states
    assert len(ha) == len(hb) == 3 and ha[0].shape == (2, 4 + 3 * 30, 128)
    assert all(torch.equal(x, y) for x, y in zip(ha, hb))
    assert sorted(ga) == sorted(gb)
    assert not [n for n in ga if n != POS and not torch.equal(ga[n], gb[n])]
    got, d_table = ga[POS].cpu(), gb[POS].cpu()
    assert got.shape == (17, 128) and d_table.shape == (31, 128)
    _, ref_b, _, gate_b = _gates(a.state_dict()[POS].detach().cpu(), d_table, 6, 5)
    scale = float(np.abs(ref_b).max())
    err = float(np.abs(got[1:].double().numpy() - ref_b[1:]).max())
    m0 = d_table[0].abs().max()
    ulp = (torch.nextafter(m0, torch.tensor(float("inf"))) - m0).item()
    d0 = (got[0] - d_table[0]).abs().max().item()
    _log(f"model {dtype}: table gradient rows 1..16 rel. error {err / scale:.2e} (gate {gate_b / scale:.2e}); row 0 |d| {d0:.2e} "
         f"(4 ulp = {4 * ulp:.2e})")
    assert err / scale <= gate_b / scale
    assert d0 <= 4 * ulp


def test_flag_on_composes_with_vidclip_checkpointing_and_the_pooled_last_layer():
    from xpretrain_amd.modeling import VidCLIP
    model = _model()
    cm = model.clipmodel
    video, ids, mask = _inputs(48, 40)
    o, l, g = _step(model, video, ids, mask, True)
    # VidCLIP.forward / forward_video with the config key
    args = ModelArgs(O.hf_config_dict(**TINY), 3)
    args.clip_vision_additional_config["interpolate_pos_encoding"] = 1
    keyed = VidCLIP(args).cuda().train()
    keyed.load_state_dict(model.state_dict())
    out = keyed(video, ids, mask)
    assert torch.equal(out["vis_features"], o.image_embeds) and torch.equal(out["text_features"], o.text_embeds)
    with torch.no_grad():
        assert torch.equal(keyed.forward_video(video), cm.get_image_features(pixel_values=video, if_norm=True, interpolate_pos_encoding=True))
        img = keyed(video, ids, mask, image=video[:, :1], caption_ids=ids[:, None], caption_masks=mask[:, None])
    assert img["img_features"].shape == (2, 64) and torch.isfinite(img["img_features"]).all()
    # gradient checkpointing: the same bits
    cm.gradient_checkpointing_enable()
    try:
        o2, l2, g2 = _step(model, video, ids, mask, True)
    finally:
        cm.gradient_checkpointing_disable()
    assert torch.equal(o2.image_embeds, o.image_embeds) and torch.equal(l2, l)
    assert not [n for n in g if not torch.equal(g[n], g2[n])]
    # the pooled last layer: the same function through other kernels (tests/test_pooled_last_layer_gpu.py's feature gate)
    cm.pooled_last_layer = True
    try:
        o3, l3, g3 = _step(model, video, ids, mask, True)
    finally:
        cm.pooled_last_layer = False
    assert o3.vision_model_output.last_hidden_state is None
    d = (o3.image_embeds - o.image_embeds).abs().max().item()
    print(f"flag on, pooled last layer vs dense: max|d| = {d:.2e}")
    assert d <= TOL["features_abs_full"] and g3[POS].shape == (17, 128)
    # decoded uint8 frames and output_attentions take the off-grid frames as well
    with torch.no_grad():
        u8 = cm(input_ids=ids, pixel_values=torch.randint(0, 256, (2, 3, 3, 48, 40), dtype=torch.uint8, device="cuda"),
                attention_mask=mask, interpolate_pos_encoding=True, output_attentions=True)
    assert torch.isfinite(u8.image_embeds).all()
    w = u8.vision_model_output.attentions
    assert len(w) == 2 and w[0].proxy.shape == (2, 2, 4, 94) and w[0].frame.shape == (2, 2, 3, 30, 34)


def test_loader_resamples_both_tables_once():
    """a 4 x 4 / temporal_size 3 state dict into a model built for image 48 (6 x 6) / temporal_size 5"""
    from xpretrain_amd import hip_ops as H
    from xpretrain_amd.utils.load_save import load_state_dict_with_mismatch
    src = seeded_model(O.hf_config_dict(**TINY), 3).state_dict()
    dst = seeded_model(O.hf_config_dict(**{**TINY, "image": 48}), 5, seed=77, perturb_seed=78)
    rep = load_state_dict_with_mismatch(dst, src, resize_embeddings=True)
    assert rep["resized"] == [POS, TEMPORAL]
    assert rep["mismatched"] == ["clipmodel.vision_model.embeddings.position_ids"]
    assert rep["missing"] == [] and rep["unexpected"] == []
    got = dst.state_dict()
    assert got[POS].device.type == "cpu" and got[POS].shape == (37, 128)
    assert torch.equal(got[POS], H.pos_resample_fwd(src[POS].cuda(), 6, 6).cpu())
    assert torch.equal(got[TEMPORAL], F.interpolate(src[TEMPORAL].transpose(1, 2), size=5, mode="linear").transpose(1, 2))
    for name, t in src.items():
        if name not in rep["resized"] and name not in rep["mismatched"]:
            assert torch.equal(got[name], t), name
    assert torch.equal(got["clipmodel.vision_model.embeddings.position_ids"], torch.arange(37)[None])
