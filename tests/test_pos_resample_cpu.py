"""CPU: the fp64 definition of the position-table resample (tests/pos_resample_ref.py) against torch's float64 ``F.interpolate``, its
autograd and transformers' ``interpolate_pos_encoding``; and the surface of the feature: the keyword on the five forward methods, the
VidCLIP config key, the refusal of a table that is no square grid, the two C-ABI symbols, the loader's default report."""
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import clipvip_oracle as O
from tests import pos_resample_ref as R
from tests.gpu_util import ModelArgs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(vision_hidden=128, vision_heads=2, vision_layers=2, vision_inter=192, patch=8, image=32,
            text_hidden=128, text_heads=2, text_layers=2, text_inter=192, vocab=120, max_pos=16, proj=64)


def _torch_resample(pos: torch.Tensor, gh: int, gw: int) -> torch.Tensor:
    g0, D = R.grid_of(pos.shape[0]), pos.shape[1]
    grid = F.interpolate(pos[1:].view(1, g0, g0, D).permute(0, 3, 1, 2), size=(gh, gw), mode="bicubic", align_corners=False)
    return torch.cat([pos[:1], grid.permute(0, 2, 3, 1).reshape(gh * gw, D)])


@pytest.mark.parametrize("g0,gh,gw", R.GRIDS)
def test_definition_equals_torch_float64_forward_and_autograd(g0, gh, gw):
    g = torch.Generator().manual_seed(100 * g0 + 10 * gh + gw)
    D = 12
    pos = (0.02 * torch.randn(1 + g0 * g0, D, generator=g, dtype=torch.float64)).requires_grad_()
    cot = torch.randn(1 + gh * gw, D, generator=g, dtype=torch.float64)
    want = _torch_resample(pos, gh, gw)
    want.backward(cot)
    got = R.forward(pos.detach().numpy(), gh, gw)
    d_fwd = float(np.abs(got - want.detach().numpy()).max())
    got_t = R.transpose(cot.numpy(), g0, gh, gw)
    d_bwd = float(np.abs(got_t - pos.grad.numpy()).max())
    print(f"{g0} -> {gh} x {gw}: |definition - torch fp64| forward {d_fwd:.1e}, transpose {d_bwd:.1e}")
    assert d_fwd <= 1e-12 and d_bwd <= 1e-12
    assert np.array_equal(got[0], pos.detach().numpy()[0]) and np.array_equal(got_t[0], cot.numpy()[0])      # row 0 untouched


@pytest.mark.parametrize("gh,gw", [(10, 13), (14, 14)])
def test_definition_equals_transformers_interpolate_pos_encoding(gh, gw):
    pytest.importorskip("transformers")
    from transformers.models.clip.configuration_clip import CLIPVisionConfig
    from transformers.models.clip.modeling_clip import CLIPVisionEmbeddings
    P, D = 4, 16
    emb = CLIPVisionEmbeddings(CLIPVisionConfig(hidden_size=D, image_size=7 * P, patch_size=P, num_hidden_layers=1,
                                                num_attention_heads=2, intermediate_size=32)).double()
    with torch.no_grad():
        emb.position_embedding.weight.normal_(0, 0.02, generator=torch.Generator().manual_seed(3))
        want = emb.interpolate_pos_encoding(torch.zeros(1, 1 + gh * gw, D, dtype=torch.float64), gh * P, gw * P)[0]
    got = R.forward(emb.position_embedding.weight.detach().numpy(), gh, gw)
    assert want.shape == (1 + gh * gw, D)
    assert float(np.abs(got - want.numpy()).max()) <= 1e-12


def test_axis_matrix_rows_sum_to_one_and_identity_is_exact():
    """(the outer weights' Horner steps pass through 8 |A| = 6: a dozen fp64 roundings of values up to 6 are 12 * 6 * 2^-53 < 1e-14)"""
    for g0, gh, gw in R.GRIDS:
        for g in (gh, gw):
            assert np.abs(R.axis_matrix(g0, g).sum(1) - 1.0).max() <= 1e-14
    assert np.array_equal(R.axis_matrix(7, 7), np.eye(7))


# ------------------------------------------------------------------------------------------------ surface
def test_keyword_exists_on_the_five_methods_and_defaults_to_false():
    from xpretrain_amd.modeling import CLIP_ViP as M
    for fn in (M.CLIPVisionViPEmbeddings.forward, M.CLIPVisionTransformer.forward, M.CLIPVisionModel.forward, M.CLIPModel.forward,
               M.CLIPModel.get_image_features):
        p = inspect.signature(fn).parameters
        assert "interpolate_pos_encoding" in p, fn.__qualname__
        assert p["interpolate_pos_encoding"].default is False, fn.__qualname__


def test_vidclip_reads_the_config_key():
    from xpretrain_amd.modeling import VidCLIP
    cfgd = O.hf_config_dict(**TINY)
    assert VidCLIP(ModelArgs(cfgd, 3)).interpolate_pos_encoding is False
    args = ModelArgs(cfgd, 3)
    args.clip_vision_additional_config["interpolate_pos_encoding"] = 1
    assert VidCLIP(args).interpolate_pos_encoding is True
    args.clip_vision_additional_config["interpolate_pos_encoding"] = 0
    assert VidCLIP(args).interpolate_pos_encoding is False


def test_table_that_is_no_square_grid_raises_value_error():
    from xpretrain_amd import functional as XF
    from xpretrain_amd import hip_ops as H
    assert H.pos_grid(17) == 4 and H.pos_grid(2) == 1 and H.pos_grid(785) == 28
    for rows in (18, 16, 1, 0, 3):
        with pytest.raises(ValueError, match="square"):
            H.pos_grid(rows)
    with pytest.raises(ValueError, match="square"):
        XF.pos_table(torch.zeros(18, 64), 3, 3)
    with pytest.raises(ValueError, match="smaller than one patch"):
        XF.pos_table(torch.zeros(17, 64), 0, 3)
    w = torch.zeros(17, 64, requires_grad=True)
    assert XF.pos_table(w, 4, 4) is w                  # the table's own grid: the parameter itself, no node


def test_resample_of_a_cpu_table_is_refused():
    from xpretrain_amd import functional as XF
    with pytest.raises(RuntimeError, match="no CPU path"):
        XF.pos_table(torch.zeros(17, 64), 6, 5)


def test_symbols_are_in_the_header_and_in_the_binding():
    from xpretrain_amd import _lib
    src = open(os.path.join(ROOT, "include", "xpretrain_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("xp_pos_resample_fwd", "xp_pos_resample_bwd"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in _lib.SIGNATURES
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.i32 and args == [_lib.vp, _lib.vp, _lib.i32, _lib.i32, _lib.i32, _lib.i32, _lib.vp]


def test_loader_without_the_option_reports_todays_three_keys():
    from xpretrain_amd.modeling import VidCLIP
    from xpretrain_amd.utils.load_save import load_state_dict_with_mismatch
    assert inspect.signature(load_state_dict_with_mismatch).parameters["resize_embeddings"].default is False
    torch.manual_seed(0)
    src = VidCLIP(ModelArgs(O.hf_config_dict(**TINY), 3))
    dst = VidCLIP(ModelArgs(O.hf_config_dict(**{**TINY, "image": 48}), 3))
    before = dst.clipmodel.vision_model.embeddings.position_embedding.weight.detach().clone()
    rep = load_state_dict_with_mismatch(dst, src.state_dict())
    assert sorted(rep) == ["mismatched", "missing", "unexpected"]
    assert rep["mismatched"] == ["clipmodel.vision_model.embeddings.position_embedding.weight",
                                 "clipmodel.vision_model.embeddings.position_ids"]
    assert rep["missing"] == [] and rep["unexpected"] == []
    assert torch.equal(dst.clipmodel.vision_model.embeddings.position_embedding.weight, before)


def test_loader_resizes_the_temporal_table_and_needs_a_gpu_for_the_position_table():
    """the temporal table's conversion is the model's own linear expression and runs anywhere; the position table's runs the HIP kernel"""
    from xpretrain_amd.modeling import VidCLIP
    from xpretrain_amd.utils.load_save import load_state_dict_with_mismatch
    torch.manual_seed(0)
    src = VidCLIP(ModelArgs(O.hf_config_dict(**TINY), 3))
    with torch.no_grad():
        src.clipmodel.vision_model.embeddings.temporal_embedding.normal_(0, 0.02)
    dst = VidCLIP(ModelArgs(O.hf_config_dict(**TINY), 5))
    rep = load_state_dict_with_mismatch(dst, src.state_dict(), resize_embeddings=True)
    name = "clipmodel.vision_model.embeddings.temporal_embedding"
    assert rep["resized"] == [name] and rep["mismatched"] == []
    te = src.clipmodel.vision_model.embeddings.temporal_embedding.detach()
    want = F.interpolate(te.transpose(1, 2), size=5, mode="linear").transpose(1, 2)
    assert torch.equal(dst.clipmodel.vision_model.embeddings.temporal_embedding.detach(), want)
    if not torch.cuda.is_available():
        big = VidCLIP(ModelArgs(O.hf_config_dict(**{**TINY, "image": 48}), 3))
        with pytest.raises(RuntimeError, match="no CPU path"):
            load_state_dict_with_mismatch(big, src.state_dict(), resize_embeddings=True)
