"""CPU: hidden_act "gelu" (erf GELU through the fused MLP epilogues, XP_EPI_BIAS_GELU_ERF / XP_EPI_GELU_ERF_BWD) -- the model
surface, the planner's treatment of the two new epilogue kinds, and the reference-generated fixture tests/golden/tiny_gelu_e2e.pt
against the oracle with its activation swapped (the GPU side: tests/test_gelu_erf_gpu.py)."""
import ctypes as C
import math

import pytest
import torch

from oracle import clipvip_oracle as O
from tests import gemm_cases as G
from tests.gpu_util import ModelArgs
from tests.test_oracle_golden import TOL, assert_maxrel
from tests.test_planning_cpu import case_budget, case_desc, set_case_env


def erf_gelu(x):
    """transformers' GELUActivation (what the reference builds for "gelu"): 0.5 x (1 + erf(x / sqrt 2))"""
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


# the tiny architecture of tests/golden/tiny_e2e.pt (make_golden.py::TINY)
TINY = dict(vision_hidden=128, vision_heads=2, vision_layers=2, vision_inter=192, patch=8, image=32,
            text_hidden=128, text_heads=2, text_layers=2, text_inter=192, vocab=120, max_pos=16, proj=64)


def tiny_config(vision="quick_gelu", text="quick_gelu"):
    cfgd = O.hf_config_dict(**TINY)
    cfgd["vision_config"]["hidden_act"], cfgd["text_config"]["hidden_act"] = vision, text
    return cfgd


# ---------------------------------------------------------------------------------------------- 1. model surface
def test_model_accepts_gelu_per_tower_and_names_what_it_supports():
    from xpretrain_amd import _lib as L
    from xpretrain_amd.modeling import VidCLIP
    torch.manual_seed(0)
    base = VidCLIP(ModelArgs(tiny_config(), 3))
    shapes = {k: tuple(v.shape) for k, v in base.state_dict().items()}
    nparams = sum(p.numel() for p in base.parameters())
    for vision, text in (("gelu", "quick_gelu"), ("quick_gelu", "gelu"), ("gelu", "gelu")):
        model = VidCLIP(ModelArgs(tiny_config(vision, text), 3))
        assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == shapes, (vision, text)
        assert sum(p.numel() for p in model.parameters()) == nparams
        # the towers choose independently, from their own sub-config
        for tower, name in ((model.clipmodel.vision_model, vision), (model.clipmodel.text_model, text)):
            assert [layer.mlp.act_kind for layer in tower.encoder.layers] == [L.ACTS[name]] * 2, (vision, text)
    assert L.ACTS == {"quick_gelu": 0, "gelu": 1}
    for kw in (dict(vision="relu"), dict(text="gelu_new")):
        with pytest.raises(NotImplementedError) as e:
            VidCLIP(ModelArgs(tiny_config(**kw), 3))
        assert "'quick_gelu'" in str(e.value) and "'gelu'" in str(e.value), str(e.value)


def test_workload_configs_take_hidden_act():
    from xpretrain_amd import workload as W
    assert W.vit_b_config() == O.vit_b_config()                                   # the default is unchanged
    cfgd = W.vit_b_config(hidden_act="gelu")
    assert cfgd["vision_config"]["hidden_act"] == cfgd["text_config"]["hidden_act"] == "gelu"
    cfgd = W.hf_config_dict(**TINY, hidden_act=("gelu", "quick_gelu"))
    assert (cfgd["vision_config"]["hidden_act"], cfgd["text_config"]["hidden_act"]) == ("gelu", "quick_gelu")


# ---------------------------------------------------------------------------------------------- 2. plan equality
_GELU_CASES = [c for c in G.CASES if c["epi"] in ("gelu", "gelu_bwd")]


def _plan_info(d):
    from xpretrain_amd import _lib as L
    info = L.XpGemmPlanInfo()
    L.check(L.lib().xp_debug_gemm_plan(C.byref(d), C.byref(info)), "xp_debug_gemm_plan")
    return bytes(info)


@pytest.mark.parametrize("c", _GELU_CASES, ids=[c["id"] for c in _GELU_CASES])
def test_erf_kinds_plan_as_their_quick_counterparts(c, monkeypatch):
    """kind 8 plans as kind 3 and kind 9 as kind 5 for every GELU case of the table: the whole XpGemmPlanInfo (family, epilogue
    implementation, tile height, split, grid, column-sum rows), the tile rows, the column-sum rows and both auto splits"""
    from xpretrain_amd import _lib as L
    lib = L.lib()
    assert len(_GELU_CASES) > 40
    erf = {L.EPI_BIAS_GELU: L.EPI_BIAS_GELU_ERF, L.EPI_GELU_BWD: L.EPI_GELU_ERF_BWD}
    assert (L.EPI_BIAS_GELU, L.EPI_GELU_BWD, L.EPI_SCALE, L.EPI_BIAS_GELU_ERF, L.EPI_GELU_ERF_BWD) == (3, 5, 7, 8, 9)
    set_case_env(c, monkeypatch)
    with case_budget(c):
        quick, other = case_desc(c), case_desc(c)
        other.epilogue = erf[quick.epilogue]
        assert _plan_info(other) == _plan_info(quick)
        for query in (lib.xp_gemm_tile_rows, lib.xp_gemm_colsum_rows, lib.xp_gemm_auto_split, lib.xp_gemm_auto_split_slack):
            assert query(C.byref(other)) == query(C.byref(quick)), query.__name__
    if c["colsum"]:
        assert L.lib().xp_gemm_colsum_rows(C.byref(other)) > 0


def test_layer_dims_carry_the_activation():
    """XpLayerDims.act: zero-initialised = quick_gelu; the ctypes mirror has the C layout (int32 after ln_eps, 8-byte aligned
    size); the workspace queries answer the same for both activations (the erf kinds plan as their quick counterparts)"""
    from xpretrain_amd import _lib as L
    assert L.XpLayerDims.act.offset == L.XpLayerDims.ln_eps.offset + 4 and C.sizeof(L.XpLayerDims) == 96
    assert L.XpLayerDims().act == L.ACT_QUICK_GELU
    lib = L.lib()
    sizes = []
    for act in (L.ACT_QUICK_GELU, L.ACT_GELU):
        d = L.XpLayerDims()
        d.rows, d.D, d.Dff, d.B, d.S, d.heads, d.M, d.N, d.L = 8 * 2356, 768, 3072, 8, 2356, 12, 4, 12, 196
        d.attn_mode, d.dtype, d.q_scale, d.ln_eps, d.act = L.ATTN_PROXY, L.XP_BF16, 0.125, 1e-5, act
        sizes.append(tuple(int(f(C.byref(d))) for f in (lib.xp_encoder_layer_fwd_workspace_bytes, lib.xp_encoder_layer_bwd_workspace_bytes,
                                                        lib.xp_encoder_layer_pooled_fwd_workspace_bytes,
                                                        lib.xp_encoder_layer_pooled_bwd_workspace_bytes)))
    assert sizes[0] == sizes[1] and all(s > 0 for s in sizes[0])


# ---------------------------------------------------------------------------------------------- 3. fixture sanity
def _cfg(fx):
    return O.OracleCfg.from_hf_dict(fx["config"], add_cls_num=fx["add_cls_num"], temporal_size=fx["temporal_size"])


def test_fixture_holds_tensors_and_the_config_only(golden):
    fx, quick = golden("tiny_gelu_e2e.pt"), golden("tiny_e2e.pt")
    assert quick["config"] == tiny_config() and fx["config"] == tiny_config("gelu", "gelu")
    assert fx["config"]["vision_config"]["hidden_act"] == fx["config"]["text_config"]["hidden_act"] == "gelu"
    assert fx.keys() == quick.keys()

    def leaves(v):
        if isinstance(v, dict):
            return [x for u in v.values() for x in leaves(u)]
        return [x for u in v for x in leaves(u)] if isinstance(v, (list, tuple)) else [v]
    for k, v in fx.items():
        if k != "config":
            assert all(isinstance(x, (torch.Tensor, int)) for x in leaves(v)), k
    # the same recipe: weights and inputs are tiny_e2e.pt's, the outputs are not
    assert all(torch.equal(fx["state_dict"][k], quick["state_dict"][k]) for k in quick["state_dict"])
    assert all(torch.equal(fx[k], quick[k]) for k in ("video", "ids", "mask"))
    assert (fx["vis_features"] - quick["vis_features"]).abs().max() > 1e-3


def test_oracle_with_erf_gelu_reproduces_the_fixture(golden, monkeypatch):
    """the yardstick of the GPU tests: the oracle with its module-level ``quick_gelu`` rebound to erf GELU against the reference's
    "gelu" model -- hidden states, features, loss and every gradient, at test_oracle_golden.py's gates for tiny_e2e.pt"""
    fx = golden("tiny_gelu_e2e.pt")
    cfg = _cfg(fx)
    monkeypatch.setattr(O, "quick_gelu", erf_gelu)
    sd = O.strip_prefix(fx["state_dict"])
    vh, th = [], []
    vlast, vpool = O.vision_tower(fx["video"], sd, cfg, collect=vh)
    for ours, ref in zip(vh[1:], fx["vision_hidden"]):
        torch.testing.assert_close(ours, ref, **TOL)
    torch.testing.assert_close(vlast, fx["vision_last"], **TOL)
    torch.testing.assert_close(vpool, fx["vision_pooled"], **TOL)
    tlast, tpool = O.text_tower(fx["ids"], fx["mask"], sd, cfg, collect=th)
    for ours, ref in zip(th, fx["text_hidden"]):
        torch.testing.assert_close(ours, ref, **TOL)
    torch.testing.assert_close(tlast, fx["text_last"], **TOL)
    torch.testing.assert_close(tpool, fx["text_pooled"], **TOL)
    sd = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
    loss, vis, txt = O.full_step(fx["video"], fx["ids"], fx["mask"], sd, cfg)
    torch.testing.assert_close(vis, fx["vis_features"], **TOL)
    torch.testing.assert_close(txt, fx["text_features"], **TOL)
    torch.testing.assert_close(loss, fx["loss"], rtol=1e-5, atol=1e-5)
    loss.backward()
    assert len(fx["grads"]) > 50
    for name, g in fx["grads"].items():
        ours = sd[name[len("clipmodel."):]].grad
        assert ours is not None, name
        assert_maxrel(ours, g, 2e-4, name)
