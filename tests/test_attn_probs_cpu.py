"""CPU: the fp64 restatements of the attention weights (tests/attn_probs_ref.py) against the oracle's attention cores and the
reference's own ``attentions`` (tests/golden/tiny_attentions.pt), the fixture against its generator where the reference tree is
present, and the C ABI of xp_attn_probs (header, binding, exported symbol)."""
import ctypes
import os
import re

import pytest
import torch

from oracle import clipvip_oracle as O
from oracle import ref_import
from tests import attn_probs_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _qkv(B, h, S, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, h, S, 64, dtype=torch.float64, generator=g) for _ in range(3)]


@pytest.mark.parametrize("size", [(1, 3, 5), (4, 2, 49), (20, 3, 7)])
def test_proxy_weights_times_v_equal_the_oracle_core(size):
    M, N, L = size
    q, k, v = _qkv(2, 2, M + N * L, seed=M + N + L)
    proxy, frame = R.proxy_probs(q, k, size)
    assert proxy.shape == (2, 2, M, M + N * L) and frame.shape == (2, 2, N, L, M + L)
    assert (R.proxy_pv(proxy, frame, v, size) - O.proxy_attention_core(q, k, v, size)).abs().max().item() <= 1e-12
    assert (proxy.sum(-1) - 1).abs().max().item() <= 1e-12 and (frame.sum(-1) - 1).abs().max().item() <= 1e-12


@pytest.mark.parametrize("mode", ["none", "ragged", "allpad"])
def test_causal_weights_times_v_equal_the_oracle_core(mode):
    B, S = 3, 12
    q, k, v = _qkv(B, 2, S, seed=S)
    mask = None
    if mode != "none":
        mask = (torch.arange(S)[None] < torch.tensor([S, 3, 7])[:, None]).long()
        if mode == "allpad":
            mask[1] = 0
    p = R.causal_probs(q, k, mask)
    assert (R.causal_pv(p, v) - O.masked_attention_core(q, k, v, mask)).abs().max().item() <= 1e-12
    assert torch.equal(p.triu(1), torch.zeros_like(p))
    if mask is not None:        # a padded key of a row that sees a kept key: exactly 0; a row of padded keys only: uniform
        sees_kept = (mask[:, None, :].expand(B, S, S).tril().sum(-1) > 0)[:, None, :, None]
        padded = (mask == 0)[:, None, None, :]
        assert torch.equal(p[(sees_kept & padded).expand_as(p)], torch.zeros((sees_kept & padded).expand_as(p).sum().item(), dtype=p.dtype))
    if mode == "allpad":
        want = (1.0 / torch.arange(1, S + 1, dtype=torch.float64))[:, None].expand(S, S).tril()
        assert (p[1] - want).abs().max().item() <= 1e-12


def test_layer_restatement_reproduces_the_reference_attentions(golden):
    """LayerNorm 1 -> q, k -> causal weights in fp64 from tiny_e2e.pt's text_hidden[i] against the reference's fp32 attentions:
    6.9e-7 measured (the reference side is fp32), gate 5e-6"""
    fx, att = golden("tiny_e2e.pt"), golden("tiny_attentions.pt")
    sd = O.strip_prefix(fx["state_dict"])
    heads = fx["config"]["text_config"]["num_attention_heads"]
    assert len(att["text_attentions"]) == fx["config"]["text_config"]["num_hidden_layers"] == len(att["text_attentions_autocast_dev"])
    for i, ref in enumerate(att["text_attentions"]):
        assert ref.dtype == torch.float32 and tuple(ref.shape) == (4, heads, 12, 12)
        assert torch.equal(ref.triu(1), torch.zeros_like(ref))
        p = R.layer_probs(fx["text_hidden"][i], sd, f"text_model.encoder.layers.{i}.", heads, pad_mask=fx["mask"])
        d = (p - ref.double()).abs().max().item()
        print(f"text layer {i}: max |fp64 restatement - reference attentions| = {d:.2e}")
        assert d <= 5e-6
    assert int(fx["mask"][0].sum()) == 3        # sample 0 keeps 3 keys: its padded columns are exactly 0 in rows >= 0
    assert torch.equal(att["text_attentions"][0][0, :, :, 3:], torch.zeros(heads, 12, 9))


@pytest.mark.skipif(not ref_import.available(), reason="the reference tree is not on this machine")
def test_generator_reproduces_the_committed_fixture(golden):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_attentions", os.path.join(ROOT, "tests", "golden", "make_golden_attentions.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    new, old = gen.tiny_attentions(ref_import.load()), golden("tiny_attentions.pt")
    assert sorted(new) == sorted(old)
    for a, b in zip(new["text_attentions"], old["text_attentions"]):
        assert torch.equal(a, b)
    assert new["text_attentions_autocast_dev"] == old["text_attentions_autocast_dev"]


def test_header_binding_and_symbol_of_xp_attn_probs_agree():
    from xpretrain_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xpretrain_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+xp_attn_probs\s*\(([^)]*)\)\s*;", src)
    assert m, "include/xpretrain_hip.h does not declare xp_attn_probs"
    ctype = {"const void*": _lib.vp, "const float*": _lib.vp, "const int64_t*": _lib.vp, "float*": _lib.vp, "void*": _lib.vp,
             "int64_t": _lib.i64, "int32_t": _lib.i32}
    args = [ctype[re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*")] for a in m.group(1).split(",")]
    res, bound = _lib.SIGNATURES["xp_attn_probs"]
    assert res is _lib.i32 and bound == args
    assert "XP_ABI_VERSION 1" in src
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "xp_attn_probs")
