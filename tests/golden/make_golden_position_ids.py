#!/usr/bin/env python
"""Generate tests/golden/text_position_ids.pt from the UNMODIFIED reference: its text tower called with custom ``position_ids``.

Run in the build container (where the reference tree exists), beside make_golden.py:

    python tests/golden/make_golden_position_ids.py

The model is the tiny CLIP-ViP of tiny_e2e.pt's shape (make_golden.py::TINY: text tower 128 wide -- the attention kernels are built
for head_dim 64 -- 2 layers, 2 heads, vocab 120, max_position_embeddings 16).  Its weights are rebuilt from seeds by this
repository's own model class (tests/gpu_util.py::seeded_model, as the full-size fixtures do) and loaded into the reference, so the
fixture holds no state dict: ``CONFIG`` / ``TEMPORAL_SIZE`` below plus a fingerprint of the weights (tensors and floats) that the
tests hold their own rebuild to.  The reference model is in ``eval()``, fp32, on the CPU.

Cases (``CASES``; B = 4): position ids as the reference's ``CLIPTextEmbeddings.forward`` (CLIP_ViP.py:210-227) takes them --
  offset     [1, 12]  t + 3: a shifted map shared by every sample
  reversed   [12]     11 - t: a permuted map, one-dimensional
  left_pad   [4, 12]  per sample: p_b padding columns in front (attention_mask 0, position 0), then 0, 1, 2, ...
  long       [1, 24]  Lt = 24 > max_position_embeddings = 16: min(t, 15), every id inside the table
Per case, from ONE call of ``get_text_features(input_ids, attention_mask, position_ids, output_hidden_states=True)``:
  ids, mask (or None), position_ids            the inputs
  text_features                                what get_text_features returns (text_projection of the pooled row)
  pooler_output, last_hidden_state             the text tower's outputs inside that call (a forward hook on text_model)
  embeds                                       hidden_states[0]: the embedding stage's output, tok[ids] + pos[position_ids]
  c_pool, c_last                               the fixed cotangents: loss = <pooler_output, c_pool> + <last_hidden_state, c_last>
  d_embeds                                     d loss / d embeds
  d_tok, d_pos                                 d loss / d token_embedding.weight, d loss / d position_embedding.weight
Read by tests/test_text_position_cpu.py and tests/test_text_position_gpu.py.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402
from oracle import clipvip_oracle as O  # noqa: E402
from tests.gpu_util import save_golden, seeded_model, weight_fingerprint  # noqa: E402

CONFIG = dict(vision_hidden=128, vision_heads=2, vision_layers=2, vision_inter=192, patch=8, image=32,
              text_hidden=128, text_heads=2, text_layers=2, text_inter=192, vocab=120, max_pos=16, proj=64)
TEMPORAL_SIZE = 3
B = 4


def _ids(Lt, seed):
    _, ids, mask = O.synthetic_inputs(B, 1, 8, Lt, vocab=CONFIG["vocab"], seed=seed)
    return ids, mask


def _left_padded(ids, mask):
    """every sample's kept tokens moved to the right end, pad token 0 in front; positions count from the first kept token"""
    Lt = ids.shape[1]
    out_ids, out_mask, pos = torch.zeros_like(ids), torch.zeros_like(mask), torch.zeros_like(ids)
    for b in range(ids.shape[0]):
        n = int(mask[b].sum())
        out_ids[b, Lt - n:], out_mask[b, Lt - n:] = ids[b, :n], 1
        pos[b, Lt - n:] = torch.arange(n)
    return out_ids, out_mask, pos


def cases():
    """name -> (ids [B, Lt], attention_mask or None, position_ids)"""
    i0, m0 = _ids(12, 11)
    i1, m1 = _ids(12, 12)
    i2, m2, p2 = _left_padded(*_ids(12, 13))
    i3, m3 = _ids(24, 14)
    return {"offset": (i0, m0, (torch.arange(12) + 3)[None]),
            "reversed": (i1, None, torch.arange(11, -1, -1)),
            "left_pad": (i2, m2, p2),
            "long": (i3, m3, torch.arange(24).clamp(max=15)[None])}


def cotangents(name, Lt, D):
    g = torch.Generator().manual_seed(500 + sorted(cases()).index(name))
    return torch.randn(B, D, generator=g), torch.randn(B, Lt, D, generator=g)


def position_id_cases(ref):
    cfgd = O.hf_config_dict(**CONFIG)
    ours = seeded_model(cfgd, TEMPORAL_SIZE)
    model = ref.VidCLIP.VidCLIP(ref_import.make_args(cfgd, add_cls_num=3, temporal_size=TEMPORAL_SIZE))
    model.load_state_dict(ours.state_dict(), strict=True)
    model.eval()
    clip = model.clipmodel
    emb = clip.text_model.embeddings
    seen = []
    hook = clip.text_model.register_forward_hook(lambda mod, args, out: seen.append(out))
    fx = dict(fingerprint=weight_fingerprint(ours.state_dict()), cases={})
    for name, (ids, mask, pos_ids) in cases().items():
        clip.zero_grad()
        del seen[:]
        feats = clip.get_text_features(input_ids=ids, attention_mask=mask, position_ids=pos_ids, output_hidden_states=True,
                                       return_dict=True)
        (out,) = seen
        embeds = out.hidden_states[0]
        embeds.retain_grad()
        c_pool, c_last = cotangents(name, ids.shape[1], CONFIG["text_hidden"])
        ((out.pooler_output * c_pool).sum() + (out.last_hidden_state * c_last).sum()).backward()
        fx["cases"][name] = dict(
            ids=ids, mask=mask, position_ids=pos_ids, text_features=feats.detach().clone(),
            pooler_output=out.pooler_output.detach().clone(), last_hidden_state=out.last_hidden_state.detach().clone(),
            embeds=embeds.detach().clone(), c_pool=c_pool, c_last=c_last, d_embeds=embeds.grad.detach().clone(),
            d_tok=emb.token_embedding.weight.grad.detach().clone(), d_pos=emb.position_embedding.weight.grad.detach().clone())
    hook.remove()
    return fx


if __name__ == "__main__":
    out = position_id_cases(ref_import.load())
    files = save_golden(out, "text_position_ids.pt")
    print("text_position_ids:", {k: tuple(v["last_hidden_state"].shape) for k, v in out["cases"].items()}, "->",
          [(os.path.basename(f), os.path.getsize(f)) for f in files])
