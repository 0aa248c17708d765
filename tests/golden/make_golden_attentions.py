#!/usr/bin/env python
"""Generate tests/golden/tiny_attentions.pt from the UNMODIFIED reference: the attention weights of the text tower of the
``tiny_e2e.pt`` model (``output_attentions=True``).

Run in the build container (where the reference tree exists), beside make_golden.py:

    python tests/golden/make_golden_attentions.py

The reference model is rebuilt from tiny_e2e.pt's own ``config`` / ``state_dict`` (no seeds involved), put in ``eval()``, and its
text tower is called on that fixture's ``ids`` / ``mask``.  Stored (tensors and floats only, tests/gpu_util.py::save_golden):

  text_attentions                 per layer, the reference's fp32 ``attentions`` [B, H, Lt, Lt] (CLIP_ViP.py:303-311)
  text_attentions_autocast_dev    per layer, max |P_autocast - P_fp32| of the same call under torch.autocast("cpu", bfloat16): the
                                  reference's own reduced-precision deviation, the yardstick of the bf16 gate

The video tower has no entry: the reference computes forward2's two softmax matrices and returns None for them
(CLIP_ViP.py:264).  Read by tests/test_attn_probs_cpu.py and tests/test_output_attentions_gpu.py.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402
from tests.gpu_util import load_golden, save_golden  # noqa: E402


def tiny_attentions(ref):
    """the fixture's content (a dict), from the reference modules ``ref`` (ref_import.load())"""
    fx = load_golden("tiny_e2e.pt")
    args = ref_import.make_args(fx["config"], add_cls_num=fx["add_cls_num"], temporal_size=fx["temporal_size"])
    model = ref.VidCLIP.VidCLIP(args)
    model.load_state_dict(fx["state_dict"])
    model.eval()
    text = model.clipmodel.text_model
    with torch.no_grad():
        p32 = text(input_ids=fx["ids"], attention_mask=fx["mask"], output_attentions=True, return_dict=True).attentions
        with torch.autocast("cpu", torch.bfloat16):
            p16 = text(input_ids=fx["ids"], attention_mask=fx["mask"], output_attentions=True, return_dict=True).attentions
        assert model.clipmodel.vision_model(pixel_values=fx["video"], output_attentions=True, return_dict=True).attentions == (None, None)
    assert all(p.dtype == torch.float32 for p in p32)
    return dict(text_attentions=[p.detach().clone() for p in p32],
                text_attentions_autocast_dev=[(a.float() - b).abs().max().item() for a, b in zip(p16, p32)])


if __name__ == "__main__":
    out = tiny_attentions(ref_import.load())
    files = save_golden(out, "tiny_attentions.pt")
    print("tiny_attentions:", [tuple(p.shape) for p in out["text_attentions"]], "autocast dev", out["text_attentions_autocast_dev"],
          "->", [os.path.basename(f) for f in files])
