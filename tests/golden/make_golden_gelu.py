#!/usr/bin/env python
"""Generate tests/golden/tiny_gelu_e2e.pt from the UNMODIFIED reference: make_golden.py::tiny_e2e with ``hidden_act = "gelu"`` in
both sub-configs (the reference then builds transformers' GELUActivation, the erf form, per tower: CLIP_ViP.py:388).

Run in the build container (where the reference tree exists), beside make_golden.py:

    python tests/golden/make_golden_gelu.py

Same recipe as tiny_e2e -- the ``TINY`` sizes, seeds, ``randomize_``, inputs and stored fields are make_golden.py's own -- so the
two fixtures differ in the activation only.  Tensors and the config dict, nothing else, go into the file (pieces of <= 1000 KiB,
tests/gpu_util.py::save_golden).  Read by tests/test_gelu_erf_cpu.py and tests/test_gelu_erf_gpu.py.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden import TINY, randomize_  # noqa: E402
from oracle import ref_import  # noqa: E402
from oracle import clipvip_oracle as O  # noqa: E402
from tests.gpu_util import save_golden  # noqa: E402


def tiny_gelu_e2e(ref):
    torch.manual_seed(1234)
    cfg_dict = O.hf_config_dict(**TINY)
    cfg_dict["vision_config"]["hidden_act"] = cfg_dict["text_config"]["hidden_act"] = "gelu"
    args = ref_import.make_args(cfg_dict, add_cls_num=3, temporal_size=3)
    model = ref.VidCLIP.VidCLIP(args)
    for tower in (model.clipmodel.vision_model, model.clipmodel.text_model):
        act = tower.encoder.layers[0].mlp.activation_fn
        assert type(act).__name__ == "GELUActivation", type(act)
    randomize_(model, 99)
    model.train()
    B, T, Lt = 4, 3, 12
    video, ids, mask = O.synthetic_inputs(B, T, TINY["image"], Lt, vocab=TINY["vocab"], seed=4321)
    # one row with EOT in the very last slot and one with the earliest legal EOT
    ids[0, 2:] = TINY["vocab"] - 1; mask[0] = 0; mask[0, :3] = 1
    ids[1, 1:-1] = torch.randint(1, TINY["vocab"] - 2, (Lt - 2,)); ids[1, -1] = TINY["vocab"] - 1; mask[1] = 1
    out = model(video, ids, mask)
    loss = ref.loss.NCELearnableTempLoss(None)(out["vis_features"], out["text_features"], model.clipmodel.logit_scale)
    loss.backward()
    with torch.no_grad():
        vo = model.clipmodel.vision_model(pixel_values=video, output_hidden_states=True, return_dict=True)
        to = model.clipmodel.text_model(input_ids=ids, attention_mask=mask, output_hidden_states=True, return_dict=True)
    fx = dict(
        config=cfg_dict, add_cls_num=3, temporal_size=3,
        state_dict={k: v.detach().clone() for k, v in model.state_dict().items()},
        video=video, ids=ids, mask=mask,
        vis_features=out["vis_features"].detach(), text_features=out["text_features"].detach(),
        loss=loss.detach(),
        grads={n: p.grad.detach().clone() for n, p in model.named_parameters()},
        vision_hidden=[h.detach() for h in vo.hidden_states], vision_last=vo.last_hidden_state.detach(),
        vision_pooled=vo.pooler_output.detach(),
        text_hidden=[h.detach() for h in to.hidden_states], text_last=to.last_hidden_state.detach(),
        text_pooled=to.pooler_output.detach(),
    )
    files = save_golden(fx, "tiny_gelu_e2e.pt")
    print("tiny_gelu_e2e: loss", float(loss), "params", sum(p.numel() for p in model.parameters()), "->", len(files), "file(s)")


if __name__ == "__main__":
    tiny_gelu_e2e(ref_import.load())
