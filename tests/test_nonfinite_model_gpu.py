"""GPU: a NaN / Inf born inside the step reaches the gradient norm, so the device-side guard skips the update; and at inference one
corrupt sample leaves the other samples' features bit for bit where they were.

The tiny model and inputs of tests/step_matrix.py on the bases dense, pooled (which also runs the listed-tile last-layer backward)
and fp32, each alone with its default switches, through configs.setup_training(..., skip_nonfinite_steps=1) as
tests/test_guarded_step_gpu.py::training_run sets it up.  No tolerance: non-finite, or torch.equal."""
import pytest
import torch

from oracle import clipvip_oracle as O
from tests import step_matrix as M
from tests.gpu_util import ModelArgs

pytestmark = pytest.mark.gpu
BASES = ("dense", "pooled", "fp32")
NAN, INF = float("nan"), float("inf")


def _model(base):
    from xpretrain_amd.modeling import VidCLIP
    torch.manual_seed(11)
    model = VidCLIP(ModelArgs(O.hf_config_dict(*M.DIMS), M.TEMPORAL, M.ADD_CLS))
    with torch.no_grad():
        model.clipmodel.vision_model.embeddings.temporal_embedding.normal_(0, 0.1)
    model.cuda().train()
    if base == "pooled":
        model.clipmodel.pooled_last_layer = True
    if base == "fp32":
        model.clipmodel.set_compute_dtype(torch.float32)
    return model


def _inputs():
    return [t.cuda() for t in O.synthetic_inputs(*M.INPUTS, vocab=M.VOCAB)]


def _pixel(video, value):
    """one pixel of sample 1's second frame"""
    video = video.clone()
    video[1, 1, 2, 17, 5] = value
    return video


def _weight(model, where):
    layers = model.clipmodel.vision_model.encoder.layers
    return layers[0].mlp.fc1.weight if where == "fc1_first" else layers[-1].mlp.fc2.weight


# name -> (what to do to (model, video) before the planted step)
def _plant_pixel(value):
    return lambda model, video: _pixel(video, value)


def _plant_weight(where):
    def f(model, video):
        with torch.no_grad():
            _weight(model, where).view(-1)[131] = NAN
        return video
    return f


def _plant_scale(model, video):
    with torch.no_grad():
        model.clipmodel.logit_scale.fill_(INF)
    return video


TRAIN_PLANTS = {
    "pixel-nan": _plant_pixel(NAN), "pixel-inf": _plant_pixel(INF), "fc1-first-layer-nan": _plant_weight("fc1_first"),
    "fc2-last-layer-nan": _plant_weight("fc2_last"), "logit-scale-inf": _plant_scale,
}


def _bits(t):
    return t.detach().contiguous().view(-1).view(torch.uint8).clone()


def _state(model, opt):
    """the bits of every parameter and of every optimizer state tensor, and the step counts"""
    out = {}
    for n, p in model.named_parameters():
        out["p:" + n] = _bits(p)
        for k, v in opt.state[p].items():
            out[f"{k}:{n}"] = _bits(v) if torch.is_tensor(v) else v
    return out


@pytest.mark.parametrize("plant", list(TRAIN_PLANTS))
@pytest.mark.parametrize("base", BASES)
def test_a_value_born_inside_the_step_reaches_the_guard(base, plant):
    """one clean step (so that the optimizer has state), then the planted one: the loss and the gradient norm are non-finite, the step
    is skipped, and no bit of any parameter or optimizer state moves"""
    from xpretrain_amd import configs as CF
    model = _model(base)
    cfg = CF.load_config(dict(optim="adamw", learning_rate=1e-4, weight_decay=0.05, lr_mul=1, lr_mul_prefix="", betas=[0.9, 0.98],
                              loss_config={"loss_name": "NCELearnableTempLoss", "if_gather": 0}, decay="linear", warmup_ratio=0.25,
                              grad_norm=0.05, skip_nonfinite_steps=1))
    tr = CF.setup_training(cfg, model, 8)
    opt = tr.optimizer
    assert opt.skip_nonfinite
    video, ids, mask = _inputs()

    def step(k, video):
        for g in opt.param_groups:
            g["lr"] = tr.lr_at(k + 1)
        out = model(video, ids, mask)
        loss = tr.loss_fn(out["vis_features"], out["text_features"], model.clipmodel.logit_scale)
        loss.backward()
        opt.clip_and_step(tr.grad_norm)
        opt.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        return loss.detach()
    loss = step(0, video)
    assert torch.isfinite(loss) and torch.isfinite(opt.last_grad_norm) and opt.skipped_steps == 0
    video = TRAIN_PLANTS[plant](model, video)
    before = _state(model, opt)
    loss = step(1, video)
    print(f"{base} {plant}: loss {loss.item()} grad norm {float(opt.last_grad_norm)} skipped {opt.skipped_steps}")
    assert not torch.isfinite(loss), "the loss swallowed the planted value"
    assert not torch.isfinite(opt.last_grad_norm), "the gradient norm swallowed the planted value"
    assert opt.skipped_steps == 1 and opt.last_step_skipped
    after = _state(model, opt)
    moved = [k for k in before if not (torch.equal(before[k], after[k]) if torch.is_tensor(before[k]) else before[k] == after[k])]
    assert before.keys() == after.keys() and not moved, f"a skipped step changed {moved[:5]}"


def _features(model, video, ids, mask):
    with torch.no_grad():
        out = model(video, ids, mask)
    torch.cuda.synchronize()
    return out["vis_features"].float().cpu(), out["text_features"].float().cpu()


@pytest.mark.parametrize("split", ["default", "forced"])
@pytest.mark.parametrize("base", BASES)
def test_one_corrupt_sample_does_not_poison_the_batch(base, split, monkeypatch):
    """under no_grad: NaN in one pixel of sample 1, then in the embedding row of a token id that only sample 2's text uses -- the
    planted sample's feature row is non-finite, every other feature row of both towers is torch.equal to the clean batch's; with the
    video tower's forward split at its default and forced on (FWD_SPLIT_MIN_ROWS = 0: two half-batch chains)"""
    import xpretrain_amd.functional as XF
    if split == "forced":
        monkeypatch.setattr(XF, "FWD_SPLIT_MIN_ROWS", 0)
    model = _model(base).eval()
    video, ids, mask = _inputs()
    B = video.shape[0]
    # the token at position 1 of sample 2: attended, before the pooled position, and no other sample's text uses its id
    only2 = int(ids[2, 1])
    assert int(mask[2, 1]) == 1 and (ids == only2).any(1).tolist() == [False, False, True, False]
    vis0, txt0 = _features(model, video, ids, mask)
    assert torch.isfinite(vis0).all() and torch.isfinite(txt0).all()
    bad = []

    def judge(tag, vis, txt, vis_row, txt_row):
        for name, got, clean, row in (("vis", vis, vis0, vis_row), ("txt", txt, txt0, txt_row)):
            for b in range(B):
                if b == row:
                    if torch.isfinite(got[b]).any():
                        bad.append(f"{tag}: {name}[{b}] has finite elements (swallowed)")
                elif not torch.equal(got[b], clean[b]):
                    bad.append(f"{tag}: {name}[{b}] moved (leaked)" + ("" if torch.isfinite(got[b]).all() else ", non-finite"))
    judge("pixel of sample 1", *_features(model, _pixel(video, NAN), ids, mask), 1, None)
    tok = model.clipmodel.text_model.embeddings.token_embedding.weight
    with torch.no_grad():
        tok[only2, 3] = NAN
    judge("token row of sample 2", *_features(model, video, ids, mask), None, 2)
    assert not bad, "\n".join(bad)
