"""CPU: tests/step_matrix.py is complete, and what it says about every entry -- which switches take part, which yield -- is what the
project's own code does with a CPU model set up that way: overlap_next_forward's attachment, the encoders' checkpointing and hook
state that CLIPEncoder.forward reads before it splits, the reducer's published gradient sinks."""
import contextlib
import itertools

import pytest
import torch

from oracle import clipvip_oracle as O
from tests import step_matrix as M
from tests.gpu_util import ModelArgs


def test_the_table_holds_every_base_single_and_pair():
    assert set(M.BASES) == {"dense", "pooled", "fp32", "dual", "frozen_text"} and len(M.SWITCHES) == len(set(M.SWITCHES)) == 10
    excl = {frozenset(x) for x in M.EXCLUSIVE}
    assert excl == {frozenset(("split_own", "split_side")), frozenset(("dp_pack", "dp_sinks"))}
    assert len(set(M.ALL_ENTRIES)) == len(M.ALL_ENTRIES) == len(M.BASES) * (1 + 10 + 45 - 2)
    for base in M.BASES:
        have = {frozenset(sw) for b, sw in M.ALL_ENTRIES if b == base}
        want = {frozenset()} | {frozenset((s,)) for s in M.SWITCHES}
        want |= {frozenset(p) for p in itertools.combinations(M.SWITCHES, 2) if frozenset(p) not in excl}
        assert have == want, (base, sorted(map(sorted, have ^ want)))
    sizes = [len(sw) for _, sw in M.ALL_ENTRIES]
    assert sizes == sorted(sizes)                       # baselines, then singles, then pairs
    # what is left out of a GPU run is named, and nothing else is missing
    assert set(M.NOT_RUN) <= set(M.ALL_ENTRIES) and M.ENTRIES == [e for e in M.ALL_ENTRIES if e not in M.NOT_RUN]
    assert len({M.entry_id(*e) for e in M.ALL_ENTRIES}) == len(M.ALL_ENTRIES)


def test_the_shapes_meet_the_splits_preconditions():
    """CLIPEncoder.forward: an even batch and a row count that is a multiple of 8; functional._layer_fwd_native: half the rows a
    multiple of 4 -- for the video pass and for the dual base's one-frame image pass.  The tiny shape lies below FWD_SPLIT_MIN_ROWS,
    which a run therefore sets to 0; layer FIRST_LATE lies strictly inside both towers."""
    import xpretrain_amd.functional as XF
    for frames in (None, 1):
        B, Mp, Lp, S, rows = M.geometry(frames)
        assert B % 2 == 0 and rows % 8 == 0 and (rows // 2) % 4 == 0 and Mp >= 1, frames
    assert M.geometry()[3:] == (16, 64) and M.geometry()[4] < XF.FWD_SPLIT_MIN_ROWS
    cfg = O.hf_config_dict(*M.DIMS)
    for tower, key in (("vision", "vision_config"), ("text", "text_config")):
        assert cfg[key]["num_hidden_layers"] == M.LAYERS[tower] > M.FIRST_LATE
    video, ids, mask = O.synthetic_inputs(*M.INPUTS, vocab=M.VOCAB)
    assert video.shape[:2] == (M.geometry()[0], M.TEMPORAL) and ids.shape == mask.shape == (4, 12)


@contextlib.contextmanager
def _one_rank_group(wanted):
    """a one-rank gloo group with the collectives forced on, for the entries that build an active reducer"""
    import torch.distributed as dist
    from xpretrain_amd import distributed as D
    if not wanted:
        yield
        return
    dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    D.FORCE_COLLECTIVES = True
    try:
        yield
    finally:
        D.FORCE_COLLECTIVES = False
        dist.destroy_process_group()


def _observed(base, switches, monkeypatch):
    """the entry's model, optimizer and reducer set up on the CPU as a run sets them up; what the project's code then says"""
    import xpretrain_amd.functional as XF
    from xpretrain_amd import distributed as D
    from xpretrain_amd.modeling import VidCLIP
    from xpretrain_amd.modeling.CLIP_ViP import _has_forward_hooks
    from xpretrain_amd.optimization import AdamW, build_e2e_optimizer_w_lr_mul
    s = set(switches)
    monkeypatch.setattr(XF, "LAYER_CALLS", "op_by_op" not in s)
    model = VidCLIP(ModelArgs(O.hf_config_dict(*M.DIMS), M.TEMPORAL, M.ADD_CLS)).train()
    clip = model.clipmodel
    if base == "pooled":
        clip.pooled_last_layer = True
    if base == "fp32":
        clip.set_compute_dtype(torch.float32)
    if base == "frozen_text":
        model.freeze_text_encoder(True)
    if "ckpt" in s:
        clip.gradient_checkpointing_enable()
    enc = {"vision": clip.vision_model.encoder, "text": clip.text_model.encoder}
    if "hook" in s:
        for e in enc.values():
            e.layers[0].register_forward_hook(lambda module, args, output: None)
    groups = build_e2e_optimizer_w_lr_mul(list(model.named_parameters()), 1e-4, 0.05, lr_mul=1, lr_mul_prefix="")
    opt = AdamW([g for g in groups if g["params"]], lr=1e-4, betas=(0.9, 0.98), skip_nonfinite="guard" in s)
    if "late" in s:
        opt.overlap_next_forward(model, M.FIRST_LATE)
    published = 0
    if s & {"dp_pack", "dp_sinks"}:
        reducer = D.GradBucketReducer(model.parameters(), bucket_mb=0.25, average=True, segments=D.tower_segments(model),
                                      layout_groups=XF.layer_grad_groups(model) if "dp_sinks" in s else None)
        assert reducer._active
        published = len(XF.GRAD_SINKS)
        reducer.remove()
        assert not XF.GRAD_SINKS
    # what CLIPEncoder.forward reads before it builds a ForwardSplit (beside the shape and the device)
    v = enc["vision"]
    ckpt = {n: e.gradient_checkpointing and e.training for n, e in enc.items()}
    hooked = _has_forward_hooks(v.layers)
    wants = bool(s & {"split_own", "split_side"})
    return dict(
        split_stream=next((m for m in ("own", "side") if "split_" + m in s), None),
        split_in_training=wants and XF.LAYER_CALLS and not ckpt["vision"] and not hooked,
        split_in_no_grad=wants and XF.LAYER_CALLS and not hooked,
        native=XF.LAYER_CALLS,
        checkpointed=sorted(n for n, on in ckpt.items() if on),
        pooled_last=bool(clip.pooled_last_layer) and not _has_forward_hooks(v.layers[-1:]),
        late_encoders=sorted(n for n, e in enc.items() if e.late_update is not None and e.late_update.first_layer == M.FIRST_LATE),
        guard=opt.skip_nonfinite,
        sinks_published=published,
    )


@pytest.mark.parametrize("base", M.BASES)
def test_every_entry_takes_part_or_yields_as_the_code_says(base, monkeypatch):
    entries = [sw for b, sw in M.ALL_ENTRIES if b == base]
    with _one_rank_group(True):
        for sw in entries:
            assert _observed(base, sw, monkeypatch) == M.expected(base, sw), M.entry_id(base, sw)
    # the yields the table's docstring names, spelled out once
    e = M.expected(base, ("split_own", "ckpt"))
    assert not e["split_in_training"] and e["split_in_no_grad"]
    assert not M.expected(base, ("split_side", "hook"))["split_in_no_grad"]
    assert not M.expected(base, ("split_side", "op_by_op"))["split_in_no_grad"]
    assert M.expected(base, ("hook",))["pooled_last"] == (base == "pooled")
    assert M.expected(base, ("late",))["late_encoders"] == ["text", "vision"]
    assert M.expected(base, ("ckpt",))["checkpointed"] == (["vision"] if base == "frozen_text" else ["text", "vision"])
