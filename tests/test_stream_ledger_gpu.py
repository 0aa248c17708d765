"""GPU: the stream ledger (tests/stream_ledger.py) of the training step's cross-stream switches -- every launch with its stream and
pointers, every observed order edge and every allocator event of three optimizer steps (A, B, A) and one no_grad forward of the tiny
model of tests/step_matrix.py, replayed against R1 (lifetime), R2 (order: the concurrent classes equal the committed table) and R3
(nothing unseen).  Unlike a bit-equality test it does not depend on timing: a missing wait or a block handed back too early is in
the ledger whether or not the kernels happened to overlap.  Two planted, benign hazards show that the recorder sees the real
allocator and real streams.  No entry of step_matrix.NOT_RUN is run."""
import contextlib
import os

import pytest
import torch

from oracle import clipvip_oracle as O
from tests import step_matrix as M
from tests import stream_ledger as SL
from tests.gpu_util import ModelArgs, dump

pytestmark = pytest.mark.gpu

_SPLITS = ((), ("split_own",), ("split_side",), ("late",))
ENTRIES = ([(base, sw) for base in ("dense", "dual") for sw in _SPLITS]
           + [("dense", ("split_own", "late")), ("dense", ("split_side", "late")), ("pooled", ("split_own",)), ("dense", ("dp_sinks",))])


def test_no_entry_is_one_that_may_not_run():
    assert len(set(ENTRIES)) == len(ENTRIES) == 12
    for e in ENTRIES:
        assert e in M.ENTRIES and e not in M.NOT_RUN, e
    assert not {M.entry_id(*e) for e in ENTRIES} & {M.entry_id(*e) for e in M.NOT_RUN}


@contextlib.contextmanager
def _one_rank_group(wanted):
    """a one-rank group with the collectives forced on, as tests/test_distributed_gpu.py runs the reducer on one GPU"""
    import torch.distributed as dist
    from xpretrain_amd import distributed as D
    if not wanted:
        yield
        return
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", store=dist.HashStore(), rank=0, world_size=1)
    D.FORCE_COLLECTIVES = True
    try:
        yield
    finally:
        D.FORCE_COLLECTIVES = False
        dist.destroy_process_group()


def _batches(dual):
    out = []
    for seed in (4321, 1234):                      # A, B
        video, ids, mask = O.synthetic_inputs(*M.INPUTS, vocab=M.VOCAB, seed=seed)
        b = dict(video=video.cuda(), text_input_ids=ids.cuda(), text_input_mask=mask.cuda())
        if dual:
            _, cap_ids, cap_mask = O.synthetic_inputs(M.INPUTS[0], 1, M.INPUTS[2], M.INPUTS[3], vocab=M.VOCAB, seed=seed + 1)
            b.update(image=video[:, 1:2].contiguous().cuda(), caption_ids=cap_ids[:, None].cuda(), caption_masks=cap_mask[:, None].cuda())
        out.append(b)
    return out


def _run(base, switches, monkeypatch, rec):
    """the entry's model, optimizer and reducer set up as tests/test_step_matrix_cpu.py::_observed sets them up, then the schedule"""
    import xpretrain_amd.functional as XF
    from xpretrain_amd import distributed as D
    from xpretrain_amd import hip_ops as H
    from xpretrain_amd.modeling import VidCLIP
    from xpretrain_amd.optimization import AdamW, build_e2e_optimizer_w_lr_mul, build_loss_func
    s, dual = set(switches), base == "dual"
    monkeypatch.setattr(H, "_ws_cache", {})                    # (scratch buffers from before the recording are blocks nobody saw)
    monkeypatch.setattr(XF, "_SPLIT_STREAMS", {})
    if s & {"split_own", "split_side"}:
        monkeypatch.setattr(XF, "FWD_SPLIT", True)
        monkeypatch.setattr(XF, "FWD_SPLIT_MIN_ROWS", 0)
        monkeypatch.setattr(XF, "FWD_SPLIT_STREAM", "own" if "split_own" in s else "side")
    torch.manual_seed(11)
    model = VidCLIP(ModelArgs(O.hf_config_dict(*M.DIMS), M.TEMPORAL, M.ADD_CLS)).cuda().train()
    if base == "pooled":
        model.clipmodel.pooled_last_layer = True
    groups = build_e2e_optimizer_w_lr_mul(list(model.named_parameters()), 1e-4, 0.05, lr_mul=1, lr_mul_prefix="")
    opt = AdamW([g for g in groups if g["params"]], lr=1e-4, betas=(0.9, 0.98))
    rec.watch(opt)
    if "late" in s:
        opt.overlap_next_forward(model, M.FIRST_LATE)
    reducer = None
    if "dp_sinks" in s:
        reducer = D.GradBucketReducer(model.parameters(), bucket_mb=0.25, average=True, segments=D.tower_segments(model),
                                      layout_groups=XF.layer_grad_groups(model))
        assert reducer._active and len(XF.GRAD_SINKS) == M.expected(base, switches)["sinks_published"]
    loss_fn = build_loss_func({"loss_name": "NCELearnableTempLoss_vsc_fc" if dual else "NCELearnableTempLoss"})
    batches = dict(zip("AB", _batches(dual)))
    made = []
    real = XF.ForwardSplit

    class Spy(real):
        def __init__(self, device):
            made.append(torch.is_grad_enabled())
            super().__init__(device)
    monkeypatch.setattr(XF, "ForwardSplit", Spy)
    for which in M.ORDER:
        out = model(**batches[which])
        feats = [out[k] for k in (("vis_features", "text_features", "img_features", "cap_features") if dual
                                  else ("vis_features", "text_features"))]
        if reducer is not None:
            feats = list(D.gather_features(*feats))
        loss_fn(*feats, model.clipmodel.logit_scale).backward()
        if reducer is not None:
            reducer.synchronize()
        opt.step()
        reducer.zero_grad() if reducer is not None else opt.zero_grad(set_to_none=True)
    with torch.no_grad():
        model(**batches["B"])
    torch.cuda.synchronize()
    if reducer is not None:
        reducer.remove()
    # the streams the entry's switches put work on, by role (torch hands out streams from a pool of 32 per process, so in a long
    # process two roles may share one handle: the ledger is keyed by handle, as the hardware is)
    streams = dict(text=model.clipmodel.shared_text_stream(torch.device("cuda")).cuda_stream)
    streams.update({f"second_chain_{i}": st.cuda_stream for i, st in XF._SPLIT_STREAMS.items()})
    if opt._late_update is not None:
        streams.update({f"late_{d}": st.cuda_stream for d, st in opt._late_update.streams.items()})
    return made, streams


@pytest.mark.parametrize("base, switches", ENTRIES, ids=[M.entry_id(*e) for e in ENTRIES])
def test_the_entrys_ledger_holds_lifetime_order_and_nothing_unseen(base, switches, monkeypatch):
    assert (base, switches) not in M.NOT_RUN
    exp = M.expected(base, switches)
    caller = torch.cuda.current_stream().cuda_stream
    with _one_rank_group("dp_sinks" in switches):
        rec = SL.Recorder().start()                 # before the model is built: every block of the run is in the trace
        try:
            made, roles = _run(base, switches, monkeypatch, rec)
        finally:
            events, initial = rec.stop()
    rep = SL.check(events, initial, known_streams=(caller,))
    summary = dict(entry=M.entry_id(base, switches), sources=rec.sources, splits_made=len(made), roles=roles, **SL.summary(rep))
    dump(f"stream_ledger_{M.entry_id(base, switches)}.json", summary)
    bad = SL.verdict(rep, concurrent=SL.applicable(split=exp["split_in_training"]))
    print(f"{summary['entry']}: streams {summary['streams']} launches {rep['n_launches']} blocks {rep['n_blocks']} frees {rep['n_frees']} "
          f"classes {len(rep['classes'])} R1 {len(rep['violations'])} unresolved {len(rep['unresolved'])} "
          f"unseen {len(rep['unseen_streams'])}; free events from {rec.sources['free_from']}")
    for line in bad[:60]:
        print("  " + line)
    # the recorder saw the run: the allocator's frees, launches on the caller's stream and on the text tower's, and the second chain
    # exactly where the table says the entry splits (three training passes -- two forward passes each on the dual base -- and the
    # no_grad forward)
    assert rec.sources["actions"].get("alloc") and rec.sources["actions"].get(rec.sources["free_from"]) and rep["n_frees"] > 100
    assert rep["streams"][caller] > 100 and all(rep["streams"][h] >= 3 for h in roles.values()), (roles, rep["streams"])
    assert set(roles) == ({"text"} | ({"second_chain_0"} if exp["split_in_training"] else set())
                          | ({"late_" + str(torch.device("cuda", 0))} if exp["late_encoders"] else set())), roles
    passes = 2 if base == "dual" else 1
    assert made == ([True] * passes * M.STEPS + [False] * passes if exp["split_in_training"] else [])
    assert not bad, f"{len(bad)} findings, the first: {bad[0]}"


@pytest.mark.parametrize("recorded", [False, True], ids=["plant1_no_record_stream", "plant2_record_stream"])
def test_a_planted_cross_stream_read_of_a_dropped_tensor_is_seen(recorded):
    """An xp_cast on a second stream reads a tensor that was allocated on the caller's stream and is then dropped with no wait:
    without record_stream the ledger must report R1 (the block is back in the caller's pool while the second stream may still read
    it), with record_stream it must be clean.  Benign: the block returns to torch's pool, not to the driver, and the test
    synchronises before anything else allocates; no kernel is altered."""
    from xpretrain_amd import hip_ops as H
    caller = torch.cuda.current_stream()
    second = torch.cuda.Stream()
    rec = SL.Recorder().start()
    try:
        src = torch.ones(1 << 16, device="cuda")
        dst = torch.empty(1 << 16, dtype=torch.bfloat16, device="cuda")
        src_addr = src.data_ptr()
        second.wait_stream(caller)                  # the read is behind the fill: only the LIFETIME is at stake
        with torch.cuda.stream(second):
            H.cast(src, torch.bfloat16, out=dst)
        if recorded:
            src.record_stream(second)
        del src                                     # no wait, no hold
        torch.cuda.synchronize()
        ok = bool((dst.float() == 1).all())
    finally:
        events, initial = rec.stop()
    rep = SL.check(events, initial, known_streams=(caller.cuda_stream,))
    dump(f"stream_ledger_plant{1 + recorded}.json", dict(sources=rec.sources, **SL.summary(rep)))
    bad = SL.verdict(rep, concurrent={})
    print(bad)
    assert ok and rep["n_launches"] == 1 and rep["streams"] == {second.cuda_stream: 1}
    assert not rep["unresolved"] and not rep["unseen_streams"] and not rep["classes"]
    if recorded:
        assert bad == []
    else:
        assert len(bad) == 1 and bad[0].startswith("R1:") and "xp_cast:src" in bad[0]
        (v,) = rep["violations"]
        assert v["block"][0] == src_addr and v["alloc_stream"] == caller.cuda_stream and v["launch"]["stream"] == second.cuda_stream
        assert v["frame"] is not None and "test_stream_ledger_gpu.py" in v["frame"]
