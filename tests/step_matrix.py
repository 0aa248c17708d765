"""The step matrix: the training step's bit-transparent switches, alone and in pairs, as plain data.

Importing this module touches neither the package nor the GPU.  tests/test_step_matrix_cpu.py holds the table complete and checks
what ``expected`` says about each entry against the project's own code, on a CPU model.

BASES are NOT bit-transparent to each other (other kernels or other graphs); each has a baseline of its own:
  dense         bf16, NCELearnableTempLoss
  pooled        clipmodel.pooled_last_layer = True (the last video layer as PooledEncoderLayerFn)
  fp32          clipmodel.set_compute_dtype(torch.float32)
  dual          NCELearnableTempLoss_vsc_fc with image / caption_ids / caption_masks: every layer is applied twice in one graph
  frozen_text   VidCLIP.freeze_text_encoder(True): the text tower in eval mode without gradients

SWITCHES each claim to leave every bit of the step where it was:
  split_own / split_side   the video tower's forward as two half-batch chains (functional.ForwardSplit), the second chain on a torch
                           stream of its own / on the library's weight-gradient stream; FWD_SPLIT_MIN_ROWS = 0 at the tiny shape
  op_by_op                 functional.LAYER_CALLS = False: the layer passes issued op by op instead of by the native calls
  ckpt                     gradient checkpointing: every layer's arena dropped after the forward and rebuilt in the backward
  late                     AdamW.overlap_next_forward(model, 1) on the groups of build_e2e_optimizer_w_lr_mul
  guard                    AdamW(skip_nonfinite=True)
  hook                     a no-op forward hook on encoder layer 0 of both towers
  zero_in_place            zero_grad(set_to_none=False) after every step
  dp_pack / dp_sinks       a one-rank process group with distributed.FORCE_COLLECTIVES: GradBucketReducer(segments=
                           tower_segments(model)) as bench.py builds it, without / with layout_groups (the gradient sinks)

An entry stands for three optimizer steps of the tiny 4-layer model (temporal_size 3) on two seeded batches in the order A, B, A and
one no_grad forward of batch B, with optimization.AdamW stepping WITHOUT a clip.  Such runs compare with torch.equal on every field:
with max_norm <= 0 csrc/optim.hip::clip_coef returns 1.0f whatever the norm is (unguarded: the partials are not even passed; guarded:
the verdict's norm only feeds clip_coef(norm, 0) = 1), and update_kernel then applies adam1 element by element -- no value of the
update depends on how multi_tensor.py partitions the tensors into launches.  The one field whose ARITHMETIC differs between entries
is ``last_grad_norm`` under ``guard``: sqrt(sum of the per-chunk partials), summed thread-strided over the partial array in launch
order (optim.hip::norm_of), and ``late`` moves the late layers' chunks behind the early ones (multi_tensor._build_plan: ``sets``); it
carries the rtol 2e-6 that tests/test_model_gpu.py::_ovl_assert_close documents for the same reordering.

``expected`` states which switches take part in an entry and which YIELD by design:
  * ckpt, hook and op_by_op switch the split off (CLIPEncoder.forward; ckpt only in training passes: a no_grad forward splits);
  * the hook sits on layer 0, so the pooled last layer stays pooled (CLIPEncoder.pools_last looks at the last layer's hooks only);
  * frozen_text: the text encoder is not checkpointed (eval mode) and publishes no gradient sink.  It DOES keep its late record:
    build_e2e_optimizer_w_lr_mul with an empty lr_mul_prefix puts every named parameter into the groups, frozen ones included, and
    overlap_next_forward attaches every encoder with a late parameter among the optimizer's -- the text tower then waits for an
    update that touches none of its weights, which costs an event wait and changes no value.

NOT_RUN names the entries no GPU run may include yet, and why.
"""
import itertools

BASES = ("dense", "pooled", "fp32", "dual", "frozen_text")
SWITCHES = ("split_own", "split_side", "op_by_op", "ckpt", "late", "guard", "hook", "zero_in_place", "dp_pack", "dp_sinks")
EXCLUSIVE = (("split_own", "split_side"), ("dp_pack", "dp_sinks"))       # two values of one switch: they do not pair with each other

STEPS = 3
ORDER = "ABA"
FIRST_LATE = 1
# the tiny 4-layer model of the existing step tests: hf_config_dict arguments, temporal size, synthetic_inputs arguments
DIMS = (128, 2, 4, 256, 16, 32, 128, 2, 4, 256, 120, 16, 64)
TEMPORAL, ADD_CLS, INPUTS, VOCAB = 3, 3, (4, 3, 32, 12), 120
LAYERS = {"vision": 4, "text": 4}

# Entries that faulted on the MI355X and whose cause is not found: a run of dual-split_own+late ended in HIP's "illegal memory
# access" (reported at a later call, so the entry is where it surfaced, not proof of the place).  dual-split_own, dual-split_side
# and dual-late had passed alone, and split_own+late had passed on the dense, pooled and fp32 bases.  Its sibling on the other
# second-chain stream stays out with it.
NOT_RUN = (("dual", ("split_own", "late")), ("dual", ("split_side", "late")))


def geometry(frames=None):
    """(B, M, L, S, rows) of the video tower's stream: M proxy tokens, L patches per frame, S tokens per sample (``frames``: of a
    pass with another frame count, the dual base's one-frame image pass)"""
    B, T, R, _ = INPUTS
    T = T if frames is None else frames
    M, Lp = 1 + ADD_CLS, (R // DIMS[4]) ** 2
    S = M + T * Lp
    return B, M, Lp, S, B * S


def _entries():
    pairs = [p for p in itertools.combinations(SWITCHES, 2) if p not in EXCLUSIVE]
    # parametrize order: every baseline, then every single, then the pairs
    return ([(b, ()) for b in BASES] + [(b, (s,)) for b in BASES for s in SWITCHES] + [(b, p) for b in BASES for p in pairs])


ALL_ENTRIES = _entries()
ENTRIES = [e for e in ALL_ENTRIES if e not in NOT_RUN]          # what a GPU run of the table may include


def entry_id(base, switches):
    return f"{base}-{'+'.join(switches) or 'baseline'}"


def expected(base, switches):
    """Which switches take part in this entry, and which yield where the design says so."""
    s = set(switches)
    assert base in BASES and s <= set(SWITCHES) and not any(set(x) <= s for x in EXCLUSIVE)
    frozen = base == "frozen_text"
    split = next((m for m in ("own", "side") if "split_" + m in s), None)
    late = "late" in s
    return dict(
        split_stream=split,
        split_in_training=split is not None and not (s & {"ckpt", "hook", "op_by_op"}),
        split_in_no_grad=split is not None and not (s & {"hook", "op_by_op"}),
        native="op_by_op" not in s,
        checkpointed=(["vision"] if frozen else ["text", "vision"]) if "ckpt" in s else [],
        pooled_last=base == "pooled",                    # (the hook on layer 0 does not undo it)
        late_encoders=["text", "vision"] if late else [],       # (frozen_text too: see the module docstring)
        guard="guard" in s,
        sinks_published=(LAYERS["vision"] + (0 if frozen else LAYERS["text"])) if "dp_sinks" in s else 0,
    )
