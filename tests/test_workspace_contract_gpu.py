"""GPU: every kernel that takes a workspace runs with EXACTLY the bytes its ``*_workspace_bytes`` function reports, inside guards,
with the scratch poisoned -- the contract include/xpretrain_hip.h and INTEGRATION.md give C callers, which the ordinary allocator
(never fewer than 1 MiB, grow-only per tag) hides from every other test.

Each case runs twice on identical inputs: under the ordinary allocator, then under tests/guarded.py::GuardedWorkspaces (a fresh,
exact-size, 0x7FA5-filled buffer per request).  Asserted: (a) every output is bit-identical (None matches None); (b) no guard
changed (a write past the reported size, a region carved larger than reported, the attention workspace -- the LAST region of the
layer backward's arena -- overrun); (c) no output of the guarded run holds a NaN the ordinary run lacks (scratch read before it
is written).

Words of scratch that are read before the launch that uses them writes them -- counters, flags, accumulate-into-scratch -- found
by reading every kernel's use of its workspace (before this file first ran on a device):
  * csrc/attention.hip, attn_bwd5_kernel / attn_bwd6_kernel: the 4-byte problem counter at the plan's ``counter`` region (the end
    of the backward workspace), taken with atomicAdd.  xp_attn_bwd2 resets it with hipMemsetAsync on the call's stream in front
    of the launch, whenever the plan says ``uses_counter`` (as the header states).  The only such word in the library.
  * the proxy partials (forward ``part``; backward ``dq`` / ``dkv``) and ``delta`` of attention.hip: written by the main launch
    for every problem, read by the merge / reduce launch (bwd_pair: delta by the dQ kernel, read by the dK/dV kernel) -- no
    accumulation into scratch.  attention_f32.hip: ``delta`` only, written by its first backward kernel.
  * csrc/attention_pooled.hip: per-chunk (m, l), O and dq partials, each written by its chunk's workgroup and combined in chunk
    order by a second launch; no counter, no atomics.
  * xp_reduce_rows_batch / xp_colsum (reduce.hip), xp_layernorm_bwd* (layernorm.hip), xp_vip_embed_bwd (embed.hip): partial rows
    written by level 1, read by level 2; segments of <= 64 rows skip level 1 and do not touch the workspace.  No such word.
  * loss_family.hip and the pair losses' file: logits, statistics, G matrices and part[] are each written by one launch and read by the following ones.
  * layer.hip: a bump allocator over the caller's workspace that checks every take against ``workspace_bytes``; the regions are
    the ones above plus GEMM outputs and split-K slabs (every slab element is written by its k-slice).
Nothing relies on previous contents."""
import functools
import os

import pytest
import torch

from oracle import clipvip_oracle as O
from tests import loss_family_ref as R
from tests.gpu_util import ModelArgs
from tests.guarded import GuardedWorkspaces
from tests.test_attention_gpu import F32, FUSED, GENERAL, WIDE, check_kernels

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float32]
IDS = ["bf16", "fp32"]


def _flat(x, prefix=""):
    """(name, tensor | None) leaves of nested tuples / lists / dicts"""
    if isinstance(x, dict):
        for k in sorted(x):
            yield from _flat(x[k], f"{prefix}.{k}")
    elif isinstance(x, (tuple, list)):
        for i, v in enumerate(x):
            yield from _flat(v, f"{prefix}[{i}]")
    else:
        yield prefix, x


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def twice(fn, tags=None):
    """fn() under the ordinary allocator, then under GuardedWorkspaces: (a) bit-identical outputs, (b) guards intact, (c) no new NaN.
    ``tags``: workspace tags the guarded run must have requested.  Returns the manager (its records)."""
    from xpretrain_amd import hip_ops as H
    real = H.workspace
    plain = fn()
    torch.cuda.synchronize()
    with GuardedWorkspaces() as gw:
        assert H.workspace is not real
        guarded = fn()
    assert H.workspace is real                                  # restored
    gw.check()                                                  # (b); synchronises first, the buffers are still held
    assert gw.records, "the case requested no workspace"
    if tags:
        assert set(tags) <= {t for t, _, _ in gw.records}, (tags, sorted({t for t, _, _ in gw.records}))
    a, b = list(_flat(plain)), list(_flat(guarded))
    assert [n for n, _ in a] == [n for n, _ in b]
    for (name, p), (_, g) in zip(a, b):
        if p is None or g is None:
            assert p is None and g is None, name
            continue
        if not torch.is_tensor(p):
            assert p == g, name
            continue
        assert p.shape == g.shape and p.dtype == g.dtype, name
        if g.is_floating_point():
            new_nan = (torch.isnan(g) & ~torch.isnan(p)).sum().item()
            assert new_nan == 0, f"{name}: {new_nan} NaNs only the poisoned-workspace run has"          # (c)
        assert torch.equal(_bits(p), _bits(g)), f"{name}: differs between the ordinary and the exact-size workspace"      # (a)
    return gw


# ------------------------------------------------------------------------------------------------ the helper itself
def test_guarded_workspaces_helper():
    """exact sizes, alignment, poison, the 0-byte body, records, a caught overrun (written by torch, not by a kernel), restoration"""
    from xpretrain_amd import hip_ops as H
    real = H.workspace
    dev = torch.device("cuda", torch.cuda.current_device())
    with GuardedWorkspaces() as gw:
        a = H.workspace(1000, dev, "a")
        z = H.workspace(0, dev, "zero")
        o = H.workspace(4097, dev, "odd")
        assert (a.numel(), z.numel(), o.numel()) == (1000, 256, 4097) and a.dtype == torch.uint8
        assert all(t.data_ptr() % 4096 == 0 for t in (a, z, o)) and z.data_ptr() != 0
        assert bool((a.view(torch.int16) == 0x7FA5).all()) and bool(torch.isnan(a.view(torch.bfloat16)).all())
        assert bool(torch.isnan(a.view(torch.float32)).all()) and int(a.view(torch.int32)[0]) > 0
        assert H.workspace(1000, dev, "a").data_ptr() != a.data_ptr()          # fresh per request
        a.zero_(); o.zero_()                                                   # the body is the caller's
    assert H.workspace is real
    assert [r[:2] for r in gw.records] == [("a", 1000), ("zero", 0), ("odd", 4097), ("a", 1000)]
    gw.check()
    with pytest.raises(AssertionError, match="'a'.*beyond the plan's 500 bytes"):
        gw.check_body_beyond("a", 500)
    for tag, nbytes, raw, off, body in gw._bufs[2:3]:                          # one byte behind the odd body
        raw[off + body] = 0
    with pytest.raises(AssertionError, match="'odd'.*behind the 4097-byte body.*offset 4097"):
        gw.check()
    with pytest.raises(RuntimeError):                                          # restored on an exception too
        with GuardedWorkspaces():
            raise RuntimeError("x")
    assert H.workspace is real                                                 # the final assertion: nothing stays patched


# ------------------------------------------------------------------------------------------------ column sums, reduce
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rows,cols", [(65, 768), (7, 64)])
def test_colsum_and_deferred_reduce(rows, cols, dtype):
    """xp_colsum, xp_colsum_partials + xp_reduce_rows_batch; a segment of `rows` partial rows: 65 takes the two-level reduce (its
    level-1 rows live in the workspace), 7 the direct one (a request the body of which no kernel touches)"""
    from xpretrain_amd import hip_ops as H
    torch.manual_seed(rows)
    X = torch.randn(rows, cols, device="cuda").to(dtype)
    part = torch.randn(rows, cols, device="cuda")

    def fn():
        d = H.DeferredReduce(X.device)
        cs = H.colsum_deferred(X, rows, cols, d)
        seg = torch.full((cols,), 3.0, device="cuda")
        d.add(part, 0, seg, rows, cols, cols, accumulate=True)
        d.flush()
        return H.colsum(X, rows, cols), cs, seg
    twice(fn, tags=["colsum", "defer:colsum", "reduce_batch"])


# ------------------------------------------------------------------------------------------------ LayerNorm backward
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rows,cols", [(60, 768), (60, 192), (4712, 768), (4712, 192)])
def test_layernorm_bwd(rows, cols, dtype):
    """immediate; deferred with dx_colsum / dres_colsum; with the fp32 side rows -- 60 rows: one block of partial rows, 4712: many"""
    from xpretrain_amd import hip_ops as H
    torch.manual_seed(rows + cols)
    side = (10, 3, 5) if rows == 60 else (2356, 4, 4)
    x, dy, dres = [torch.randn(rows, cols, device="cuda").to(dtype) for _ in range(3)]
    xs = torch.randn((rows + side[0] - 1) // side[0] * side[2], cols, device="cuda")
    g, b = torch.randn(cols, device="cuda"), torch.randn(cols, device="cuda")
    _, mean, rstd = H.layernorm_fwd(x, g, b, rows, cols)
    _, mean_s, rstd_s = H.layernorm_fwd(x, g, b, rows, cols, x_side=xs, side=side)

    def fn():
        out = [H.layernorm_bwd(dy, x, g, mean, rstd, rows, cols, dres=dres),
               H.layernorm_bwd(dy, x, g, mean_s, rstd_s, rows, cols, dres=dres, x_side=xs, side=side)]
        d = H.DeferredReduce(x.device)
        out.append(H.layernorm_bwd(dy, x, g, mean, rstd, rows, cols, defer=d, name="ln_a"))
        out.append(H.layernorm_bwd(dy, x, g, mean, rstd, rows, cols, dres=dres, defer=d, dx_colsum=True, name="ln_b"))
        out.append(H.layernorm_bwd(dy, x, g, mean, rstd, rows, cols, dres=dres, defer=d, dx_colsum=True, dres_colsum=True, name="ln_c"))
        out.append(H.layernorm_bwd(dy, x, g, mean_s, rstd_s, rows, cols, dres=dres, defer=d, dx_colsum=True, dres_colsum=True,
                                   name="ln_side", x_side=xs, side=side))
        d.flush()
        return out
    gw = twice(fn, tags=["ln", "defer:ln_a", "defer:ln_c", "reduce_batch"])
    nb = H.L.lib().xp_layernorm_bwd_workspace_bytes(rows, cols)
    assert all(n == nb for t, n, _ in gw.records if t == "ln" or t.startswith("defer:ln"))


# ------------------------------------------------------------------------------------------------ embedding backward
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_vip_embed_bwd(dtype):
    from xpretrain_amd import hip_ops as H
    B, M, T, Lp, D = 3, 4, 5, 9, 128
    torch.manual_seed(1)
    dx = torch.randn(B, M + T * Lp, D, device="cuda").to(dtype)
    twice(lambda: H.vip_embed_bwd(dx, B, M, T, Lp, D), tags=["embed"])


# ------------------------------------------------------------------------------------------------ losses
LOSS_SHAPES = [(k, s) for k in R.KINDS for s in ((9, 9, 30), (200, 200, 96))] + \
              [(k, (200, 72, 96)) for k in ("vidimg", "vidimg_divide")]          # the only workspace formula with n + m


@pytest.mark.parametrize("kind,shape", LOSS_SHAPES, ids=[f"{k}-{'x'.join(map(str, s))}" for k, s in LOSS_SHAPES])
def test_contrastive_loss(kind, shape):
    from xpretrain_amd import hip_ops as H
    n, m, d = shape
    feats = [f.float().cuda() for f in R.unit_feats(n, m, d, seed=n + m + d)]
    v, t, i, c = R.operands(kind, feats)
    ls = torch.tensor(3.7, device="cuda")
    gw = twice(lambda: H.contrastive_loss(R.KIND_IDS[kind], v, t, i, c, log_scale=ls), tags=["loss"])
    assert gw.records[0][1] == H.L.lib().xp_contrastive_loss_workspace_bytes(R.KIND_IDS[kind], n, m if (i is not None or c is not None) else n, d)


@pytest.mark.parametrize("n,d", [(9, 30), (200, 96)])
def test_nce_and_vsc_fc_entry_points(n, d):
    """the two losses that once had entries of their own, through their modules and autograd (the benchmark's route to the family
    entry): the loss and every gradient"""
    from xpretrain_amd.optimization import NCELearnableTempLoss, NCELearnableTempLoss_vsc_fc
    feats = [f.float().cuda().requires_grad_() for f in R.unit_feats(n, n, d, seed=n + d)]
    ls = torch.tensor(4.6, device="cuda", requires_grad=True)

    def run(fn, ops):
        loss = fn(*ops, ls)
        return loss.detach(), torch.autograd.grad(loss, ops + [ls])
    twice(lambda: (run(NCELearnableTempLoss(), feats[:2]), run(NCELearnableTempLoss_vsc_fc(), feats)), tags=["loss"])


# ------------------------------------------------------------------------------------------------ dense attention
# (kernels, size | None, B, H, S, causal mask mode, dtype, variant): one shape per kernel name of _lib.ATTN_KERNELS / ATTN_OPTIN_KERNELS
ATTN_CASES = [(FUSED, (1, 3, 5), 2, 1, None, torch.bfloat16, None), (FUSED, (4, 12, 196), 1, 2, None, torch.bfloat16, None),
              (WIDE, (4, 3, 300), 2, 2, None, torch.bfloat16, None), (GENERAL, (17, 2, 180), 1, 1, None, torch.bfloat16, None),
              (F32, (4, 2, 49), 2, 2, None, torch.float32, None), (("fwd3", "bwd_pair"), (4, 12, 196), 1, 2, None, torch.bfloat16, "split"),
              (("fwd4", "bwd6"), (4, 3, 300), 2, 2, None, torch.bfloat16, "wide"), (GENERAL, None, 2, 2, (77, "ragged"), torch.bfloat16, None)]


def test_attention_cases_name_every_kernel():
    from xpretrain_amd import _lib as L
    named = {k for c in ATTN_CASES for k in c[0]}
    assert named == set(L.ATTN_KERNELS) | set(L.ATTN_OPTIN_KERNELS.values())


@pytest.mark.parametrize("kernels,size,B,Hh,causal,dtype,variant", ATTN_CASES,
                         ids=[f"{c[0][0]}-{c[0][1]}-{c[1] or c[4]}" for c in ATTN_CASES])
def test_dense_attention(kernels, size, B, Hh, causal, dtype, variant, monkeypatch):
    """hip_ops.attn_fwd / attn_bwd with colsum_defer (the bias column sums' partial rows and their reduce included)"""
    from xpretrain_amd import hip_ops as H
    from tests.attn_emulation import pad_mask_of
    if size is not None:
        S, pad = size[0] + size[1] * size[2], None
    else:
        S = causal[0]
        pad = pad_mask_of(B, S, causal[1]).cuda()
    prev_wide, prev_debug = H.get_attn_bwd_wide(), os.environ.get("XPRETRAIN_DEBUG")
    try:
        if variant == "split":
            monkeypatch.setenv("XPRETRAIN_DEBUG", ",".join(filter(None, [prev_debug, "attn_bwd_split"])))
        elif variant == "wide":
            H.set_attn_bwd_wide(True)
        check_kernels(kernels, B, S, Hh, size=size, pad=pad is not None, dtype=dtype)
        torch.manual_seed(S)
        qkv = (torch.randn(B * S, 3 * Hh * 64, device="cuda") * 0.7).to(dtype)
        dout = torch.randn(B * S, Hh * 64, device="cuda").to(dtype)

        def fn():
            out, stats = H.attn_fwd(qkv, B, S, Hh, size=size, pad_mask=pad)
            d = H.DeferredReduce(qkv.device)
            dqkv, cs = H.attn_bwd(qkv, out, dout, stats, B, S, Hh, size=size, pad_mask=pad, q_scale=0.125, colsum_defer=d)
            d.flush()
            return out, stats, dqkv, cs
        gw = twice(fn, tags=["attn", "defer:dbqkv", "reduce_batch"])
        M, N, Lp = size if size is not None else (0, 1, S)
        nb = H.L.lib().xp_attn_workspace_bytes(H.L.ATTN_PROXY if size is not None else H.L.ATTN_CAUSAL, B, Hh, M, N, Lp)
        assert [n for t, n, _ in gw.records if t == "attn"] == [nb, nb]
    finally:
        H.set_attn_bwd_wide(prev_wide)
        monkeypatch.undo()
    assert H.get_attn_bwd_wide() == prev_wide and os.environ.get("XPRETRAIN_DEBUG") == prev_debug


# ------------------------------------------------------------------------------------------------ single-query attention
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,S,Hh", [(2, 102, 2), (2, 904, 2)])
def test_pooled_attention(B, S, Hh, dtype):
    """S = 102: the smallest split of the keys; S = 904: many chunks per problem (the chunk partials and their combine live in the
    workspace: 15 chunks on 256 CUs)"""
    from xpretrain_amd import hip_ops as H
    chunks = H.attn_pooled_plan(B, S, Hh, dtype=dtype)["chunks"]
    assert chunks >= (8 if S == 904 else 1), chunks
    torch.manual_seed(S)
    q = torch.randn(B, Hh * 64, device="cuda").to(dtype)
    kv = torch.randn(B * S, 2 * Hh * 64, device="cuda").to(dtype)
    dout = torch.randn(B, Hh * 64, device="cuda").to(dtype)

    def fn():
        out, stats = H.attn_pooled_fwd(q, kv, B, S, Hh)
        d = H.DeferredReduce(q.device)
        dq, dkv, cs = H.attn_pooled_bwd(q, kv, out, dout, stats, B, S, Hh, q_scale=0.125, colsum_defer=d)
        d.flush()
        return out, stats, dq, dkv, cs
    gw = twice(fn, tags=["attn_pooled", "defer:dbkv", "reduce_batch"])
    nb = H.L.lib().xp_attn_pooled_workspace_bytes(B, Hh, S, H._dt(q))
    assert [n for t, n, _ in gw.records if t == "attn_pooled"] == [nb, nb]


# ------------------------------------------------------------------------------------------------ the whole step
@functools.lru_cache(maxsize=None)
def _step_inputs():
    return tuple(t.cuda() for t in O.synthetic_inputs(4, 4, 32, 8, vocab=120))


@pytest.mark.parametrize("pooled", [False, True], ids=["dense_last", "pooled_last"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_whole_training_step(dtype, pooled, monkeypatch):
    """the tiny model of test_loss_family_gpu.test_model_hand_off_vs_vc_fc_and_dsl (B 4): forward, NCELearnableTempLoss, backward,
    AdamW.clip_and_step, with the second forward chain and the side stream running (FWD_SPLIT_MIN_ROWS = 0).  Loss, gradient norm,
    every parameter gradient and every parameter after the step are bit-identical: xp_encoder_layer_fwd / _bwd / _pooled_fwd /
    _pooled_bwd are held to their own *_workspace_bytes, the split-K slabs to theirs."""
    import xpretrain_amd.functional as XF
    from xpretrain_amd.modeling import VidCLIP
    from xpretrain_amd.optimization import AdamW, NCELearnableTempLoss, build_e2e_optimizer_w_lr_mul
    monkeypatch.setattr(XF, "FWD_SPLIT_MIN_ROWS", 0)
    made = []

    class Spy(XF.ForwardSplit):
        def __init__(self, device):
            made.append(1)
            super().__init__(device)
    monkeypatch.setattr(XF, "ForwardSplit", Spy)
    cfgd = O.hf_config_dict(128, 2, 2, 256, 16, 32, 128, 2, 2, 256, 120, 16, 64)
    video, ids, mask = _step_inputs()

    def fn():
        torch.manual_seed(11)
        model = VidCLIP(ModelArgs(cfgd, 4))
        with torch.no_grad():
            model.clipmodel.vision_model.embeddings.temporal_embedding.normal_(0, 0.1)
        model.cuda().train()
        model.clipmodel.set_compute_dtype(dtype)
        model.clipmodel.pooled_last_layer = pooled
        groups = build_e2e_optimizer_w_lr_mul(list(model.named_parameters()), 1e-3, 0.05, lr_mul=1, lr_mul_prefix="")
        opt = AdamW([g for g in groups if g["params"]], lr=1e-3, betas=(0.9, 0.98))
        out = model(video, ids, mask)
        loss = NCELearnableTempLoss()(out["vis_features"], out["text_features"], model.clipmodel.logit_scale)
        loss.backward()
        grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
        assert set(grads) == {n for n, _ in model.named_parameters()}
        norm = opt.clip_and_step(0.05)
        torch.cuda.synchronize()
        return loss.detach().clone(), norm.clone(), grads, {n: p.detach().clone() for n, p in model.named_parameters()}
    gw = twice(fn)
    tags = {t for t, _, _ in gw.records}
    want = {"layer_fwd", "layer_bwd", "loss"} | ({"layer_pooled_fwd", "layer_pooled_bwd"} if pooled else set())
    assert want <= tags, sorted(tags)
    print(f"whole step {dtype} pooled={pooled}: {len(gw.records)} workspace requests, tags {sorted(tags)}")
    streams = {s for t, _, s in gw.records if t == "layer_fwd"}
    print(f"layer_fwd workspaces on {len(streams)} streams; {len(made)} forward splits in the two runs")
    assert len(made) == 2, "the video tower's forward did not run as two half-batch chains"
    assert len(streams) >= 2, "no layer forward asked for its workspace on a second stream"
