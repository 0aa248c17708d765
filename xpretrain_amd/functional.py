"""Autograd layer over the HIP kernels: one ``torch.autograd.Function`` per *fused block* of the path.

The unit of fusion is the transformer layer (``EncoderLayerFn``), not the op: the forward chains
LN -> fused-QKV GEMM (+bias, q-scale) -> fused attention -> out-proj GEMM (+bias +residual) -> LN ->
fc1 GEMM (+bias +quick_gelu or erf gelu) -> fc2 GEMM (+bias +residual); the backward chains the matching dX / dW
GEMMs with the activation-derivative and residual-gradient adds folded into GEMM / LayerNorm epilogues.
All arithmetic happens in ``libxpretrain_hip.so`` (``hip_ops``); torch only owns the buffers and the graph.

Activations are 2-D ``[tokens, features]`` tensors in the compute dtype (bf16 by default); parameters stay
fp32 masters and are cast once per weight version (``WeightCache``).  Parameter gradients are fp32.
Reference call sites are cited per class (paths relative to /root/reference/CLIP-ViP/src).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import weakref
from typing import Optional, Tuple

import torch

from . import _lib as L
from . import hip_ops as H


# ------------------------------------------------------------------------------------------ weights
class _Entry:
    __slots__ = ("ver", "buf", "refs")

    def __init__(self, ver, buf, refs):
        self.ver, self.buf, self.refs = ver, buf, refs


class WeightCache:
    """Compute-dtype copies of fp32 master weights.  An entry is refreshed when (a) the parameter's version counter
    moved (``load_state_dict`` / in-place edits), or (b) ANY optimizer stepped since the copy was made -- fused / foreach
    optimizers update parameters without bumping ``Tensor._version`` (observed with ``AdamW(fused=True)``), so a global
    optimizer-step hook advances ``generation``.  ``invalidate()`` forces a refresh by hand.  An optimizer that rewrites
    the copies itself (``optimization.AdamW``: the shadows are written by the update kernel) asks for their addresses
    with ``shadow_bindings`` and keeps them valid through ``invalidate(keep=...)``."""

    def __init__(self):
        self._c = {}
        self.generation = 0
        self.structure_version = 0      # bumped whenever a cached buffer is (re)allocated
        self.casts = 0                  # bumped whenever a cast kernel is launched (on the caller's current stream)
        self._hooked = False

    def _ensure_hook(self):
        if not self._hooked:
            from torch.optim.optimizer import register_optimizer_step_post_hook

            def hook(opt, args, kwargs):
                after = getattr(opt, "_xp_after_step", None)
                if after is not None:
                    after(self)
                else:
                    self.invalidate()
            register_optimizer_step_post_hook(hook)
            self._hooked = True

    def _ver(self, ws):
        return tuple((w._version, w.data_ptr(), self.generation) for w in ws)

    def invalidate(self, keep=None):
        """Every cached copy goes stale, except the entries in ``keep`` (a list from ``shadow_bindings``) which the
        caller has just rewritten from the current master values."""
        self.generation += 1
        for key, ent in keep or ():
            if self._c.get(key) is ent:
                ws = [r() for r in ent.refs]
                if all(w is not None for w in ws):
                    ent.ver = self._ver(ws)
                # the buffer was rewritten through a raw pointer: tell autograd, so that a graph which saved it for backward
                # (forward -> optimizer.step() -> backward) fails loudly instead of computing dX with the new weights
                torch.autograd.graph.increment_version(ent.buf)

    @staticmethod
    def _alive(ent, ws) -> bool:
        """ids are only unique among LIVE objects: an entry is valid only while its weak references still point at
        the very tensors being asked about (a freed model's id can be reused by a new parameter)."""
        return ent is not None and all(r() is w for r, w in zip(ent.refs, ws))

    def get(self, w: torch.Tensor, dtype) -> torch.Tensor:
        if dtype == torch.float32:
            return w.detach()
        return self.fused((w,), dtype, _single=True)

    def fused(self, ws, dtype, _single=False) -> torch.Tensor:
        """Row-concatenation of several [n_i, k] weights (or 1-D biases) in `dtype`: the fused QKV operand."""
        self._ensure_hook()
        key = (tuple(id(w) for w in ws), dtype)
        ver = self._ver(ws)
        ent = self._c.get(key)
        if not self._alive(ent, ws) or ent.ver != ver:
            rows = sum(w.shape[0] for w in ws) if not _single else ws[0].shape[0]
            shape = tuple(ws[0].shape) if _single else (rows,) + tuple(ws[0].shape[1:])
            reuse = ent is not None and tuple(ent.buf.shape) == shape and ent.buf.device == ws[0].device
            if not reuse:
                self.structure_version += 1
            buf = ent.buf if reuse else torch.empty(shape, dtype=dtype, device=ws[0].device)
            if reuse:
                torch.autograd.graph.increment_version(buf)      # in-place rewrite below (raw pointer): see invalidate()
            self.casts += 1
            if _single:
                H.cast(ws[0].detach(), dtype, out=buf)
            else:
                r = 0
                for w in ws:
                    H.cast(w.detach(), dtype, out=buf[r:r + w.shape[0]])
                    r += w.shape[0]
            ent = _Entry(ver, buf, tuple(weakref.ref(w) for w in ws))
            self._c[key] = ent
        return ent.buf

    def shadow_bindings(self, params):
        """For an optimizer that rewrites the cached copies in its update kernel: ``({id(p): (device address, XP dtype
        code)}, entries)`` over the cache entries ALL of whose source tensors are in ``params`` (at most one copy per
        parameter; any other copy simply goes stale at the step)."""
        ids = {id(p) for p in params}
        shadows, entries = {}, []
        for key, ent in self._c.items():
            ws = [r() for r in ent.refs]
            if any(w is None or id(w) not in ids or id(w) in shadows for w in ws) or not ent.buf.is_contiguous():
                continue
            code = {torch.bfloat16: 0, torch.float32: 1}.get(ent.buf.dtype)
            if code is None:
                continue
            off = 0
            for w in ws:
                shadows[id(w)] = (ent.buf.data_ptr() + off * ent.buf.element_size(), code)
                off += w.numel()
            entries.append((key, ent))
        return shadows, entries

    def clear(self):
        self._c.clear()
        self.structure_version += 1


WEIGHTS = WeightCache()


_SPLITS = {}


def _split_for(n_out: int, n_in: int, rows: int, dtype: torch.dtype, a_remap, slack: bool = False, lddy: Optional[int] = None,
               ldx: Optional[int] = None) -> int:
    """split-K factor for the weight-gradient GEMMs (kernel-family aware, decided by the library; memoised).  ``slack``: a launch
    nothing waits for soon (the first three dW GEMMs of a layer's backward, as csrc/layer.hip issues them): fewer, longer slabs.
    ``lddy`` / ``ldx``: row pitches of the two operands (default: dense, n_out / n_in)."""
    lddy, ldx = lddy or n_out, ldx or n_in
    key = (n_out, n_in, rows, dtype, a_remap, slack, lddy, ldx)   # (the CU budget is part of the plan: set_cu_budget clears the memo)
    s = _SPLITS.get(key)
    if s is None:
        s = _SPLITS[key] = H.gemm_auto_split(n_out, n_in, rows, dtype, lda=lddy, ldb=ldx, a_remap=a_remap, slack=slack)
    return s


def _wgrad(dy: torch.Tensor, x: torch.Tensor, rows: int, n_out: int, n_in: int, a_remap=(0, 0, 0), slack: bool = False, *,
           lddy: Optional[int] = None, ldx: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dW[n_out, n_in] = dY[rows, n_out]^T . X[rows, n_in] in fp32 (both operands read k-strided with row pitches ``lddy`` /
    ``ldx``, split-K), into ``out`` when given."""
    lddy, ldx = lddy or n_out, ldx or n_in
    split = _split_for(n_out, n_in, rows, dy.dtype, tuple(a_remap), slack, lddy, ldx)
    dw = torch.empty((n_out, n_in), dtype=torch.float32, device=dy.device) if out is None else out.view(n_out, n_in)
    if split <= 1:
        H.gemm(dy, x, n_out, n_in, rows, a_kstrided=True, b_kstrided=True, lda=lddy, ldb=ldx, out=dw,
               out_dtype=torch.float32, a_remap=a_remap)
    else:
        ws = H.workspace(split * n_out * n_in * 4, dy.device, "splitk")
        H.gemm(dy, x, n_out, n_in, rows, a_kstrided=True, b_kstrided=True, lda=lddy, ldb=ldx, out=ws,
               split_k=split, a_remap=a_remap)
        H.splitk_reduce(ws, dw, splits=split)
    return dw


# ------------------------------------------------------------------------------------------ encoder layer, native sequencing
# LAYER_CALLS (default): one C-ABI call per layer pass (xp_encoder_layer_fwd / _bwd, csrc/layer.hip) -- the same entry points in
# the same order with the same arguments as the op-by-op path below, issued from native code; XPRETRAIN_DEBUG=op_by_op keeps the
# op-by-op path (tools/determinism_hunt.py fingerprints every call of it; tests compare the two paths bit for bit).
LAYER_CALLS = "op_by_op" not in L.DEBUG
# XPRETRAIN_SPARSE_LAST_BWD=0: the last video layer's backward runs dense even where its incoming gradient is known to be zero outside
# "row r0 of every sample" (default: the MLP / out_proj GEMMs of that backward run over tile lists -- _dx3_support; same bits)
SPARSE_LAST_BWD = os.environ.get("XPRETRAIN_SPARSE_LAST_BWD", "1") != "0"
_DT_CODE = {torch.bfloat16: L.XP_BF16, torch.float32: L.XP_F32}
_NULLCTX = contextlib.nullcontext()
_ES = {torch.bfloat16: 2, torch.float32: 4}
_PLANS = {}


def set_cu_budget(cus: int) -> None:
    """CUs the split-K planning of the weight-gradient GEMMs may fill (xp_set_cu_budget; 256 = the whole MI355X).  A data-parallel
    run lowers it by the workgroups its collectives keep resident beside the backward pass (distributed.reserve_cus_for_collectives).
    The memoised split factors and layer plans (workspace sizes depend on the split) are dropped."""
    L.check(L.lib().xp_set_cu_budget(int(cus)), "xp_set_cu_budget")
    _SPLITS.clear()
    _PLANS.clear()


def _arena_layout(pieces):
    """``(((name, offset, bytes per row), ...), total bytes)`` of (name, row count, bytes per row) pieces laid out one after the
    other, each 256-byte aligned"""
    fill, o = [], 0
    for name, n, bpr in pieces:
        fill.append((name, o, bpr))
        o += (n * bpr + 255) & ~255
    return tuple(fill), o


def _piece_views(plan, arena):
    """The saved pieces of ``arena`` as tensors by field name, as the hip_ops wrappers take them (the op-by-op sequencers' buffers;
    the native calls take the same addresses from _layer_args): [n, .] matrices in the compute dtype; the LayerNorm and attention
    statistics flat in fp32 (the wrappers take those by element count)."""
    views = {}
    for (name, n, bpr), (_, o, _) in zip(plan.pieces, plan.fill):
        raw = arena[o:o + n * bpr]
        views[name] = raw.view(torch.float32) if name[:4] in ("mean", "rstd", "stat") else raw.view(plan.dtype).view(n, -1)
    return views


def _finish_plan(plan, dims, dtype, pieces, queries):
    """what _LayerPlan and _PooledLayerPlan derive from their table of saved pieces and their two workspace queries"""
    plan.dims, plan.pieces, plan.dtype, plan.side_row = dims, pieces, dtype, dims.D * 4
    plan.rD, plan.size = dims.D * _ES[dtype], (dims.M, dims.N, dims.L) if dims.attn_mode == L.ATTN_PROXY else None
    # (rD: bytes of a [., D] compute-dtype row; size: None for the causal text layer)
    plan.side_S, plan.side_M = (dims.S, dims.M) if dims.attn_mode == L.ATTN_PROXY else (1, 1)      # fp32 side rows: [B*M, D] / [rows, D]
    plan.fill, plan.arena_bytes = _arena_layout(pieces)
    plan.fwd_ws, plan.bwd_ws = (int(getattr(L.lib(), q)(C.byref(dims))) for q in queries)
    # flat fp32 parameter gradients, in the order of EncoderLayerFn.forward's parameter arguments
    D, Dff = dims.D, dims.Dff
    plan.gsizes = [D, D, 3 * D * D, 3 * D, D * D, D, D, D, Dff * D, Dff, D * Dff, D]
    plan.gnames = ["dln1_w", "dln1_b", "dwqkv", "dbqkv", "dwo", "dbo", "dln2_w", "dln2_b", "dw1", "db1", "dw2", "db2"]
    plan.gtotal = sum(plan.gsizes)


class _LayerPlan:
    """Sizes / offsets of one (shape, dtype) of encoder layer: the saved-activation arena of the forward, the flat
    parameter-gradient buffer of the backward, the workspace sizes.  ``pieces`` is THE table of what the forward saves for the
    backward: (field name in XpLayerFwd and XpLayerBwd, row count, bytes per row), in arena order -- compute-dtype activations, then
    fp32 statistics.  The arena layout (``fill``, ``arena_bytes``), the pointer fill of both argument structs (_layer_args) and the
    second forward chain's offsets (first row * bytes per row: every piece is row-proportional, ``stats`` holds heads * 2 floats
    per token row) all come from it: a new saved piece is one row here."""

    def __init__(self, rows, D, Dff, B, S, heads, size, dtype, act=L.ACT_QUICK_GELU):
        d = L.XpLayerDims()
        d.rows, d.D, d.Dff, d.B, d.S, d.heads = rows, D, Dff, B, S, heads
        d.M, d.N, d.L = size if size is not None else (0, 1, S)
        d.attn_mode = L.ATTN_PROXY if size is not None else L.ATTN_CAUSAL
        d.dtype, d.q_scale, d.ln_eps = _DT_CODE[dtype], (D // heads) ** -0.5, 1e-5
        d.act = act                 # the MLP's activation (L.ACTS): the fc1 / dpre epilogue kinds the native stages pick
        rD, rF = D * _ES[dtype], Dff * _ES[dtype]      # bytes of a [., D] / [., Dff] row
        _finish_plan(self, d, dtype, (("h1", rows, rD), ("qkv", rows, 3 * rD), ("attn_o", rows, rD), ("x2", rows, rD), ("h2", rows, rD),
                                   ("pre", rows, rF), ("act", rows, rF), ("mean1", rows, 4), ("rstd1", rows, 4), ("mean2", rows, 4),
                                   ("rstd2", rows, 4), ("stats", rows, heads * 2 * 4)),
                     ("xp_encoder_layer_fwd_workspace_bytes", "xp_encoder_layer_bwd_workspace_bytes"))


def _layer_plan(rows, D, Dff, B, S, heads, size, dtype, act=L.ACT_QUICK_GELU) -> _LayerPlan:
    key = (rows, D, Dff, B, S, heads, size, dtype, act)
    p = _PLANS.get(key)
    if p is None:
        p = _PLANS[key] = _LayerPlan(*key)
    return p


def _native_ok(x, params, pad_mask) -> bool:
    """The native layer calls hand raw device pointers to C: everything the op-by-op path validates per call (hip_ops._chk)
    is validated here in one place -- of ``params`` (in _FWD_PARAMS order) the 1-D parameters contiguous fp32 on x's device, the
    weight copies ("W..") contiguous in the compute dtype; an int64 contiguous padding mask.  False -> the caller takes the
    op-by-op path, whose checks raise a TypeError that names the offending argument (a model cast with .bfloat16(), a bool mask,
    a strided parameter ...)."""
    dev = x.device
    if not x.is_cuda or not x.is_contiguous():
        return False
    for n, t in zip(_FWD_PARAMS, params):
        if t.dtype != (x.dtype if n[0] == "W" else torch.float32) or t.device != dev or not t.is_contiguous():
            return False
    if pad_mask is not None and (pad_mask.dtype != torch.int64 or pad_mask.device != dev or not pad_mask.is_contiguous()):
        return False
    return True


# ---- weights the optimizer is still writing (optimization.AdamW(overlap=...)) ---------------------------------------------------
# AdamW.step can run the update of the encoder layers >= K of both towers on a stream of its own, so that the HBM-bound optimizer
# pass overlaps the MFMA-bound first layers of the NEXT forward instead of standing between two steps.  One LateUpdate per
# overlap_next_forward() call owns that protocol: the side stream, the event of the latest late launch and the encoders whose forward
# waits for it in front of layer K (CLIPEncoder.late_update).  Anything else that reads or writes those parameters, their moments or
# their gradients outside a model forward calls join_late_weights() first: the model's state_dict / load_state_dict pre-hooks and the
# optimizer's state_dict, load_state_dict, zero_grad(set_to_none=False) and step do.
_LATE_UPDATES = weakref.WeakSet()


class LateUpdate:
    """The update of the encoder layers >= ``first_layer`` that ``owner`` (an optimizer) runs beside the next forward."""

    def __init__(self, first_layer, owner=None):
        self.first_layer = int(first_layer)
        self.streams = {}               # device -> the side stream the late launches run on
        self.event = None               # of the latest late launch, until a join finds it finished
        self.owner = weakref.ref(owner) if owner is not None else None
        self.encoders = weakref.WeakSet()
        _LATE_UPDATES.add(self)

    @contextlib.contextmanager
    def launch(self, main_stream):
        """The body runs on the side stream (yielded), behind everything ``main_stream`` has enqueued so far; its end is the event
        the next forward waits for."""
        side = self.streams.get(main_stream.device)
        if side is None:
            side = self.streams[main_stream.device] = torch.cuda.Stream(device=main_stream.device)
        side.wait_stream(main_stream)
        with torch.cuda.stream(side):
            yield side
            ev = torch.cuda.Event()
            ev.record(side)
        self.event = ev

    def _ordered(self) -> bool:
        # A capturing stream neither queries nor waits: step() refuses to overlap under capture, so a pending event was recorded
        # before the capture began, and torch.cuda.graph synchronises the device before it begins one.
        return self.event is None or torch.cuda.is_current_stream_capturing()

    def wait(self, layer_index, *streams):
        """Before encoder layer ``layer_index`` runs on ``streams`` (default: the current stream)."""
        if layer_index != self.first_layer or self._ordered():
            return
        for st in (streams or (torch.cuda.current_stream(),)):
            st.wait_event(self.event)

    def join(self):
        """The current stream is ordered behind the pending update.  A finished update is forgotten; an unfinished one stays pending,
        other streams may still have to wait for it."""
        if self._ordered():
            return
        if self.event.query():
            self.event = None
        else:
            torch.cuda.current_stream().wait_event(self.event)

    def attach(self, encoders):
        """``encoders`` wait for this update from now on.  One overlapped optimizer per encoder: a record of the same owner (or of a
        dead one) is joined and replaced, another live owner's is a ``ValueError`` (raised before anything changed)."""
        mine = self.owner() if self.owner is not None else None
        for enc in encoders:
            other = enc.late_update
            if other is not None and other.owner is not None and other.owner() not in (None, mine):
                raise ValueError("overlap_next_forward: this encoder already waits for another optimizer's late update")
        for enc in encoders:
            if enc.late_update is not None:
                enc.late_update.join()
            enc.late_update = self
            self.encoders.add(enc)

    def detach(self):
        self.join()
        for enc in list(self.encoders):
            if enc.late_update is self:
                enc.late_update = None
        self.encoders.clear()

    def __deepcopy__(self, memo):       # a copy of the model holds other parameters: no optimizer updates them late
        return None


def join_late_weights():
    """The current stream waits for every optimizer's late update (no-op when none is pending)."""
    for lu in list(_LATE_UPDATES):
        lu.join()


# ---- streams on which a backward pass allocates parameter gradients -----------------------------------------------------------------
# Autograd replays a node's backward on the stream of its forward, so the text tower's parameter gradients are allocated on the text
# tower's stream -- and the caching allocator hands a freed block back at once, but only to the stream that allocated it.  An
# optimizer reads those gradients on ITS stream; zero_grad(set_to_none=True) right behind the step would return them to the text
# stream's pool while the update kernel may still read them, and whatever allocates on that stream next (the shared stream also
# carries utils.prefetch.PrefetchLoader's copies) could overwrite them: only CLIPModel.forward's own fork orders that stream behind
# the caller's.  So the step orders every such stream behind its reads: one event per step, on a stream that is idle until the next
# forward forks from the caller's stream anyway.  (distributed.GradBucketReducer's pack path and the late update record_stream their
# gradients for the same reason; found by tests/stream_ledger.py)
GRADIENT_STREAMS = {}           # device index -> stream; CLIPModel.shared_text_stream registers the text tower's


def order_gradient_streams_behind(reader):
    """Every registered gradient stream of ``reader``'s device waits for what ``reader`` has enqueued so far (an optimizer step's
    reads of the gradients).  Not under capture: a wait would pull the other stream into the capture."""
    st = GRADIENT_STREAMS.get(reader.device.index)
    if st is not None and st != reader and not torch.cuda.is_current_stream_capturing():
        st.wait_stream(reader)


# XPRETRAIN_FWD_SPLIT=0: the whole batch as one chain (A/B switch for the two half-batch chains of the video tower's forward)
FWD_SPLIT = os.environ.get("XPRETRAIN_FWD_SPLIT", "1") != "0"
FWD_SPLIT_MIN_ROWS = 8192          # below this a half-batch launch no longer fills the chip beside its twin
FWD_SPLIT_HOLD_BYTES = 48 << 30    # forward-only passes: the most a split may hold until its join (every layer's buffers; 4.2 GB at cfg #2)
# FWD_SPLIT_STREAM (module attribute; tools set it): which stream the second chain runs on.  "side": the library's weight-gradient stream, idle
# during the forward (xp_side_stream) -- the step then touches main + text tower + side = three streams, as before the split.  "own":
# a torch stream of its own.  Same speed on one GPU (15.75 vs 15.75-15.79 ms per step, profiles/r04w_in_step_ab_second_chain_stream.txt);
# the fewer streams a step touches the better it survives the streams a collective library or a prefetcher adds: a fifth stream
# touched by the step cost 5 ms per step on this runtime, a fourth nothing (profiles/r04u_stream_count_probe.txt).
FWD_SPLIT_STREAM = "side"
_SPLIT_STREAMS = {}


def second_chain_stream_mode() -> str:
    return "own" if FWD_SPLIT_STREAM == "own" else "side"


def _second_chain_stream(device):
    st = _SPLIT_STREAMS.get(device.index)
    if st is None:
        if second_chain_stream_mode() == "side":
            with torch.cuda.device(device):
                ptr = L.lib().xp_side_stream()
            if ptr:
                st = torch.cuda.ExternalStream(ptr, device=device)
        if st is None:
            st = torch.cuda.Stream(device=device)
        _SPLIT_STREAMS[device.index] = st
    return st


class ForwardSplit:
    """The video tower's training forward as TWO half-batch chains: samples are independent in the forward, every kernel of a layer
    is row-parallel (GEMM rows, LayerNorm rows, attention per sample), so the second half of the batch runs the same layer call on a
    second stream into the second half of the SAME full-batch buffers.  The chains do not wait for each other between layers -- except
    at a layer whose compute-dtype weight copy was (re)cast inside the call (the first pass after a checkpoint load or an optimizer
    that does not maintain the shadows; xp_adamw_step writes them itself, so training steps never re-cast): the second chain then waits
    for that cast.  One chain's HBM-bound kernels (LayerNorm, attention, GEMM epilogues) run beside the other's MFMA main loops, and each chain's 111- /
    333- / 444-tile GEMMs fill the CUs the other leaves idle.  The backward sees ordinary full-batch buffers.  Results are bit-identical
    to the single chain (the same kernels compute every row).  Nothing of a layer may be freed before the chains are joined: a
    training pass keeps its activations for the backward anyway; a forward-only pass (torch.no_grad: retrieval, inference) has the
    split HOLD every layer's buffers until join() (round 6; ~0.46 GB per layer at cfg #2).  Measured: profiles/r04r_split_batch_probe_gemm256_forced.txt
    (probe), r04s_in_step_ab_forward_two_chains.txt (the step: -0.46 ms)."""

    def __init__(self, device):
        self.stream = _second_chain_stream(device)
        self.main = torch.cuda.current_stream(device)
        self.stream.wait_stream(self.main)          # fork: everything the tower's input depends on
        self.held = []

    def hold(self, *tensors):
        """buffers the second chain reads or writes: alive until the chains are joined (the caching allocator knows only the stream
        that allocated them, and without an autograd node a layer's input and arena die when the next layer returns)"""
        self.held.extend(t for t in tensors if t is not None)

    def join(self):
        self.main.wait_stream(self.stream)
        self.held.clear()       # (freed on the main stream, behind the join)


# ---- the argument structs of the four native layer calls ----------------------------------------------------------------------------
# Parameter pointer fields of the forward / backward structs, in the order their tensors are handed around
_FWD_PARAMS = ("ln1_w", "ln1_b", "Wqkv", "bqkv", "Wo", "bo", "ln2_w", "ln2_b", "W1", "b1", "W2", "b2")
_BWD_PARAMS = ("ln1_w", "ln2_w", "Wqkv", "Wo", "W1", "W2")


def _layer_args(struct, plan, dims, names, params, arena, r0=0, keep_pre=True, **tensors):
    """An argument struct of a native layer call: ``dims``, the parameter pointers (``names``: _FWD_PARAMS / _BWD_PARAMS, of the
    tensors ``params``), the saved pieces (plan.fill over ``arena``) and ``tensors`` by field name (x, x3, dx3, dx, the parameter
    gradients, the pooled layer's side rows; None: the field stays NULL) -- the pieces and the [., D] streams from token row ``r0``
    on (the second forward chain).  ``keep_pre`` False: a forward-only pass, the MLP pre-activation is not written (pre = NULL).
    Nothing is launched and no workspace is taken (_call_native does that), so a CPU test can build the structs."""
    a = struct()
    a.dims = dims
    for n, t in zip(names, params):
        setattr(a, n, t.data_ptr())
    base = arena.data_ptr()
    for n, o, bpr in plan.fill:
        setattr(a, n, base + o + r0 * bpr)
    if not keep_pre:
        a.pre = 0
    first = r0 * plan.rD
    for n, t in tensors.items():
        if t is not None:
            setattr(a, n, t.data_ptr() + first)
    return a


def _side_args(a, plan, r0, **sides):
    """the dense layer's fp32 side rows from token row ``r0`` on, and their geometry"""
    a.side_S, a.side_M = plan.side_S, plan.side_M
    first = r0 // plan.side_S * plan.side_M * plan.side_row
    for n, t in sides.items():
        if t is not None:
            setattr(a, n, t.data_ptr() + first)


def _call_native(entry, a, ws_bytes, device, ws_tag, *extra):
    """``extra``: what the entry point takes between the argument struct and the stream"""
    ws = H.workspace(ws_bytes, device, ws_tag)          # (per stream)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    L.check(getattr(L.lib(), entry)(C.byref(a), *extra, H._stream()), entry)


def _layer_fwd_args(plan, dims, x, params, pad_mask, arena, x3, keep_pre, side, side_out, side_x2, r0=0):
    """``dims``: the full batch's (plan.dims) or one chain's; the buffers are always the full batch's"""
    a = _layer_args(L.XpLayerFwd, plan, dims, _FWD_PARAMS, params, arena, r0, keep_pre, x=x, x3=x3)
    a.pad_mask = 0 if pad_mask is None else pad_mask.data_ptr()
    if side is not None:
        _side_args(a, plan, r0, side_in=side, side_out=side_out, side_x2=side_x2)
    return a


def _layer_fwd_native(plan, x, params, pad_mask, arena, x3, keep_pre, side, side_out, side_x2, split):
    dev, d = x.device, plan.dims
    if split is None:
        parts = [(plan, 0, None)]
    else:                       # two half-batch chains: (plan of half the batch, first row, stream)
        hp = _layer_plan(d.rows // 2, d.D, d.Dff, d.B // 2, d.S, d.heads, (d.M, d.N, d.L), x.dtype, d.act)
        if (d.rows // 2) % 4:   # the second chain's statistics / stream pointers are offset by rows/2 elements: keep them 16-byte aligned
            raise RuntimeError(f"ForwardSplit: (B/2)*S = {d.rows // 2} rows per chain must be a multiple of 4")
        parts = [(hp, 0, None), (hp, d.rows // 2, split.stream)]
    for pl, r0, stream in parts:
        with (torch.cuda.stream(stream) if stream is not None else _NULLCTX):
            a = _layer_fwd_args(plan, pl.dims, x, params, pad_mask, arena, x3, keep_pre, side, side_out, side_x2, r0)
            _call_native("xp_encoder_layer_fwd", a, pl.fwd_ws, dev, "layer_fwd")


# Gradient sinks (distributed.GradBucketReducer(layout_groups=...)): flat fp32 buffers -- slices of the reducer's all-reduce
# buckets -- keyed by the storage of a layer's 16 parameters.  The native layer backward writes its parameter gradients straight
# into the sink instead of a private buffer, so the bucket never needs a pack copy.  Used only while every parameter of the layer
# has ``.grad is None`` (gradient accumulation: the second micro-step must not overwrite what autograd is about to add to) and only
# by the first application of the layer in a backward pass (_claim_sink).
GRAD_SINKS = {}
# One backward pass may hand a sink to ONE layer call only.  A layer applied twice in one graph (VidCLIP.forward's second image /
# caption pass, VidCLIP.py:70-79) backpropagates through both applications before the AccumulateGrad nodes of the shared parameters
# run, so ``p.grad is None`` still holds at the second call: writing the sink again would overwrite the views the first call
# returned and autograd would sum two aliases (2 * g2 instead of g1 + g2).  The claim is keyed by autograd's graph-task id (one id
# per ``backward()`` call), so it needs no reset between steps; the second application gets a private buffer and autograd adds it.
_SINK_CLAIMS = {}


def grad_sink_key(params16):
    return tuple(p.data_ptr() for p in params16)


def _claim_sink(key, sink, numel, device, params):
    """The sink of ``key`` if this layer call may write its gradients straight into it, else None (private buffer).  A sink that
    does not start on a 16-byte boundary is declined: the native layer backward asks
    that of every gradient pointer (include/xpretrain_hip.h, "Pointer alignment"), and a reducer whose bucket holds an odd-sized
    parameter -- the one-element logit_scale -- in front of a layer group puts the group's slice 4 bytes off.  The private buffer
    and the reducer's pack copy take over: the same gradients."""
    if sink is None or sink.numel() != numel or sink.device != device or not all(p.grad is None for p in params):
        return None
    if sink.data_ptr() % 16:
        return None
    task = torch._C._current_graph_task_id()
    if task < 0 or _SINK_CLAIMS.get(key) == task:      # outside a backward pass / second application in this pass
        return None
    _SINK_CLAIMS[key] = task
    return sink


def release_grad_sinks():
    """forget the per-backward sink claims (GradBucketReducer.zero_grad / remove; graph-task ids restart in a new process only,
    so this is hygiene, not a correctness requirement)"""
    _SINK_CLAIMS.clear()


def layer_grad_groups(model):
    """For ``GradBucketReducer(layout_groups=...)``: the 16 parameters of every CLIPEncoderLayer of ``model`` in the order of the
    native layer backward's flat gradient buffer (_LayerPlan.gnames; q / k / v rows of the fused dWqkv and dbqkv in that order)."""
    groups = []
    for m in model.modules():
        if all(hasattr(m, a) for a in ("self_attn", "mlp", "layer_norm1", "layer_norm2")):
            a, f = m.self_attn, m.mlp
            groups.append([m.layer_norm1.weight, m.layer_norm1.bias, a.q_proj.weight, a.k_proj.weight, a.v_proj.weight,
                           a.q_proj.bias, a.k_proj.bias, a.v_proj.bias, a.out_proj.weight, a.out_proj.bias,
                           m.layer_norm2.weight, m.layer_norm2.bias, f.fc1.weight, f.fc1.bias, f.fc2.weight, f.fc2.bias])
    return groups


def _record_sink(ctx, ln1_w, ln1_b, wq, bq, wk, bk, wv, bv, wo, bo, ln2_w, ln2_b, w1, b1, w2, b2):
    """(data-parallel runs only) remember the layer's parameters, in the flat gradient order, for the backward's sink lookup"""
    if GRAD_SINKS:
        ctx.sink_params = (ln1_w, ln1_b, wq, wk, wv, bq, bk, bv, wo, bo, ln2_w, ln2_b, w1, b1, w2, b2)
        ctx.sink_key = grad_sink_key(ctx.sink_params)
    else:
        ctx.sink_params, ctx.sink_key = (), None


def _qkv_grads(dwqkv, dbqkv, need, D):
    """the gradients of wq, bq, wk, bk, wv, bv (forward argument positions 3..8): row slices of the fused dwqkv [3D, D] / dbqkv
    [3D], None for a frozen parameter"""
    pick = lambda t, i, ok: t[i * D:(i + 1) * D] if (t is not None and ok) else None
    return (pick(dwqkv, 0, need[3]), pick(dbqkv, 0, need[4]), pick(dwqkv, 1, need[5]), pick(dbqkv, 1, need[6]),
            pick(dwqkv, 2, need[7]), pick(dbqkv, 2, need[8]))


def _layer_backward(ctx, build, entry, ws_tag, ops, x, *rest, extra=()):
    """The parameter-gradient plumbing of a layer backward and the pass itself: the native call ``entry`` on the argument struct
    ``build(plan, x, *rest, dx, grads)`` (_layer_bwd_args / _pooled_bwd_args) or, where the forward ran op by op, the sequencer
    ``ops`` on the same arguments.  The gradients go to the layer's sink or a private flat buffer (plan.gnames order); a frozen
    parameter has no entry in ``grads`` (natively: its pointer stays NULL).  Returns the 17 leading outputs of the Function's
    backward: dx and the gradients in forward's argument order."""
    plan, dev, need = ctx.plan, x.device, ctx.needs_input_grad
    flat = None
    if GRAD_SINKS and ctx.sink_key is not None and all(need[1:17]):
        flat = _claim_sink(ctx.sink_key, GRAD_SINKS.get(ctx.sink_key), plan.gtotal, dev, ctx.sink_params)
    if flat is None:
        flat = torch.empty(plan.gtotal, dtype=torch.float32, device=dev)
    # forward argument positions: 1,2 ln1 | 3..8 wq,bq,wk,bk,wv,bv | 9,10 wo,bo | 11,12 ln2 | 13,14 w1,b1 | 15,16 w2,b2
    want = dict(dln1_w=need[1], dln1_b=need[2], dwqkv=need[3] or need[5] or need[7], dbqkv=need[4] or need[6] or need[8],
                dwo=need[9], dbo=need[10], dln2_w=need[11], dln2_b=need[12], dw1=need[13], db1=need[14], dw2=need[15], db2=need[16])
    g = {name: t for name, t in zip(plan.gnames, flat.split_with_sizes(plan.gsizes)) if want[name]}
    dx = torch.empty_like(x)
    if ctx.native:
        _call_native(entry, build(plan, x, *rest, dx, g), plan.bwd_ws, dev, ws_tag, *extra)
    else:
        ops(plan, x, *rest, dx, g)
    D, Dff = plan.dims.D, plan.dims.Dff
    gw = lambda n, shape: g[n].view(shape) if n in g else None
    return (dx, g.get("dln1_w"), g.get("dln1_b"), *_qkv_grads(gw("dwqkv", (3 * D, D)), g.get("dbqkv"), need, D),
            gw("dwo", (D, D)), g.get("dbo"), g.get("dln2_w"), g.get("dln2_b"),
            gw("dw1", (Dff, D)), g.get("db1"), gw("dw2", (D, Dff)), g.get("db2"))


# ---- a gradient that is zero outside one row per sample (the contrastive path reads token 0 of the last video layer) ---------------
# GatherRowsFn.backward knows the scatter pattern of the tensor it returns and registers it here; EncoderLayerFn.backward looks its
# incoming gradient up.  The claim is the tensor OBJECT at the version it was registered with: any second consumer of the layer
# output makes autograd sum gradients (a new tensor, or an in-place add that bumps the version), a hook that rewrites the gradient
# returns another tensor, an in-place write bumps the version -- the claim is then gone and the layer runs dense.  No data is read.
_ROW_CLAIMS = {}            # id(tensor) -> (weakref, _version, data_ptr, (B, S, r0))
_SUPPORTS = {}              # (device, layer plan, r0, CU budget) -> _Dx3Support (the lists depend on the shape and the splits only)
sparse_last_bwd_calls = 0   # native layer backward calls that ran over tile lists (tests count them)


def claim_row_support(t, B, S, r0):
    """``t`` ([B*S, D]) is zero outside row ``b*S + r0`` of every sample ``b``."""
    key = id(t)
    _ROW_CLAIMS[key] = (weakref.ref(t, lambda _, key=key: _ROW_CLAIMS.pop(key, None)), t._version, t.data_ptr(), (int(B), int(S), int(r0)))


def row_support_of(t):
    """``(B, S, r0)`` if ``t`` is a tensor claim_row_support registered and nothing has written to it since, else None."""
    c = _ROW_CLAIMS.get(id(t))
    if c is None or c[0]() is not t or c[1] != t._version or c[2] != t.data_ptr():
        return None
    return c[3]


def dx3_tile_lists(B, S, r0, slabs):
    """The tile lists of a [B*S, .] gradient that is zero outside rows ``b*S + r0``: ``(m_tiles, [(k_tiles, k_tile_begin), ...])``,
    one pair per ``(split, k_per_split)`` of ``slabs`` (a split-K weight gradient over those rows; k_per_split a multiple of 64).
    k_tiles: per slab, ascending, the 64-row tiles that hold such a row; a slab with fewer than 2 (the GEMM pipeline's depth) is
    padded with other 64-row tiles of its own range -- first those that share a 256-row tile with a listed one, then the slab's
    first ones.  m_tiles: ascending, every 256-row tile that holds a k-tile of any list (padding included: the rows of a padding tile
    are zero only where they were computed).  Pure host arithmetic."""
    rows = B * S
    active = sorted({(b * S + r0) // 64 for b in range(B)})
    hot = {kt // 4 for kt in active}
    m, lists = set(hot), []
    for split, kps in slabs:
        tiles, begin = [], [0]
        for z in range(split):
            k0, k1 = z * kps // 64, (min((z + 1) * kps, rows) + 63) // 64
            mine = [kt for kt in active if k0 <= kt < k1]
            spare = [kt for kt in range(k0, k1) if kt not in mine]
            spare.sort(key=lambda kt: (kt // 4 not in hot, kt))
            mine = sorted(mine + spare[:max(0, 2 - len(mine))])
            if len(mine) < 2:
                raise ValueError(f"dx3_tile_lists: slab {z} of {split} x {kps} rows has fewer than 2 k-tiles")
            tiles += mine
            begin.append(len(tiles))
        m.update(kt // 4 for kt in tiles)
        lists.append((tiles, begin))
    return sorted(m), lists


class _Dx3Support:
    """XpDx3Support of one (device, shape): the device arrays, the host copies the library validates, the struct itself"""

    def __init__(self, dev, m_tiles, lists, splits):
        put = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
        self.keep = [put(m_tiles)]
        s = self.struct = L.XpDx3Support()
        s.m_tiles, s.n_m_tiles = self.keep[0].data_ptr(), len(m_tiles)
        for w, ((tiles, begin), split) in enumerate(zip(lists, splits)):
            host = (C.c_int32 * len(begin))(*begin)
            self.keep += [put(tiles), put(begin), host]
            s.k_tiles[w], s.k_tile_begin[w], s.k_tile_begin_host[w] = self.keep[-3].data_ptr(), self.keep[-2].data_ptr(), C.addressof(host)
            s.split[w] = split


def _dx3_lists(dims, r0):
    """The host half of _dx3_support: ``(m_tiles, lists, splits)`` of a dense layer of ``dims`` whose dx3 is zero outside row ``r0`` of
    every sample, from the library's own table of the backward's GEMMs (H.layer_bwd_gemms) and their plans; None where one of the
    six is not planned on the 256-wide family or fc1's bias sums are not fused (fp32, small shapes).  No device, no upload."""
    table = H.layer_bwd_gemms(dims)
    dw = [table[i] for i in (L.XP_LAYER_GEMM_DW2, L.XP_LAYER_GEMM_DW1, L.XP_LAYER_GEMM_DWO)]
    plans = [H.gemm_plan_of(g) for g in dw + [table[i] for i in (L.XP_LAYER_GEMM_DPRE, L.XP_LAYER_GEMM_DH2, L.XP_LAYER_GEMM_DATTN)]]
    if not all(p["family"] == L.GEMM_FAMILY_256 for p in plans) or plans[3]["colsum_rows"] <= 0:
        return None
    m_tiles, lists = dx3_tile_lists(dims.B, dims.S, r0, [(p["split"], p["k_per_split"]) for p in plans[:3]])
    return m_tiles, lists, tuple(g.split_k for g in dw)


def _dx3_support(plan, dev, claim):
    """The XpDx3Support (xp_encoder_layer_bwd_listed) of a dense video layer whose dx3 carries ``claim`` = (B, S, r0); None where the
    claim is for another shape or _dx3_lists has none for this one: the layer then runs dense."""
    d = plan.dims
    if claim is None or (claim[0], claim[1]) != (d.B, d.S) or not 0 <= claim[2] < d.S:
        return None
    key = (dev, plan, claim[2], L.lib().xp_get_cu_budget())       # (the CU budget moves the splits)
    if key not in _SUPPORTS:
        if torch.cuda.is_current_stream_capturing():              # (the lists are uploaded with blocking copies: not inside a capture)
            return None
        host = _dx3_lists(d, claim[2])
        _SUPPORTS[key] = None if host is None else _Dx3Support(dev, *host)
    return _SUPPORTS[key]


def _layer_bwd_args(plan, x, params, arena, dx3, pad_mask, side, side_x2, dx, grads):
    a = _layer_args(L.XpLayerBwd, plan, plan.dims, _BWD_PARAMS, params, arena, x=x, dx3=dx3, dx=dx, **grads)
    a.pad_mask = 0 if pad_mask is None else pad_mask.data_ptr()
    if side is not None and side_x2 is not None:          # the forward's fp32 side rows of x and x2: read by the LayerNorm backward passes
        _side_args(a, plan, 0, side_in=side, side_x2=side_x2)
    return a


# ------------------------------------------------------------------------------------------ encoder layer, op by op
# The same entry points in the same order with the same arguments as csrc/layer.hip issues them (XPRETRAIN_DEBUG=op_by_op, or
# arguments the native calls do not take).  The stages the dense and the pooled layer share are written once, as in layer.hip
# (out_proj_mlp_fwd, mlp_out_proj_bwd): out_proj onward over ``n`` rows -- all rows, or the B pooled ones.  Every operator is
# looked up on ``H`` at call time (tools/determinism_hunt.py wraps those attributes).  The four sequencers (_layer_fwd_ops,
# _layer_bwd_ops, _pooled_fwd_ops, _pooled_bwd_ops) take what the native calls take -- the arena (as _piece_views), the outputs, the
# named slices of the flat gradient buffer -- so the Functions save, and _layer_backward plumbs, one thing whoever issues the launches;
# only the workspace temporaries (dpre, dqkv ...) are torch allocations here.
def _attn_front_ops(v, x, ln1_w, ln1_b, Wqkv, bqkv, B, S, heads, size, pad_mask, side, lns):
    """h1 = LN1(x), qkv = h1 Wqkv^T + bqkv (q columns scaled), the fused attention forward: into the buffers ``v`` names (h1, mean1,
    rstd1, qkv, attn_o, stats; one it does not name is allocated).  Returns ``(qkv, stats)``."""
    rows, D = x.shape
    h1, _, _ = H.layernorm_fwd(x, ln1_w, ln1_b, rows, D, x_side=side, side=lns, y=v.get("h1"), mean=v.get("mean1"), rstd=v.get("rstd1"))
    qkv = H.gemm(h1, Wqkv, rows, 3 * D, D, epilogue=L.EPI_BIAS_QSCALE, bias=bqkv, scale=64 ** -0.5, scale_cols=D, out=v.get("qkv"))
    _, stats = H.attn_fwd(qkv, B, S, heads, size=size, pad_mask=pad_mask, out=v.get("attn_o"), stats=v.get("stats"))
    return qkv, stats


def _mlp_fwd_ops(v, p, x, ldr, n, training, side_x, side_x2, side_out, sd, x3, act):
    """x2 = x + attn_o Wo^T + bo (x read with row pitch ``ldr``), x3 = x2 + fc2(act(fc1(LN2(x2)))) over ``n`` rows, from attn_o of the
    saved pieces ``v`` into its x2, h2, mean2, rstd2, act (``training``: and pre) and into ``x3``.  ``p``: the parameters by _FWD_PARAMS name.
    ``sd = (S, M)``: geometry of the fp32 side rows of the n rows (``side_x`` of x, ``side_x2`` / ``side_out`` written), or None.
    ``act``: the activation (L.ACT_*), i.e. which of the two fc1 epilogue kinds runs."""
    D, Dff = p["Wo"].shape[0], p["W1"].shape[0]
    lns = None if sd is None else (sd[0], sd[1], sd[1])
    x2 = H.gemm(v["attn_o"], p["Wo"], n, D, D, epilogue=L.EPI_BIAS_RESID, bias=p["bo"].detach(), resid=x, ldr=ldr, out=v["x2"],
                resid_side=side_x, out_side=side_x2, side=sd)
    h2, _, _ = H.layernorm_fwd(x2, p["ln2_w"], p["ln2_b"], n, D, x_side=side_x2, side=lns, y=v["h2"], mean=v["mean2"], rstd=v["rstd2"])
    a = H.gemm(h2, p["W1"], n, Dff, D, epilogue=L.EPI_ACT_FWD[act], bias=p["b1"].detach(), aux=v["pre"] if training else None,
               out=v["act"])
    H.gemm(a, p["W2"], n, D, Dff, epilogue=L.EPI_BIAS_RESID, bias=p["b2"].detach(), resid=x2, out=x3,
           resid_side=side_x2, out_side=side_out, side=sd)


def _mlp_bwd_ops(v, p, g, dx3, n, defer, db1_fused, side_x2, lns, act):
    """The backward of ``_mlp_fwd_ops`` down to ``dattn = dx2 . Wo``: returns ``(dx2, dattn)`` and writes the gradients ``g`` names
    (final after ``defer.flush()``; without a name a weight's GEMM and fc1's bias sum are skipped, a sum that rides on the LayerNorm
    pass lands in a buffer nobody reads).  ``p``: the parameters by _BWD_PARAMS name.  ``db1_fused``: fc1's bias gradient out of the
    dpre GEMM's epilogue where the library offers it (the dense layer), else always a column-sum pass over dpre (the pooled layer).
    ``act``: the activation (L.ACT_*) whose derivative the dpre epilogue applies."""
    D, Dff = p["Wo"].shape[0], p["W1"].shape[0]
    epi = L.EPI_ACT_BWD[act]
    if "db1" in g and db1_fused:
        dpre, _ = H.gemm(dx3, p["W2"], n, Dff, D, b_kstrided=True, epilogue=epi, resid=v["pre"], colsum_defer=defer,
                         colsum_name="db1", colsum_out=g["db1"])
    else:
        dpre = H.gemm(dx3, p["W2"], n, Dff, D, b_kstrided=True, epilogue=epi, resid=v["pre"])
        if "db1" in g:
            H.colsum_deferred(dpre, n, Dff, defer, name="db1", out=g["db1"])
    if "dw2" in g:
        _wgrad(dx3, v["act"], n, D, Dff, slack=True, out=g["dw2"])
    dh2 = H.gemm(dpre, p["W1"], n, D, Dff, b_kstrided=True)
    if "dw1" in g:
        _wgrad(dpre, v["h2"], n, Dff, D, slack=True, out=g["dw1"])
    # out_proj's bias gradient = column sums of dx2, fc2's = column sums of dx3: both accumulated by the LayerNorm backward
    # that reads dx3 and writes dx2
    dx2 = H.layernorm_bwd(dh2, v["x2"], p["ln2_w"], v["mean2"], v["rstd2"], n, D, dres=dx3, defer=defer, dx_colsum=True,
                          dres_colsum=True, name="ln2", x_side=side_x2, side=lns, dgamma=g.get("dln2_w"), dbeta=g.get("dln2_b"),
                          dx_colsum_out=g.get("dbo"), dres_colsum_out=g.get("db2"))[0]
    dattn = H.gemm(dx2, p["Wo"], n, D, D, b_kstrided=True)
    if "dwo" in g:
        _wgrad(dx2, v["attn_o"], n, D, D, slack=True, out=g["dwo"])
    return dx2, dattn


def _layer_fwd_ops(plan, x, params, pad_mask, arena, x3, training, side, side_out, side_x2):
    """xp_encoder_layer_fwd, op by op"""
    d = plan.dims
    v, p = _piece_views(plan, arena), dict(zip(_FWD_PARAMS, params))
    sd, lns = (None, None) if side is None else ((plan.side_S, plan.side_M), (plan.side_S, plan.side_M, plan.side_M))
    if side is not None and side_x2 is None:       # a forward-only pass: nobody keeps the x2 side rows (natively: in the workspace)
        side_x2 = torch.empty_like(side)
    _attn_front_ops(v, x, p["ln1_w"], p["ln1_b"], p["Wqkv"], p["bqkv"], d.B, d.S, d.heads, plan.size, pad_mask, side, lns)
    _mlp_fwd_ops(v, p, x, None, d.rows, training, side, side_x2, side_out, sd, x3, d.act)


def _layer_bwd_ops(plan, x, params, arena, dx3, pad_mask, side, side_x2, dx, g):
    """xp_encoder_layer_bwd, op by op"""
    d = plan.dims
    rows, D = d.rows, d.D
    v, p = _piece_views(plan, arena), dict(zip(_BWD_PARAMS, params))
    lns = None if side is None else (plan.side_S, plan.side_M, plan.side_M)
    defer = H.DeferredReduce(x.device)       # the 4 bias + 4 LayerNorm-parameter reductions finish in 2 launches
    # ---- MLP: x3 = x2 + fc2(act(fc1(LN2(x2)))), then dattn = dx2 . Wo
    dx2, dattn = _mlp_bwd_ops(v, p, g, dx3, rows, defer, True, side_x2, lns, d.act)
    # ---- attention: x2 = x + out_proj(attn(qkv(LN1(x))))
    # the q/k/v bias gradients (column sums of dqkv) come out of the attention backward kernels: ``(dqkv, sums)`` with ``colsum_defer``
    dbqkv = g.get("dbqkv")
    dqkv = H.attn_bwd(v["qkv"], v["attn_o"], dattn, v["stats"], d.B, d.S, d.heads, size=plan.size, pad_mask=pad_mask,
                      q_scale=64 ** -0.5, colsum_defer=None if dbqkv is None else defer, colsum_name="dbqkv", colsum_out=dbqkv)
    dqkv = dqkv if dbqkv is None else dqkv[0]
    dh1 = H.gemm(dqkv, p["Wqkv"], rows, D, 3 * D, b_kstrided=True)
    if "dwqkv" in g:
        _wgrad(dqkv, v["h1"], rows, 3 * D, D, out=g["dwqkv"])
    H.layernorm_bwd(dh1, x, p["ln1_w"], v["mean1"], v["rstd1"], rows, D, dres=dx2, dx=dx, defer=defer, name="ln1", x_side=side,
                    side=lns, dgamma=g.get("dln1_w"), dbeta=g.get("dln1_b"))
    defer.flush()


# ---- what EncoderLayerFn and PooledEncoderLayerFn share ---------------------------------------------------------------------------
def _check_layer_args(name, x, heads, act, side, side_rows, side_what):
    if act not in (L.ACT_QUICK_GELU, L.ACT_GELU):
        raise ValueError(f"{name}: act={act!r} is not one of {L.ACTS}")
    if side is not None and (x.dtype != torch.bfloat16 or side.dtype != torch.float32 or not side.is_contiguous() or side.device != x.device
                             or tuple(side.shape) != (side_rows, x.shape[1])):
        raise TypeError(f"{name}: side rows must be a contiguous fp32 {side_what} tensor beside a bf16 stream")
    if x.shape[1] // heads != 64:
        raise RuntimeError(f"xpretrain_amd attention kernels are built for head_dim 64, got {x.shape[1] // heads}")


def _compute_weights(dt, wq, bq, wk, bk, wv, bv, wo, w1, w2):
    """``(Wqkv, bqkv, Wo, W1, W2)``: the fused q/k/v operand and the other weights in the compute dtype (WeightCache)"""
    get = WEIGHTS.get
    return WEIGHTS.fused((wq, wk, wv), dt), WEIGHTS.fused((bq, bk, bv), torch.float32), get(wo, dt), get(w1, dt), get(w2, dt)


def _layer_outputs(ctx, x3, side_out):
    if side_out is None:
        return x3
    ctx.mark_non_differentiable(side_out)
    ctx.set_materialize_grads(False)       # no zero-filled "gradient" of the side rows in the backward
    return x3, side_out


def _check_dx3(name, dx3, x, shape):
    if dx3.dtype != x.dtype or dx3.device != x.device or tuple(dx3.shape) != tuple(shape):
        raise TypeError(f"{name}.backward: incoming gradient is {dx3.dtype} {tuple(dx3.shape)} on {dx3.device}, "
                        f"expected {x.dtype} {tuple(shape)} on {x.device}")
    return dx3.contiguous()


class EncoderLayerFn(torch.autograd.Function):
    """CLIPEncoderLayer.forward (modeling/CLIP_ViP.py:444-460) with CLIPAttention.forward2 (:332-381, video
    tower, ``size=(M,N,L)``) or CLIPAttention.forward (:266-330, text tower, causal + padding) and CLIPMLP
    (:392-396)."""

    @staticmethod
    def forward(ctx, x, ln1_w, ln1_b, wq, bq, wk, bk, wv, bv, wo, bo, ln2_w, ln2_b, w1, b1, w2, b2,
                B: int, S: int, heads: int, size: Optional[Tuple[int, int, int]], pad_mask: Optional[torch.Tensor],
                training: bool = True, side: Optional[torch.Tensor] = None, split: Optional["ForwardSplit"] = None,
                act: int = L.ACT_QUICK_GELU):
        """``act``: the MLP's activation (L.ACTS[config.hidden_act]).
        ``side`` (fp32, bf16 compute only): the fp32 side rows of ``x`` (SideRows, csrc/gemm_common.h) -- [B*M, D], the proxy rows of
        every sample, in the video tower; [B*S, D], the whole stream, in the text tower.  The call then returns ``(x3, side_out)``."""
        dt = x.dtype
        _check_layer_args("EncoderLayerFn", x, heads, act, side, B * size[0] if size is not None else B * S,
                          "[B*M, D] (video) / [B*S, D] (text)")
        rows, D = x.shape
        Dff = w1.shape[0]
        casts0 = WEIGHTS.casts
        Wqkv, bqkv, Wo, W1, W2 = _compute_weights(dt, wq, bq, wk, bk, wv, bv, wo, w1, w2)
        params = (ln1_w, ln1_b, Wqkv, bqkv, Wo, bo, ln2_w, ln2_b, W1, b1, W2, b2)          # (_FWD_PARAMS)
        plan = _layer_plan(rows, D, Dff, B, S, heads, size, dt, act)
        arena = torch.empty(plan.arena_bytes, dtype=torch.uint8, device=x.device)
        x3 = torch.empty_like(x)
        side_out = None if side is None else torch.empty_like(side)
        side_x2 = torch.empty_like(side) if side is not None and training else None      # kept for the backward's second LayerNorm
        ctx.plan, ctx.native = plan, LAYER_CALLS and _native_ok(x, params, pad_mask)      # (native: who issues both passes' launches)
        if ctx.native:
            if split is not None and (size is None or B % 2 or pad_mask is not None):
                split = None
            if split is not None and WEIGHTS.casts != casts0:       # a weight copy was (re)made on this stream just now: the second
                split.stream.wait_stream(torch.cuda.current_stream())   # chain must not read it before the cast has run
            _layer_fwd_native(plan, x, params, pad_mask, arena, x3, training, side, side_out, side_x2, split)
            if split is not None:
                split.hold(x, arena, x3, side, side_out, side_x2)
        else:
            _layer_fwd_ops(plan, x, params, pad_mask, arena, x3, training, side, side_out, side_x2)
        ctx.save_for_backward(x, arena, ln1_w, ln2_w, Wqkv, Wo, W1, W2, pad_mask, side, side_x2)
        _record_sink(ctx, ln1_w, ln1_b, wq, bq, wk, bk, wv, bv, wo, bo, ln2_w, ln2_b, w1, b1, w2, b2)
        return _layer_outputs(ctx, x3, side_out)

    @staticmethod
    def backward(ctx, dx3, _dside=None):
        if dx3 is None:             # (set_materialize_grads(False): the layer output did not reach the loss)
            return (None,) * 26
        x, arena, *params, pad_mask, side, side_x2 = ctx.saved_tensors          # (params: _BWD_PARAMS)
        claim = row_support_of(dx3)
        dx3 = _check_dx3("EncoderLayerFn", dx3, x, x.shape)
        entry, extra = "xp_encoder_layer_bwd", ()
        if SPARSE_LAST_BWD and ctx.native and ctx.plan.size is not None and claim is not None:
            # (video tower, native path: the op-by-op path stays dense on purpose -- it is the bit reference)
            support = _dx3_support(ctx.plan, x.device, claim)
            if support is not None:
                global sparse_last_bwd_calls
                sparse_last_bwd_calls += 1
                entry, extra = "xp_encoder_layer_bwd_listed", (C.byref(support.struct),)
        return _layer_backward(ctx, _layer_bwd_args, entry, "layer_bwd", _layer_bwd_ops, x, params, arena, dx3,
                               pad_mask, side, side_x2, extra=extra) + (None,) * 9


# ------------------------------------------------------------------------------------------ pooled last layer (video tower)
class _PooledLayerPlan:
    """Sizes / offsets of one (shape, dtype) of the pooled last layer (xp_encoder_layer_pooled_fwd / _bwd), as _LayerPlan: the table
    holds the every-row pieces (h1, kv, LayerNorm-1 statistics), then the pooled rows' pieces ([B, .])."""

    def __init__(self, rows, D, Dff, B, S, heads, size, dtype, act=L.ACT_QUICK_GELU):
        rD, rF = D * _ES[dtype], Dff * _ES[dtype]
        _finish_plan(self, _layer_plan(rows, D, Dff, B, S, heads, size, dtype, act).dims, dtype,
                     (("h1", rows, rD), ("kv", rows, 2 * rD), ("mean1", rows, 4), ("rstd1", rows, 4), ("h1p", B, rD), ("q", B, rD),
                      ("attn_o", B, rD), ("x2", B, rD), ("h2", B, rD), ("pre", B, rF), ("act", B, rF), ("mean1p", B, 4),
                      ("rstd1p", B, 4), ("mean2", B, 4), ("rstd2", B, 4), ("stats", B, heads * 2 * 4)),
                     ("xp_encoder_layer_pooled_fwd_workspace_bytes", "xp_encoder_layer_pooled_bwd_workspace_bytes"))


def _pooled_plan(rows, D, Dff, B, S, heads, size, dtype, act=L.ACT_QUICK_GELU) -> _PooledLayerPlan:
    key = ("pooled", rows, D, Dff, B, S, heads, size, dtype, act)
    p = _PLANS.get(key)
    if p is None:
        p = _PLANS[key] = _PooledLayerPlan(rows, D, Dff, B, S, heads, size, dtype, act)
    return p


def _pooled_fwd_args(plan, x, params, arena, x3, keep_pre, side, side_out, side_x2):
    return _layer_args(L.XpLayerPooledFwd, plan, plan.dims, _FWD_PARAMS, params, arena, keep_pre=keep_pre, x=x, x3=x3,
                       side_in=side, side_out=side_out, side_x2=side_x2)


def _pooled_bwd_args(plan, x, params, arena, dx3, side, side_x2, dx, grads):
    return _layer_args(L.XpLayerPooledBwd, plan, plan.dims, _BWD_PARAMS, params, arena, x=x, dx3=dx3, dx=dx, side_in=side,
                       side_x2=side_x2, **grads)


def _pooled_fwd_ops(plan, x, params, arena, x3, training, side, side_out, side_x2):
    """xp_encoder_layer_pooled_fwd, op by op"""
    d = plan.dims
    rows, D, B, S, M = d.rows, d.D, d.B, d.S, d.M
    v, p = _piece_views(plan, arena), dict(zip(_FWD_PARAMS, params))
    Wqkv, bqkv = p["Wqkv"], p["bqkv"]
    lns, p1, sd = (None, None, None) if side is None else ((S, M, M), (1, 1, 1), (1, 1))
    h1, _, _ = H.layernorm_fwd(x, p["ln1_w"], p["ln1_b"], rows, D, x_side=side, side=lns, y=v["h1"], mean=v["mean1"], rstd=v["rstd1"])
    side0 = None if side is None else H.gather_rows(side, None, B, M, D)
    h1p, _, _ = H.layernorm_fwd(x, p["ln1_w"], p["ln1_b"], B, D, ldx=S * D, x_side=side0, side=p1, y=v["h1p"], mean=v["mean1p"],
                                rstd=v["rstd1p"])
    kv = H.gemm(h1, Wqkv[D:], rows, 2 * D, D, epilogue=L.EPI_BIAS, bias=bqkv[D:], out=v["kv"])
    q = H.gemm(h1p, Wqkv, B, D, D, epilogue=L.EPI_BIAS_QSCALE, bias=bqkv, scale=64 ** -0.5, scale_cols=D, out=v["q"])
    H.attn_pooled_fwd(q, kv, B, S, d.heads, out=v["attn_o"], stats=v["stats"])
    _mlp_fwd_ops(v, p, x, S * D, B, training, side0, side_x2, side_out, sd, x3, d.act)


def _pooled_bwd_ops(plan, x, params, arena, dx3, side, side_x2, dx, g):
    """xp_encoder_layer_pooled_bwd, op by op"""
    d = plan.dims
    rows, D, B, S, M = d.rows, d.D, d.B, d.S, d.M
    v, p = _piece_views(plan, arena), dict(zip(_BWD_PARAMS, params))
    Wqkv, dbqkv = p["Wqkv"], g.get("dbqkv")
    lns, p1 = (None, None) if side is None else ((S, M, M), (1, 1, 1))
    defer = H.DeferredReduce(x.device)
    # ---- MLP and dattn = dx2 . Wo on the pooled rows
    dx2, dattn = _mlp_bwd_ops(v, p, g, dx3, B, defer, False, side_x2, p1, d.act)
    # ---- attention.  dqkv [rows, 3D]: dk / dv in the k / v columns of every row, dq in the q columns of the pooled rows only
    dqkv = torch.empty((rows, 3 * D), dtype=x.dtype, device=x.device)
    dq_view, dkv = dqkv.view(B, S * 3 * D)[:, :D], dqkv[:, D:]
    # (the k / v bias gradients come out of the attention backward kernel; without ``colsum_defer`` it gets no partial rows)
    H.attn_pooled_bwd(v["q"], v["kv"], v["attn_o"], dattn, v["stats"], B, S, d.heads, q_scale=64 ** -0.5, dq=dq_view, dkv=dkv,
                      colsum_defer=None if dbqkv is None else defer, colsum_name="dbkv", colsum_out=None if dbqkv is None else dbqkv[D:])
    dh1 = H.gemm(dkv, Wqkv[D:], rows, D, 2 * D, lda=3 * D, b_kstrided=True, ldb=D)
    H.gemm(dqkv, Wqkv, B, D, 3 * D, b_kstrided=True, ldb=D, a_remap=(1, S, 0), c_remap=(1, S, 0), out=dh1)
    if "dwqkv" in g:
        dwqkv = g["dwqkv"].view(3 * D, D)
        _wgrad(dqkv, v["h1p"], B, D, D, a_remap=(1, S, 0), slack=True, lddy=3 * D, out=dwqkv[:D])
        _wgrad(dkv, v["h1"], rows, 2 * D, D, lddy=3 * D, out=dwqkv[D:])
    if dbqkv is not None:
        H.colsum_deferred(dqkv, B, D, defer, ldx=S * 3 * D, name="dbq", out=dbqkv)
    H.layernorm_bwd(dh1, x, p["ln1_w"], v["mean1"], v["rstd1"], rows, D, dx=dx, defer=defer, name="ln1", x_side=side, side=lns,
                    dgamma=g.get("dln1_w"), dbeta=g.get("dln1_b"))
    # the pooled rows once more, with their residual gradient (the parameter-gradient partial rows of this pass are dropped)
    H.layernorm_bwd(dh1, x, p["ln1_w"], v["mean1p"], v["rstd1p"], B, D, ldx=S * D, lddy=S * D, dres=dx2, dx=dx, lddx=S * D, defer=defer,
                    param_grads=False, name="ln1_pooled", x_side=side, side=(1, 1, M))
    defer.flush()


class PooledEncoderLayerFn(torch.autograd.Function):
    """The LAST CLIPEncoderLayer of the video tower when only the pooled feature leaves it (``pooled_output =
    last_hidden_state[:, 0]``, modeling/CLIP_ViP.py:360-366): returns row ``b*S`` of ``EncoderLayerFn``'s output for every sample
    -- ``[B, D]`` (and, with ``side``, those rows in fp32) -- computed without the dead rows.  LayerNorm 1 and the K/V projection
    see every row (token 0 is a proxy row: it attends all S keys, CLIPAttention.forward2); the Q projection, the single-query
    attention (csrc/attention_pooled.hip), out_proj, LayerNorm 2 and the MLP run on B rows.  The backward's ``dx`` is dense and
    every parameter receives its gradient.  Exactly the function of the dense layer, not bit-equal to it in bf16: the dense
    attention rounds P and dS to bf16 as matrix-core operands, the single-query kernel keeps them in fp32."""

    @staticmethod
    def forward(ctx, x, ln1_w, ln1_b, wq, bq, wk, bk, wv, bv, wo, bo, ln2_w, ln2_b, w1, b1, w2, b2,
                B: int, S: int, heads: int, size: Tuple[int, int, int], training: bool = True, side: Optional[torch.Tensor] = None,
                act: int = L.ACT_QUICK_GELU):
        dt = x.dtype
        rows, D = x.shape
        M = size[0]
        _check_layer_args("PooledEncoderLayerFn", x, heads, act, side, B * M, "[B*M, D]")
        Dff = w1.shape[0]
        if M < 1 or S != M + size[1] * size[2] or rows != B * S:
            raise RuntimeError(f"PooledEncoderLayerFn: token 0 must be a proxy row of a [B*S, D] stream (size={size}, S={S}, rows={rows})")
        Wqkv, bqkv, Wo, W1, W2 = _compute_weights(dt, wq, bq, wk, bk, wv, bv, wo, w1, w2)
        dev = x.device
        x3 = torch.empty((B, D), dtype=dt, device=dev)
        side_out = side_x2 = None
        if side is not None:
            side_out = torch.empty((B, D), dtype=torch.float32, device=dev)
            side_x2 = torch.empty((B, D), dtype=torch.float32, device=dev)
        params = (ln1_w, ln1_b, Wqkv, bqkv, Wo, bo, ln2_w, ln2_b, W1, b1, W2, b2)          # (_FWD_PARAMS)
        plan = _pooled_plan(rows, D, Dff, B, S, heads, tuple(size), dt, act)
        arena = torch.empty(plan.arena_bytes, dtype=torch.uint8, device=dev)
        ctx.plan, ctx.native = plan, LAYER_CALLS and _native_ok(x, params, None)
        if ctx.native:
            a = _pooled_fwd_args(plan, x, params, arena, x3, training, side, side_out, side_x2)
            _call_native("xp_encoder_layer_pooled_fwd", a, plan.fwd_ws, dev, "layer_pooled_fwd")
        else:
            _pooled_fwd_ops(plan, x, params, arena, x3, training, side, side_out, side_x2)
        ctx.save_for_backward(x, arena, ln1_w, ln2_w, Wqkv, Wo, W1, W2, side, side_x2)
        _record_sink(ctx, ln1_w, ln1_b, wq, bq, wk, bk, wv, bv, wo, bo, ln2_w, ln2_b, w1, b1, w2, b2)
        return _layer_outputs(ctx, x3, side_out)

    @staticmethod
    def backward(ctx, dx3, _dside=None):
        if dx3 is None:
            return (None,) * 24
        x, arena, *params, side, side_x2 = ctx.saved_tensors          # (params: _BWD_PARAMS)
        dx3 = _check_dx3("PooledEncoderLayerFn", dx3, x, (ctx.plan.dims.B, x.shape[1]))
        return _layer_backward(ctx, _pooled_bwd_args, "xp_encoder_layer_pooled_bwd", "layer_pooled_bwd", _pooled_bwd_ops, x, params,
                               arena, dx3, side, side_x2) + (None,) * 7


def pooled_encoder_layer(x, layer, B, S, heads, size, side=None):
    """Apply ``PooledEncoderLayerFn`` with the parameters of a ``CLIPEncoderLayer`` module: ``[B, D]`` (with ``side``: also the fp32
    rows)."""
    return PooledEncoderLayerFn.apply(x, *_layer_params(layer), B, S, heads, tuple(size), torch.is_grad_enabled(), side, _layer_act(layer))


# ------------------------------------------------------------------------------------------ fp32 side rows (proxy tokens)
# XPRETRAIN_PROXY_FP32=1 (default): the video tower's M proxy tokens of every sample keep their residual stream in fp32 beside the
# bf16 rows ([B*M, D] fp32 "side rows": read by the LayerNorms, read / written by the residual GEMM epilogues).  Measured with the
# oracle's storage emulation (tools/residual_precision_experiment.py): |loss - fp32 reference| at configs[1] batch 2 drops from
# 4.4e-2 to 5.6e-3, the feature error halves -- the same as a fully fp32 residual stream, for 4 of 2356 rows.
PROXY_SIDE = os.environ.get("XPRETRAIN_PROXY_FP32", "1") != "0"


def proxy_side_rows(class_emb, added_cls, pos_w, B: int, M: int) -> torch.Tensor:
    """[B*M, D] fp32: class_embedding / added_cls + position_embedding[0] (CLIP_ViP.py:187-191), exact"""
    D = class_emb.shape[0]
    side = torch.empty((B * M, D), dtype=torch.float32, device=class_emb.device)
    return H.vip_proxy_rows(class_emb.detach(), added_cls.detach().contiguous(), pos_w.detach().contiguous(), side, B, M, M, D)


def with_side_rows(x: torch.Tensor, side: Optional[torch.Tensor], B: int, S: int) -> torch.Tensor:
    """hidden state for ``output_hidden_states``: with side rows, an fp32 copy of x whose proxy rows are the exact fp32 ones"""
    if side is None:
        return x
    D = x.shape[1]
    h = x.detach().float()
    h.view(B, S, D)[:, :side.shape[0] // B] = side.view(B, -1, D)      # (text tower: the side rows are the whole stream)
    return h


# False: always materialise the patch matrix instead of gathering it in the GEMM loader (module attribute: tests compare the two)
PATCH_GATHER = True


# ------------------------------------------------------------------------------------------ embeddings
class VisionEmbedFn(torch.autograd.Function):
    """CLIPVisionViPEmbeddings.forward (modeling/CLIP_ViP.py:168-197): conv patch embed as im2col + MFMA GEMM
    whose epilogue adds temporal[t] + position[1+l] and writes straight into token slot M + t*L + l; proxy rows
    (class_embedding / added_cls + position[0]) by a small fill kernel.  ``time_table`` is the [T,D] temporal
    table (already interpolated by the caller when T != temporal_size, :171-174)."""

    @staticmethod
    def forward(ctx, video, patch_w, class_emb, added_cls, pos_w, time_table, dtype, want_wgrad=True):
        """``want_wgrad``: the caller's ``torch.is_grad_enabled() and patch_w.requires_grad`` (grad mode is off inside
        Function.forward, and ``ctx.needs_input_grad`` ignores ``torch.no_grad()``): False lets the loader gather the patches."""
        Bv, T, Cc, Hh, Ww = video.shape
        D, _, P, _ = patch_w.shape
        gh, gw = Hh // P, Ww // P
        Lp = gh * gw
        M = 1 + added_cls.shape[0]
        S = M + T * Lp
        if pos_w.shape[0] != 1 + Lp:
            raise ValueError(f"position_embedding has {pos_w.shape[0]} rows but the frame has {Lp} patches (+1)")
        K = 3 * P * P
        frames = video.reshape(Bv * T, Cc, Hh, Ww).contiguous()
        if frames.dtype != torch.uint8:
            frames = frames.float()
        Wp = WEIGHTS.get(patch_w, dtype).view(D, K)
        x = torch.empty((Bv * S, D), dtype=dtype, device=video.device)
        pos = pos_w.detach().contiguous()
        tt = time_table.detach().contiguous().float()
        # The patch matrix is only materialised when the backward needs it (dW of the patch embedding reads it k-strided).  A pass
        # that does not (inference, a frozen patch embedding) lets the GEMM's operand loader gather the 8-pixel strips straight from
        # [BT,3,H,W] (XpGemmDesc::a_frames): same bf16 operand values, no im2col round trip.
        need_patches = bool(want_wgrad) and ctx.needs_input_grad[1]
        on_the_fly = (not need_patches and PATCH_GATHER and dtype == torch.bfloat16 and P % 8 == 0 and Ww % 8 == 0)
        patches = None
        if on_the_fly:
            H.gemm(None, Wp, Bv * T * Lp, D, K, out=x, epilogue=L.EPI_PATCH, tab1=tt, tab2=pos[1:], tab_L=Lp, c_remap=(T * Lp, S, M),
                   frames=frames, frame_patch=P, frame_norm=(H.CLIP_MEAN, H.CLIP_STD) if frames.dtype == torch.uint8 else None)
        else:
            if frames.dtype == torch.uint8:     # decoded frames: /255, CLIP mean/std and the cast happen inside the gather
                patches = H.im2col_u8(frames, P, dtype)
            else:
                patches = H.im2col(frames, P, dtype)
            H.gemm(patches, Wp, Bv * T * Lp, D, K, out=x, epilogue=L.EPI_PATCH, tab1=tt, tab2=pos[1:], tab_L=Lp,
                   c_remap=(T * Lp, S, M))
        H.vip_proxy_rows(class_emb.detach(), added_cls.detach().contiguous(), pos, x, Bv, S, M, D)
        ctx.save_for_backward(patches)
        ctx.meta = (Bv, T, Lp, M, S, D, K, tuple(patch_w.shape), added_cls.shape[0])
        return x

    @staticmethod
    def backward(ctx, dx):
        (patches,) = ctx.saved_tensors
        Bv, T, Lp, M, S, D, K, wshape, nadd = ctx.meta
        dx = dx.contiguous()
        d_class, d_added, d_pos, d_time = H.vip_embed_bwd(dx, Bv, M, T, Lp, D)
        dwp = None if patches is None else _wgrad(dx, patches, Bv * T * Lp, D, K, a_remap=(T * Lp, S, M)).view(wshape)
        return None, dwp, d_class, d_added[:nadd], d_pos, d_time, None, None


class PosResampleFn(torch.autograd.Function):
    """``interpolate_pos_encoding`` (transformers' CLIPVisionEmbeddings): the position table [1 + g0*g0, D] resampled to the frame's
    gh x gw patch grid -- row 0 copied, the grid bicubic -- as the table VisionEmbedFn then reads; the backward is the transposed
    map, in a fixed summation order, onto the parameter's own shape.  Callers skip it on the native grid (``pos_table``)."""

    @staticmethod
    def forward(ctx, pos_w, gh, gw):
        ctx.meta = (H.pos_grid(pos_w.shape[0]), gh, gw)
        return H.pos_resample_fwd(pos_w.detach().contiguous(), gh, gw)

    @staticmethod
    def backward(ctx, d_out):
        return H.pos_resample_bwd(d_out.contiguous(), *ctx.meta), None, None


def pos_table(pos_w, gh: int, gw: int):
    """the position table of a gh x gw patch grid: the parameter itself on its own grid (no kernel, no autograd node), else resampled"""
    if gh < 1 or gw < 1:
        raise ValueError(f"interpolate_pos_encoding: the frame is smaller than one patch (grid {gh} x {gw})")
    g0 = H.pos_grid(pos_w.shape[0])
    return pos_w if gh == gw == g0 else PosResampleFn.apply(pos_w, gh, gw)


class TextEmbedFn(torch.autograd.Function):
    """CLIPTextEmbeddings.forward (modeling/CLIP_ViP.py:210-227): token_embedding[ids] + position_embedding[:Lt]."""

    @staticmethod
    def forward(ctx, ids, tok_w, pos_w, dtype):
        ids = ids.contiguous()
        x = H.text_embed_fwd(ids, tok_w.detach(), pos_w.detach(), dtype)
        ctx.save_for_backward(ids)
        ctx.meta = (tok_w.shape[0], pos_w.shape[0])
        return x

    @staticmethod
    def backward(ctx, dx):
        (ids,) = ctx.saved_tensors
        d_tok, d_pos = H.text_embed_bwd(ids, dx.contiguous(), *ctx.meta)
        return None, d_tok, d_pos, None


class TextEmbedPosFn(torch.autograd.Function):
    """CLIPTextEmbeddings.forward with caller-given ``position_ids`` (modeling/CLIP_ViP.py:221-227):
    token_embedding[ids] + position_embedding[pos_ids], ``pos_ids`` int64 ``[1 | B, Lt]`` on the GPU.  The position table's gradient
    is a scatter with repeated indices, summed by the kernel in row order (bit-reproducible); ids equal to ``arange(Lt)`` give
    TextEmbedFn's bits, forward and backward."""

    @staticmethod
    def forward(ctx, ids, pos_ids, tok_w, pos_w, dtype):
        ids, pos_ids = ids.contiguous(), pos_ids.contiguous()
        x = H.text_embed_fwd_pos(ids, pos_ids, tok_w.detach(), pos_w.detach(), dtype)
        ctx.save_for_backward(ids, pos_ids)
        ctx.meta = (tok_w.shape[0], pos_w.shape[0])
        return x

    @staticmethod
    def backward(ctx, dx):
        ids, pos_ids = ctx.saved_tensors
        d_tok, d_pos = H.text_embed_bwd_pos(ids, pos_ids, dx.contiguous(), *ctx.meta)
        return None, None, d_tok, d_pos, None


# ------------------------------------------------------------------------------------------ small blocks
class LayerNormFn(torch.autograd.Function):
    """nn.LayerNorm (pre_layrnorm :881, post_layernorm :893, final_layer_norm :772)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, x_side=None, side=None, want_y_side=False):
        """``x_side`` (fp32) with ``side = (S, M, stride)``: rows r with r % S < M are read from x_side (fp32 side rows of the
        residual stream); ``want_y_side``: their fp32 result is returned too (``(y, y_side)``, y_side laid out like x_side)."""
        rows, D = x.shape
        y_side = torch.empty_like(x_side) if want_y_side else None
        y, mean, rstd = H.layernorm_fwd(x, gamma.detach(), beta.detach(), rows, D, x_side=x_side, y_side=y_side, side=side)
        ctx.save_for_backward(x, gamma, mean, rstd, x_side)
        ctx.side = side
        if want_y_side:
            ctx.mark_non_differentiable(y_side)
            ctx.set_materialize_grads(False)
            return y, y_side
        return y

    @staticmethod
    def backward(ctx, dy, _dys=None):
        if dy is None:
            return (None,) * 6
        x, gamma, mean, rstd, x_side = ctx.saved_tensors
        rows, D = x.shape
        dx, dg, db = H.layernorm_bwd(dy.contiguous(), x, gamma.detach(), mean, rstd, rows, D, x_side=x_side, side=ctx.side)
        return dx, dg, db, None, None, None


class GatherRowsFn(torch.autograd.Function):
    """pooled[b] = x[b, idx[b]]  (EOT-argmax pooling :776; idx=None -> token 0, the class proxy, :892)."""

    @staticmethod
    def forward(ctx, x, idx, B, S):
        D = x.shape[1]
        ctx.save_for_backward(idx)
        ctx.meta = (B, S, D)
        return H.gather_rows(x, idx, B, S, D)

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        B, S, D = ctx.meta
        dx = H.scatter_rows(dout.contiguous(), idx, B, S, D)
        if idx is None:             # token 0 of every sample: a host-known pattern (an EOS index is data: no claim)
            claim_row_support(dx, B, S, 0)
        return dx, None, None, None


class ProjectionFn(torch.autograd.Function):
    """bias-free nn.Linear: visual_projection / text_projection (:1142,:1145)."""

    @staticmethod
    def forward(ctx, x, w):
        rows, K = x.shape
        N = w.shape[0]
        Wc = WEIGHTS.get(w, x.dtype)
        ctx.save_for_backward(x, Wc)
        return H.gemm(x, Wc, rows, N, K)

    @staticmethod
    def backward(ctx, dy):
        x, Wc = ctx.saved_tensors
        rows, K = x.shape
        N = Wc.shape[0]
        dy = dy.contiguous()
        dx = H.gemm(dy, Wc, rows, K, N, b_kstrided=True)
        dw = _wgrad(dy, x, rows, N, K)
        return dx, dw


class L2NormFn(torch.autograd.Function):
    """x / ||x||_2 (:1148-1149); fp32 unit-norm features out."""

    @staticmethod
    def forward(ctx, x):
        rows, D = x.shape
        y, inv = H.l2norm_fwd(x, rows, D)
        ctx.save_for_backward(y, inv)
        ctx.dtype = x.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        y, inv = ctx.saved_tensors
        rows, D = y.shape
        return H.l2norm_bwd(dy.contiguous().float(), y, inv, rows, D, ctx.dtype)


_sim = H.sim_matrix      # a . b^T in fp32 through xp_sim_matrix (csrc/small_gemm.hip) -- the package launches no vendor GEMM


class SimLogitsFn(torch.autograd.Function):
    """``logits_per_text = text_embeds @ image_embeds.T * logit_scale.exp()`` (CLIP_ViP.py:1151-1153) of ``CLIPModel.forward``:
    a [B, B] fp32 product that VidCLIP never reads (modeling/CLIP_ViP.py resolves it on access).  Forward and both input gradients
    are products of the same small-matrix kernel."""

    @staticmethod
    def forward(ctx, text, image, log_scale):
        scale = log_scale.detach().float().exp()
        logits = _sim(text, image) * scale
        ctx.save_for_backward(text, image, logits, scale)
        return logits

    @staticmethod
    def backward(ctx, g):
        text, image, logits, scale = ctx.saved_tensors
        g = g.contiguous().float()
        gs = g * scale
        dt = _sim(gs, image.float().t()).to(text.dtype) if ctx.needs_input_grad[0] else None         # [n, m] . [m, d]
        di = _sim(gs.t(), text.float().t()).to(image.dtype) if ctx.needs_input_grad[1] else None     # [m, n] . [n, d]
        dls = (g * logits).sum().reshape(()) if ctx.needs_input_grad[2] else None                     # d/d log_scale of s * e^ls
        return dt, di, dls


class _FusedLossFn(torch.autograd.Function):
    """A loss whose library call produces the loss and its gradients in one pass; backward only applies the incoming scalar.
    A subclass's forward returns ``_keep(ctx, loss, slots)``, ``slots`` holding one entry per forward argument: its gradient, or
    ``None`` (an argument that is no tensor, or an operand the loss does not read)."""

    @staticmethod
    def _keep(ctx, loss, slots):
        ctx.has = [g is not None for g in slots]
        ctx.save_for_backward(*[g for g in slots if g is not None])
        return loss

    @staticmethod
    def backward(ctx, g):
        saved = iter(ctx.saved_tensors)
        return tuple(next(saved) * g if h else None for h in ctx.has)


class ContrastiveLossFn(_FusedLossFn):
    """Any loss of the learnable-temperature family (optimization/loss.py:126-324) by its ``XP_LOSS_*`` kind; loss and
    gradients in one kernel pass.  An operand the kind does not read gets no gradient (``None``): with ``vs_vc`` / ``vsc`` the
    frame pass of the video tower has no backward at all, as in the reference."""

    @staticmethod
    def forward(ctx, kind, vis, txt, img, cap, log_scale):
        def f(t):
            return None if t is None else t.contiguous().float()
        loss, *grads = H.contrastive_loss(kind, f(vis), f(txt), f(img), f(cap), log_scale=log_scale.detach().float().reshape(()))
        return _FusedLossFn._keep(ctx, loss, (None, *grads))


class PairLossFn(_FusedLossFn):
    """One of the fixed-temperature losses (optimization/loss.py:22-124) by its ``XP_PAIR_*`` kind; loss and both feature
    gradients in one library call.  ``params``: the keyword arguments of ``hip_ops.pair_loss``."""

    @staticmethod
    def forward(ctx, kind, vis, txt, params):
        loss, dv, dt = H.pair_loss(kind, vis.contiguous().float(), txt.contiguous().float(), **params)
        return _FusedLossFn._keep(ctx, loss, (None, dv, dt, None))


def _layer_params(layer):
    """the 16 parameters of a CLIPEncoderLayer in EncoderLayerFn's argument order.  The sub-module handles are cached on the layer
    (nn.Module.__getattr__ chains cost ~10 us per call otherwise); the Parameter objects are read from the modules' own tables
    every time, so a replaced Parameter is always seen."""
    cached = layer.__dict__.get("_xp_mods")
    if cached is not None:
        # all 8 sub-modules are re-checked by identity through plain dict lookups (nn.Module keeps children in _modules):
        # module surgery on ANY of them (adapters, replaced LayerNorms ...) rebuilds the table
        mods, tabs = cached
        lm = layer._modules
        a, m = lm["self_attn"]._modules, lm["mlp"]._modules
        live = (lm["layer_norm1"], a["q_proj"], a["k_proj"], a["v_proj"], a["out_proj"], lm["layer_norm2"], m["fc1"], m["fc2"])
        for x, y, t in zip(live, mods, tabs):
            if x is not y or x._parameters is not t:
                cached = None
                break
    if cached is None:
        a, m = layer.self_attn, layer.mlp
        mods = (layer.layer_norm1, a.q_proj, a.k_proj, a.v_proj, a.out_proj, layer.layer_norm2, m.fc1, m.fc2)
        tabs = tuple(x._parameters for x in mods)
        layer.__dict__["_xp_mods"] = (mods, tabs)
    return tuple(d[k] for d in tabs for k in ("weight", "bias"))


def _layer_act(layer) -> int:
    """the activation of a CLIPEncoderLayer's MLP (CLIPMLP.act_kind, from its tower's config.hidden_act) as L.ACT_*"""
    return layer._modules["mlp"].__dict__.get("act_kind", L.ACT_QUICK_GELU)


def layer_attentions(x, layer, B, S, size, pad_mask, side=None):
    """The attention weights of a ``CLIPEncoderLayer`` on its input ``x`` (``side``: x's fp32 side rows), for ``output_attentions``:
    LayerNorm 1, the QKV projection and the fused attention forward as the op-by-op layer forward calls them (_attn_front_ops) -- the
    native layer call computes the same bits -- then ``hip_ops.attn_probs`` on that qkv and those statistics.  Causal (``size`` None):
    fp32 ``[B, H, S, S]``; video: ``(proxy [B,H,M,S], frame [B,H,N,L,M+L])``.  No autograd: the weights are detached, new memory."""
    ln1_w, ln1_b, wq, bq, wk, bk, wv, bv = _layer_params(layer)[:8]
    heads = layer.num_heads
    _check_layer_args("layer_attentions", x, heads, L.ACT_QUICK_GELU, side, B * size[0] if size is not None else B * S,
                      "[B*M, D] (video) / [B*S, D] (text)")
    with torch.no_grad():
        Wqkv, bqkv = WEIGHTS.fused((wq, wk, wv), x.dtype), WEIGHTS.fused((bq, bk, bv), torch.float32)
        lns = None if side is None else ((S, size[0], size[0]) if size is not None else (1, 1, 1))
        qkv, stats = _attn_front_ops({}, x.detach(), ln1_w.detach(), ln1_b.detach(), Wqkv, bqkv, B, S, heads, size, pad_mask, side, lns)
        return H.attn_probs(qkv, stats, B, S, heads, size=size, pad_mask=pad_mask)


def encoder_layer(x, layer, B, S, heads, size, pad_mask, side=None, split=None):
    """Apply ``EncoderLayerFn`` with the parameters of a ``CLIPEncoderLayer`` module.  With ``side`` (the proxy rows of x in fp32)
    returns ``(x3, side_out)``.  ``split``: a ``ForwardSplit`` (the tower runs as two half-batch chains)."""
    # `training` argument: forward-only passes (torch.no_grad: retrieval / inference) skip the MLP pre-activation
    return EncoderLayerFn.apply(x, *_layer_params(layer), B, S, heads, size, pad_mask, torch.is_grad_enabled(), side, split,
                                _layer_act(layer))
