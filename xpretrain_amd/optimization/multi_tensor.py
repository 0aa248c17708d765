"""What the on-device optimizers (``AdamW``, ``Adam``, ``Adamax``) share: ONE multi-tensor HIP launch per step (plus one for the
gradient norm) over fp32 masters and two fp32 state tensors per parameter.

A subclass supplies three things:

* ``_STATE``: the names of its two state tensors, in the order of ``XpAdamTensor``'s ``m`` and ``v`` slots;
* ``_group_struct(group, step)``: a param group and a step count (after the increment) as the kernel's group struct;
* ``_ENTRY`` and ``_KIND``: the names of its update entry point and of that call's guarded twin, and the ``kind`` argument in front of
  their common argument list (``None``: the entry points take none).  ``_launch`` here makes the checked call from them.

On top of the ``torch.optim.Optimizer`` surface:

* ``step(max_grad_norm=...)`` / ``clip_and_step(max_norm)`` fuse ``clip_grad_norm_(params, max_norm)``
  (``tasks/run_video_retrieval.py:390-392``) into the update: the kernel scales the gradients on the fly, the norm
  is left in ``last_grad_norm`` (device scalar, no host sync).  The clipped gradients are not written back.
* the compute-dtype copies of the weights (``functional.WEIGHTS``) are rewritten by the same kernel, so no cast
  kernels run in the next forward.
* ``overlap_next_forward(model, first_late_layer=K)``: the update of the encoder layers >= K of both towers runs on a stream of its
  own, behind the gradient norm, and the NEXT forward waits for it in front of layer K (``functional.LateUpdate``, one per call,
  attached to the model's encoders): the HBM-bound optimizer pass (4.5 GB at ViT-B/16 + text tower, 0.78 ms) overlaps the MFMA-bound
  first layers instead of standing between two steps.  Same kernel, same arguments, same results.  Whoever else touches the late
  parameters, their moments or their gradients before that forward calls ``functional.join_late_weights()`` first: the model's
  ``state_dict`` and ``load_state_dict`` pre-hooks do, and so do this optimizer's ``state_dict``, ``load_state_dict``,
  ``zero_grad(set_to_none=False)`` and ``step``.
* ``skip_nonfinite=True`` (default off: then nothing below exists, the launches and their arguments are the unguarded ones): a step
  whose global gradient norm is not finite changes no parameter, no state tensor and no step count -- what a skipped
  ``optimizer.step()`` was under apex's dynamic loss scale (``run_pretrain.py:234-236, 374-377``), without the scaling.  Decided on the
  device: the norm partials always run, ``xp_step_verdict`` reduces them once on the caller's stream in front of the fork of
  ``overlap_next_forward``, and every update launch, early or late, is the guarded twin reading that one verdict.  ``step()`` does not
  wait for it: the verdict is copied to a pinned buffer behind the step, and the NEXT ``step()`` -- or ``state_dict()``,
  ``load_state_dict()``, ``skipped_steps``, ``last_step_skipped``, ``last_nonfinite_param`` / ``_name`` when read -- waits for that copy
  and, if the step was skipped, takes the ``state["step"]`` increments back from exactly the parameters of that step (``take_back``), so
  the bias corrections count applied steps.  ``last_grad_norm`` is the verdict's norm (not finite on a skipped step, as
  ``clip_grad_norm_`` would return).  A guarded step under stream capture raises ``RuntimeError``: a replay cannot take a count back.

``state["step"]`` is a Python int; ``load_state_dict`` also takes the scalar tensor ``torch.optim`` stores there.

There is no eager fallback: without the HIP library the step raises.
"""
import ctypes as C
import logging

import torch
from torch.optim import Optimizer

from .. import _lib as L
from .. import hip_ops as H

_LOG = logging.getLogger("xpretrain_amd")


def take_back(states, finite, first_bad_chunk, chunk_params):
    """The bookkeeping of one guarded step once its verdict is on the host.  ``states``: the state dicts whose ``step`` the step
    incremented; ``chunk_params``: the parameter owning each global chunk.  An applied step changes nothing and returns None; a skipped
    one takes the increment back from exactly those states and returns the parameter owning ``first_bad_chunk`` (None when it is -1:
    every partial was finite and only their sum overflowed)."""
    if finite:
        return None
    for st in states:
        st["step"] -= 1
    return chunk_params[first_bad_chunk] if first_bad_chunk >= 0 else None


class MultiTensorOptimizer(Optimizer):
    _STATE = None           # (name of the m-slot state tensor, name of the v-slot state tensor)
    _ENTRY = None           # (the unguarded entry point of the update, its guarded twin)
    _KIND = None            # the entry points' leading ``kind`` argument; None: they take none

    def __init__(self, params, defaults, skip_nonfinite=False):
        super().__init__(params, defaults)
        self.last_grad_norm = None      # device fp32 scalar after a clipped (or guarded) step
        self._plan = None
        self._late = None               # (ids of the late parameters, first late layer) -- overlap_next_forward()
        self._late_update = None        # functional.LateUpdate: the side stream, the pending event, the encoders that wait for it
        self.skip_nonfinite = bool(skip_nonfinite)
        self.param_names = None         # id(parameter) -> name, where the builder knows them (setup_e2e_optimizer)
        self._verdict = None            # device XpStepVerdict (as bytes), zeroed once: its counters run over the optimizer's life
        self._verdict_host = None       # pinned copy, written behind each guarded step
        self._pending = None            # (event behind that copy, the stepped state dicts, the plan's chunk -> parameter list)
        self._skipped = 0
        self._last_skipped = False
        self._last_bad = None

    def _group_struct(self, group, step):
        raise NotImplementedError

    def _launch(self, lib, la, groups, n_groups, partials, n_partials, max_norm, norm, stream, verdict=None):
        """The checked kernel call for one launch record ``la`` of the plan.  ``verdict`` None: the unguarded entry point; else the
        device address of the step's XpStepVerdict and the guarded twin."""
        entry = self._ENTRY[verdict is not None]
        lead = () if self._KIND is None else (self._KIND,)
        tail = (stream,) if verdict is None else (verdict, stream)
        L.check(getattr(lib, entry)(*lead, la["table"].data_ptr(), la["chunk_map"].data_ptr(), la["n_chunks"], la["grads"], la["grp"],
                                    la["n"], groups, n_groups, partials, n_partials, max_norm, norm, *tail), entry)

    # ------------------------------------------------------------------------------------------ the step guard
    def _reconcile(self):
        """Wait for the verdict of the latest guarded step (a whole forward and backward old by the next step) and, if that step was
        skipped, take its step-count increments back.  Everything that reads or builds on the step counts comes through here."""
        if self._pending is None:
            return
        event, states, chunk_params = self._pending
        self._pending = None
        event.synchronize()
        v = L.XpStepVerdict.from_buffer_copy(bytes(self._verdict_host.tolist()))
        self._skipped, self._last_skipped = int(v.skipped), not v.finite
        self._last_bad = take_back(states, bool(v.finite), int(v.first_bad_chunk), chunk_params)
        if self._last_skipped:
            who = "only the sum of the chunk sums overflowed" if self._last_bad is None else \
                f"first non-finite chunk in {self.last_nonfinite_name or 'a parameter of shape ' + str(tuple(self._last_bad.shape))}"
            _LOG.warning("%s: step skipped, gradient norm %s (%s); %d skipped so far", type(self).__name__, v.norm, who, self._skipped)

    @property
    def skipped_steps(self):
        """how many guarded steps were skipped so far (int; waits for the latest step's verdict)"""
        self._reconcile()
        return self._skipped

    @property
    def last_step_skipped(self):
        self._reconcile()
        return self._last_skipped

    @property
    def last_nonfinite_param(self):
        """the Parameter owning the first chunk whose own sum of squares was not finite in the latest step; None when that step was
        applied, or skipped because only the total overflowed"""
        self._reconcile()
        return self._last_bad

    @property
    def last_nonfinite_name(self):
        """``last_nonfinite_param``'s name, where the builder gave the names (``setup_e2e_optimizer``); else None"""
        p = self.last_nonfinite_param
        return None if p is None or self.param_names is None else self.param_names.get(id(p))

    def overlap_next_forward(self, model, first_late_layer=2):
        """Run the update of ``encoder.layers[first_late_layer:]`` of the model's towers on a side stream (see the module docstring).
        ``first_late_layer=None`` switches it off.  One overlapped optimizer per encoder: ``ValueError`` when an encoder already
        waits for another live optimizer; a second call replaces this optimizer's own record (after joining it)."""
        from ..functional import LateUpdate
        ids, encoders = set(), []
        if first_late_layer is not None:
            own = {id(p) for group in self.param_groups for p in group["params"]}
            for m in model.modules():
                layers = getattr(m, "layers", None)
                if isinstance(layers, torch.nn.ModuleList) and type(m).__name__ == "CLIPEncoder":
                    late = {id(p) for layer in layers[first_late_layer:] for p in layer.parameters()}
                    ids |= late
                    if late & own:
                        encoders.append(m)
        new = LateUpdate(first_late_layer, self) if ids else None
        if new is not None:
            new.attach(encoders)                # (raises before anything changed; takes over the encoders of this optimizer's old record)
        if self._late_update is not None:
            self._late_update.detach()
        self._plan = None
        self._late_update = new
        self._late = (frozenset(ids), int(first_late_layer)) if ids else None
        return self

    # ------------------------------------------------------------------------------------------ planning
    def _active(self):
        act = []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
                act.append((gi, p))
        return act

    def _build_plan(self, act, cache):
        """Static part of a step: device tables, chunk maps, shadow bindings.  Rebuilt when the set of stepped
        parameters, their storage, or the weight cache's set of buffers changes."""
        name, (sm, sv) = type(self).__name__, self._STATE
        dev = act[0][1].device
        shadows, entries = cache.shadow_bindings([p for _, p in act])
        launches, tensors = [], []
        for gi, p in act:
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
                raise TypeError(f"xpretrain_amd {name}: parameters must be contiguous fp32 tensors on one device")
            st = self.state[p]
            if any(st[k].dtype != torch.float32 or not st[k].is_contiguous() or st[k].device != dev or st[k].shape != p.shape
                   for k in (sm, sv)):
                raise TypeError(f"xpretrain_amd {name}: optimizer state must be contiguous fp32 tensors on the parameter's device")
            tensors.append((gi, p, st))
        late_ids = self._late[0] if self._late else frozenset()
        sets = [[t for t in tensors if id(t[1]) not in late_ids], [t for t in tensors if id(t[1]) in late_ids]]
        parts = [(tl[i0:i0 + L.XP_OPT_MAX_TENSORS], k == 1) for k, tl in enumerate(sets) for i0 in range(0, len(tl), L.XP_OPT_MAX_TENSORS)]
        n_total_chunks, chunk_params = 0, []
        for part, late in parts:
            tab = (L.XpAdamTensor * len(part))()
            cmap = []
            for j, (gi, p, st) in enumerate(part):
                sh = shadows.get(id(p))
                tab[j].p, tab[j].m, tab[j].v = p.data_ptr(), st[sm].data_ptr(), st[sv].data_ptr()
                tab[j].shadow = sh[0] if sh else 0
                tab[j].shadow_dtype = sh[1] if sh else 0
                tab[j].numel = p.numel()
                for c in range((p.numel() + L.XP_OPT_CHUNK - 1) // L.XP_OPT_CHUNK):
                    cmap += [j, c]
                    chunk_params.append(p)            # (global chunk index -> its parameter: XpStepVerdict.first_bad_chunk)
            raw = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8)
            launches.append(dict(part=part, table=raw.to(dev), n=len(part),
                                 chunk_map=torch.tensor(cmap, dtype=torch.int32).to(dev),
                                 n_chunks=len(cmap) // 2, chunk_base=n_total_chunks, late=late,
                                 grads=(C.c_void_p * len(part))(), grp=(C.c_uint8 * len(part))()))
            n_total_chunks += len(cmap) // 2
        return dict(key=self._plan_key(act, cache), sig=[(gi, p, p.data_ptr(), self.state[p], self.state[p][sm].data_ptr(), self.state[p][sv].data_ptr())
                         for gi, p in act], sv=cache.structure_version,
                    launches=launches, n_chunks=n_total_chunks, chunk_params=chunk_params, entries=entries,
                    partials=torch.empty(n_total_chunks, dtype=torch.float32, device=dev),
                    norm=torch.zeros((), dtype=torch.float32, device=dev))

    def _plan_key(self, act, cache):
        # parameter storage, state storage (load_state_dict replaces the state tensors) and the weight cache's buffers
        sm, sv = self._STATE

        def moments(p):
            st = self.state.get(p)
            return (st[sm].data_ptr(), st[sv].data_ptr()) if st and sm in st else (0, 0)
        return (tuple((gi, id(p), p.data_ptr()) + moments(p) for gi, p in act), cache.structure_version, self._late)

    # ------------------------------------------------------------------------------------------ step
    @torch.no_grad()
    def step(self, closure=None, max_grad_norm=None):
        if self._late_update is not None:       # a previous step's late update nobody waited for (two steps without a forward) still
            self._late_update.join()            # reads the gradients and the norm partials
        guard = self.skip_nonfinite
        if guard and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"xpretrain_amd {type(self).__name__}: skip_nonfinite cannot run under stream capture: a skipped step's "
                               "count is taken back on the host, which a replay cannot do")
        self._reconcile()                       # the step counts below are those of the APPLIED steps
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        act = self._active()
        if not act:
            return loss
        from ..functional import WEIGHTS, order_gradient_streams_behind
        name, (sm, sv) = type(self).__name__, self._STATE
        plan = self._plan
        # steady state: the same parameters and state tensors with the same storage as when the plan was built, and no change in the
        # weight cache's buffers (the same facts _plan_key() hashes, checked without building the key)
        if not (plan is not None and plan["sv"] == WEIGHTS.structure_version and len(act) == len(plan["sig"])
                and all(a[1] is s[1] and a[0] == s[0] and a[1].data_ptr() == s[2] and self.state.get(a[1]) is s[3]
                        and s[3][sm].data_ptr() == s[4]
                        and s[3][sv].data_ptr() == s[5] for a, s in zip(act, plan["sig"]))):
            for _, p in act:                 # state initialisation (adamw.py:62-68) before the plan key looks at it
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = 0
                    st[sm] = torch.zeros_like(p.data)
                    st[sv] = torch.zeros_like(p.data)
            if plan is None or plan["key"] != self._plan_key(act, WEIGHTS):
                self._plan = self._build_plan(act, WEIGHTS)
            plan = self._plan
        clip = max_grad_norm is not None and max_grad_norm > 0
        stream = H._stream()
        lib = L.lib()
        # effective hyper-parameter groups: (param group, step count) pairs
        eff, eff_index = [], {}
        for la in plan["launches"]:
            for j, (gi, p, st) in enumerate(la["part"]):
                g = p.grad
                if g.dtype != torch.float32 or not g.is_contiguous():
                    raise TypeError(f"xpretrain_amd {name}: gradients must be contiguous fp32 tensors")
                la["grads"][j] = g.data_ptr()
                st["step"] += 1
                k = (gi, st["step"])
                idx = eff_index.get(k)
                if idx is None:
                    idx = eff_index[k] = len(eff)
                    eff.append(self._group_struct(self.param_groups[gi], st["step"]))
                la["grp"][j] = idx
        if len(eff) > L.XP_OPT_MAX_GROUPS:
            raise RuntimeError(f"xpretrain_amd {name}: {len(eff)} distinct (group, step) pairs in one step (max "
                               f"{L.XP_OPT_MAX_GROUPS}); step parameters with diverging step counts separately")
        groups = (type(eff[0]) * len(eff))(*eff)
        dev = plan["norm"].device
        if clip or guard:                       # (the verdict needs the partials also when nothing is clipped)
            for la in plan["launches"]:
                part = plan["partials"][la["chunk_base"]:]
                L.check(lib.xp_grad_sqnorm_partials(la["table"].data_ptr(), la["chunk_map"].data_ptr(), la["n_chunks"],
                                                    la["grads"], la["n"], part.data_ptr(), stream),
                        "xp_grad_sqnorm_partials")
        verdict = None
        if guard:                               # one launch on the caller's stream, in front of the fork below: every guarded launch
            if self._verdict is None or self._verdict.device != dev:                               # reads this one verdict
                self._verdict = torch.zeros(C.sizeof(L.XpStepVerdict), dtype=torch.uint8, device=dev)
                self._verdict_host = torch.zeros(C.sizeof(L.XpStepVerdict), dtype=torch.uint8).pin_memory()
            verdict = C.cast(self._verdict.data_ptr(), C.POINTER(L.XpStepVerdict))
            L.check(lib.xp_step_verdict(plan["partials"].data_ptr(), plan["n_chunks"], verdict, stream), "xp_step_verdict")
        late = [la for la in plan["launches"] if la["late"]]
        overlap = bool(late) and not torch.cuda.is_current_stream_capturing()

        def run(la, st):
            if guard:
                self._launch(lib, la, groups, len(eff), plan["partials"].data_ptr(), plan["n_chunks"],
                             float(max_grad_norm) if clip else 0.0, plan["norm"].data_ptr(), st, verdict=verdict)
                return
            self._launch(lib, la, groups, len(eff), plan["partials"].data_ptr() if clip else None,
                         plan["n_chunks"] if clip else 0, float(max_grad_norm) if clip else 0.0,
                         plan["norm"].data_ptr() if clip else None, st)
        if overlap:
            # first in program order: beside the early launches and whatever the main stream enqueues next.  (Launching it BEHIND the
            # early launches -- so that those run alone at full bandwidth -- measured the same: 14.385 vs 14.369 ms per step,
            # profiles/r06s_in_step_ab_optimizer_overlap_order.txt)
            # behind everything the current stream has enqueued so far (the gradients, the norm partials)
            with self._late_update.launch(torch.cuda.current_stream(dev)) as side:
                seen = set()
                for la in late:
                    for _, p, _ in la["part"]:          # the caching allocator must not hand a freed gradient to the next forward
                        sp = p.grad.untyped_storage().data_ptr()      # while this stream still reads it (zero_grad(set_to_none=True))
                        if sp not in seen:
                            seen.add(sp)
                            p.grad.record_stream(side)
                    run(la, side.cuda_stream)
        for la in plan["launches"]:
            if not (overlap and la["late"]):
                run(la, stream)
        # gradients another stream's backward allocated (the text tower's) go back to THAT stream's pool when they are freed:
        # it must not reuse them before the launches above have read them
        order_gradient_streams_behind(torch.cuda.current_stream(dev))
        if guard:
            # What happened reaches the host behind the step, with no wait here: the next step() (or whoever reads the counts first)
            # waits for this event, a forward and a backward later, and takes the increments above back if the step was skipped.
            self._verdict_host.copy_(self._verdict, non_blocking=True)
            event = torch.cuda.Event()
            event.record(torch.cuda.current_stream(dev))
            self._pending = (event, [st for la in plan["launches"] for _, _, st in la["part"]], plan["chunk_params"])
        self.last_grad_norm = plan["norm"] if clip or guard else None
        self._wrote = plan["entries"]
        return loss

    def state_dict(self):
        from .. import functional as XF
        XF.join_late_weights()           # the state tensors of the late layers may still be in flight on the optimizer's stream
        self._reconcile()                # (a skipped step's count is not a step)
        return super().state_dict()

    def zero_grad(self, set_to_none=True):
        """``set_to_none=False`` zeroes in place, so it first joins a pending late update, which still reads the late gradients.  The
        rule for every other writer: an in-place write to a late parameter's gradient between ``step()`` and the next forward comes
        after ``functional.join_late_weights()``.  (A freed gradient needs no join: ``step()`` recorded it on the side stream.)"""
        if not set_to_none and self._late_update is not None:
            self._late_update.join()
        super().zero_grad(set_to_none=set_to_none)

    def load_state_dict(self, state_dict):
        from .. import functional as XF
        XF.join_late_weights()
        self._reconcile()
        super().load_state_dict(state_dict)
        for st in self.state.values():   # torch.optim keeps the step count as a scalar tensor; here it is a Python int
            if torch.is_tensor(st.get("step")):
                st["step"] = int(st["step"].item())
        self._plan = None                # the state tensors were replaced

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._plan = None

    def clip_and_step(self, max_norm):
        """``clip_grad_norm_(params, max_norm)`` + ``step()`` in one pass; returns the (device) gradient norm."""
        self.step(max_grad_norm=max_norm)
        return self.last_grad_norm

    def _xp_after_step(self, cache):
        """Called by the weight cache's optimizer hook instead of a blanket invalidation: every cached copy goes stale
        except the ones this step rewrote."""
        wrote = getattr(self, "_wrote", None)
        self._wrote = None
        cache.invalidate(keep=wrote)
