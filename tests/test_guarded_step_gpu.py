"""GPU: the device-side step guard (``skip_nonfinite=True``: xp_step_verdict + xp_adamw_step_guarded / xp_optim_step_guarded) for
AdamW, Adam and Adamax, with and without clipping.

Everything here is an exact statement, so there is no tolerance: a finite step equals the unguarded entry point bit for bit; a step
with a non-finite gradient norm changes no bit of (p, m, v, step), rewrites the shadows from the unchanged p, and the next finite step
equals the one of a run that never saw the bad gradients (tests/guarded_step_ref.py is the definition; tests/test_guarded_step_cpu.py
holds it against live torch).  On the code before the guard the planted cases end with every tensor NaN.

The ragged set (XP_OPT_CHUNK = 64 Ki): numel 1, 3, 4, CHUNK - 1, CHUNK, CHUNK + 1 and 2 CHUNK + 5 (last); three biases behind one fused
fp32 shadow; bf16 shadows on numel 4 and CHUNK; a parameter, a gradient and a state tensor that each start one element into their
buffer (the 16-byte path is off for the whole tensor); tiny tensors up to 260 in all: two launch tables (256 + 4)."""
import ctypes as C
import functools

import pytest
import torch

from oracle import clipvip_oracle as O
from tests import guarded_step_ref as G
from tests.gpu_util import ModelArgs
from tests.guarded import Guarded

pytestmark = pytest.mark.gpu

CHUNK = G.CHUNK
KINDS = G.KINDS
CLIPS = [None, 0.5]
BF = torch.bfloat16
SIZES = [1, 3, 4, CHUNK - 1, CHUNK, CHUNK + 1, 64, 64, 64, 41 * 13, 41 * 13, 41 * 13] + [3 + i % 5 for i in range(247)] + [2 * CHUNK + 5]
I_BF_SMALL, I_BF_CHUNK, I_BIAS, I_MIS_P, I_MIS_G, I_MIS_S, I_TABLE2, I_LAST = 2, 4, (6, 7, 8), 9, 10, 11, 257, len(SIZES) - 1
N_CHUNKS = sum(-(-n // CHUNK) for n in SIZES)
BETAS = (0.8, 0.95)
VALUES = {"+inf": float("inf"), "-inf": float("-inf"), "nan": float("nan")}


def ours(kind):
    from xpretrain_amd import optimization as XO
    return {"adamw": XO.AdamW, "adam": XO.Adam, "adamax": XO.Adamax}[kind]


def off_by_one(t):
    """the same values, starting one element (4 bytes) into a fresh buffer"""
    buf = torch.zeros(t.numel() + 1, device="cuda")
    buf[1:] = t.reshape(-1)
    out = buf[1:].view(t.shape)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


@functools.lru_cache(maxsize=None)
def ragged_inputs():
    gen = torch.Generator().manual_seed(17)
    init = [torch.randn(n, generator=gen) * 0.1 for n in SIZES]
    grads = [[(torch.randn(n, generator=gen) * 0.05 * (1.0, 0.01, 1.0)[t]).cuda() for n in SIZES] for t in range(3)]
    return init, grads


class Set:
    """parameters + optimizer + how to hand it one step's gradients; ``late``: the parameters updated on the side stream"""

    def __init__(self, params, opt, place_grad, late=()):
        self.params, self.opt, self.place_grad, self.late = params, opt, place_grad, late
        self.kind = {"AdamW": "adamw", "Adam": "adam", "Adamax": "adamax"}[type(opt).__name__]

    def step(self, grads, clip, plant=None):
        """one step on clones of ``grads``; ``plant`` = (parameter index, flat element, value)"""
        for i, (p, g) in enumerate(zip(self.params, grads)):
            g = self.place_grad(i, g.clone())
            if plant is not None and plant[0] == i:
                g.view(-1)[plant[1]] = plant[2]
            p.grad = g
        self.opt.step(max_grad_norm=clip)

    def tensors(self):
        """clones of every p, m, v (in parameter order)"""
        a, b = G.STATE[self.kind]
        return [t.detach().clone() for p in self.params for t in (p, self.opt.state[p][a], self.opt.state[p][b])]

    def steps(self):
        return [self.opt.state[p]["step"] for p in self.params]

    def shadows(self):
        """(the shadow buffer, what it must hold: the cast of its parameters) for every cache entry the plan rewrites"""
        index = {id(p): i for i, p in enumerate(self.params)}
        out = []
        for _, ent in sorted(self.opt._plan["entries"], key=lambda e: index[id(e[1].refs[0]())]):      # (the cache's own order is not stable)
            ws = [r().detach().reshape(-1) for r in ent.refs]
            out.append((ent.buf, torch.cat(ws).to(ent.buf.dtype).view(ent.buf.shape)))
        return out

    def shadows_hold(self):
        sh = self.shadows()
        assert sh and all(torch.equal(buf, want) for buf, want in sh)
        return sh


def ragged_set(kind, guard):
    from xpretrain_amd.functional import WEIGHTS
    init, _ = ragged_inputs()
    params = [torch.nn.Parameter(off_by_one(p.cuda()) if i == I_MIS_P else p.clone().cuda()) for i, p in enumerate(init)]
    WEIGHTS.get(params[I_BF_SMALL], BF), WEIGHTS.get(params[I_BF_CHUNK], BF), WEIGHTS.fused(tuple(params[i] for i in I_BIAS), torch.float32)
    half = len(params) // 2
    opt = ours(kind)([dict(params=params[:half], weight_decay=0.3, lr=1e-2), dict(params=params[half:], weight_decay=0.0, lr=3e-3)],
                     betas=BETAS, skip_nonfinite=guard)
    a, b = G.STATE[kind]
    p = params[I_MIS_S]
    opt.state[p] = {"step": 0, a: off_by_one(torch.zeros_like(p)), b: torch.zeros_like(p)}
    s = Set(params, opt, lambda i, g: off_by_one(g) if i == I_MIS_G else g)
    return s


_CFG = O.hf_config_dict(128, 2, 4, 256, 16, 32, 128, 2, 4, 256, 120, 16, 64)


@functools.lru_cache(maxsize=None)
def model_grads():
    """three steps of synthetic gradients for the tiny model's parameters, by name order (no backward: the optimizer alone is under test)"""
    from xpretrain_amd.modeling import VidCLIP
    torch.manual_seed(11)
    shapes = [p.shape for p in VidCLIP(ModelArgs(_CFG, 2)).parameters()]
    gen = torch.Generator().manual_seed(23)
    return [[(torch.randn(s, generator=gen) * 0.01).cuda() for s in shapes] for _ in range(3)]


def model_set(kind, guard):
    """the tiny 4-layer model of tests/test_optim_family_gpu.py with overlap_next_forward(model, 1): the encoder layers >= 1 of both towers
    are updated on the side stream.  One forward first, so that the weight cache holds the model's real shadows."""
    from xpretrain_amd.modeling import VidCLIP
    torch.manual_seed(11)
    model = VidCLIP(ModelArgs(_CFG, 2)).cuda().train()
    with torch.no_grad():
        model(*(t.cuda() for t in O.synthetic_inputs(4, 2, 32, 8, vocab=120)))
    params = list(model.parameters())
    late = [p for m in model.modules() if type(m).__name__ == "CLIPEncoder" for layer in m.layers[1:] for p in layer.parameters()]
    opt = ours(kind)([dict(params=[p for p in params if p.ndim >= 2], weight_decay=0.05), dict(params=[p for p in params if p.ndim < 2])],
                     lr=1e-3, betas=BETAS, skip_nonfinite=guard)
    opt.overlap_next_forward(model, 1)
    s = Set(params, opt, lambda i, g: g, late=late)
    s.model = model
    return s


def grads_of(which):
    return ragged_inputs()[1] if which == "ragged" else model_grads()


def make(which, kind, guard):
    return (ragged_set if which == "ragged" else model_set)(kind, guard)


def finish(s):
    """everything the side stream still does is done and visible"""
    from xpretrain_amd import functional as XF
    XF.join_late_weights()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ 1. finite gradients: the unguarded twin's bits
@functools.lru_cache(maxsize=None)
def finite_run(which, kind, clip, guard, steps=(0, 1, 2), rep=0):
    """(p, m, v of every parameter; shadow buffers; norm per step; step counts) after the gradients ``steps``"""
    s = make(which, kind, guard)
    grads, norms = grads_of(which), []
    for t in steps:
        s.step(grads[t], clip)
        norms.append(None if s.opt.last_grad_norm is None else s.opt.last_grad_norm.clone())
    finish(s)
    if which == "ragged":
        assert len(s.opt._plan["launches"]) == 2 and s.opt._plan["n_chunks"] == N_CHUNKS
    else:
        assert s.late and any(la["late"] for la in s.opt._plan["launches"]) and not all(la["late"] for la in s.opt._plan["launches"])
    sh = s.shadows_hold()
    assert {buf.dtype for buf, _ in sh} == {BF, torch.float32} if which == "ragged" else BF in {buf.dtype for buf, _ in sh}
    if guard:
        assert (s.opt.skipped_steps, s.opt.last_step_skipped, s.opt.last_nonfinite_param) == (0, False, None)
    return s.tensors(), [buf.clone() for buf, _ in sh], norms, s.steps()


@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", ["ragged", "model"])
def test_finite_steps_have_the_unguarded_bits(which, kind, clip):
    """three steps, gradient scales x1, x0.01, x1 (the clip at 0.5 is active, idle, active on the ragged set)"""
    got, ref = finite_run(which, kind, clip, True), finite_run(which, kind, clip, False)
    assert len(got[0]) == len(ref[0]) and all(torch.equal(a, b) for a, b in zip(got[0], ref[0]))
    assert len(got[1]) == len(ref[1]) and all(torch.equal(a, b) for a, b in zip(got[1], ref[1]))
    assert got[3] == ref[3] == [3] * len(got[3])
    # the norm depends on the gradients alone: the guarded run has it with and without clipping, the unguarded one when it clips
    clipped = finite_run(which, kind, 0.5, False)[2]
    assert all(n is not None and torch.equal(n, c) for n, c in zip(got[2], clipped))
    assert all(torch.isfinite(t).all() for t in got[0])
    if which == "ragged":
        assert float(clipped[0]) > 0.5 > float(clipped[1])


# ------------------------------------------------------------------------------------------ 2. planted non-finite gradients
PLACES = {                       # name -> (set, parameter index or None = a late parameter, flat element)
    "first element of tensor 0": ("ragged", 0, 0),
    "last element of the last chunk of the last tensor": ("ragged", I_LAST, SIZES[I_LAST] - 1),
    "scalar tail of the misaligned tensor": ("ragged", I_MIS_P, SIZES[I_MIS_P] - 1),
    "a tensor of the second launch table": ("ragged", I_TABLE2, 1),
    "a late-layer parameter, overlap on": ("model", None, 5),
}


def planted_run(place, kind, clip, value):
    which, index, elem = PLACES[place]
    s = make(which, kind, True)
    grads = grads_of(which)
    if index is None:
        index = next(i for i, p in enumerate(s.params) if any(p is q for q in s.late) and p.ndim >= 2 and p.numel() > elem)
    s.step(grads[0], clip)
    finish(s)
    before, steps_before, skipped_before = s.tensors(), s.steps(), s.opt.skipped_steps
    assert steps_before == [1] * len(s.params) and skipped_before == 0
    for buf, _ in s.shadows():
        buf.zero_()                                       # the skipped step must REWRITE the shadows, not merely leave them
    s.step(grads[1], clip, plant=(index, elem, value))
    bad_norm = s.opt.last_grad_norm.clone()
    finish(s)
    after = s.tensors()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, after)), "a skipped step changed p, m or v"
    s.shadows_hold()
    assert s.opt.last_step_skipped is True and s.opt.skipped_steps == skipped_before + 1
    assert s.steps() == steps_before
    assert s.opt.last_nonfinite_param is s.params[index]
    assert not torch.isfinite(bad_norm)
    s.step(grads[2], clip)
    finish(s)
    assert s.opt.last_step_skipped is False and s.opt.skipped_steps == skipped_before + 1 and s.opt.last_nonfinite_param is None
    assert s.steps() == [2] * len(s.params)
    s.shadows_hold()
    return s.tensors()


@pytest.mark.parametrize("value", list(VALUES))
@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("place", list(PLACES))
def test_planted_nonfinite_gradient_skips_the_step_and_nothing_else(place, kind, clip, value):
    """finite, planted, finite: the planted step is the identity, says so and names the parameter; the step after it equals, bit for bit,
    the second step of a run that never saw the bad gradients (same t = 2 in the bias corrections).  Without the guard every tensor is
    NaN after the planted step."""
    got = planted_run(place, kind, clip, VALUES[value])
    ref = finite_run(PLACES[place][0], kind, clip, True, steps=(0, 2))
    assert ref[3] == [2] * len(ref[3])
    assert len(got) == len(ref[0]) and all(torch.equal(a, b) for a, b in zip(got, ref[0]))
    assert all(torch.isfinite(t).all() for t in got)


# ------------------------------------------------------------------------------------------ 3. only the total overflows
def verdict_of(opt):
    from xpretrain_amd import _lib as L
    torch.cuda.synchronize()
    return L.XpStepVerdict.from_buffer_copy(bytes(opt._verdict.cpu().tolist()))


@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("kind", KINDS)
def test_overflow_of_the_total_alone_skips_and_blames_nobody(kind, clip):
    """1.5e19 ** 2 = 2.25e38 is finite in fp32, the sum of two of them is not"""
    params = [torch.nn.Parameter(torch.full((1,), 0.5, device="cuda")) for _ in range(2)]
    opt = ours(kind)(params, lr=1e-2, skip_nonfinite=True)
    for p in params:
        p.grad = torch.full((1,), 1.5e19, device="cuda")
    opt.step(max_grad_norm=clip)
    v = verdict_of(opt)
    assert (opt._plan["partials"] == torch.tensor(1.5e19).square().item()).all()
    assert (v.finite, v.first_bad_chunk, v.applied, v.skipped) == (0, -1, 0, 1) and v.norm == float("inf")
    assert opt.last_step_skipped and opt.skipped_steps == 1 and opt.last_nonfinite_param is None
    assert all(opt.state[p]["step"] == 0 for p in params)
    assert all(float(p.detach()) == 0.5 and not any(opt.state[p][k].any() for k in G.STATE[kind]) for p in params)
    assert float(opt.last_grad_norm) == float("inf")
    # one of them alone is a step like any other
    params[1].grad = torch.zeros(1, device="cuda")
    opt.step(max_grad_norm=clip)
    v = verdict_of(opt)
    assert (v.finite, v.first_bad_chunk, v.applied, v.skipped) == (1, -1, 1, 1) and v.norm == pytest.approx(1.5e19, rel=1e-6)
    assert not opt.last_step_skipped and opt.skipped_steps == 1 and all(opt.state[p]["step"] == 1 for p in params)
    assert float(params[0].detach()) != 0.5 and torch.isfinite(params[0]).all()


# ------------------------------------------------------------------------------------------ 4. the verdict and the partials at their sizes
@pytest.mark.parametrize("kind", KINDS)
def test_verdict_and_partials_sit_between_poisoned_guards(kind):
    """the partials array at exactly n_chunks floats and the verdict at exactly sizeof(XpStepVerdict), each between the poisoned guards of
    tests/guarded.py, over an applied and a skipped step"""
    from xpretrain_amd import _lib as L
    s = ragged_set(kind, True)
    grads = grads_of("ragged")
    s.step(grads[0], 0.5)                                  # builds the plan
    finish(s)
    assert s.opt.skipped_steps == 0
    gp, gv = Guarded(1, N_CHUNKS, torch.float32), Guarded(1, C.sizeof(L.XpStepVerdict) // 4, torch.float32)
    gv.mat.zero_()
    assert gv.mat.data_ptr() % 8 == 0 and s.opt._plan["partials"].numel() == N_CHUNKS
    s.opt._plan["partials"], s.opt._verdict = gp.mat.view(-1), gv.mat.view(-1).view(torch.uint8)
    s.step(grads[1], 0.5)
    s.step(grads[2], None, plant=(I_LAST, SIZES[I_LAST] - 1, float("nan")))
    finish(s)
    v = verdict_of(s.opt)
    assert (v.finite, v.first_bad_chunk, v.applied, v.skipped) == (0, N_CHUNKS - 1, 1, 1)
    assert s.opt.last_step_skipped and s.opt.last_nonfinite_param is s.params[I_LAST] and s.steps() == [2] * len(SIZES)
    gp.check("partials", 1, N_CHUNKS)
    gv.check("verdict", 1, C.sizeof(L.XpStepVerdict) // 4)
    assert torch.isfinite(gp.mat[0, :-1]).all() and torch.isnan(gp.mat[0, -1])


# ------------------------------------------------------------------------------------------ 5. refusals
@pytest.mark.parametrize("kind", KINDS)
def test_null_verdict_and_unknown_kind_are_refused_before_any_launch(kind):
    from xpretrain_amd import _lib as L
    from xpretrain_amd import hip_ops as H
    s = ragged_set(kind, True)
    grads = grads_of("ragged")
    s.step(grads[0], 0.5)
    finish(s)
    before, plan = s.tensors(), s.opt._plan
    shadows = [buf.clone() for buf, _ in s.shadows()]
    la = plan["launches"][0]
    grp = s.opt._group_struct(s.opt.param_groups[0], 2)
    groups = (type(grp) * 1)(grp)
    for j in range(la["n"]):
        la["grp"][j] = 0

    def call(verdict):
        s.opt._launch(L.lib(), la, groups, 1, plan["partials"].data_ptr(), plan["n_chunks"], 0.5, plan["norm"].data_ptr(), H._stream(),
                      verdict=verdict)
    entry = "xp_adamw_step_guarded" if kind == "adamw" else "xp_optim_step_guarded"
    with pytest.raises(RuntimeError, match=rf"{entry} failed \(rc=-1\): {entry}: null verdict"):
        call(C.POINTER(L.XpStepVerdict)())
    if kind != "adamw":
        s.opt._KIND = 7
        with pytest.raises(RuntimeError, match=r"xp_optim_step_guarded failed \(rc=-1\): xp_optim_step_guarded: unknown kind 7"):
            call(C.cast(s.opt._verdict.data_ptr(), C.POINTER(L.XpStepVerdict)))
    with pytest.raises(RuntimeError, match=r"xp_step_verdict failed \(rc=-1\): xp_step_verdict: null argument"):
        L.check(L.lib().xp_step_verdict(plan["partials"].data_ptr(), plan["n_chunks"], C.POINTER(L.XpStepVerdict)(), H._stream()), "xp_step_verdict")
    finish(s)
    assert all(torch.equal(a, b) for a, b in zip(before, s.tensors()))
    assert all(torch.equal(a, buf) for a, (buf, _) in zip(shadows, s.shadows()))
    v = verdict_of(s.opt)
    assert (v.applied, v.skipped) == (1, 0)


# ------------------------------------------------------------------------------------------ 6. determinism
@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("kind", KINDS)
def test_two_runs_with_a_skipped_step_in_the_middle_are_bit_identical(kind, clip):
    place = "a tensor of the second launch table"
    a, b = planted_run(place, kind, clip, float("nan")), planted_run(place, kind, clip, float("nan"))
    assert all(x is not y and torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------ model level
def training_run(kind, batches, plant_at=None):
    """steps over ``batches`` (loop step k feeds batch k and sets the schedule's learning rate of step k) through configs.setup_training
    with skip_nonfinite_steps: 1 and the late layers overlapped; ``plant_at``: after that step's backward a NaN goes into one element of
    one late-layer gradient.  Returns the final state_dicts and the optimizer."""
    from xpretrain_amd import configs as CF
    from xpretrain_amd.modeling import VidCLIP
    torch.manual_seed(11)
    model = VidCLIP(ModelArgs(_CFG, 2)).cuda().train()
    cfg = CF.load_config(dict(optim=kind, learning_rate=1e-4, weight_decay=0.05, lr_mul=1, lr_mul_prefix="", betas=[0.9, 0.98],
                              loss_config={"loss_name": "NCELearnableTempLoss", "if_gather": 0}, decay="linear", warmup_ratio=0.25,
                              grad_norm=0.05, skip_nonfinite_steps=1))
    tr = CF.setup_training(cfg, model, 8)
    opt = tr.optimizer.overlap_next_forward(model, 1)
    assert opt.skip_nonfinite and tr.grad_norm == 0.05
    late = [(n, p) for n, p in model.named_parameters() if ".encoder.layers.3." in n and p.ndim >= 2]
    for k in batches:
        for g in opt.param_groups:
            g["lr"] = tr.lr_at(k + 1)
        video, ids, mask = (t.cuda() for t in O.synthetic_inputs(4, 2, 32, 8, vocab=120, seed=100 + k))
        out = model(video, ids, mask)
        tr.loss_fn(out["vis_features"], out["text_features"], model.clipmodel.logit_scale).backward()
        if k == plant_at:
            late[0][1].grad.view(-1)[7] = float("nan")
        opt.clip_and_step(tr.grad_norm)
        opt.zero_grad(set_to_none=True)
    if plant_at is not None:
        assert opt.skipped_steps == 1
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    osd = opt.state_dict()
    torch.cuda.synchronize()
    return sd, osd, opt, late[0]


@pytest.mark.parametrize("kind", KINDS)
def test_a_nan_in_step_two_costs_one_batch_not_the_run(kind):
    """four steps, NaN in one late-layer gradient after the second backward: the model's and the optimizer's final state_dict() equal,
    bit for bit, those of a run fed batches 1, 3 and 4 (with the learning rates of steps 1, 3 and 4: the schedule is the caller's)"""
    sd, osd, opt, _ = training_run(kind, (0, 1, 2, 3), plant_at=1)
    ref_sd, ref_osd, ref_opt, _ = training_run(kind, (0, 2, 3))
    assert ref_opt.skipped_steps == 0 and not opt.last_step_skipped and opt.last_nonfinite_param is None
    assert sd.keys() == ref_sd.keys() and all(torch.equal(sd[k], ref_sd[k]) for k in sd)
    assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
    assert osd["state"].keys() == ref_osd["state"].keys() and osd["param_groups"] == ref_osd["param_groups"]
    for i, st in osd["state"].items():
        assert st.keys() == ref_osd["state"][i].keys() == {"step"} | set(G.STATE[kind]) and st["step"] == ref_osd["state"][i]["step"] == 3
        assert all(torch.equal(st[k], ref_osd["state"][i][k]) for k in G.STATE[kind])


def test_the_skipped_step_names_the_parameter():
    """the same run, stopped behind the planted step: setup_e2e_optimizer gave the optimizer the names"""
    _, _, opt, (name, param) = training_run("adamw", (0, 1), plant_at=1)
    assert opt.last_step_skipped and opt.last_nonfinite_param is param and opt.last_nonfinite_name == name
