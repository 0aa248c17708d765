"""GPU: the fused clip + Adam / Adamax (+ shadow copies) launch (xp_optim_step) against the unmodified reference's run
(tests/golden/optim_adam_adamax.pt) and against live torch.optim.Adam / Adamax on the CPU in fp64.

Tolerance: the yardstick is the reference's own fp32 arithmetic.  Beside every fp64 reference stands the same optimizer run in fp32 on
the CPU on the same inputs; d_ref is the worst per-tensor deviation of that fp32 run from the fp64 run, max|a - b| over the larger of
max|b| and a scale floor (1e-3 parameters, 1e-6 exp_avg, 1e-9 second state tensor: the floors of tests/test_optim_gpu.py).  The kernel
gets 4 x d_ref per quantity: it does the same fp32 work with other rounding points (explicit fused multiply-adds where torch has
lerp_ / addcdiv_, the norm over chunk partials instead of per-tensor norms).  Norms: 1e-5 relative."""
import copy
import functools

import pytest
import torch

from oracle import clipvip_oracle as O
from tests import optim_family_ref as R
from tests.gpu_util import ModelArgs

pytestmark = pytest.mark.gpu

FLOORS = (1e-3, 1e-6, 1e-9)                  # parameters, exp_avg, exp_avg_sq / exp_inf
MARGIN = 4.0
TORCH = {"adam": torch.optim.Adam, "adamax": torch.optim.Adamax}


def ours(kind):
    from xpretrain_amd import optimization as XO
    return {"adam": XO.Adam, "adamax": XO.Adamax}[kind]


def worst(got, ref, floor):
    """worst over the tensors of max|a - b| / max(max|b|, floor)"""
    return max(((a.detach().cpu().double() - b.double()).abs().max() / max(b.abs().max().item(), floor)).item() for a, b in zip(got, ref))


def hold(tag, got, ref64, ref32):
    """got, ref64, ref32: (parameters, first state tensors, second state tensors); prints d_ref and the kernel's deviation per quantity,
    then asserts deviation <= MARGIN * d_ref"""
    lines, ok = [], True
    for name, floor, g, r64, r32 in zip(("p", "state_a", "state_b"), FLOORS, got, ref64, ref32):
        d_ref, dev = worst(r32, r64, floor), worst(g, r64, floor)
        lines.append(f"{tag} {name}: d_ref {d_ref:.3e} kernel {dev:.3e} bound {MARGIN * d_ref:.3e} {'OK' if dev <= MARGIN * d_ref else 'FAIL'}")
        ok = ok and dev <= MARGIN * d_ref
    print("\n".join(lines))
    assert ok, "\n".join(lines)


def state_of(opt, params, kind):
    return tuple([opt.state[p][k] for p in params] for k in R.STATE[kind])


# ------------------------------------------------------------------------------------------ a. the reference's run
@pytest.mark.parametrize("kind", R.KINDS)
def test_fixture_run(golden, kind):
    """The reference's setup_e2e_optimizer(optim=kind) run through clip_and_step.  fp64: the restatement on the fixture's inputs
    (pinned to the fixture by tests/test_optim_family_cpu.py); fp32: the fixture itself, torch's own fp32 run."""
    from xpretrain_amd.optimization.utils import build_e2e_optimizer_w_lr_mul
    fx = golden(R.FIXTURE)
    k = fx["kinds"][kind]
    params = [torch.nn.Parameter(p.clone().cuda()) for p in fx["init"]]
    groups = build_e2e_optimizer_w_lr_mul(list(zip(fx["names"], params)), fx["learning_rate"], fx["weight_decay"],
                                          lr_mul=fx["lr_mul"], lr_mul_prefix=fx["lr_mul_prefix"])
    opt = ours(kind)(groups, lr=fx["learning_rate"], betas=tuple(fx["betas"]))
    assert opt.defaults["eps"] == k["eps"]
    for t, gs in enumerate(fx["grads"]):
        for gi, g in enumerate(opt.param_groups):
            g["lr"] = (fx["lr_mul"] if gi < 2 else 1.0) * fx["lrs"][t]
        for p, g in zip(params, gs):
            p.grad = g.clone().cuda()
        norm = opt.clip_and_step(fx["max_norm"])
        assert abs(norm.item() - float(k["norms"][t])) <= 1e-5 * float(k["norms"][t])
    ref64 = R.train_steps(kind, fx["init"], fx["grads"], R.fixture_groups(fx, kind), max_norm=fx["max_norm"])[:3]
    hold(f"{kind} fixture", (params,) + state_of(opt, params, kind), ref64, (k["final"], k["state_a"], k["state_b"]))
    assert [opt.state[p]["step"] for p in params] == k["step"]


# ------------------------------------------------------------------------------------------ b. c. g. ragged shapes against live torch
# (), (1,), (3,), (7, 5): below one vector; 65536 * 2 + 13: three chunks with an unaligned tail; 270 tiny tensors: more than
# XP_OPT_MAX_TENSORS, two launches sharing one partials array; the last parameter starts one element into its buffer: a misaligned base
# pointer, the scalar path for a whole tensor.
SHAPES = [(), (1,), (3,), (7, 5), (65536 * 2 + 13,)] + [(17 + i % 9, 3 + i % 5) for i in range(270)] + [(41, 13)]
STEPS, BETAS = 8, (0.8, 0.95)
GROUPS = (dict(weight_decay=0.3, lr=1e-2), dict(weight_decay=0.0, lr=3e-3))
HALF = len(SHAPES) // 2


@functools.lru_cache(maxsize=None)
def ragged_inputs():
    gen = torch.Generator().manual_seed(5)
    init = [torch.randn(s, generator=gen) * 0.1 for s in SHAPES]
    grads = []
    for t in range(STEPS):
        gs = [torch.randn(s, generator=gen) * 0.05 * (1.0, 0.1, 0.01)[t % 3] for s in SHAPES]
        for g in gs:
            g.view(-1)[3::7] = 0.0                  # every 7th element exactly 0
        grads.append(gs)
    return init, grads


def two_groups(params, half):
    return [dict(params=params[:half], **GROUPS[0]), dict(params=params[half:], **GROUPS[1])]


def torch_run(kind, init, grads, half, clip, eps, dtype, state_dict_after=None):
    """torch's optimizer on the CPU, single-tensor path: (parameters, first, second state tensors), norms[, state_dict and parameters after
    ``state_dict_after`` steps]"""
    params = [torch.nn.Parameter(p.to(dtype).clone()) for p in init]       # (.to alone aliases an fp32 input)
    opt = TORCH[kind](two_groups(params, half), betas=BETAS, eps=eps, foreach=False)
    norms, mid = [], None
    for t, gs in enumerate(grads):
        for p, g in zip(params, gs):
            p.grad = g.to(dtype).clone()                                         # (clip_grad_norm_ scales it in place)
        if clip:
            norms.append(float(torch.nn.utils.clip_grad_norm_(params, clip, foreach=False)))
        opt.step()
        if t + 1 == state_dict_after:
            mid = (copy.deepcopy(opt.state_dict()), [p.detach().clone() for p in params])
    out = tuple([p.detach() for p in params] if k is None else [opt.state[p][k] for p in params] for k in (None,) + R.STATE[kind])
    return (out, norms) if state_dict_after is None else (out, norms, mid)


@functools.lru_cache(maxsize=None)
def ragged_reference(kind, clip, eps, dtype):
    init, grads = ragged_inputs()
    return torch_run(kind, init, grads, HALF, clip, eps, dtype)


@functools.lru_cache(maxsize=None)
def ragged_gpu(kind, clip, eps, rep=0):
    init, grads = ragged_inputs()
    params = [torch.nn.Parameter(p.clone().cuda()) for p in init[:-1]]
    buf = torch.zeros(init[-1].numel() + 1, device="cuda")
    buf[1:] = init[-1].reshape(-1).cuda()
    params.append(torch.nn.Parameter(buf[1:].view(init[-1].shape)))
    assert params[-1].data_ptr() % 16 == 4 and params[-1].is_contiguous()
    opt = ours(kind)(two_groups(params, HALF), betas=BETAS, eps=eps)
    norms = []
    for gs in grads:
        for p, g in zip(params, gs):
            p.grad = g.clone().cuda()
        opt.step(max_grad_norm=clip)
        if clip:
            norms.append(opt.last_grad_norm.item())
    assert len(opt._plan["launches"]) == 2 and opt._plan["n_chunks"] == len(SHAPES) + 2
    assert all(opt.state[p]["step"] == STEPS for p in params)
    return tuple([t.detach().cpu() for t in ts] for ts in (params,) + state_of(opt, params, kind)), norms


def ragged_case(kind, clip, eps):
    got, norms = ragged_gpu(kind, clip, eps)
    ref64, norms64 = ragged_reference(kind, clip, eps, torch.float64)
    ref32, _ = ragged_reference(kind, clip, eps, torch.float32)
    if clip:
        assert len(norms) == STEPS
        for a, b in zip(norms, norms64):
            assert abs(a - b) <= 1e-5 * b
        assert norms64[0] > clip and norms64[-1] > clip          # the clip is active (and idle at the x0.01 steps: both sides of the min)
        assert min(norms64) < clip
    hold(f"{kind} ragged clip={clip} eps={eps:g}", got, ref64, ref32)
    for ts in got:
        assert all(torch.isfinite(t).all() for t in ts)


@pytest.mark.parametrize("clip", [None, 0.5])
@pytest.mark.parametrize("kind", R.KINDS)
def test_ragged_run_against_live_torch(kind, clip):
    """Eight steps, two groups (coupled decay 0.3 at lr 1e-2; none at lr 3e-3), every path of the kernel (SHAPES), gradients with exact
    zeros and magnitudes x1, x0.1, x0.01 by step.  Applying the decay decoupled would move the result by about 1."""
    ragged_case(kind, clip, 1e-8)


@pytest.mark.parametrize("clip", [None, 0.5])
@pytest.mark.parametrize("kind", R.KINDS)
def test_large_eps_pins_where_eps_sits(kind, clip):
    """eps = 1e-3 is on the scale of the gradients: eps outside the bias correction (Adam) or outside the max operand (Adamax) moves the
    result by 9.9e-2 / 1.9e-3 here, against 4e-4 / 1e-7 at eps = 1e-8."""
    ragged_case(kind, clip, 1e-3)


@pytest.mark.parametrize("clip", [None, 0.5])
@pytest.mark.parametrize("kind", R.KINDS)
def test_two_identical_runs_are_bit_identical(kind, clip):
    (a, na), (b, nb) = ragged_gpu(kind, clip, 1e-8), ragged_gpu(kind, clip, 1e-8, rep=1)
    assert a is not b and na == nb
    for ta, tb in zip(a, b):
        assert all(torch.equal(x, y) for x, y in zip(ta, tb))


# ------------------------------------------------------------------------------------------ d. shadows
@pytest.mark.parametrize("kind", R.KINDS)
def test_step_rewrites_weight_shadows(kind):
    """The update kernel rewrites the bf16 / fused f32 copies held by functional.WEIGHTS in the same pass: the same buffers, equal to the
    new parameters bit for bit after each step; a parameter without a gradient gets no state."""
    from xpretrain_amd.functional import WEIGHTS
    torch.manual_seed(9)
    wq, wk, wv = (torch.nn.Parameter(torch.randn(64, 32, device="cuda") * 0.1) for _ in range(3))
    bq, bk, bv = (torch.nn.Parameter(torch.randn(64, device="cuda") * 0.1) for _ in range(3))
    w1 = torch.nn.Parameter(torch.randn(96, 64, device="cuda") * 0.1)
    frozen = torch.nn.Parameter(torch.randn(16, 16, device="cuda"))
    bf = torch.bfloat16
    fq, fb, s1 = WEIGHTS.fused((wq, wk, wv), bf), WEIGHTS.fused((bq, bk, bv), torch.float32), WEIGHTS.get(w1, bf)
    WEIGHTS.get(frozen, bf)
    opt = ours(kind)([wq, wk, wv, bq, bk, bv, w1, frozen], lr=1e-2, weight_decay=0.1)
    for step in range(2):
        before = w1.detach().clone()
        casts = WEIGHTS.casts
        for p in (wq, wk, wv, bq, bk, bv, w1):
            p.grad = torch.randn_like(p)
        opt.step(max_grad_norm=1.0)
        assert not torch.equal(before, w1.detach())
        assert WEIGHTS.fused((wq, wk, wv), bf).data_ptr() == fq.data_ptr()
        assert WEIGHTS.fused((bq, bk, bv), torch.float32).data_ptr() == fb.data_ptr()
        assert WEIGHTS.get(w1, bf).data_ptr() == s1.data_ptr()
        assert WEIGHTS.casts == casts                            # no cast kernel ran for the stepped parameters
        assert torch.equal(fq, torch.cat([wq, wk, wv]).detach().to(bf))
        assert torch.equal(fb, torch.cat([bq, bk, bv]).detach())
        assert torch.equal(s1, w1.detach().to(bf))
        assert torch.equal(WEIGHTS.get(frozen, bf), frozen.detach().to(bf))
    assert len(opt.state[frozen]) == 0
    assert set(opt.state[w1]) == {"step"} | set(R.STATE[kind])


# ------------------------------------------------------------------------------------------ e. resume
RESUME_SHAPES = [(33, 17), (17,), (), (300, 70)]


@functools.lru_cache(maxsize=None)
def resume_inputs():
    gen = torch.Generator().manual_seed(2)
    return ([torch.randn(s, generator=gen) * 0.1 for s in RESUME_SHAPES],
            [[torch.randn(s, generator=gen) * 0.1 for s in RESUME_SHAPES] for _ in range(4)])


def gpu_steps(params, opt, grads, clip=1.0):
    for gs in grads:
        for p, g in zip(params, gs):
            p.grad = g.clone().cuda()
        opt.clip_and_step(clip)


@pytest.mark.parametrize("kind", R.KINDS)
def test_resume_from_a_torch_checkpoint(kind):
    """E2E_TrainingRestorer-style resume (utils/load_save.py:306-314) across the two implementations: torch's state_dict after 2 steps
    (fp64 on the CPU, ``step`` a scalar tensor) loads into this optimizer; two more steps give what torch's uninterrupted 4-step run
    gives."""
    init, grads = resume_inputs()
    ref64, _, (sd, mid) = torch_run(kind, init, grads, 2, 1.0, 1e-8, torch.float64, state_dict_after=2)
    ref32, _ = torch_run(kind, init, grads, 2, 1.0, 1e-8, torch.float32)
    assert all(torch.is_tensor(st["step"]) for st in sd["state"].values())
    params = [torch.nn.Parameter(p.float().cuda()) for p in mid]
    opt = ours(kind)(two_groups(params, 2), betas=BETAS)
    opt.load_state_dict(sd)
    assert all(opt.state[p]["step"] == 2 and type(opt.state[p]["step"]) is int for p in params)
    assert all(opt.state[p][k].dtype == torch.float32 and opt.state[p][k].is_cuda for p in params for k in R.STATE[kind])
    gpu_steps(params, opt, grads[2:])
    hold(f"{kind} resume", (params,) + state_of(opt, params, kind), ref64, ref32)
    assert all(opt.state[p]["step"] == 4 for p in params)


@pytest.mark.parametrize("kind", R.KINDS)
def test_own_state_dict_round_trip_is_bit_identical(kind):
    """state_dict() -> a NEW optimizer -> load_state_dict continues exactly as the uninterrupted run (the step plan follows the replaced
    state tensors)."""
    init, grads = resume_inputs()

    def make(src):
        ps = [torch.nn.Parameter(p.detach().clone().cuda()) for p in src]
        return ps, ours(kind)(two_groups(ps, 2), betas=BETAS)
    pa, oa = make(init)
    gpu_steps(pa, oa, grads)                             # uninterrupted
    pb, ob = make(init)
    gpu_steps(pb, ob, grads[:2])
    sd = ob.state_dict()
    sd = dict(param_groups=copy.deepcopy(sd["param_groups"]),                                # as torch.save / load would
              state={i: {k: (v.cpu().clone() if torch.is_tensor(v) else v) for k, v in st.items()} for i, st in sd["state"].items()})
    assert all(set(st) == {"step"} | set(R.STATE[kind]) and st["step"] == 2 for st in sd["state"].values())
    pc, oc = make(pb)
    oc.load_state_dict(sd)
    gpu_steps(pc, oc, grads[2:])
    for a, c in zip(pa, pc):
        assert torch.equal(a.detach(), c.detach())
    for sa, sc in zip(state_of(oa, pa, kind), state_of(oc, pc, kind)):
        assert all(torch.equal(x, y) for x, y in zip(sa, sc))
    assert all(oc.state[p]["step"] == 4 for p in pc)


# ------------------------------------------------------------------------------------------ f. overlap
_OVL_CFG = O.hf_config_dict(128, 2, 4, 256, 16, 32, 128, 2, 4, 256, 120, 16, 64)


def overlap_run(kind, K):
    """Four clipped steps of the tiny 4-layer model of tests/test_model_gpu.py.  The parameter groups list the early parameters first and
    the late ones (encoder layers >= 1 of both towers) after them -- the order in which the overlapped plan launches them, so both runs sum
    the norm's chunk partials in one order.  (With another group order the clip factor may differ in its last bit between the two runs:
    tests/test_model_gpu.py holds AdamW to 2e-6 for that reason.)"""
    from xpretrain_amd.modeling import VidCLIP
    from xpretrain_amd.optimization import NCELearnableTempLoss
    torch.manual_seed(11)
    model = VidCLIP(ModelArgs(_OVL_CFG, 2)).cuda().train()
    late = {id(p) for m in model.modules() if type(m).__name__ == "CLIPEncoder" for layer in m.layers[1:] for p in layer.parameters()}
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    groups = [dict(params=[p for n, p in named if (id(p) in late) == is_late and (p.ndim < 2) == no_decay], weight_decay=0.0 if no_decay else 0.05)
              for is_late in (False, True) for no_decay in (False, True)]
    assert all(g["params"] for g in groups) and len(late) > 0
    opt = ours(kind)(groups, lr=1e-4, betas=(0.9, 0.98))
    if K is not None:
        opt.overlap_next_forward(model, K)
    video, ids, mask = (t.cuda() for t in O.synthetic_inputs(4, 2, 32, 8, vocab=120))
    trace = []
    for _ in range(4):
        out = model(video, ids, mask)
        loss = NCELearnableTempLoss()(out["vis_features"], out["text_features"], model.clipmodel.logit_scale)
        loss.backward()
        norm = opt.clip_and_step(0.05)
        if K is not None:
            recs = [m.late_update for m in model.modules() if type(m).__name__ == "CLIPEncoder"]
            assert len(recs) == 2 and all(r is not None and r.event is not None and r.first_layer == K for r in recs)
        trace.append((loss.detach().clone(), norm.clone()))
        opt.zero_grad(set_to_none=True)
    sd = {k: v.clone() for k, v in model.state_dict().items()}                  # (pre-hook: waits for the late update)
    osd = opt.state_dict()["state"]
    assert all(float(n) > 0.05 for _, n in trace)                               # the clip is active
    return trace, sd, [osd[i][k].clone() for i in sorted(osd) for k in R.STATE[kind]]


@pytest.mark.parametrize("kind", R.KINDS)
def test_overlapping_the_next_forward_trains_bit_identically(kind):
    (t1, sd1, m1), (t0, sd0, m0) = overlap_run(kind, 1), overlap_run(kind, None)
    for (l0, n0), (l1, n1) in zip(t0, t1):
        assert torch.equal(l0, l1) and torch.equal(n0, n1)
    assert sd0.keys() == sd1.keys() and all(torch.equal(sd0[k], sd1[k]) for k in sd0)
    assert len(m0) == len(m1) and all(torch.equal(a, b) for a, b in zip(m0, m1))
    assert not torch.equal(t0[0][0], t0[-1][0])                                 # the four steps did train


# ------------------------------------------------------------------------------------------ h. error surface
@pytest.mark.parametrize("kind", R.KINDS)
def test_unknown_kind_is_refused_before_any_launch(kind):
    p = torch.nn.Parameter(torch.ones(100, device="cuda"))
    opt = ours(kind)([p], lr=0.1)
    opt._KIND = 7
    p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match=r"xp_optim_step failed \(rc=-1\): xp_optim_step: unknown kind 7"):
        opt.step()
    torch.cuda.synchronize()
    assert torch.equal(p.detach(), torch.ones_like(p))
    assert all(not opt.state[p][k].any() for k in R.STATE[kind])
