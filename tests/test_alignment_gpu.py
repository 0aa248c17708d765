"""GPU: the pointer-alignment rule (include/xpretrain_hip.h, "Pointer alignment"; the table is tests/alignment_cases.py) on real buffers.

  need rows   every refusal of the table with real, pattern-filled buffers: non-zero return, the message, and every operand and
              workspace of the call still holds its pattern -- nothing was launched, cleared or written
  any rows    operands carved from guarded buffers 1 and 3 elements off an aligned base, one at a time and all together: the result
              has the aligned run's bits (alignment_cases.ANY_HELD_TO says why that is the contract of each entry) and the words
              in front of and behind every output still hold their pattern
  Python      a contiguous view one element into its buffer through hip_ops.attn_fwd / gemm / layernorm_fwd / cast: RuntimeError
              carrying the C message
  the floors  LayerNorm forward and backward at a base aligned to their stated N and not to 2N (bf16: 8, fp32: 16) against
              tests/layernorm_ref.py at its own bounds; xp_gemm's uint8 frame tensor refused below 8 bytes and served at 8

No kernel is ever launched on a pointer its class does not serve: a ``need`` row's misaligned call is refused on the host."""
import ctypes as C

import pytest
import torch

from tests import alignment_cases as A
from tests import layernorm_ref as LR
from tests.guarded import Guarded

pytestmark = pytest.mark.gpu
PATTERN = 0xA5
NEED_ROWS = A.need_rows()


def _lib():
    from xpretrain_amd import _lib as L
    return L


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------------------------ need rows
@pytest.mark.parametrize("entry", sorted({r[0] for r in NEED_ROWS}))
def test_a_refused_call_leaves_real_buffers_untouched(entry):
    L = _lib()
    ops = list(A.ROWS[entry])
    # one pattern-filled buffer per operand, each large enough for the table's call (the workspace: the size the call is told)
    size = {o: (A.WS if o.split(".")[-1] == "workspace" else 1 << 20) + 8192 for o in ops}
    bufs = {o: torch.full((size[o],), PATTERN, dtype=torch.uint8, device="cuda") for o in ops}
    base = {o: b.data_ptr() + (-b.data_ptr()) % 4096 for o, b in bufs.items()}
    torch.cuda.synchronize()
    made = 0
    for _, operand, dtype, n, offsets in [r for r in NEED_ROWS if r[0] == entry]:
        for off in offsets:
            at = dict(base)
            at[operand] += off
            args, keep = A.build_call(entry, dtype, at.__getitem__, extra=(operand,))
            rc = getattr(L.lib(), entry)(*args)
            msg = L.lib().xp_last_error().decode()
            assert rc == L.XP_ERR_ARG, (entry, operand, dtype, off, rc, msg)
            assert msg.startswith(entry + ":") and f" {operand}=" in msg and f"is not {n}-byte aligned" in msg, msg
            made += 1
    assert made
    torch.cuda.synchronize()
    for o, b in bufs.items():
        assert bool((b == PATTERN).all()), f"{entry}: a refused call wrote to {o}"


# ------------------------------------------------------------------------------------------------------------------ any rows
SHIFTS = (1, 3)                                  # elements off a 256-byte aligned base


class Carved:
    """`n` elements of `dtype`, `shift` elements behind a 256-byte boundary of a buffer that holds a NaN pattern everywhere else"""
    LEAD = 128

    def __init__(self, src, shift):
        src = src.contiguous()
        self.g = Guarded(1, src.numel() + 8, src.dtype, lead=self.LEAD)
        assert self.g.flat.data_ptr() % 256 == 0
        self.n, self.shift = src.numel(), shift
        self.view = self.g.flat[self.LEAD + shift:self.LEAD + shift + self.n].view(src.shape)
        self.view.copy_(src)
        assert self.view.data_ptr() % 16 == (shift * src.element_size()) % 16 and self.view.is_contiguous()

    def check(self, tag):
        """nothing but the window was written"""
        flat = self.g.flat.view(self.g.itype)
        lo = self.LEAD + self.shift
        assert bool((flat[:lo] == self.g.sent).all()) and bool((flat[lo + self.n:] == self.g.sent).all()), f"{tag}: written outside its window"


def shift_plans(names):
    """no shift; each operand alone by 1 and by 3 elements; all together"""
    plans = [dict.fromkeys(names, 0)]
    for s in SHIFTS:
        plans += [dict(dict.fromkeys(names, 0), **{n: s}) for n in names]
        plans.append(dict.fromkeys(names, s))
    return plans


def run_shifted(names, inputs, call, outputs):
    """call(carved views by name) for every shift plan; the outputs of every plan equal the unshifted run's, bit for bit"""
    first = None
    for plan in shift_plans(names):
        carved = {n: Carved(inputs[n], plan[n]) for n in names}
        call({n: c.view for n, c in carved.items()})
        torch.cuda.synchronize()
        for n, c in carved.items():
            c.check(f"{n} at shifts {plan}")
        got = {n: carved[n].view.clone() for n in outputs}
        if first is None:
            first = got
            assert all(not torch.equal(got[n], inputs[n]) for n in outputs), "the unshifted run wrote nothing"
        for n in outputs:
            assert torch.equal(got[n].view(torch.int32) if got[n].dtype == torch.float32 else got[n],
                               first[n].view(torch.int32) if first[n].dtype == torch.float32 else first[n]), (n, plan)


def _feats(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=-1).cuda()


def test_sim_matrix_serves_any_element_aligned_base():
    L = _lib()
    na, nb, d = 5, 7, 30
    inputs = dict(a=_feats(na, d, 1), b=_feats(nb, d, 2), sim=torch.full((na, nb), 7.0, device="cuda"))

    def call(v):
        L.check(L.lib().xp_sim_matrix(v["a"].data_ptr(), v["b"].data_ptr(), v["sim"].data_ptr(), na, nb, d, _stream()), "xp_sim_matrix")
    run_shifted(("a", "b", "sim"), inputs, call, ("sim",))


def test_reduce_rows_batch_serves_any_element_aligned_base():
    """two segments -- 70 rows (both levels) of width 8 at pitch 12, 3 rows (direct) of width 260 accumulated -- whose widths and
    pitches allow the four-column kernels: a base off 16 bytes selects the one-column kernels, same tree per column"""
    L = _lib()
    g = torch.Generator().manual_seed(3)
    segs = [(70, 8, 12, 0), (3, 260, 260, 1)]
    inputs = {}
    for i, (nrows, width, stride, acc) in enumerate(segs):
        inputs[f"in{i}"] = torch.randn(nrows * stride, generator=g).cuda()
        inputs[f"out{i}"] = torch.randn(width, generator=g).cuda()

    def call(v):
        arr = (L.XpReduceSeg * len(segs))()
        for i, (nrows, width, stride, acc) in enumerate(segs):
            arr[i].in_, arr[i].out = v[f"in{i}"].data_ptr(), v[f"out{i}"].data_ptr()
            arr[i].stride, arr[i].nrows, arr[i].width, arr[i].accumulate = stride, nrows, width, acc
        nb = L.lib().xp_reduce_rows_batch_workspace_bytes(arr, len(segs))
        assert nb % 4 == 0
        L.check(L.lib().xp_reduce_rows_batch(arr, len(segs), v["ws"].data_ptr(), nb, _stream()), "xp_reduce_rows_batch")
    arr = (L.XpReduceSeg * len(segs))()
    for i, (nrows, width, stride, acc) in enumerate(segs):
        arr[i].width = width
    inputs["ws"] = torch.zeros(L.lib().xp_reduce_rows_batch_workspace_bytes(arr, len(segs)) // 4, device="cuda")
    run_shifted(tuple(inputs), inputs, call, ("out0", "out1"))
    ref = inputs["in1"].view(3, 260).double().sum(0) + inputs["out1"].double()          # (and the sums are sums)
    c = Carved(inputs["out1"], 0)
    call(dict({k: Carved(t, 0).view for k, t in inputs.items()}, out1=c.view))
    assert (c.view.double() - ref).abs().max().item() < 1e-5


RS = dict(nq=70, ng=133, d=32, k=5, theta=10.0)             # more than one gallery tile, a ragged last tile, d % 4 == 0 (the 16-byte path)


def _rs_inputs():
    return dict(q=_feats(RS["nq"], RS["d"], 11), g=_feats(RS["ng"], RS["d"], 12))


def test_retrieval_ranks_streamed_serves_any_element_aligned_base():
    from xpretrain_amd import hip_ops as H
    res = []
    for plan in shift_plans(("q", "g")):
        c = {n: Carved(t, plan[n]) for n, t in _rs_inputs().items()}
        for dsl in (False, True):
            out = H.retrieval_ranks_streamed(c["q"].view, c["g"].view, labels_q=list(range(RS["nq"])), labels_g=[j % RS["nq"] for j in range(RS["ng"])],
                                             dsl=dsl, theta=RS["theta"])
            torch.cuda.synchronize()
            res.append((plan, dsl, [t.cpu() for t in out]))
        for n in c:
            c[n].check(n)
    for plan, dsl, out in res:
        base = next(o for p, s, o in res if s == dsl and not any(p.values()))
        assert all(torch.equal(a, b) for a, b in zip(out, base)), (plan, dsl)
    assert int(res[0][2][1].sum()) >= RS["nq"]                       # every label's own entry counts as equal


@pytest.mark.parametrize("dsl_of", [None, "gallery", "queries"])
def test_retrieval_topk_and_dsl_stats_serve_any_element_aligned_base(dsl_of):
    from xpretrain_amd import hip_ops as H
    res = []
    for plan in shift_plans(("q", "g") if dsl_of is None else ("q", "g", "mx", "sum")):
        c = {n: Carved(t, plan[n]) for n, t in _rs_inputs().items()}
        q, g = c["q"].view, c["g"].view
        if dsl_of is None:
            out = H.retrieval_topk(q, g, RS["k"])
        else:                                       # the statistics: formed over q, g where they lie, searched with from a shifted copy
            over, of = (q, g) if dsl_of == "gallery" else (g, q)
            stats = H.retrieval_dsl_stats(over, of, theta=RS["theta"])
            c.update(mx=Carved(stats[0], plan["mx"]), sum=Carved(stats[1], plan["sum"]))
            out = H.retrieval_topk(q, g, RS["k"], dsl=(c["mx"].view, c["sum"].view), dsl_of=dsl_of, theta=RS["theta"]) + stats
        torch.cuda.synchronize()
        for n in c:
            c[n].check(n)
        res.append((plan, [t.cpu() for t in out]))
    for plan, out in res[1:]:
        assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
                   for a, b in zip(out, res[0][1])), plan
    assert torch.isfinite(res[0][1][0]).all()


# ---- the optimizer: one tensor of three chunks with a ragged tail, every pointer of the table and the gradient shifted
OPT_N = 65536 * 2 + 13


def _optim_run(kind, guarded, plan):
    L = _lib()
    lib = L.lib()
    g = torch.Generator().manual_seed(21)
    src = dict(p=torch.randn(OPT_N, generator=g) * 0.1, m=torch.randn(OPT_N, generator=g) * 0.01, v=torch.rand(OPT_N, generator=g) * 1e-3,
               grad=torch.randn(OPT_N, generator=g) * 0.05, shadow=torch.zeros(OPT_N, dtype=torch.bfloat16), partials=torch.zeros(3))
    c = {n: Carved(t.cuda(), plan.get(n, 0)) for n, t in src.items()}
    t = L.XpAdamTensor()
    t.p, t.m, t.v, t.shadow = (c[n].view.data_ptr() for n in ("p", "m", "v", "shadow"))
    t.numel, t.shadow_dtype = OPT_N, L.XP_BF16
    table = torch.frombuffer(bytearray(bytes(t)), dtype=torch.uint8).cuda()
    chunk_map = torch.tensor([0, 0, 0, 1, 0, 2], dtype=torch.int32, device="cuda")
    grads = (C.c_void_p * 1)(c["grad"].view.data_ptr())
    group_of = (C.c_uint8 * 1)(0)
    L.check(lib.xp_grad_sqnorm_partials(table.data_ptr(), chunk_map.data_ptr(), 3, grads, 1, c["partials"].view.data_ptr(), _stream()),
            "xp_grad_sqnorm_partials")
    tail = ()
    if guarded:
        verdict = torch.zeros(C.sizeof(L.XpStepVerdict), dtype=torch.uint8, device="cuda")
        vp = C.cast(verdict.data_ptr(), C.POINTER(L.XpStepVerdict))
        aligned = c["partials"].view.clone()             # (xp_step_verdict's partials are the whole step's array: need 16)
        L.check(lib.xp_step_verdict(aligned.data_ptr(), 3, vp, _stream()), "xp_step_verdict")
        tail = (vp,)
    if kind == "adamw":
        grp = L.XpAdamGroup()
        grp.lr, grp.beta1, grp.beta2, grp.eps, grp.weight_decay, grp.step_size = 1e-2, 0.8, 0.95, 1e-8, 0.3, 1e-2
        fn = lib.xp_adamw_step_guarded if guarded else lib.xp_adamw_step
        rc = fn(table.data_ptr(), chunk_map.data_ptr(), 3, grads, group_of, 1, C.byref(grp), 1, None, 0, 0.0, None, *tail, _stream())
    else:
        grp = L.XpOptGroup()
        grp.lr, grp.beta1, grp.beta2, grp.eps, grp.weight_decay, grp.step_size = 1e-2, 0.8, 0.95, 1e-8, 0.3, 1e-2
        grp.bias2_sqrt, grp.one_minus_beta1 = 0.5, 0.2
        fn = lib.xp_optim_step_guarded if guarded else lib.xp_optim_step
        rc = fn(L.XP_OPT_ADAM if kind == "adam" else L.XP_OPT_ADAMAX, table.data_ptr(), chunk_map.data_ptr(), 3, grads, group_of, 1, C.byref(grp), 1,
                None, 0, 0.0, None, *tail, _stream())
    L.check(rc, "optimizer step")
    torch.cuda.synchronize()
    for n, cv in c.items():
        cv.check(f"{kind} {n} at shifts {plan}")
    assert torch.equal(c["grad"].view.cpu(), src["grad"])
    return {n: c[n].view.cpu() for n in ("p", "m", "v", "shadow", "partials")}, src


@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guarded"])
@pytest.mark.parametrize("kind", ["adamw", "adam", "adamax"])
def test_optimizer_serves_any_element_aligned_base(kind, guarded):
    """No clipping: the update is element by element, so every shift has the aligned run's bits in p, m, v and the shadow copy.  The
    norm partials change their summation order with the gradient's alignment: held to the fp64 sum at 1e-5, the bound
    tests/test_optim_family_gpu.py holds the norm to."""
    names = ("p", "m", "v", "grad", "shadow", "partials")
    base, src = _optim_run(kind, guarded, {})
    assert not torch.equal(base["p"], src["p"]) and torch.equal(base["shadow"], base["p"].to(torch.bfloat16))
    ref = torch.stack([src["grad"][i * 65536:(i + 1) * 65536].double().square().sum() for i in range(3)])
    for s in SHIFTS:
        for plan in [{n: s} for n in names] + [dict.fromkeys(names, s)]:
            got, _ = _optim_run(kind, guarded, plan)
            for n in ("p", "m", "v"):
                assert torch.equal(got[n].view(torch.int32), base[n].view(torch.int32)), (kind, n, plan)
            assert torch.equal(got["shadow"].view(torch.int16), base["shadow"].view(torch.int16)), (kind, plan)
            assert ((got["partials"].double() - ref).abs() <= 1e-5 * ref).all(), (kind, plan)
    assert ((base["partials"].double() - ref).abs() <= 1e-5 * ref).all()


# ---- the frame transforms: the output at any float, the source at any byte
def _frames_call(entry, src, out, ws=None):
    L = _lib()
    spec = A.CALLS[entry]
    at = {"videos_host[].src": src.data_ptr(), "out": out.data_ptr(), "workspace": 0 if ws is None else ws.data_ptr()}
    args, keep = A.build_call(entry, A.F32, at.__getitem__)
    args[-1] = _stream()
    L.check(getattr(L.lib(), entry)(*args), entry)


@pytest.mark.parametrize("entry", ["xp_frames_resize_norm", "xp_frames_transform", "xp_frames_transform_aa"])
def test_frame_transforms_serve_any_output_and_source_base(entry):
    g = torch.Generator().manual_seed(31)
    inputs = dict(src=torch.randint(0, 256, (8 * 8 * 3,), dtype=torch.uint8, generator=g).cuda(), out=torch.full((3 * 4 * 4,), 9.0, device="cuda"))
    ws = torch.empty(A.WS, dtype=torch.uint8, device="cuda") if entry.endswith("_aa") else None
    first = None
    for plan in shift_plans(("src", "out")):
        src = torch.zeros(8 * 8 * 3 + 16, dtype=torch.uint8, device="cuda")
        s = src[plan["src"]:plan["src"] + 8 * 8 * 3]
        s.copy_(inputs["src"])
        out = Carved(inputs["out"], plan["out"])
        _frames_call(entry, s, out.view, ws)
        torch.cuda.synchronize()
        out.check(f"{entry} out at {plan}")
        got = out.view.cpu()
        first = got if first is None else first
        assert torch.equal(got.view(torch.int32), first.view(torch.int32)), plan
    assert torch.isfinite(first).all() and not torch.equal(first, inputs["out"].cpu())


# ------------------------------------------------------------------------------------------------------------------ through Python
def _off_by_one(t):
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device="cuda")
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == t.element_size()
    return v


def test_python_wrappers_carry_the_refusal():
    from xpretrain_amd import hip_ops as H
    bf = torch.bfloat16
    qkv = torch.randn(2 * 16, 192, device="cuda").to(bf)
    good, _ = H.attn_fwd(qkv, 2, 16, 1, size=(1, 3, 5))
    with pytest.raises(RuntimeError, match=r"xp_attn_fwd: qkv=0x[0-9a-f]+ is not 16-byte aligned"):
        H.attn_fwd(_off_by_one(qkv), 2, 16, 1, size=(1, 3, 5))
    with pytest.raises(RuntimeError, match=r"xp_attn_fwd: out=0x[0-9a-f]+ is not 16-byte aligned"):
        H.attn_fwd(qkv, 2, 16, 1, size=(1, 3, 5), out=_off_by_one(torch.zeros(32, 64, dtype=bf, device="cuda")))
    a, b = torch.randn(128, 128, device="cuda").to(bf), torch.randn(128, 128, device="cuda").to(bf)
    bias = torch.randn(128, device="cuda")
    H.gemm(a, b, 128, 128, 128, epilogue=H.L.EPI_BIAS, bias=bias)
    with pytest.raises(RuntimeError, match=r"xp_gemm: desc.A=0x[0-9a-f]+ is not 16-byte aligned"):
        H.gemm(_off_by_one(a), b, 128, 128, 128, epilogue=H.L.EPI_BIAS, bias=bias)
    with pytest.raises(RuntimeError, match=r"xp_gemm: desc.bias=0x[0-9a-f]+ is not 16-byte aligned"):
        H.gemm(a, b, 128, 128, 128, epilogue=H.L.EPI_BIAS, bias=_off_by_one(bias))
    x = torch.randn(5, 128, device="cuda").to(bf)
    gamma, beta = torch.randn(128, device="cuda"), torch.randn(128, device="cuda")
    with pytest.raises(RuntimeError, match=r"xp_layernorm_fwd: x=0x[0-9a-f]+ is not 8-byte aligned"):
        H.layernorm_fwd(_off_by_one(x), gamma, beta, 5, 128)
    with pytest.raises(RuntimeError, match=r"xp_layernorm_fwd: gamma=0x[0-9a-f]+ is not 16-byte aligned"):
        H.layernorm_fwd(x, _off_by_one(gamma), beta, 5, 128)
    with pytest.raises(RuntimeError, match=r"xp_layernorm_fwd: x=0x[0-9a-f]+ is not 16-byte aligned"):
        H.layernorm_fwd(_off_by_one(x.float()), gamma, beta, 5, 128)
    w = torch.randn(128, device="cuda")
    with pytest.raises(RuntimeError, match=r"xp_cast: src=0x[0-9a-f]+ is not 16-byte aligned"):
        H.cast(_off_by_one(w), bf)
    with pytest.raises(RuntimeError, match=r"xp_cast_back: dst=0x[0-9a-f]+ is not 16-byte aligned"):
        H.cast_back(w.to(bf), out=_off_by_one(torch.zeros(128, device="cuda")), accumulate=True)
    torch.cuda.synchronize()
    again, _ = H.attn_fwd(qkv, 2, 16, 1, size=(1, 3, 5))
    assert torch.equal(good, again)


# ------------------------------------------------------------------------------------------------------------------ the floors
@pytest.mark.parametrize("dtype,cols", [("bf16", 128), ("bf16", 768), ("f32", 128), ("f32", 768)])
def test_layernorm_forward_at_its_stated_floor(dtype, cols):
    """x and y at a base aligned to the class's N and not to 2N -- bf16: 8 bytes (the gate falls from the 16-byte kernel to
    ln_fwd_kernel<bf16_t>, four elements = 8 bytes per lane), fp32: 16 bytes -- five rows; tests/layernorm_ref.py's own bounds"""
    from xpretrain_amd import hip_ops as H
    case = LR.Case("fwd", dtype, 5, cols, x_off=4, tag="floor")
    assert case.kernel == ("ln_fwd_kernel<bf16_t>" if dtype == "bf16" else "ln_fwd_kernel<float>")
    inp = LR.build(case)
    xbuf = inp["xbuf"].cuda()
    x = xbuf[4:]
    esz = x.element_size()
    gy = Guarded(5, cols, case.tdtype, lead=64 + 4)
    assert x.data_ptr() % (8 * esz) == 4 * esz and gy.mat.data_ptr() % (8 * esz) == 4 * esz
    gm, gr = Guarded(1, 5, torch.float32), Guarded(1, 5, torch.float32)
    H.layernorm_fwd(x, inp["gamma"].cuda(), inp["beta"].cuda(), 5, cols, ldx=inp["ldx"], eps=case.eps, y=gy.mat, mean=gm.mat, rstd=gr.mat)
    torch.cuda.synchronize()
    gy.check("y", 5, cols); gm.check("mean", 1, 5); gr.check("rstd", 1, 5)
    v = LR.judge_fwd(case, inp, {"y": gy.mat.cpu(), "mean": gm.mat[0].cpu(), "rstd": gr.mat[0].cpu(), "y_side": None})
    v.assert_ok()


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_layernorm_backward_at_its_stated_floor(dtype):
    """dy, x, dres and dx (need 8/16) at a base aligned to N and not to 2N, five rows of 128 columns, the immediate form;
    tests/layernorm_ref.py's own bounds for dx, dgamma and dbeta"""
    from xpretrain_amd import hip_ops as H
    case = LR.Case("bwd", dtype, 5, 128, x_off=4, form="immediate", tag="floor")
    inp = LR.build(case)
    esz = 2 if dtype == "bf16" else 4

    def at_floor(t):                                   # the same elements, four elements behind an aligned base
        buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device="cuda")
        v = buf[4:4 + t.numel()]
        v.copy_(t.reshape(-1))
        assert v.data_ptr() % (8 * esz) == 4 * esz
        return v
    x = inp["xbuf"].cuda()[4:]
    dy, dres = at_floor(inp["dybuf"]), at_floor(inp["dres"])
    gamma = inp["gamma"].cuda()
    _, mean, rstd = H.layernorm_fwd(x, gamma, inp["beta"].cuda(), 5, 128, ldx=inp["ldx"], eps=case.eps)
    gdx = Guarded(5, 128, case.tdtype, lead=64 + 4)
    assert x.data_ptr() % (8 * esz) == 4 * esz and gdx.mat.data_ptr() % (8 * esz) == 4 * esz
    dg, db = torch.full((128,), 3.0, device="cuda"), torch.full((128,), 3.0, device="cuda")
    H.layernorm_bwd(dy, x, gamma, mean, rstd, 5, 128, ldx=inp["ldx"], lddy=inp["ldx"], dres=dres, lddres=128, dx=gdx.mat, lddx=128,
                    dgamma=dg, dbeta=db)
    torch.cuda.synchronize()
    gdx.check("dx", 5, 128)
    v = LR.judge_bwd(case, inp, mean.cpu(), rstd.cpu(), {"dx": gdx.mat.cpu(), "dgamma": dg.cpu(), "dbeta": db.cpu()})
    v.assert_ok()


def test_gemm_uint8_frames_are_refused_below_8_bytes_and_served_at_8():
    """xp_gemm's desc.a_frames with a_frames_u8 = 1 (alignment_cases.GEMM_U8_FRAMES): refused 1, 2 and 4 bytes off, nothing written;
    at 8 bytes off a 16-byte boundary -- its floor -- the gathered product has the aligned run's bits"""
    L = _lib()
    operand, n, offsets = A.GEMM_U8_FRAMES_NEED
    g = torch.Generator().manual_seed(41)
    frames = torch.randint(0, 256, (2 * 3 * 16 * 16,), dtype=torch.uint8, generator=g)
    fbuf = torch.zeros(frames.numel() + 64, dtype=torch.uint8, device="cuda")
    W = (torch.randn(128, 192, generator=g) * 0.1).to(torch.bfloat16).cuda()
    outs = []
    for off in (0, 8) + tuple(offsets):
        fbuf.zero_()
        fbuf[off:off + frames.numel()].copy_(frames)
        gc = Guarded(8, 128, torch.bfloat16)
        at = {"desc.a_frames": fbuf.data_ptr() + off, "desc.B": W.data_ptr(), "desc.C": gc.mat.data_ptr()}
        args, keep = A.build_call("xp_gemm", A.BF16, at.__getitem__, spec=A.GEMM_U8_FRAMES)
        args[-1] = _stream()
        rc = L.lib().xp_gemm(*args)
        msg = L.lib().xp_last_error().decode()
        torch.cuda.synchronize()
        if off % n:
            assert rc == L.XP_ERR_ARG and msg.startswith("xp_gemm:") and f" {operand}=" in msg and f"is not {n}-byte aligned" in msg, (off, rc, msg)
            gc.check("C of a refused call", 0, 0)
        else:
            assert rc == 0, (off, msg)
            gc.check("C", 8, 128)
            outs.append(gc.mat.cpu())
    assert len(outs) == 2 and torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)) and torch.isfinite(outs[0].float()).all()
    assert float(outs[0].float().abs().max()) > 0
