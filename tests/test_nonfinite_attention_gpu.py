"""GPU: NaN and +Inf planted in one element of qkv (q of a proxy row and of a frame row, k of a proxy key, k and v of a key in the last
frame, k of a padded position) and of dout, through xp_attn_fwd / xp_attn_bwd2 driven as tests/test_attention_guarded_gpu.py::_run
drives them: regime flat, the fused, wide (default and the wide backward switch), general and fp32 kernels, proxy and causal masks.
The other sample and the other heads keep their bits; NaN in the ldqkv / ldo padding changes nothing.  tests/nonfinite.py states
the rule, tests/test_nonfinite_cpu.py proves the reference side.  (No +-Inf in k: inf * q takes q's sign and exact-zero underflow
differs between the reference's precisions.)"""
import pytest
import torch

from tests import attn_emulation as E
from tests import nonfinite as NF
from tests import nonfinite_cases as NC
from tests.test_attention_gpu import F32, check_kernels
from tests.test_attention_guarded_gpu import KERNELS

pytestmark = pytest.mark.gpu


def _run(case, variant, pitch_pad=False, pad_value=0.0):
    from xpretrain_amd import _lib as L
    from xpretrain_amd import hip_ops as Hh
    name, dt = case.extra["name"], case.extra["dt"]
    dtype = NC.ATTN_DT[dt]
    size, B, H, S, mode = E.CASES[name]
    D, rows = H * 64, B * S
    amode = L.ATTN_PROXY if size is not None else L.ATTN_CAUSAL
    M, N, Lp = size if size is not None else (0, 1, S)
    ldq, ldo = 3 * D + (16 if pitch_pad else 0), D + (8 if pitch_pad else 0)
    pad = None if case.extra["pad"] is None else case.extra["pad"].cuda()
    kernels = F32 if dt == "fp32" else KERNELS[name]
    if variant == "wide":
        kernels = (Hh.attn_plan(B, S, H, size=size)["kernel"], "bwd6")
    check_kernels(kernels, B, S, H, size=size, pad=pad is not None, dtype=dtype)

    def padded(t, ld):
        store = torch.full((t.shape[0], ld), pad_value, dtype=t.dtype, device="cuda")
        store[:, :t.shape[1]] = t.cuda()
        return store

    def run(inputs):
        qkv, dout = padded(inputs["qkv"], ldq), padded(inputs["dout"], ldo)
        out = torch.zeros((rows, ldo), dtype=dtype, device="cuda")
        dqkv = torch.zeros((rows, ldq), dtype=dtype, device="cuda")
        stats = torch.zeros((B * H * S, 2), dtype=torch.float32, device="cuda")
        lib, dtc, dev = L.lib(), Hh._dt(qkv), qkv.device
        nrows = int(lib.xp_attn_bwd_colsum_rows(amode, B, H, S, M, N, Lp, dtc))
        part = torch.zeros((max(nrows, 1), 3 * D), dtype=torch.float32, device="cuda")
        ws_bytes = int(lib.xp_attn_workspace_bytes(amode, B, H, M, N, Lp))
        ws = Hh.workspace(ws_bytes, dev, "attn_fwd")
        L.check(lib.xp_attn_fwd(Hh._p(qkv), ldq, Hh._p(out), ldo, Hh._p(stats), Hh._p(pad), amode, B, H, S, M, N, Lp, dtc,
                                Hh._p(ws), ws.numel(), Hh._stream()), "xp_attn_fwd")
        ws_b = Hh.workspace(ws_bytes, dev, "attn_bwd")
        L.check(lib.xp_attn_bwd2(Hh._p(qkv), ldq, Hh._p(out), Hh._p(dout), ldo, Hh._p(stats), Hh._p(pad), Hh._p(dqkv),
                                 E.Q_SCALE, amode, B, H, S, M, N, Lp, dtc, Hh._p(ws_b), ws_b.numel(),
                                 Hh._p(part if nrows else None), Hh._stream()), "xp_attn_bwd2")
        defer = Hh.DeferredReduce(dev)
        if nrows:
            cs = torch.empty(3 * D, dtype=torch.float32, device=dev)
            defer.add(part, 0, cs, nrows, 3 * D, 3 * D)
        else:                                   # fp32 mode: the separate pass over dqkv, as hip_ops.attn_bwd
            cs = Hh.colsum_deferred(dqkv, rows, 3 * D, defer, ldx=ldq, name="dbqkv")
        defer.flush()
        torch.cuda.synchronize()
        heads = lambda t: t.reshape(B, S, H, 64).transpose(1, 2).float().cpu()
        lse = stats.view(B, H, S, 2).sum(-1).cpu()
        if pad is not None:                     # (stats are not defined at padded query positions: left out, as in the guarded test)
            lse = torch.where(case.extra["pad"].bool()[:, None, :], lse, torch.zeros(()))
        got = {"out": heads(out[:, :D]), "lse": lse, "colsum": cs.cpu()}
        for j, n in enumerate(("dq", "dk", "dv")):
            got[n] = heads(dqkv[:, j * D:(j + 1) * D])
        return got
    return run


def _with_variant(variant, fn):
    from xpretrain_amd import hip_ops as Hh
    prev = Hh.get_attn_bwd_wide()
    try:
        if variant == "wide":
            Hh.set_attn_bwd_wide(True)
        return fn()
    finally:
        Hh.set_attn_bwd_wide(prev)


_IDS = [f"{n}-{d}{'-' + v if v else ''}" for n, d, v in NC.ATTN_RUNS]


@pytest.mark.parametrize("name,dt,variant", NC.ATTN_RUNS, ids=_IDS)
def test_attention_carries_a_planted_value_inside_its_head(name, dt, variant):
    """out, the row sums of stats, dq / dk / dv and the bias column sums: non-finite on every query row of the same (b, h) that the
    mask lets see the planted key (on the planted query row and its keys; for dout on what its row's dS and P reach), finite and
    bit-equal in the other sample and the other heads.  A padded key's NaN reaches nothing there, and its own dk / dv stay zero."""
    case = NC.attn_case(name, dt)

    def go():
        run = _run(case, variant)
        n = NF.drive(case, run)
        if "padded_key" in case.extra:
            b, h, j = case.extra["padded_key"]
            p = next(p for p in case.plants if "padded key" in p.where)
            got = run(NF.plant(case.inputs, p.which, p.index, NF.NAN))
            assert not got["dk"][b, h, j].any() and not got["dv"][b, h, j].any(), "a padded key's own dk / dv are not exactly zero"
        return n
    print(f"{name} {dt} {variant}: {_with_variant(variant, go)} required outputs non-finite")


@pytest.mark.parametrize("name,dt,variant", NC.ATTN_RUNS, ids=_IDS)
def test_attention_never_reads_its_padding(name, dt, variant):
    """NaN in the ldqkv / ldo pitch padding of qkv and dout: every output torch.equal to the run with zeros there"""
    case = NC.attn_case(name, dt)
    nan, zero = _with_variant(variant, lambda: [_run(case, variant, True, v)(case.inputs) for v in (NF.NAN, 0.0)])
    NF.check_equal(nan, zero, f"{name} {dt} {variant}")


# ------------------------------------------------------------------------------------------- single-query (pooled) attention
def _run_pooled(case, kv_pad=0, pad_value=0.0):
    from tests import attn_pooled_emulation as P
    from xpretrain_amd import hip_ops as Hh
    B, H, S = P.CASES[NC.POOLED_CASE]
    D = H * 64

    def run(inputs):
        q, dout = inputs["q"].cuda(), inputs["dout"].cuda()
        store = torch.full((B * S, 2 * D + kv_pad), pad_value, dtype=q.dtype, device="cuda")
        store[:, :2 * D] = inputs["kv"].cuda()
        kv = store[:, :2 * D]                                           # rows at pitch 2 D + kv_pad
        out, stats = Hh.attn_pooled_fwd(q, kv, B, S, H)
        defer = Hh.DeferredReduce(q.device)
        dq, dkv, cs = Hh.attn_pooled_bwd(q, kv, out, dout, stats, B, S, H, q_scale=E.Q_SCALE, colsum_defer=defer)
        defer.flush()
        torch.cuda.synchronize()
        dk, dv = dkv.view(B, S, 2, H, 64).float().cpu().unbind(2)
        return {"out": out.view(B, H, 64).float().cpu(), "lse": stats.sum(-1).cpu(), "dq": dq.view(B, H, 64).float().cpu(),
                "dk": dk, "dv": dv, "colsum": cs.cpu()}
    return run


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_pooled_attention_carries_a_planted_value_inside_its_head(dt):
    """xp_attn_pooled_fwd / _bwd at the smallest case with a second key, sample and head: q, k of the first and of the last key, v and
    dout -> out, the row sum of stats, dq, dk / dv of every key and the k / v bias column sums of the same (b, h); the other sample
    and the other head keep their bits; NaN in the kv pitch padding changes nothing"""
    case = NC.pooled_case(dt)
    print(f"{case.name}: {NF.drive(case, _run_pooled(case))} required outputs non-finite")
    NF.check_equal(_run_pooled(case, 16, NF.NAN)(case.inputs), _run_pooled(case, 16, 0.0)(case.inputs), case.name + " kv padding")


# ---------------------------------------------------------------------------------------------------------- attention weights
_PROBS = NC.probs_cases()


@pytest.mark.parametrize("case", _PROBS, ids=[c.name for c in _PROBS])
def test_attention_weights_carry_a_planted_value_along_their_rows(case):
    """xp_attn_probs on the stats xp_attn_fwd returns, proxy and masked causal: q -> its row of weights, k -> the visible entries of every
    row that sees the key; the other sample (and head) keeps its bits; a NaN in v, which the weights do not read, changes nothing"""
    from xpretrain_amd import hip_ops as Hh
    size, B, H, S, mode = E.CASES[case.extra["name"]]
    pad = None if case.extra["pad"] is None else case.extra["pad"].cuda()

    def run(inputs):
        qkv = inputs["qkv"].cuda()
        _, stats = Hh.attn_fwd(qkv, B, S, H, size=size, pad_mask=pad)
        res = Hh.attn_probs(qkv, stats, B, S, H, size=size, pad_mask=pad)
        torch.cuda.synchronize()
        return {"probs": res.cpu()} if size is None else {"proxy": res[0].cpu(), "frame": res[1].cpu()}
    print(f"{case.name}: {NF.drive(case, run)} required outputs non-finite")
