"""GPU: every LayerNorm kernel instantiation of csrc/layernorm.hip against the fp64 definition, row by row and column by column
(tests/layernorm_ref.py: definition, metrics, gates, input families and the case table this file shares with
tests/test_layernorm_ref_cpu.py, which shows that fourteen wrong kernels fail these gates).  Every output lies in a guard buffer, every
case logs its worst row to the parity log of tests/gpu_util.py and asserts that a second run gives the same bits; the refusals at the
end are host checks: nothing there launches a kernel."""
import json
import os

import pytest
import torch

from tests import layernorm_ref as R
from tests.gpu_util import OUT
from tests.guarded import Guarded, GuardedWorkspaces

pytestmark = pytest.mark.gpu
NAN = float("nan")
_worst = {}


def _log(v):
    os.makedirs(OUT, exist_ok=True)
    lines = v.lines()
    print("\n".join(lines))
    with open(os.path.join(OUT, "parity_log.txt"), "a") as f:
        f.write("\n".join(lines) + "\n")
    v.worst_by_group(_worst)
    with open(os.path.join(OUT, "layernorm_contract_worst.json"), "w") as f:
        json.dump({f"{k[0]} {k[1]}": {"u": m, "gate_u": g, "case": c} for k, (m, g, c) in sorted(_worst.items())}, f, indent=1)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _dev(inp):
    d = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    d["x"] = d["xbuf"][inp["x_off"]:]
    return d


# ------------------------------------------------------------------------------------------------------------------ forward
def _fwd(case, d, y_side=False):
    """one forward launch into guard buffers -> (outputs on the CPU, the guards)"""
    from xpretrain_amd import hip_ops as H
    rows, cols = case.rows, case.cols
    ldy = cols + case.ldy_pad
    gy, gm, gr = Guarded(rows, ldy, case.tdtype), Guarded(1, rows, torch.float32), Guarded(1, rows, torch.float32)
    ys = torch.full_like(d["x_side"], NAN) if y_side else None
    H.layernorm_fwd(d["x"], d["gamma"], d["beta"], rows, cols, ldx=d["ldx"], eps=case.eps, x_side=d.get("x_side"), y_side=ys,
                    side=case.side, ldy=ldy, y=gy.mat, mean=gm.mat, rstd=gr.mat)
    torch.cuda.synchronize()
    gy.check(f"{case.id} y", rows, cols)                       # no gap column, no tail row
    gm.check(f"{case.id} mean", 1, rows)
    gr.check(f"{case.id} rstd", 1, rows)
    out = {"y": gy.mat[:, :cols].cpu(), "mean": gm.mat[0].cpu(), "rstd": gr.mat[0].cpu(), "y_side": None if ys is None else ys.cpu()}
    return out, (gy, gm, gr, ys)


@pytest.mark.parametrize("case", R.FWD_CASES, ids=lambda c: c.id)
def test_forward(case):
    inp = R.build(case)
    d = _dev(inp)
    if case.kernel == "ln_fwd_kernel<bf16_t>" and case.cols % 8 == 0:          # cases that must be forced onto the 8-byte kernel
        assert d["ldx"] % 8 or d["x"].data_ptr() % 16
    out, g1 = _fwd(case, d, y_side=bool(case.side))
    v = R.judge_fwd(case, inp, out)
    _log(v)
    v.assert_ok()
    out2, g2 = _fwd(case, d, y_side=bool(case.side))
    for a, b in zip(g1[:3], g2[:3]):
        assert _same_bits(a.flat, b.flat), "second run differs"
    if case.side:
        assert _same_bits(g1[3], g2[3])
        ro, _ = _fwd(case, d, y_side=False)                                     # read-only form: the same y, mean, rstd
        assert all(_same_bits(ro[k], out[k]) for k in ("y", "mean", "rstd"))


# ------------------------------------------------------------------------------------------------------------------ backward
def _Defer():
    """a DeferredReduce whose partial-row slot lies in a guard buffer of exactly the requested bytes"""
    from xpretrain_amd import hip_ops as H

    class Defer(H.DeferredReduce):
        def slot(self, nbytes, name):
            assert nbytes % 4 == 0
            self.nbytes, self.guard = nbytes, Guarded(1, nbytes // 4, torch.float32)
            return self.guard.mat.view(-1).view(torch.uint8)
    return Defer(torch.device("cuda"))


def _stats(case, d):
    from xpretrain_amd import hip_ops as H
    _, mean, rstd = H.layernorm_fwd(d["x"], d["gamma"], d["beta"], case.rows, case.cols, ldx=d["ldx"], eps=case.eps, x_side=d.get("x_side"),
                                    side=case.side)
    return mean, rstd


def _bwd(case, d, mean, rstd, form=None, alias=False, accumulate=False, contiguous=False):
    """one backward call -> (outputs on the CPU, dx's guard)"""
    from xpretrain_amd import hip_ops as H
    rows, cols, mode = case.rows, case.cols, case.mode
    form = form or case.form
    ld = d["ldx"]
    dy, x = d["dybuf"], d["x"]
    if contiguous and ld != cols:                     # the same rows, packed
        dy = dy.as_strided((rows, cols), (ld, 1)).contiguous()
        x = x.as_strided((rows, cols), (ld, 1)).contiguous()
        ld = cols
    span = ld // cols if ld % cols == 0 else 1
    gdx = Guarded(rows * span, cols, case.tdtype) if span > 1 else Guarded(rows, ld, case.tdtype)
    dres, lddres = d["dres"], cols
    if alias:
        gdx.mat.view(-1).as_strided((rows, cols), (ld, 1)).copy_(dres)
        dres, lddres = gdx.mat, ld
    kw = dict(ldx=ld, lddy=ld, dres=dres, dx=gdx.mat, lddx=ld, lddres=lddres, x_side=d.get("x_side"), side=case.side)
    out = {}
    if form == "immediate":
        dg, db = torch.full((cols,), 3.0, device="cuda"), torch.full((cols,), 3.0, device="cuda")
        with GuardedWorkspaces() as gw:               # a workspace of exactly xp_layernorm_bwd_workspace_bytes
            H.layernorm_bwd(dy, x, d["gamma"], mean, rstd, rows, cols, dgamma=dg, dbeta=db, accumulate=accumulate, **kw)
        gw.check()
        assert [r[1] for r in gw.records] == [H.L.lib().xp_layernorm_bwd_workspace_bytes(rows, cols)]
        out.update(dgamma=dg.cpu(), dbeta=db.cpu())
    else:
        df = _Defer()
        res = H.layernorm_bwd(dy, x, d["gamma"], mean, rstd, rows, cols, defer=df, dx_colsum=mode >= 1, dres_colsum=mode == 2, name="ln", **kw)
        torch.cuda.synchronize()
        assert df.nbytes == H.L.lib().xp_layernorm_bwd_workspace_bytes(rows, cols)
        nrows, pitch = H.L.lib().xp_layernorm_bwd_partial_rows(rows), (2 + mode) * cols
        assert nrows == R.RE.ln_bwd_blocks(rows)
        df.guard.check(f"{case.id} partial rows", 1, nrows * pitch)           # exactly partial_rows x pitch floats are written
        part = df.guard.mat[0, :nrows * pitch].clone()
        assert bool(torch.isfinite(part).all()), "a partial-row element was not written"
        out["part"] = part.view(nrows, pitch).cpu()
        df.flush()
        for n, t in zip(("dgamma", "dbeta", "colsum_dx", "colsum_dres"), res[1:]):
            out[n] = t.cpu()
    torch.cuda.synchronize()
    written = torch.arange(rows, device="cuda") * span if span > 1 else rows
    gdx.check(f"{case.id} dx", written, cols)
    out["dx"] = gdx.mat.view(-1).as_strided((rows, cols), (ld, 1)).cpu()
    return out, gdx


@pytest.mark.parametrize("case", R.BWD_CASES, ids=lambda c: c.id)
def test_backward(case):
    inp = R.build(case)
    d = _dev(inp)
    mean, rstd = _stats(case, d)
    mc, rc = mean.cpu(), rstd.cpu()
    out, g1 = _bwd(case, d, mean, rstd)
    v = R.judge_bwd(case, inp, mc, rc, out)
    if case.form == "immediate":                       # store was judged above (into buffers that held 3.0); now accumulate
        acc, g3 = _bwd(case, d, mean, rstd, accumulate=True)
        assert _same_bits(g3.flat, g1.flat)
        va = R.judge_bwd(case, inp, mc, rc, {k: acc[k] for k in ("dx", "dgamma", "dbeta")}, accumulated=3.0)
        v.rows += [(n + " (accumulate)", *r) for (n, *r) in va.rows[1:]]
    _log(v)
    v.assert_ok()
    out2, g2 = _bwd(case, d, mean, rstd)
    assert _same_bits(g1.flat, g2.flat), "second run differs (dx)"
    for k in out:
        assert _same_bits(out[k], out2[k]), f"second run differs ({k})"
    if case.form == "deferred" and case.mode == 0 and not case.side:          # deferred and immediate form: the same dx bits
        imm, g4 = _bwd(case, d, mean, rstd, form="immediate")
        assert _same_bits(g4.flat, g1.flat)
        vi = R.judge_bwd(case, inp, mc, rc, {k: imm[k] for k in ("dx", "dgamma", "dbeta")})
        vi.assert_ok()
    if case.dres:                                                            # dres may alias dx
        al, g5 = _bwd(case, d, mean, rstd, alias=True)
        assert _same_bits(al["dx"], out["dx"]), "dres aliasing dx changes dx"
        for k in out:
            assert _same_bits(al[k], out[k]), f"dres aliasing dx changes {k}"
    if case.form == "pooled":                                                # the same five rows, run contiguously
        ct, _ = _bwd(case, d, mean, rstd, contiguous=True)
        for k in out:
            assert _same_bits(ct[k], out[k]), f"strided and contiguous rows differ ({k})"


def test_constant_rows_backward_is_finite():
    """rows of 0.5: x-hat is exactly 0 and rstd = 1 / sqrt(eps); the sweep holds them to the dx gate, here they are looked at alone"""
    case = R.CASES["ln_bwd_kernel<float,2,2>-37x260-deferred"]
    inp = R.build(case)
    d = _dev(inp)
    mean, rstd = _stats(case, d)
    out, _ = _bwd(case, d, mean, rstd)
    const = torch.tensor([f == "const" for f in R.family_of(case.rows, inp["first"])])
    assert int(const.sum()) >= 6 and bool(torch.isfinite(out["dx"][const]).all())
    assert bool((mean.cpu()[const] == 0.5).all())


# ------------------------------------------------------------------------------------------------------------------ refusals
ROWS, COLS, BUF = 4, 8, 4 * 1040
XP_ERR_ARG = -1                 # include/xpretrain_hip.h: refused by a host check, before any launch (a failed launch is -2)


class _Args:
    """valid arguments of the three entry points at 4 x 8; every output in a guard buffer"""

    def __init__(self, dtype=torch.bfloat16):
        from xpretrain_amd import hip_ops as H
        self.H, self.lib = H, H.L.lib()
        dev = "cuda"
        self.x, self.dy, self.dres = (torch.ones(BUF, dtype=dtype, device=dev) for _ in range(3))
        self.gamma, self.beta = torch.ones(1040, device=dev), torch.zeros(1040, device=dev)
        self.mean_in, self.rstd_in = torch.zeros(ROWS, device=dev), torch.ones(ROWS, device=dev)
        self.x_side = torch.ones(BUF, device=dev)
        self.y, self.dx = Guarded(1, BUF, dtype), Guarded(1, BUF, dtype)
        self.mean, self.rstd = Guarded(1, ROWS, torch.float32), Guarded(1, ROWS, torch.float32)
        self.dgamma, self.dbeta, self.y_side = Guarded(1, 1040, torch.float32), Guarded(1, 1040, torch.float32), Guarded(1, BUF, torch.float32)
        self.ws_bytes = self.lib.xp_layernorm_bwd_workspace_bytes(ROWS, 1028)
        self.ws = Guarded(1, self.ws_bytes // 4, torch.float32)
        self.dt = H._dt(self.x)

    def fwd(self, cols=COLS, ldx=None, ldy=None, dtype=None, x_side=False, y_side=False, S=2, M=1, stride=1):
        p = self.H._p
        return self.lib.xp_layernorm_fwd_side(p(self.x), ldx or cols, p(self.gamma), p(self.beta), p(self.y.mat), ldy or cols, p(self.mean.mat),
                                              p(self.rstd.mat), ROWS, cols, 1e-5, self.dt if dtype is None else dtype,
                                              p(self.x_side if x_side else None), p(self.y_side.mat if y_side else None), S, M, stride,
                                              self.H._stream())

    def bwd(self, form, cols=COLS, lddy=None, ldx=None, lddx=None, lddres=None, dtype=None, dres=True, colsum=0, ws_short=0, x_side=False,
            S=2, M=1, stride=1, dgamma=True):
        p = self.H._p
        nb = self.lib.xp_layernorm_bwd_workspace_bytes(ROWS, cols) - ws_short if cols % 4 == 0 and cols <= 1024 else self.ws_bytes
        head = (p(self.dy), lddy or cols, p(self.x), ldx or cols, p(self.gamma), p(self.mean_in), p(self.rstd_in), p(self.dres if dres else None),
                lddres or cols, p(self.dx.mat), lddx or cols)
        tail = (ROWS, cols, self.dt if dtype is None else dtype, p(self.x_side if x_side else None), S, M, stride, p(self.ws.mat), nb,
                self.H._stream())
        if form == "immediate":
            assert colsum == 0
            return self.lib.xp_layernorm_bwd_side(*head, p(self.dgamma.mat if dgamma else None), p(self.dbeta.mat), 0, *tail)
        return self.lib.xp_layernorm_bwd_partials_side(*head, colsum, *tail)

    def untouched(self, tag):
        torch.cuda.synchronize()
        for n in ("y", "dx", "mean", "rstd", "dgamma", "dbeta", "y_side", "ws"):
            getattr(self, n).check(f"{tag}: {n}", 0, 0)


FWD_REFUSALS = {
    "cols=6": dict(cols=6, ldx=8, ldy=8),       # (every ld stays a multiple of 4: the width alone is what is refused)
    "cols=1028": dict(cols=1028), "ldx=10": dict(ldx=10), "ldy=10": dict(ldy=10), "dtype=2": dict(dtype=2),
    "side_M>side_S": dict(x_side=True, S=2, M=3, stride=3), "side_stride<side_M": dict(x_side=True, S=4, M=2, stride=1),
    "side_S=0,x_side": dict(x_side=True, S=0, M=1, stride=1), "side_S=0,y_side": dict(y_side=True, S=0, M=1, stride=1),
}
BWD_REFUSALS = {
    "cols=6": dict(cols=6, lddy=8, ldx=8, lddx=8, lddres=8),
    "cols=1028": dict(cols=1028), "lddy=10": dict(lddy=10), "ldx=10": dict(ldx=10), "lddx=10": dict(lddx=10),
    "lddres=10": dict(lddres=10), "dtype=2": dict(dtype=2), "workspace one byte short": dict(ws_short=1),
    "side_M>side_S": dict(x_side=True, S=2, M=3, stride=3), "side_stride<side_M": dict(x_side=True, S=4, M=2, stride=1),
    "side_S=0,x_side": dict(x_side=True, S=0, M=1, stride=1),
}
PARTIALS_ONLY = {"with_dx_colsum=2 without dres": dict(colsum=2, dres=False), "with_dx_colsum=3": dict(colsum=3)}
IMMEDIATE_ONLY = {"NULL dgamma": dict(dgamma=False)}


def test_valid_arguments_are_accepted():
    """the argument sets the refusals below vary are themselves accepted (so each refusal is caused by the one change)"""
    a = _Args()
    assert a.fwd() == 0 and a.fwd(x_side=True, y_side=True) == 0
    assert a.bwd("immediate") == 0 and a.bwd("partials", colsum=2, x_side=True) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("what", list(FWD_REFUSALS))
def test_forward_refuses(what):
    a = _Args()
    assert a.fwd(**FWD_REFUSALS[what]) == XP_ERR_ARG, f"xp_layernorm_fwd_side did not refuse {what} as an argument error"
    assert a.lib.xp_last_error()
    a.untouched(what)


@pytest.mark.parametrize("form,what", [(f, w) for f in ("immediate", "partials") for w in BWD_REFUSALS] +
                         [("partials", w) for w in PARTIALS_ONLY] + [("immediate", w) for w in IMMEDIATE_ONLY])
def test_backward_refuses(form, what):
    a = _Args()
    kw = {**BWD_REFUSALS, **PARTIALS_ONLY, **IMMEDIATE_ONLY}[what]
    assert a.bwd(form, **kw) == XP_ERR_ARG, f"the {form} form did not refuse {what} as an argument error"
    assert a.lib.xp_last_error()
    a.untouched(f"{form} {what}")
