"""GPU: NaN and +-Inf planted in one element of x (a plain row and an fp32 side row), dy, gamma and dres of the LayerNorm kernels --
every width of layernorm_ref.FWD_WIDTHS / BWD_WIDTHS, both SIDES, bf16 and f32 (tests/nonfinite_cases.py::layernorm_table) -- and NaN
in the bytes the kernels never read.  tests/nonfinite.py states the rule; tests/test_nonfinite_cpu.py proves the reference side."""
import pytest
import torch

from tests import nonfinite as NF
from tests import nonfinite_cases as NC

pytestmark = pytest.mark.gpu
CASES = NC.layernorm_cases()


def _run(case):
    """forward: y, mean, rstd (and the fp32 side output); backward: the forward's mean / rstd on the same x, then dx, dgamma / dbeta
    and the column sums after the deferred reduce (or the immediate form)"""
    from xpretrain_amd import hip_ops as H
    rows, cols = case.rows, case.cols

    def run(inputs):
        d = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in inputs.items()}
        ld = d["xbuf_ld"]
        x = d["xbuf"][case.x_off:]
        if case.kind == "fwd":
            ys = torch.zeros_like(d["x_side"]) if case.side else None
            y, mean, rstd = H.layernorm_fwd(x, d["gamma"], d["beta"], rows, cols, ldx=ld, eps=case.eps, x_side=d.get("x_side"), y_side=ys,
                                            side=case.side, ldy=cols + case.ldy_pad)
            out = {"y": y[:, :cols], "mean": mean, "rstd": rstd}
            if case.side:
                out["y_side"] = ys
            return {k: v.cpu() for k, v in out.items()}
        _, mean, rstd = H.layernorm_fwd(x, d["gamma"], d["beta"], rows, cols, ldx=ld, eps=case.eps, x_side=d.get("x_side"), side=case.side)
        dxbuf = torch.zeros(rows * ld + 8, dtype=case.tdtype, device="cuda")
        kw = dict(ldx=ld, lddy=ld, dres=d.get("dres"), dx=dxbuf, lddx=ld, lddres=cols, x_side=d.get("x_side"), side=case.side)
        if case.form == "immediate":
            res = H.layernorm_bwd(d["dybuf"], x, d["gamma"], mean, rstd, rows, cols, **kw)
        else:
            df = H.DeferredReduce(torch.device("cuda"))
            res = H.layernorm_bwd(d["dybuf"], x, d["gamma"], mean, rstd, rows, cols, defer=df, dx_colsum=case.mode >= 1,
                                  dres_colsum=case.mode == 2, name="ln", **kw)
            df.flush()
        out = {"dx": dxbuf.as_strided((rows, cols), (ld, 1))}
        out.update(zip(("dgamma", "dbeta", "colsum_dx", "colsum_dres"), res[1:]))
        return {k: v.cpu() for k, v in out.items()}
    return run


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_layernorm_carries_a_planted_value_along_its_row(case):
    """x (first row, last row, a row of the second partial-row group; side rows in the fp32 side buffer), dy, gamma, dres: the row of
    y / dx, the statistics, the column of a parameter gradient or column sum that reads the element are non-finite; every other row
    (other column, for gamma in the forward) keeps its bits; the bf16 x of a side row changes nothing"""
    n = NF.drive(case, _run(case.extra["case"]))
    print(f"{case.name}: {n} required outputs non-finite")


PADDED = [c for c in CASES if (lambda k: k.ldx_pad or k.x_off or k.side or k.form == "pooled")(c.extra["case"])]


@pytest.mark.parametrize("case", PADDED, ids=[c.name for c in PADDED])
def test_layernorm_never_reads_its_padding(case):
    """NaN in the ldx / lddy pitch padding, before x_off, behind the last row, in the bf16 x of side rows and in the side rows no row
    maps to: every output torch.equal to the run with zeros there"""
    k = case.extra["case"]
    run = _run(k)
    NF.check_equal(run(NC.layernorm_padding(k, case.inputs, NF.NAN)), run(NC.layernorm_padding(k, case.inputs, 0.0)), case.name)
