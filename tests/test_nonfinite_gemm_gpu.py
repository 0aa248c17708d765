"""GPU: NaN and +Inf planted in one element of a GEMM operand -- a row of A (row 0, the ragged last row, a row of the second row tile),
a row of B, one element of bias / resid / a side row / the patch tables -- for one case per kernel family and epilogue, the tn split-K
cases and the padded ones of tests/gemm_cases.py (tests/nonfinite_cases.py::gemm_selection picks them by field); and NaN in every
element of the operands' storage that the descriptor says is not read.  Launched as tests/test_gemm_plans_gpu.py::run_case launches;
tests/nonfinite.py states the rule, tests/test_nonfinite_cpu.py proves the reference side."""
import pytest
import torch

from tests import gemm_cases as G
from tests import nonfinite as NF
from tests import nonfinite_cases as NC
from tests.test_planning_cpu import case_budget, case_desc, check_plan, resolve_split, set_case_env

pytestmark = pytest.mark.gpu
CASES = NC.gemm_cases()


def _store(val, ks, ld_pad, remap, pad):
    """the storage of a logical [rows][K] operand: [K'][ld] (k-strided) or [rows'][ld] with the row remap; `pad` everywhere else"""
    rows, K = val.shape
    sidx = NC.gemm_remap(*remap, torch.arange(K if ks else rows))
    ld = (rows if ks else K) + ld_pad
    store = torch.full((int(sidx[-1]) + 1, ld), pad, dtype=val.dtype)
    if ks:
        store[sidx, :rows] = val.t()
    else:
        store[sidx, :K] = val
    return store.cuda().contiguous()


def _run(case, pad=0.0):
    """run(inputs) -> the outputs' windows on the CPU; everything the descriptor does not read holds `pad`"""
    from xpretrain_amd import hip_ops as H
    c = case.extra["case"]
    M, N, K, p, epi = c["M"], c["N"], c["K"], c["pad"], c["epi"]
    aks, bks = G.LAYOUTS[c["layout"]]
    dt, ot = NC.GEMM_DT[c["dtype"]], NC.GEMM_DT[c["out"]]
    crow = NC.gemm_remap(*c["c_remap"], torch.arange(M))
    crows = int(crow[-1]) + 1

    def run(inputs):
        kw = dict(a_kstrided=bool(aks), b_kstrided=bool(bks), a_remap=c["a_remap"], c_remap=c["c_remap"], epilogue=G.EPIS.index(epi),
                  out_dtype=ot)
        if c["frames"]:
            A = None
            kw.update(frames=inputs["frames"].cuda(), frame_patch=c["frames"][3])
            if c["frames"][4]:
                kw["frame_norm"] = (H.CLIP_MEAN, H.CLIP_STD)
        else:
            A = _store(inputs["A"], aks, p.get("lda", 0), c["a_remap"], pad)
            kw["lda"] = A.shape[1]
        B = _store(inputs["B"], bks, p.get("ldb", 0), (0, 0, 0), pad)
        kw["ldb"] = B.shape[1]
        if "bias" in inputs:
            kw["bias"] = inputs["bias"].cuda()
        if epi == "qscale":
            kw.update(scale=c["scale"], scale_cols=c["scale_cols"])
        if epi == "scale":
            kw["scale"] = c["scale"]
        aux = None
        if epi == "gelu" and c["aux"]:
            aux = torch.zeros((crows, N + p.get("ldaux", 0)), dtype=ot, device="cuda")
            kw.update(aux=aux, ldaux=aux.shape[1])
        if "resid" in inputs:
            ldr = N + p.get("ldr", 0)
            R = torch.full((crows, ldr), pad, dtype=dt)
            R[crow, :N] = inputs["resid"]
            kw.update(resid=R.cuda(), ldr=ldr)
        out_side = None
        if case.extra["side"]:
            out_side = torch.zeros_like(inputs["resid_side"]).cuda()
            kw.update(resid_side=inputs["resid_side"].cuda(), out_side=out_side, side=c["side"])
        if epi == "patch":
            kw.update(tab1=inputs["tab1"].cuda(), tab2=inputs["tab2"].cuda(), tab_L=c["patch"][1])
        with case_budget(c):
            split = resolve_split(c, case_desc(c))
            kw["split_k"] = split
            if split > 1:
                slabs = torch.zeros((split, M, N), dtype=torch.float32, device="cuda")
                kw["out"] = slabs
            else:
                Cbuf = torch.zeros((crows, N + p.get("ldc", 0)), dtype=ot, device="cuda")
                kw.update(out=Cbuf, ldc=Cbuf.shape[1])
            check_plan(c, H.gemm(A, B, M, N, K, plan_only=True, **kw), split)
            defer = H.DeferredReduce(torch.device("cuda")) if case.extra["colsum"] else None
            if defer is not None:
                kw["colsum_defer"] = defer
            res = H.gemm(A, B, M, N, K, **kw)
        out = {}
        if split > 1:
            out["C"] = H.splitk_reduce(slabs, torch.zeros((M, N), dtype=torch.float32, device="cuda"))
        else:
            out["C"] = Cbuf[crow.cuda(), :N]
        if aux is not None:
            out["aux"] = aux[crow.cuda(), :N]
        if out_side is not None:
            out["out_side"] = out_side
        if defer is not None:
            sg, slot = defer.segs[-1], defer._keep[-1][0]             # the partial rows (of the epilogue, or of the pass over C)
            part = slot.view(torch.float32)[:sg.nrows * sg.stride].view(sg.nrows, sg.stride)[:, :sg.width].clone()
            defer.flush()
            out["colsum"] = res[1]
            out["colsum_rows_sum"] = part.sum(0)
        torch.cuda.synchronize()
        return {k: v.float().cpu() if v.dtype == torch.bfloat16 else v.cpu() for k, v in out.items()}
    return run


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_gemm_carries_a_planted_value_along_its_row_or_column(case, monkeypatch):
    """a plant in row r of A: the whole output row (C, aux, the fp32 side row; every column sum); in row n of B or in bias[n]: the whole
    output column; in resid / a side row / a patch table: the elements that add it.  Every other row (column) keeps its bits."""
    set_case_env(case.extra["case"], monkeypatch)
    n = NF.drive(case, _run(case))
    print(f"{case.name}: {n} required outputs non-finite")


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_gemm_never_reads_its_padding(case, monkeypatch):
    """NaN in the lda / ldb / ldr padding and in the storage rows no remap reaches: every output torch.equal to the run with zeros"""
    set_case_env(case.extra["case"], monkeypatch)
    NF.check_equal(_run(case, NF.NAN)(case.inputs), _run(case, 0.0)(case.inputs), case.name)
