"""CPU: the LayerNorm definition of tests/layernorm_ref.py is stated twice (explicit formulas == fp64 torch layer_norm + autograd),
the float32 emulation of the kernels passes every gate in every case of the shared table, and each of fourteen wrong kernels -- the
emulation with one change -- fails a gate in a named case.  The last list is the proof that tests/test_layernorm_contract_gpu.py
would notice: a wrong kernel that passes means a case or a gate is missing."""
import functools
import math

import pytest
import torch

from tests import layernorm_ref as R

CPU_CASES = [c for c in R.FWD_CASES + R.BWD_CASES if c.rows < R.BIG or c.cols == 8]          # the 16395-row cases at cols = 8 only


# ------------------------------------------------------------------------------------------------- the definition, stated twice
@pytest.mark.parametrize("cols", [8, 260, 1024])
def test_definition_agrees_with_fp64_layer_norm_and_autograd(cols):
    rows = 36
    g = torch.Generator().manual_seed(cols)
    x = R.family_rows(rows, cols, g).double()
    fam = R.family_of(rows)
    const = torch.tensor([f == "const" for f in fam])
    gamma, beta = (1 + 0.3 * torch.randn(cols, generator=g)).double(), (0.1 * torch.randn(cols, generator=g)).double()
    dy, dres = torch.randn(rows, cols, generator=g).double(), torch.randn(rows, cols, generator=g).double()
    f = R.ref_fwd(x, gamma, beta, 1e-5)
    eps = float(torch.tensor(1e-5, dtype=torch.float32))
    xa, ga, ba = x.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    ya = torch.nn.functional.layer_norm(xa, (cols,), ga, ba, eps)
    ya.backward(dy)
    # autograd runs with its own exact statistics: feed the fp64 mean / rstd to the formulas
    b = R.ref_bwd(dy, x, gamma, f["mean"], f["rstd"], dres)

    def rel(a, ref, rows_=slice(None)):
        return ((a - ref)[rows_].abs().max() / ref[rows_].abs().max().clamp_min(1e-300)).item()
    nc = ~const
    assert rel(f["y"], ya.detach(), nc) <= 1e-12
    assert rel(b["dx"], xa.grad + dres, nc) <= 1e-12
    # column sums over the non-constant rows (the constant rows add exact zeros to dgamma)
    assert rel(b["dgamma"], ga.grad) <= 1e-12 and rel(b["dbeta"], ba.grad) <= 1e-12
    assert rel(b["colsum_dx"], (xa.grad + dres).sum(0)) <= 1e-9           # 316 x cancellation in the constant rows' dx
    assert rel(b["colsum_dres"], dres.sum(0)) <= 1e-12
    # constant rows against the closed form: xh = 0, rstd = 1 / sqrt(eps), y = beta, dx = rstd * (gy - mean(gy)) + dres
    r0 = 1.0 / math.sqrt(eps)
    assert torch.equal(f["mean"][const], torch.full((int(const.sum()),), 0.5, dtype=torch.float64))
    assert ((f["rstd"][const] - r0).abs() <= 1e-12 * r0).all()
    assert torch.equal(f["y"][const], beta.expand(int(const.sum()), -1))
    gy = dy[const] * gamma
    closed = r0 * (gy - gy.mean(1, keepdim=True)) + dres[const]
    assert rel(b["dx"][const], closed) <= 1e-12
    assert rel((xa.grad + dres)[const], closed) <= 1e-9                   # autograd is fine there too


# ------------------------------------------------------------------------------------------------- the emulation passes every gate
def _run(case, mutant=None, alias=False):
    inp = R.build(case)
    if case.kind == "fwd":
        return R.judge_fwd(case, inp, R.emu_fwd(case, inp, mutant))
    f = R.emu_fwd(case, inp)                     # the backward's mean / rstd are inputs: from the unmutated forward
    return R.judge_bwd(case, inp, f["mean"], f["rstd"], R.emu_bwd(case, inp, f["mean"], f["rstd"], mutant, alias))


@functools.lru_cache(maxsize=None)
def _verdict(case):
    return _run(case, alias=case.kind == "bwd" and case.dres)


@pytest.mark.parametrize("case", CPU_CASES, ids=lambda c: c.id)
def test_emulation_passes_every_gate(case):
    v = _verdict(case)
    print("\n".join(v.lines()))
    v.assert_ok()


# the emulation's worst multiple of u per kernel group and metric over CPU_CASES, before any allowance: the figures in the docstring of
# tests/layernorm_ref.py.  The emulation is plain float32 arithmetic on seeded inputs, so they are reproducible; a change of the case
# table, the families or the emulation that moves one has to move the docstring with it.
EMULATION_WORST = {
    ("ln_fwd_h_kernel", "y"): 1.34, ("ln_fwd_h_kernel", "y_side"): 2.03, ("ln_fwd_h_kernel", "mean"): 2.03, ("ln_fwd_h_kernel", "rstd"): 2.74,
    ("ln_fwd_kernel<bf16_t>", "y"): 0.857, ("ln_fwd_kernel<bf16_t>", "y_side"): 1.94, ("ln_fwd_kernel<bf16_t>", "mean"): 1.95,
    ("ln_fwd_kernel<bf16_t>", "rstd"): 2.27,
    ("ln_fwd_kernel<float>", "y"): 3.44, ("ln_fwd_kernel<float>", "y_side"): 3.44, ("ln_fwd_kernel<float>", "mean"): 2.9,
    ("ln_fwd_kernel<float>", "rstd"): 3.05,
    ("ln_bwd_kernel", "dx"): 2.98, ("ln_bwd_kernel", "dgamma"): 2.5, ("ln_bwd_kernel", "dbeta"): 1.26, ("ln_bwd_kernel", "colsum_dres"): 1.16,
    ("ln_bwd_kernel", "colsum_dx"): 990.0,                       # before the dx-gate allowance (0 after it), gate 9 u: one row
    ("ln_bwd_kernel", "colsum_dx vs stored dx"): 1.87,           # fp32 only: the summation alone, gate 45 u
}


def test_emulation_worst_multiples_are_the_documented_ones():
    worst = {}
    for case in CPU_CASES:
        _verdict(case).worst_by_group(worst)
    for k in sorted(worst):
        print("WORST", k, "%.3g u of %.4g u in %s" % worst[k])
    assert set(worst) == set(EMULATION_WORST), sorted(set(worst) ^ set(EMULATION_WORST))
    for k, (m, _, cid) in worst.items():
        assert abs(m - EMULATION_WORST[k]) <= 0.01 * EMULATION_WORST[k] + 5e-3, f"{k}: {m:.4g} u in {cid}, documented {EMULATION_WORST[k]}"


def test_case_table_names_every_instantiation():
    names = {c.kernel for c in R.FWD_CASES + R.BWD_CASES}
    fwd = {f"ln_fwd_h_kernel<{j}>" for j in (1, 2, 3, 4)} | {"ln_fwd_kernel<bf16_t>", "ln_fwd_kernel<float>"}
    want = fwd | {f"ln_bwd_kernel<{t},{j},{d}>" for t in ("bf16_t", "float") for j in (1, 2, 3, 4) for d in (0, 1, 2)}
    assert want <= names, sorted(want - names)
    # the three forward kernels (half-wave, bf16 wave, fp32 wave) run with side rows too -- nine forward variants in all -- each
    # with both side geometries, and every such case id carries the side variant
    for rows, side in R.SIDES:
        reached = {c.kernel for c in R.FWD_CASES if c.side == side and c.rows == rows}
        assert fwd <= reached, (side, sorted(fwd - reached))
    assert all(f"-side{'_'.join(map(str, c.side))}" in c.id for c in R.FWD_CASES + R.BWD_CASES if c.side)
    # ... and beyond the grid, where one wave serves side rows and ordinary rows in turn
    assert {c.kernel for c in R.FWD_CASES if c.side and c.rows == R.BIG} == {"ln_fwd_kernel<bf16_t>", "ln_fwd_kernel<float>"}
    assert {c.kernel for c in R.BWD_CASES if c.side} >= {"ln_bwd_kernel<bf16_t,4,2>", "ln_bwd_kernel<float,2,2>"}
    assert R.CASES["ln_fwd_kernel<bf16_t>-37x256-ldx+4"].kernel == R.CASES["ln_fwd_kernel<bf16_t>-37x256-xoff4"].kernel


# ------------------------------------------------------------------------------------------------- every wrong kernel fails
@pytest.mark.parametrize("mutant,where", list(R.MUTANTS.items()) + list(R.MUTANTS_ALSO.items()), ids=lambda v: v if isinstance(v, str) else v[1])
def test_wrong_kernel_fails_a_gate(mutant, where):
    kind, cid = where
    case = R.CASES[cid]
    assert case.kind == kind
    good = _run(case, alias=True)
    good.assert_ok()
    bad = _run(case, mutant, alias=True)
    print("\n".join(bad.lines()))
    assert bad.failed, f"the wrong kernel {mutant!r} passes every gate of {cid}"
