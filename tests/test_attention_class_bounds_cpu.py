"""CPU: where the per-row-class bounds of tests/test_attention_guarded_gpu.py come from.  tests/attn_emulation.py restates the
attention kernels' arithmetic on the CPU (fp64 with the bf16 storage roundings; the same formulas in float32) on the very inputs
the GPU test uses, and every class error of that restatement against the fp64 oracle cores must sit well inside the bound the GPU
test holds the kernels to: bound / 1.5 in bf16; in fp32 the bound IS 4 x the recorded float32 error, and the error measured here may
exceed the recorded one by at most 1.5 x plus one float32 ulp of the class scale (the summation order of a float32 matrix product
differs between CPUs and thread counts).
No GPU is involved: a bound in that table cannot have been fitted to the kernels."""
import pytest
import torch

from tests import attn_emulation as E
from tests.test_attention_guarded_gpu import CLASS_BOUNDS, DT, RUNS, WHOLE


def test_the_table_covers_every_run():
    need = {(dt, case, regime) for dt, case, _ in RUNS for regime in E.REGIMES}
    assert need <= set(CLASS_BOUNDS)
    assert all(case in E.CASES for _, case, _ in CLASS_BOUNDS)


@pytest.mark.parametrize("dt,case,regime", list(CLASS_BOUNDS), ids=["-".join(k) for k in CLASS_BOUNDS])
def test_restatement_is_inside_the_class_bounds(dt, case, regime):
    errs = E.restated_class_errors(case, regime, DT[dt])
    table = CLASS_BOUNDS[(dt, case, regime)]
    assert {f"{n}/{c}" for n, c in errs} == set(table)
    for (n, c), e in errs.items():
        recorded, bound = table[f"{n}/{c}"]
        print(f"{dt} {case} {regime} {n}/{c}: restatement {e:.2e} (recorded {recorded:.2e}) bound {bound:.1e}")
        if dt == "bf16":
            base = WHOLE["bf16"][0 if n == "out" else 1]
            assert e <= bound / 1.5, (n, c, e, bound)
            # the bound is the existing whole-tensor one, or -- only where the restatement needs it -- 1.5 x the recorded restatement
            assert bound == base or (recorded > base / 1.5 and bound <= 1.5 * recorded * 1.05), (n, c, recorded, bound)
        else:
            assert 4 * recorded <= bound <= 4 * recorded * 1.1 + 1e-12, (n, c, recorded, bound)
            assert e <= 1.5 * recorded + (2.0 ** -24 if recorded else 0.0), (n, c, e, recorded)      # (+ one fp32 ulp of the class scale)


def test_restatement_equals_the_reference_without_rounding():
    """the restatement with no storage rounding in fp64 IS the reference: the class errors above are rounding, not a formula slip"""
    for case in ("proxy4x3x70-B1H3", "causal77ragged-B2H2", "causal16allpad-B2H2"):
        size, B, H, S, mode = E.CASES[case]
        qkv, dout, pad = E.inputs(case, "peaked", torch.bfloat16)
        q, k, v = E.split_heads(qkv, B, S, H)
        do = dout.view(B, S, H, 64).double().transpose(1, 2)
        ref, emu = E.reference(q, k, v, do, size, pad), E.emulate(q, k, v, do, size, pad, store=None)
        keep = torch.ones(B, S, dtype=torch.bool) if pad is None else pad.bool()
        for n in ("out", "dq", "dk", "dv"):
            assert E.class_error(emu[n], ref[n], torch.ones(B, S, dtype=torch.bool)) <= 1e-12, (case, n)
        assert (emu["lse"] - ref["lse"]).transpose(1, 2)[keep].abs().max() <= 1e-12, case
