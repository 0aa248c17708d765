"""GPU: xp_attn_pooled_fwd / xp_attn_pooled_bwd (csrc/attention_pooled.hip, four kernels, bf16 and fp32) called through the C ABI with
every output inside a guard buffer, the workspace at exactly xp_attn_pooled_workspace_bytes, row pitches beyond the dense ones, and
the error held PER CLASS against an fp64 softmax over all keys.

What tests/test_attention_pooled_gpu.py cannot see: it draws q as randn and passes it unscaled (scores of standard deviation 8: the
softmax is near one-hot) and measures max|a-b| / max|b| over the whole tensor, so the dk / dv rows of almost every key -- 1e-5 of the
tensor's scale --, the weights the chunk combine gives every chunk but the one with the maximum, the short last chunk and the `valid`
masking of past-the-end lanes are not held at all (tests/test_attention_pooled_class_bounds_cpu.py shows it on the CPU: whole blocks
of dk / dv written as zero, a last key dropped or counted twice all pass that metric).  Here

  a. every case of tests/attn_pooled_emulation.py runs in both dtypes and two regimes (``peaked`` = q as drawn, ``flat`` = q * 0.125,
     an early-training step: the proxy token attends nearly uniformly and every chunk carries weight) and out, dq, dk, dv are held per
     problem (b, h), in the flat regime dk and dv also per (b, h, block of 32 consecutive keys), each class to its own max|ref|;
     ``stats[..., 0] + stats[..., 1]`` to the fp64 logsumexp within min(1e-3, 1 / (8 S)) on every (b, h) -- one key of uniform weight
     moves it by 1 / S; the summed column-sum partial rows to the stored dkv rows at 1e-5; everything finite; second run bit-identical;
  b. a planted key (k[j*] = c q / |q|^2 with c 80 above every other score) at the chunk and workgroup-step boundaries of the DEVICE's
     plan: out == v[j*], dv[j*] == dout bit for bit, log l = 0, every other dv row < 1e-30 -- no tolerance to choose, any dtype;
  c. uniform weights (q = 0): lse = log S, out = mean(v), dk == 0, dv = dout / S.

Per call: ``out``, ``stats``, ``dq`` (pitch H*64 + 8), ``dkv`` (pitch 2*H*64 + 16) and the column-sum partial rows sit in ``Guarded``
buffers and nothing outside the output windows may change; ``kv`` is read at pitch 2*H*64 + 16 with PAD_VALUE in the padding; the
workspace comes from ``GuardedWorkspaces`` with exactly xp_attn_pooled_workspace_bytes, and its bytes at or beyond the device plan's
``workspace_bytes`` of the direction must still hold the poison.

CLASS_BOUNDS -- where the numbers come from.  None is taken from the kernels.  Per (dtype, case, regime) and "quantity/class kind":
``(restatement's error, bound)``, one worst value per class kind.  The restatement is tests/attn_pooled_emulation.py::emulate on the
CPU, on the same seeded inputs:
  * bf16: fp64 arithmetic with the outputs rounded to bf16 and delta from the stored output.  The bound is the existing 1.2e-2 (out) /
    2e-2 (dq, dk, dv), now per class; it is raised to 1.5 x the restatement (rounded up to two digits) only where the restatement
    exceeds bound / 1.5.  That happens where a class's reference all but cancels: dq / dk of a problem whose softmax is one-hot to
    1e-6 (dS = P o (dP - delta) is then the rounding of the stored output and nothing else: B4H16S1100 peaked, 3.0 of the class scale
    in CORRECT bf16 arithmetic), and the dk of a block that holds a single key (B2H2S65 flat).  Those classes say little; the flat
    regime, where no class cancels (<= 4.0e-3 per block, <= 3.7e-3 per problem), and the exact tests b / c carry the weight;
  * fp32: the same formulas evaluated in torch.float32 on the CPU against fp64; the bound is 4 x that error (rounded up to two digits)
    -- 4 and not 1.5 because the summation order of an fp32 sum is the kernel's own.
tests/test_attention_pooled_class_bounds_cpu.py re-derives every entry.  A class whose reference is exactly zero (dq / dk of the
single-key case: softmax of one score has no gradient) must come out exactly zero."""
import math
import os

import pytest
import torch

from tests import attn_pooled_emulation as E
from tests.gpu_util import OUT, report
from tests.guarded import Guarded, GuardedWorkspaces

pytestmark = pytest.mark.gpu

PAD_VALUE = 1000.0                          # input elements outside the operands' extents (tests/test_attention_guarded_gpu.py)
DT = E.DT
WHOLE = {"bf16": (1.2e-2, 2e-2)}            # tests/test_attention_pooled_gpu.py: forward, backward -- here per class
STEP_KEYS = {"bf16": 128, "fp32": 64}       # keys one workgroup step covers: UNROLL * PW * (64 lanes / lanes per key row)
UNIT = {"bf16": 2.0 ** -8, "fp32": 2.0 ** -24}       # one rounding to the storage type, relative

# (dtype, case, regime) -> {"quantity/class kind": (restatement's error on the CPU, bound)}; see the module docstring
CLASS_BOUNDS = {
    ("bf16", "B2H2S1", "peaked"): {"out/problem": (0.00e+00, 1.2e-02), "dq/problem": (0.00e+00, 2.0e-02), "dk/problem": (0.00e+00, 2.0e-02), "dv/problem": (0.00e+00, 2.0e-02)},
    ("bf16", "B2H2S1", "flat"): {"out/problem": (0.00e+00, 1.2e-02), "dq/problem": (0.00e+00, 2.0e-02), "dk/problem": (0.00e+00, 2.0e-02), "dv/problem": (0.00e+00, 2.0e-02), "dk/block": (0.00e+00, 2.0e-02), "dv/block": (0.00e+00, 2.0e-02)},
    ("bf16", "B1H2S9", "peaked"): {"out/problem": (1.98e-03, 1.2e-02), "dq/problem": (6.29e-01, 9.5e-01), "dk/problem": (8.64e-01, 1.3e+00), "dv/problem": (2.43e-03, 2.0e-02)},
    ("bf16", "B1H2S9", "flat"): {"out/problem": (2.70e-03, 1.2e-02), "dq/problem": (2.12e-03, 2.0e-02), "dk/problem": (2.43e-03, 2.0e-02), "dv/problem": (2.45e-03, 2.0e-02), "dk/block": (2.43e-03, 2.0e-02), "dv/block": (2.45e-03, 2.0e-02)},
    ("bf16", "B2H2S33", "peaked"): {"out/problem": (2.58e-03, 1.2e-02), "dq/problem": (1.10e-01, 1.7e-01), "dk/problem": (1.59e-01, 2.4e-01), "dv/problem": (2.57e-03, 2.0e-02)},
    ("bf16", "B2H2S33", "flat"): {"out/problem": (2.42e-03, 1.2e-02), "dq/problem": (2.71e-03, 2.0e-02), "dk/problem": (2.91e-03, 2.0e-02), "dv/problem": (2.11e-03, 2.0e-02), "dk/block": (4.01e-03, 2.0e-02), "dv/block": (2.37e-03, 2.0e-02)},
    ("bf16", "B2H2S65", "peaked"): {"out/problem": (2.45e-03, 1.2e-02), "dq/problem": (8.51e-03, 2.0e-02), "dk/problem": (1.22e-02, 2.0e-02), "dv/problem": (2.94e-03, 2.0e-02)},
    ("bf16", "B2H2S65", "flat"): {"out/problem": (3.29e-03, 1.2e-02), "dq/problem": (3.11e-03, 2.0e-02), "dk/problem": (2.41e-03, 2.0e-02), "dv/problem": (2.94e-03, 2.0e-02), "dk/block": (1.36e-01, 2.1e-01), "dv/block": (3.37e-03, 2.0e-02)},
    ("bf16", "B1H1S129", "peaked"): {"out/problem": (2.85e-03, 1.2e-02), "dq/problem": (3.27e-03, 2.0e-02), "dk/problem": (2.25e-03, 2.0e-02), "dv/problem": (2.91e-03, 2.0e-02)},
    ("bf16", "B1H1S129", "flat"): {"out/problem": (2.73e-03, 1.2e-02), "dq/problem": (1.67e-03, 2.0e-02), "dk/problem": (2.63e-03, 2.0e-02), "dv/problem": (2.13e-03, 2.0e-02), "dk/block": (2.63e-03, 2.0e-02), "dv/block": (3.09e-03, 2.0e-02)},
    ("bf16", "B3H5S201", "peaked"): {"out/problem": (3.34e-03, 1.2e-02), "dq/problem": (1.64e-01, 2.5e-01), "dk/problem": (1.76e-01, 2.7e-01), "dv/problem": (3.07e-03, 2.0e-02)},
    ("bf16", "B3H5S201", "flat"): {"out/problem": (3.61e-03, 1.2e-02), "dq/problem": (2.97e-03, 2.0e-02), "dk/problem": (3.01e-03, 2.0e-02), "dv/problem": (3.60e-03, 2.0e-02), "dk/block": (3.54e-03, 2.0e-02), "dv/block": (3.80e-03, 2.0e-02)},
    ("bf16", "B2H2S904", "peaked"): {"out/problem": (2.62e-03, 1.2e-02), "dq/problem": (3.87e-02, 5.9e-02), "dk/problem": (5.06e-02, 7.6e-02), "dv/problem": (2.29e-03, 2.0e-02)},
    ("bf16", "B2H2S904", "flat"): {"out/problem": (2.81e-03, 1.2e-02), "dq/problem": (2.49e-03, 2.0e-02), "dk/problem": (2.88e-03, 2.0e-02), "dv/problem": (3.55e-03, 2.0e-02), "dk/block": (3.46e-03, 2.0e-02), "dv/block": (3.60e-03, 2.0e-02)},
    ("bf16", "B1H2S4096", "peaked"): {"out/problem": (2.88e-03, 1.2e-02), "dq/problem": (2.43e-03, 2.0e-02), "dk/problem": (2.12e-03, 2.0e-02), "dv/problem": (2.04e-03, 2.0e-02)},
    ("bf16", "B1H2S4096", "flat"): {"out/problem": (2.10e-03, 1.2e-02), "dq/problem": (2.01e-03, 2.0e-02), "dk/problem": (1.60e-03, 2.0e-02), "dv/problem": (3.06e-03, 2.0e-02), "dk/block": (3.62e-03, 2.0e-02), "dv/block": (3.88e-03, 2.0e-02)},
    ("bf16", "B4H16S1100", "peaked"): {"out/problem": (3.26e-03, 1.2e-02), "dq/problem": (3.00e+00, 4.6e+00), "dk/problem": (3.13e+00, 4.7e+00), "dv/problem": (3.69e-03, 2.0e-02)},
    ("bf16", "B4H16S1100", "flat"): {"out/problem": (3.51e-03, 1.2e-02), "dq/problem": (3.68e-03, 2.0e-02), "dk/problem": (3.64e-03, 2.0e-02), "dv/problem": (3.50e-03, 2.0e-02), "dk/block": (3.87e-03, 2.0e-02), "dv/block": (3.89e-03, 2.0e-02)},
    ("fp32", "B2H2S1", "peaked"): {"out/problem": (0.00e+00, 0.0e+00), "dq/problem": (0.00e+00, 0.0e+00), "dk/problem": (0.00e+00, 0.0e+00), "dv/problem": (0.00e+00, 0.0e+00)},
    ("fp32", "B2H2S1", "flat"): {"out/problem": (0.00e+00, 0.0e+00), "dq/problem": (0.00e+00, 0.0e+00), "dk/problem": (0.00e+00, 0.0e+00), "dv/problem": (0.00e+00, 0.0e+00), "dk/block": (0.00e+00, 0.0e+00), "dv/block": (0.00e+00, 0.0e+00)},
    ("fp32", "B1H2S9", "peaked"): {"out/problem": (7.26e-08, 3.0e-07), "dq/problem": (5.29e-05, 2.2e-04), "dk/problem": (7.31e-05, 3.0e-04), "dv/problem": (8.75e-08, 3.6e-07)},
    ("fp32", "B1H2S9", "flat"): {"out/problem": (1.42e-07, 5.7e-07), "dq/problem": (1.75e-07, 7.1e-07), "dk/problem": (1.34e-07, 5.4e-07), "dv/problem": (8.78e-08, 3.6e-07), "dk/block": (1.34e-07, 5.4e-07), "dv/block": (8.78e-08, 3.6e-07)},
    ("fp32", "B2H2S33", "peaked"): {"out/problem": (6.78e-07, 2.8e-06), "dq/problem": (1.93e-04, 7.8e-04), "dk/problem": (2.85e-04, 1.2e-03), "dv/problem": (5.37e-07, 2.2e-06)},
    ("fp32", "B2H2S33", "flat"): {"out/problem": (2.42e-07, 9.7e-07), "dq/problem": (2.46e-07, 9.9e-07), "dk/problem": (2.54e-07, 1.1e-06), "dv/problem": (2.68e-07, 1.1e-06), "dk/block": (3.45e-07, 1.4e-06), "dv/block": (5.82e-07, 2.4e-06)},
    ("fp32", "B2H2S65", "peaked"): {"out/problem": (4.90e-07, 2.0e-06), "dq/problem": (2.47e-06, 9.9e-06), "dk/problem": (2.72e-06, 1.1e-05), "dv/problem": (3.23e-07, 1.3e-06)},
    ("fp32", "B2H2S65", "flat"): {"out/problem": (2.03e-07, 8.2e-07), "dq/problem": (2.48e-07, 1.0e-06), "dk/problem": (2.58e-07, 1.1e-06), "dv/problem": (2.76e-07, 1.2e-06), "dk/block": (2.10e-05, 8.4e-05), "dv/block": (5.46e-07, 2.2e-06)},
    ("fp32", "B1H1S129", "peaked"): {"out/problem": (7.41e-07, 3.0e-06), "dq/problem": (2.22e-07, 8.9e-07), "dk/problem": (2.16e-07, 8.7e-07), "dv/problem": (5.22e-07, 2.1e-06)},
    ("fp32", "B1H1S129", "flat"): {"out/problem": (1.91e-07, 7.7e-07), "dq/problem": (2.13e-07, 8.6e-07), "dk/problem": (9.26e-08, 3.8e-07), "dv/problem": (2.05e-07, 8.3e-07), "dk/block": (3.13e-07, 1.3e-06), "dv/block": (2.63e-07, 1.1e-06)},
    ("fp32", "B3H5S201", "peaked"): {"out/problem": (1.99e-06, 8.0e-06), "dq/problem": (3.48e-05, 1.4e-04), "dk/problem": (3.65e-05, 1.5e-04), "dv/problem": (1.29e-06, 5.2e-06)},
    ("fp32", "B3H5S201", "flat"): {"out/problem": (4.03e-07, 1.7e-06), "dq/problem": (5.93e-07, 2.4e-06), "dk/problem": (4.84e-07, 2.0e-06), "dv/problem": (5.98e-07, 2.4e-06), "dk/block": (6.77e-07, 2.8e-06), "dv/block": (5.98e-07, 2.4e-06)},
    ("fp32", "B2H2S904", "peaked"): {"out/problem": (1.72e-06, 6.9e-06), "dq/problem": (1.64e-05, 6.6e-05), "dk/problem": (2.12e-05, 8.5e-05), "dv/problem": (1.91e-06, 7.7e-06)},
    ("fp32", "B2H2S904", "flat"): {"out/problem": (6.25e-07, 2.5e-06), "dq/problem": (5.99e-07, 2.4e-06), "dk/problem": (3.76e-07, 1.6e-06), "dv/problem": (5.61e-07, 2.3e-06), "dk/block": (7.58e-07, 3.1e-06), "dv/block": (6.47e-07, 2.6e-06)},
    ("fp32", "B1H2S4096", "peaked"): {"out/problem": (1.94e-06, 7.8e-06), "dq/problem": (1.27e-06, 5.1e-06), "dk/problem": (2.04e-06, 8.2e-06), "dv/problem": (1.92e-06, 7.7e-06)},
    ("fp32", "B1H2S4096", "flat"): {"out/problem": (1.05e-06, 4.2e-06), "dq/problem": (1.54e-06, 6.2e-06), "dk/problem": (2.85e-07, 1.2e-06), "dv/problem": (9.57e-07, 3.9e-06), "dk/block": (9.42e-07, 3.8e-06), "dv/block": (9.97e-07, 4.0e-06)},
    ("fp32", "B4H16S1100", "peaked"): {"out/problem": (3.83e-06, 1.6e-05), "dq/problem": (4.32e-02, 1.8e-01), "dk/problem": (5.05e-02, 2.1e-01), "dv/problem": (3.01e-06, 1.3e-05)},
    ("fp32", "B4H16S1100", "flat"): {"out/problem": (1.15e-06, 4.7e-06), "dq/problem": (1.36e-06, 5.5e-06), "dk/problem": (7.88e-07, 3.2e-06), "dv/problem": (8.46e-07, 3.4e-06), "dk/block": (1.11e-06, 4.5e-06), "dv/block": (1.08e-06, 4.4e-06)},
}


def _log(line):
    print(line)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "parity_log.txt"), "a") as f:
        f.write(line + "\n")


def _held(tag, e, bound):
    """a `report`-style line; True when the figure is inside its bound"""
    ok = e <= bound
    _log(f"{tag}: err={e:.3e} bound={bound:.1e} {'OK' if ok else 'FAIL'}")
    return ok


def _padded_input(t, ld):
    """[rows, cols] -> the same values at row pitch ld, PAD_VALUE in the padding"""
    rows, cols = t.shape
    store = torch.full((rows, ld), PAD_VALUE, dtype=t.dtype, device="cuda")
    store[:, :cols] = t.cuda()
    return store


def _call(tag, B, H, S, q_c, kv_c, dout_c):
    """one guarded forward + backward through the C ABI on CPU operands q [B, H*64], kv [B*S, 2*H*64], dout [B, H*64]; every guard
    and window is checked.  -> CPU tensors out, dq [B, H, 64], dk, dv [B, S, H, 64], stats [B, H, 2], colsum, colsum_of_stored"""
    from xpretrain_amd import _lib as L
    from xpretrain_amd import hip_ops as Hh
    dtype = q_c.dtype
    D = H * 64
    ldkv, lddq, lddkv = 2 * D + 16, D + 8, 2 * D + 16
    q, dout, kv = q_c.cuda().contiguous(), dout_c.cuda().contiguous(), _padded_input(kv_c, ldkv)
    q0, dout0, kv0 = q.clone(), dout.clone(), kv.clone()
    lib, dtc, dev = L.lib(), Hh._dt(q), q.device
    out_g, stats_g = Guarded(B, D, dtype), Guarded(B * H, 2, torch.float32)
    dq_g, dkv_g = Guarded(B, lddq, dtype), Guarded(B * S, lddkv, dtype)
    nrows = int(lib.xp_attn_pooled_colsum_rows(B, H, S, dtc))
    plans = [Hh.attn_pooled_plan(B, S, H, dtype=dtype, backward=b) for b in (False, True)]
    assert nrows == B * plans[1]["chunks"] > 0
    cs_g = Guarded(nrows, 2 * D, torch.float32)
    ws_bytes = int(lib.xp_attn_pooled_workspace_bytes(B, H, S, dtc))
    assert 0 < max(p["workspace_bytes"] for p in plans) <= ws_bytes
    with GuardedWorkspaces() as gw:
        ws_f = Hh.workspace(ws_bytes, dev, "attn_pooled_fwd")
        L.check(lib.xp_attn_pooled_fwd(Hh._p(q), Hh._p(kv), ldkv, Hh._p(out_g.mat), Hh._p(stats_g.mat), B, H, S, dtc, Hh._p(ws_f),
                                       ws_f.numel(), Hh._stream()), "xp_attn_pooled_fwd")
        ws_b = Hh.workspace(ws_bytes, dev, "attn_pooled_bwd")
        L.check(lib.xp_attn_pooled_bwd(Hh._p(q), Hh._p(kv), ldkv, Hh._p(out_g.mat), Hh._p(dout), Hh._p(stats_g.mat), Hh._p(dq_g.mat), lddq,
                                       Hh._p(dkv_g.mat), lddkv, E.Q_SCALE, B, H, S, dtc, Hh._p(ws_b), ws_b.numel(), Hh._p(cs_g.mat),
                                       Hh._stream()), "xp_attn_pooled_bwd")
        defer = Hh.DeferredReduce(dev)
        cs = torch.empty(2 * D, dtype=torch.float32, device=dev)
        defer.add(cs_g.mat, 0, cs, nrows, 2 * D, 2 * D)
        defer.flush()
        assert [r[:2] for r in gw.records[:2]] == [("attn_pooled_fwd", ws_bytes), ("attn_pooled_bwd", ws_bytes)]
        assert ws_f.numel() == ws_bytes == ws_b.numel()
    gw.check()
    gw.check_body_beyond("attn_pooled_fwd", plans[0]["workspace_bytes"])
    gw.check_body_beyond("attn_pooled_bwd", plans[1]["workspace_bytes"])
    out_g.check(tag + " out", B, D)
    stats_g.check(tag + " stats", B * H, 2)
    dq_g.check(tag + " dq", B, D)
    dkv_g.check(tag + " dkv", B * S, 2 * D)
    cs_g.check(tag + " colsum partial rows", nrows, 2 * D)
    assert torch.equal(q, q0) and torch.equal(dout, dout0) and torch.equal(kv, kv0), tag + ": an input changed"
    dk, dv = dkv_g.mat[:, :2 * D].reshape(B, S, 2, H, 64).unbind(2)
    got = {"out": out_g.mat.view(B, H, 64), "dq": dq_g.mat[:, :D].reshape(B, H, 64), "dk": dk, "dv": dv,
           "stats": stats_g.mat.view(B, H, 2), "colsum": cs, "colsum_of_stored": dkv_g.mat[:, :2 * D].double().sum(0)}
    got = {n: t.cpu().contiguous() for n, t in got.items()}
    assert all(torch.isfinite(t.float()).all() for t in got.values()), tag + ": not finite"
    return got


def _lse(got):
    return got["stats"].double().sum(-1)


# ------------------------------------------------------------------------------------------------ a. per class against fp64
@pytest.mark.parametrize("regime", list(E.REGIMES))
@pytest.mark.parametrize("case", list(E.CASES))
@pytest.mark.parametrize("dt", list(DT))
def test_pooled_attention_per_class(dt, case, regime):
    B, H, S = E.CASES[case]
    ops = E.inputs(case, regime, DT[dt])
    tag = f"attn_pooled guarded {dt} {case} {regime}"
    got = _call(tag, B, H, S, *ops)
    ref = E.case_reference(case, regime, DT[dt])
    bounds = CLASS_BOUNDS[(dt, case, regime)]
    errs = E.class_errors(got, ref, regime)
    assert set(errs) == set(bounds)
    fails = [key for key, (restated, bound) in bounds.items()
             if not _held(f"{tag} {key} (restatement {restated:.2e})", errs[key], bound)]
    if not _held(f"{tag} lse", (_lse(got) - ref["lse"]).abs().max().item(), E.lse_bound(S)):
        fails.append("lse")
    if report(f"{tag} colsum vs stored", got["colsum"], got["colsum_of_stored"], 1e-5, scale_floor=1e-3) > 1e-5:
        fails.append("colsum")
    again = _call(tag + " (second run)", B, H, S, *ops)
    for n in got:
        assert torch.equal(got[n], again[n]), f"{tag}: two runs differ in {n}"
    assert not fails, f"{tag}: beyond their bounds: {fails}"


# ------------------------------------------------------------------------------------------------ b. planted key
def _planted_positions(dt, plan, S):
    ck, chunks = plan["chunk_keys"], plan["chunks"]
    assert chunks >= 3 and ck % E.BLOCK == 0, plan
    full = ck // STEP_KEYS[dt] * STEP_KEYS[dt]              # the keys of chunk 1 that whole workgroup steps cover (none: the chunk's own)
    pos = {"key 0": 0, "last key of chunk 0": ck - 1, "first key of chunk 1": ck, "first key of the last chunk": (chunks - 1) * ck,
           "key S - 1": S - 1, "last key of a full workgroup step in chunk 1": ck + (full or ck) - 1}
    assert all(0 <= j < S for j in pos.values())
    return pos


@pytest.mark.parametrize("case", ["B3H5S201", "B2H2S904", "B4H16S1100"])
@pytest.mark.parametrize("dt", list(DT))
def test_planted_key_is_found_exactly(dt, case):
    """k[j*] = c q / |q|^2 with c 80 above the largest other score: p[j*] = 1 and every other p <= e^-79 < 1e-34 in fp64, fp32 and
    bf16 alike, so out == v[j*], dv[j*] == dout, log l == 0 and the row maximum is the planted score.  An index slip at a chunk or
    workgroup-step boundary reads another key; a doubled last key gives log l = log 2."""
    from xpretrain_amd import hip_ops as Hh
    B, H, S = E.CASES[case]
    plan = Hh.attn_pooled_plan(B, S, H, dtype=DT[dt])
    fails = []
    for regime in E.REGIMES:
        q_c, kv_c, dout_c = E.inputs(case, regime, DT[dt])
        q, k, v, _ = E.split(q_c, kv_c, dout_c, B, H, S)
        s = torch.einsum("bhd,bshd->bhs", q, k)
        for name, j in _planted_positions(dt, plan, S).items():
            others = s.clone()
            others[:, :, j] = -math.inf
            c = others.amax(-1) + 80.0                                           # [B, H]
            kv_p = kv_c.clone().view(B, S, 2, H, 64)
            kv_p[:, j, 0] = (c[..., None] * q / (q * q).sum(-1, keepdim=True)).to(DT[dt])
            planted = (q * kv_p[:, j, 0].double()).sum(-1)                       # the score of the planted key as stored, fp64
            assert (planted - others.amax(-1)).min() >= 79.0                     # (the inputs' own condition, not the kernel's)
            tag = f"attn_pooled planted {dt} {case} {regime} {name} (j* = {j})"
            got = _call(tag, B, H, S, q_c, kv_p.view(B * S, -1), dout_c)
            dv_other = got["dv"].clone()
            dv_other[:, j] = 0
            # the row maximum: an fp32 sum of 64 products of one sign, in any order, is within 64 roundings of the sum
            e_max = ((got["stats"][..., 0].double() - planted).abs() / ((q * kv_p[:, j, 0].double()).abs().sum(-1) * 64 * 2.0 ** -24)).max().item()
            checks = {"out == v[j*]": torch.equal(got["out"], kv_p[:, j, 1].to(DT[dt])), "dv[j*] == dout": torch.equal(got["dv"][:, j], dout_c.view(B, H, 64)),
                      "log l == 0": got["stats"][..., 1].abs().max().item() <= 1e-6, "row max": e_max <= 1.0,
                      "other dv rows < 1e-30": dv_other.float().abs().max().item() < 1e-30}
            _log(f"{tag}: log l {got['stats'][..., 1].abs().max().item():.1e}, row max off by {e_max:.2f} of its bound, other dv rows "
                 f"{dv_other.float().abs().max().item():.1e} -- {'OK' if all(checks.values()) else 'FAIL'}")
            fails += [f"{regime} {name}: {n}" for n, ok in checks.items() if not ok]
    assert not fails, f"planted key {dt} {case} (device plan {plan['chunks']} x {plan['chunk_keys']}): {fails}"


# ------------------------------------------------------------------------------------------------ c. uniform weights
@pytest.mark.parametrize("case", list(E.CASES))
@pytest.mark.parametrize("dt", list(DT))
def test_uniform_weights(dt, case):
    """q = 0: every score is 0, so lse = log S, out = mean(v), dS = (dO . v_j - dO . out) / S, dk = dS q = 0 exactly, and
    dv = dout / S within one rounding of the storage type in bf16; in fp32 within that rounding plus the documented errors of the
    operations between log l and p (attn_pooled_emulation.uniform_dv_bound: (4 log S + 3) 2^-24; measured on MI355X 0 .. 11.4
    roundings, largest at S = 904 where the bound is 30).  With one key out == v and dv == dout bit for bit, and dS -- zero by
    cancellation, not by a zero factor -- leaves in dq and dk at most 4 x what the restatement leaves on the same inputs."""
    B, H, S = E.CASES[case]
    _, kv_c, dout_c = E.inputs(case, "flat", DT[dt])
    q_c = torch.zeros(B, H * 64, dtype=DT[dt])
    tag = f"attn_pooled uniform {dt} {case}"
    got = _call(tag, B, H, S, q_c, kv_c, dout_c)
    q, k, v, dout = E.split(q_c, kv_c, dout_c, B, H, S)
    fails = []
    if not _held(f"{tag} lse - log S", (_lse(got) - math.log(S)).abs().max().item(), E.lse_bound(S)):
        fails.append("lse")
    mean = v.mean(1)                                                             # [B, H, 64]
    e_out = ((got["out"].double() - mean).abs().amax(-1) / mean.abs().amax(-1)).max().item()
    if not _held(f"{tag} out vs mean(v), per problem", e_out, CLASS_BOUNDS[(dt, case, "flat")]["out/problem"][1]):
        fails.append("out")
    if got["dk"].float().abs().max().item() != 0:
        fails.append("dk != 0")
    want = dout[:, None] / S
    e_dv = ((got["dv"].double() - want).abs() / want.abs().clamp_min(1e-300)).max().item()
    _log(f"{tag} dv vs dout / S: {e_dv / UNIT[dt]:.2f} roundings of the storage type")
    if not _held(f"{tag} dv vs dout / S, per element", e_dv, E.uniform_dv_bound(dt, S)):
        fails.append("dv")
    if S == 1:
        emu = E.emulate(q, k, v, dout) if dt == "bf16" else E.emulate(q, k, v, dout, work=torch.float32, store=None)
        if not (torch.equal(got["out"], kv_c.view(B, S, 2, H, 64)[:, 0, 1]) and torch.equal(got["dv"][:, 0], dout_c.view(B, H, 64))):
            fails.append("out == v, dv == dout")
        for n in ("dq", "dk"):
            if not _held(f"{tag} |{n}|", got[n].float().abs().max().item(), 4 * emu[n].abs().max().item()):
                fails.append(n)
    assert not fails, f"{tag}: {fails}"
