"""CPU: the one table of a layer backward's GEMMs (csrc/layer.hip, read through xp_debug_layer_bwd_gemms).  The workspace queries,
which size their split-K slabs and partial rows from it, answer what tests/golden/layer_gemm_table_workspace_bytes.json records;
for the step's towers the table is the ``step-*`` rows of tests/gemm_cases.py; and the host half of functional._dx3_support, which
reads it, builds the lists tests/test_tile_lists_cpu.py::CASES names.

The fixture was written by ``python tests/test_layer_gemm_table_cpu.py --record`` with the library built from the commit BEFORE the
table existed (2c8ab01, where every carver re-described its GEMMs by hand): the sizes are part of the C ABI and must not move."""
import ctypes as C
import json
import os
import sys

import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import gemm_cases as G  # noqa: E402
from tests.test_layer_boundary_cpu import QUERIES, _dims  # noqa: E402
from xpretrain_amd import _lib as L  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layer_gemm_table_workspace_bytes.json")
V, T = G.VIDEO, G.TEXT
# name: (B, S, D, Dff, heads, size | None); a video shape is also the pooled case
SHAPES = {"step_video": (G.BATCH, V["S"], V["D"], V["Dff"], 12, (V["Mp"], V["T"], V["Lp"])),
          "step_text": (G.BATCH, T["rows"] // G.BATCH, T["D"], T["Dff"], 8, None),
          "listed_8240": (2, 4120, 768, 3072, 12, (4, 21, 196)),          # the layer of tests/test_tile_lists_gpu.py
          "small_video": (4, 10, 128, 512, 2, (2, 2, 4)),                  # the 128-wide family: 40 rows ...
          "small_text": (3, 50, 256, 1024, 4, None)}                       # ... and 150
DTYPES = ((L.XP_BF16, "bf16"), (L.XP_F32, "fp32"))
ACTS = ((L.ACT_QUICK_GELU, "quick_gelu"), (L.ACT_GELU, "gelu"))
BUDGETS = (256, 128)


class _budget:
    def __init__(self, cus):
        self.cus = cus

    def __enter__(self):
        self.prev = L.lib().xp_get_cu_budget()
        L.check(L.lib().xp_set_cu_budget(self.cus), "xp_set_cu_budget")

    def __exit__(self, *exc):
        L.lib().xp_set_cu_budget(self.prev)


def _sizes():
    """{"shape-dtype-act-cuBUDGET": [forward, backward, pooled forward, pooled backward] (the pooled pair for a video shape only)}"""
    lib = L.lib()
    out = {}
    for budget in BUDGETS:
        with _budget(budget):
            for name, shape in SHAPES.items():
                for dt, dn in DTYPES:
                    for act, an in ACTS:
                        d = _dims(shape, dt, act)
                        out[f"{name}-{dn}-{an}-cu{budget}"] = [int(getattr(lib, q)(C.byref(d))) for q in (QUERIES if shape[5] else QUERIES[:2])]
    return out


def test_workspace_sizes_equal_the_ones_recorded_before_the_table():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = _sizes()
    assert set(got) == set(want) and len(got) == len(SHAPES) * 2 * 2 * 2
    assert all(v > 256 for vs in got.values() for v in vs)
    assert got == want


# ------------------------------------------------------------------------------------------------ the table is the step's
# entry of the table -> (name of the step-* case, split rule of a weight gradient | None)
DENSE_ENTRIES = {"DPRE": ("dpre", None), "DW2": ("dw2", "slack"), "DH2": ("dh2", None), "DW1": ("dw1", "slack"),
                 "DATTN": ("dattn", None), "DWO": ("dwo", "slack"), "DH1": ("dh1", None), "DWQKV": ("dwqkv", "general")}
FIELDS = ("M", "N", "K", "a_kstrided", "b_kstrided", "lda", "ldb", "ldc", "ldr", "in_dtype", "out_dtype", "epilogue", "split_k",
          "a_grp", "a_grp_stride", "a_off", "c_grp", "c_grp_stride", "c_off")
PRESENCE = ("A", "B", "C", "bias", "resid", "aux", "colsum_partials", "m_tiles", "k_tiles")


@pytest.mark.parametrize("budget", BUDGETS)
@pytest.mark.parametrize("dt,dn", DTYPES, ids=[n for _, n in DTYPES])
@pytest.mark.parametrize("tower", ["video", "text"])
def test_the_table_is_the_case_table_of_the_step(tower, dt, dn, budget):
    """shape, layout, pitches, dtypes, epilogue, row remaps, which optional operands the planner sees, and the split the call will
    use, field by field against gemm_cases.desc_fields; the operands themselves are null"""
    from xpretrain_amd import hip_ops as H
    cases = {c["id"]: c for c in G.CASES}
    with _budget(budget):
        table = H.layer_bwd_gemms(_dims(SHAPES[f"step_{tower}"], dt))
    assert len(table) == len(DENSE_ENTRIES) == L.XP_LAYER_GEMM_DENSE_COUNT
    for entry, (name, rule) in DENSE_ENTRIES.items():
        d = table[getattr(L, "XP_LAYER_GEMM_" + entry)]
        c = cases[f"step-{dn if dn != 'fp32' else 'f32'}-{tower}-{name}" + (f"-{rule}-cu{budget}" if rule else "")]
        want = G.desc_fields(c)
        if rule:
            want["split_k"] = c["expect"]["split"]
        assert {f: getattr(d, f) for f in FIELDS} == {f: want[f] for f in FIELDS}, (c["id"], entry)
        assert {f: bool(getattr(d, f)) for f in PRESENCE} == {f: bool(want.get(f)) for f in PRESENCE}, (c["id"], entry)


def test_the_pooled_table_and_the_refusals():
    from xpretrain_amd import hip_ops as H
    lib = L.lib()
    B, S, D, Dff = G.BATCH, V["S"], V["D"], V["Dff"]
    d = _dims(SHAPES["step_video"])
    table = H.layer_bwd_gemms(d, pooled=True)
    assert len(table) == L.XP_LAYER_GEMM_POOLED_COUNT
    mnk = lambda i: (table[i].M, table[i].N, table[i].K)
    # the shared stages over the B pooled rows, fc1's bias gradient never fused; the front over every row and the pooled rows
    assert [mnk(getattr(L, "XP_LAYER_GEMM_" + n)) for n in ("DPRE", "DW2", "DH2", "DW1", "DATTN", "DWO")] == \
        [(B, Dff, D), (D, Dff, B), (B, D, Dff), (Dff, D, B), (B, D, D), (D, D, B)]
    assert not table[L.XP_LAYER_GEMM_DPRE].colsum_partials and table[L.XP_LAYER_GEMM_DPRE].resid
    kv, q, wq, wkv = (table[getattr(L, "XP_LAYER_GEMM_" + n)] for n in ("DH1_KV", "DH1_Q", "DWQ", "DWKV"))
    assert mnk(L.XP_LAYER_GEMM_DH1_KV) == (B * S, D, 2 * D) and (kv.lda, kv.ldb, kv.b_kstrided) == (3 * D, D, 1)
    assert mnk(L.XP_LAYER_GEMM_DH1_Q) == (B, D, 3 * D) and (q.a_grp, q.a_grp_stride, q.c_grp, q.c_grp_stride) == (1, S, 1, S)
    assert mnk(L.XP_LAYER_GEMM_DWQ) == (D, D, B) and (wq.lda, wq.ldb, wq.a_grp, wq.a_grp_stride, wq.out_dtype) == (3 * D, D, 1, S, L.XP_F32)
    assert mnk(L.XP_LAYER_GEMM_DWKV) == (2 * D, D, B * S) and (wkv.lda, wkv.ldb, wkv.a_kstrided, wkv.b_kstrided) == (3 * D, D, 1, 1)
    for w, ask in ((wq, lib.xp_gemm_auto_split_slack), (wkv, lib.xp_gemm_auto_split)):
        assert w.split_k == max(1, ask(C.byref(w)))
    # nothing is written past `cap`, bad dims and a text layer asked for its pooled table are refused
    out = (L.XpGemmDesc * L.XP_LAYER_GEMM_MAX)()
    assert lib.xp_debug_layer_bwd_gemms(C.byref(d), 0, out, L.XP_LAYER_GEMM_DENSE_COUNT - 1) == L.XP_ERR_ARG and not out[0].M
    assert lib.xp_debug_layer_bwd_gemms(None, 0, out, len(out)) == L.XP_ERR_ARG
    assert lib.xp_debug_layer_bwd_gemms(C.byref(_dims(SHAPES["step_text"])), 1, out, len(out)) == L.XP_ERR_ARG
    bad = _dims(SHAPES["step_video"])
    bad.rows += 1
    assert lib.xp_debug_layer_bwd_gemms(C.byref(bad), 0, out, len(out)) == L.XP_ERR_ARG


# ------------------------------------------------------------------------------------------------ the lists are unchanged
@pytest.mark.parametrize("shape,slabs", [("step_video", [(3, 6336), (3, 6336), (12, 1600)]), ("listed_8240", [(3, 2752), (3, 2752), (12, 704)])])
def test_the_host_half_of_dx3_support_builds_the_recorded_lists(shape, slabs):
    """the splits and slab lengths are rows 0 and 1 of tests/test_tile_lists_cpu.py::CASES; the lists are dx3_tile_lists' of them"""
    import xpretrain_amd.functional as XF
    from tests.test_tile_lists_cpu import CASES
    b, s, d_, dff, heads, size = SHAPES[shape]
    assert (b, s, 0, slabs) in CASES
    plan = XF._layer_plan(b * s, d_, dff, b, s, heads, size, torch.bfloat16)
    m_tiles, lists, splits = XF._dx3_lists(plan.dims, 0)
    assert splits == (3, 3, 12)
    assert (m_tiles, lists) == XF.dx3_tile_lists(b, s, 0, slabs)
    assert XF._dx3_lists(plan.dims, s - 1) is not None and XF._dx3_support(plan, "cpu", (b, s + 1, 0)) is None


def test_fp32_and_a_small_shape_run_dense():
    import xpretrain_amd.functional as XF
    b, s, d_, dff, heads, size = SHAPES["step_video"]
    assert XF._dx3_lists(XF._layer_plan(b * s, d_, dff, b, s, heads, size, torch.float32).dims, 0) is None
    b, s, d_, dff, heads, size = SHAPES["small_video"]
    assert XF._dx3_lists(XF._layer_plan(b * s, d_, dff, b, s, heads, size, torch.bfloat16).dims, 0) is None


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    with open(GOLDEN, "w") as f:
        json.dump(_sizes(), f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {GOLDEN}")
