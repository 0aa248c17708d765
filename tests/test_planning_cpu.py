"""CPU: the host-side planning entry points of the C ABI (no kernel is launched, no GPU needed): split-K planning,
fused-column-sum availability, partial-row counts and workspace sizes, the GEMM and attention plans."""
import ctypes as C
import os
import re

import pytest

from xpretrain_amd import _lib as L


def _desc(M, N, K, *, a_ks=True, b_ks=True, dtype=L.XP_BF16, out=L.XP_F32, epi=L.EPI_NONE, split=1):
    d = L.XpGemmDesc()
    d.M, d.N, d.K = M, N, K
    d.lda = M if a_ks else K
    d.ldb = N if b_ks else K
    d.ldc = N
    d.a_kstrided, d.b_kstrided = int(a_ks), int(b_ks)
    d.in_dtype, d.out_dtype, d.epilogue, d.split_k = dtype, out, epi, split
    return d


def _valid_split(K, s, ke=64):
    kps = -(-(-(-K // s)) // ke) * ke
    return -(-K // kps) == s


@pytest.mark.parametrize("M,N,K,expect", [(2304, 768, 18848, 5), (768, 768, 18848, 16), (3072, 768, 18848, 4),
                                          (768, 3072, 18848, 4)])
def test_auto_split_cfg2_weight_gradients(M, N, K, expect):
    """split-K launches fill at most 144 CUs (csrc/gemm.hip::XP_SPLITK_FILL, 176 in round 5: they run beside the dX chain, and every
    split is an fp32 slab written and read again): 36 / 27 / 9 tiles x 4 / 5 / 16"""
    s = L.lib().xp_gemm_auto_split(C.byref(_desc(M, N, K)))
    assert s == expect and _valid_split(K, s) and s * (-(-M // 256)) * (-(-N // 256)) <= 144


@pytest.mark.parametrize("M,N,K,expect", [(768, 768, 18848, 12), (3072, 768, 18848, 3), (768, 3072, 18848, 3), (2304, 768, 18848, 4)])
def test_auto_split_of_launches_with_slack(M, N, K, expect):
    """xp_gemm_auto_split_slack: the first three weight-gradient GEMMs of a layer's backward (nothing waits for them soon) fill at most
    112 CUs: fc2 / fc1 3 slabs, out_proj 12; never more slabs than the general plan"""
    lib = L.lib()
    s = lib.xp_gemm_auto_split_slack(C.byref(_desc(M, N, K)))
    assert s == expect and _valid_split(K, s) and s <= lib.xp_gemm_auto_split(C.byref(_desc(M, N, K)))


def test_auto_split_is_always_accepted():
    lib = L.lib()
    for M, N in [(512, 512), (1536, 512), (2048, 512), (512, 2048), (768, 768), (256, 256), (3072, 768), (128, 96)]:
        for K in [31, 64, 200, 256, 1000, 4096, 6276 * 8, 18848, 100000]:
            for dtype in (L.XP_BF16, L.XP_F32):
                s = lib.xp_gemm_auto_split(C.byref(_desc(M, N, K, dtype=dtype)))
                assert s >= 1
                ke = 64 if dtype == L.XP_BF16 else 32
                assert s == 1 or _valid_split(K, s, ke) or _valid_split(K, s, 64), (M, N, K, dtype, s)


def test_fused_colsum_availability():
    lib = L.lib()
    big = dict(a_ks=False, b_ks=True, out=L.XP_BF16)
    assert lib.xp_gemm_colsum_rows(C.byref(_desc(18848, 3072, 768, epi=L.EPI_GELU_BWD, **big))) == 2 * 74      # 74 tiles of 256 rows (default height)
    assert lib.xp_gemm_colsum_rows(C.byref(_desc(18848, 768, 768, epi=L.EPI_NONE, **big))) == 2 * 74
    assert lib.xp_gemm_colsum_rows(C.byref(_desc(256, 2048, 512, epi=L.EPI_GELU_BWD, **big))) == 0          # text tower: 128 family
    assert lib.xp_gemm_colsum_rows(C.byref(_desc(18848, 3072, 768, epi=L.EPI_BIAS, **big))) == 0            # other epilogue
    assert lib.xp_gemm_colsum_rows(C.byref(_desc(18848, 3072, 768, a_ks=False, b_ks=True, out=L.XP_F32))) == 0
    assert lib.xp_gemm_colsum_rows(C.byref(_desc(18848, 3072, 768, split=2, **big))) == 0
    assert lib.xp_gemm_colsum_rows(C.byref(_desc(18848, 3072, 768, dtype=L.XP_F32, **big))) == 0


def test_tile_height_planning():
    """xp_gemm_tile_rows: 256 for everything the 256-wide family serves (video-tower activations and weight gradients), 128 = the
    128x128 family (text tower, fp32 inputs)."""
    lib = L.lib()
    act = dict(a_ks=False, b_ks=False, out=L.XP_BF16)
    for N in (768, 2304, 3072):
        assert lib.xp_gemm_tile_rows(C.byref(_desc(18848, N, 768, **act))) == 256
    assert lib.xp_gemm_tile_rows(C.byref(_desc(18848, 768, 3072, a_ks=False, b_ks=True, out=L.XP_BF16))) == 256
    assert lib.xp_gemm_tile_rows(C.byref(_desc(50208, 768, 768, **act))) == 256
    assert lib.xp_gemm_tile_rows(C.byref(_desc(3072, 768, 18848, split=4))) == 256        # dW1: 36 tiles x 4 slabs
    assert lib.xp_gemm_tile_rows(C.byref(_desc(256, 2048, 512, **act))) == 128            # text tower
    assert lib.xp_gemm_tile_rows(C.byref(_desc(18848, 768, 768, dtype=L.XP_F32, a_ks=False, b_ks=False))) == 128


def _tile_rows(M, N, K, b_kstrided=False, split_k=1, out_f32=False):
    d = L.XpGemmDesc()
    d.M, d.N, d.K, d.lda, d.ldb, d.ldc, d.ldr, d.ldaux = M, N, K, K, (N if b_kstrided else K), N, N, N
    d.b_kstrided, d.in_dtype, d.out_dtype, d.split_k = int(b_kstrided), L.XP_BF16, (L.XP_F32 if out_f32 else L.XP_BF16), split_k
    return int(L.lib().xp_gemm_tile_rows(C.byref(d)))


def test_kernel_family_per_shape():
    """the video-tower shapes of BASELINE cfg #2 / configs[3] run the 256-wide family, small problems the 128x128 family"""
    assert _tile_rows(18848, 768, 768) == 256 and _tile_rows(18848, 3072, 768, b_kstrided=True) == 256
    assert _tile_rows(50208, 768, 768) == 256 and _tile_rows(16384, 1024, 512) == 256
    assert _tile_rows(256, 512, 768) == 128


def _cdiv(a, b):
    return -(-a // b)


_SWEEP_ROWS = (300, 2356, 4609, 4712, 9424, 16384, 18848, 18848 - 200, 50208)
_SWEEP_DIMS = (128, 512, 768, 1280, 1536, 2048, 2304, 3072)


@pytest.mark.parametrize("rows", _SWEEP_ROWS)
def test_plan_invariants(rows):
    """What one plan guarantees to the callers that size buffers by the planning queries (hip_ops.gemm, csrc/layer.hip): fused column
    sums only in the 256-wide family, one partial row per 128 output rows; split-K answers that xp_gemm accepts, the slack one never
    with more slabs than the general one; the 256-wide family only where it can run the split (bf16, whole 64-deep k-tiles per slab,
    >= 2 of them in the last slab).  (A split from the 128x128 family's formula may run on the 256-wide family.)"""
    lib = L.lib()
    for a, b in [(a, b) for a in _SWEEP_DIMS for b in _SWEEP_DIMS]:
        for M, N, K, a_ks, b_ks in ((rows, a, b, False, False), (rows, a, b, False, True), (a, b, rows, True, True), (a, b, rows, True, False)):
            for dtype, out in ((L.XP_BF16, L.XP_BF16), (L.XP_BF16, L.XP_F32), (L.XP_F32, L.XP_F32)):
                for epi in (L.EPI_NONE, L.EPI_GELU_BWD, L.EPI_BIAS):
                    d = _desc(M, N, K, a_ks=a_ks, b_ks=b_ks, dtype=dtype, out=out, epi=epi)
                    if epi == L.EPI_GELU_BWD:
                        d.resid, d.ldr = 1, N
                    cs = lib.xp_gemm_colsum_rows(C.byref(d))
                    if cs > 0:
                        assert lib.xp_gemm_tile_rows(C.byref(d)) == 256 and cs == 2 * _cdiv(M, 256), (M, N, K, epi)
                    s, slack = lib.xp_gemm_auto_split(C.byref(d)), lib.xp_gemm_auto_split_slack(C.byref(d))
                    assert slack <= s, (M, N, K)
                    for split in (s, slack):
                        assert split == 1 or _valid_split(K, split, 64 if dtype == L.XP_BF16 else 32), (M, N, K, dtype, split)
                        d.split_k = split
                        if lib.xp_gemm_tile_rows(C.byref(d)) == 256:
                            kps = _cdiv(_cdiv(K, split), 64) * 64
                            assert dtype == L.XP_BF16 and _valid_split(K, split) and K - (split - 1) * kps > 64, (M, N, K, split)
                    d.split_k = 1


def test_cu_budget_shrinks_the_split():
    """xp_set_cu_budget: a data-parallel run reserves the CUs its collective kernels own (distributed.reserve_cus_for_collectives);
    the dW launches must then fit the remaining CUs in one round."""
    lib = L.lib()
    try:
        for budget, expect in ((256, (4, 5, 16)), (224, (4, 5, 16)), (160, (4, 5, 16)), (128, (3, 4, 14))):      # (whole 64-token k-steps per slab)
            assert lib.xp_set_cu_budget(budget) == 0 and lib.xp_get_cu_budget() == budget
            got = tuple(lib.xp_gemm_auto_split(C.byref(_desc(M, N, 18848))) for M, N in ((3072, 768), (2304, 768), (768, 768)))
            tiles = (36, 27, 9)
            assert all(s * t <= budget for s, t in zip(got, tiles)), (budget, got)
            assert got == expect, (budget, got)
        assert lib.xp_set_cu_budget(32) != 0           # out of range: refused
    finally:
        lib.xp_set_cu_budget(256)


def test_partial_row_counts_and_workspaces():
    lib = L.lib()
    for rows in (1, 31, 256, 18848, 50208):
        for cols in (64, 768, 2304, 3072):
            n = lib.xp_colsum_partial_rows(rows, cols)
            assert 1 <= n <= -(-rows // 32) and n >= -(-rows // 128)
            assert lib.xp_colsum_workspace_bytes(rows, cols) >= (n + 32) * cols * 4
        nb = lib.xp_layernorm_bwd_partial_rows(rows)
        assert 1 <= nb <= 512
        assert lib.xp_layernorm_bwd_workspace_bytes(rows, 768) >= nb * 3 * 768 * 4
    segs = (L.XpReduceSeg * 3)()
    for i, w in enumerate((768, 3072, 64)):
        segs[i].width, segs[i].nrows, segs[i].stride = w, 100, w
    assert lib.xp_reduce_rows_batch_workspace_bytes(segs, 3) >= 32 * (768 + 3072 + 64) * 4
    # attention: forward partials / backward (delta + proxy partials) share one workspace
    assert lib.xp_attn_workspace_bytes(L.ATTN_PROXY, 8, 12, 4, 12, 196) >= 8 * 12 * 2356 * 4
    assert lib.xp_attn_workspace_bytes(L.ATTN_CAUSAL, 8, 8, 0, 1, 32) == 8 * 8 * 32 * 4
    assert lib.xp_contrastive_loss_workspace_bytes(L.XP_LOSS_NCE, 64, 64, 512) >= 2 * 64 * 64 * 4
    assert lib.xp_contrastive_loss_workspace_bytes(L.XP_LOSS_VSC_FC, 64, 64, 512) >= 6 * 64 * 64 * 4


def _dims(rows, D, Dff, B, S, heads, size, dtype=L.XP_BF16):
    d = L.XpLayerDims()
    d.rows, d.D, d.Dff, d.B, d.S, d.heads = rows, D, Dff, B, S, heads
    d.M, d.N, d.L = size if size else (0, 1, S)
    d.attn_mode = L.ATTN_PROXY if size else L.ATTN_CAUSAL
    d.dtype, d.q_scale, d.ln_eps = dtype, 0.125, 1e-5
    return d


def test_encoder_layer_workspace_planning():
    """xp_encoder_layer_{fwd,bwd}_workspace_bytes (csrc/layer.hip): the backward workspace holds the six activation-gradient
    temporaries, the largest split-K slab set, the deferred partial rows, the reduce scratch and the attention workspace."""
    lib = L.lib()
    d = _dims(8 * 2356, 768, 3072, 8, 2356, 12, (4, 12, 196))
    fwd, bwd = lib.xp_encoder_layer_fwd_workspace_bytes(C.byref(d)), lib.xp_encoder_layer_bwd_workspace_bytes(C.byref(d))
    rows, D, Dff = 8 * 2356, 768, 3072
    temporaries = rows * (Dff + 4 * D + 3 * D) * 2
    slabs = 4 * 3072 * 768 * 4                                     # fc1 / fc2 dW: split-K 4 (test above)
    assert fwd >= lib.xp_attn_workspace_bytes(L.ATTN_PROXY, 8, 12, 4, 12, 196)
    assert temporaries + slabs < bwd < temporaries + slabs + (64 << 20)
    # text tower shape, fp32 mode: still consistent, and empty dims give 0
    t = _dims(8 * 32, 512, 2048, 8, 32, 8, None, L.XP_F32)
    assert lib.xp_encoder_layer_bwd_workspace_bytes(C.byref(t)) > 8 * 32 * (2048 + 7 * 512) * 4
    z = _dims(0, 512, 2048, 8, 32, 8, None)
    assert lib.xp_encoder_layer_bwd_workspace_bytes(C.byref(z)) == 0


def test_encoder_layer_rejects_bad_arguments():
    lib = L.lib()
    a = L.XpLayerFwd()
    a.dims = _dims(100, 768, 3072, 8, 2356, 12, (4, 12, 196))       # rows != B*S
    assert lib.xp_encoder_layer_fwd(C.byref(a), None) != 0 and b"rows" in lib.xp_last_error()
    b = L.XpLayerBwd()
    b.dims = _dims(8 * 32, 512, 2048, 8, 32, 8, None)
    assert lib.xp_encoder_layer_bwd(C.byref(b), None) != 0 and b"null pointer" in lib.xp_last_error()


# ---------------------------------------------------------------------------------------------- the plan query and the case table
from tests import gemm_cases as G      # noqa: E402  (plain data)


def case_desc(c):
    d = L.XpGemmDesc()
    for k, v in G.desc_fields(c).items():
        setattr(d, k, v)
    return d


def set_case_env(c, monkeypatch):
    """the case's XPRETRAIN_GEMM256 / XPRETRAIN_DEBUG (the library reads both at every call); the CU budget is set by case_budget"""
    if c["gemm256"] is None:
        monkeypatch.delenv("XPRETRAIN_GEMM256", raising=False)
    else:
        monkeypatch.setenv("XPRETRAIN_GEMM256", str(c["gemm256"]))
    if c["debug"]:
        monkeypatch.setenv("XPRETRAIN_DEBUG", ",".join(c["debug"]))
    else:
        monkeypatch.delenv("XPRETRAIN_DEBUG", raising=False)


class case_budget:
    """xp_set_cu_budget(case budget) for the duration of a with-block, the previous budget restored after"""

    def __init__(self, c):
        self.budget = c["budget"]

    def __enter__(self):
        self.prev = L.lib().xp_get_cu_budget()
        assert L.lib().xp_set_cu_budget(self.budget) == 0
        return self

    def __exit__(self, *exc):
        L.lib().xp_set_cu_budget(self.prev)


def resolve_split(c, d):
    """the case's split: its int, or what xp_gemm_auto_split / _slack answer for its descriptor"""
    if c["split"] == "general":
        return int(L.lib().xp_gemm_auto_split(C.byref(d)))
    if c["split"] == "slack":
        return int(L.lib().xp_gemm_auto_split_slack(C.byref(d)))
    return int(c["split"])


def check_plan(c, plan, split):
    """the plan the case declares"""
    e = c["expect"]
    got = dict(family=G.FAMILIES[plan["family"]], impl=G.IMPLS[plan["epi_impl"]], split=split)
    assert got == e, (c["id"], got, e)
    assert plan["split"] == split and plan["tile_rows"] == G.TILE_ROWS[e["family"]], (c["id"], plan)
    assert plan["colsum_rows"] > 0 or not c["colsum"], (c["id"], plan)


@pytest.mark.parametrize("c", G.CASES, ids=[c["id"] for c in G.CASES])
def test_case_table_plans(c, monkeypatch):
    """every case of tests/gemm_cases.py gets the plan (kernel family / loader, epilogue implementation, split) it declares"""
    from xpretrain_amd import hip_ops as H
    set_case_env(c, monkeypatch)
    with case_budget(c):
        d = case_desc(c)
        split = resolve_split(c, d)
        d.split_k = split
        plan = H.gemm_plan_of(d)
    check_plan(c, plan, split)


def _sweep_descs():
    for rows in _SWEEP_ROWS:
        for a, b in [(a, b) for a in _SWEEP_DIMS for b in _SWEEP_DIMS]:
            for M, N, K, a_ks, b_ks in ((rows, a, b, False, False), (rows, a, b, False, True), (a, b, rows, True, True),
                                        (a, b, rows, True, False)):
                for dtype, out in ((L.XP_BF16, L.XP_BF16), (L.XP_BF16, L.XP_F32), (L.XP_F32, L.XP_F32)):
                    yield _desc(M, N, K, a_ks=a_ks, b_ks=b_ks, dtype=dtype, out=out)


@pytest.mark.parametrize("rows", _SWEEP_ROWS)
def test_plan_query_agrees_with_the_planning_queries(rows):
    """xp_debug_gemm_plan answers from the plan the other planning queries read: tile rows, column-sum rows, the auto splits; its
    grid covers every tile and every slab exactly once"""
    from xpretrain_amd import hip_ops as H
    lib = L.lib()
    for d in _sweep_descs():
        if d.M != rows and d.K != rows:
            continue
        for epi in (L.EPI_NONE, L.EPI_GELU_BWD, L.EPI_BIAS):
            d.epilogue, d.resid, d.ldr, d.split_k = epi, (1 if epi == L.EPI_GELU_BWD else 0), d.N, 1
            for cs in (0, 1):
                d.colsum_partials = cs
                p = H.gemm_plan_of(d)
                assert p["colsum_rows"] == lib.xp_gemm_colsum_rows(C.byref(d)), (d.M, d.N, d.K, epi)
            d.colsum_partials = 0
            for split in (1, lib.xp_gemm_auto_split(C.byref(d)), lib.xp_gemm_auto_split_slack(C.byref(d))):
                d.split_k = split
                p = H.gemm_plan_of(d)
                assert p["tile_rows"] == lib.xp_gemm_tile_rows(C.byref(d)) and p["split"] == split, (d.M, d.N, d.K, split, p)
                assert p["tiles_m"] == _cdiv(d.M, p["tile_rows"]) and p["tiles_n"] == _cdiv(d.N, p["tile_rows"])
                assert (split - 1) * p["k_per_split"] < d.K <= split * p["k_per_split"], (d.M, d.N, d.K, split, p)
                tiles = p["tiles_m"] * p["tiles_n"]
                assert p["grid"] == ((tiles * split, 1, 1) if p["flat_split"] else (tiles, 1, split)), p
                assert p["flat_split"] in (0, split) and (p["flat_split"] == 0 or (p["family"] == L.GEMM_FAMILY_256 and split > 1))
                assert p["family"] == L.GEMM_FAMILY_256 or p["colsum_rows"] == 0


def _accepted(d):
    """the argument rules of xp_gemm that do not concern data (csrc/gemm.hip::xp_gemm)"""
    epc = 8 if d.in_dtype == L.XP_BF16 else 4
    a_contig, b_contig = (d.M if d.a_kstrided else d.K), (d.N if d.b_kstrided else d.K)
    return (a_contig % epc == 0 and b_contig % epc == 0 and d.lda % epc == 0 and d.ldb % epc == 0 and d.N % 4 == 0 and
            d.ldc % 4 == 0 and (d.out_dtype == d.in_dtype or d.out_dtype == L.XP_F32))


_LAYOUT_NAME = {v: k for k, v in G.LAYOUTS.items()}


def planner_combinations():
    """(variant, layout, epilogue kind, epilogue implementation, output dtype) of every plan over the _SWEEP_* grid, every epilogue
    kind, under each switch (XPRETRAIN_GEMM256=2, gemm_no_glds, gemm_slow_epi) and with the descriptor changes that move a problem
    to another variant (a pitch that is not a multiple of 8, a row-remapped output, a padded / remapped A)"""
    lib = L.lib()
    info = L.XpGemmPlanInfo()
    found = set()
    perturb = [(lo, ep) for lo in (None, "lda", "a_remap") for ep in (None, "ldc", "c_remap")]
    envs = [dict(), dict(XPRETRAIN_GEMM256="2"), dict(XPRETRAIN_DEBUG="gemm_no_glds"), dict(XPRETRAIN_DEBUG="gemm_slow_epi")]
    saved = {k: os.environ.get(k) for k in ("XPRETRAIN_GEMM256", "XPRETRAIN_DEBUG")}
    try:
        for env in envs:
            for k in saved:
                os.environ.pop(k, None)
            os.environ.update(env)
            for d in _sweep_descs():
                lay = _LAYOUT_NAME[(d.a_kstrided, d.b_kstrided)]
                out = "bf16" if d.out_dtype == L.XP_BF16 else "f32"
                for lo, ep in (perturb if not env else [(None, None)]):
                    d.lda, d.ldc = (d.M if d.a_kstrided else d.K), d.N
                    d.a_grp = d.c_grp = 0
                    if ep == "ldc":
                        d.ldc = d.N + 4
                    elif ep == "c_remap":
                        d.c_grp, d.c_grp_stride, d.c_off = 64, 96, 16
                    if lo == "lda":
                        d.lda += 8
                    elif lo == "a_remap":
                        d.a_grp, d.a_grp_stride, d.a_off = 64, 80, 16
                    if not _accepted(d):
                        continue
                    for epi in range(8):
                        d.epilogue = epi
                        d.resid, d.ldr = (1 if epi in (L.EPI_BIAS_RESID, L.EPI_GELU_BWD) else 0), d.N
                        assert lib.xp_debug_gemm_plan(C.byref(d), C.byref(info)) == 0
                        found.add((G.FAMILIES[info.family], lay, G.EPIS[epi], G.IMPLS[info.epi_impl], out))
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return found


def test_case_table_covers_every_plan():
    """Coverage: every (variant, layout, epilogue kind, epilogue implementation, output dtype) the planner produces over the sweep
    has a case in tests/gemm_cases.py.  If the planner stops routing a case's problem to its variant, test_case_table_plans fails;
    if it starts producing a new combination, this does -- the GPU tests never quietly run something else than they name."""
    found = planner_combinations()
    have = {(c["expect"]["family"], c["layout"], c["epi"], c["expect"]["impl"], c["out"]) for c in G.CASES}
    missing = sorted(found - have)
    assert not missing, f"{len(missing)} planner combinations without a case in tests/gemm_cases.py, e.g. {missing[:10]}"


# ---------------------------------------------------------------------------------------------- attention plans
from tests import test_attention_gpu as AG      # noqa: E402  (its case tables)

_PERSISTENT = ("fwd3", "fwd4", "bwd5")


def _attn_rule(mode, B, H, S, M, N, Lp, f32, pad, bwd, cus, split):
    """(kernel, main grid) by the rules of csrc/attention.hip::plan_attn, restated"""
    if f32:
        return "f32", 0
    R, nprob = (M + Lp if mode == L.ATTN_PROXY else S), B * H * N
    persistent = mode == L.ATTN_PROXY and M <= 16 and not pad
    if not bwd and persistent and R <= 208:
        return "fwd3", min(nprob, cus)
    if not bwd and persistent and cus % 8 == 0 and cus // 8 >= _cdiv(_cdiv(R, 16), 16):
        return "fwd4", cus
    if bwd and persistent and R <= 208 and not split:
        return "bwd5", min(nprob, cus)
    return ("bwd_pair" if bwd else "fwd"), _cdiv(nprob, 8) * 8 * _cdiv(R, 112)


def _attn_geoms():
    """(mode, B, H, S, M, N, L): proxy rows R = M + L on both sides of 208, M on both sides of 16, and causal problems"""
    for B, H in ((1, 1), (2, 3), (8, 12)):
        for M in (1, 4, 16, 17, 20):
            for N in (1, 3, 12):
                for Lp in (5, 49, 192, 196, 204, 205, 300, 784, 1023):
                    yield L.ATTN_PROXY, B, H, M + N * Lp, M, N, Lp
        for S in (7, 32, 77, 130, 300):
            yield L.ATTN_CAUSAL, B, H, S, 0, 1, S


@pytest.mark.parametrize("split", [False, True])
def test_attention_plan_rules(split, monkeypatch):
    """xp_debug_attn_plan over geometries, padding, CU counts, dtypes and both directions: the kernel and grids of the rules above;
    dynamic LDS exactly for the persistent kernels; the problem counter exactly for attn_bwd5; workspace regions of the sizes the
    kernels write, 4-byte aligned, disjoint and inside xp_attn_workspace_bytes, which keeps its formula; column-sum rows as
    xp_attn_bwd_colsum_rows"""
    import torch
    from xpretrain_amd import hip_ops as H
    lib = L.lib()
    if split:
        monkeypatch.setenv("XPRETRAIN_DEBUG", "attn_bwd_split")
    else:
        monkeypatch.delenv("XPRETRAIN_DEBUG", raising=False)
    for mode, B, Hh, S, M, N, Lp in _attn_geoms():
        P = B * Hh * N
        size = (M, N, Lp) if mode == L.ATTN_PROXY else None
        ws = lib.xp_attn_workspace_bytes(mode, B, Hh, M, N, Lp)
        assert ws == (4 * max(P * M * 66, B * Hh * S + P * M * 192 + 64) if size else 4 * B * Hh * S), (size, B, Hh)
        for f32 in (False, True):
            dtype = L.XP_F32 if f32 else L.XP_BF16
            rows = lib.xp_attn_bwd_colsum_rows(mode, B, Hh, S, M, N, Lp, dtype)
            for pad in (False, True):
                for cus in (256, 80, 36, 8):
                    for bwd in (False, True):
                        p = H.attn_plan(B, S, Hh, size=size, pad_mask=(True if pad else None),
                                        dtype=(torch.float32 if f32 else torch.bfloat16), backward=bwd, cus=cus)
                        case = (size, B, Hh, S, f32, pad, cus, bwd, p)
                        assert (p["kernel"], p["grid"]) == _attn_rule(mode, B, Hh, S, M, N, Lp, f32, pad, bwd, cus, split), case
                        assert (p["lds_bytes"] > 0) == (p["kernel"] in _PERSISTENT) and p["lds_bytes"] <= 160 * 1024, case
                        assert p["uses_counter"] == (p["kernel"] == "bwd5"), case
                        assert p["reduce_grid"] == (B * Hh * M if size and not f32 else 0), case
                        assert p["colsum_rows"] == rows, case
                        want = (dict(part=0, delta=4 * B * Hh * S, dq=4 * P * M * 64, dkv=4 * P * M * 128, counter=256 if size else 0)
                                if bwd else dict(part=4 * P * M * 66, delta=0, dq=0, dkv=0, counter=0))
                        assert {r: p[r][1] for r in want} == want, case
                        used = sorted(p[r] for r in want if p[r][1])
                        assert all(off % 4 == 0 and n % 4 == 0 for off, n in used), case
                        assert all(a[0] + a[1] <= b[0] for a, b in zip(used, used[1:])), case
                        end = used[-1][0] + used[-1][1] if used else 0
                        assert p["workspace_bytes"] == end <= ws, case


def test_attention_gpu_cases_name_the_kernels_they_run():
    """Every case of tests/test_attention_gpu.py names the kernels the planner gives it at 256 CUs (an MI355X), and every
    XP_ATTN_KERNEL_* is run by some case.  If the planner moves a case to another kernel, or a kernel loses its last case, this
    fails -- the GPU tests never quietly run something else than they name."""
    import torch
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "xpretrain_hip.h")).read()
    declared = {int(v): n.lower() for n, v in re.findall(r"XP_ATTN_KERNEL_(\w+) = (\d+)", header)}
    assert declared == dict(enumerate(L.ATTN_KERNELS))
    run = set()

    def check(kernels, B, S, H, **kw):
        AG.check_kernels(kernels, B, S, H, cus=256, **kw)
        run.update(kernels)
    for (size, B, H), kernels in list(AG.PROXY_CASES.items()) + [(AG.RESCALE_CASE, AG.FUSED)] + \
            [(c, AG.FUSED) for c in AG.FUSED_VS_SPLIT_CASES]:
        check(kernels, B, size[0] + size[1] * size[2], H, size=size)
    for size, B, H in AG.PROXY_F32_CASES:
        check(AG.F32, B, size[0] + size[1] * size[2], H, size=size, dtype=torch.float32)
    for (B, S, H, mode), kernels in [(c, AG.GENERAL) for c in AG.CAUSAL_CASES] + [(c, AG.F32) for c in AG.CAUSAL_F32_CASES]:
        check(kernels, B, S, H, pad=mode != "none", dtype=(torch.float32 if kernels == AG.F32 else torch.bfloat16))
    missing = sorted(set(L.ATTN_KERNELS) - run)
    assert not missing, f"no case of tests/test_attention_gpu.py runs XP_ATTN_KERNEL_{'/'.join(m.upper() for m in missing)}"
