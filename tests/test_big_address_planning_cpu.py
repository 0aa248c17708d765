"""CPU: the planner's three address-span limits, each pinned from both sides, and the entry points' refusals of what their kernels
cannot address (no kernel is launched, no GPU needed).

The limits are restated here from the constants of csrc/gemm.hip::glds_ok, csrc/gemm256.hip::xp_gemm256_legal and
csrc/gemm.hip::plan_gemm -- nothing below is taken from the planner's answers:

  DIRECT family (buffer_load ... lds):   (rows + 128) * ld * esz  <  0xFFFFFFF0 - 256 MiB     for A and for B
  256-wide family:                       (rows + 256) * ld * 2    <  0xFFFFFFF0 - 512 MiB     for A and for B
  fast epilogue (32-bit row offsets):    (M + 256) * ld * size    <  0xFFFFFF00 - 64          for C, resid and aux

(rows: the operand's row count as stored -- M or N when k-contiguous, K when k-strided.)  Every operand is taken to the largest
row count below its limit and to the smallest one at or above it that the families' alignment preconditions admit; the plan's
family, epilogue implementation and split, and what xp_gemm_tile_rows / xp_gemm_colsum_rows / xp_gemm_auto_split answer (a caller
sizes its partial-row and slab buffers from these), must be what the rules say on both sides."""
import ctypes as C

import pytest

from xpretrain_amd import _lib as L

MiB = 1 << 20
LIM_DIRECT, PAD_DIRECT = 0xFFFFFFF0 - 256 * MiB, 128
LIM_256, PAD_256 = 0xFFFFFFF0 - 512 * MiB, 256
LIM_EPI, PAD_EPI = 0xFFFFFF00 - 64, 256
PITCH = 1 << 20                       # the epilogue operands' row pitch in elements

FAMILIES = ("g256", "direct", "staged", "frames")
IMPLS = ("fast", "row8", "row4")
ESZ = {L.XP_BF16: 2, L.XP_F32: 4}
FAST_KINDS = (L.EPI_NONE, L.EPI_BIAS, L.EPI_BIAS_QSCALE, L.EPI_BIAS_GELU, L.EPI_BIAS_RESID, L.EPI_GELU_BWD)


def _cdiv(a, b):
    return -(-a // b)


def rows_below(lim, pad, row_bytes, align=1):
    """the largest row count (a multiple of align) with (rows + pad) * row_bytes < lim"""
    return ((lim - 1) // row_bytes - pad) // align * align


def rows_at(lim, pad, row_bytes, align=1):
    """the smallest row count (a multiple of align) with (rows + pad) * row_bytes >= lim"""
    return _cdiv(_cdiv(lim, row_bytes) - pad, align) * align


def test_the_two_points_straddle_each_limit():
    for lim, pad in ((LIM_DIRECT, PAD_DIRECT), (LIM_256, PAD_256), (LIM_EPI, PAD_EPI)):
        for rb in (256 * 2, 512 * 4, 8192 * 2, 8192 * 4, PITCH * 2, PITCH * 4):
            for align in (1, 8):
                lo, hi = rows_below(lim, pad, rb, align), rows_at(lim, pad, rb, align)
                assert (lo + pad) * rb < lim <= (hi + pad) * rb and 0 < hi - lo <= align and lo % align == hi % align == 0


def desc(M, N, K, layout, dtype, out, *, epi=L.EPI_NONE, ldc=None, ldr=None, ldaux=None, resid=False, aux=False, split=1,
         colsum=False):
    a_ks, b_ks = {"nt": (0, 0), "nn": (0, 1), "tn": (1, 1), "tk": (1, 0)}[layout]
    d = L.XpGemmDesc()
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldb, d.ldc = (M if a_ks else K), (N if b_ks else K), ldc or N
    d.a_kstrided, d.b_kstrided, d.in_dtype, d.out_dtype, d.epilogue, d.split_k = a_ks, b_ks, dtype, out, epi, split
    d.ldr, d.ldaux = ldr or N, ldaux or N
    d.resid, d.aux, d.colsum_partials = int(resid), int(aux), int(colsum)      # (the planner reads them as present / absent)
    return d


# ---------------------------------------------------------------------------------------------- the rules, restated
def _operand_ok(d, lim, pad, esz, bm, ke):
    """glds_ok / xp_gemm256_legal without their switches: dense operands, whole k-tiles of k-contiguous operands, whole tiles of
    k-strided row extents, both spans below the limit"""
    for ks, rows_c, rows_s, ld in ((d.a_kstrided, d.M, d.K, d.lda), (d.b_kstrided, d.N, d.K, d.ldb)):
        if ks and (rows_c % bm or ld != rows_c):
            return False
        if not ks and (d.K % ke or ld != d.K):
            return False
        if ((rows_s if ks else rows_c) + pad) * ld * esz >= lim:
            return False
    return True


def expected_plan(d, split, mode):
    """(family, impl, tile rows, column-sum rows) by the rules of plan_gemm for an un-remapped problem; mode: XPRETRAIN_GEMM256"""
    esz, f32 = ESZ[d.in_dtype], d.out_dtype == L.XP_F32
    osz, ke, rows = (4 if f32 else esz), 128 // esz, d.M + PAD_EPI
    wide = d.N % 8 == 0 and d.ldc % 8 == 0 and (not d.resid or d.ldr % 8 == 0) and (not d.aux or d.ldaux % 8 == 0)
    fast = (wide and rows * d.ldc * osz < LIM_EPI and (not d.resid or rows * d.ldr * esz < LIM_EPI) and
            (not d.aux or rows * d.ldaux * osz < LIM_EPI))
    cs_kind = d.epilogue in (L.EPI_NONE, L.EPI_GELU_BWD)
    special = (not f32 and cs_kind) if d.colsum_partials else (d.epilogue == L.EPI_NONE if f32 else d.epilogue in FAST_KINDS)
    impl = "fast" if fast and special else "row8" if wide else "row4"
    kps = _cdiv(_cdiv(d.K, split), ke) * ke
    k_last = d.K - (split - 1) * kps
    legal256 = d.in_dtype == L.XP_BF16 and _operand_ok(d, LIM_256, PAD_256, 2, 256, 64)
    if (mode != 0 and legal256 and impl == "fast" and (mode != 1 or _cdiv(d.M, 256) * _cdiv(d.N, 256) * split >= 96) and
            _cdiv(k_last, 64) >= 2 and (split == 1 or _cdiv(d.K, kps) == split)):
        return "g256", impl, 256, (2 * _cdiv(d.M, 256) if split == 1 and not f32 and cs_kind else 0)
    return ("direct" if _operand_ok(d, LIM_DIRECT, PAD_DIRECT, esz, 128, ke) else "staged"), impl, 128, 0


def _valid_split(K, s0, ke):
    return 1 if s0 <= 1 else _cdiv(K, _cdiv(_cdiv(K, s0), ke) * ke)


def expected_auto_split(d, mode, fill=144, budget=256):
    """xp_gemm_auto_split by its rules (csrc/gemm.hip::auto_split_fill): the 256-wide family's split where that family takes it"""
    ke, t256 = 128 // ESZ[d.in_dtype], _cdiv(d.M, 256) * _cdiv(d.N, 256)
    s256 = _valid_split(d.K, min(min(budget, fill) // t256, d.K // 512), 64)
    if expected_plan(d, s256, mode)[0] == "g256":
        return s256
    t128 = _cdiv(d.M, 128) * _cdiv(d.N, 128)
    return 1 if t128 >= 256 else _valid_split(d.K, min(512 // t128, d.K // 512), ke)


def check_point(d, mode, family, impl, monkeypatch, *, split=1, auto_split=None):
    """the plan of `d` is (family, impl, split), and every planning query answers from it"""
    from xpretrain_amd import hip_ops as H
    lib = L.lib()
    monkeypatch.delenv("XPRETRAIN_DEBUG", raising=False)
    monkeypatch.setenv("XPRETRAIN_GEMM256", str(mode))
    assert lib.xp_get_cu_budget() == 256
    d.split_k = split
    where = (d.M, d.N, d.K, d.lda, d.ldb, d.ldc, d.ldr, d.ldaux, split)
    want = expected_plan(d, split, mode)
    assert want[:2] == (family, impl), ("the restated rules disagree with the case's own expectation", where, want)
    p = H.gemm_plan_of(d)
    assert (FAMILIES[p["family"]], IMPLS[p["epi_impl"]], p["split"]) == (family, impl, split), (where, p)
    assert (p["tile_rows"], p["colsum_rows"]) == want[2:], (where, p, want)
    assert lib.xp_gemm_tile_rows(C.byref(d)) == want[2] and lib.xp_gemm_colsum_rows(C.byref(d)) == want[3], where
    if auto_split is not None:
        d.split_k = 1
        got, exp = lib.xp_gemm_auto_split(C.byref(d)), expected_auto_split(d, mode)
        assert got == exp == auto_split, (where, got, exp, auto_split)
        assert lib.xp_gemm_auto_split_slack(C.byref(d)) <= got


# ---------------------------------------------------------------------------------------------- A and B: the two loader limits
# (name, layout, descriptor of `rows`, bytes per stored row / esz, row alignment xp_gemm and the fast epilogue ask of `rows`)
OPERANDS = {
    "A_kcontig": ("nt", lambda r: dict(M=r, N=128, K=8192), 8192, 1),
    "A_kstrided": ("tn", lambda r: dict(M=512, N=256, K=r), 512, 1),          # (B's span is half of A's: only A crosses)
    "B_kcontig": ("nt", lambda r: dict(M=128, N=r, K=8192), 8192, 8),
    "B_kstrided": ("tn", lambda r: dict(M=256, N=512, K=r), 512, 1),
}


def _operand_desc(op, rows, dtype, **kw):
    layout, dims, _, _ = OPERANDS[op]
    out = L.XP_F32 if layout == "tn" or dtype == L.XP_F32 else L.XP_BF16      # weight gradients are written in fp32
    return desc(layout=layout, dtype=dtype, out=out, **dims(rows), **kw)


@pytest.mark.parametrize("op", list(OPERANDS))
def test_bf16_operand_leaves_the_256_wide_family_at_its_limit(op, monkeypatch):
    """XPRETRAIN_GEMM256=2 (the 256-wide family wherever legal): 256-wide below 0xFFFFFFF0 - 512 MiB, DIRECT from there on"""
    _, _, ld, align = OPERANDS[op]
    lo, hi = rows_below(LIM_256, PAD_256, ld * 2, align), rows_at(LIM_256, PAD_256, ld * 2, align)
    assert (hi + PAD_DIRECT) * ld * 2 < LIM_DIRECT
    check_point(_operand_desc(op, lo, L.XP_BF16), 2, "g256", "fast", monkeypatch)
    check_point(_operand_desc(op, hi, L.XP_BF16), 2, "direct", "fast", monkeypatch)


@pytest.mark.parametrize("dtype", [L.XP_BF16, L.XP_F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("op", list(OPERANDS))
def test_operand_leaves_the_direct_family_at_its_limit(op, dtype, monkeypatch):
    """DIRECT below 0xFFFFFFF0 - 256 MiB, the register-staged loader from there on; with the 256-wide family switched off and with it
    wherever legal (it is not, above its own lower limit)"""
    _, _, ld, align = OPERANDS[op]
    esz = ESZ[dtype]
    lo, hi = rows_below(LIM_DIRECT, PAD_DIRECT, ld * esz, align), rows_at(LIM_DIRECT, PAD_DIRECT, ld * esz, align)
    assert (lo + PAD_256) * ld * esz >= LIM_256
    for mode in (0, 2):
        check_point(_operand_desc(op, lo, dtype), mode, "direct", "fast", monkeypatch)
        check_point(_operand_desc(op, hi, dtype), mode, "staged", "fast", monkeypatch)


@pytest.mark.parametrize("op", ["A_kstrided", "B_kstrided"])
def test_weight_gradient_split_on_both_sides_of_both_limits(op, monkeypatch):
    """The weight-gradient layout (k rows = tokens): the automatic split is the 256-wide family's (72 slabs of the 2 tiles' 144 CUs)
    while that family is legal and the 128x128 family's (512 / 8 tiles = 64 slabs) above its limit; a split plan stays in the family
    of the unsplit one, and the last slab of split 3 begins beyond 2 GiB on the far side of the DIRECT limit."""
    _, _, ld, _ = OPERANDS[op]
    lo6, hi6 = rows_below(LIM_256, PAD_256, ld * 2), rows_at(LIM_256, PAD_256, ld * 2)
    lo, hi = rows_below(LIM_DIRECT, PAD_DIRECT, ld * 2), rows_at(LIM_DIRECT, PAD_DIRECT, ld * 2)
    for rows, family in ((lo6, "g256"), (hi6, "direct"), (lo, "direct"), (hi, "staged")):
        s = 72 if family == "g256" else 64
        check_point(_operand_desc(op, rows, L.XP_BF16), 2, family, "fast", monkeypatch, auto_split=s)
        for split in (3, s):
            check_point(_operand_desc(op, rows, L.XP_BF16), 2, family, "fast", monkeypatch, split=split)
    kps = _cdiv(_cdiv(hi, 3), 64) * 64
    assert 2 * kps * ld * 2 > 1 << 31


# ---------------------------------------------------------------------------------------------- C, resid, aux: the epilogue limit
def _epi_desc(which, M, dtype, out, ld=PITCH):
    kw = dict(C=dict(epi=L.EPI_BIAS, ldc=ld), C_none=dict(epi=L.EPI_NONE, ldc=ld),
              resid=dict(epi=L.EPI_BIAS_RESID, ldr=ld, resid=True), aux=dict(epi=L.EPI_BIAS_GELU, ldaux=ld, aux=True))[which]
    return desc(M, 128, 128, "nt", dtype, out, **kw)


@pytest.mark.parametrize("which", ["C", "C_none", "resid", "aux"])
def test_bf16_epilogue_operand_leaves_the_fast_epilogue_at_its_limit(which, monkeypatch):
    """(M + 256) rows of 2^20 bf16 elements below 0xFFFFFF00 - 64: the fast epilogue, and with XPRETRAIN_GEMM256=2 the 256-wide
    family, which has no other; from there on the generic 8-column epilogue of the 128x128 family"""
    lo, hi = rows_below(LIM_EPI, PAD_EPI, PITCH * 2), rows_at(LIM_EPI, PAD_EPI, PITCH * 2)
    assert (lo, hi) == (1791, 1792)
    for mode, family in ((2, "g256"), (0, "direct")):
        check_point(_epi_desc(which, lo, L.XP_BF16, L.XP_BF16), mode, family, "fast", monkeypatch)
        check_point(_epi_desc(which, hi, L.XP_BF16, L.XP_BF16), mode, "direct", "row8", monkeypatch)
    if which == "C_none":          # the fused column sums go with the family: a caller that sized 2 rows per tile gets none above
        d = _epi_desc(which, lo, L.XP_BF16, L.XP_BF16)
        monkeypatch.setenv("XPRETRAIN_GEMM256", "2")
        assert L.lib().xp_gemm_colsum_rows(C.byref(d)) == 2 * _cdiv(lo, 256) == 14
        assert L.lib().xp_gemm_colsum_rows(C.byref(_epi_desc(which, hi, L.XP_BF16, L.XP_BF16))) == 0


@pytest.mark.parametrize("dtype", [L.XP_BF16, L.XP_F32], ids=["bf16", "f32"])
def test_fp32_output_moves_the_epilogue_limit_with_its_element_size(dtype, monkeypatch):
    """fp32 C (the fast epilogue specialises EPI_NONE only): half the rows of the bf16 limit, from bf16 and from fp32 inputs"""
    lo, hi = rows_below(LIM_EPI, PAD_EPI, PITCH * 4), rows_at(LIM_EPI, PAD_EPI, PITCH * 4)
    assert (lo, hi) == (767, 768)
    g = "g256" if dtype == L.XP_BF16 else "direct"
    check_point(_epi_desc("C_none", lo, dtype, L.XP_F32), 2, g, "fast", monkeypatch)
    check_point(_epi_desc("C_none", hi, dtype, L.XP_F32), 2, "direct", "row8", monkeypatch)


@pytest.mark.parametrize("which", ["C", "resid", "aux"])
def test_fp32_epilogue_operands_have_no_fast_epilogue_to_leave(which, monkeypatch):
    """fp32 outputs with an epilogue kind other than EPI_NONE: the generic epilogue (64-bit row pointers) on both sides"""
    for esz_lim in (2, 4):
        for M in (rows_below(LIM_EPI, PAD_EPI, PITCH * esz_lim), rows_at(LIM_EPI, PAD_EPI, PITCH * esz_lim)):
            check_point(_epi_desc(which, M, L.XP_F32, L.XP_F32), 2, "direct", "row8", monkeypatch)


@pytest.mark.parametrize("which", ["C", "resid", "aux"])
def test_a_pitch_off_the_8_element_grid_is_row4_on_both_sides(which, monkeypatch):
    """fast -> row4 does not exist: a pitch with ld % 8 == 4 never had the fast epilogue, nor the 256-wide family"""
    ld = PITCH + 4
    for M in (rows_below(LIM_EPI, PAD_EPI, ld * 2), rows_at(LIM_EPI, PAD_EPI, ld * 2)):
        check_point(_epi_desc(which, M, L.XP_BF16, L.XP_BF16, ld=ld), 2, "direct", "row4", monkeypatch)


# ---------------------------------------------------------------------------------------------- refusals
def _attn_call(fn, S, ldqkv, ldo, dtype, mode=L.ATTN_CAUSAL, B=1, H=1, size=(0, 1, None)):
    """xp_attn_fwd / xp_attn_bwd2 with non-null dummy pointers: without a device an accepted call ends in XP_ERR_LAUNCH (-2), a
    refused one in XP_ERR_ARG (-1) before anything is launched"""
    lib, p = L.lib(), C.c_void_p(4096)
    M, N, Lp = size[0], size[1], (size[2] if size[2] is not None else S)
    ws = lib.xp_attn_workspace_bytes(mode, B, H, M, N, Lp)
    if fn == "fwd":
        return lib.xp_attn_fwd(p, ldqkv, p, ldo, p, None, mode, B, H, S, M, N, Lp, dtype, p, ws, None)
    return lib.xp_attn_bwd2(p, ldqkv, p, p, ldo, p, None, p, 1.0, mode, B, H, S, M, N, Lp, dtype, p, ws, None, None)


ATTN_SPAN = 0xFFFFFF00          # csrc/attention.hip::OOB: the offset its loaders use for "out of range"


@pytest.mark.parametrize("fn", ["fwd", "bwd"])
@pytest.mark.parametrize("operand", ["ldqkv", "ldo"])
def test_attention_refuses_a_sample_span_it_cannot_address(fn, operand):
    """bf16 attention reaches a sample's rows with 32-bit token * pitch offsets under a descriptor of S * ld * 2 bytes: refused from
    S * ld * 2 >= 4 GiB - 256 on, for ldqkv and for ldo, causal and proxy; accepted just below, at any batch size; fp32 mode, whose
    kernels use 64-bit pointers, accepts both.  (The accepted calls are made only where there is no device: with one they would launch
    on the dummy pointers.  tests/test_big_address_gpu.py runs accepted pitches on real buffers.)"""
    import torch
    lib, no_device = L.lib(), torch.cuda.device_count() == 0
    for mode, S, size in ((L.ATTN_CAUSAL, 16, (0, 1, None)), (L.ATTN_PROXY, 16, (1, 3, 5))):
        at = _cdiv(_cdiv(ATTN_SPAN, 2 * S), 8) * 8              # the smallest legal pitch (a multiple of 8) at or above the limit
        below = at - 8
        assert S * below * 2 < ATTN_SPAN <= S * at * 2 and S * at * 2 < 1 << 32
        for ld, rc in ((at, -1), (1 << 28, -1)) + (((below, -2),) if no_device else ()):
            ldqkv, ldo = (ld, 64) if operand == "ldqkv" else (192, ld)
            got = _attn_call(fn, S, ldqkv, ldo, L.XP_BF16, mode, B=33, size=size)
            assert got == rc, (mode, operand, ld, got, lib.xp_last_error())
            if rc == -1:
                msg = lib.xp_last_error()
                assert b"4 GiB" in msg and str(S * ld * 2).encode() in msg, msg
        ldqkv, ldo = (at, 64) if operand == "ldqkv" else (192, at)
        if no_device:
            assert _attn_call(fn, S, ldqkv, ldo, L.XP_F32, mode, B=33, size=size) == -2, lib.xp_last_error()
