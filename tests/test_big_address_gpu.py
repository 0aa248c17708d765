"""GPU: every kernel's addressing where an operand crosses byte offsets 2^31 and 2^32 (tests/big_address.py).

Each address span is crossed with the smallest arithmetic that still crosses it: wide pitches make rows * ld large while the
problem stays tiny; an operand is dense only where the code path needs one (DIRECT and the 256-wide family need lda == K).  Every
case asserts the plan it means to run, the boundary rows (tests/big_address.py::boundary_rows) against fp64 at the bound of the
kernel's existing fp64 test, the guard of every output, and that the inputs are unchanged.  Where the same plan also serves a compact
copy of the same rows (the STAGED loader, the generic epilogues, every non-GEMM kernel) the two must agree bit for bit: an address
is not an operand of the arithmetic.  A wrapped 32-bit offset is an O(1) error, so no tolerance here is new:

  GEMM                 tests/test_gemm_plans_gpu.py::TOL (6e-3 bf16 / 2e-5 fp32 of the tensor scale), 2e-5 on fp32 side rows,
                       1e-5 of the stored output on the fused column sums (tests/test_attention_guarded_gpu.py)
  LayerNorm            tests/layernorm_ref.py: 64 u of the row scale (bf16 outputs: + 2^-8 |ref|), (rows + 8) u on column sums
  row reductions       bit-equal to the compact twin (tests/reduce_emulation.py fixes the order)
  attention            tests/test_attention_guarded_gpu.py::WHOLE (B = 33 / 17 is not a case of its CLASS_BOUNDS table)
  gather / scatter     exact

No case holds more than 14 GiB at once (asserted from the allocator's peak), and each gives back what it took."""
import gc

import pytest
import torch

from tests import attn_emulation as E
from tests import big_address as BA
from tests import layernorm_ref as R
from tests.guarded import Guarded, _guarded_defer
from tests.test_attention_gpu import F32 as K_F32
from tests.test_attention_gpu import FUSED, GENERAL, check_kernels
from tests.test_attention_guarded_gpu import WHOLE
from tests.test_big_address_planning_cpu import (ATTN_SPAN, LIM_256, LIM_DIRECT, LIM_EPI, PAD_256, PAD_DIRECT, PAD_EPI, PITCH, desc,
                                                 expected_auto_split, rows_at, rows_below)
from tests.test_gemm_plans_gpu import TOL as GEMM_TOL

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
NAME = {BF: "bf16", F32: "f32"}
ESZ = {BF: 2, F32: 4}
FAMILIES = ("g256", "direct", "staged", "frames")
IMPLS = ("fast", "row8", "row4")
GiB = 1 << 30


@pytest.fixture(autouse=True)
def _memory():
    """each case starts from an empty allocator, stays below 14 GiB and frees what it took"""
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    yield
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    gc.collect()
    torch.cuda.empty_cache()
    print(f"peak device memory of the case: {peak / GiB:.2f} GiB")
    assert peak <= 14 * GiB, f"the case held {peak / GiB:.2f} GiB at once"


def _cdiv(a, b):
    return -(-a // b)


def _maxrel(a, ref):
    a, ref = a.double(), ref.double()
    return ((a - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def _hold(tag, a, ref, tol):
    e = _maxrel(a, ref)
    print(f"{tag}: maxrel {e:.3e} tol {tol:.0e}")
    assert bool(torch.isfinite(a.double()).all()) and e <= tol, (tag, e, tol)


def _plan_is(plan, family, impl, split=1):
    got = (FAMILIES[plan["family"]], IMPLS[plan["epi_impl"]], plan["split"])
    assert got == (family, impl, split), (got, (family, impl, split))


def _env(monkeypatch, gemm256="2", debug=""):
    monkeypatch.setenv("XPRETRAIN_GEMM256", gemm256)
    monkeypatch.setenv("XPRETRAIN_DEBUG", debug)


# =============================================================================================== GEMM: C, resid, aux at a pitch of 2^20
def _m_points(osz):
    """M just below the fast-epilogue limit, the next tile up, and M * ldc * osz > 2^32 + one 128-row tile"""
    lo, hi = rows_below(LIM_EPI, PAD_EPI, PITCH * osz), rows_at(LIM_EPI, PAD_EPI, PITCH * osz)
    big = ((1 << 32) + 128 * PITCH * osz) // (PITCH * osz) + 1
    assert big * PITCH * osz > (1 << 32) + 128 * PITCH * osz
    return {"fast": lo, "row8": hi, "beyond4G": big}


EPI_CASES = [(epi, pt, BF, None) for epi in ("bias", "resid", "gelu") for pt in ("fast", "row8", "beyond4G")] + \
            [("resid", pt, BF, (60, 3)) for pt in ("fast", "beyond4G")] + \
            [("none", pt, F32, None) for pt in ("fast", "row8", "beyond4G")]


@pytest.mark.parametrize("epi,point,out_dt,side", EPI_CASES,
                         ids=[f"{e}-{p}-{NAME[o]}out{'-side' if s else ''}" for e, p, o, s in EPI_CASES])
def test_gemm_epilogue_operands_at_a_pitch_of_2_20(epi, point, out_dt, side, monkeypatch):
    """bf16 A [M, 128] x B [136, 128]; C -- and resid (pitched ldr, with and without fp32 side rows) or the kept pre-activation aux
    (pitched ldaux) -- at a row pitch of 2^20 elements: the fast epilogue (256-wide family) just below its limit, the generic 8-column
    epilogue (128x128 family) from there on and beyond 4 GiB; fp32 C from bf16 inputs, where the limits move with the element size"""
    from xpretrain_amd import _lib as L
    from xpretrain_amd import hip_ops as H
    N, K, osz = 136, 128, ESZ[out_dt]
    M = _m_points(osz)[point]
    tag = f"gemm {epi} {point} {NAME[out_dt]} out M={M}"
    seed = 1000 + M + len(epi)
    A, B = BA.Pitched(M, K, K, BF, seed, 0.5), BA.Pitched(N, K, K, BF, seed + 1, 0.5)
    g = torch.Generator(device="cuda").manual_seed(seed + 2)
    bias = torch.randn(N, generator=g, device="cuda")
    Cg = BA.BigGuarded(M, PITCH, out_dt)
    kind = {"none": L.EPI_NONE, "bias": L.EPI_BIAS, "resid": L.EPI_BIAS_RESID, "gelu": L.EPI_BIAS_GELU}[epi]
    kw = dict(out=Cg.mat, ldc=PITCH, out_dtype=out_dt, epilogue=kind)
    if epi != "none":
        kw["bias"] = bias
    resid = auxg = sideg = None
    if epi == "resid":
        resid = BA.Pitched(M, N, PITCH, BF, seed + 3)
        kw.update(resid=resid.mat, ldr=PITCH)
    if epi == "gelu":
        auxg = BA.BigGuarded(M, PITCH, out_dt)
        kw.update(aux=auxg.mat, ldaux=PITCH)
    if side:
        S, Ms = side
        nside = -(-M // S) * Ms
        rs = torch.randn((nside, N), generator=g, device="cuda")
        rs0 = rs.clone()
        sideg = BA.BigGuarded(nside, N, F32)
        kw.update(resid_side=rs, out_side=sideg.mat, side=side)
    _env(monkeypatch, "2")
    plan = H.gemm(A.mat, B.mat, M, N, K, plan_only=True, **kw)
    _plan_is(plan, *(("g256", "fast") if point == "fast" else ("direct", "row8")))
    assert BA.crossed(M, PITCH, osz) == ([31, 32] if point == "beyond4G" else [31])
    H.gemm(A.mat, B.mat, M, N, K, **kw)
    torch.cuda.synchronize()

    rows = BA.boundary_rows(M, PITCH, osz, 128, seed)
    acc = A.window(rows).double() @ B.mat.double().t()
    ref = acc + (bias.double() if epi != "none" else 0.0)
    if epi == "resid":
        ref = ref + resid.window(rows).double()
    if epi == "gelu":
        auxg.check(tag + " aux", M, N)
        _hold(tag + " aux", auxg.mat[rows, :N], ref, GEMM_TOL[NAME[out_dt]])
        ref = ref * torch.sigmoid(1.702 * ref)
    got = Cg.mat[rows, :N]
    if side:
        is_side = (rows % S) < Ms
        sidx = ((rows // S) * Ms + rows % S)[is_side]
        ref = ref.clone()
        ref[is_side] = acc[is_side] + bias.double() + rs[sidx].double()
        m = torch.arange(M, device="cuda")
        written = torch.zeros(nside, dtype=torch.bool, device="cuda")
        written[((m // S) * Ms + m % S)[(m % S) < Ms]] = True
        sideg.check(tag + " out_side", written, N)
        _hold(tag + " out_side", sideg.mat[sidx], ref[is_side], 2e-5)
        assert torch.equal(got[is_side], sideg.mat[sidx].to(out_dt)) and torch.equal(rs, rs0)
    Cg.check(tag, M, N)
    _hold(tag, got, ref, GEMM_TOL[NAME[out_dt]])
    for t, n in ((A, "A"), (B, "B"), (resid, "resid")):
        if t is not None:
            t.assert_unchanged(f"{tag} {n}")

    if point != "fast" and not side:          # the generic epilogue also serves the compact copy of the same rows: equal bits
        Mc = rows.numel()
        Ac = A.window(rows).contiguous()
        ckw = dict(out_dtype=out_dt, epilogue=kind, bias=kw.get("bias"))
        if epi == "resid":
            ckw["resid"] = resid.window(rows).contiguous()
        if epi == "gelu":
            ckw["aux"] = torch.empty((Mc, N), dtype=out_dt, device="cuda")
        _env(monkeypatch, "2", "gemm_slow_epi")
        _plan_is(H.gemm(Ac, B.mat, Mc, N, K, plan_only=True, **ckw), "direct", "row8")
        Cc = H.gemm(Ac, B.mat, Mc, N, K, **ckw)
        assert torch.equal(Cc, got), f"{tag}: the pitched rows differ from their compact twin"
        if epi == "gelu":
            assert torch.equal(ckw["aux"], auxg.mat[rows, :N]), f"{tag}: aux differs from its compact twin"


def test_gemm_fused_column_sums_just_below_the_limit(monkeypatch):
    """The 256-wide family's fused column sums with C at a pitch of 2^20, M just below the fast-epilogue limit: the partial rows lie
    in a guard, equal those of the compact twin bit for bit, give the fp64 column sums at the 2e-3 of tests/test_gemm_plans_gpu.py and
    the column sums of the STORED output at 1e-5, as the attention backward's do.

    The inputs are seeded randn rounded to integers (|a| <= 4): every output is an integer of magnitude far below 256, which bf16
    holds exactly, so the stored output IS the finished fp32 value and its column sums are what the partial rows must add up to.
    XpGemmDesc::colsum_partials sums the finished fp32 values BEFORE they are rounded to bf16 (include/xpretrain_hip.h; the attention
    kernels sum what they store): on inputs whose outputs bf16 rounds, the sums and the stored output differ by that rounding of
    1791 outputs per column (plain randn * 0.5: 1.30e-3 on the MI355X, pitched and compact alike, with the sums 9.0e-8 from fp64),
    which says nothing about an address.  A partial row that misses, repeats or misplaces a row of C is off by whole integers."""
    from xpretrain_amd import hip_ops as H
    N, K = 136, 128
    M = _m_points(2)["fast"]
    tag = f"gemm colsum M={M}"
    A, B = BA.Pitched(M, K, K, BF, 77, 0.7, grid=1.0), BA.Pitched(N, K, K, BF, 78, 0.7, grid=1.0)
    assert float(A.mat.abs().max()) <= 4 and float(B.mat.abs().max()) <= 4 and float(A.mat.abs().max()) >= 2
    Cg = BA.BigGuarded(M, PITCH, BF)
    _env(monkeypatch, "2")
    nrows = 2 * -(-M // 256)
    defer = _guarded_defer(nrows, N)
    kw = dict(out=Cg.mat, ldc=PITCH, colsum_defer=defer)
    plan = H.gemm(A.mat, B.mat, M, N, K, plan_only=True, **kw)
    _plan_is(plan, "g256", "fast")
    assert plan["colsum_rows"] == nrows
    _, cs = H.gemm(A.mat, B.mat, M, N, K, **kw)
    defer.flush()
    torch.cuda.synchronize()
    Cg.check(tag, M, N)
    defer.guard.check(tag + " partial rows", nrows, N)
    rows = BA.boundary_rows(M, PITCH, 2, 128, 77)
    _hold(tag, Cg.mat[rows, :N], A.window(rows).double() @ B.mat.double().t(), GEMM_TOL["bf16"])
    A.assert_unchanged(tag + " A")
    B.assert_unchanged(tag + " B")
    _hold(tag + " column sums vs fp64", cs, (A.mat.double() @ B.mat.double().t()).sum(0), 2e-3)
    twin = _guarded_defer(nrows, N)
    Cc, csc = H.gemm(A.mat, B.mat, M, N, K, colsum_defer=twin)
    twin.flush()
    torch.cuda.synchronize()
    assert torch.equal(Cc, Cg.mat[:, :N]) and torch.equal(twin.guard.mat, defer.guard.mat) and torch.equal(csc, cs), tag + ": differs from the compact twin"
    stored = Cg.mat[:, :N].double()
    assert float(stored.abs().max()) < 256 and torch.equal(stored, A.mat.double() @ B.mat.double().t())      # (the premise above)
    want = stored.sum(0)
    e = ((cs.double() - want).abs().max() / want.abs().max().clamp_min(1e-3)).item()
    print(f"{tag}: column sums vs the stored output {e:.3e} (bound 1e-5)")
    assert e <= 1e-5, (tag, "column sums vs the stored output", e)


# =============================================================================================== GEMM: dense k-contiguous A, K = 8192
def _dense_a_points():
    rb = 8192 * 2
    return {"g256": (rows_below(LIM_256, PAD_256, rb), BF, "g256"), "direct": (rows_at(LIM_256, PAD_256, rb), BF, "direct"),
            "direct-top": (rows_below(LIM_DIRECT, PAD_DIRECT, rb), BF, "direct"),
            "staged": (rows_at(LIM_DIRECT, PAD_DIRECT, rb), BF, "staged"), "staged-beyond4G": ((1 << 32) // rb + 129, BF, "staged"),
            "f32-direct-top": (rows_below(LIM_DIRECT, PAD_DIRECT, 2 * rb), F32, "direct"),
            "f32-staged": (rows_at(LIM_DIRECT, PAD_DIRECT, 2 * rb), F32, "staged")}


@pytest.mark.parametrize("point", list(_dense_a_points()))
def test_gemm_dense_a_on_both_sides_of_the_loader_limits(point, monkeypatch):
    """A [M, 8192] dense x B [128, 8192]: the 256-wide family just below its limit, DIRECT between the two limits and just below its
    own, the register-staged loader just above it and with M * K * 2 > 2^32; fp32 on both sides of the DIRECT limit.  The staged
    rows equal their compact twin bit for bit."""
    from xpretrain_amd import hip_ops as H
    M, dt, family = _dense_a_points()[point]
    N, K = 128, 8192
    tag = f"gemm dense A {point} M={M}"
    A, B = BA.Pitched(M, K, K, dt, 5 + M, 0.5), BA.Pitched(N, K, K, dt, 6 + M, 0.2)
    Cg = BA.BigGuarded(M, N, dt)
    _env(monkeypatch, "2")
    _plan_is(H.gemm(A.mat, B.mat, M, N, K, plan_only=True, out=Cg.mat), family, "fast")
    assert (32 in BA.crossed(M, K, ESZ[dt])) == (point == "staged-beyond4G")
    H.gemm(A.mat, B.mat, M, N, K, out=Cg.mat)
    torch.cuda.synchronize()
    Cg.check(tag, M, N)
    rows = BA.boundary_rows(M, K, ESZ[dt], 256, M)
    got = Cg.mat[rows]
    _hold(tag, got, A.window(rows).double() @ B.mat.double().t(), GEMM_TOL[NAME[dt]])
    A.assert_unchanged(tag + " A")
    B.assert_unchanged(tag + " B")
    if family == "staged":
        Ac = A.window(rows).contiguous()
        _env(monkeypatch, "0", "gemm_no_glds")          # (the compact copy is legal for DIRECT and the 256-wide family)
        _plan_is(H.gemm(Ac, B.mat, rows.numel(), N, K, plan_only=True), "staged", "fast")
        assert torch.equal(H.gemm(Ac, B.mat, rows.numel(), N, K), got), f"{tag}: rows differ from their compact twin"


# =============================================================================================== GEMM: padded and remapped operands
def test_gemm_padded_a_beyond_4_gib(monkeypatch):
    """lda = 2^20 + 8 with M * lda * 2 > 2^32: the register-staged loader; bit-equal to the compact twin"""
    from xpretrain_amd import hip_ops as H
    N, K, lda = 136, 128, PITCH + 8
    M = (1 << 32) // (lda * 2) + 130
    tag = f"gemm lda=2^20+8 M={M}"
    A, B = BA.Pitched(M, K, lda, BF, 91, 0.5), BA.Pitched(N, K, K, BF, 92, 0.5)
    assert BA.crossed(M, lda, 2) == [31, 32]
    Cg = BA.BigGuarded(M, N, BF)
    _env(monkeypatch, "2")
    _plan_is(H.gemm(A.mat, B.mat, M, N, K, lda=lda, plan_only=True, out=Cg.mat), "staged", "fast")
    H.gemm(A.mat, B.mat, M, N, K, lda=lda, out=Cg.mat)
    torch.cuda.synchronize()
    Cg.check(tag, M, N)
    rows = BA.boundary_rows(M, lda, 2, 128, 91)
    got = Cg.mat[rows]
    _hold(tag, got, A.window(rows).double() @ B.mat.double().t(), GEMM_TOL["bf16"])
    A.assert_unchanged(tag + " A")
    Ac = A.window(rows).contiguous()
    _env(monkeypatch, "0", "gemm_no_glds")
    _plan_is(H.gemm(Ac, B.mat, rows.numel(), N, K, plan_only=True), "staged", "fast")
    assert torch.equal(H.gemm(Ac, B.mat, rows.numel(), N, K), got), f"{tag}: rows differ from their compact twin"


@pytest.mark.parametrize("which", ["a_remap", "c_remap", "c_remap_patch"])
def test_gemm_row_remap_whose_last_group_lies_beyond_4_gib(which, monkeypatch):
    """three groups of 64 rows at a group stride of 2^23 + 64 rows of 128 bf16 elements: the last group begins beyond 4 GiB.  As
    a_remap (the register-staged loader gathers A's rows), as c_remap (the generic epilogue scatters C's rows) and as the PATCH
    epilogue's token slots (4 frames x 16 patches per sample, its two tables added); the rows between the groups hold PAD_VALUE /
    the guard pattern.  Bit-equal to the same problem at low addresses."""
    from xpretrain_amd import _lib as L
    from xpretrain_amd import hip_ops as H
    M, N, K, grp, stride, off = 192, 128, 128, 64, (1 << 23) + 64, 16
    store_rows = 2 * stride + off + grp
    assert store_rows * 128 * 2 > 1 << 32 and (2 * stride + off) * 128 * 2 > 1 << 32
    m = torch.arange(M, device="cuda")
    srow = (m // grp) * stride + off + m % grp
    tag = f"gemm {which}"
    extra = 0.0
    B = BA.Pitched(N, K, K, BF, 12, 0.5)
    dense = BA.Pitched(M, K, K, BF, 11, 0.5)
    _env(monkeypatch, "2")
    if which == "a_remap":
        A = torch.full((store_rows, K), BA.PAD_VALUE, dtype=BF, device="cuda")
        A[srow] = dense.mat
        Cg = BA.BigGuarded(M, N, BF)
        kw = dict(a_remap=(grp, stride, off), out=Cg.mat)
        _plan_is(H.gemm(A, B.mat, M, N, K, plan_only=True, **kw), "staged", "fast")
        H.gemm(A, B.mat, M, N, K, **kw)
        torch.cuda.synchronize()
        Cg.check(tag, M, N)
        got = Cg.mat
        assert torch.equal(A[srow], dense.mat), tag + ": A changed"
        A[srow] = BA.PAD_VALUE
        for r0 in range(0, store_rows, BA.CHUNK // K):
            assert bool((A[r0:r0 + BA.CHUNK // K] == BA.PAD_VALUE).all()), tag + ": A changed"
        _env(monkeypatch, "0", "gemm_no_glds")
        twin = dict()
    else:
        Cg = BA.BigGuarded(store_rows, N, BF)
        kw = dict(c_remap=(grp, stride, off), out=Cg.mat, out_rows=store_rows)
        if which == "c_remap_patch":
            g = torch.Generator(device="cuda").manual_seed(13)
            tab1, tab2 = torch.randn((4, N), generator=g, device="cuda"), torch.randn((16, N), generator=g, device="cuda")
            patch = dict(epilogue=L.EPI_PATCH, tab1=tab1, tab2=tab2, tab_L=16)
            kw.update(patch)
            extra = tab1.double()[(m % grp) // 16] + tab2.double()[(m % grp) % 16]
        _plan_is(H.gemm(dense.mat, B.mat, M, N, K, plan_only=True, **kw), "direct", "row8")
        H.gemm(dense.mat, B.mat, M, N, K, **kw)
        torch.cuda.synchronize()
        written = torch.zeros(store_rows, dtype=torch.bool, device="cuda")
        written[srow] = True
        Cg.check(tag, written, N)
        got = Cg.mat[srow]
        _env(monkeypatch, "2", "gemm_slow_epi")
        twin = dict(c_remap=(grp, grp, 0), **patch) if which == "c_remap_patch" else dict()      # (PATCH takes its table row from m % grp)
    _hold(tag, got, dense.mat.double() @ B.mat.double().t() + extra, GEMM_TOL["bf16"])
    dense.assert_unchanged(tag + " A")
    B.assert_unchanged(tag + " B")
    want = ("staged", "fast") if which == "a_remap" else ("direct", "row8")
    _plan_is(H.gemm(dense.mat, B.mat, M, N, K, plan_only=True, **twin), *want)
    assert torch.equal(H.gemm(dense.mat, B.mat, M, N, K, **twin), got), f"{tag}: differs from the un-remapped problem"


def test_gemm_weight_gradient_a_remap_whose_last_group_lies_beyond_4_gib(monkeypatch):
    """the patch-embedding dW form: A stored [k-rows][256] (k-strided) with its 192 k-rows in three groups of 64 at a group stride of
    2^22 + 64 rows of 512 bytes, the last group beyond 4 GiB, PAD_VALUE between the groups; B [192][256] dense, fp32 out.  The
    register-staged loader gathers the k-rows; bit-equal to the un-remapped problem."""
    from xpretrain_amd import hip_ops as H
    M, N, K, grp, stride, off = 256, 256, 192, 64, (1 << 22) + 64, 16
    store_rows = 2 * stride + off + grp
    assert (2 * stride + off) * M * 2 > 1 << 32
    k = torch.arange(K, device="cuda")
    srow = (k // grp) * stride + off + k % grp
    tag = "gemm tn a_remap"
    dense, B = BA.Pitched(K, M, M, BF, 15, 0.5), BA.Pitched(K, N, N, BF, 16, 0.5)
    A = torch.full((store_rows, M), BA.PAD_VALUE, dtype=BF, device="cuda")
    A[srow] = dense.mat
    Cg = BA.BigGuarded(M, N, F32)
    lay = dict(a_kstrided=True, b_kstrided=True, out_dtype=F32)
    _env(monkeypatch, "2")
    _plan_is(H.gemm(A, B.mat, M, N, K, plan_only=True, a_remap=(grp, stride, off), out=Cg.mat, **lay), "staged", "fast")
    H.gemm(A, B.mat, M, N, K, a_remap=(grp, stride, off), out=Cg.mat, **lay)
    torch.cuda.synchronize()
    Cg.check(tag, M, N)
    _hold(tag, Cg.mat, dense.mat.double().t() @ B.mat.double(), GEMM_TOL["f32"])
    assert torch.equal(A[srow], dense.mat), tag + ": A changed"
    A[srow] = BA.PAD_VALUE
    for r0 in range(0, store_rows, BA.CHUNK // M):
        assert bool((A[r0:r0 + BA.CHUNK // M] == BA.PAD_VALUE).all()), tag + ": A changed"
    dense.assert_unchanged(tag + " A")
    B.assert_unchanged(tag + " B")
    _env(monkeypatch, "0", "gemm_no_glds")
    _plan_is(H.gemm(dense.mat, B.mat, M, N, K, plan_only=True, **lay), "staged", "fast")
    assert torch.equal(H.gemm(dense.mat, B.mat, M, N, K, **lay), Cg.mat), f"{tag}: differs from the un-remapped problem"


# =============================================================================================== GEMM: the weight-gradient layout
def _tn_points():
    rb = 256 * 2
    return {"g256": (rows_below(LIM_256, PAD_256, rb), "g256"), "direct": (rows_at(LIM_256, PAD_256, rb), "direct"),
            "direct-top": (rows_below(LIM_DIRECT, PAD_DIRECT, rb), "direct"), "staged": (rows_at(LIM_DIRECT, PAD_DIRECT, rb), "staged")}


@pytest.mark.parametrize("point", list(_tn_points()))
def test_gemm_weight_gradient_k_rows_on_both_sides_of_the_loader_limits(point, monkeypatch):
    """dW [256, 256] fp32 = Y^T X with Y, X [K, 256] bf16 dense (both k-strided), K rows on each side of both loader limits: split 3
    -- the last slab begins beyond 2 GiB -- and the automatic split, each slab set reduced by xp_splitk_reduce and held to the fp64
    product, which is summed on the device in row chunks.

    The inputs are seeded randn on a grid of 1/8: every product is a multiple of 1/64 and every partial sum of the 7.9 M-term dot
    products (|sum| < 2^18) is exact in fp32, whatever the order.  The 2e-5 of tests/test_gemm_plans_gpu.py belongs to accumulations
    of at most 18 848 terms; with plain randn a slab of 2.4 M terms (split 3) lands at 2.05e-5 .. 2.35e-5 on the MI355X from the
    rounding of its fp32 accumulator alone.  On the grid the same bound measures the addresses and nothing else."""
    from xpretrain_amd import hip_ops as H
    from xpretrain_amd import _lib as L
    K, family = _tn_points()[point]
    M = N = 256
    auto = expected_auto_split(desc(M, N, K, "tn", L.XP_BF16, L.XP_F32), 2)          # (the restated rules of the CPU planning test)
    assert auto > 3
    tag = f"gemm tn {point} K={K}"
    Y, X = BA.Pitched(K, M, M, BF, 21, 0.5, grid=0.125), BA.Pitched(K, N, N, BF, 22, 0.5, grid=0.125)
    _env(monkeypatch, "2")
    assert H.gemm_auto_split(M, N, K, BF) == auto
    ref = torch.zeros((M, N), dtype=torch.float64, device="cuda")
    step = 1 << 19
    for k0 in range(0, K, step):
        ref += Y.mat[k0:k0 + step].double().t() @ X.mat[k0:k0 + step].double()
    for split in (3, auto):
        slabs = BA.BigGuarded(split * M, N, F32)
        kw = dict(a_kstrided=True, b_kstrided=True, split_k=split, out=slabs.mat.view(split, M, N))
        plan = H.gemm(Y.mat, X.mat, M, N, K, plan_only=True, **kw)
        _plan_is(plan, family, "fast", split)
        if split == 3:
            assert 2 * plan["k_per_split"] * M * 2 > 1 << 31
        H.gemm(Y.mat, X.mat, M, N, K, **kw)
        out = Guarded(M, N, F32)
        H.splitk_reduce(slabs.mat.view(split, M, N), out.mat)
        torch.cuda.synchronize()
        slabs.check(f"{tag} split {split} slabs", split * M, N)
        out.check(f"{tag} split {split} reduce", M, N)
        _hold(f"{tag} split {split}", out.mat, ref, GEMM_TOL["f32"])
        del slabs, out
    Y.assert_unchanged(tag + " Y")
    X.assert_unchanged(tag + " X")


# =============================================================================================== LayerNorm
def _ln_hold(tag, out, ref, scale, gate, bf16=False, axis=1):
    m, i = R.worst(out, ref, scale, bf16, axis)
    g = gate * (1.01 if bf16 else 1.0)
    print(f"{tag}: {m:.3g} u (gate {g:.4g} u) at {i}")
    assert m <= g, (tag, m, g, i)


LN_LD = {BF: 59_000_000, F32: 29_500_000}          # 37 rows of either: 4.37 GB, so row 18 holds byte 2^31 and row 36 byte 2^32


@pytest.mark.parametrize("side", [None, (8, 1, 1)], ids=["plain", "side"])
@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
def test_layernorm_37_rows_across_4_gib(dt, side, monkeypatch):
    """xp_layernorm_fwd / _bwd (and their _side forms) on 37 rows of 768 columns at ldx = ldy = lddy = lddx with rows * ld * esz > 2^32:
    every row against the fp64 definition at the gates of tests/layernorm_ref.py, and bit-equal to the same rows at ld = 768"""
    from xpretrain_amd import hip_ops as H
    rows, cols, ld = 37, 768, LN_LD[dt]
    assert BA.crossed(rows, ld, ESZ[dt]) == [31, 32]
    tag = f"layernorm {NAME[dt]} 37x768 ld={ld}{' side' if side else ''}"
    x = BA.Pitched(rows, cols, ld, dt, 31, 1.0)
    g = torch.Generator(device="cuda").manual_seed(32)
    gamma = 1 + 0.3 * torch.randn(cols, generator=g, device="cuda")
    beta = 0.1 * torch.randn(cols, generator=g, device="cuda")
    skw, x_side = {}, None
    x_read = x.mat[:, :cols].double()
    if side:
        S, Ms, stride = side
        r = torch.arange(rows, device="cuda")
        is_side, sidx = (r % S) < Ms, (r // S) * stride + r % S
        x_side = torch.randn((-(-rows // S) * stride, cols), generator=g, device="cuda")
        x_read = x_read.clone()
        x_read[is_side] = x_side[sidx[is_side]].double()
        skw = dict(x_side=x_side, side=side)
    yg = BA.BigGuarded(rows, ld, dt)
    mg, rg = Guarded(1, rows, F32), Guarded(1, rows, F32)
    H.layernorm_fwd(x.mat, gamma, beta, rows, cols, ldx=ld, ldy=ld, y=yg.mat, mean=mg.mat, rstd=rg.mat, **skw)
    torch.cuda.synchronize()
    yg.check(tag + " y", rows, cols)
    mg.check(tag + " mean", 1, rows)
    rg.check(tag + " rstd", 1, rows)
    bf = dt == BF
    ref = R.ref_fwd(x_read, gamma, beta, 1e-5)
    mean, rstd = mg.mat[0].clone(), rg.mat[0].clone()
    _ln_hold(tag + " y", yg.mat[:, :cols], ref["y"], ref["scale_y"], R.GATE_ROW, bf)
    _ln_hold(tag + " mean", mean[:, None], ref["mean"][:, None], ref["scale_mean"], R.GATE_ROW)
    _ln_hold(tag + " rstd", rstd[:, None], ref["rstd"][:, None], ref["rstd"], R.GATE_ROW)
    xc = x.mat[:, :cols].contiguous()
    yc, mc, rc = H.layernorm_fwd(xc, gamma, beta, rows, cols, **skw)
    assert torch.equal(yc, yg.mat[:, :cols]) and torch.equal(mc, mean) and torch.equal(rc, rstd), tag + ": forward differs from its compact twin"
    del yg
    torch.cuda.empty_cache()

    dy = BA.Pitched(rows, cols, ld, dt, 33, 1.0)
    dres = (torch.randn((rows, cols), generator=g, device="cuda")).to(dt)
    dxg = BA.BigGuarded(rows, ld, dt)
    dg, db = torch.full((cols,), 3.0, device="cuda"), torch.full((cols,), 3.0, device="cuda")
    H.layernorm_bwd(dy.mat, x.mat, gamma, mean, rstd, rows, cols, ldx=ld, lddy=ld, dres=dres, dx=dxg.mat, lddx=ld, dgamma=dg, dbeta=db,
                    **skw)
    torch.cuda.synchronize()
    dxg.check(tag + " dx", rows, cols)
    rb = R.ref_bwd(dy.mat[:, :cols].double(), x_read, gamma, mean, rstd, dres)
    _ln_hold(tag + " dx", dxg.mat[:, :cols], rb["dx"], rb["scale_dx"], R.GATE_ROW, bf)
    _ln_hold(tag + " dgamma", dg, rb["dgamma"], rb["scale_dgamma"], R.col_gate(rows), axis=0)
    _ln_hold(tag + " dbeta", db, rb["dbeta"], rb["scale_dbeta"], R.col_gate(rows), axis=0)
    dxc, dgc, dbc = H.layernorm_bwd(dy.mat[:, :cols].contiguous(), xc, gamma, mean, rstd, rows, cols, dres=dres, **skw)
    assert torch.equal(dxc, dxg.mat[:, :cols]) and torch.equal(dgc, dg) and torch.equal(dbc, db), tag + ": backward differs from its compact twin"
    x.assert_unchanged(tag + " x")
    dy.assert_unchanged(tag + " dy")


def test_layernorm_dense_4_3_gb_bf16():
    """2 796 300 x 768 bf16, dense (4.3 GB per operand): the boundary rows of y, mean, rstd and dx against the fp64 definition at the
    row gates; dgamma / dbeta against fp64 sums over all rows, computed on the device in row chunks, at the column-sum gate"""
    from xpretrain_amd import hip_ops as H
    rows, cols = 2_796_300, 768
    assert BA.crossed(rows, cols, 2) == [31, 32]
    tag = "layernorm bf16 2796300x768"
    x = BA.Pitched(rows, cols, cols, BF, 41, 1.0)
    g = torch.Generator(device="cuda").manual_seed(42)
    gamma = 1 + 0.3 * torch.randn(cols, generator=g, device="cuda")
    beta = 0.1 * torch.randn(cols, generator=g, device="cuda")
    pick = BA.boundary_rows(rows, cols, 2, 64, 41)
    yg = BA.BigGuarded(rows, cols, BF)
    mg, rg = Guarded(1, rows, F32), Guarded(1, rows, F32)
    H.layernorm_fwd(x.mat, gamma, beta, rows, cols, y=yg.mat, mean=mg.mat, rstd=rg.mat)
    torch.cuda.synchronize()
    yg.check(tag + " y", rows, cols)
    mg.check(tag + " mean", 1, rows)
    rg.check(tag + " rstd", 1, rows)
    mean, rstd = mg.mat[0].clone(), rg.mat[0].clone()
    assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(rstd).all())
    ref = R.ref_fwd(x.mat[pick].double(), gamma, beta, 1e-5)
    _ln_hold(tag + " y", yg.mat[pick], ref["y"], ref["scale_y"], R.GATE_ROW, True)
    _ln_hold(tag + " mean", mean[pick][:, None], ref["mean"][:, None], ref["scale_mean"], R.GATE_ROW)
    _ln_hold(tag + " rstd", rstd[pick][:, None], ref["rstd"][:, None], ref["rstd"], R.GATE_ROW)
    yc, mc, rc = H.layernorm_fwd(x.mat[pick].contiguous(), gamma, beta, pick.numel(), cols)
    assert torch.equal(yc, yg.mat[pick]) and torch.equal(mc, mean[pick]) and torch.equal(rc, rstd[pick]), tag + ": rows differ from their compact twin"
    del yg, mg, rg
    torch.cuda.empty_cache()

    dy = BA.Pitched(rows, cols, cols, BF, 43, 1.0)
    dxg = BA.BigGuarded(rows, cols, BF)
    dg, db = torch.full((cols,), 3.0, device="cuda"), torch.full((cols,), 3.0, device="cuda")
    H.layernorm_bwd(dy.mat, x.mat, gamma, mean, rstd, rows, cols, dx=dxg.mat, dgamma=dg, dbeta=db)
    torch.cuda.synchronize()
    dxg.check(tag + " dx", rows, cols)
    rb = R.ref_bwd(dy.mat[pick].double(), x.mat[pick].double(), gamma, mean[pick], rstd[pick], None)
    _ln_hold(tag + " dx", dxg.mat[pick], rb["dx"], rb["scale_dx"], R.GATE_ROW, True)
    sums = {n: torch.zeros(cols, dtype=torch.float64, device="cuda") for n in ("dgamma", "dbeta", "scale_dgamma", "scale_dbeta")}
    step = 1 << 14
    for r0 in range(0, rows, step):
        sl = slice(r0, r0 + step)
        d = dy.mat[sl].double()
        t = d * ((x.mat[sl].double() - mean[sl].double()[:, None]) * rstd[sl].double()[:, None])
        sums["dgamma"] += t.sum(0)
        sums["scale_dgamma"] += t.abs().sum(0)
        sums["dbeta"] += d.sum(0)
        sums["scale_dbeta"] += d.abs().sum(0)
    _ln_hold(tag + " dgamma", dg, sums["dgamma"], sums["scale_dgamma"], R.col_gate(rows), axis=0)
    _ln_hold(tag + " dbeta", db, sums["dbeta"], sums["scale_dbeta"], R.col_gate(rows), axis=0)
    x.assert_unchanged(tag + " x")
    dy.assert_unchanged(tag + " dy")


# =============================================================================================== row reductions
@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
def test_column_sums_of_a_pitched_matrix_across_4_gib(dt):
    """xp_colsum and xp_colsum_partials + flush on X [rows, 768] at a pitch of 2^20 with rows * ldx * esz > 2^32: bit-equal to the
    compact twin (the summation order is a function of rows and cols alone), and within (rows + 8) u of the fp64 sums"""
    from xpretrain_amd import hip_ops as H
    cols, esz = 768, ESZ[dt]
    rows = (1 << 32) // (PITCH * esz) + 130
    assert BA.crossed(rows, PITCH, esz) == [31, 32]
    tag = f"colsum {NAME[dt]} {rows}x{cols} ldx=2^20"
    X = BA.Pitched(rows, cols, PITCH, dt, 51, 1.0)
    Xc = X.mat[:, :cols].contiguous()
    a = H.colsum(X.mat, rows, cols, ldx=PITCH)
    b = H.colsum(Xc, rows, cols)
    d1, d2 = H.DeferredReduce(torch.device("cuda")), H.DeferredReduce(torch.device("cuda"))
    pa = H.colsum_deferred(X.mat, rows, cols, d1, ldx=PITCH, name="pitched")
    d1.flush()
    pb = H.colsum_deferred(Xc, rows, cols, d2, name="compact")
    d2.flush()
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(pa, pb), tag + ": differs from the compact twin"
    want, scale = Xc.double().sum(0), Xc.double().abs().sum(0)
    _ln_hold(tag + " xp_colsum", a, want, scale, R.col_gate(rows), axis=0)
    _ln_hold(tag + " partials + flush", pa, want, scale, R.col_gate(rows), axis=0)
    X.assert_unchanged(tag)


# =============================================================================================== dense attention
ATTN = {"proxy1x3x5": ((1, 3, 5), 16), "causal16": (None, 16)}
LDQKV, LDO = 1 << 22, 1 << 21


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("case", list(ATTN))
def test_attention_samples_128_mib_apart(case, dt, monkeypatch):
    """xp_attn_fwd / xp_attn_bwd2, H = 1, S = 16, ldqkv = 2^22 and ldo = 2^21 elements: every sample of qkv / dqkv spans 128 MiB
    (bf16), the 33 samples 4.1 GiB -- sample 16 begins at byte 2^31, sample 32 at 2^32.  fp32 runs 17 samples (its elements are
    twice as wide: 4.25 GiB, and the 14 GiB cap on the four big operands allows no more).  out, dqkv, stats and the column-sum
    partial rows sit in guards; every sample is held to the fp64 cores at WHOLE and equals its compact twin bit for bit."""
    from xpretrain_amd import _lib as L
    from xpretrain_amd import hip_ops as Hh
    monkeypatch.delenv("XPRETRAIN_DEBUG", raising=False)
    size, S = ATTN[case]
    B, H, D = (33 if dt == BF else 17), 1, 64
    rows = B * S
    assert BA.crossed(rows, LDQKV, ESZ[dt]) == [31, 32] and S * LDQKV * ESZ[dt] < ATTN_SPAN
    amode = L.ATTN_PROXY if size is not None else L.ATTN_CAUSAL
    M, N, Lp = size if size is not None else (0, 1, S)
    kernels = K_F32 if dt == F32 else (FUSED if size is not None else GENERAL)
    check_kernels(kernels, B, S, H, size=size, dtype=dt)
    tag = f"attn {case} {NAME[dt]} B={B} ldqkv=2^22 ldo=2^21"
    qkv, dout = BA.Pitched(rows, 3 * D, LDQKV, dt, 61, 1.0), BA.Pitched(rows, D, LDO, dt, 62, 1.0)
    lib, dtc, dev = L.lib(), Hh._dt(qkv.mat), qkv.mat.device
    nrows = int(lib.xp_attn_bwd_colsum_rows(amode, B, H, S, M, N, Lp, dtc))
    ws_bytes = int(lib.xp_attn_workspace_bytes(amode, B, H, M, N, Lp))

    def run(qkv_t, ldq, dout_t, ldo, out_t, dqkv_t, stats_t, cs_t):
        ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=dev)
        L.check(lib.xp_attn_fwd(Hh._p(qkv_t), ldq, Hh._p(out_t), ldo, Hh._p(stats_t), None, amode, B, H, S, M, N, Lp, dtc,
                                Hh._p(ws), ws_bytes, Hh._stream()), "xp_attn_fwd")
        L.check(lib.xp_attn_bwd2(Hh._p(qkv_t), ldq, Hh._p(out_t), Hh._p(dout_t), ldo, Hh._p(stats_t), None, Hh._p(dqkv_t), E.Q_SCALE,
                                 amode, B, H, S, M, N, Lp, dtc, Hh._p(ws), ws_bytes, Hh._p(cs_t), Hh._stream()), "xp_attn_bwd2")
        torch.cuda.synchronize()

    out_g, dqkv_g = BA.BigGuarded(rows, LDO, dt), BA.BigGuarded(rows, LDQKV, dt)
    stats_g = Guarded(B * H * S, 2, F32)
    cs_g = Guarded(nrows, 3 * D, F32) if nrows else None
    run(qkv.mat, LDQKV, dout.mat, LDO, out_g.mat, dqkv_g.mat, stats_g.mat, cs_g.mat if nrows else None)
    out_g.check(tag + " out", rows, D)
    dqkv_g.check(tag + " dqkv", rows, 3 * D)
    stats_g.check(tag + " stats", B * H * S, 2)
    if nrows:
        cs_g.check(tag + " colsum partial rows", nrows, 3 * D)
        want = dqkv_g.mat[:, :3 * D].double().sum(0)
        e = ((cs_g.mat[:nrows].double().sum(0) - want).abs().max() / want.abs().max().clamp_min(1e-3)).item()
        assert e <= 1e-5, (tag, "colsum vs stored", e)
    qkv.assert_unchanged(tag + " qkv")
    dout.assert_unchanged(tag + " dout")

    qc, dc = qkv.mat[:, :3 * D].contiguous(), dout.mat[:, :D].contiguous()
    q, k, v = E.split_heads(qc, B, S, H)
    ref = E.reference(q, k, v, dc.view(B, S, H, 64).double().transpose(1, 2), size, None)
    got = {"out": out_g.mat[:, :D]}
    for j, n in enumerate(("dq", "dk", "dv")):
        got[n] = dqkv_g.mat[:, j * D:(j + 1) * D]
    tf, tb = WHOLE["bf16" if dt == BF else "fp32"]
    for n, t in got.items():
        want = ref[n].transpose(1, 2).reshape(rows, D)
        tol = tf if n == "out" else tb
        _hold(f"{tag} {n}", t, want, tol)
    lse = stats_g.mat.view(B, H, S, 2).double().sum(-1)
    e_lse = (lse - ref["lse"]).abs().max().item()
    assert e_lse <= 1e-3, (tag, "lse", e_lse)

    out_c, dqkv_c = torch.empty((rows, D), dtype=dt, device=dev), torch.empty((rows, 3 * D), dtype=dt, device=dev)
    stats_c = torch.empty((B * H * S, 2), dtype=F32, device=dev)
    cs_c = torch.empty((nrows, 3 * D), dtype=F32, device=dev) if nrows else None
    run(qc, 3 * D, dc, D, out_c, dqkv_c, stats_c, cs_c)
    assert torch.equal(out_c, got["out"]) and torch.equal(dqkv_c, dqkv_g.mat[:, :3 * D]), tag + ": differs from the compact twin"
    assert torch.equal(stats_c, stats_g.mat[:B * H * S]) and (not nrows or torch.equal(cs_c, cs_g.mat[:nrows])), tag + ": stats / column sums differ"


# =============================================================================================== single-query attention
POOLED_LD = {BF: 33_000_000, F32: 16_500_000}       # 66 rows of either: 4.36 GB


@pytest.mark.parametrize("regime", ["peaked", "flat"])
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_single_query_attention_kv_rows_across_4_gib(dt, regime):
    """xp_attn_pooled_fwd / _bwd on the existing case B2H2S33 (its own seeded inputs, reference and CLASS_BOUNDS entries, lse bound
    and 1e-5 on the column sums of the stored dkv) with kv and dkv at a row pitch where B * S * ldkv * esz > 2^32: sample 1 begins at
    2.2 GB and ends beyond 4 GiB.  Bit-equal to the same call at the dense pitch."""
    from tests import attn_pooled_emulation as PE
    from tests.test_attention_pooled_guarded_gpu import CLASS_BOUNDS as POOLED_BOUNDS
    from xpretrain_amd import _lib as L
    from xpretrain_amd import hip_ops as Hh
    case, dtype = "B2H2S33", PE.DT[dt]
    B, H, S = PE.CASES[case]
    D, ld = H * 64, POOLED_LD[dtype]
    assert BA.crossed(B * S, ld, ESZ[dtype]) == [31, 32]
    tag = f"attn_pooled {dt} {case} {regime} ldkv={ld}"
    q_c, kv_c, dout_c = PE.inputs(case, regime, dtype)
    q, dout = q_c.cuda().contiguous(), dout_c.cuda().contiguous()
    q0, dout0 = q.clone(), dout.clone()
    kv = BA.Pitched(B * S, 2 * D, ld, dtype, values=kv_c)
    lib, dtc, dev = L.lib(), Hh._dt(q), q.device
    nrows = int(lib.xp_attn_pooled_colsum_rows(B, H, S, dtc))
    ws_bytes = int(lib.xp_attn_pooled_workspace_bytes(B, H, S, dtc))
    plans = [Hh.attn_pooled_plan(B, S, H, dtype=dtype, backward=b) for b in (False, True)]
    assert nrows == B * plans[1]["chunks"] > 0

    def run(kv_t, ldkv, dkv_t, lddkv):
        out_g, stats_g, dq_g = Guarded(B, D, dtype), Guarded(B * H, 2, F32), Guarded(B, D, dtype)
        cs_g = Guarded(nrows, 2 * D, F32)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        L.check(lib.xp_attn_pooled_fwd(Hh._p(q), Hh._p(kv_t), ldkv, Hh._p(out_g.mat), Hh._p(stats_g.mat), B, H, S, dtc, Hh._p(ws), ws_bytes,
                                       Hh._stream()), "xp_attn_pooled_fwd")
        L.check(lib.xp_attn_pooled_bwd(Hh._p(q), Hh._p(kv_t), ldkv, Hh._p(out_g.mat), Hh._p(dout), Hh._p(stats_g.mat), Hh._p(dq_g.mat), D,
                                       Hh._p(dkv_t), lddkv, PE.Q_SCALE, B, H, S, dtc, Hh._p(ws), ws_bytes, Hh._p(cs_g.mat), Hh._stream()),
                "xp_attn_pooled_bwd")
        torch.cuda.synchronize()
        for gd, n, r, c in ((out_g, "out", B, D), (stats_g, "stats", B * H, 2), (dq_g, "dq", B, D), (cs_g, "colsum partial rows", nrows, 2 * D)):
            gd.check(f"{tag} {n}", r, c)
        return out_g.mat, stats_g.mat, dq_g.mat, cs_g.mat[:nrows]

    dkv_g = BA.BigGuarded(B * S, ld, dtype)
    out, stats, dq, cs = run(kv.mat, ld, dkv_g.mat, ld)
    dkv_g.check(tag + " dkv", B * S, 2 * D)
    kv.assert_unchanged(tag + " kv")
    assert torch.equal(q, q0) and torch.equal(dout, dout0), tag + ": an input changed"
    dkv = dkv_g.mat[:, :2 * D]
    dk, dv = dkv.reshape(B, S, 2, H, 64).unbind(2)
    got = {"out": out.view(B, H, 64), "dq": dq.reshape(B, H, 64), "dk": dk, "dv": dv, "stats": stats.view(B, H, 2)}
    got = {n: t.cpu().contiguous() for n, t in got.items()}
    assert all(bool(torch.isfinite(t.float()).all()) for t in got.values()), tag + ": not finite"
    ref = PE.case_reference(case, regime, dtype)
    bounds, errs = POOLED_BOUNDS[(dt, case, regime)], PE.class_errors(got, ref, regime)
    assert set(errs) == set(bounds)
    for key, (_, bound) in bounds.items():
        print(f"{tag} {key}: {errs[key]:.3e} bound {bound:.1e}")
        assert errs[key] <= bound, (tag, key, errs[key], bound)
    e_lse = (got["stats"].double().sum(-1) - ref["lse"]).abs().max().item()
    assert e_lse <= PE.lse_bound(S), (tag, "lse", e_lse)
    want = dkv.double().sum(0)
    e_cs = ((cs.double().sum(0) - want).abs().max() / want.abs().max().clamp_min(1e-3)).item()
    assert e_cs <= 1e-5, (tag, "colsum vs stored", e_cs)
    dkv_c = torch.empty((B * S, 2 * D), dtype=dtype, device=dev)
    twin = run(kv.mat[:, :2 * D].contiguous(), 2 * D, dkv_c, 2 * D)
    assert all(torch.equal(a, b) for a, b in zip(twin, (out, stats, dq, cs))) and torch.equal(dkv_c, dkv), tag + ": differs from the compact twin"


# =============================================================================================== gather / scatter
def test_gather_and_scatter_rows_beyond_2_31_elements():
    """xp_gather_rows / xp_scatter_rows at B * S * D = 2^31 + one row (bf16, 4 GiB + 1 KiB): the gathered rows are the indexed ones;
    the scattered gradient holds dout at the indexed token of every sample and zero everywhere else (checked in chunks)"""
    from xpretrain_amd import hip_ops as H
    S, D = 5, 512
    B = ((1 << 31) // D + 1) // S
    assert B * S * D == (1 << 31) + D
    g = torch.Generator(device="cuda").manual_seed(71)
    idx = torch.randint(0, S, (B,), generator=g, device="cuda")
    idx[0], idx[-1] = 0, S - 1                       # the first and the last row of the operand
    idx0 = idx.clone()
    x = BA.Pitched(B * S, D, D, BF, 72, 1.0)
    out = H.gather_rows(x.mat, idx, B, S, D)
    torch.cuda.synchronize()
    src = torch.arange(B, device="cuda") * S + idx
    step = 1 << 17
    for b0 in range(0, B, step):
        assert torch.equal(out[b0:b0 + step], x.mat[src[b0:b0 + step]]), f"gather: samples {b0}.. wrong"
    x.assert_unchanged("gather x")
    del x
    torch.cuda.empty_cache()
    dx = H.scatter_rows(out, idx, B, S, D)
    torch.cuda.synchronize()
    for b0 in range(0, B, step):
        assert torch.equal(dx[src[b0:b0 + step]], out[b0:b0 + step]), f"scatter: samples {b0}.. wrong"
    nz = 0
    for r0 in range(0, B * S, BA.CHUNK // D):
        nz += int((dx[r0:r0 + BA.CHUNK // D].view(torch.int16) != 0).any(1).sum())
    assert nz <= B and nz == int((out.view(torch.int16) != 0).any(1).sum()), "scatter: rows other than the indexed ones are not zero"
    assert torch.equal(idx, idx0)


# =============================================================================================== refusals, with real buffers
@pytest.mark.parametrize("fn", ["fwd", "bwd"])
@pytest.mark.parametrize("operand", ["ldqkv", "ldo"])
def test_attention_refusal_leaves_real_buffers_untouched(fn, operand):
    """bf16 attention with S * ld * 2 = 4 GiB - 256 (the first span refused), every buffer really of that size: XP_ERR_ARG, a message
    that names the limit, and no output element changed"""
    from xpretrain_amd import _lib as L
    from xpretrain_amd import hip_ops as Hh
    S, D = 16, 64
    at = _cdiv(_cdiv(ATTN_SPAN, 2 * S), 8) * 8
    assert S * at * 2 >= ATTN_SPAN and S * (at - 8) * 2 < ATTN_SPAN
    ldq, ldo = (at, D) if operand == "ldqkv" else (3 * D, at)
    lib = L.lib()
    qkv = torch.zeros((S, ldq), dtype=BF, device="cuda")
    out_g, stats_g = BA.BigGuarded(S, ldo, BF), Guarded(S, 2, F32)
    ws_bytes = int(lib.xp_attn_workspace_bytes(L.ATTN_CAUSAL, 1, 1, 0, 1, S))
    ws_g = Guarded(1, max(ws_bytes // 4, 64), F32)
    guards = [out_g, stats_g, ws_g]
    if fn == "fwd":
        rc = lib.xp_attn_fwd(Hh._p(qkv), ldq, Hh._p(out_g.mat), ldo, Hh._p(stats_g.mat), None, L.ATTN_CAUSAL, 1, 1, S, 0, 1, S, L.XP_BF16,
                             Hh._p(ws_g.mat), ws_bytes, Hh._stream())
    else:
        dout = torch.zeros((S, ldo), dtype=BF, device="cuda")
        dqkv_g = BA.BigGuarded(S, ldq, BF)
        guards.append(dqkv_g)
        rc = lib.xp_attn_bwd2(Hh._p(qkv), ldq, Hh._p(out_g.mat), Hh._p(dout), ldo, Hh._p(stats_g.mat), None, Hh._p(dqkv_g.mat), 0.125,
                              L.ATTN_CAUSAL, 1, 1, S, 0, 1, S, L.XP_BF16, Hh._p(ws_g.mat), ws_bytes, None, Hh._stream())
    assert rc == -1 and b"4 GiB" in lib.xp_last_error(), (rc, lib.xp_last_error())
    torch.cuda.synchronize()
    for gd in guards:
        gd.check(f"refused attention {fn} {operand}", 0, 0)
