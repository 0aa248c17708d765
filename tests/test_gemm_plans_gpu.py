"""GPU: every case of tests/gemm_cases.py -- each kernel variant the planner can choose -- against an fp64 reference of the same
operation on the kernel's own (bf16-rounded / fp32) inputs.

Per case: the plan is asserted through xp_debug_gemm_plan before the launch (the descriptor hip_ops.gemm builds); the output is held
to the tolerances of tests/test_gemm_gpu.py tensor-wide AND on the last tile row, the last tile column and the last k-slab alone; C,
aux, the split-K slabs, the column-sum partials and the fp32 side rows sit inside larger buffers filled with a sentinel bit pattern,
and nothing outside the outputs' windows may change.  Input padding (pitches, rows no remap reaches) holds a large finite value, so
a loader that reads it shows up as a wrong result.  Then: bit identity across the variants that must compute the same thing, the
split-K reduce, and the two split-K grids."""
import ctypes
import os
import zlib

import pytest
import torch

from tests import gemm_cases as G
from tests.gpu_util import OUT, report
from tests.guarded import _SENT, Guarded, _guarded_defer      # noqa: F401  (the guard helpers, shared with the workspace tests)
from tests.test_planning_cpu import case_budget, case_desc, check_plan, resolve_split, set_case_env

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f32": torch.float32}
TOL = {"bf16": 6e-3, "f32": 2e-5}           # tests/test_gemm_gpu.py: output rounding (bf16) / accumulation (fp32 output)
PAD_VALUE = 1000.0                          # input elements outside the operands' extents


def _remap(grp, stride, off, r):
    return r if grp == 0 else (r // grp) * stride + off + r % grp


def _operand(rows, K, ks, ld_pad, remap, dtype, scale, gen):
    """logical [rows][K] operand and its storage: [K'][ld] (k-strided) or [rows'][ld] with row remap, padding = PAD_VALUE"""
    idx = torch.arange(K if ks else rows, device="cuda")
    sidx = _remap(*remap, idx)
    ld = (rows if ks else K) + ld_pad
    store = torch.full((int(sidx[-1]) + 1, ld), PAD_VALUE, device="cuda")
    val = (torch.randn((rows, K), generator=gen, device="cuda") * scale).to(dtype)
    if ks:
        store[sidx, :rows] = val.t().float()
    else:
        store[sidx, :K] = val.float()
    return val, store.to(dtype).contiguous()


def _frames(c, gen):
    """a frame tensor and the patch matrix the loader gathers from it (bf16, rows (bt, gy, gx), k (c, dy, dx))"""
    BT, H, W, P, u8 = c["frames"]
    if u8:
        fr = torch.randint(0, 256, (BT, 3, H, W), generator=gen, device="cuda", dtype=torch.int32).to(torch.uint8)
        from xpretrain_amd import hip_ops as H_
        mean = torch.tensor(H_.CLIP_MEAN, device="cuda").view(1, 3, 1, 1)
        std = torch.tensor(H_.CLIP_STD, device="cuda").view(1, 3, 1, 1)
        x = (fr.float() / 255.0 - mean) / std
    else:
        fr = torch.randn((BT, 3, H, W), generator=gen, device="cuda")
        x = fr
    patches = x.unfold(2, P, P).unfold(3, P, P).permute(0, 2, 3, 1, 4, 5).reshape(-1, 3 * P * P)
    return fr, patches.to(torch.bfloat16)


def _maxrel(a, ref):
    """max|a - ref| / max|ref| on the GPU (the tensor-scale relative error of gpu_util.maxrel)"""
    a, ref = a.double(), ref.double()
    return ((a - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def _bad_columns(C, ref, tol, n=12):
    """the first columns whose error exceeds tol (relative to the tensor scale), for the failure message"""
    err = (C.double() - ref.double()).abs().max(0).values / ref.double().abs().max().clamp_min(1e-30)
    return (err > tol).nonzero().flatten()[:n].tolist()


def _edges_ok(tag, C, ref, plan, tol):
    """the last tile row and the last tile column alone: a wrong edge tile cannot hide behind the tensor-wide maximum"""
    tr = plan["tile_rows"]
    r0, c0 = (plan["tiles_m"] - 1) * tr, (plan["tiles_n"] - 1) * tr
    e_row = _maxrel(C[r0:], ref[r0:])
    e_col = _maxrel(C[:, c0:], ref[:, c0:])
    print(f"{tag}: last tile row {e_row:.2e} last tile column {e_col:.2e}")
    assert e_row <= tol and e_col <= tol, (tag, e_row, e_col)
    return max(e_row, e_col)


def _log(line):
    print(line)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "gemm_plan_errors.txt"), "a") as f:
        f.write(line + "\n")


def run_case(c, monkeypatch):
    """launch one case, check it; returns (output window, max error)"""
    from xpretrain_amd import _lib as L
    from xpretrain_amd import hip_ops as H
    set_case_env(c, monkeypatch)
    gen = torch.Generator(device="cuda").manual_seed(zlib.crc32(c["id"].encode()))
    M, N, K, pad = c["M"], c["N"], c["K"], c["pad"]
    aks, bks = G.LAYOUTS[c["layout"]]
    dt, ot = DT[c["dtype"]], DT[c["out"]]
    big = M * K > (1 << 22)
    s_in = 0.5 if dt == torch.bfloat16 else 1.0
    kw = dict(a_kstrided=bool(aks), b_kstrided=bool(bks), a_remap=c["a_remap"], c_remap=c["c_remap"], epilogue=G.EPIS.index(c["epi"]),
              out_dtype=ot)
    if c["frames"]:
        fr, Aval = _frames(c, gen)
        A = None
        kw.update(frames=fr, frame_patch=c["frames"][3])
        if c["frames"][4]:
            kw["frame_norm"] = (H.CLIP_MEAN, H.CLIP_STD)
    else:
        Aval, A = _operand(M, K, aks, pad.get("lda", 0), c["a_remap"], dt, s_in, gen)
        kw["lda"] = A.shape[1]
    Bval, B = _operand(N, K, bks, pad.get("ldb", 0), (0, 0, 0), dt, 0.2 if big else s_in, gen)
    kw["ldb"] = B.shape[1]
    crow = _remap(*c["c_remap"], torch.arange(M, device="cuda"))
    crows = int(crow[-1]) + 1
    acc = Aval.double() @ Bval.double().t()
    bias = torch.randn(N, generator=gen, device="cuda")
    ref, aux_ref, side_ref = acc, None, None
    epi = c["epi"]
    if epi in ("bias", "qscale", "gelu", "resid"):
        kw["bias"] = bias
        ref = acc + bias.double()
    if epi == "qscale":
        kw.update(scale=c["scale"], scale_cols=c["scale_cols"])
        cols = torch.arange(N, device="cuda")
        ref = ref * torch.where(cols < c["scale_cols"], c["scale"], 1.0).double()
    if epi == "scale":
        kw["scale"] = c["scale"]
        ref = acc * c["scale"]
    if epi == "gelu":
        aux_ref = ref
        ref = ref * torch.sigmoid(1.702 * ref)
        if c["aux"]:
            auxg = Guarded(crows, N + pad.get("ldaux", 0), ot)
            kw.update(aux=auxg.mat, ldaux=auxg.cols)
    if epi in ("resid", "gelu_bwd"):
        ldr = N + pad.get("ldr", 0)
        R = torch.full((crows, ldr), PAD_VALUE, device="cuda")
        R[crow, :N] = torch.randn((M, N), generator=gen, device="cuda")
        R = R.to(dt)
        kw.update(resid=R, ldr=ldr)
        r = R[crow, :N].double()
        if epi == "resid":
            ref = ref + r
        else:
            s = torch.sigmoid(1.702 * r)
            ref = acc * (s * (1 + 1.702 * r * (1 - s)))
    if epi == "resid" and c["side"]:
        S, Ms = c["side"]
        nb = (M + S - 1) // S
        rs = torch.randn((nb * Ms, N), generator=gen, device="cuda")
        sideg = Guarded(nb * Ms, N, torch.float32)
        m = torch.arange(M, device="cuda")
        is_side = (m % S) < Ms
        sidx = ((m // S) * Ms + m % S)[is_side]
        kw.update(resid_side=rs, out_side=sideg.mat, side=(S, Ms))
        ref = ref.clone()
        ref[is_side] = acc[is_side] + bias.double() + rs[sidx].double()
        side_ref = ref[is_side]
    if epi == "patch":
        T, Lp, Mp = c["patch"]
        tab1, tab2 = torch.randn((T, N), generator=gen, device="cuda"), torch.randn((Lp, N), generator=gen, device="cuda")
        kw.update(tab1=tab1, tab2=tab2, tab_L=Lp)
        w = torch.arange(M, device="cuda") % (T * Lp)
        ref = acc + tab1.double()[w // Lp] + tab2.double()[w % Lp]

    with case_budget(c):
        split = resolve_split(c, case_desc(c))
        kw["split_k"] = split
        if split > 1:
            slabs = Guarded(split * M, N, torch.float32)
            kw["out"] = slabs.mat.view(split, M, N)
        else:
            Cg = Guarded(crows, N + pad.get("ldc", 0), ot)
            kw.update(out=Cg.mat, ldc=Cg.cols)
        defer = None
        if c["colsum"]:
            cdesc = case_desc(c)
            cdesc.colsum_partials = 1
            nrows = L.lib().xp_gemm_colsum_rows(ctypes.byref(cdesc))
            defer = _guarded_defer(nrows, N)
            kw["colsum_defer"] = defer
        plan = H.gemm(A, B, M, N, K, plan_only=True, **kw)
        check_plan(c, plan, split)
        d = case_desc(c)
        d.split_k = split
        assert H.gemm_plan_of(d) == plan, (c["id"], "the case's descriptor plans differently from the launched one")
        res = H.gemm(A, B, M, N, K, **kw)
    tol = TOL[c["out"]]
    tag = f"plan {c['id']}"
    errs = []
    if split > 1:
        slabs.check(tag + " slabs", split * M, N)
        kps = plan["k_per_split"]
        for z in range(split):
            part = Aval[:, z * kps:(z + 1) * kps].double() @ Bval[:, z * kps:(z + 1) * kps].double().t()
            e = _maxrel(slabs.mat.view(split, M, N)[z], part)
            if z == split - 1:
                print(f"{tag}: last k-slab {e:.2e}")
            assert e <= tol, (tag, "slab", z, e)
            errs.append(e)
        out = Guarded(M, N, torch.float32)
        H.splitk_reduce(slabs.mat.view(split, M, N), out.mat)
        out.check(tag + " reduce", M, N)
        C = out.mat
    else:
        C = Cg.mat[crow, :N]
        Cg.check(tag, crow, N)
    errs.append(_maxrel(C, ref))
    assert errs[-1] <= tol, (tag, errs[-1], "wrong columns", _bad_columns(C, ref, tol))
    errs.append(_edges_ok(tag, C, ref, plan, tol))
    if aux_ref is not None and c["aux"]:
        auxg.check(tag + " aux", crow, N)
        e = _maxrel(auxg.mat[crow, :N], aux_ref)
        assert e <= tol, (tag, "aux", e)
        errs.append(e)
    if side_ref is not None:
        sideg.check(tag + " out_side", sidx, N)
        e = _maxrel(sideg.mat[sidx], side_ref)
        assert e <= 2e-5, (tag, "out_side", e)
        assert torch.equal(C[is_side], sideg.mat[sidx].to(ot))
    if defer is not None:
        cs = res[1]
        defer.flush()
        defer.guard.check(tag + " colsum partials", plan["colsum_rows"], N)
        e = _maxrel(cs, ref.sum(0))
        assert e <= 2e-3, (tag, "colsum", e)
    e = c["expect"]
    _log(f"{c['id']} {e['family']} {e['impl']} {c['dtype']}->{c['out']} split {split}: maxrel {max(errs):.3e} tol {tol:.0e}")
    return C, max(errs)


_FAST = [c for c in G.CASES if not c["step"]]
_STEP = [c for c in G.CASES if c["step"]]


@pytest.mark.parametrize("c", _FAST, ids=[c["id"] for c in _FAST])
def test_case(c, monkeypatch):
    run_case(c, monkeypatch)


@pytest.mark.parametrize("c", _STEP, ids=[c["id"] for c in _STEP])
def test_step_case(c, monkeypatch):
    """the training step's own GEMMs at BASELINE cfg #2 (18848 video rows, 256 text rows), bf16 and fp32 compute"""
    run_case(c, monkeypatch)


# ---------------------------------------------------------------------------------------------- bit identity across variants
def _run(A, B, M, N, K, monkeypatch, gemm256="0", debug="", **kw):
    from xpretrain_amd import hip_ops as H
    monkeypatch.setenv("XPRETRAIN_GEMM256", gemm256)
    monkeypatch.setenv("XPRETRAIN_DEBUG", debug)
    plan = H.gemm(A, B, M, N, K, plan_only=True, **kw)
    return H.gemm(A, B, M, N, K, **kw), plan


_IDENT = [("nt", 300, 264, 256), ("nn", 300, 256, 192), ("tn", 256, 256, 200), ("tk", 256, 136, 192)]


@pytest.mark.parametrize("layout,M,N,K", _IDENT)
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_direct_and_staged_loaders_are_bit_identical(layout, M, N, K, dtype, monkeypatch):
    """DIRECT (global -> LDS) and STAGED (through registers) loaders build the same LDS tile image: each output element sees the
    same mma16 sequence in the same k order, the same epilogue, the same rounding -- the outputs are equal"""
    aks, bks = G.LAYOUTS[layout]
    dt = DT[dtype]
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    A = (torch.randn((K, M) if aks else (M, K), generator=g, device="cuda") * 0.5).to(dt)
    B = (torch.randn((K, N) if bks else (N, K), generator=g, device="cuda") * 0.5).to(dt)
    kw = dict(a_kstrided=bool(aks), b_kstrided=bool(bks))
    for out in ((dt, torch.float32) if dt == torch.bfloat16 else (dt,)):
        d, pd = _run(A, B, M, N, K, monkeypatch, out_dtype=out, **kw)
        s, ps = _run(A, B, M, N, K, monkeypatch, debug="gemm_no_glds", out_dtype=out, **kw)
        assert (pd["family"], ps["family"]) == (G.FAMILIES.index("direct"), G.FAMILIES.index("staged"))
        assert torch.equal(d, s), f"{layout} {dtype}->{out}: max |direct - staged| = {(d.double() - s.double()).abs().max().item():.3e}"


@pytest.mark.parametrize("epi", ["none", "bias", "qscale", "gelu", "resid", "gelu_bwd"])
@pytest.mark.parametrize("loader", ["direct", "staged"])
def test_fast_and_generic_epilogues_are_bit_identical(epi, loader, monkeypatch):
    """the fast epilogue against the generic 8-column one (XPRETRAIN_DEBUG=gemm_slow_epi) and the generic 4-column one (an output
    pitch that is not a multiple of 8): same fp32 arithmetic, same bf16 rounding"""
    M, N, K = 300, 264, 192
    bf = torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(7)
    A = (torch.randn((M, K), generator=g, device="cuda") * 0.5).to(bf)
    B = (torch.randn((N, K), generator=g, device="cuda") * 0.5).to(bf)
    kw = dict(epilogue=G.EPIS.index(epi))
    if epi in ("bias", "qscale", "gelu", "resid"):
        kw["bias"] = torch.randn(N, generator=g, device="cuda")
    if epi == "qscale":
        kw.update(scale=0.125, scale_cols=130)
    if epi in ("resid", "gelu_bwd"):
        kw["resid"] = torch.randn((M, N), generator=g, device="cuda").to(bf)
    flags = "gemm_no_glds" if loader == "staged" else ""
    outs = {}
    for impl, extra, dbg in (("fast", {}, ""), ("row8", {}, "gemm_slow_epi"), ("row4", {"ldc": N + 4}, "")):
        C = torch.empty((M, extra.get("ldc", N)), dtype=bf, device="cuda")
        aux = torch.empty((M, N), dtype=bf, device="cuda") if epi == "gelu" else None
        o, plan = _run(A, B, M, N, K, monkeypatch, debug=",".join(f for f in (flags, dbg) if f), out=C, aux=aux, **extra, **kw)
        assert G.IMPLS[plan["epi_impl"]] == impl and G.FAMILIES[plan["family"]] == loader, plan
        outs[impl] = (C[:, :N].clone(), None if aux is None else aux.clone())
    for impl in ("row8", "row4"):
        for i, what in enumerate(("C", "aux")):
            a, b = outs["fast"][i], outs[impl][i]
            if a is None:
                continue
            assert torch.equal(a, b), f"{epi} {what}: fast vs {impl}: max diff {(a.double() - b.double()).abs().max().item():.3e}"


@pytest.mark.parametrize("layout,M,N,K", [("nt", 300, 264, 256), ("nn", 300, 256, 192), ("tn", 512, 256, 200), ("tk", 256, 264, 192)])
def test_256_and_128_families_agree(layout, M, N, K, monkeypatch):
    """the 256 family against the 128x128 family on problems both admit: they tile and stage differently, so by tolerance only"""
    aks, bks = G.LAYOUTS[layout]
    bf = torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(11)
    A = (torch.randn((K, M) if aks else (M, K), generator=g, device="cuda") * 0.5).to(bf)
    B = (torch.randn((K, N) if bks else (N, K), generator=g, device="cuda") * 0.5).to(bf)
    for out in (bf, torch.float32):
        kw = dict(a_kstrided=bool(aks), b_kstrided=bool(bks), out_dtype=out)
        c256, p256 = _run(A, B, M, N, K, monkeypatch, gemm256="2", **kw)
        c128, p128 = _run(A, B, M, N, K, monkeypatch, gemm256="0", **kw)
        assert (p256["tile_rows"], p128["tile_rows"]) == (256, 128)
        tol = TOL["bf16" if out == bf else "f32"]
        assert report(f"256 vs 128 {layout} {out}", c256, c128, tol) <= tol


# ---------------------------------------------------------------------------------------------- split-K reduce and grids
@pytest.mark.parametrize("splits,shape,accumulate", [(1, (300, 264), True), (4, (300, 264), False), (5, (3072, 3072), True),
                                                     (6, (300, 264), True), (7, (256, 512), False), (8, (64, 64), True)])
def test_splitk_reduce(splits, shape, accumulate):
    """xp_splitk_reduce: every residue of its 4-wide unroll, accumulate on / off, an output past one grid-stride pass
    (n / 4 > 8192 x 256); bit-identical to the same fp32 additions in the kernel's order, and nothing outside `out` written"""
    from xpretrain_amd import hip_ops as H
    g = torch.Generator(device="cuda").manual_seed(splits)
    M, N = shape
    slabs = torch.randn((splits, M, N), generator=g, device="cuda")
    out = Guarded(M, N, torch.float32)
    init = torch.randn((M, N), generator=g, device="cuda")
    out.mat.copy_(init)
    H.splitk_reduce(slabs, out.mat, accumulate=accumulate)
    out.check(f"splitk_reduce {splits}", M, N)
    s = init.clone() if accumulate else torch.zeros_like(init)
    z = 0
    while z + 4 <= splits:
        s = s + ((slabs[z] + slabs[z + 1]) + (slabs[z + 2] + slabs[z + 3]))
        z += 4
    while z < splits:
        s = s + slabs[z]
        z += 1
    assert torch.equal(out.mat, s)
    want = slabs.double().sum(0) + (init.double() if accumulate else 0)
    assert report(f"splitk_reduce {splits} acc={accumulate}", out.mat, want, 2e-6) <= 2e-6


_DW256 = [c for c in _STEP if c["layout"] == "tn" and c["expect"]["family"] == "g256" and c["expect"]["split"] > 1 and c["budget"] == 256]


@pytest.mark.parametrize("c", _DW256, ids=[c["id"] for c in _DW256])
def test_dw_tile_major_grid_is_bit_identical(c, monkeypatch):
    """the weight gradients' split-K slabs on the chunk-major 1-D grid (default) and on the (tile, z) grid (XPRETRAIN_DEBUG=
    dw_tile_major, read at every call) at the planner's splits: the grid changes which CU computes a slab, never the slab"""
    from xpretrain_amd import hip_ops as H
    M, N, K = c["M"], c["N"], c["K"]
    g = torch.Generator(device="cuda").manual_seed(M + N)
    Y = (torch.randn((K, M), generator=g, device="cuda") * 0.3).to(torch.bfloat16)
    X = (torch.randn((K, N), generator=g, device="cuda") * 0.3).to(torch.bfloat16)
    split = c["expect"]["split"]
    kw = dict(a_kstrided=True, b_kstrided=True, split_k=split)
    monkeypatch.delenv("XPRETRAIN_GEMM256", raising=False)
    monkeypatch.delenv("XPRETRAIN_DEBUG", raising=False)
    pc = H.gemm(Y, X, M, N, K, plan_only=True, **kw)
    chunk = H.gemm(Y, X, M, N, K, **kw)
    monkeypatch.setenv("XPRETRAIN_DEBUG", "dw_tile_major")
    pt = H.gemm(Y, X, M, N, K, plan_only=True, **kw)
    tile = H.gemm(Y, X, M, N, K, **kw)
    assert pc["flat_split"] == split and pt["flat_split"] == 0 and pt["grid"][2] == split
    assert torch.equal(chunk, tile)
