"""The GEMM case table: every kernel variant the planner (csrc/gemm.hip::plan_gemm) can choose, as plain data.

No imports of the package and nothing that touches the GPU: tests/test_planning_cpu.py checks on the CPU that every case gets the
plan it declares (and that the table covers every (variant, layout, epilogue kind, epilogue implementation, output dtype) the
planner produces), tests/test_gemm_plans_gpu.py runs the cases against fp64.

A case is a dict:
  id                     unique name (the pytest id)
  M, N, K                problem size; layout: "nt" (A [M][K], B [N][K]), "nn" (B stored [K][N]), "tn" (both stored [K][row]),
                         "tk" (A stored [K][M], B [N][K])
  dtype, out             input / output dtype: "bf16" or "f32"
  epi                    epilogue kind (EPIS); aux (BIAS_GELU keeps the pre-activation), side = (S, Ms) (BIAS_RESID fp32 side rows),
                         scale, scale_cols (BIAS_QSCALE / SCALE), patch = (T, Lp, Mp) (PATCH: C rows remapped into token slots)
  pad                    extra elements per row beyond the extent: {"lda", "ldb", "ldc", "ldr", "ldaux"}
  a_remap, c_remap       (grp, stride, off) row remaps of A's m index (its k-rows when k-strided) and of the output rows
  frames                 (BT, H, W, P, u8): A gathered from a frame tensor (the patch embedding without im2col); K = 3 P^2
  colsum                 the fused column sums of the outputs (bias gradient), written as partial rows
  split                  k slabs: an int, or "general" / "slack" (ask xp_gemm_auto_split / _slack)
  gemm256, debug, budget the environment: XPRETRAIN_GEMM256 (None: unset), XPRETRAIN_DEBUG flags, xp_set_cu_budget
  expect                 the plan: {"family", "impl", "split"} (split: what "general" / "slack" must resolve to)
"""

LAYOUTS = {"nt": (0, 0), "nn": (0, 1), "tn": (1, 1), "tk": (1, 0)}      # (a_kstrided, b_kstrided)
EPIS = ("none", "bias", "qscale", "gelu", "resid", "gelu_bwd", "patch", "scale")    # index = XP_EPI_*
FAMILIES = ("g256", "direct", "staged", "frames")                                     # index = XP_GEMM_FAMILY_*
IMPLS = ("fast", "row8", "row4")                                                      # index = XP_GEMM_EPI_*
TILE_ROWS = {"g256": 256, "direct": 128, "staged": 128, "frames": 128}


def case(cid, M, N, K, layout="nt", *, dtype="bf16", out=None, epi="none", aux=False, side=None, scale=0.125, scale_cols=0,
         pad=None, a_remap=(0, 0, 0), c_remap=(0, 0, 0), patch=None, frames=None, colsum=False, split=1, gemm256=None, debug=(),
         budget=256, family, impl, expect_split=None, step=False):
    assert layout in LAYOUTS and epi in EPIS and family in FAMILIES and impl in IMPLS
    if patch is not None:
        T, Lp, Mp = patch
        c_remap = (T * Lp, Mp + T * Lp, Mp)
    return dict(id=cid, M=M, N=N, K=K, layout=layout, dtype=dtype, out=out or dtype, epi=epi, aux=aux, side=side, scale=scale,
                scale_cols=scale_cols, pad=dict(pad or {}), a_remap=tuple(a_remap), c_remap=tuple(c_remap), patch=patch,
                frames=frames, colsum=colsum, split=split, gemm256=gemm256, debug=tuple(debug), budget=budget,
                expect=dict(family=family, impl=impl, split=expect_split if expect_split is not None else split), step=step)


def _fast_specialised(epi, out):
    """csrc/gemm_common.h::fast_epi_specialised without column sums"""
    return epi == "none" if out == "f32" else EPIS.index(epi) <= EPIS.index("gelu_bwd")


def _epi_args(epi, i):
    """operands of an epilogue kind; i varies the optional parts (aux, scale_cols) over the cases"""
    if epi == "gelu":
        return dict(aux=i % 2 == 0)
    if epi == "qscale":
        return dict(scale_cols=(0, 256, 136, 130, 100000)[i % 5])
    if epi == "scale":
        return dict(scale=3.0)
    if epi == "patch":
        return dict(patch=(2, 5, 3))
    return {}


# ------------------------------------------------------------------------- variant x layout x epilogue x implementation x dtype
def _matrix():
    cases, n = [], 0
    for family in ("g256", "direct", "staged"):
        for layout, (aks, bks) in LAYOUTS.items():
            dts = (("bf16", "bf16"), ("bf16", "f32")) if family == "g256" else (("bf16", "bf16"), ("bf16", "f32"), ("f32", "f32"))
            for dtype, out in dts:
                for epi in EPIS:
                    for impl in IMPLS:
                        fast_ok = _fast_specialised(epi, out)
                        if impl == "fast" and not fast_ok:
                            continue
                        if family == "g256" and impl != "fast":
                            continue
                        if epi == "patch" and impl == "fast":
                            continue
                        n += 1
                        kw = _epi_args(epi, n)
                        pad, debug = {}, []
                        ke = 64 if dtype == "bf16" else 32
                        # shapes the variant admits: the 256 family needs whole 64-deep k-tiles of k-contiguous operands and
                        # 256-multiples of k-strided row extents, DIRECT whole k-tiles and 128-multiples
                        if family == "g256":
                            M = 512 if aks else 300
                            N = 512 if bks else 264
                            K = 192 if not (aks and bks) else 200
                        else:
                            M = 256 if aks else 200
                            N = 256 if bks else 136
                            K = 3 * ke if not (aks and bks) else 77
                        if impl == "row8" and fast_ok:
                            # a kind the fast epilogue has, sent to the generic one: the debug switch, or a row-remapped output
                            if n % 2 and epi != "resid" or kw.get("patch"):
                                debug.append("gemm_slow_epi")
                            else:
                                kw["c_remap"] = (64, 96, 16)
                        if impl == "row4":
                            # not 8 columns per lane: N % 8 == 4 where the layout allows it, else a pitch that is not a multiple of 8
                            if not bks and family == "staged" and n % 2:
                                N = 132
                            elif epi in ("resid", "gelu_bwd") and n % 3 == 0:
                                pad["ldr"] = 4
                            elif epi == "gelu" and kw.get("aux"):
                                pad["ldaux"] = 4
                            else:
                                pad["ldc"] = 4
                        a_remap = (0, 0, 0)
                        if family == "staged":
                            # the register-staged loader: forced by the switch, or what DIRECT cannot take (ragged k, a padded
                            # pitch, a remapped A)
                            why = n % 4
                            if why == 0:
                                debug.append("gemm_no_glds")
                            elif why == 1:
                                if aks and bks:
                                    M = 200
                                else:
                                    K = 200
                            elif why == 2:
                                pad["lda"] = 8
                            else:
                                a_remap = (40, 56, 8) if aks else (64, 80, 16)
                        gemm256 = 2 if family == "g256" else (None if n % 3 else 0)
                        cases.append(case(f"{family}-{layout}-{dtype}{out}-{epi}-{impl}-{n}", M, N, K, layout, dtype=dtype, out=out,
                                          epi=epi, pad=pad, a_remap=a_remap, debug=debug, gemm256=gemm256, family=family, impl=impl,
                                          **kw))
    return cases


# ------------------------------------------------------------------------- edges
def _edges():
    c = []
    g = dict(gemm256=2)
    # M: 1, a tile minus / plus one, ragged
    for M in (1, 127, 129, 383):
        c.append(case(f"edge-M{M}-direct", M, 256, 128, family="direct", impl="fast", epi="bias"))
    for M in (255, 257, 700):
        c.append(case(f"edge-M{M}-g256", M, 256, 128, family="g256", impl="fast", epi="resid", **g))
    c.append(case("edge-M1-staged-f32", 1, 132, 200, dtype="f32", family="staged", impl="row4"))
    # N: 4, 12, a tile -+ 8
    for N, impl in ((4, "row4"), (12, "row4"), (120, "fast"), (136, "fast")):
        c.append(case(f"edge-N{N}", 200, N, 128, family="direct", impl=impl, epi="qscale", scale_cols=N // 2 + 2))
    for N in (248, 264):
        c.append(case(f"edge-N{N}-g256", 300, N, 128, family="g256", impl="fast", epi="gelu", aux=True, **g))
    # K of k-contiguous operands: 8, 56, 200 (ragged k-tiles: register-staged), a multiple of 64
    for K, fam in ((8, "staged"), (56, "staged"), (200, "staged"), (320, "direct")):
        c.append(case(f"edge-K{K}-nt", 130, 136, K, family=fam, impl="fast"))
        c.append(case(f"edge-K{K}-nt-f32", 130, 136, K, dtype="f32", family="staged" if K % 32 else "direct", impl="fast"))
    c.append(case("edge-K56-nn", 130, 256, 56, "nn", family="staged", impl="fast", epi="gelu_bwd"))
    # K of k-strided operands (dW over a few rows: the projections' weight gradients have K = batch): 1, 2, 8, 77
    for K in (1, 2, 8, 77):
        c.append(case(f"edge-K{K}-tn", 128, 256, K, "tn", out="f32", family="direct", impl="fast"))
        c.append(case(f"edge-K{K}-tn-staged", 136, 264, K, "tn", out="f32", family="staged", impl="fast"))
        c.append(case(f"edge-K{K}-tn-f32", 136, 128, K, "tn", dtype="f32", family="staged", impl="fast"))
    c.append(case("edge-K72-tk", 256, 136, 72, "tk", family="staged", impl="fast", epi="bias"))
    # pitches larger than the extents
    c.append(case("edge-ld-all", 200, 136, 128, family="staged", impl="fast", epi="resid",
                  pad=dict(lda=64, ldb=8, ldc=16, ldr=24)))
    c.append(case("edge-ld-gelu-aux", 200, 136, 128, family="direct", impl="fast", epi="gelu", aux=True, pad=dict(ldc=8, ldaux=40)))
    c.append(case("edge-ld-tn", 200, 136, 300, "tn", out="f32", family="staged", impl="fast", pad=dict(lda=8, ldb=16, ldc=8)))
    # EPI_BIAS_QSCALE's scale_cols: 0, a multiple of 256, 136, 130 (not a multiple of 4: the per-column rule), > N -- every variant
    for sc in (0, 256, 136, 130, 514):
        c.append(case(f"qscale-{sc}-g256", 300, 512, 128, epi="qscale", scale_cols=sc, family="g256", impl="fast", **g))
        c.append(case(f"qscale-{sc}-direct", 300, 512, 128, epi="qscale", scale_cols=sc, family="direct", impl="fast"))
        c.append(case(f"qscale-{sc}-row8", 300, 512, 128, epi="qscale", scale_cols=sc, family="direct", impl="row8",
                      debug=["gemm_slow_epi"]))
        c.append(case(f"qscale-{sc}-row4", 300, 508, 128, epi="qscale", scale_cols=sc, family="direct", impl="row4"))
    # BIAS_RESID with fp32 side rows on each implementation
    c.append(case("side-g256", 600, 256, 128, epi="resid", side=(50, 3), family="g256", impl="fast", **g))
    c.append(case("side-direct", 600, 256, 128, epi="resid", side=(50, 3), family="direct", impl="fast"))
    c.append(case("side-row8", 600, 256, 128, epi="resid", side=(50, 3), family="direct", impl="row8", debug=["gemm_slow_epi"]))
    c.append(case("side-staged-all-rows", 200, 136, 200, epi="resid", side=(1, 1), family="staged", impl="fast"))
    # SCALE with bf16 and fp32 output
    c.append(case("scale-bf16", 200, 136, 128, epi="scale", scale=3.0, family="direct", impl="row8"))
    c.append(case("scale-f32out", 200, 136, 128, epi="scale", scale=3.0, out="f32", family="direct", impl="row8"))
    # a_remap of a k-contiguous A; the patch-embedding weight gradient (a_remap of a k-strided A with split-K)
    c.append(case("aremap-kc", 100, 136, 128, a_remap=(30, 50, 7), family="staged", impl="fast", epi="bias"))
    c.append(case("aremap-ks-split", 128, 256, 1000, "tn", out="f32", a_remap=(90, 100, 4), split=3, family="staged", impl="fast"))
    # frame gather (patch embedding without im2col): fp32 and uint8 frames, PATCH into token slots, other epilogues
    c.append(case("frames-patch", 2 * 4 * 4, 136, 3 * 16 * 16, frames=(2, 64, 64, 16, 0), epi="patch", patch=(2, 16, 3),
                  family="frames", impl="row8"))
    c.append(case("frames-u8-bias", 3 * 4 * 8, 256, 3 * 16 * 16, frames=(3, 64, 128, 16, 1), epi="bias",
                  family="frames", impl="fast"))
    c.append(case("frames-f32out", 2 * 9, 132, 3 * 8 * 8, frames=(2, 24, 24, 8, 0), out="f32", family="frames", impl="row4"))
    # split-K slabs: every residue of the reduce's 4-wide unroll, each family
    for s in (2, 3, 4, 5):
        c.append(case(f"splitk-{s}-g256", 256, 512, 192 * s - 40, "tn", out="f32", split=s, family="g256", impl="fast", **g))
        c.append(case(f"splitk-{s}-direct", 256, 256, 256 * s - 56, "tn", out="f32", split=s, family="direct", impl="fast"))
        c.append(case(f"splitk-{s}-f32", 136, 128, 700, "tn", dtype="f32", split=s, family="staged", impl="fast"))
    c.append(case("splitk-nt", 300, 264, 640, "nt", out="f32", split=3, family="direct", impl="fast"))
    return c


# ------------------------------------------------------------------------- the training step's GEMMs, BASELINE cfg #2
VIDEO = dict(rows=8 * 2356, D=768, Dff=3072, S=2356, Mp=4, T=12, Lp=196, P=16)
TEXT = dict(rows=8 * 32, D=512, Dff=2048)
BATCH = 8

# the plan of every step GEMM: family per (tower, compute dtype, pass); dW splits (general, slack) per budget
_DW_SPLITS = {      # (dtype, M, N, K) -> {budget: (general, slack)}
    ("bf16", 768, 3072, 18848): {256: (4, 3), 128: (3, 3)},
    ("bf16", 3072, 768, 18848): {256: (4, 3), 128: (3, 3)},
    ("bf16", 768, 768, 18848): {256: (16, 12), 128: (14, 12)},
    ("bf16", 2304, 768, 18848): {256: (5, 4), 128: (4, 4)},
    ("bf16", 512, 2048, 256): {256: (1, 1), 128: (1, 1)},
    ("bf16", 2048, 512, 256): {256: (1, 1), 128: (1, 1)},
    ("bf16", 512, 512, 256): {256: (1, 1), 128: (1, 1)},
    ("bf16", 1536, 512, 256): {256: (1, 1), 128: (1, 1)},
    ("f32", 768, 3072, 18848): {256: (3, 3), 128: (3, 3)},
    ("f32", 3072, 768, 18848): {256: (3, 3), 128: (3, 3)},
    ("f32", 768, 768, 18848): {256: (14, 14), 128: (14, 14)},
    ("f32", 2304, 768, 18848): {256: (4, 4), 128: (4, 4)},
    ("f32", 512, 2048, 256): {256: (1, 1), 128: (1, 1)},
    ("f32", 2048, 512, 256): {256: (1, 1), 128: (1, 1)},
    ("f32", 512, 512, 256): {256: (1, 1), 128: (1, 1)},
    ("f32", 1536, 512, 256): {256: (1, 1), 128: (1, 1)},
}


def _step():
    c = []
    for dt in ("bf16", "f32"):
        bf = dt == "bf16"
        for tower, d in (("video", VIDEO), ("text", TEXT)):
            R, D, F = d["rows"], d["D"], d["Dff"]
            video = tower == "video"
            # forward: 256 family for the bf16 video tower; 128x128 (direct-to-LDS) for the text tower and fp32
            fam = "g256" if bf and video else "direct"
            fx = lambda epi: "fast" if _fast_specialised(epi, dt) else "row8"        # (fp32 compute: fp32 out, fast only after NONE)
            side = ((d["S"], d["Mp"]) if video else (1, 1)) if bf else None
            t = f"step-{dt}-{tower}"
            c.append(case(f"{t}-qkv", R, 3 * D, D, dtype=dt, epi="qscale", scale=0.125, scale_cols=D, family=fam, impl=fx("qscale"), step=True))
            c.append(case(f"{t}-out", R, D, D, dtype=dt, epi="resid", side=side, family=fam, impl=fx("resid"), step=True))
            c.append(case(f"{t}-fc1", R, F, D, dtype=dt, epi="gelu", aux=True, family=fam, impl=fx("gelu"), step=True))
            c.append(case(f"{t}-fc2", R, D, F, dtype=dt, epi="resid", side=side, family=fam, impl=fx("resid"), step=True))
            # dX (B read k-strided); fc1's bias gradient from the epilogue where the plan has it (256 family)
            c.append(case(f"{t}-dpre", R, F, D, "nn", dtype=dt, epi="gelu_bwd", colsum=bf and video, family=fam, impl=fx("gelu_bwd"), step=True))
            c.append(case(f"{t}-dh2", R, D, F, "nn", dtype=dt, family=fam, impl="fast", step=True))
            c.append(case(f"{t}-dattn", R, D, D, "nn", dtype=dt, family=fam, impl="fast", step=True))
            c.append(case(f"{t}-dh1", R, D, 3 * D, "nn", dtype=dt, family=fam, impl="fast", step=True))
            # dW at the planner's splits: the 256 family takes the video tower's bf16 split-K, 128x128 everything else
            for name, M, N in (("dw2", D, F), ("dw1", F, D), ("dwo", D, D), ("dwqkv", 3 * D, D)):
                for budget in (256, 128):
                    for which, s in zip(("general", "slack"), _DW_SPLITS[(dt, M, N, R)][budget]):
                        fam_w = "g256" if bf and video else "direct"
                        c.append(case(f"{t}-{name}-{which}-cu{budget}", M, N, R, "tn", dtype=dt, out="f32", split=which, budget=budget,
                                      family=fam_w, impl="fast", expect_split=s, step=True))
        # patch embedding: forward into the token slots (materialised patches; the frame gather when no weight gradient is
        # wanted), dW with the token rows remapped onto the patch rows
        v = VIDEO
        P, T, Lp, Mp, S = v["P"], v["T"], v["Lp"], v["Mp"], v["S"]
        Rp, K = BATCH * T * Lp, 3 * P * P
        c.append(case(f"step-{dt}-patch-fwd", Rp, v["D"], K, dtype=dt, epi="patch", patch=(T, Lp, Mp), family="direct", impl="row8",
                      step=True))
        if bf:
            c.append(case("step-bf16-patch-fwd-frames", Rp, v["D"], K, epi="patch", patch=(T, Lp, Mp), frames=(BATCH * T, 224, 224, P, 1),
                          family="frames", impl="row8", step=True))
        c.append(case(f"step-{dt}-patch-dw", v["D"], K, Rp, "tn", dtype=dt, out="f32", a_remap=(T * Lp, S, Mp), split="general",
                      family="staged", impl="fast", expect_split=14, step=True))
        # projections (bias-free Linear on the pooled features: BATCH rows): forward, dX, dW with K = BATCH
        for tower, Din in (("visual", VIDEO["D"]), ("text", TEXT["D"])):
            c.append(case(f"step-{dt}-proj-{tower}-fwd", BATCH, 512, Din, dtype=dt, family="direct", impl="fast", step=True))
            c.append(case(f"step-{dt}-proj-{tower}-dx", BATCH, Din, 512, "nn", dtype=dt, family="direct", impl="fast", step=True))
            c.append(case(f"step-{dt}-proj-{tower}-dw", 512, Din, BATCH, "tn", dtype=dt, out="f32", split="general", family="direct",
                          impl="fast", expect_split=1, step=True))
    return c


def desc_fields(c):
    """XpGemmDesc fields of a case for the planning queries (no data: pointers are 1 where the planner reads their presence, the
    operands 0); tests/test_gemm_plans_gpu.py builds the launched descriptor through hip_ops.gemm and checks it plans the same."""
    aks, bks = LAYOUTS[c["layout"]]
    M, N, K, pad = c["M"], c["N"], c["K"], c["pad"]
    f = dict(M=M, N=N, K=K, a_kstrided=aks, b_kstrided=bks, in_dtype=0 if c["dtype"] == "bf16" else 1,
             out_dtype=0 if c["out"] == "bf16" else 1, epilogue=EPIS.index(c["epi"]), split_k=1,
             lda=(M if aks else K) + pad.get("lda", 0), ldb=(N if bks else K) + pad.get("ldb", 0), ldc=N + pad.get("ldc", 0),
             ldr=N + pad.get("ldr", 0), ldaux=N + pad.get("ldaux", 0), scale=c["scale"], scale_cols=c["scale_cols"])
    f["a_grp"], f["a_grp_stride"], f["a_off"] = c["a_remap"]
    f["c_grp"], f["c_grp_stride"], f["c_off"] = c["c_remap"]
    if c["epi"] in ("resid", "gelu_bwd"):
        f["resid"] = 1
    if c["epi"] == "gelu" and c["aux"]:
        f["aux"] = 1
    if c["colsum"]:
        f["colsum_partials"] = 1
    if c["frames"]:
        BT, H, W, P, u8 = c["frames"]
        f.update(a_frames=1, a_frames_u8=u8, fr_H=H, fr_W=W, fr_P=P)
    if isinstance(c["split"], int):
        f["split_k"] = c["split"]
    return f


CASES = _matrix() + _edges() + _step()
assert len({c["id"] for c in CASES}) == len(CASES), "duplicate case ids"
