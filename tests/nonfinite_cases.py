"""The cases of the non-finite tests (a helper, not a test; CPU only): for every kernel family the inputs, the fp64 reference and the
planted elements, built from the existing case tables and references.  tests/test_nonfinite_cpu.py proves the reference side of every
(case, element, value) listed here; the GPU files run the kernels on the same lists."""
import functools
import zlib

import torch

from tests import attn_emulation as AE
from tests import attn_pooled_emulation as APE
from tests import attn_probs_ref as PR
from tests import embed_ref as ER
from tests import gemm_cases as GC
from tests import layernorm_ref as LR
from tests import loss_family_ref as LF
from tests import pair_loss_ref as PL
from tests.nonfinite import INF, NAN, Case, Plant


def _all(t):
    return torch.ones(t.shape, dtype=torch.bool)


# ---------------------------------------------------------------------------------------------------------------- the loss family
# (n, m, d): tiled logits (d % 4 != 0), the small-logits form, and another row count for img / cap (the two VidImg kinds)
LOSS_SHAPES = [(9, 9, 30), (70, 70, 32)]
LOSS_RECT = (5, 10, 32)
LOSS_LOG_SCALE = 3.7
# the operands that meet in one logit matrix (or in one merged-negatives group): a plant in one of them reaches exactly the gradients
# of the operands it shares a group with, the loss and d log_scale
LOSS_GROUPS = {
    "nce": ["vt"], "dsl": ["vt"], "vs_vc": ["vt", "vc"], "vs_vc_fc": ["vt", "vc", "ic"], "vsc": ["vtc"], "vsc_fc": ["vtc", "ic"],
    "vidimg": ["vtic"], "vidimg_divide": ["vt", "ic"],
}
_OPERANDS = {"v": "vis", "t": "txt", "i": "img", "c": "cap"}


def loss_ref(kind):
    def ref(inputs, dtype=torch.float64):
        feats = [inputs[k] for k in ("vis", "txt", "img", "cap")]
        loss, grads, dls = LF.loss_and_grads(kind, feats, inputs["log_scale"], dtype=dtype)
        out = {"loss": loss}
        out.update({"d_" + k: g for k, g in zip(("vis", "txt", "img", "cap"), grads)})
        out["d_log_scale"] = dls
        return out
    return ref


@functools.lru_cache(maxsize=None)
def loss_case(kind, shape):
    n, m, d = shape
    feats = [f.float() for f in LF.unit_feats(n, m, d, seed=1000 + n + m + d)]
    inputs = dict(zip(("vis", "txt", "img", "cap"), feats), log_scale=torch.tensor(LOSS_LOG_SCALE, dtype=torch.float32))
    ref = loss_ref(kind)
    clean = ref(inputs)
    reads = {"vis": True, "txt": True, "img": LF.KINDS[kind][1], "cap": LF.KINDS[kind][2]}
    rows = {"vis": n, "txt": n, "img": m, "cap": m}
    # one element each, in the last row (the ragged tile), row 3, row 1 and row 0.  (Elements whose probe leaves some gradient row
    # unchanged to the last fp64 bit -- a saturated softmax row -- were passed over: vis[n-1, d-1], txt[1, 0], img[m/2, 3], cap[0, d/2].)
    at = {"vis": (n - 1) * d, "txt": 3 * d, "img": d + 3, "cap": 0}
    plants = []
    for letter, name in _OPERANDS.items():
        if not reads[name]:
            continue
        reached = set("".join(g for g in LOSS_GROUPS[kind] if letter in g))
        expect = {"loss": _all(clean["loss"]), "d_log_scale": _all(clean["d_log_scale"])}
        expect.update({"d_" + _OPERANDS[x]: _all(clean["d_" + _OPERANDS[x]]) for x in reached})
        assert at[name] < rows[name] * d
        plants.append(Plant(name, at[name], (NAN,), expect, where=f"{name}@{at[name]}"))
    everything = {k: _all(v) for k, v in clean.items() if v is not None}
    plants.append(Plant("log_scale", 0, (NAN, INF), everything, where="log_scale"))
    return Case("loss", f"{kind}-{n}x{m}x{d}", inputs, ref, plants, extra=dict(kind=kind, shape=shape, reads=reads))


def loss_cases():
    out = [loss_case(k, s) for k in LF.KINDS for s in LOSS_SHAPES]
    return out + [loss_case(k, LOSS_RECT) for k in ("vidimg", "vidimg_divide")]


# ---------------------------------------------------------------------------------------------------------------- the pair losses
PAIR_SHAPE = (9, 30, 1039)          # (n, d, seed): tests/test_pair_loss_gpu.py::ODD_D


def pair_key(p):
    return tuple(sorted(dict(PL.DEFAULTS, **p).items()))


@functools.lru_cache(maxsize=None)
def pair_case(kind, key):
    p = dict(key)
    n, d, seed = PAIR_SHAPE
    vis, txt = (f.float() for f in PL.unit_feats(n, d, seed, bag=p["bag"]))
    inputs = dict(vis=vis, txt=txt)

    def ref(inputs, dtype=torch.float64):
        loss, (dv, dt) = PL.loss_and_grads(kind, [inputs["vis"], inputs["txt"]], dtype=dtype, **p)
        return {"loss": loss, "d_vis": dv, "d_txt": dt}
    # nce and milnce couple every pair through their softmaxes; the selecting kinds have no structural set that is easy to state
    smooth = kind in ("nce", "milnce") or (kind == "hardneg" and p["hard_negative_num"] == n)
    expect = {"loss": torch.ones((), dtype=torch.bool), "d_vis": _all(vis), "d_txt": _all(txt)} if smooth else None
    plants = [Plant("vis", 4 * d + 7, (NAN,), expect, where="vis[4,7]"),
              Plant("txt", (txt.shape[0] - 1) * d + d - 1, (NAN,), expect, where="txt[last,last]")]
    name = kind + "".join(f"-{k}={v}" for k, v in p.items() if v != PL.DEFAULTS[k])
    return Case("pair", name, inputs, ref, plants, selects=kind == "triplet", extra=dict(kind=kind, params=p))


def pair_cases():
    return [pair_case(k, pair_key(p)) for k, p in PL.configs(PAIR_SHAPE[0])]


# ---------------------------------------------------------------------------------------------- embedding, pooling, normalise
# fp64 restatements of tests/embed_ref.py's index maps and sums (those fix an fp32 add order; here only WHICH inputs an output reads
# matters).  Every one of these ops works column by column, so I(e) is the complement of D(e): every other row and column.

TEXT_CASE, VIP_BWD_CASE, GATHER_CASE, L2NORM_CASE = ER.TEXT_CASES[1], ER.VIP_BWD_CASES[1], ER.GATHER_CASES[1], ER.L2NORM_CASES[1]


def _f(t, dtype):
    return t.to(dtype)


def _mask(shape, *index):
    m = torch.zeros(shape, dtype=torch.bool)
    m[index] = True
    return m


def _plant_col(which, t, index, expect, values=(NAN, INF)):
    """a plant at multi-index `index` of t, I = the complement of the structural D"""
    flat = int(torch.arange(t.numel()).view(t.shape)[index])
    return Plant(which, flat, values, expect, {k: ~m for k, m in expect.items()}, where=f"{which}{list(index)}")


@functools.lru_cache(maxsize=None)
def text_fwd_case(dtype):
    B, Lt, D, V = TEXT_CASE
    inp = ER.text_inputs(TEXT_CASE, dtype)
    ids = inp["ids"]
    inputs = dict(ids=ids, tok=inp["tok"], pos=inp["pos"])

    def ref(inputs, dtype=torch.float64):
        return {"x": ER.text_embed(inputs["ids"], _f(inputs["tok"], dtype), _f(inputs["pos"], dtype))}
    counts = [(int(tid), (ids == tid).any(1).sum().item()) for tid in ids.unique()]
    once = next(tid for tid, k in counts if k == 1)                       # a token id that one sample alone uses
    unused = V - 2
    assert not (ids == unused).any()
    used = (ids == once)[:, :, None].expand(B, Lt, D) & _mask((B, Lt, D), slice(None), slice(None), 5)
    plants = [_plant_col("tok", inputs["tok"], (once, 5), {"x": used}),
              _plant_col("tok", inputs["tok"], (unused, 5), {"x": torch.zeros(B, Lt, D, dtype=torch.bool)}),
              _plant_col("pos", inputs["pos"], (Lt - 1, D - 1), {"x": _mask((B, Lt, D), slice(None), Lt - 1, D - 1)}),
              _plant_col("pos", inputs["pos"], (Lt, 0), {"x": torch.zeros(B, Lt, D, dtype=torch.bool)})]      # a row beyond Lt
    return Case("embed", f"text_fwd-{str(dtype)[6:]}", inputs, ref, plants, extra=dict(dtype=dtype, empty_ok=True))


@functools.lru_cache(maxsize=None)
def text_bwd_case(dtype):
    B, Lt, D, V = TEXT_CASE
    inp = ER.text_inputs(TEXT_CASE, dtype)
    ids = inp["ids"]
    inputs = dict(ids=ids, dx=inp["dx"])

    def ref(inputs, dtype=torch.float64):
        dx = _f(inputs["dx"], dtype)
        d_tok = torch.zeros(V, D, dtype=dtype).index_add_(0, inputs["ids"].reshape(-1), dx.reshape(B * Lt, D))
        return {"d_tok": d_tok, "d_pos": dx.sum(0)}
    plants = []
    for b, t, c in ((0, 0, 0), (B - 1, Lt - 1, D - 1), (1, 2, 7)):
        expect = {"d_tok": _mask((V, D), int(ids[b, t]), c), "d_pos": _mask((Lt, D), t, c)}
        plants.append(_plant_col("dx", inputs["dx"], (b, t, c), expect))
    return Case("embed", f"text_bwd-{str(dtype)[6:]}", inputs, ref, plants, extra=dict(dtype=dtype))


@functools.lru_cache(maxsize=None)
def vip_bwd_case(dtype):
    B, M, T, L, D = VIP_BWD_CASE
    dx, _ = ER.vip_bwd_inputs(VIP_BWD_CASE, dtype)
    inputs = dict(dx=dx)

    def ref(inputs, dtype=torch.float64):
        x = _f(inputs["dx"], dtype)
        fr = x[:, M:].reshape(B, T, L, D)
        d_pos = torch.cat([x[:, :M].sum((0, 1))[None], fr.sum((0, 1))])
        return {"d_class": x[:, 0].sum(0), "d_added": x[:, 1:M].sum(0), "d_pos": d_pos, "d_time": fr.sum((0, 2))}
    shapes = {"d_class": (D,), "d_added": (M - 1, D), "d_pos": (1 + L, D), "d_time": (T, D)}

    def expect(**hit):
        return {k: _mask(s, *hit[k]) if k in hit else torch.zeros(s, dtype=torch.bool) for k, s in shapes.items()}
    plants = [_plant_col("dx", dx, (1, 0, 3), expect(d_class=(3,), d_pos=(0, 3))),
              _plant_col("dx", dx, (B - 1, 2, D - 1), expect(d_added=(1, D - 1), d_pos=(0, D - 1))),
              _plant_col("dx", dx, (0, M, 0), expect(d_pos=(1, 0), d_time=(0, 0))),
              _plant_col("dx", dx, (B - 1, M + T * L - 1, 64), expect(d_pos=(L, 64), d_time=(T - 1, 64)))]
    return Case("embed", f"vip_bwd-{str(dtype)[6:]}", inputs, ref, plants, extra=dict(dtype=dtype))


@functools.lru_cache(maxsize=None)
def gather_case(dtype):
    B, S, D = GATHER_CASE
    x, dout, idx = ER.gather_inputs(GATHER_CASE, dtype)
    inputs = dict(x=x, idx=idx)

    def ref(inputs, dtype=torch.float64):
        return {"out": ER.gather_rows(_f(inputs["x"], dtype), inputs["idx"])}
    other = (int(idx[1]) + 1) % S                                          # a row of sample 1 that is not gathered
    plants = [_plant_col("x", x, (1, int(idx[1]), D - 1), {"out": _mask((B, D), 1, D - 1)}),
              _plant_col("x", x, (0, int(idx[0]), 0), {"out": _mask((B, D), 0, 0)}),
              _plant_col("x", x, (1, other, 4), {"out": torch.zeros(B, D, dtype=torch.bool)})]
    return Case("embed", f"gather-{str(dtype)[6:]}", inputs, ref, plants, extra=dict(dtype=dtype, empty_ok=True))


@functools.lru_cache(maxsize=None)
def scatter_case(dtype):
    B, S, D = GATHER_CASE
    x, dout, idx = ER.gather_inputs(GATHER_CASE, dtype)
    inputs = dict(dout=dout, idx=idx)

    def ref(inputs, dtype=torch.float64):
        return {"dx": ER.scatter_rows(_f(inputs["dout"], dtype), inputs["idx"], S)}
    plants = [_plant_col("dout", dout, (b, c), {"dx": _mask((B, S, D), b, int(idx[b]), c)}) for b, c in ((0, 0), (B - 1, D - 1))]
    return Case("embed", f"scatter-{str(dtype)[6:]}", inputs, ref, plants, extra=dict(dtype=dtype))


@functools.lru_cache(maxsize=None)
def l2norm_fwd_case(dtype):
    rows, cols = L2NORM_CASE
    x, _ = ER.l2norm_inputs(L2NORM_CASE, dtype)

    def ref(inputs, dtype=torch.float64):
        xd = _f(inputs["x"], dtype)
        n = xd.norm(dim=-1, keepdim=True)
        return {"y": xd / n, "inv": (1.0 / n)[:, 0]}
    plants = [_plant_col("x", x, (r, c), {"y": _mask((rows, cols), r), "inv": _mask((rows,), r)}, (NAN,))
              for r, c in ((0, 0), (rows - 1, cols - 1), (1, 129))]
    return Case("embed", f"l2norm_fwd-{str(dtype)[6:]}", dict(x=x), ref, plants, extra=dict(dtype=dtype))


@functools.lru_cache(maxsize=None)
def l2norm_bwd_case(dtype):
    """dx = inv (dy - y <y, dy>) on fp32 dy, y, inv (y and inv of the fp64 forward, rounded to fp32); dx is stored in `dtype`"""
    rows, cols = L2NORM_CASE
    x, dy = ER.l2norm_inputs(L2NORM_CASE, dtype)
    y, inv = (t.float() for t in ER.l2norm_fwd64(x))

    def ref(inputs, dtype=torch.float64):
        return {"dx": ER.l2norm_bwd64(inputs["dy"], inputs["y"], inputs["inv"]).to(dtype)}
    inputs = dict(dy=dy, y=y, inv=inv)
    row = lambda r: {"dx": _mask((rows, cols), r)}
    plants = [_plant_col("dy", dy, (0, 0), row(0), (NAN,)), _plant_col("dy", dy, (rows - 1, cols - 1), row(rows - 1), (NAN,)),
              _plant_col("y", y, (1, 129), row(1), (NAN,)), _plant_col("inv", inv, (rows - 1,), row(rows - 1), (NAN,))]
    return Case("embed", f"l2norm_bwd-{str(dtype)[6:]}", inputs, ref, plants, extra=dict(dtype=dtype))


def embed_cases():
    makers = (text_fwd_case, text_bwd_case, vip_bwd_case, gather_case, scatter_case, l2norm_fwd_case, l2norm_bwd_case)
    return [mk(dt) for mk in makers for dt in ER.DTYPES]


# ---------------------------------------------------------------------------------------------------------------- LayerNorm


def _ln_pick(kind, dtype, cols, **kw):
    """the shortest case of the table with these fields that has more than one row (a one-row case has no independent row)"""
    pool = [c for c in (LR.FWD_CASES if kind == "fwd" else LR.BWD_CASES)
            if c.dtype == dtype and c.cols == cols and c.rows > 1 and c.rows < LR.BIG and c.eps == 1e-5
            and all(getattr(c, k) == v for k, v in dict(dict(side=None, ldx_pad=0, x_off=0, ldy_pad=0, form=None, mode=None,
                                                             dres=None), **kw).items() if v is not None or k == "side")]
    assert pool, (kind, dtype, cols, kw)
    return min(pool, key=lambda c: c.rows)


def layernorm_table():
    """forward: every width of FWD_WIDTHS, bf16 and f32; both SIDES on the half-wave and the wave-per-row kernel; the cases whose rows
    have padding.  Backward: every width of BWD_WIDTHS in mode 2 (all four partial vectors, with dres), one plain case without dres,
    the side rows and the pooled form."""
    f = [_ln_pick("fwd", dt, cols) for dt in ("bf16", "f32") for cols in LR.FWD_WIDTHS]
    for rows, side in LR.SIDES:
        f += [_ln_pick("fwd", "bf16", 256, side=side), _ln_pick("fwd", "bf16", 260, side=side), _ln_pick("fwd", "f32", 260, side=side)]
    f += [_ln_pick("fwd", "bf16", 256, ldx_pad=4), _ln_pick("fwd", "bf16", 256, x_off=4), _ln_pick("fwd", "bf16", 256, ldy_pad=8)]
    b = [_ln_pick("bwd", dt, cols, form="deferred", mode=2, dres=True) for dt in ("bf16", "f32") for cols in LR.BWD_WIDTHS]
    b += [_ln_pick("bwd", dt, 260, form="deferred", mode=0, dres=False) for dt in ("bf16", "f32")]
    b += [_ln_pick("bwd", "bf16", 260, form="immediate", mode=0, dres=True)]
    b += [_ln_pick("bwd", "bf16", 256, mode=2, side=LR.SIDES[0][1]), _ln_pick("bwd", "f32", 260, mode=2, side=LR.SIDES[0][1]),
          _ln_pick("bwd", "bf16", 512, form="pooled", side=(1, 1, 4))]
    return f, b


def _ln_x(case, inputs, dtype):
    x = LR.rows_view(inputs["xbuf"], case.x_off, inputs["xbuf_ld"], case.rows, case.cols).to(dtype).clone()
    if case.side:
        is_side, sidx = LR.side_index(case.rows, case.side)
        x[is_side] = inputs["x_side"][sidx[is_side]].to(dtype)
    return x


def _ln_stats(x, eps):
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    return mean, 1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))


@functools.lru_cache(maxsize=None)
def layernorm_case(case):
    """tests/layernorm_ref.py's case with build(case)'s tensors.  The backward is the pair the model runs: mean and rstd come from the
    forward on the same x, so a plant in x reaches them.  In fp64 the reference is LR.ref_fwd / LR.ref_bwd themselves; the
    restatement in another dtype only serves the +-inf comparison."""
    inp = LR.build(case)
    rows, cols, ld = case.rows, case.cols, inp["ldx"]
    inputs = {k: inp[k] for k in ("xbuf", "gamma", "beta", "x_side", "dybuf", "dres") if inp.get(k) is not None}
    inputs["xbuf_ld"] = ld
    is_side, sidx = LR.side_index(rows, case.side) if case.side else (torch.zeros(rows, dtype=torch.bool), None)
    n_side = inputs["x_side"].shape[0] if case.side else 0

    def ref(inputs, dtype=torch.float64):
        x, gamma, beta = _ln_x(case, inputs, dtype), inputs["gamma"].to(dtype), inputs["beta"].to(dtype)
        if dtype == torch.float64:
            fw = LR.ref_fwd(x, gamma, beta, case.eps)
            mean, rstd, y = fw["mean"], fw["rstd"], fw["y"]
        else:
            mean, rstd = _ln_stats(x, case.eps)
            y = (x - mean[:, None]) * rstd[:, None] * gamma + beta
        if case.kind == "fwd":
            out = {"y": y, "mean": mean, "rstd": rstd}
            if case.side:
                out["y_side"] = torch.zeros(n_side, cols, dtype=dtype)
                out["y_side"][sidx[is_side]] = y[is_side]
            return out
        dy = LR.rows_view(inputs["dybuf"], 0, ld, rows, cols).to(dtype)
        dres = inputs["dres"].to(dtype) if case.dres else None
        if dtype == torch.float64:
            bw = LR.ref_bwd(dy, x, gamma, mean, rstd, dres)
        else:
            xh, gy = (x - mean[:, None]) * rstd[:, None], dy * gamma
            c1, c2 = gy.mean(1, keepdim=True), (gy * xh).mean(1, keepdim=True)
            r = torch.zeros_like(dy) if dres is None else dres
            dx = rstd[:, None] * (gy - c1 - xh * c2) + r
            bw = {"dx": dx, "dgamma": (dy * xh).sum(0), "dbeta": dy.sum(0), "colsum_dx": dx.sum(0), "colsum_dres": r.sum(0)}
        keys = ["dx", "dgamma", "dbeta"] + (["colsum_dx"] if case.mode >= 1 else []) + (["colsum_dres"] if case.mode == 2 else [])
        return {k: bw[k] for k in keys}
    clean = ref(inputs)
    shapes = {k: v.shape for k, v in clean.items()}
    x_read = _ln_x(case, inputs, torch.float64)
    varies = ~(x_read == x_read[:, :1]).all(1)               # a constant row has x-hat = 0: gamma does not reach its y

    def sets(**hit):
        """(D, I): D from per-output index tuples ("all" = everything), I its complement"""
        D = {}
        for k, s in shapes.items():
            h = hit.get(k)
            D[k] = torch.ones(s, dtype=torch.bool) if h == "all" else (torch.zeros(s, dtype=torch.bool) if h is None else _mask(s, *h))
        return D, {k: ~m for k, m in D.items()}

    def x_plant(r, c):
        """element (r, c) of the x the kernel reads: in the fp32 side rows, or in the padded buffer"""
        if bool(is_side[r]):
            return "x_side", int(sidx[r]) * cols + c
        return "xbuf", case.x_off + r * ld + c
    third = 20 if rows > 20 else rows // 2                     # the backward's second partial-row group (16 rows each)
    x_rows = sorted({0, rows - 1, third})                      # (with SIDES[0]: rows 0 and 20 are side rows, the last one is plain)
    plants = []
    c0 = cols - 1
    for r in x_rows:
        c = (r * 5 + 3) % cols
        which, idx = x_plant(r, c)
        if case.kind == "fwd":
            hit = dict(y=(r,), mean=(r,), rstd=(r,))
            if bool(is_side[r]):
                hit["y_side"] = (int(sidx[r]),)
        else:
            hit = dict(dx=(r,), dgamma="all", colsum_dx="all")
        D, I = sets(**hit)
        plants.append(Plant(which, idx, (NAN, INF, -INF), D, I, where=f"x[{r},{c}]"))
        if case.kind == "bwd":
            D, I = sets(dx=(r,), dgamma=(c,) if bool(varies[r]) else None, dbeta=(c,), colsum_dx="all")
            I["dgamma"][c] = False                             # (a constant row has x-hat = 0: 0 * NaN, unasserted)
            plants.append(Plant("dybuf", r * ld + c, (NAN, INF, -INF), D, I, where=f"dy[{r},{c}]"))
    if case.kind == "fwd":
        col = torch.zeros(shapes["y"], dtype=torch.bool)
        col[varies, c0] = True
        D, I = sets()
        D["y"] = col
        if case.side:
            D["y_side"][sidx[is_side & varies], c0] = True
        I = {k: ~m for k, m in D.items()}
        I["y"][:, c0] = False                                  # (a constant row's y[c0] is beta either way: unasserted)
        if case.side:
            I["y_side"][:, c0] = False
        plants.append(Plant("gamma", c0, (NAN, INF), D, I, where=f"gamma[{c0}]"))
    else:
        D, I = sets(dx="all", colsum_dx="all")
        plants.append(Plant("gamma", c0, (NAN, INF), D, I, where=f"gamma[{c0}]"))
        if case.dres:
            r, c = rows - 1, 1
            D, I = sets(dx=(r, c), colsum_dx=(c,), colsum_dres=(c,))
            plants.append(Plant("dres", r * cols + c, (NAN, INF), D, I, where=f"dres[{r},{c}]"))
    if case.side and not bool(is_side.all()):                  # the bf16 x of a side row is never read
        r = int(is_side.nonzero()[0])
        D, I = sets()
        plants.append(Plant("xbuf", case.x_off + r * ld + 2, (NAN,), D, I, where=f"xbuf[{r},2] (a side row's bf16 x)"))
    return Case("layernorm", case.id, inputs, ref, plants, extra=dict(case=case, is_side=is_side, sidx=sidx))


def layernorm_cases():
    f, b = layernorm_table()
    return [layernorm_case(c) for c in f + b]


def layernorm_padding(case, inputs, value):
    """`inputs` with `value` in every element of xbuf / dybuf / x_side that the case's header says is not read: the pitch padding, the
    elements before x_off and behind the last row, the bf16 x of side rows, the side rows no row maps to"""
    out = dict(inputs)
    is_side, sidx = LR.side_index(case.rows, case.side) if case.side else (torch.zeros(case.rows, dtype=torch.bool), None)
    ld = inputs["xbuf_ld"]
    for name, off, skip in (("xbuf", case.x_off, is_side), ("dybuf", 0, torch.zeros_like(is_side))):
        if name not in inputs:
            continue
        buf = torch.full_like(inputs[name], value)
        view = LR.rows_view(buf, off, ld, case.rows, case.cols)
        view[~skip] = LR.rows_view(inputs[name], off, ld, case.rows, case.cols)[~skip]
        out[name] = buf
    if case.side:
        xs = torch.full_like(inputs["x_side"], value)
        xs[sidx[is_side]] = inputs["x_side"][sidx[is_side]]
        out["x_side"] = xs
    return out


# ---------------------------------------------------------------------------------------------------------------- GEMM
GEMM_DT = {"bf16": torch.bfloat16, "f32": torch.float32}
# the epilogues that read a further operand: (epilogue, what else the case must have)
GEMM_EPIS = (("bias", None), ("gelu", "aux"), ("resid", "side"), ("gelu_bwd", None), ("qscale", None), ("patch", None))


def gemm_selection():
    """by field, not by id: per family the smallest case of every epilogue that reads a further operand (gelu with aux, resid with
    side rows; the gelu_bwd case is run with its column sums); one tn split-K case per family and aremap-ks-split; edge-ld-*"""
    small = [c for c in GC.CASES if not c["step"]]
    out = []
    for fam in GC.FAMILIES:
        for epi, need in GEMM_EPIS:
            pool = [c for c in small if c["expect"]["family"] == fam and c["epi"] == epi and (need is None or c[need])
                    and c["split"] == 1]
            if pool:
                # (a case with a second row tile first: the plant in it needs one)
                out.append(min(pool, key=lambda c: (c["M"] <= GC.TILE_ROWS[fam] + 3, c["M"] * c["N"] * c["K"], c["id"])))
    by_id = {c["id"]: c for c in small}
    out += [by_id[i] for i in ("splitk-3-g256", "splitk-3-direct", "splitk-3-f32", "aremap-ks-split")]
    out += [c for c in small if c["id"].startswith("edge-ld-")]
    seen, uniq = set(), []
    for c in out:
        if c["id"] not in seen:
            seen.add(c["id"])
            uniq.append(c)
    return uniq


def gemm_remap(grp, stride, off, r):
    return r if grp == 0 else (r // grp) * stride + off + r % grp


def gemm_side_index(M, side):
    S, Ms = side
    m = torch.arange(M)
    is_side = (m % S) < Ms
    return is_side, (m // S) * Ms + m % S


@functools.lru_cache(maxsize=None)
def _gemm_case(cid):
    """the LOGICAL operands of the case (A [M, K], B [N, K], bias, resid [M, N], the fp32 side rows, the patch tables; frames instead
    of A for the frame gather), drawn as tests/test_gemm_plans_gpu.py::run_case draws them, and run_case's fp64 reference"""
    c = next(x for x in GC.CASES if x["id"] == cid)
    g = torch.Generator().manual_seed(zlib.crc32(cid.encode()))
    M, N, K, epi = c["M"], c["N"], c["K"], c["epi"]
    dt = GEMM_DT[c["dtype"]]
    s_in = 0.5 if dt == torch.bfloat16 else 1.0
    inputs = {}
    u8 = bool(c["frames"] and c["frames"][4])
    if c["frames"]:
        BT, H, W, P, _ = c["frames"]
        if u8:
            inputs["frames"] = torch.randint(0, 256, (BT, 3, H, W), generator=g, dtype=torch.int32).to(torch.uint8)
        else:
            inputs["frames"] = torch.randn(BT, 3, H, W, generator=g)
    else:
        inputs["A"] = (torch.randn(M, K, generator=g) * s_in).to(dt)
    inputs["B"] = (torch.randn(N, K, generator=g) * s_in).to(dt)
    if epi in ("bias", "qscale", "gelu", "resid"):
        inputs["bias"] = torch.randn(N, generator=g)
    if epi in ("resid", "gelu_bwd"):
        inputs["resid"] = torch.randn(M, N, generator=g).to(dt)
    side = c["side"] if epi == "resid" else None
    if side:
        is_side, sidx = gemm_side_index(M, side)
        n_side = ((M + side[0] - 1) // side[0]) * side[1]
        inputs["resid_side"] = torch.randn(n_side, N, generator=g)
    if epi == "patch":
        T, Lp, Mp = c["patch"]
        inputs["tab1"], inputs["tab2"] = torch.randn(T, N, generator=g), torch.randn(Lp, N, generator=g)
    colsum = epi == "gelu_bwd"

    def patches(fr, dtype):
        BT, H, W, P, _ = c["frames"]
        if u8:
            mean = torch.tensor(ER.CLIP_MEAN).view(1, 3, 1, 1)
            std = torch.tensor(ER.CLIP_STD).view(1, 3, 1, 1)
            fr = (fr.float() / 255.0 - mean) / std
        x = fr.unfold(2, P, P).unfold(3, P, P).permute(0, 2, 3, 1, 4, 5).reshape(-1, 3 * P * P)
        return x.to(torch.bfloat16).to(dtype)                         # the loader rounds what it gathers to bf16

    def ref(inputs, dtype=torch.float64):
        A = patches(inputs["frames"], dtype) if c["frames"] else inputs["A"].to(dtype)
        acc = A @ inputs["B"].to(dtype).t()
        out, aux = acc, None
        if "bias" in inputs:
            out = acc + inputs["bias"].to(dtype)
        if epi == "qscale":
            out = out * torch.where(torch.arange(N) < c["scale_cols"], c["scale"], 1.0).to(dtype)
        if epi == "scale":
            out = acc * c["scale"]
        if epi == "gelu":
            aux = out
            out = out * torch.sigmoid(1.702 * out)
        if epi == "resid":
            r = inputs["resid"].to(dtype)
            if side:
                r = r.clone()
                r[is_side] = inputs["resid_side"].to(dtype)[sidx[is_side]]
            out = out + r
        if epi == "gelu_bwd":
            r = inputs["resid"].to(dtype)
            s = torch.sigmoid(1.702 * r)
            out = acc * (s * (1 + 1.702 * r * (1 - s)))
        if epi == "patch":
            w = torch.arange(M) % (T * Lp)
            out = acc + inputs["tab1"].to(dtype)[w // Lp] + inputs["tab2"].to(dtype)[w % Lp]
        res = {"C": out}
        if aux is not None and c["aux"]:
            res["aux"] = aux
        if side:
            res["out_side"] = torch.zeros(n_side, N, dtype=dtype)
            res["out_side"][sidx[is_side]] = out[is_side]
        if colsum:
            res["colsum"] = out.sum(0)
            res["colsum_rows_sum"] = out.sum(0)                       # the sum of the epilogue's partial rows, where it writes them
        return res
    clean = ref(inputs)
    shapes = {k: v.shape for k, v in clean.items()}

    def sets(row=None, col=None, elem=None, rows=None):
        D = {k: torch.zeros(s, dtype=torch.bool) for k, s in shapes.items()}
        for k in ("C", "aux"):
            if k in D:
                if row is not None:
                    D[k][row] = True
                if col is not None:
                    D[k][:, col] = True
                if elem is not None:
                    D[k][elem] = True
                if rows is not None:
                    D[k][rows[0], rows[1]] = True
        if "out_side" in D:
            full = torch.zeros(M, N, dtype=torch.bool)
            full |= D["C"]
            D["out_side"][sidx[is_side]] = full[is_side]
        for k in ("colsum", "colsum_rows_sum"):
            if k in D:
                D[k] = D["C"].any(0)
        I = {k: ~m for k, m in D.items()}
        return D, I
    tile = GC.TILE_ROWS[c["expect"]["family"]]
    plants = []
    both = (NAN, INF)
    a_rows = sorted({0, M - 1} | ({tile + 3} if M > tile + 3 else set()))
    b_rows = sorted({0, N - 1} | ({tile + 3} if N > tile + 3 else set()))
    if c["frames"] and not u8:
        BT, H, W, P, _ = c["frames"]
        gw, per = W // P, (H // P) * (W // P)
        for r in a_rows:                                               # a pixel of patch r: row r of the gathered A
            bt, gy, gx = r // per, (r % per) // gw, r % gw
            idx = int(torch.arange(BT * 3 * H * W).view(BT, 3, H, W)[bt, 1, gy * P + 2, gx * P + 5])
            D, I = sets(row=r)
            plants.append(Plant("frames", idx, both, D, I, where=f"frames->A[{r}]"))
    elif not c["frames"]:
        for r in a_rows:
            D, I = sets(row=r)
            plants.append(Plant("A", r * K + (r * 7 + 1) % K, both, D, I, where=f"A[{r},{(r * 7 + 1) % K}]"))
    for n in b_rows:
        D, I = sets(col=n)
        plants.append(Plant("B", n * K + (n * 5 + 2) % K, both, D, I, where=f"B[{n},{(n * 5 + 2) % K}]"))
    if "bias" in inputs:
        D, I = sets(col=N - 1)
        plants.append(Plant("bias", N - 1, both, D, I, where=f"bias[{N - 1}]"))
    if "resid" in inputs:
        plain = [i for i in range(M - 1, -1, -1) if not (side and bool(is_side[i]))]      # the rows read from resid itself
        if plain:
            D, I = sets(elem=(plain[0], 3))
            plants.append(Plant("resid", plain[0] * N + 3, both if epi == "resid" else (NAN,), D, I, where=f"resid[{plain[0]},3]"))
        if side:                                                       # the bf16 resid of a side row is never read
            r = int(is_side.nonzero()[0])
            D, I = sets()
            plants.append(Plant("resid", r * N + 3, (NAN,), D, I, where=f"resid[{r},3] (a side row's bf16 resid)"))
    if side:
        r = int(is_side.nonzero()[-1])
        D, I = sets(elem=(r, N - 2))
        plants.append(Plant("resid_side", int(sidx[r]) * N + N - 2, both, D, I, where=f"resid_side[row of {r},{N - 2}]"))
    if epi == "patch":
        w = torch.arange(M) % (T * Lp)
        D, I = sets(rows=((w // Lp) == T - 1, 1))
        plants.append(Plant("tab1", (T - 1) * N + 1, both, D, I, where=f"tab1[{T - 1},1]"))
        D, I = sets(rows=((w % Lp) == 0, N - 1))
        plants.append(Plant("tab2", N - 1, both, D, I, where=f"tab2[0,{N - 1}]"))
    return Case("gemm", cid, inputs, ref, plants, extra=dict(case=c, side=(is_side, sidx) if side else None, colsum=colsum))


def gemm_cases():
    return [_gemm_case(c["id"]) for c in gemm_selection()]


# ---------------------------------------------------------------------------------------------------------------- attention
# (case, dtype name, variant): regime flat; bf16 everywhere, fp32 on three cases; the wide backward on the 300-key case
ATTN_RUNS = [("proxy1x3x5-B2H1", "bf16", None), ("proxy4x3x70-B1H3", "bf16", None), ("proxy4x2x49-B2H2", "bf16", None),
             ("proxy4x3x300-B2H2", "bf16", None), ("proxy4x3x300-B2H2", "bf16", "wide"), ("proxy17x2x180-B1H1", "bf16", None),
             ("causal77ragged-B2H2", "bf16", None), ("causal16allpad-B2H2", "bf16", None),
             ("proxy4x2x49-B2H2", "fp32", None), ("proxy4x3x300-B2H2", "fp32", None), ("causal77ragged-B2H2", "fp32", None)]
ATTN_DT = {"bf16": torch.bfloat16, "fp32": torch.float32}


def attn_visible(size, B, S, pad):
    """bool [B, S, S]: query i of sample b gives key j a weight that is not exactly zero"""
    add = AE.additive_mask(size, S, pad, torch.float64)
    vis = (add > torch.finfo(torch.float64).min).expand(B, 1, S, S)[:, 0].clone()
    return vis


@functools.lru_cache(maxsize=None)
def attn_case(name, dt):
    size, B, H, S, mode = AE.CASES[name]
    dtype = ATTN_DT[dt]
    qkv, dout, pad = AE.inputs(name, "flat", dtype)
    D = H * 64
    inputs = dict(qkv=qkv, dout=dout)
    vis = attn_visible(size, B, S, pad)
    kept = torch.ones(B, S, dtype=torch.bool) if pad is None else pad.bool()

    def ref(inputs, dtype=torch.float64):
        q, k, v = (t.transpose(1, 2) for t in inputs["qkv"].view(B, S, 3, H, 64).to(dtype).unbind(2))
        do = inputs["dout"].view(B, S, H, 64).to(dtype).transpose(1, 2)
        r = AE.reference(q, k, v, do, size, pad)
        out = {n: r[n] for n in ("out", "lse", "dq", "dk", "dv")}
        out["colsum"] = torch.cat([r[n].sum((0, 2)).reshape(-1) for n in ("dq", "dk", "dv")])
        return out
    shapes = dict(out=(B, H, S, 64), lse=(B, H, S), dq=(B, H, S, 64), dk=(B, H, S, 64), dv=(B, H, S, 64), colsum=(3 * D,))

    def sets(b, h, **hit):
        """D from {output: (rows mask [S], column or None)} inside problem (b, h); I: the other samples and the other heads.  The
        row sums (lse) of padded query positions are left out on both sides (the kernels' stats are not defined there)."""
        Dm = {k: torch.zeros(s, dtype=torch.bool) for k, s in shapes.items()}
        for k, (rows, col) in hit.items():
            if k == "lse":
                Dm[k][b, h, rows] = True
            elif col is None:
                Dm[k][b, h, rows] = True
            else:
                Dm[k][b, h, rows, col] = True
        Dm["lse"] &= kept[:, None, :]
        Dm["colsum"] = torch.cat([Dm[n].any(2).any(0).reshape(-1) for n in ("dq", "dk", "dv")])
        Im = {}
        for k, s in shapes.items():
            if k == "colsum":
                m = torch.ones(3, H, 64, dtype=torch.bool)
                m[:, h] = False
                Im[k] = m.reshape(-1)
            else:
                m = torch.ones(s, dtype=torch.bool)
                m[b, h] = False
                Im[k] = m
        Im["lse"] &= kept[:, None, :]
        return Dm, Im

    def at(b, s, j, h, d):
        return (b * S + s) * 3 * D + j * D + h * 64 + d
    b, h = B - 1, H - 1
    if mode == "allpad":
        b = 0                                                         # (sample 1 is all padding: its rows see no kept key)
    one = lambda i: torch.arange(S) == i
    plants = []
    # (causal: not row 0 -- it sees key 0 alone, its softmax is 1 whatever q is)
    q_rows = [0, size[0] + size[2] + 1 if size[1] > 1 else size[0] + 1] if size is not None else [2, int(kept[b].nonzero()[-1])]
    assert size is not None or int(kept[b].sum()) > 3
    for i in q_rows:                                                  # q of a proxy row and of a frame row (causal: first / last kept)
        keys = vis[b, i]
        Dm, Im = sets(b, h, out=(one(i), None), lse=(one(i), None), dq=(one(i), None), dk=(keys, None), dv=(keys, None))
        plants.append(Plant("qkv", at(b, i, 0, h, 5), (NAN, INF), Dm, Im, where=f"q[{b},{h},{i},5]"))
    k_keys = [min(1, size[0] - 1), S - 1] if size is not None else [1, int(kept[b].nonzero()[-1])]
    for n, j in enumerate(k_keys):                                    # k of a proxy key; k and v of a key in the last frame
        Q = vis[b, :, j]
        keys = vis[b][Q].any(0)
        Dm, Im = sets(b, h, out=(Q, None), lse=(Q, None), dq=(Q, None), dk=(keys, None), dv=(keys, None))
        plants.append(Plant("qkv", at(b, j, 1, h, 9), (NAN,), Dm, Im, where=f"k[{b},{h},{j},9]"))
        if n == 1:
            Dm, Im = sets(b, h, out=(Q, 11), dq=(Q, None), dk=(keys, None))
            plants.append(Plant("qkv", at(b, j, 2, h, 11), (NAN, INF), Dm, Im, where=f"v[{b},{h},{j},11]"))
    i = q_rows[1]
    Dm, Im = sets(b, h, dq=(one(i), None), dk=(vis[b, i], None), dv=(vis[b, i], 7))
    plants.append(Plant("dout", (b * S + i) * D + h * 64 + 7, (NAN, INF), Dm, Im, where=f"dout[{b},{h},{i},7]"))
    extra = dict(name=name, dt=dt, pad=pad)
    if mode == "ragged":                                              # k of a padded position: read, and weighted exactly zero
        bp = int((~kept).any(1).nonzero()[0])
        j = int((~kept[bp]).nonzero()[0])
        Dm, Im = sets(bp, h)
        plants.append(Plant("qkv", at(bp, j, 1, h, 3), (NAN,), Dm, Im, where=f"k[{bp},{h},{j},3] (a padded key)", unread=False))
        extra["padded_key"] = (bp, h, j)

    def derive(Dm):
        Dm["lse"] &= kept[:, None, :]                                  # (the row sums of padded query positions: see sets)
        Dm["colsum"] = torch.cat([Dm[n].any(2).any(0).reshape(-1) for n in ("dq", "dk", "dv")])
    return Case("attention", f"{name}-{dt}", inputs, ref, plants, extra=extra, derive=derive)


def attention_cases():
    seen, out = set(), []
    for name, dt, _ in ATTN_RUNS:
        if (name, dt) not in seen:
            seen.add((name, dt))
            out.append(attn_case(name, dt))
    return out


# ------------------------------------------------------------------------------------------- single-query (pooled) attention
# the smallest case with more than one key, a second sample and a second head (B2H2S1 has one key: its softmax is 1 whatever q and k)
POOLED_CASE = "B2H2S33"


@functools.lru_cache(maxsize=None)
def pooled_case(dt):
    B, H, S = APE.CASES[POOLED_CASE]
    q, kv, dout = APE.inputs(POOLED_CASE, "flat", APE.DT[dt])
    D = H * 64
    inputs = dict(q=q, kv=kv, dout=dout)

    def ref(inputs, dtype=torch.float64):
        k, v = inputs["kv"].to(dtype).view(B, S, 2, H, 64).unbind(2)
        r = APE.reference(inputs["q"].to(dtype).view(B, H, 64), k, v, inputs["dout"].to(dtype).view(B, H, 64))
        out = {n: r[n] for n in ("out", "lse", "dq", "dk", "dv")}
        out["colsum"] = torch.cat([r[n].sum((0, 1)).reshape(-1) for n in ("dk", "dv")])
        return out
    shapes = dict(out=(B, H, 64), lse=(B, H), dq=(B, H, 64), dk=(B, S, H, 64), dv=(B, S, H, 64), colsum=(2 * D,))

    def derive(Dm):
        Dm["colsum"] = torch.cat([Dm[n].any(1).any(0).reshape(-1) for n in ("dk", "dv")])

    def sets(b, h, out=None, lse=False, dq=False, dk=False, dv=None):
        """out / dv: False or None nothing, True the whole (b, h) slice, an int that column"""
        Dm = {k: torch.zeros(s, dtype=torch.bool) for k, s in shapes.items()}
        if out is not None:
            Dm["out"][b, h, slice(None) if out is True else out] = True
        Dm["lse"][b, h] = lse
        Dm["dq"][b, h] = dq
        Dm["dk"][b, :, h] = dk
        if dv is not None:
            Dm["dv"][b, :, h, slice(None) if dv is True else dv] = True
        derive(Dm)
        Im = {}
        for k, s in shapes.items():
            m = torch.ones(s, dtype=torch.bool)
            if k == "colsum":
                m = m.view(2, H, 64)
                m[:, h] = False
                m = m.reshape(-1)
            elif k in ("dk", "dv"):
                m[b, :, h] = False
            else:
                m[b, h] = False
            Im[k] = m
        return Dm, Im
    b, h = B - 1, H - 1
    plants = []
    Dm, Im = sets(b, h, out=True, lse=True, dq=True, dk=True, dv=True)
    plants.append(Plant("q", b * D + h * 64 + 5, (NAN, INF), Dm, Im, where=f"q[{b},{h},5]"))
    for s in (0, S - 1):                                              # the first key; the one key of the second 32-key block
        plants.append(Plant("kv", (b * S + s) * 2 * D + h * 64 + 9, (NAN,), Dm, Im, where=f"k[{b},{s},{h},9]"))
    Dv, Iv = sets(b, h, out=11, dq=True, dk=True)
    plants.append(Plant("kv", (b * S + S - 1) * 2 * D + D + h * 64 + 11, (NAN, INF), Dv, Iv, where=f"v[{b},{S - 1},{h},11]"))
    Do, Io = sets(b, h, dq=True, dk=True, dv=7)
    plants.append(Plant("dout", b * D + h * 64 + 7, (NAN, INF), Do, Io, where=f"dout[{b},{h},7]"))
    return Case("pooled", f"{POOLED_CASE}-{dt}", inputs, ref, plants, extra=dict(dt=dt), derive=derive)


def pooled_cases():
    return [pooled_case(dt) for dt in ("bf16", "fp32")]


# ---------------------------------------------------------------------------------------------------------- attention weights
PROBS_CASES = ("proxy1x3x5-B2H1", "causal16allpad-B2H2")          # the smallest proxy and the smallest masked causal case


@functools.lru_cache(maxsize=None)
def probs_case(name, dt):
    """xp_attn_probs behind xp_attn_fwd's stats: the softmax matrices of tests/attn_probs_ref.py from qkv alone (v is not read)"""
    size, B, H, S, mode = AE.CASES[name]
    qkv, _, pad = AE.inputs(name, "flat", ATTN_DT[dt])
    D = H * 64
    vis = attn_visible(size, B, S, pad)

    def ref(inputs, dtype=torch.float64):
        q, k, _ = (t.transpose(1, 2) for t in inputs["qkv"].view(B, S, 3, H, 64).to(dtype).unbind(2))
        if size is None:
            return {"probs": PR.causal_probs(q, k, pad)}
        proxy, frame = PR.proxy_probs(q, k, size)
        return {"proxy": proxy, "frame": frame}
    b, h = (0 if mode == "allpad" else B - 1), H - 1

    def sets(rows):
        """D: the visible entries of the query rows `rows` (bool [S]) of problem (b, h); I: the other samples and heads"""
        full = torch.zeros(B, H, S, S, dtype=torch.bool)
        full[b, h] = rows[:, None] & vis[b]
        if size is None:
            Dm = {"probs": full}
        else:
            M, N, L = size
            fr = full[:, :, M:].reshape(B, H, N, L, S)
            frame = torch.cat([fr[..., :M]] + [torch.stack([fr[:, :, n, :, M + n * L:M + (n + 1) * L] for n in range(N)], 2)], -1)
            Dm = {"proxy": full[:, :, :M], "frame": frame}
        Im = {}
        for k, m in Dm.items():
            i = torch.ones_like(m)
            i[b, h] = False
            Im[k] = i
        return Dm, Im

    def at(s, j, d):
        return (b * S + s) * 3 * D + j * D + h * 64 + d
    one = lambda i: torch.arange(S) == i
    if size is not None:
        q_rows, k_keys = [0, size[0] + size[2] + 1], [0, S - 1]
    else:
        q_rows, k_keys = [2, S - 1], [1, S - 1]
    plants = []
    for i in q_rows:
        Dm, Im = sets(one(i))
        plants.append(Plant("qkv", at(i, 0, 5), (NAN, INF), Dm, Im, where=f"q[{b},{h},{i},5]"))
    for j in k_keys:
        Dm, Im = sets(vis[b, :, j] & (vis[b].sum(1) > 1))              # (a row that sees one key has weight 1 whatever k is)
        plants.append(Plant("qkv", at(j, 1, 9), (NAN,), Dm, Im, where=f"k[{b},{h},{j},9]"))
    Dm, Im = sets(torch.zeros(S, dtype=torch.bool))
    Im = {k: torch.ones_like(m) for k, m in Im.items()}
    plants.append(Plant("qkv", at(S - 1, 2, 11), (NAN,), Dm, Im, where=f"v[{b},{h},{S - 1},11] (the weights do not read v)"))
    return Case("probs", f"{name}-{dt}", dict(qkv=qkv), ref, plants, extra=dict(name=name, dt=dt, pad=pad))


def probs_cases():
    return [probs_case(n, dt) for n in PROBS_CASES for dt in ("bf16", "fp32")]
