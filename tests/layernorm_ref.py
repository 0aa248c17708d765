"""LayerNorm (csrc/layernorm.hip): the fp64 definition of every entry point, the per-row / per-column metrics that hold the
kernels to it, a float32 emulation of the kernels' arithmetic on the CPU, the input families and the ONE case table that
tests/test_layernorm_ref_cpu.py (emulation + wrong kernels, no GPU) and tests/test_layernorm_contract_gpu.py (the kernels) share.
Plain helper module, no tests of its own.

The definition (every input as the kernel gets it, i.e. after rounding to its storage type, then widened to fp64)
---------------------------------------------------------------------------------------------------------------
forward    mean = mean_c(x);  rstd = 1 / sqrt(var_biased + eps);  y = (x - mean) * rstd * gamma + beta; a side row is read from x_side.
backward   the fp32 mean / rstd are INPUTS (converted to fp64, not recomputed):
           xh = (x - mean) * rstd;  gy = dy * gamma;  c1 = mean_c(gy);  c2 = mean_c(gy * xh)
           dx = rstd * (gy - c1 - xh * c2) + dres;  dgamma = sum_r dy * xh;  dbeta = sum_r dy
           colsum(dx) = column sums of the UNROUNDED dx (the kernel adds `o` before store4 rounds it); colsum(dres) of dres as read.

The metrics, u = 2^-24
----------------------
    quantity            scale of row r (or column c)                                                 gate
    y                   rstd_r * max_c|x| * max|gamma| + max|beta|                                   64 u
    mean                max_c|x|                                                                     64 u
    rstd                rstd_r                                                                       64 u
    dx                  rstd_r * (max|gy| + |c1| + max|xh| * |c2|) + max_c|dres|                     64 u
    every column sum    fp64 sum of the absolute values of that column's terms                       (rows + 8) u
A bf16 output gets 2^-8 * |ref| + 1.01 * gate per element (one round-to-nearest of the fp32 value).  A multiple reported for a bf16
output is what is left of the error after the 2^-8 * |ref| allowance, in units of u * scale.

Where 64 u comes from: a count of roundings, not a measurement.  Each statistic (sum x, sum d^2; sum gy, sum gy * xh) is a sum of at
most 1024 terms: per lane at most 32 sequential adds (half-wave kernel: 4 slabs x 8 elements as 4 adds of pre-summed groups of 8,
wave kernels: 16), then a 5- or 6-step butterfly -- at most 38 roundings along any path, each relative to a partial sum that the
row's scale bounds, and they enter the result divided by cols.  Two statistics feed every output and fewer than 10 element-wise
roundings follow them (x - mean, * rstd, * gamma, + beta; rsqrt itself is 1-2 ulp).  The worst case of one statistic alone is
38 u; the two do not reach their worst case in the same direction at the same element, and the element-wise tail adds < 10 u:
64 u bounds the sum with the statistics at 27 u each.  (rows + 8) u: any summation order over `rows` fp32 terms has a forward error of
at most (rows - 1) u times the sum of absolute values, and each term carries a few roundings of its own (x - mean, * rstd, dy * xh).

colsum(dx), re-derived.  Its terms are NOT a few roundings away from exact: a term is the unrounded dx of one row, which carries the
error of that row's two statistics -- up to the dx gate, 64 u * scale_dx_r, and scale_dx_r is not bounded by |dx|: where
gy - c1 - xh * c2 cancels, |dx| is hundreds of times smaller.  With one row the column sum IS that dx, so (rows + 8) u * |dx| cannot
hold for any kernel that merely meets the dx gate: at 1 x 1024 in fp32 (gate 9 u) the emulation reaches 990 u and the MI355X 1770 u,
both with dx itself at < 3 u of ITS scale.  This is the gate's count, not the kernel: ln_bwd_kernel adds the very `o` it stores.  The
count that holds: |colsum(dx) - ref| <= (rows + 8) u * sum_r |dx_rc|  +  64 u * sum_r scale_dx_r -- the summation as for every column
sum, plus what the dx gate allows the terms (``slack_colsum_dx``).  The logs give both figures (after and before that allowance).
The wrong kernel that sums the ROUNDED dx still fails by three orders (tests/test_layernorm_ref_cpu.py).

Measured: worst multiple of u over the whole case table (gate 64, bf16 outputs 64.64; column sums rows + 8)
--------------------------------------------------------------------------------------------------------
                                   CPU emulation (kernels' summation shape, no FMA)      MI355X
    ln_fwd_h_kernel<1..4>          y 1.34   mean 2.03   rstd 2.74   y_side 2.03          y 1.34   mean 2.03   rstd 2.61   y_side 2.03
    ln_fwd_kernel<bf16_t>          y 0.86   mean 1.95   rstd 2.27   y_side 1.94          y 1.80   mean 3.25   rstd 2.79   y_side 3.24
    ln_fwd_kernel<float>           y 3.44   mean 2.90   rstd 3.05   y_side 3.44          y 3.44   mean 2.90   rstd 3.30   y_side 3.44
    ln_bwd_kernel<T, NJ, DXS>      dx 2.98                                               dx 2.81
    column sums (gate in brackets) dgamma 2.50 (9)   dbeta 1.26 (45)                     dgamma 2.50 (9)   dbeta 1.26 (45)
                                   colsum(dres) 1.16 (45)                                colsum(dres) 1.16 (45)
                                   colsum(dx) 0 after the dx-gate allowance, 990 (9) before it        0 after, 1770 (9) before
                                   colsum(dx) against the stored fp32 dx 1.87 (45)       1.87 (45)
    accumulate form (3.0 + sum)    (store only)                                          dgamma 1.20 (24)   dbeta 0.02 (24)
(The bf16 wave kernel's MI355X figures come from the 16395 x 12 side-row case, which the CPU file does not run.)  The emulation's column
is asserted by tests/test_layernorm_ref_cpu.py::test_emulation_worst_multiples_are_the_documented_ones; the MI355X column is read off
the per-case log of tests/test_layernorm_contract_gpu.py.  Every case gives the same bits on a second run.  Nothing is near a gate: the
gates are worst-case counts, the figures are what random roundings leave of them (about the square root).

Because the dx-gate allowance swallows colsum(dx)'s whole error (the constant rows' rstd = 316 dominates it), the SUMMATION of
colsum(dx) is also held on its own where that is possible: in fp32 the kernel adds the very `o` it stores, so colsum(dx) and the sums
of its partial rows are compared with the fp64 column sums of the STORED dx at (rows + 8) u of sum|dx|, with no allowance.
"""
import math
from dataclasses import dataclass

import torch

from tests import reduce_emulation as RE

U = 2.0 ** -24
GATE_ROW = 64.0                       # multiples of u
BF16_REL = 2.0 ** -8
DT = {"bf16": torch.bfloat16, "f32": torch.float32}
FAMILIES = ("normal", "offset", "tight", "large", "outlier", "const")



def col_gate(rows):
    return rows + 8.0


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------------------ the case table
@dataclass(frozen=True)
class Case:
    kind: str                 # "fwd" | "bwd"
    dtype: str                # "bf16" | "f32"
    rows: int
    cols: int
    eps: float = 1e-5
    ldx_pad: int = 0          # ldx = cols + ldx_pad
    x_off: int = 0            # x starts this many elements into its buffer
    ldy_pad: int = 0
    side: tuple = None        # (S, M, stride)
    mode: int = 0             # backward: 0 plain, 1 dx_colsum, 2 dx_colsum + dres_colsum
    dres: bool = True
    form: str = "deferred"    # backward: "deferred" | "immediate" | "pooled"
    S: int = 0                # pooled: sequence length (ldx = lddy = lddx = S * cols, lddres = cols)
    tag: str = ""

    @property
    def tdtype(self):
        return DT[self.dtype]

    @property
    def kernel(self):
        nj = cdiv(self.cols, 256)
        if self.kind == "bwd":
            return f"ln_bwd_kernel<{'bf16_t' if self.dtype == 'bf16' else 'float'},{nj},{self.mode}>"
        return fwd_kernel_name(self.dtype, self.cols, self.cols + self.ldx_pad, self.cols + self.ldy_pad, self.x_off)

    @property
    def id(self):
        s = f"{self.kernel}-{self.rows}x{self.cols}"
        if self.kind == "bwd":
            s += f"-{self.form}" + ("" if self.dres else "-nodres")
        if self.side:
            s += "-side" + "_".join(map(str, self.side))
        return s + (f"-{self.tag}" if self.tag else "")

    @property
    def seed(self):
        return (self.rows * 1009 + self.cols * 7 + self.mode * 3 + len(self.id)) % (2 ** 31)


def fwd_kernel_name(dtype, cols, ldx, ldy, x_off=0):
    """the forward kernel xp_layernorm_fwd_side launches (x_off: element offset of x in a 16-byte aligned buffer)"""
    if dtype == "f32":
        return "ln_fwd_kernel<float>"
    if cols % 8 == 0 and ldx % 8 == 0 and ldy % 8 == 0 and (x_off * 2) % 16 == 0:
        return f"ln_fwd_h_kernel<{cdiv(cols, 256)}>"
    return "ln_fwd_kernel<bf16_t>"


FWD_WIDTHS = (4, 8, 252, 256, 260, 512, 1020, 1024)
BWD_WIDTHS = (8, 260, 512, 768, 1024)          # NJ = 1, 2, 2, 3, 4 (768: the only width of NJ = 3)
SIDES = ((60, (10, 3, 5)), (8, (1, 1, 1)))
# a case with fewer rows than families (1 row; the pooled form's 5) starts at this family, so that over the widths of a sweep the
# one-row cases meet every family: forward 4 .. 1024 -> normal, const, tight, offset, large, tight, outlier, offset;
# backward 8, 260, 512, 768, 1024 -> const, large, tight, outlier, offset (normal: every longer case).  128 (in no sweep: the
# five-row cases of tests/test_alignment_gpu.py at the alignment floor) -> offset
SHORT_FIRST = {4: "normal", 8: "const", 128: "offset", 252: "tight", 256: "offset", 260: "large", 512: "tight", 768: "outlier", 1020: "outlier",
               1024: "offset"}
BIG = 16395                                   # beyond both grid caps (forward 16384 rows, backward 8192)


def _cases():
    f, b = [], []
    for dt in ("bf16", "f32"):
        for cols in FWD_WIDTHS:
            for rows in (1, 7, 37):
                f.append(Case("fwd", dt, rows, cols))
    f.append(Case("fwd", "bf16", 37, 768))                                   # ln_fwd_h_kernel<3>
    for cols in (256, 512, 768, 1024, 260):                                  # eps = 1e-6 once per kernel
        f.append(Case("fwd", "bf16", 7, cols, eps=1e-6, tag="eps1e-6"))
    f.append(Case("fwd", "f32", 7, 260, eps=1e-6, tag="eps1e-6"))
    f.append(Case("fwd", "bf16", 37, 256, ldx_pad=4, tag="ldx+4"))            # both must take the 8-byte kernel
    f.append(Case("fwd", "bf16", 37, 256, x_off=4, tag="xoff4"))
    f.append(Case("fwd", "bf16", 37, 256, ldy_pad=8, tag="ldy+8"))            # strided output, still the half-wave kernel
    f.append(Case("fwd", "bf16", 7, 260, ldy_pad=4, tag="ldy+4"))
    f.append(Case("fwd", "f32", 37, 260, ldy_pad=4, tag="ldy+4"))
    f.append(Case("fwd", "bf16", BIG, 8, tag="grid"))
    f.append(Case("fwd", "f32", BIG, 8, tag="grid"))
    f.append(Case("fwd", "bf16", BIG, 12, tag="grid"))
    for rows, side in SIDES:
        for cols in (256, 512, 1024):
            f.append(Case("fwd", "bf16", rows, cols, side=side))
        f.append(Case("fwd", "bf16", rows, 768, side=side))                   # ln_fwd_h_kernel<3> with side rows
        # the wave-per-row kernels with side rows (srow map, the fp32 xs load and the side.yout store of ln_fwd_kernel)
        f.append(Case("fwd", "bf16", rows, 260, side=side))
        f.append(Case("fwd", "bf16", rows, 256, ldx_pad=4, side=side, tag="ldx+4"))
        for cols in (260, 1024):
            f.append(Case("fwd", "f32", rows, cols, side=side))
    # beyond the grid with side rows: one wave serves side rows and ordinary rows across its grid-stride loop
    f.append(Case("fwd", "f32", BIG, 8, side=(10, 3, 5), tag="grid"))
    f.append(Case("fwd", "bf16", BIG, 12, side=(10, 3, 5), tag="grid"))
    for dt in ("bf16", "f32"):
        for cols in BWD_WIDTHS:
            for rows in (37, 1):
                for mode in (0, 1, 2):
                    b.append(Case("bwd", dt, rows, cols, mode=mode))
                    if mode < 2:
                        b.append(Case("bwd", dt, rows, cols, mode=mode, dres=False))
    b.append(Case("bwd", "bf16", 16, 260, form="immediate"))                  # 1, 38 and 512 partial rows
    b.append(Case("bwd", "f32", 600, 260, form="immediate"))
    b.append(Case("bwd", "bf16", BIG, 8, form="immediate", tag="grid"))
    b.append(Case("bwd", "f32", BIG, 8, mode=2, tag="grid"))                  # the block cap with all four partial vectors
    for cols in (512, 1024):
        b.append(Case("bwd", "bf16", 5, cols, form="pooled", S=7, side=(1, 1, 4)))
    for cols in (256, 512, 1024):
        for mode in (0, 2):
            b.append(Case("bwd", "bf16", 60, cols, mode=mode, side=(10, 3, 5)))
    b.append(Case("bwd", "f32", 60, 260, mode=2, side=(10, 3, 5)))
    return f, b


FWD_CASES, BWD_CASES = _cases()
CASES = {c.id: c for c in FWD_CASES + BWD_CASES}
assert len(CASES) == len(FWD_CASES) + len(BWD_CASES), "case ids must be unique"


# ------------------------------------------------------------------------------------------------------------ inputs
def family_rows(rows, cols, g, first=0):
    """fp32 [rows, cols]: row r belongs to family FAMILIES[(r + first) % 6]"""
    x = torch.empty(rows, cols, dtype=torch.float32)
    for r in range(rows):
        fam = FAMILIES[(r + first) % len(FAMILIES)]
        n = torch.randn(cols, generator=g)
        if fam == "normal":
            v = 2 * n + 0.5
        elif fam == "offset":
            v = 64 + n
        elif fam == "tight":
            v = 1 + 1e-3 * n
        elif fam == "large":
            v = 1e4 * n
        elif fam == "outlier":
            v = 2 * n + 0.5
            v[3] = 300.0
        else:
            v = torch.full((cols,), 0.5)
        x[r] = v
    return x


def family_of(rows, first=0):
    return [FAMILIES[(r + first) % len(FAMILIES)] for r in range(rows)]


def side_index(rows, side):
    """(is_side [rows] bool, sidx [rows]) of xp_layernorm_fwd_side's row -> side row map"""
    S, M, stride = side
    r = torch.arange(rows)
    return (r % S) < M, (r // S) * stride + r % S


def build(case):
    """CPU tensors of a case, every one in its storage type.  x / dy / dx are described as (flat buffer, offset, ld)."""
    g = torch.Generator().manual_seed(case.seed)
    rows, cols, dt = case.rows, case.cols, case.tdtype
    ldx = case.S * cols if case.form == "pooled" else cols + case.ldx_pad
    first = 0 if rows >= len(FAMILIES) else FAMILIES.index(SHORT_FIRST[cols])      # fewer rows than families: see SHORT_FIRST
    inp = {"ldx": ldx, "x_off": case.x_off, "first": first}
    xbuf = torch.randn(case.x_off + rows * ldx + 8, generator=g)            # what lies between the rows is unrelated noise
    xv = xbuf.as_strided((rows, cols), (ldx, 1), case.x_off)
    xv.copy_(family_rows(rows, cols, g, first))
    inp["xbuf"] = xbuf.to(dt)
    inp["gamma"] = 1 + 0.3 * torch.randn(cols, generator=g)
    inp["beta"] = 0.1 * torch.randn(cols, generator=g)
    if case.side:
        is_side, sidx = side_index(rows, case.side)
        n_side = int(sidx[is_side].max()) + 1 if bool(is_side.any()) else 1
        n_side = max(n_side, cdiv(rows, case.side[0]) * case.side[2])
        inp["x_side"] = family_rows(n_side, cols, g, first=1)
    if case.kind == "bwd":
        dybuf = torch.randn(rows * ldx + 8, generator=g)
        inp["dybuf"] = dybuf.to(dt)
        inp["dres"] = torch.randn(rows, cols, generator=g).to(dt) if case.dres else None
    return inp


def rows_view(buf, off, ld, rows, cols):
    return buf.as_strided((rows, cols), (ld, 1), off)


def x_as_read(case, inp):
    """fp64 [rows, cols]: the x the kernel normalises (side rows from x_side)"""
    x = rows_view(inp["xbuf"], inp["x_off"], inp["ldx"], case.rows, case.cols).double().clone()
    if case.side:
        is_side, sidx = side_index(case.rows, case.side)
        x[is_side] = inp["x_side"][sidx[is_side]].double()
    return x


# ------------------------------------------------------------------------------------------------------------ fp64 definition
def ref_fwd(x, gamma, beta, eps):
    """x fp64 [rows, cols] as read -> dict(y, mean, rstd, scale_y, scale_mean)"""
    gamma, beta = gamma.double(), beta.double()
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))      # eps reaches the kernel as a float
    y = (x - mean[:, None]) * rstd[:, None] * gamma + beta
    xmax = x.abs().amax(1)
    return {"y": y, "mean": mean, "rstd": rstd, "scale_y": rstd * xmax * gamma.abs().max() + beta.abs().max(), "scale_mean": xmax}


def ref_bwd(dy, x, gamma, mean, rstd, dres):
    """fp64 inputs as read (mean / rstd: the fp32 values given to the kernel) -> outputs and their scales"""
    gamma = gamma.double()
    mean, rstd = mean.double()[:, None], rstd.double()[:, None]
    xh = (x - mean) * rstd
    gy = dy * gamma
    c1 = gy.mean(1, keepdim=True)
    c2 = (gy * xh).mean(1, keepdim=True)
    r = torch.zeros_like(dy) if dres is None else dres.double()
    dx = rstd * (gy - c1 - xh * c2) + r
    scale_dx = (rstd * (gy.abs().amax(1, keepdim=True) + c1.abs() + xh.abs().amax(1, keepdim=True) * c2.abs()) + r.abs().amax(1, keepdim=True))[:, 0]
    out = {"dx": dx, "dgamma": (dy * xh).sum(0), "dbeta": dy.sum(0), "colsum_dx": dx.sum(0), "scale_dx": scale_dx,
           "slack_colsum_dx": (GATE_ROW * U * scale_dx.sum()).expand(dx.shape[1]),
           "scale_dgamma": (dy * xh).abs().sum(0), "scale_dbeta": dy.abs().sum(0), "scale_colsum_dx": dx.abs().sum(0)}
    if dres is not None:
        out["colsum_dres"], out["scale_colsum_dres"] = r.sum(0), r.abs().sum(0)
    return out


# ------------------------------------------------------------------------------------------------------------ metrics
def worst(out, ref, scale, bf16=False, axis=1, slack=None):
    """(worst multiple of u, its row / column).  out [rows, cols] against ref with a per-row scale (axis=1), or [cols] against a
    per-column scale (axis=0).  For a bf16 output the 2^-8 * |ref| allowance is taken off the error first; ``slack``: an absolute
    allowance per element (colsum(dx): what the dx gate allows its terms) taken off as well."""
    out, ref, scale = out.double(), ref.double(), scale.double()
    if not bool(torch.isfinite(out).all()):
        bad = (~torch.isfinite(out)).nonzero()[0]
        return math.inf, int(bad[0])
    err = (out - ref).abs()
    if bf16:
        err = (err - BF16_REL * ref.abs()).clamp_min(0)
    if slack is not None:
        err = (err - slack.double()).clamp_min(0)
    if out.dim() == 2 and axis == 1:
        err = err.amax(1)
    m = torch.where(scale > 0, err / (scale * U).clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    i = int(m.argmax())
    return float(m[i]), i


class Verdict:
    """the worst multiple of u of each metric of one case, its gate and where it was"""

    def __init__(self, case):
        self.case, self.rows = case, []

    def add(self, name, out, ref, scale, gate, bf16=False, axis=1, slack=None):
        m, i = worst(out, ref, scale, bf16, axis, slack)
        raw = m if slack is None else worst(out, ref, scale, bf16, axis)[0]          # before the allowance: logged, not gated
        self.rows.append((name, m, gate * (1.01 if bf16 else 1.0), i, raw))

    def require(self, name, ok, what):
        self.rows.append((name, 0.0 if ok else math.inf, 0.0, what, 0.0 if ok else math.inf))

    @property
    def failed(self):
        return [r for r in self.rows if not r[1] <= r[2]]

    def lines(self):
        return [f"{self.case.id} {n}: {m:.3g} u (gate {g:.4g} u{'' if raw == m else f'; {raw:.3g} u before the dx-gate allowance'}) at {i} "
                f"{'OK' if m <= g else 'FAIL'}" for n, m, g, i, raw in self.rows]

    def worst_by_group(self, into):
        """fold this case into {(kernel group, metric): (multiple of u before any allowance, gate in u, case id)}, keeping the entry
        that is nearest to its gate"""
        grp = self.case.kernel.split("<")[0] + ("<bf16_t>" if self.case.kind == "fwd" and self.case.kernel == "ln_fwd_kernel<bf16_t>" else
                                                "<float>" if self.case.kernel == "ln_fwd_kernel<float>" else "")
        for n, m, g, _, raw in self.rows:
            if g > 0:
                key = (grp, n.replace("partial rows ", ""))
                if key not in into or raw / g > into[key][0] / into[key][1]:
                    into[key] = (raw, g, self.case.id)
        return into

    def assert_ok(self):
        assert not self.failed, "\n".join(self.lines())


def judge_fwd(case, inp, out, v=None):
    """out: dict(y [rows, cols], mean, rstd, optional y_side [n_side, cols]) in the kernel's output types"""
    v = v or Verdict(case)
    ref = ref_fwd(x_as_read(case, inp), inp["gamma"], inp["beta"], case.eps)
    bf = case.dtype == "bf16"
    v.add("y", out["y"], ref["y"], ref["scale_y"], GATE_ROW, bf)
    v.add("mean", out["mean"][:, None], ref["mean"][:, None], ref["scale_mean"], GATE_ROW)
    v.add("rstd", out["rstd"][:, None], ref["rstd"][:, None], ref["rstd"], GATE_ROW)
    fam = family_of(case.rows, inp["first"])
    const = torch.tensor([f == "const" for f in fam])
    if case.side:
        is_side, sidx = side_index(case.rows, case.side)
        sfam = family_of(inp["x_side"].shape[0], 1)
        for r in range(case.rows):
            if bool(is_side[r]):
                const[r] = sfam[int(sidx[r])] == "const"
        if out.get("y_side") is not None:
            ys = out["y_side"]
            rs = is_side.nonzero()[:, 0]
            v.add("y_side", ys[sidx[rs]], ref["y"][rs], ref["scale_y"][rs], GATE_ROW)            # fp32: held to the fp32 gate
            touched = torch.zeros(ys.shape[0], dtype=torch.bool)
            touched[sidx[rs]] = True
            v.require("y_side untouched rows keep their NaN fill", bool(torch.isnan(ys[~touched]).all()), "side rows")
            v.require("y == bf16(y_side) on side rows", torch.equal(out["y"][rs], ys[sidx[rs]].to(out["y"].dtype)), "side rows")
    if bool(const.any()):                                                           # constant rows of 0.5: exact statistics
        v.require("constant rows: mean == 0.5", bool((out["mean"][const] == 0.5).all()), "const rows")
        want = inp["beta"].to(case.tdtype).expand(int(const.sum()), -1)
        v.require("constant rows: y == beta bit for bit", torch.equal(out["y"][const], want), "const rows")
        r0 = 1.0 / math.sqrt(case.eps)
        v.require("constant rows: rstd within 4 u of 1/sqrt(eps)",
                  bool(((out["rstd"][const].double() - r0).abs() <= 4 * U * r0).all()), "const rows")
    return v


def judge_bwd(case, inp, mean, rstd, out, v=None, accumulated=0.0):
    """out: dict(dx, and any of part [nrows, pitch], dgamma, dbeta, colsum_dx, colsum_dres); ``accumulated``: what the flushed
    outputs held before (accumulate form)"""
    v = v or Verdict(case)
    rows, cols = case.rows, case.cols
    ld = inp["ldx"]
    dy = rows_view(inp["dybuf"], 0, ld, rows, cols).double()
    ref = ref_bwd(dy, x_as_read(case, inp), inp["gamma"], mean, rstd, inp["dres"])
    v.add("dx", out["dx"], ref["dx"], ref["scale_dx"], GATE_ROW, case.dtype == "bf16")
    names = ["dgamma", "dbeta", "colsum_dx", "colsum_dres"][:2 + case.mode]
    if out.get("part") is not None:
        part = out["part"].double()
        for q, n in enumerate(names):
            v.add(f"partial rows {n}", part[:, q * cols:(q + 1) * cols].sum(0), ref[n], ref["scale_" + n], col_gate(rows), axis=0,
                  slack=ref.get("slack_" + n))
    for n in names:
        if out.get(n) is not None:
            v.add(n, out[n], ref[n] + accumulated, ref["scale_" + n] + abs(accumulated), col_gate(rows), axis=0, slack=ref.get("slack_" + n))
    if case.dtype == "f32" and case.mode >= 1:
        # fp32 stores the very `o` it adds: against the fp64 column sums of the STORED dx the summation alone is measured, at
        # (rows + 8) u of sum|dx| with no allowance, whatever the row statistics did to the terms
        stored = out["dx"].double()
        for n, got in (("partial rows colsum_dx", out["part"].double()[:, 2 * cols:3 * cols].sum(0) if out.get("part") is not None else None),
                       ("colsum_dx", out.get("colsum_dx"))):
            if got is not None:
                v.add(n + " vs stored dx", got, stored.sum(0), stored.abs().sum(0), col_gate(rows), axis=0)
    return v


# ------------------------------------------------------------------------------------------------------------ float32 emulation
def _f32(x):
    return torch.tensor(x, dtype=torch.float32)


def _butterfly(v):
    """v [rows, L] (L = 64: wave_sum, L = 32: half_sum) -> [rows]; xor butterfly from L/2 down to 1"""
    L = v.shape[1]
    idx = torch.arange(L)
    o = L // 2
    while o:
        v = v + v[:, idx ^ o]
        o >>= 1
    return v[:, 0]


def _pad(x, nj):
    p = torch.zeros(x.shape[0], nj * 256, dtype=torch.float32)
    p[:, :x.shape[1]] = x
    return p


def fwd_grid_rows(rows, half):
    """rows one grid-stride iteration of the forward covers"""
    return min(cdiv(rows, 8), 2048) * 8 if half else min(cdiv(rows, 4), 4096) * 4


def emu_fwd(case, inp, mutant=None):
    """float32 emulation of xp_layernorm_fwd_side with the kernel's summation shape: lane-strided partial sums, then the butterfly,
    for the wave-per-row (64 lanes x 4 elements per slab) and the half-wave (32 lanes x 8) layout.  Rows a (mutated) kernel does not
    process keep a NaN fill.  -> dict(y, mean, rstd, y_side)"""
    rows, cols, dt = case.rows, case.cols, case.tdtype
    half = case.kernel.startswith("ln_fwd_h_kernel")
    ldx = cols if mutant == "ld_ignored" else inp["ldx"]
    x = rows_view(inp["xbuf"], inp["x_off"], ldx, rows, cols).float().clone()
    if case.side and mutant != "side_from_x":
        is_side, sidx = side_index(rows, case.side)
        x[is_side] = inp["x_side"][sidx[is_side]]
    nj = cdiv(cols, 256)
    L, E = (32, 8) if half else (64, 4)
    mask = torch.zeros(nj * 256, dtype=torch.float32)
    mask[:cols] = 1
    if mutant == "skip_tail4" and cols % 256:
        mask[cols - 4:cols] = 0
    vv = _pad(x, nj).view(rows, nj, L, E)
    mm = mask.view(nj, L, E)
    s = torch.zeros(rows, L)
    for j in range(nj):
        t = vv[:, j] * mm[j]
        if half:
            s = s + ((((t[..., 0] + t[..., 1]) + (t[..., 2] + t[..., 3])) + (t[..., 4] + t[..., 5])) + (t[..., 6] + t[..., 7]))
        else:
            s = s + (((t[..., 0] + t[..., 1]) + t[..., 2]) + t[..., 3])
    inv = _f32(1.0) / _f32(float(cols))
    mu = _butterfly(s) * inv
    q = torch.zeros(rows, L)
    for j in range(nj):
        d = (vv[:, j] if mutant == "var_e2" else vv[:, j] - mu[:, None, None]) * mm[j]
        if half:
            for e in range(4):
                q = q + (d[..., e] * d[..., e] + d[..., 4 + e] * d[..., 4 + e])
        else:
            for e in range(4):
                q = q + d[..., e] * d[..., e]
    var = _butterfly(q) * (_f32(1.0) / _f32(float(cols - 1)) if mutant == "var_unbiased" else inv)
    if mutant == "var_e2":
        var = var - mu * mu
    eps = _f32(case.eps)
    rs = 1.0 / (torch.sqrt(var) + eps) if mutant == "eps_outside" else 1.0 / torch.sqrt(var + eps)
    o = (x - mu[:, None]) * rs[:, None] * inp["gamma"] + inp["beta"]
    done = torch.ones(rows, dtype=torch.bool)
    if mutant == "skip_last_odd_row" and rows % 2:
        done[rows - 1] = False
    if mutant == "skip_second_iteration":
        done[fwd_grid_rows(rows, half):] = False
    nan = float("nan")
    out = {"y": torch.where(done[:, None], o, _f32(nan)).to(dt), "mean": torch.where(done, mu, _f32(nan)),
           "rstd": torch.where(done, rs, _f32(nan)), "y_side": None}
    if case.side:
        is_side, sidx = side_index(rows, case.side)
        ys = torch.full_like(inp["x_side"], nan)
        ys[sidx[is_side & done]] = o[is_side & done]
        out["y_side"] = ys
    return out


def emu_bwd(case, inp, mean, rstd, mutant=None, alias=False):
    """float32 emulation of ln_bwd_kernel and what finishes its partial rows: per row the lane-strided c1 / c2 sums and the butterfly;
    per wave the walk over rows wave, wave + stride, ... (two per iteration) into the dgamma / dbeta / colsum accumulators; per block
    the four-wave combine into one partial row (``bwd_blocks`` partial rows as in the source); then xp_reduce_rows_batch's order
    (deferred, pooled) or rows_reduce + ln_param_reduce2 (immediate) from tests/reduce_emulation.py.
    -> dict(dx, part, dgamma, dbeta, colsum_dx, colsum_dres)"""
    rows, cols, dt, mode = case.rows, case.cols, case.tdtype, case.mode
    ld = cols if mutant == "ld_ignored" else inp["ldx"]
    x = rows_view(inp["xbuf"], inp["x_off"], ld, rows, cols).float().clone()
    dy = rows_view(inp["dybuf"], 0, ld, rows, cols).float()
    if case.side and mutant != "side_from_x":
        is_side, sidx = side_index(rows, case.side)
        x[is_side] = inp["x_side"][sidx[is_side]]
    nj = cdiv(cols, 256)
    W = nj * 256
    xv, dv, gm = _pad(x, nj).view(rows, nj, 64, 4), _pad(dy, nj).view(rows, nj, 64, 4), _pad(inp["gamma"][None], nj).view(1, nj, 64, 4)
    rv = torch.zeros(rows, W) if inp["dres"] is None or mutant == "no_dres" else _pad(inp["dres"].float(), nj)
    rv = rv.view(rows, nj, 64, 4)
    mu, rs = mean.float()[:, None, None, None], rstd.float()[:, None, None, None]
    xh = (xv - mu) * rs
    gy = dv * gm
    g2 = dv if mutant == "c2_from_dy" else gy
    c1, c2 = torch.zeros(rows, 64), torch.zeros(rows, 64)
    for j in range(nj):
        for e in range(4):
            c1 = c1 + gy[:, j, :, e]
            c2 = c2 + g2[:, j, :, e] * xh[:, j, :, e]
    inv = _f32(1.0) / _f32(float(cols))
    c1 = (_butterfly(c1) * inv)[:, None, None, None]
    c2 = (_butterfly(c2) * inv)[:, None, None, None]
    if mutant == "no_c1":
        c1 = torch.zeros_like(c1)
    o = rs * (gy - c1 - xh * c2) + rv
    if mutant == "dres_twice_when_aliased" and alias:
        o = o + rv
    o, dgt, dbt, rvf = o.view(rows, W), (dv * xh).view(rows, W), dv.reshape(rows, W), rv.reshape(rows, W)
    dxs_t = o.to(dt).float() if mutant == "colsum_of_rounded_dx" else o
    blocks = RE.ln_bwd_blocks(rows)
    stride = blocks * 4
    NV = 2 + mode
    acc = torch.zeros(stride, NV, W)
    done = torch.zeros(rows, dtype=torch.bool)
    for k in range(cdiv(rows, stride)):                 # iteration k // 2, row k % 2 of it
        if mutant == "skip_second_iteration" and k >= 2:
            break
        r0, r1 = k * stride, min((k + 1) * stride, rows)
        if mutant == "skip_last_odd_row" and rows % 2 and r1 == rows:
            r1 -= 1
        n = r1 - r0
        if n <= 0:
            continue
        done[r0:r1] = True
        acc[:n, 0] += dgt[r0:r1]
        acc[:n, 1] += dbt[r0:r1]
        if mode >= 1:
            acc[:n, 2] += dxs_t[r0:r1]
        if mode == 2:
            acc[:n, 3] += rvf[r0:r1]
    red = acc.view(blocks, 4, NV, W)
    part = (((red[:, 0] + red[:, 1]) + red[:, 2]) + red[:, 3])[:, :, :cols].reshape(blocks, NV * cols).contiguous()
    out = {"dx": torch.where(done[:, None], o[:, :cols], _f32(float("nan"))).to(dt), "part": part}
    names = ["dgamma", "dbeta", "colsum_dx", "colsum_dres"][:NV]
    if case.form == "immediate":
        p = part[:-1] if mutant == "drop_partial_row" else part
        dg, _ = RE.ln_param_reduce(p, cols) if p.shape[0] else (torch.zeros(cols), None)
        _, db = RE.ln_param_reduce(part, cols)
        out["dgamma"], out["dbeta"] = dg, db
    else:
        for q, n in enumerate(names):
            p = part[:-1] if (mutant == "drop_partial_row" and n == "dgamma") else part
            out[n] = RE.batch_segment(p[:, q * cols:(q + 1) * cols].contiguous()) if p.shape[0] else torch.zeros(cols)
    return out


# ------------------------------------------------------------------------------------------------------------ wrong kernels
# mutant -> the id of a case in which at least one gate must fail (tests/test_layernorm_ref_cpu.py asserts it)
MUTANTS = {
    "var_e2": ("fwd", "ln_fwd_kernel<float>-37x1024"),                       # variance as E[x^2] - mean^2
    "var_unbiased": ("fwd", "ln_fwd_h_kernel<4>-37x1024"),                   # variance divided by cols - 1
    "eps_outside": ("fwd", "ln_fwd_h_kernel<2>-37x512"),                     # eps added outside the square root
    "skip_tail4": ("fwd", "ln_fwd_kernel<bf16_t>-37x260"),                   # last 4 columns of a ragged slab not in the statistics
    "skip_last_odd_row": ("fwd", "ln_fwd_h_kernel<1>-37x256"),               # last row of an odd row count
    "skip_second_iteration": ("fwd", f"ln_fwd_h_kernel<1>-{BIG}x8-grid"),    # rows of the second grid-stride iteration
    "no_c1": ("bwd", "ln_bwd_kernel<bf16_t,2,0>-37x512-deferred"),
    "c2_from_dy": ("bwd", "ln_bwd_kernel<float,4,0>-37x1024-deferred"),      # c2 from dy instead of gy
    "no_dres": ("bwd", "ln_bwd_kernel<bf16_t,1,1>-37x8-deferred"),
    "dres_twice_when_aliased": ("bwd", "ln_bwd_kernel<float,2,0>-37x260-deferred"),
    "colsum_of_rounded_dx": ("bwd", "ln_bwd_kernel<bf16_t,4,2>-37x1024-deferred"),
    "side_from_x": ("bwd", "ln_bwd_kernel<bf16_t,2,0>-5x512-pooled-side1_1_4"),
    "ld_ignored": ("bwd", "ln_bwd_kernel<bf16_t,4,0>-5x1024-pooled-side1_1_4"),
    "drop_partial_row": ("bwd", "ln_bwd_kernel<float,2,0>-600x260-immediate"),
}
# the same wrong kernels in the other direction, where they apply
MUTANTS_ALSO = {
    "skip_last_odd_row": ("bwd", "ln_bwd_kernel<float,1,0>-37x8-deferred"),
    "skip_second_iteration": ("bwd", "ln_bwd_kernel<bf16_t,3,1>-37x768-deferred"),
    "side_from_x": ("fwd", "ln_fwd_h_kernel<2>-60x512-side10_3_5"),
    "ld_ignored": ("fwd", "ln_fwd_kernel<bf16_t>-37x256-ldx+4"),
}
