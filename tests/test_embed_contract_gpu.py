"""GPU: every kernel of csrc/embed.hip against tests/embed_ref.py (index maps, ordered fp32 sums, integer bf16 rounding: torch.equal;
l2norm: fp64 with the project's tolerances), called through the C ABI, every output and workspace inside a guard buffer
(tests/guarded.py).  tests/test_embed_ref_cpu.py shows on the CPU that the references are right and that the case tables used here
tell a swapped grid, another summation order, a wrong chunk boundary, a last maximum and a truncating conversion from the real thing.

Covered (kernel: entry point, dtypes, test):
    [x] im2col_kernel<bf16_t|float>              xp_im2col              test_im2col, test_im2col_beyond_the_grid_cap (bf16)
    [x] im2col_u8_kernel<bf16_t|float>           xp_im2col_u8           test_im2col_u8 (two mean/std triples), ..._beyond_the_grid_cap (bf16)
    [x] vip_proxy_rows_kernel<bf16_t|float>      xp_vip_proxy_rows      test_proxy_rows
    [x] vip_embed_bwd_pos_kernel<bf16_t|float>   xp_vip_embed_bwd       test_vip_embed_bwd: accumulate 0 / 1, d_time present / NULL
    [x] vip_embed_bwd_time_kernel<bf16_t|float>  xp_vip_embed_bwd       test_vip_embed_bwd (workspace of exactly ..._workspace_bytes)
    [x] text_embed_fwd_kernel<bf16_t|float>      xp_text_embed_fwd      test_text_embed_fwd
    [x] text_embed_bwd_tok_kernel<bf16_t|float>  xp_text_embed_bwd      test_text_embed_bwd: accumulate 0 / 1, second column pass, chunk edges
    [x] text_embed_bwd_pos_kernel<bf16_t|float>  xp_text_embed_bwd      test_text_embed_bwd
    [x] argmax_rows_kernel                       xp_argmax_rows         test_argmax_rows
    [x] gather_rows_kernel<bf16_t|float>         xp_gather_rows         test_gather_and_scatter_rows (idx and NULL)
    [x] scatter_rows_kernel<bf16_t|float>        xp_scatter_rows        test_gather_and_scatter_rows, test_scatter_rows_beyond_the_grid_cap (bf16)
    [x] l2norm_fwd_kernel<bf16_t|float>          xp_l2norm_fwd          test_l2norm, test_l2norm_zero_row
    [x] l2norm_bwd_kernel<bf16_t|float>          xp_l2norm_bwd          test_l2norm, test_l2norm_zero_row
    [x] cast_kernel<bf16_t|float>                xp_cast                test_cast, test_cast_special_values, test_cast_subnormals
    [x] cast_back_kernel<bf16_t|float>           xp_cast_back           test_cast_back: accumulate 0 / 1
Every ordered-sum case runs twice and must give the same bits.  The refusals at the end are host checks: each is an argument error
that names its entry point and leaves every guarded output untouched, i.e. nothing was launched.  No test passes an id, index or
label outside its range: the library does not check them on the device.

Measured on the MI355X by this file:
    * xp_im2col_u8 equals the same-order numpy fp32 value ((u8 / 255) - mean) / std bit for bit, in both output types and for both
      mean/std triples: hipcc's fp32 division is correctly rounded, nothing is contracted across it;
    * xp_cast keeps fp32 subnormals: round-to-nearest-even onto the bf16 subnormals, no flush to zero."""
import ctypes as C

import pytest
import torch

from tests import embed_ref as R
from tests.gpu_util import report
from tests.guarded import Guarded

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
TOL_BWD = {BF16: 6e-3, F32: 1e-5}
I64_SENT = -0x5A5A5A5A5A5A5A5B
XP_ERR_ARG = -1
_ids = str


def _H():
    from xpretrain_amd import hip_ops as H
    return H, H.L.lib()


def _dt(dtype):
    return {BF16: 0, F32: 1}[dtype]


def _ok(rc, lib):
    assert rc == 0, lib.xp_last_error()
    torch.cuda.synchronize()


def _filled(old):
    """a guard buffer whose window holds `old` (the seeded previous contents of an accumulate destination)"""
    old2 = old.reshape(old.shape[0], -1) if old.dim() > 1 else old.reshape(1, -1)
    g = Guarded(old2.shape[0], old2.shape[1], old.dtype)
    g.mat.copy_(old2.cuda())
    return g


class GuardedI64:
    """n int64 elements between two runs of a sentinel (tests/guarded.Guarded holds bf16 and fp32 only)"""

    def __init__(self, n, lead=64):
        self.flat = torch.full((lead + n + lead,), I64_SENT, dtype=torch.int64, device="cuda")
        self.lead, self.n = lead, n
        self.win = self.flat[lead:lead + n]

    def check(self, tag, written):
        f = self.flat.cpu()
        keep = torch.cat([f[:self.lead], f[self.lead + written:]])
        assert bool((keep == I64_SENT).all()), f"{tag}: written outside the output window"


# ------------------------------------------------------------------------------------------------------------------ im2col
def _im2col(case, dtype, u8=None):
    H, lib = _H()
    BT, Hh, W, P = case
    rows, K = BT * (Hh // P) * (W // P), 3 * P * P
    g = Guarded(rows, K, dtype)
    if u8 is None:
        v = R.frames_f32(case)
        d = v.cuda()
        _ok(lib.xp_im2col(H._p(d), H._p(g.mat), BT, Hh, W, P, _dt(dtype), H._stream()), lib)
        ref = R.im2col(v, P)
    else:
        mean, std = R.NORMS[u8]
        v = R.frames_u8(case)
        d = v.cuda()
        assert d.data_ptr() % 8 == 0
        _ok(lib.xp_im2col_u8(H._p(d), (C.c_float * 3)(*mean), (C.c_float * 3)(*std), H._p(g.mat), BT, Hh, W, P, _dt(dtype), H._stream()), lib)
        ref = R.im2col(R.image_norm_u8(v, mean, std), P)
    g.check(f"im2col {case} {dtype} {u8}", rows, K)
    return g.mat.cpu(), R.store(ref, dtype)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_ids)
@pytest.mark.parametrize("case", R.IM2COL_CASES, ids=_ids)
def test_im2col(case, dtype):
    got, ref = _im2col(case, dtype)
    assert R.same(got, ref)


@pytest.mark.parametrize("norm", list(R.NORMS))
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_ids)
@pytest.mark.parametrize("case", R.IM2COL_CASES, ids=_ids)
def test_im2col_u8(case, dtype, norm):
    """bit-equal to the numpy fp32 value of ((u8 / 255) - mean[c]) / std[c], rounded once to the output type: the Makefile passes no
    fast-math flag, hipcc's fp32 division is correctly rounded and no multiply-add can be contracted across a division and a
    subtraction.  Measured on the MI355X: equal, every case, both types, both triples."""
    got, ref = _im2col(case, dtype, u8=norm)
    ne = int((got.float() != ref.float()).sum())
    print(f"im2col_u8 {case} {dtype} {norm}: {ne} of {ref.numel()} elements differ from the numpy fp32 value")
    assert R.same(got, ref)


@pytest.mark.parametrize("u8", [None, "clip"], ids=["fp32", "uint8"])
def test_im2col_beyond_the_grid_cap(u8):
    """128 frames of 224 x 224: 2.4 M eight-element vectors for 8192 x 256 threads, the grid-stride loop runs twice"""
    got, ref = _im2col(R.IM2COL_BIG, BF16, u8=u8)
    assert R.same(got, ref)


# ------------------------------------------------------------------------------------------------------------------ proxy rows
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_ids)
@pytest.mark.parametrize("case", R.PROXY_CASES, ids=_ids)
def test_proxy_rows(case, dtype):
    H, lib = _H()
    B, S, M, D = case
    cls, added, pos = R.proxy_inputs(case)
    g = Guarded(B * S, D, dtype)
    dc, da, dp = cls.cuda(), None if added is None else added.cuda(), pos.cuda()
    _ok(lib.xp_vip_proxy_rows(H._p(dc), H._p(da), H._p(dp), H._p(g.mat), B, S, M, D, _dt(dtype), H._stream()), lib)
    written = (torch.arange(B)[:, None] * S + torch.arange(M)[None]).reshape(-1).cuda()
    g.check(f"proxy rows {case}", written, D)                  # rows m >= M of every sample keep the sentinel
    assert R.same(g.mat.view(B, S, D)[:, :M].cpu(), R.store(R.proxy_rows(cls, added, pos, B, M), dtype))


# ------------------------------------------------------------------------------------------------------------------ vip_embed_bwd
def _vip_bwd(case, dx, old, accumulate, with_time):
    H, lib = _H()
    B, M, T, L, D = case
    shapes = {"d_class": (1, D), "d_added": (M - 1, D), "d_pos": (1 + L, D), "d_time": (T, D)}
    g = {}
    for k, (r, c) in shapes.items():
        if r == 0 or (k == "d_time" and not with_time):
            g[k] = None
        else:
            g[k] = _filled(old[k]) if accumulate else Guarded(r, c, F32)
    nb = lib.xp_vip_embed_bwd_workspace_bytes(B, T, L, D)
    assert nb == B * T * D * 4
    ws = Guarded(1, nb // 4, F32) if with_time else None
    ptr = {k: H._p(None if v is None else v.mat) for k, v in g.items()}
    d = dx.cuda()
    _ok(lib.xp_vip_embed_bwd(H._p(d), ptr["d_class"], ptr["d_added"], ptr["d_pos"], ptr["d_time"], B, M, T, L, D, _dt(dx.dtype),
                             int(accumulate), H._p(None if ws is None else ws.mat), nb if with_time else 0, H._stream()), lib)
    for k, v in g.items():
        if v is not None:
            v.check(f"vip_embed_bwd {case} {k}", *shapes[k])
    if ws is not None:
        ws.check(f"vip_embed_bwd {case} workspace", 1, nb // 4)
    return {k: v.mat.cpu().view(old[k].shape) for k, v in g.items() if v is not None}


@pytest.mark.parametrize("with_time", [True, False], ids=["d_time", "no_d_time"])
@pytest.mark.parametrize("accumulate", [0, 1], ids=["store", "accumulate"])
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_ids)
@pytest.mark.parametrize("case", R.VIP_BWD_CASES, ids=_ids)
def test_vip_embed_bwd(case, dtype, accumulate, with_time):
    B, M, T, L, D = case
    dx, old = R.vip_bwd_inputs(case, dtype)
    ref = R.vip_embed_bwd(dx, M, T, L, old=old if accumulate else None)
    got = _vip_bwd(case, dx, old, accumulate, with_time)
    assert set(got) == {k for k in ref if ref[k].numel() and (with_time or k != "d_time")}
    for k in got:
        assert torch.equal(got[k], ref[k]), f"{k}: {int((got[k] != ref[k]).sum())} elements differ from the ordered fp32 sum"
    again = _vip_bwd(case, dx, old, accumulate, with_time)
    assert all(R.same(again[k], got[k]) for k in got), "second run differs"


# ------------------------------------------------------------------------------------------------------------------ text embeddings
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_ids)
@pytest.mark.parametrize("case", R.TEXT_CASES, ids=_ids)
def test_text_embed_fwd(case, dtype):
    H, lib = _H()
    B, Lt, D, V = case
    inp = R.text_inputs(case, dtype)
    g = Guarded(B * Lt, D, dtype)
    ids, tok, pos = inp["ids"].cuda(), inp["tok"].cuda(), inp["pos"].cuda()
    _ok(lib.xp_text_embed_fwd(H._p(ids), H._p(tok), H._p(pos), H._p(g.mat), B, Lt, D, V, _dt(dtype), H._stream()), lib)
    g.check(f"text_embed_fwd {case}", B * Lt, D)
    assert R.same(g.mat.view(B, Lt, D).cpu(), R.store(R.text_embed(inp["ids"], inp["tok"], inp["pos"]), dtype))


def _text_bwd(case, inp, accumulate):
    H, lib = _H()
    B, Lt, D, V = case
    npos = inp["npos"]
    gt = _filled(inp["old_tok"]) if accumulate else Guarded(V, D, F32)
    gp = _filled(inp["old_pos"]) if accumulate else Guarded(npos, D, F32)
    ids, dx = inp["ids"].cuda(), inp["dx"].cuda()
    _ok(lib.xp_text_embed_bwd(H._p(ids), H._p(dx), H._p(gt.mat), H._p(gp.mat), B, Lt, D, V, _dt(dx.dtype), int(accumulate), H._stream()), lib)
    gt.check(f"text_embed_bwd {case} d_tok", V, D)
    gp.check(f"text_embed_bwd {case} d_pos", npos if accumulate else Lt, D)      # store: rows >= Lt still hold the sentinel
    return gt.mat.cpu(), gp.mat.cpu()


@pytest.mark.parametrize("accumulate", [0, 1], ids=["store", "accumulate"])
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_ids)
@pytest.mark.parametrize("case", R.TEXT_CASES, ids=_ids)
def test_text_embed_bwd(case, dtype, accumulate):
    B, Lt, D, V = case
    inp = R.text_inputs(case, dtype)
    d_tok, d_pos = _text_bwd(case, inp, accumulate)
    absent = torch.tensor([i not in set(inp["ids"].view(-1).tolist()) for i in range(V)])
    assert bool(absent.any()) or V == 1
    if accumulate:
        rt, rp = R.text_embed_bwd(inp["ids"], inp["dx"], V, old_tok=inp["old_tok"], old_pos=inp["old_pos"])
        assert R.same(d_tok[absent], inp["old_tok"][absent]), "accumulate: the rows of absent ids must keep their bits"
        assert R.same(d_pos[Lt:], inp["old_pos"][Lt:]), "accumulate: d_pos rows >= Lt must keep their bits"
    else:
        rt, rp = R.text_embed_bwd(inp["ids"], inp["dx"], V)
        assert bool((d_tok[absent].view(torch.int32) == 0).all()), "store: the rows of absent ids must be zero bits"
        d_pos = d_pos[:Lt]
    assert torch.equal(d_tok, rt), f"d_tok: rows {sorted(set((d_tok != rt).nonzero()[:, 0].tolist()))} differ from the ordered fp32 sum"
    assert torch.equal(d_pos, rp)
    t2, p2 = _text_bwd(case, inp, accumulate)
    assert R.same(t2, d_tok) and R.same(p2[:d_pos.shape[0]], d_pos), "second run differs"


# ------------------------------------------------------------------------------------------------------------------ pooling
@pytest.mark.parametrize("case", R.ARGMAX_CASES, ids=_ids)
def test_argmax_rows(case):
    H, lib = _H()
    B, Lt = case
    ids = R.argmax_ids(case)
    g = GuardedI64(B)
    d = ids.cuda()
    _ok(lib.xp_argmax_rows(H._p(d), H._p(g.win), B, Lt, H._stream()), lib)
    g.check(f"argmax {case}", B)
    assert torch.equal(g.win.cpu(), R.argmax_rows(ids))


def _gather_scatter(case, dtype, with_idx):
    H, lib = _H()
    B, S, D = case
    x, dout, idx = R.gather_inputs(case, dtype)
    idx = idx if with_idx else None
    di = None if idx is None else idx.cuda()
    go, gd = Guarded(B, D, dtype), Guarded(B * S, D, dtype)
    dx_, dd = x.cuda(), dout.cuda()
    _ok(lib.xp_gather_rows(H._p(dx_), H._p(di), H._p(go.mat), B, S, D, _dt(dtype), H._stream()), lib)
    _ok(lib.xp_scatter_rows(H._p(dd), H._p(di), H._p(gd.mat), B, S, D, _dt(dtype), H._stream()), lib)
    go.check(f"gather {case}", B, D)
    gd.check(f"scatter {case}", B * S, D)
    assert R.same(go.mat.cpu(), R.gather_rows(x, idx))
    ref = R.scatter_rows(dout, idx, S)
    got = gd.mat.view(B, S, D).cpu()
    assert R.same(got, ref)                                    # same bits: the zeros are +0
    return got


@pytest.mark.parametrize("with_idx", [True, False], ids=["idx", "NULL"])
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_ids)
@pytest.mark.parametrize("case", R.GATHER_CASES, ids=_ids)
def test_gather_and_scatter_rows(case, dtype, with_idx):
    _gather_scatter(case, dtype, with_idx)


@pytest.mark.parametrize("with_idx", [True, False], ids=["idx", "NULL"])
def test_scatter_rows_beyond_the_grid_cap(with_idx):
    """8 x 2356 x 768, the production shape: 3.6 M four-element vectors for 8192 x 256 threads"""
    got = _gather_scatter(R.SCATTER_BIG, BF16, with_idx)
    assert int((got != 0).any(-1).sum()) == R.SCATTER_BIG[0]


# ------------------------------------------------------------------------------------------------------------------ l2norm
def _l2norm(case, dtype, zero_row=False):
    H, lib = _H()
    rows, cols = case
    x, dy = R.l2norm_inputs(case, dtype, zero_row)
    gy, gi, gx = Guarded(rows, cols, F32), Guarded(1, rows, F32), Guarded(rows, cols, dtype)
    d, ddy = x.cuda(), dy.cuda()
    _ok(lib.xp_l2norm_fwd(H._p(d), H._p(gy.mat), H._p(gi.mat), rows, cols, _dt(dtype), H._stream()), lib)
    _ok(lib.xp_l2norm_bwd(H._p(ddy), H._p(gy.mat), H._p(gi.mat), H._p(gx.mat), rows, cols, _dt(dtype), H._stream()), lib)
    gy.check(f"l2norm y {case}", rows, cols)
    gi.check(f"l2norm inv {case}", 1, rows)
    gx.check(f"l2norm dx {case}", rows, cols)
    return x, dy, gy.mat.cpu(), gi.mat[0].cpu(), gx.mat.cpu()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_ids)
@pytest.mark.parametrize("case", R.L2NORM_CASES, ids=_ids)
def test_l2norm(case, dtype):
    x, dy, y, inv, dx = _l2norm(case, dtype)
    yr, ir = R.l2norm_fwd64(x)
    tag = f"l2norm {case} {dtype}"
    assert report(tag + " y", y, yr, 1e-5) <= 1e-5
    assert report(tag + " inv", inv, ir, 1e-5) <= 1e-5
    assert report(tag + " dx", dx, R.l2norm_bwd64(dy, y, inv), TOL_BWD[dtype]) <= TOL_BWD[dtype]


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_ids)
def test_l2norm_zero_row(dtype):
    """a row of zeros: inv = inf and y = NaN (include/xpretrain_hip.h; the reference's x / x.norm() gives the same); the other three
    rows of its workgroup are what they are without it"""
    x, dy, y, inv, dx = _l2norm(R.L2NORM_ZERO_ROW, dtype, zero_row=True)
    assert bool(torch.isnan(y[1]).all()) and inv[1].item() == float("inf") and bool(torch.isnan(dx[1]).all())
    keep = [0, 2, 3]
    yr, ir = R.l2norm_fwd64(x[keep])
    assert report(f"l2norm zero row {dtype} y", y[keep], yr, 1e-5) <= 1e-5
    assert report(f"l2norm zero row {dtype} inv", inv[keep], ir, 1e-5) <= 1e-5
    ref = R.l2norm_bwd64(dy[keep], y[keep], inv[keep])
    assert report(f"l2norm zero row {dtype} dx", dx[keep], ref, TOL_BWD[dtype]) <= TOL_BWD[dtype]
    _, _, y0, inv0, dx0 = _l2norm(R.L2NORM_ZERO_ROW, dtype)                       # the same case without the zero row: same bits
    assert R.same(y0[keep], y[keep]) and R.same(inv0[keep], inv[keep]) and R.same(dx0[keep], dx[keep])


# ------------------------------------------------------------------------------------------------------------------ casts
def _cast(x, dtype):
    H, lib = _H()
    n = x.numel()
    g = Guarded(1, n, dtype)
    d = x.cuda()
    _ok(lib.xp_cast(H._p(d), H._p(g.mat), n, _dt(dtype), H._stream()), lib)
    g.check(f"cast {n} {dtype}", 1, n)
    return g.mat[0].cpu()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_ids)
@pytest.mark.parametrize("n", R.CAST_N)
def test_cast(n, dtype):
    x = R.cast_input(n)
    assert R.same(_cast(x, dtype), R.store(x, dtype))


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_ids)
def test_cast_special_values(dtype):
    """ties both ways, one ulp either side, the carry into the exponent, the overflow edge, infinities, signed zeros, a NaN"""
    x = R.table_f32(R.SPECIAL)
    got = _cast(x, dtype)
    if dtype == BF16:
        want = torch.tensor([b for _, b in R.SPECIAL], dtype=torch.int32).to(torch.int16).view(BF16)
        assert R.same(R.store(x, dtype), want)
    assert R.same(got, R.store(x, dtype)), [hex(v & 0xFFFF) for v in got.view(torch.int16).tolist()] if dtype == BF16 else None


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_ids)
def test_cast_subnormals(dtype):
    """fp32 subnormals of both signs: kept, rounded to nearest even onto the bf16 subnormals like torch's CPU conversion (measured on
    the MI355X: no flush to zero; include/xpretrain_hip.h states it)"""
    x = R.table_f32(R.SUBNORMAL)
    got = _cast(x, dtype)
    print(f"cast subnormals {dtype}:", [hex(v & 0xFFFFFFFF) for v in got.view(torch.int16 if dtype == BF16 else torch.int32).tolist()])
    assert R.same(got, R.store(x, dtype))


@pytest.mark.parametrize("accumulate", [0, 1], ids=["store", "accumulate"])
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_ids)
@pytest.mark.parametrize("n", R.CAST_N + [len(R.SPECIAL)])
def test_cast_back(n, dtype, accumulate):
    H, lib = _H()
    src = R.store(R.cast_input(n), dtype)
    old = R.randn(n, seed=n + 1)
    g = _filled(old) if accumulate else Guarded(1, n, F32)
    d = src.cuda()
    _ok(lib.xp_cast_back(H._p(d), H._p(g.mat), n, _dt(dtype), accumulate, H._stream()), lib)
    g.check(f"cast_back {n} {dtype}", 1, n)
    assert R.same(g.mat[0].cpu(), R.cast_back(src, old if accumulate else None))


# ------------------------------------------------------------------------------------------------------------------ refusals
BUF = 16384                # elements of every buffer: enough for every argument set below, refused or not
OUTS = ("out_a", "out_b", "out_c", "out_d", "out_e", "ws")
# entry point -> its arguments in ABI order.  A string names a buffer of _Args, "ws_bytes" is the sizing function's value (minus
# `ws_short`), "stream" the current stream; everything else is passed as it is.
ENTRY = {
    "xp_im2col": [("video", "f32"), ("patches", "out_a"), ("BT", 1), ("H", 8), ("W", 8), ("P", 8), ("dtype", 0), ("stream", "stream")],
    "xp_im2col_u8": [("frames", "u8"), ("mean", "mean"), ("std", "std"), ("patches", "out_a"), ("BT", 1), ("H", 8), ("W", 8), ("P", 8),
                     ("dtype", 0), ("stream", "stream")],
    "xp_vip_proxy_rows": [("class_emb", "f32"), ("added_cls", "f32"), ("pos", "f32"), ("x", "out_a"), ("B", 2), ("S", 3), ("M", 2), ("D", 8),
                          ("dtype", 0), ("stream", "stream")],
    "xp_vip_embed_bwd": [("dx", "bf16"), ("d_class", "out_b"), ("d_added", "out_c"), ("d_pos", "out_d"), ("d_time", "out_e"), ("B", 2),
                         ("M", 2), ("T", 1), ("L", 1), ("D", 8), ("dtype", 0), ("accumulate", 0), ("workspace", "ws"),
                         ("workspace_bytes", "ws_bytes"), ("stream", "stream")],
    "xp_text_embed_fwd": [("ids", "ids"), ("tok", "f32"), ("pos", "f32"), ("x", "out_a"), ("B", 2), ("Lt", 2), ("D", 8), ("vocab", 4),
                          ("dtype", 0), ("stream", "stream")],
    "xp_text_embed_bwd": [("ids", "ids"), ("dx", "bf16"), ("d_tok", "out_b"), ("d_pos", "out_c"), ("B", 2), ("Lt", 2), ("D", 8), ("vocab", 4),
                          ("dtype", 0), ("accumulate", 0), ("stream", "stream")],
    "xp_argmax_rows": [("ids", "ids"), ("idx", "out_i64"), ("B", 2), ("Lt", 2), ("stream", "stream")],
    "xp_gather_rows": [("x", "bf16"), ("idx", None), ("out", "out_a"), ("B", 2), ("S", 3), ("D", 8), ("dtype", 0), ("stream", "stream")],
    "xp_scatter_rows": [("dout", "bf16"), ("idx", None), ("dx", "out_a"), ("B", 2), ("S", 3), ("D", 8), ("dtype", 0), ("stream", "stream")],
    "xp_l2norm_fwd": [("x", "bf16"), ("y", "out_b"), ("inv", "out_c"), ("rows", 2), ("cols", 8), ("dtype", 0), ("stream", "stream")],
    "xp_l2norm_bwd": [("dy", "f32"), ("y", "f32"), ("inv", "f32"), ("dx", "out_a"), ("rows", 2), ("cols", 8), ("dtype", 0), ("stream", "stream")],
    "xp_cast": [("src", "f32"), ("dst", "out_a"), ("n", 8), ("dtype", 0), ("stream", "stream")],
    "xp_cast_back": [("src", "bf16"), ("dst", "out_b"), ("n", 8), ("dtype", 0), ("accumulate", 0), ("stream", "stream")],
}
POINTERS = {e: [n for n, v in a if isinstance(v, str) and v not in ("ws_bytes", "stream")] for e, a in ENTRY.items()}


class _Args:
    """valid small arguments of every entry point; every output (and the workspace) in a guard buffer of BUF elements"""

    def __init__(self):
        self.H, self.lib = _H()
        dev = "cuda"
        self.buf = {"f32": torch.ones(BUF, device=dev), "bf16": torch.ones(BUF, dtype=BF16, device=dev),
                    "u8": torch.ones(BUF, dtype=torch.uint8, device=dev), "ids": torch.zeros(BUF, dtype=torch.int64, device=dev)}
        self.out = {"out_a": Guarded(1, BUF, BF16), **{k: Guarded(1, BUF, F32) for k in OUTS[1:]}}
        self.out_i64 = GuardedI64(BUF)
        self.mean, self.std = (C.c_float * 3)(*R.CLIP_MEAN), (C.c_float * 3)(*R.CLIP_STD)

    def call(self, entry, ws_short=0, std1=None, frames_offset=0, **over):
        names = [n for n, _ in ENTRY[entry]]
        assert set(over) <= set(names), (entry, over)
        vals = {n: over.get(n, v) for n, v in ENTRY[entry]}
        args = []
        for n in names:
            v = vals[n]
            if v == "stream" and n == "stream":
                a = self.H._stream()
            elif v == "ws_bytes":
                a = self.lib.xp_vip_embed_bwd_workspace_bytes(vals["B"], vals["T"], vals["L"], vals["D"]) - ws_short
                assert 0 <= a <= BUF * 4
            elif v in ("mean", "std"):
                a = getattr(self, v)
                if v == "std" and std1 is not None:
                    a = (C.c_float * 3)(R.CLIP_STD[0], std1, R.CLIP_STD[2])
            elif v is None and n in ("mean", "std"):
                a = None                                       # (a host pointer: ctypes passes NULL)
            elif v == "out_i64":
                a = self.H._p(self.out_i64.win)
            elif isinstance(v, str):
                t = self.buf[v] if v in self.buf else self.out[v].mat
                a = C.c_void_p(t.data_ptr() + (frames_offset if n == "frames" else 0))
            elif v is None and n in POINTERS[entry] + ["idx"]:
                a = C.c_void_p(0)
            else:
                a = v
            args.append(a)
        return getattr(self.lib, entry)(*args)

    def untouched(self, tag):
        torch.cuda.synchronize()
        for n, g in self.out.items():
            g.check(f"{tag}: {n}", 0, 0)
        self.out_i64.check(tag, 0)


def _refusals():
    out = []
    for e in ENTRY:
        out += [(e, f"NULL {n}", {n: None}) for n in POINTERS[e]]
        if any(n == "dtype" for n, _ in ENTRY[e]):
            out.append((e, "dtype=2", {"dtype": 2}))
    for e in ("xp_vip_proxy_rows", "xp_vip_embed_bwd", "xp_text_embed_fwd", "xp_text_embed_bwd", "xp_gather_rows", "xp_scatter_rows"):
        out.append((e, "D=6", {"D": 6}))
    out += [("xp_l2norm_fwd", "cols=6", {"cols": 6}), ("xp_l2norm_bwd", "cols=6", {"cols": 6}), ("xp_cast", "n=6", {"n": 6}),
            ("xp_cast_back", "n=6", {"n": 6})]
    for e in ("xp_im2col", "xp_im2col_u8"):
        out += [(e, "P=4", {"P": 4}), (e, "H=12", {"H": 12}), (e, "W=12", {"W": 12})]
    out += [("xp_im2col_u8", "std[1]=0", {"std1": 0.0}), ("xp_im2col_u8", "frames + 1 byte", {"frames_offset": 1}),
            ("xp_vip_proxy_rows", "M=4 > S=3", {"M": 4}),
            ("xp_vip_embed_bwd", "D=1028", {"D": 1028}), ("xp_vip_embed_bwd", "workspace one byte short", {"ws_short": 1}),
            ("xp_vip_embed_bwd", "dtype=2, accumulate", {"dtype": 2, "accumulate": 1}),
            ("xp_text_embed_bwd", "dtype=2, accumulate", {"dtype": 2, "accumulate": 1})]
    return out


REFUSALS = _refusals()
# the optional pointers: NULL is a valid argument, in the accepted list below, not a refusal
REFUSALS = [r for r in REFUSALS if (r[0], r[1]) not in {("xp_vip_embed_bwd", "NULL d_time")}]
ACCEPTED = [
    ("xp_vip_proxy_rows", "M=1 with NULL added_cls", {"M": 1, "added_cls": None}),
    ("xp_vip_embed_bwd", "M=1 with NULL d_added", {"M": 1, "d_added": None}),
    ("xp_vip_embed_bwd", "NULL d_time with NULL workspace", {"d_time": None, "workspace": None, "workspace_bytes": 0}),
    ("xp_gather_rows", "NULL idx", {"idx": None}), ("xp_scatter_rows", "NULL idx", {"idx": None}),
    ("xp_gather_rows", "idx", {"idx": "ids"}), ("xp_scatter_rows", "idx", {"idx": "ids"}),
]


def test_valid_arguments_are_accepted():
    """the argument sets the refusals vary are themselves accepted, and so are the valid edge arguments"""
    a = _Args()
    for e in ENTRY:
        assert a.call(e) == 0, (e, a.lib.xp_last_error())
    for e, what, kw in ACCEPTED:
        assert a.call(e, **kw) == 0, (e, what, a.lib.xp_last_error())
    torch.cuda.synchronize()
    for n, g in a.out.items():
        g.check(f"accepted calls: {n}", 1, BUF)
    a.out_i64.check("accepted calls", BUF)


@pytest.mark.parametrize("entry,what,kw", REFUSALS, ids=[f"{e}-{w}" for e, w, _ in REFUSALS])
def test_refuses(entry, what, kw):
    a = _Args()
    assert a.call(entry, **kw) == XP_ERR_ARG, f"{entry} did not refuse {what} as an argument error"
    msg = a.lib.xp_last_error().decode()
    assert msg.startswith(entry + ":") or msg.startswith(entry + "("), f"{entry} refused {what} with {msg!r}"
    a.untouched(f"{entry} {what}")
