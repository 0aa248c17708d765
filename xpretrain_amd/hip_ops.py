"""Tensor-level wrappers over the C ABI (no autograd here -- see ``functional.py``).

Every function takes CUDA(HIP) tensors, allocates outputs with torch (device memory is
PyTorch's job), passes raw ``data_ptr()``s plus the current HIP stream to
``libxpretrain_hip.so`` and raises ``RuntimeError`` with ``xp_last_error()`` on failure.
Nothing here computes with torch ops.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
from typing import NamedTuple, Optional

import torch

from . import _lib as L

_DT = {torch.bfloat16: L.XP_BF16, torch.float32: L.XP_F32}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t: Optional[torch.Tensor]):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _dt(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"unsupported dtype {t.dtype}; xpretrain_amd computes in bfloat16 or float32")


def _chk(t: torch.Tensor, name: str, dtype=None):
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor -- xpretrain_amd has no CPU path")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    return t


_ws_cache = {}


def workspace(nbytes: int, device, tag: str = "ws") -> torch.Tensor:
    """Grow-only per-(device, stream, tag) scratch buffer.  Kernels on one stream execute in
    order, so consecutive users of the same tag never overlap."""
    key = (device.index if device.index is not None else torch.cuda.current_device(),
           torch.cuda.current_stream().cuda_stream, tag)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


# --------------------------------------------------------------------------------------- GEMM
def _gemm_desc(M, N, K, in_dtype, out_dtype, a_kstrided=False, b_kstrided=False, *, lda=None, ldb=None, ldc=None, ldr=None, ldaux=None,
               epilogue=L.EPI_NONE, split_k=1, a_remap=(0, 0, 0), c_remap=(0, 0, 0), scale=1.0, scale_cols=0) -> L.XpGemmDesc:
    """An XpGemmDesc without operands: shape, layouts, dtype codes, epilogue, split, row remaps -- and THE leading-dimension defaults
    (an operand's extent along its contiguous dimension; N for the output, resid and aux)."""
    d = L.XpGemmDesc()
    d.M, d.N, d.K = M, N, K
    d.lda = lda if lda is not None else (M if a_kstrided else K)
    d.ldb = ldb if ldb is not None else (N if b_kstrided else K)
    d.ldc, d.ldr, d.ldaux = (N if v is None else v for v in (ldc, ldr, ldaux))
    d.a_kstrided, d.b_kstrided = int(a_kstrided), int(b_kstrided)
    d.in_dtype, d.out_dtype = in_dtype, out_dtype
    d.epilogue, d.split_k = epilogue, split_k
    d.a_grp, d.a_grp_stride, d.a_off = a_remap
    d.c_grp, d.c_grp_stride, d.c_off = c_remap
    d.scale, d.scale_cols = float(scale), scale_cols
    return d


def gemm(A: torch.Tensor, B: torch.Tensor, M: int, N: int, K: int, *, lda=None, ldb=None, out=None, ldc=None,
         a_kstrided=False, b_kstrided=False, out_dtype=None, epilogue=L.EPI_NONE, bias=None, scale=1.0,
         scale_cols=0, resid=None, ldr=None, aux=None, ldaux=None, tab1=None, tab2=None, tab_L=0,
         a_remap=(0, 0, 0), c_remap=(0, 0, 0), split_k=1, out_rows=None, colsum_defer=None, colsum_name="gemm_colsum",
         colsum_out=None, resid_side=None, out_side=None, side=None, frames=None, frame_patch=0, frame_norm=None, plan_only=False,
         m_tiles=None, k_tiles=None, k_tile_begin=None):
    """C[M,N] = epilogue(sum_k A(m,k) B(n,k)); see include/xpretrain_hip.h::XpGemmDesc.

    ``plan_only``: launch nothing and return the plan xp_gemm would launch for this call's descriptor (``gemm_plan_of``).

    ``frames`` ([BT,3,H,W] fp32 or uint8, contiguous) with ``frame_patch`` = P: A is the patch matrix of the frames, gathered by the
    operand loader (no im2col pass; pass ``A=None``); uint8 frames need ``frame_norm = (mean3, std3)``.

    ``m_tiles`` / ``k_tiles`` + ``k_tile_begin`` (sequences of int; XpGemmDesc's tile lists): uploaded per call -- the test and tool
    interface of the lists (the layer backward keeps device copies per shape, functional._dx3_support).

    ``colsum_defer`` (a DeferredReduce): also return the column sums of C (a bias gradient), as ``(C, colsum)``; the
    sums come out of the GEMM epilogue where the library supports it, otherwise from a separate pass over C; either
    way they are final only after ``colsum_defer.flush()``; written to ``colsum_out`` if given."""
    if frames is not None:
        _chk(frames, "frames"); _chk(B, "B", torch.bfloat16)
        if A is not None or frames.dim() != 4 or frames.shape[1] != 3 or not frames.is_contiguous() or \
                frames.dtype not in (torch.float32, torch.uint8) or (frames.dtype == torch.uint8 and frame_norm is None):
            raise TypeError("gemm: frames must be a contiguous [BT,3,H,W] fp32 / uint8 (with frame_norm) tensor and A must be None")
        A = B                                          # (dtype / device of the compute path; the descriptor's A stays NULL)
    else:
        _chk(A, "A"); _chk(B, "B", A.dtype)
    out_dtype = out_dtype or A.dtype
    if split_k > 1:
        out = torch.empty((split_k, M, N), dtype=torch.float32, device=A.device) if out is None else out
        out_dtype = torch.float32
    elif out is None:
        out = torch.empty((out_rows or M, N), dtype=out_dtype, device=A.device)
    d = _gemm_desc(M, N, K, _dt(A), _DT[out_dtype], a_kstrided, b_kstrided, lda=lda, ldb=ldb, ldc=ldc, ldr=ldr, ldaux=ldaux,
                   epilogue=epilogue, split_k=split_k, a_remap=a_remap, c_remap=c_remap, scale=scale, scale_cols=scale_cols)
    d.A, d.B, d.C = (0 if frames is not None else A.data_ptr()), B.data_ptr(), out.data_ptr()
    if frames is not None:
        d.a_frames, d.a_frames_u8 = frames.data_ptr(), int(frames.dtype == torch.uint8)
        d.fr_H, d.fr_W, d.fr_P = frames.shape[2], frames.shape[3], int(frame_patch)
        if frame_norm is not None:
            for c in range(3):
                d.fr_mean[c], d.fr_std[c] = float(frame_norm[0][c]), float(frame_norm[1][c])
    d.bias = 0 if bias is None else _chk(bias, "bias", torch.float32).data_ptr()
    d.resid = 0 if resid is None else _chk(resid, "resid", A.dtype).data_ptr()
    d.aux = 0 if aux is None else _chk(aux, "aux", out_dtype).data_ptr()       # BIAS_GELU without aux: forward-only
    d.tab1 = 0 if tab1 is None else _chk(tab1, "tab1", torch.float32).data_ptr()
    d.tab2 = 0 if tab2 is None else _chk(tab2, "tab2", torch.float32).data_ptr()
    d.tab_L = tab_L
    if resid_side is not None or out_side is not None:       # fp32 side rows of the residual stream: side = (S, M)
        _chk(resid_side, "resid_side", torch.float32); _chk(out_side, "out_side", torch.float32)
        S_, M_ = side
        need = ((M - 1) // S_ * M_ + min(M_, S_)) * N
        if not (resid_side.is_contiguous() and out_side.is_contiguous()) or resid_side.numel() < need or out_side.numel() < need:
            raise ValueError("gemm: resid_side / out_side are too small or not contiguous")
        d.resid_side, d.out_side, d.side_S, d.side_M = resid_side.data_ptr(), out_side.data_ptr(), S_, M_
    lists = [None if v is None else torch.tensor(list(v), dtype=torch.int32, device=B.device) for v in (m_tiles, k_tiles, k_tile_begin)]
    if m_tiles is not None:
        d.m_tiles, d.n_m_tiles = lists[0].data_ptr(), lists[0].numel()
    if k_tiles is not None or k_tile_begin is not None:
        if k_tiles is None or k_tile_begin is None or len(k_tile_begin) != max(split_k, 1) + 1:
            raise ValueError("gemm: k_tiles and k_tile_begin go together, k_tile_begin with split_k + 1 entries")
        begin_host = (C.c_int32 * len(k_tile_begin))(*k_tile_begin)
        d.k_tiles, d.k_tile_begin, d.k_tile_begin_host = lists[1].data_ptr(), lists[2].data_ptr(), C.addressof(begin_host)
    if plan_only:
        if colsum_defer is not None and L.lib().xp_gemm_colsum_rows(C.byref(d)) > 0:
            d.colsum_partials = 1          # (the planner reads the pointer only as present / absent)
        return gemm_plan_of(d)
    nrows = L.lib().xp_gemm_colsum_rows(C.byref(d)) if colsum_defer is not None else 0
    if nrows:
        part = colsum_defer.slot(nrows * N * 4, colsum_name)
        d.colsum_partials = part.data_ptr()
    L.check(L.lib().xp_gemm(C.byref(d), _stream()), "xp_gemm")
    if colsum_defer is None:
        return out
    if not nrows:
        return out, colsum_deferred(out, M, N, colsum_defer, ldx=d.ldc, name=colsum_name, out=colsum_out)
    cs = torch.empty(N, dtype=torch.float32, device=A.device) if colsum_out is None else colsum_out
    colsum_defer.add(part, 0, cs, nrows, N, N)
    return out, cs


def gemm_plan_of(d: L.XpGemmDesc) -> dict:
    """The plan xp_gemm launches for descriptor ``d`` (xp_debug_gemm_plan: host only, nothing launched) as a dict of the
    XpGemmPlanInfo fields."""
    info = L.XpGemmPlanInfo()
    L.check(L.lib().xp_debug_gemm_plan(C.byref(d), C.byref(info)), "xp_debug_gemm_plan")
    return {f: (tuple(getattr(info, f)) if f == "grid" else getattr(info, f)) for f, _ in info._fields_ if f != "reserved"}


def gemm_plan(M: int, N: int, K: int, dtype: torch.dtype, *, a_kstrided=False, b_kstrided=False, split_k=1, epilogue=L.EPI_NONE,
              colsum=False) -> dict:
    """The plan (gemm_plan_of) of a dense-operand problem described by its shape alone: no tensors, nothing launched.  ``colsum``: with
    fused column sums where the library offers them.  Split-K problems write fp32 slabs, the others the compute dtype."""
    d = _gemm_desc(M, N, K, _DT[dtype], _DT[torch.float32 if split_k > 1 or (a_kstrided and b_kstrided) else dtype], a_kstrided, b_kstrided,
                   epilogue=epilogue, split_k=split_k)
    d.resid = int(epilogue in L.EPI_ACT_BWD)       # (the planner reads these pointers only as present / absent)
    if colsum and L.lib().xp_gemm_colsum_rows(C.byref(d)) > 0:
        d.colsum_partials = 1
    return gemm_plan_of(d)


def gemm_auto_split(M: int, N: int, K: int, dtype: torch.dtype, *, a_kstrided=True, b_kstrided=True, lda=None,
                    ldb=None, a_remap=(0, 0, 0), slack=False) -> int:
    """Split-K factor for a weight-gradient GEMM (see include/xpretrain_hip.h::xp_gemm_auto_split / _slack)."""
    d = _gemm_desc(M, N, K, _DT[dtype], L.XP_F32, a_kstrided, b_kstrided, lda=lda, ldb=ldb, a_remap=a_remap)
    return int((L.lib().xp_gemm_auto_split_slack if slack else L.lib().xp_gemm_auto_split)(C.byref(d)))


def layer_bwd_gemms(dims: L.XpLayerDims, pooled=False) -> list:
    """The GEMMs of a layer backward for ``dims`` as the native call describes, sizes and launches them (xp_debug_layer_bwd_gemms: host
    only, nothing launched): XpGemmDesc's without operands, indexed by L.XP_LAYER_GEMM_*, each weight gradient at its split."""
    out = (L.XpGemmDesc * L.XP_LAYER_GEMM_MAX)()
    n = L.lib().xp_debug_layer_bwd_gemms(C.byref(dims), int(pooled), out, len(out))
    L.check(min(n, 0), "xp_debug_layer_bwd_gemms")
    return list(out[:n])


def splitk_reduce(slabs: torch.Tensor, out: torch.Tensor, accumulate=False, splits=None) -> torch.Tensor:
    n = out.numel()
    if splits is None:
        if slabs.dtype != torch.float32:
            raise TypeError("splitk_reduce: pass `splits` explicitly when the slab buffer is an untyped workspace")
        splits = slabs.numel() // n
    L.check(L.lib().xp_splitk_reduce(_p(slabs), _p(out), n, splits, int(accumulate), _stream()),
            "xp_splitk_reduce")
    return out


def colsum(X: torch.Tensor, rows: int, cols: int, ldx=None, out=None, accumulate=False) -> torch.Tensor:
    _chk(X, "X")
    out = torch.empty(cols, dtype=torch.float32, device=X.device) if out is None else out
    nb = L.lib().xp_colsum_workspace_bytes(rows, cols)
    ws = workspace(nb, X.device, "colsum")
    L.check(L.lib().xp_colsum(_p(X), rows, cols, ldx or cols, _dt(X), _p(out), int(accumulate), _p(ws), ws.numel(),
                              _stream()), "xp_colsum")
    return out


class DeferredReduce:
    """Collects the second-level reductions of several bias / LayerNorm-parameter gradients and finishes them in two
    launches (xp_reduce_rows_batch).  Each deferred producer keeps its partial rows in its own workspace slot."""

    def __init__(self, device):
        self.device = device
        self.segs = []
        self._keep = []
        self._names = set()

    def add(self, part: torch.Tensor, part_offset: int, out: torch.Tensor, nrows: int, width: int, stride: int,
            accumulate=False):
        sg = L.XpReduceSeg()
        sg.in_ = part.data_ptr() + 4 * part_offset
        sg.out = out.data_ptr()
        sg.stride, sg.nrows, sg.width, sg.accumulate = stride, nrows, width, int(accumulate)
        self.segs.append(sg)
        self._keep.append((part, out))

    def slot(self, nbytes: int, name: str) -> torch.Tensor:
        """partial-row buffer of the producer called `name` (one slot per producer NAME: reordering the producers of a
        layer cannot alias two live partial buffers)"""
        if name in self._names:
            raise RuntimeError(f"DeferredReduce: two producers named {name!r} before flush()")
        self._names.add(name)
        return workspace(nbytes, self.device, "defer:" + name)

    def flush(self):
        if not self.segs:
            return
        lib = L.lib()
        for i in range(0, len(self.segs), L.XP_REDUCE_MAX_SEGS):
            chunk = self.segs[i:i + L.XP_REDUCE_MAX_SEGS]
            arr = (L.XpReduceSeg * len(chunk))(*chunk)
            nb = lib.xp_reduce_rows_batch_workspace_bytes(arr, len(chunk))
            ws = workspace(nb, self.device, "reduce_batch")
            L.check(lib.xp_reduce_rows_batch(arr, len(chunk), _p(ws), ws.numel(), _stream()), "xp_reduce_rows_batch")
        self.segs, self._keep, self._names = [], [], set()


def colsum_deferred(X: torch.Tensor, rows: int, cols: int, defer: DeferredReduce, ldx=None, name="colsum", out=None,
                    accumulate=False) -> torch.Tensor:
    """Bias gradient whose final reduction is finished by ``defer.flush()``; written (``accumulate``: added) to the first ``cols``
    elements of ``out`` if given."""
    _chk(X, "X")
    out = torch.empty(cols, dtype=torch.float32, device=X.device) if out is None else out
    chunks = L.lib().xp_colsum_partial_rows(rows, cols)
    part = defer.slot(chunks * cols * 4, name)
    L.check(L.lib().xp_colsum_partials(_p(X), rows, cols, ldx or cols, _dt(X), _p(part), part.numel(), _stream()),
            "xp_colsum_partials")
    defer.add(part, 0, out, chunks, cols, cols, accumulate)
    return out


# --------------------------------------------------------------------------------------- LayerNorm
def layernorm_fwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, rows: int, cols: int, ldx=None,
                  eps: float = 1e-5, x_side=None, y_side=None, side=None, ldy=None, y=None, mean=None, rstd=None):
    """``side = (S, M, stride)`` with ``x_side`` / ``y_side`` (fp32 [.., cols]): rows r with r % S < M are read from x_side
    instead of x / also written in fp32 to y_side, at side row (r // S) * stride + r % S (xp_layernorm_fwd_side).
    ``y`` (row pitch ``ldy``, default cols), ``mean``, ``rstd``: the caller's output buffers."""
    _chk(x, "x"); _chk(gamma, "gamma", torch.float32); _chk(beta, "beta", torch.float32)
    ldy = ldy or cols
    if y is None:
        y = torch.empty((rows, ldy), dtype=x.dtype, device=x.device)
    else:
        _chk(y, "y", x.dtype)
        if not y.is_contiguous() or y.numel() < (rows - 1) * ldy + cols:
            raise ValueError("layernorm_fwd: y is too small or not contiguous")
    for t, nm in ((mean, "mean"), (rstd, "rstd")):
        if t is not None:
            _chk(t, nm, torch.float32)
            if not t.is_contiguous() or t.numel() < rows:
                raise ValueError(f"layernorm_fwd: {nm} is too small or not contiguous")
    mean = torch.empty(rows, dtype=torch.float32, device=x.device) if mean is None else mean
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device) if rstd is None else rstd
    if x_side is None and y_side is None:
        L.check(L.lib().xp_layernorm_fwd(_p(x), ldx or cols, _p(gamma), _p(beta), _p(y), ldy, _p(mean), _p(rstd),
                                         rows, cols, eps, _dt(x), _stream()), "xp_layernorm_fwd")
    else:
        S, M, stride = side
        for t, nm in ((x_side, "x_side"), (y_side, "y_side")):
            if t is not None:
                _chk(t, nm, torch.float32)
                if not t.is_contiguous() or t.numel() < ((rows - 1) // S * stride + min(M, S)) * cols:
                    raise ValueError(f"layernorm_fwd: {nm} is too small or not contiguous")
        L.check(L.lib().xp_layernorm_fwd_side(_p(x), ldx or cols, _p(gamma), _p(beta), _p(y), ldy, _p(mean), _p(rstd),
                                              rows, cols, eps, _dt(x), _p(x_side), _p(y_side), S, M, stride, _stream()),
                "xp_layernorm_fwd_side")
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, rows, cols, *, ldx=None, lddy=None, dres=None, dx=None, lddx=None,
                  dgamma=None, dbeta=None, accumulate=False, defer: "DeferredReduce" = None, dx_colsum=False, dres_colsum=False,
                  name="ln", x_side=None, side=None, param_grads=True, lddres=None, dx_colsum_out=None, dres_colsum_out=None):
    """Returns (dx, dgamma, dbeta) -- plus colsum(dx) when ``dx_colsum``, plus colsum(dres) when ``dres_colsum`` (deferred mode only;
    written to ``dx_colsum_out`` / ``dres_colsum_out`` if given).
    ``lddres``: row pitch of ``dres`` (default cols); ``dres`` may be ``dx`` itself.
    ``x_side`` / ``side = (S, M, stride)``: the fp32 side rows of x the forward normalised (layernorm_fwd).
    ``param_grads=False`` (deferred mode, no column sums): dx only -- the pass's parameter-gradient partial rows stay in its slot
    and are not registered with ``defer`` (rows another pass has already counted): returns (dx, None, None)."""
    _chk(dy, "dy"); _chk(x, "x", dy.dtype)
    S, M, stride = side if x_side is not None else (0, 0, 0)
    if x_side is not None:
        _chk(x_side, "x_side", torch.float32)
        if not x_side.is_contiguous() or x_side.numel() < ((rows - 1) // S * stride + min(M, S)) * cols:
            raise ValueError("layernorm_bwd: x_side is too small or not contiguous")
    if not param_grads and (defer is None or dx_colsum or dres_colsum):
        raise ValueError("layernorm_bwd: param_grads=False needs a DeferredReduce and no column sums")
    dx = torch.empty((rows, cols), dtype=dy.dtype, device=dy.device) if dx is None else dx
    if param_grads:
        dgamma = torch.empty(cols, dtype=torch.float32, device=dy.device) if dgamma is None else dgamma
        dbeta = torch.empty(cols, dtype=torch.float32, device=dy.device) if dbeta is None else dbeta
    nb = L.lib().xp_layernorm_bwd_workspace_bytes(rows, cols)
    if defer is not None:     # parameter-gradient partial rows stay in their own slot until defer.flush()
        ws = defer.slot(nb, name)
        L.check(L.lib().xp_layernorm_bwd_partials_side(_p(dy), lddy or cols, _p(x), ldx or cols, _p(gamma), _p(mean), _p(rstd),
                                                       _p(dres), lddres or cols, _p(dx), lddx or cols, 2 if dres_colsum else int(dx_colsum),
                                                       rows, cols, _dt(dy), _p(x_side), S, M, stride, _p(ws), ws.numel(), _stream()),
                "xp_layernorm_bwd_partials_side")
        if not param_grads:
            return dx, None, None
        nrows = L.lib().xp_layernorm_bwd_partial_rows(rows)
        if dres_colsum and not (dx_colsum and dres is not None):
            raise ValueError("layernorm_bwd: dres_colsum needs dx_colsum and dres")
        pitch = (4 if dres_colsum else 3 if dx_colsum else 2) * cols
        defer.add(ws, 0, dgamma, nrows, cols, pitch, accumulate)
        defer.add(ws, cols, dbeta, nrows, cols, pitch, accumulate)
        if dx_colsum:
            dxs = torch.empty(cols, dtype=torch.float32, device=dy.device) if dx_colsum_out is None else dx_colsum_out
            defer.add(ws, 2 * cols, dxs, nrows, cols, pitch)
            if dres_colsum:
                drs = torch.empty(cols, dtype=torch.float32, device=dy.device) if dres_colsum_out is None else dres_colsum_out
                defer.add(ws, 3 * cols, drs, nrows, cols, pitch)
                return dx, dgamma, dbeta, dxs, drs
            return dx, dgamma, dbeta, dxs
        return dx, dgamma, dbeta
    if dx_colsum:
        raise ValueError("layernorm_bwd: dx_colsum needs a DeferredReduce")
    ws = workspace(nb, dy.device, "ln")
    L.check(L.lib().xp_layernorm_bwd_side(_p(dy), lddy or cols, _p(x), ldx or cols, _p(gamma), _p(mean), _p(rstd),
                                          _p(dres), lddres or cols, _p(dx), lddx or cols, _p(dgamma), _p(dbeta), int(accumulate),
                                          rows, cols, _dt(dy), _p(x_side), S, M, stride, _p(ws), ws.numel(), _stream()),
            "xp_layernorm_bwd_side")
    return dx, dgamma, dbeta


# --------------------------------------------------------------------------------------- probes
def probe_mfma_bf16(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    c = torch.empty((64, 4), dtype=torch.float32, device=a.device)
    L.check(L.lib().xp_probe_mfma_bf16(_p(a), _p(b), _p(c), _stream()), "xp_probe_mfma_bf16")
    return c


def probe_mfma_f32(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    c = torch.empty((64, 4), dtype=torch.float32, device=a.device)
    L.check(L.lib().xp_probe_mfma_f32(_p(a), _p(b), _p(c), _stream()), "xp_probe_mfma_f32")
    return c


def probe_tr16(data: torch.Tensor, lane_off: torch.Tensor) -> torch.Tensor:
    out = torch.empty((64, 4), dtype=torch.int16, device=data.device)
    L.check(L.lib().xp_probe_tr16(_p(data), _p(lane_off), _p(out), _stream()), "xp_probe_tr16")
    return out


# --------------------------------------------------------------------------------------- embeddings / glue
def im2col(video: torch.Tensor, P: int, dtype) -> torch.Tensor:
    """video fp32 [BT,3,H,W] -> [BT*(H/P)*(W/P), 3*P*P] in `dtype`."""
    _chk(video, "video", torch.float32)
    BT, Cc, H, W = video.shape
    assert Cc == 3 and video.is_contiguous()
    out = torch.empty((BT * (H // P) * (W // P), 3 * P * P), dtype=dtype, device=video.device)
    L.check(L.lib().xp_im2col(_p(video), _p(out), BT, H, W, P, _DT[dtype], _stream()), "xp_im2col")
    return out


# CLIP pixel statistics used by every CLIP-ViP transform (datasets/dataloader.py:212-213)
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def im2col_u8(frames: torch.Tensor, P: int, dtype, mean=CLIP_MEAN, std=CLIP_STD) -> torch.Tensor:
    """decoded uint8 frames [BT,3,H,W] -> normalised patch matrix [BT*(H/P)*(W/P), 3*P*P] in `dtype`."""
    if frames.dtype != torch.uint8 or not frames.is_cuda or not frames.is_contiguous():
        raise TypeError("im2col_u8: frames must be a contiguous uint8 tensor on the GPU (no CPU path)")
    BT, Cc, H, W = frames.shape
    assert Cc == 3
    out = torch.empty((BT * (H // P) * (W // P), 3 * P * P), dtype=dtype, device=frames.device)
    m, sd = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    L.check(L.lib().xp_im2col_u8(_p(frames), m, sd, _p(out), BT, H, W, P, _DT[dtype], _stream()), "xp_im2col_u8")
    return out


class FrameGeometry(NamedTuple):
    """XpFrameSrc's geometry fields: the source box that is resized, the size of its (never materialised) resized image, where
    the output window sits in that image, and the horizontal flip"""
    box_y: int
    box_x: int
    box_h: int
    box_w: int
    rh: int
    rw: int
    top: int = 0
    left: int = 0
    flip: int = 0


def _frames_args(what, videos, geometry, oh, ow, out):
    """the argument checks frames_resize_norm and frames_transform share: (videos, geometry per video, frames, out)"""
    videos = list(videos)
    geometry = [geometry] * len(videos) if hasattr(geometry, "box_y") else list(geometry)
    if not videos or len(geometry) != len(videos):
        raise ValueError(f"{what}: {len(videos)} videos with {len(geometry)} geometries")
    for v in videos:
        if not isinstance(v, torch.Tensor) or v.dtype != torch.uint8 or not v.is_cuda:
            raise TypeError(f"{what}: every video must be a uint8 tensor on the GPU (no CPU path)")
        if v.dim() != 4 or v.shape[3] != 3:
            raise ValueError(f"{what}: a video must be indexed [T, H, W, 3], got {tuple(v.shape)}")
    frames = sum(v.shape[0] for v in videos)
    if out is None:
        out = torch.empty((frames, 3, oh, ow), dtype=torch.float32, device=videos[0].device)
    else:
        _chk(out, "out", torch.float32)
        if tuple(out.shape) != (frames, 3, oh, ow) or not out.is_contiguous():
            raise ValueError(f"{what}: out must be a contiguous [{frames}, 3, {oh}, {ow}] tensor")
    return videos, geometry, out


def frames_resize_norm(videos, geometry, oh: int, ow: int, mean=CLIP_MEAN, std=CLIP_STD, out=None) -> torch.Tensor:
    """Decoded uint8 videos -> normalised fp32 frames [sum of T, 3, oh, ow] in video order: bicubic resize of each video's box,
    window, flip, /255, (x - mean) / std (include/xpretrain_hip.h: xp_frames_resize_norm).  ``videos``: uint8 GPU tensors indexed
    [T, H, W, 3] with ANY strides (the decoder's THWC, a ``permute``d TCHW tensor, a sliced view); ``geometry``: one FrameGeometry
    (or any object with its fields) per video, or a single one for all.  Strides and the readable extent come from each tensor's
    storage; batches beyond XP_FRAMES_MAX_VIDEOS are split into several launches."""
    videos, geometry, out = _frames_args("frames_resize_norm", videos, geometry, oh, ow, out)
    m, sd = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    done = 0
    for lo in range(0, len(videos), L.XP_FRAMES_MAX_VIDEOS):
        part = videos[lo:lo + L.XP_FRAMES_MAX_VIDEOS]
        tab = frame_table(part, geometry[lo:])
        L.check(L.lib().xp_frames_resize_norm(tab, len(part), m, sd, C.c_void_p(out.data_ptr() + done * 3 * oh * ow * 4), oh, ow,
                                              _stream()), "xp_frames_resize_norm")
        done += sum(v.shape[0] for v in part)
    return out


def _fill_frame_src(d, v, g):
    d.src, d.src_bytes = v.data_ptr(), v.untyped_storage().nbytes() - v.storage_offset()
    d.stride_t, d.stride_y, d.stride_x, d.stride_c = v.stride()
    d.T, d.H, d.W = v.shape[:3]
    d.box_y, d.box_x, d.box_h, d.box_w = g.box_y, g.box_x, g.box_h, g.box_w
    d.rh, d.rw, d.top, d.left, d.flip = g.rh, g.rw, g.top, g.left, int(bool(g.flip))


def frame_table(videos, geometry):
    """the XpFrameSrc array of one xp_frames_resize_norm call: pointer, byte strides and readable extent of each [T, H, W, 3]-indexed
    uint8 tensor, with its geometry"""
    tab = (L.XpFrameSrc * len(videos))()
    for d, v, g in zip(tab, videos, geometry):
        _fill_frame_src(d, v, g)
    return tab


class FrameTwoStage(NamedTuple):
    """XpFrameTransform's two-stage fields: the size of the (never materialised) stage-1 image the box is resized to, and the window
    of it that stage 2 resizes to FrameGeometry's (rh, rw)"""
    mid_h: int
    mid_w: int
    crop_y: int
    crop_x: int
    crop_h: int
    crop_w: int


COLOR_OPS = {"brightness": L.XP_FRAMES_COLOR_BRIGHTNESS, "saturation": L.XP_FRAMES_COLOR_SATURATION, "hue": L.XP_FRAMES_COLOR_HUE}


def frames_transform(videos, geometry, oh: int, ow: int, mean=CLIP_MEAN, std=CLIP_STD, out=None, two_stage=None,
                     color=None, antialias=False) -> torch.Tensor:
    """frames_resize_norm with a choice of filter and a colour stage (include/xpretrain_hip.h: xp_frames_transform).
    ``two_stage``: None -- the one-stage bicubic of frames_resize_norm, same bits -- or a FrameTwoStage per video (or one for all):
    box -> stage-1 image -> its crop window -> (rh, rw), both bilinear, in one launch.  ``color``: None, or per video a sequence of up
    to three ``(op, factor)`` pairs in the order of application, ``op`` one of "brightness", "saturation", "hue" (or the
    XP_FRAMES_COLOR_* value); an empty sequence leaves that video's colours alone.  Batches beyond
    XP_FRAMES_TRANSFORM_MAX_VIDEOS are split into several launches.
    ``antialias=True``: the same call through xp_frames_transform_aa -- ``F.interpolate(..., antialias=True)``, what torchvision >= 0.17
    computes: a second definition (Keys A = -0.5, a support that widens with the scale, normalised weights), not these bits.  Its
    tables live in a workspace of exactly xp_frames_transform_aa_workspace_bytes; a geometry with more than XP_FRAMES_AA_MAX_TAPS taps
    on an axis is refused."""
    videos, geometry, out = _frames_args("frames_transform", videos, geometry, oh, ow, out)
    n = len(videos)
    if two_stage is not None:
        two_stage = [two_stage] * n if hasattr(two_stage, "mid_h") else list(two_stage)
        if len(two_stage) != n:
            raise ValueError(f"frames_transform: {n} videos with {len(two_stage)} two-stage records")
    if color is not None:
        color = [tuple(c) if c is not None else () for c in color]
        if len(color) != n:
            raise ValueError(f"frames_transform: {n} videos with {len(color)} colour records")
        if any(len(c) > 3 for c in color):
            raise ValueError("frames_transform: at most three colour ops per video (brightness, saturation, hue)")
    m, sd = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    done = 0
    for lo in range(0, n, L.XP_FRAMES_TRANSFORM_MAX_VIDEOS):
        hi = min(n, lo + L.XP_FRAMES_TRANSFORM_MAX_VIDEOS)
        tab = frame_transform_table(videos[lo:hi], geometry[lo:hi], two_stage and two_stage[lo:hi], color and color[lo:hi])
        outp = C.c_void_p(out.data_ptr() + done * 3 * oh * ow * 4)
        if antialias:
            nbytes = L.lib().xp_frames_transform_aa_workspace_bytes(tab, hi - lo, oh, ow)
            ws = workspace(nbytes, out.device, "frames_aa") if nbytes else None       # (0: the call below says what is refused)
            L.check(L.lib().xp_frames_transform_aa(tab, hi - lo, m, sd, outp, oh, ow, _p(ws), nbytes, _stream()),
                    "xp_frames_transform_aa")
        else:
            L.check(L.lib().xp_frames_transform(tab, hi - lo, m, sd, outp, oh, ow, _stream()), "xp_frames_transform")
        done += sum(v.shape[0] for v in videos[lo:hi])
    return out


def frame_transform_table(videos, geometry, two_stage=None, color=None):
    """the XpFrameTransform array of one xp_frames_transform call (frame_table's fields, the filter, the colour ops)"""
    tab = (L.XpFrameTransform * len(videos))()
    for i, (e, v, g) in enumerate(zip(tab, videos, geometry)):
        _fill_frame_src(e.src, v, g)
        e.filter = L.XP_FRAMES_FILTER_BICUBIC
        if two_stage is not None:
            e.filter = L.XP_FRAMES_FILTER_BILINEAR2
            e.mid_h, e.mid_w, e.crop_y, e.crop_x, e.crop_h, e.crop_w = two_stage[i]
        ops = color[i] if color is not None else ()
        e.n_color = len(ops)
        for k, (op, factor) in enumerate(ops):
            if isinstance(op, str) and op not in COLOR_OPS:
                raise ValueError(f"frames_transform: unknown colour op {op!r} (one of {sorted(COLOR_OPS)})")
            e.color_op[k], e.color_factor[k] = COLOR_OPS[op] if isinstance(op, str) else int(op), float(factor)
    return tab


def vip_proxy_rows(class_emb, added_cls, pos, x, B, S, M, D):
    L.check(L.lib().xp_vip_proxy_rows(_p(class_emb), _p(added_cls), _p(pos), _p(x), B, S, M, D, _dt(x), _stream()),
            "xp_vip_proxy_rows")
    return x


def vip_embed_bwd(dx, B, M, T, Lp, D, want_time=True):
    dev = dx.device
    d_class = torch.empty(D, dtype=torch.float32, device=dev)
    d_added = torch.empty((max(M - 1, 1), D), dtype=torch.float32, device=dev)
    d_pos = torch.empty((1 + Lp, D), dtype=torch.float32, device=dev)
    d_time = torch.empty((T, D), dtype=torch.float32, device=dev) if want_time else None
    nb = L.lib().xp_vip_embed_bwd_workspace_bytes(B, T, Lp, D)
    ws = workspace(nb, dev, "embed")
    L.check(L.lib().xp_vip_embed_bwd(_p(dx), _p(d_class), _p(d_added), _p(d_pos), _p(d_time), B, M, T, Lp, D, _dt(dx), 0,
                                     _p(ws), ws.numel(), _stream()), "xp_vip_embed_bwd")
    return d_class, d_added[: M - 1], d_pos, d_time


def pos_grid(rows: int) -> int:
    """g0 of a position table of ``rows`` = 1 + g0*g0 rows (ValueError for any other row count)"""
    g0 = math.isqrt(max(int(rows) - 1, 0))
    if g0 < 1 or g0 * g0 != rows - 1:
        raise ValueError(f"position table has {rows} rows: not 1 + a square grid, so it cannot be resampled")
    return g0


def _pos_table(t, name, rows=None):
    _chk(t, name, torch.float32)
    if t.dim() != 2 or not t.is_contiguous() or (rows is not None and t.shape[0] != rows):
        raise ValueError(f"{name}: expected a contiguous [{'rows' if rows is None else rows}, D] fp32 table, got {tuple(t.shape)}")
    return t


def pos_resample_fwd(pos: torch.Tensor, gh: int, gw: int, out=None) -> torch.Tensor:
    """position table fp32 [1 + g0*g0, D] -> [1 + gh*gw, D]: row 0 copied, the g0 x g0 grid resampled bicubically
    (include/xpretrain_hip.h: xp_pos_resample_fwd; transformers' interpolate_pos_encoding)"""
    _pos_table(pos, "pos")
    g0, D = pos_grid(pos.shape[0]), pos.shape[1]
    if out is None:
        out = torch.empty((1 + gh * gw, D), dtype=torch.float32, device=pos.device)
    else:
        _pos_table(out, "out", 1 + gh * gw)
    L.check(L.lib().xp_pos_resample_fwd(_p(pos), _p(out), g0, gh, gw, D, _stream()), "xp_pos_resample_fwd")
    return out


def pos_resample_bwd(d_out: torch.Tensor, g0: int, gh: int, gw: int, d_pos=None) -> torch.Tensor:
    """the transpose: d_out fp32 [1 + gh*gw, D] -> d_pos fp32 [1 + g0*g0, D], fixed summation order"""
    _pos_table(d_out, "d_out", 1 + gh * gw)
    D = d_out.shape[1]
    if d_pos is None:
        d_pos = torch.empty((1 + g0 * g0, D), dtype=torch.float32, device=d_out.device)
    else:
        _pos_table(d_pos, "d_pos", 1 + g0 * g0)
    L.check(L.lib().xp_pos_resample_bwd(_p(d_out), _p(d_pos), g0, gh, gw, D, _stream()), "xp_pos_resample_bwd")
    return d_pos


def text_embed_fwd(ids, tok, pos, dtype):
    _chk(ids, "ids", torch.int64)
    B, Lt = ids.shape
    vocab, D = tok.shape
    x = torch.empty((B * Lt, D), dtype=dtype, device=ids.device)
    L.check(L.lib().xp_text_embed_fwd(_p(ids), _p(tok), _p(pos), _p(x), B, Lt, D, vocab, _DT[dtype], _stream()),
            "xp_text_embed_fwd")
    return x


def text_embed_bwd(ids, dx, vocab, npos):
    B, Lt = ids.shape
    D = dx.shape[-1]
    d_tok = torch.empty((vocab, D), dtype=torch.float32, device=dx.device)
    d_pos = torch.zeros((npos, D), dtype=torch.float32, device=dx.device)
    L.check(L.lib().xp_text_embed_bwd(_p(ids), _p(dx), _p(d_tok), _p(d_pos), B, Lt, D, vocab, _dt(dx), 0, _stream()),
            "xp_text_embed_bwd")
    return d_tok, d_pos


def _pos_ids(pos_ids, B, Lt):
    """pos_ids as the ``_pos`` entries read them: a contiguous int64 GPU tensor [pos_B, Lt], pos_B 1 or B; returns pos_B"""
    _chk(pos_ids, "pos_ids", torch.int64)
    if pos_ids.dim() != 2 or pos_ids.shape[1] != Lt or pos_ids.shape[0] not in (1, B) or not pos_ids.is_contiguous():
        raise ValueError(f"pos_ids must be a contiguous [1, {Lt}] or [{B}, {Lt}] tensor, got {tuple(pos_ids.shape)}")
    return pos_ids.shape[0]


def text_embed_fwd_pos(ids, pos_ids, tok, pos, dtype):
    """text_embed_fwd with caller-given position ids [1 | B, Lt] (xp_text_embed_fwd_pos): a row whose id is outside the table is NaN"""
    _chk(ids, "ids", torch.int64)
    B, Lt = ids.shape
    pos_B = _pos_ids(pos_ids, B, Lt)
    vocab, D = tok.shape
    x = torch.empty((B * Lt, D), dtype=dtype, device=ids.device)
    L.check(L.lib().xp_text_embed_fwd_pos(_p(ids), _p(pos_ids), pos_B, _p(tok), _p(pos), _p(x), B, Lt, D, vocab, pos.shape[0],
                                          _DT[dtype], _stream()), "xp_text_embed_fwd_pos")
    return x


def text_embed_bwd_pos(ids, pos_ids, dx, vocab, npos):
    """(d_tok [vocab, D], d_pos [npos, D]) of text_embed_fwd_pos (xp_text_embed_bwd_pos): ordered fp32 sums, every row written"""
    _chk(ids, "ids", torch.int64)
    B, Lt = ids.shape
    pos_B = _pos_ids(pos_ids, B, Lt)
    D = dx.shape[-1]
    d_tok = torch.empty((vocab, D), dtype=torch.float32, device=dx.device)
    d_pos = torch.empty((npos, D), dtype=torch.float32, device=dx.device)
    L.check(L.lib().xp_text_embed_bwd_pos(_p(ids), _p(pos_ids), pos_B, _p(dx), _p(d_tok), _p(d_pos), B, Lt, D, vocab, npos, _dt(dx), 0,
                                          _stream()), "xp_text_embed_bwd_pos")
    return d_tok, d_pos


def argmax_rows(ids):
    B, Lt = ids.shape
    idx = torch.empty(B, dtype=torch.int64, device=ids.device)
    L.check(L.lib().xp_argmax_rows(_p(ids), _p(idx), B, Lt, _stream()), "xp_argmax_rows")
    return idx


def gather_rows(x, idx, B, S, D):
    out = torch.empty((B, D), dtype=x.dtype, device=x.device)
    L.check(L.lib().xp_gather_rows(_p(x), _p(idx), _p(out), B, S, D, _dt(x), _stream()), "xp_gather_rows")
    return out


def scatter_rows(dout, idx, B, S, D):
    dx = torch.empty((B * S, D), dtype=dout.dtype, device=dout.device)
    L.check(L.lib().xp_scatter_rows(_p(dout), _p(idx), _p(dx), B, S, D, _dt(dout), _stream()), "xp_scatter_rows")
    return dx


def l2norm_fwd(x, rows, cols):
    y = torch.empty((rows, cols), dtype=torch.float32, device=x.device)
    inv = torch.empty(rows, dtype=torch.float32, device=x.device)
    L.check(L.lib().xp_l2norm_fwd(_p(x), _p(y), _p(inv), rows, cols, _dt(x), _stream()), "xp_l2norm_fwd")
    return y, inv


def l2norm_bwd(dy, y, inv, rows, cols, dtype):
    _chk(dy, "dy", torch.float32)
    dx = torch.empty((rows, cols), dtype=dtype, device=dy.device)
    L.check(L.lib().xp_l2norm_bwd(_p(dy), _p(y), _p(inv), _p(dx), rows, cols, _DT[dtype], _stream()), "xp_l2norm_bwd")
    return dx


def cast(src: torch.Tensor, dtype, out=None) -> torch.Tensor:
    _chk(src, "src", torch.float32)
    out = torch.empty(src.shape, dtype=dtype, device=src.device) if out is None else out
    L.check(L.lib().xp_cast(_p(src), _p(out), src.numel(), _DT[dtype], _stream()), "xp_cast")
    return out


def cast_back(src: torch.Tensor, out=None, accumulate=False) -> torch.Tensor:
    out = torch.empty(src.shape, dtype=torch.float32, device=src.device) if out is None else out
    L.check(L.lib().xp_cast_back(_p(src), _p(out), src.numel(), _dt(src), int(accumulate), _stream()), "xp_cast_back")
    return out


# --------------------------------------------------------------------------------------- loss
@functools.lru_cache(maxsize=None)
def loss_operands(kind: int):
    """(reads img, reads cap) of an ``L.XP_LOSS_*`` kind, from the library's kind table (asked once per kind); an unknown kind is
    refused"""
    img, cap = C.c_int32(), C.c_int32()
    L.check(L.lib().xp_contrastive_loss_operands(kind, C.byref(img), C.byref(cap)), "xp_contrastive_loss_operands")
    return bool(img.value), bool(cap.value)


def contrastive_loss(kind: int, vis, txt, img=None, cap=None, *, log_scale):
    """xp_contrastive_loss: any loss of the learnable-temperature family (``L.XP_LOSS_*``) and all its gradients in one call.
    vis/txt [n,d], img/cap [m,d].  Returns (loss, d_vis, d_txt, d_img, d_cap, d_log_scale) -- fp32 device tensors, ``None``
    where the kind has no such operand (an ``img`` / ``cap`` it does not read is ignored; it goes to the library as NULL).  What
    the kind itself rules out (m != n, a missing operand, an unknown kind) is refused by the library before anything is launched."""
    kind = int(kind)
    use_img, use_cap = loss_operands(kind)
    img, cap = img if use_img else None, cap if use_cap else None
    ops = [(vis, "vis"), (txt, "txt"), (img, "img"), (cap, "cap")]
    for t, name in ops + [(log_scale, "log_scale")]:
        if t is not None:
            _chk(t, name, torch.float32)
    for t, name in ops:
        if t is not None and (t.dim() != 2 or t.shape[1] != vis.shape[-1] or not t.is_contiguous()):
            raise ValueError(f"contrastive_loss: {name} must be a contiguous [rows, {vis.shape[-1]}] matrix, got {tuple(t.shape)}")
    if txt.shape != vis.shape or (img is not None and cap is not None and img.shape != cap.shape):
        raise ValueError(f"contrastive_loss: feature shapes differ: {[None if t is None else tuple(t.shape) for t, _ in ops]}")
    n, d = vis.shape
    side = cap if cap is not None else img
    m = n if side is None else side.shape[0]
    dev = vis.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    dls = torch.empty((), dtype=torch.float32, device=dev)
    grads = [None if t is None else torch.empty_like(t) for t, _ in ops]
    nb = L.lib().xp_contrastive_loss_workspace_bytes(kind, n, m, d)
    ws = workspace(nb, dev, "loss")
    L.check(L.lib().xp_contrastive_loss(kind, _p(vis), _p(txt), _p(img), _p(cap), _p(log_scale), _p(loss), _p(grads[0]),
                                        _p(grads[1]), _p(grads[2]), _p(grads[3]), _p(dls), n, m, d, _p(ws), ws.numel(),
                                        _stream()), "xp_contrastive_loss")
    return (loss, *grads, dls)


def pair_loss(kind: int, vis, txt, *, temp=1.0, margin=0.0, max_violation=False, order_measure=False, hard_negative_num=1, bag=1):
    """xp_pair_loss: one of the four fixed-temperature losses (``L.XP_PAIR_*``) and both feature gradients in one call.
    vis [n,d], txt [n*bag,d] (``bag`` = 1 except for MIL-NCE).  Returns (loss, d_vis, d_txt) -- fp32 device tensors.  A parameter
    the kind does not read is ignored; what the kind rules out (temp <= 0, hard_negative_num outside [1, n], an unknown kind) is
    refused by the library before anything is launched."""
    kind, bag = int(kind), int(bag)
    for t, name in ((vis, "vis"), (txt, "txt")):
        _chk(t, name, torch.float32)
        if t.dim() != 2 or t.shape[1] != vis.shape[-1] or not t.is_contiguous():
            raise ValueError(f"pair_loss: {name} must be a contiguous [rows, {vis.shape[-1]}] matrix, got {tuple(t.shape)}")
    n, d = vis.shape
    if txt.shape[0] != n * bag:
        raise ValueError(f"pair_loss: txt must have n * bag = {n} * {bag} rows, got {tuple(txt.shape)}")
    prm = L.XpPairLossParams(float(temp), float(margin), int(bool(max_violation)), int(bool(order_measure)), int(hard_negative_num),
                             bag)
    dev = vis.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    dv, dt = torch.empty_like(vis), torch.empty_like(txt)
    nb = L.lib().xp_pair_loss_workspace_bytes(kind, C.byref(prm), n, d)
    ws = workspace(nb, dev, "loss")
    L.check(L.lib().xp_pair_loss(kind, C.byref(prm), _p(vis), _p(txt), _p(loss), _p(dv), _p(dt), n, d, _p(ws), ws.numel(), _stream()),
            "xp_pair_loss")
    return loss, dv, dt


def sim_matrix(a: torch.Tensor, b: torch.Tensor, out=None) -> torch.Tensor:
    """xp_sim_matrix: out[i][j] = a[i] . b[j] in fp32 of a [na, d] and b [nb, d], any device dtype (converted) and layout
    (made contiguous); ``out``: a contiguous fp32 [na, nb] buffer to write into."""
    a, b = _chk(a, "a").contiguous().float(), _chk(b, "b").contiguous().float()
    out = _dest("sim_matrix", out, "out", torch.float32, (a.shape[0], b.shape[0]), a.device)
    L.check(L.lib().xp_sim_matrix(_p(a), _p(b), _p(out), a.shape[0], b.shape[0], a.shape[1], _stream()), "xp_sim_matrix")
    return out


# --------------------------------------------------------------------------------------- attention
def _attn_ws(mode, B, H, M, N, Lp, device):
    nb = L.lib().xp_attn_workspace_bytes(mode, B, H, M, N, Lp)
    return workspace(nb, device, "attn")


def _dest(what, t, name, dtype, shape, device):
    """an attention output: a new tensor, or the caller's contiguous buffer ``t`` of that element count (any shape), viewed as ``shape``"""
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    _chk(t, name, dtype)
    if not t.is_contiguous() or t.numel() != math.prod(shape):
        raise ValueError(f"{what}: {name} must be a contiguous {dtype} tensor of {math.prod(shape)} elements")
    return t.view(shape)


def attn_fwd(qkv: torch.Tensor, B: int, S: int, H: int, *, size=None, pad_mask=None, out=None, stats=None):
    """qkv [B*S, 3*H*64] (q pre-scaled).  size=(M,N,L) selects the video-proxy pattern, otherwise the
    causal(+padding) text pattern.  Returns (out [B*S, H*64], stats [B,H,S,2]): the caller's buffers if given."""
    _chk(qkv, "qkv")
    mode = L.ATTN_PROXY if size is not None else L.ATTN_CAUSAL
    M, N, Lp = size if size is not None else (0, 1, S)
    out = _dest("attn_fwd", out, "out", qkv.dtype, (B * S, H * 64), qkv.device)
    stats = _dest("attn_fwd", stats, "stats", torch.float32, (B, H, S, 2), qkv.device)
    if pad_mask is not None:
        _chk(pad_mask, "pad_mask", torch.int64)
    ws = _attn_ws(mode, B, H, M, N, Lp, qkv.device)
    L.check(L.lib().xp_attn_fwd(_p(qkv), 3 * H * 64, _p(out), H * 64, _p(stats), _p(pad_mask), mode, B, H, S, M, N, Lp,
                                _dt(qkv), _p(ws), ws.numel(), _stream()), "xp_attn_fwd")
    return out, stats


def attn_probs(qkv: torch.Tensor, stats: torch.Tensor, B: int, S: int, H: int, *, size=None, pad_mask=None, out=None):
    """The attention weights ``attn_fwd`` never stores (xp_attn_probs), from the ``qkv`` it read, the ``stats`` it returned and the
    ``pad_mask`` it was given; fp32 whatever the storage of qkv.  Causal: ``[B,H,S,S]`` (CLIPAttention.forward's
    attn_weights_reshaped).  ``size=(M,N,L)``: ``(proxy [B,H,M,S], frame [B,H,N,L,M+L])``, forward2's second and first attn_weights
    (proxy queries over all keys; frame-n queries over [M proxies | frame n]).  ``out``: the buffer (causal) or the
    ``(proxy, frame)`` pair to write into -- contiguous fp32 tensors of those element counts, any shape; the results are views."""
    _chk(qkv, "qkv"); _chk(stats, "stats", torch.float32)
    mode = L.ATTN_PROXY if size is not None else L.ATTN_CAUSAL
    M, N, Lp = size if size is not None else (0, 1, S)
    if stats.numel() != B * H * S * 2 or not stats.is_contiguous() or not qkv.is_contiguous() or qkv.numel() != B * S * 3 * H * 64:
        raise ValueError("attn_probs: qkv must be a contiguous [B*S, 3*H*64] matrix and stats attn_fwd's contiguous [B,H,S,2]")
    if pad_mask is not None:
        _chk(pad_mask, "pad_mask", torch.int64)
    shapes = ((B, H, M, S), (B, H, N, Lp, M + Lp)) if size is not None else ((B, H, S, S),)
    outs = (out,) if isinstance(out, torch.Tensor) else tuple(out) if out is not None else (None,) * len(shapes)
    if len(outs) != len(shapes):
        raise ValueError(f"attn_probs: out must be {'the (proxy, frame) pair' if size is not None else 'one tensor'}")
    bufs = [_dest("attn_probs", t, nm, torch.float32, shp, qkv.device) for t, shp, nm in zip(outs, shapes, ("out[0]", "out[1]"))]
    frame, proxy = (bufs[1], bufs[0]) if size is not None else (bufs[0], None)
    L.check(L.lib().xp_attn_probs(_p(qkv), 3 * H * 64, _p(stats), _p(pad_mask), _p(frame), _p(proxy), mode, B, H, S, M, N, Lp,
                                  _dt(qkv), _stream()), "xp_attn_probs")
    return (proxy, frame) if size is not None else frame


def attn_plan(B: int, S: int, H: int, *, size=None, pad_mask=None, dtype=torch.bfloat16, backward=False, cus=0) -> dict:
    """The plan attn_fwd (``backward``: attn_bwd) launches for these arguments (xp_debug_attn_plan: host only, nothing launched) as
    a dict of the XpAttnPlanInfo fields, ``kernel`` by name (_lib.ATTN_KERNELS, _lib.ATTN_OPTIN_KERNELS); ``pad_mask`` counts as
    present or absent.  ``cus``
    > 0: a device of that many CUs that grants every dynamic-LDS opt-in (no GPU needed); <= 0: the current device."""
    mode = L.ATTN_PROXY if size is not None else L.ATTN_CAUSAL
    M, N, Lp = size if size is not None else (0, 1, S)
    info = L.XpAttnPlanInfo()
    L.check(L.lib().xp_debug_attn_plan(mode, B, H, S, M, N, Lp, _DT[dtype], int(pad_mask is not None), int(backward), cus,
                                       C.byref(info)), "xp_debug_attn_plan")
    plan = {f: getattr(info, f) for f, _ in info._fields_ if f != "reserved"}
    plan.update({f: tuple(plan[f]) for f in ("part", "delta", "dq", "dkv", "counter")}, kernel=L.ATTN_OPTIN_KERNELS.get(info.kernel) or L.ATTN_KERNELS[info.kernel])
    return plan


def set_attn_bwd_wide(on: bool) -> None:
    """Opt-in (default off, or XPRETRAIN_ATTN_BWD_WIDE=1; this call wins over the environment): proxy attention backwards whose
    window is wider than one LDS group (208 < M + L <= 1152, M <= 16, no padding mask, bf16) run as one persistent launch
    (attn_bwd6_kernel, plan name ``bwd6``) instead of the dQ / dKV kernel pair.  Process-global planning state, like the CU budget."""
    L.check(L.lib().xp_set_attn_bwd_wide(int(bool(on))), "xp_set_attn_bwd_wide")


def get_attn_bwd_wide() -> bool:
    return bool(L.lib().xp_get_attn_bwd_wide())


def attn_bwd(qkv, out, dout, stats, B, S, H, *, size=None, pad_mask=None, q_scale=1.0, colsum_defer=None,
             colsum_name="dbqkv", colsum_out=None):
    """dqkv; with ``colsum_defer`` (a DeferredReduce) also the column sums of dqkv (the q/k/v bias gradients) as ``(dqkv, colsum)``:
    out of the backward kernels where the library supports it, otherwise from a separate pass; final after ``flush()``; written to
    ``colsum_out`` if given."""
    mode = L.ATTN_PROXY if size is not None else L.ATTN_CAUSAL
    M, N, Lp = size if size is not None else (0, 1, S)
    dqkv = torch.empty_like(qkv)
    ws = _attn_ws(mode, B, H, M, N, Lp, qkv.device)
    nrows = int(L.lib().xp_attn_bwd_colsum_rows(mode, B, H, S, M, N, Lp, _dt(qkv))) if colsum_defer is not None else 0
    part = colsum_defer.slot(nrows * 3 * H * 64 * 4, colsum_name) if nrows else None
    L.check(L.lib().xp_attn_bwd2(_p(qkv), 3 * H * 64, _p(out), _p(dout), H * 64, _p(stats), _p(pad_mask), _p(dqkv),
                                 float(q_scale), mode, B, H, S, M, N, Lp, _dt(qkv), _p(ws), ws.numel(), _p(part), _stream()),
            "xp_attn_bwd")
    if colsum_defer is None:
        return dqkv
    if not nrows:
        return dqkv, colsum_deferred(dqkv, B * S, 3 * H * 64, colsum_defer, name=colsum_name, out=colsum_out)
    cs = torch.empty(3 * H * 64, dtype=torch.float32, device=qkv.device) if colsum_out is None else colsum_out
    colsum_defer.add(part, 0, cs, nrows, 3 * H * 64, 3 * H * 64)
    return dqkv, cs


# --------------------------------------------------------------------------------------- single-query proxy attention
def _rows_ld(t: torch.Tensor, name: str, width: int) -> int:
    """row pitch of a 2-D operand whose rows are contiguous (a column slice of a wider matrix is fine: kv = qkv[:, D:])"""
    _chk(t, name)
    if t.dim() != 2 or t.stride(1) != 1 or t.shape[1] < width:
        raise TypeError(f"{name}: expected a [rows, >= {width}] matrix with contiguous rows, got {tuple(t.shape)} strides {t.stride()}")
    return t.stride(0)


def attn_pooled_fwd(q: torch.Tensor, kv: torch.Tensor, B: int, S: int, H: int, *, out=None, stats=None):
    """Token 0 of every sample against all S keys (the pooled last layer of the video tower).  q [B, H*64] (pre-scaled), kv
    [B*S, 2*H*64] = [k | v] rows (any row pitch).  Returns (out [B, H*64], stats [B, H, 2]): the caller's buffers if given."""
    _chk(q, "q")
    ld = _rows_ld(kv, "kv", 2 * H * 64)
    if not q.is_contiguous() or tuple(q.shape) != (B, H * 64) or kv.shape[0] != B * S or kv.dtype != q.dtype:
        raise TypeError("attn_pooled_fwd: q must be a contiguous [B, H*64] matrix and kv [B*S, 2*H*64] of the same dtype")
    out = _dest("attn_pooled_fwd", out, "out", q.dtype, (B, H * 64), q.device)
    stats = _dest("attn_pooled_fwd", stats, "stats", torch.float32, (B, H, 2), q.device)
    ws = workspace(L.lib().xp_attn_pooled_workspace_bytes(B, H, S, _dt(q)), q.device, "attn_pooled")
    L.check(L.lib().xp_attn_pooled_fwd(_p(q), _p(kv), ld, _p(out), _p(stats), B, H, S, _dt(q), _p(ws), ws.numel(), _stream()),
            "xp_attn_pooled_fwd")
    return out, stats


def attn_pooled_bwd(q, kv, out, dout, stats, B, S, H, *, q_scale=1.0, dq=None, dkv=None, colsum_defer=None, colsum_name="dbkv",
                    colsum_out=None):
    """(dq [B, H*64] -- times q_scale --, dkv [B*S, 2*H*64]); with ``colsum_defer`` also the column sums of dkv (the k / v bias
    gradients, final after ``flush()``; written to ``colsum_out`` if given).  ``dq`` / ``dkv``: optional outputs with contiguous
    rows (any row pitch)."""
    ld = _rows_ld(kv, "kv", 2 * H * 64)
    if dq is None:
        dq = torch.empty_like(q)
    if dkv is None:
        dkv = torch.empty((B * S, 2 * H * 64), dtype=q.dtype, device=q.device)
    lddq, lddkv = _rows_ld(dq, "dq", H * 64), _rows_ld(dkv, "dkv", 2 * H * 64)
    for t, n in ((out, "out"), (dout, "dout")):
        _chk(t, n, q.dtype)
        if not t.is_contiguous() or t.shape != q.shape:
            raise TypeError(f"attn_pooled_bwd: {n} must be contiguous and shaped like q")
    lib = L.lib()
    ws = workspace(lib.xp_attn_pooled_workspace_bytes(B, H, S, _dt(q)), q.device, "attn_pooled")
    nrows = int(lib.xp_attn_pooled_colsum_rows(B, H, S, _dt(q))) if colsum_defer is not None else 0
    part = colsum_defer.slot(nrows * 2 * H * 64 * 4, colsum_name) if nrows else None
    L.check(lib.xp_attn_pooled_bwd(_p(q), _p(kv), ld, _p(out), _p(dout), _p(stats), _p(dq), lddq, _p(dkv), lddkv, float(q_scale),
                                   B, H, S, _dt(q), _p(ws), ws.numel(), _p(part), _stream()), "xp_attn_pooled_bwd")
    if colsum_defer is None:
        return dq, dkv
    cs = torch.empty(2 * H * 64, dtype=torch.float32, device=q.device) if colsum_out is None else colsum_out
    colsum_defer.add(part, 0, cs, nrows, 2 * H * 64, 2 * H * 64)
    return dq, dkv, cs


def attn_pooled_plan(B: int, S: int, H: int, *, dtype=torch.bfloat16, backward=False, cus=0) -> dict:
    """The plan attn_pooled_fwd (``backward``: attn_pooled_bwd) launches (xp_debug_attn_pooled_plan: host only, nothing launched) as
    a dict of the XpAttnPooledPlanInfo fields.  ``cus`` > 0: a device of that many CUs (no GPU needed); <= 0: the current device."""
    info = L.XpAttnPooledPlanInfo()
    L.check(L.lib().xp_debug_attn_pooled_plan(B, H, S, _DT[dtype], int(backward), cus, C.byref(info)), "xp_debug_attn_pooled_plan")
    plan = {f: getattr(info, f) for f, _ in info._fields_}
    plan.update({f: tuple(plan[f]) for f in ("part_ml", "part_acc", "part_dq")})
    return plan


# --------------------------------------------------------------------------------------- retrieval at gallery scale
RETRIEVAL_TILE, RETRIEVAL_MAX_K = L.XP_RETRIEVAL_TILE, L.XP_RETRIEVAL_MAX_K


def _feature_rows(t, name, d=None):
    _chk(t, name, torch.float32)
    if t.dim() != 2 or not t.is_contiguous() or t.shape[0] == 0 or t.shape[1] == 0 or (d is not None and t.shape[1] != d):
        raise ValueError(f"{name}: expected a contiguous non-empty [rows, {'d' if d is None else d}] fp32 matrix, got {tuple(t.shape)}")
    return t


def _labels(labels, name, n, limit, device):
    """int64 [n] on the device, every entry in [0, limit) -- checked here, on the host's copy, when the labels come from the host"""
    if labels is None:
        return None
    if isinstance(labels, torch.Tensor) and labels.is_cuda:
        lab = labels.to(torch.int64).contiguous()
    else:
        host = torch.as_tensor(labels, dtype=torch.int64).reshape(-1)
        if host.numel() and (int(host.min()) < 0 or int(host.max()) >= limit):
            raise ValueError(f"{name}: labels must lie in [0, {limit})")
        lab = host.to(device)
    if lab.dim() != 1 or lab.numel() != n:
        raise ValueError(f"{name}: expected one label per query ({n}), got {tuple(lab.shape)}")
    return lab


def retrieval_stream_plan(nq: int, ng: int, k: int = 1) -> dict:
    """the tiling xp_retrieval_ranks_streamed / xp_retrieval_topk use at this shape (include/xpretrain_hip.h)"""
    a, b = C.c_int32(0), C.c_int32(0)
    L.check(L.lib().xp_retrieval_stream_plan(nq, ng, k, C.byref(a), C.byref(b)), "xp_retrieval_stream_plan")
    return dict(tile=RETRIEVAL_TILE, stat_tiles_per_split=a.value, topk_tiles_per_split=b.value)


def retrieval_ranks_streamed(q: torch.Tensor, g: torch.Tensor, labels_q=None, labels_g=None, *, rows=True, cols=True, dsl=False,
                             theta=100.0):
    """(greater_q, equal_q, greater_g, equal_g): int32 count vectors of the directions asked for (None for the other), straight
    from the features q [nq, d] / g [ng, d] -- the [nq, ng] matrix is never built (include/xpretrain_hip.h)"""
    _feature_rows(q, "q")
    _feature_rows(g, "g", q.shape[1])
    nq, ng, d = q.shape[0], g.shape[0], q.shape[1]
    if not (rows or cols):
        raise ValueError("retrieval_ranks_streamed: no direction asked for")
    lq = _labels(labels_q, "labels_q", nq, ng, q.device) if rows else None
    lg = _labels(labels_g, "labels_g", ng, nq, q.device) if cols else None
    need = L.lib().xp_retrieval_ranks_streamed_workspace_bytes(nq, ng, d, int(bool(dsl)))
    if need == 0:
        raise ValueError(f"xp_retrieval_ranks_streamed_workspace_bytes: {L.lib().xp_last_error().decode()}")
    ws = workspace(need, q.device, "retrieval_ranks")
    new = lambda n: torch.empty(n, dtype=torch.int32, device=q.device)
    gq, eq = (new(nq), new(nq)) if rows else (None, None)
    gg, eg = (new(ng), new(ng)) if cols else (None, None)
    L.check(L.lib().xp_retrieval_ranks_streamed(_p(q), _p(g), _p(lq), _p(lg), nq, ng, d, int(bool(dsl)), float(theta), _p(gq), _p(eq),
                                                _p(gg), _p(eg), _p(ws), ws.numel(), _stream()), "xp_retrieval_ranks_streamed")
    return gq, eq, gg, eg


DSL_OF = {"gallery": L.XP_DSL_OF_GALLERY, "queries": L.XP_DSL_OF_QUERIES}


def _stat_pair(pair, name, n, what, device):
    """``pair`` = (mx, sum): two contiguous fp32 GPU vectors of length n"""
    if not isinstance(pair, (tuple, list)) or len(pair) != 2:
        raise TypeError(f"{name}: expected the pair (mx, sum) of fp32 GPU vectors of length {n} ({what}), got {type(pair).__name__}")
    for t, part in zip(pair, ("mx", "sum")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
            raise TypeError(f"{name}[{part}]: expected a contiguous fp32 GPU vector of length {n} ({what}), got "
                            f"{f'{t.dtype} on {t.device}' if isinstance(t, torch.Tensor) else type(t).__name__}")
        if t.dim() != 1 or t.numel() != n or not t.is_contiguous() or t.device != device:
            raise ValueError(f"{name}[{part}]: expected a contiguous fp32 vector of length {n} ({what}) on {device}, got "
                             f"{tuple(t.shape)} on {t.device}")
    return pair


def retrieval_dsl_stats(over: torch.Tensor, of: torch.Tensor, theta: float = 100.0, out=None):
    """(mx, sum) [rows of ``of``]: mx[j] = max_i theta over_i . of_j, sum[j] = sum_i exp(theta over_i . of_j - mx[j]) -- the dual
    softmax's statistics xp_retrieval_ranks_streamed(q=over, g=of, dsl=1) forms internally, bit for bit.  ``out`` = (mx, sum) of an
    earlier call over other rows of ``over``: they lead the fold and the pair is updated in place (include/xpretrain_hip.h)"""
    _feature_rows(over, "over")
    _feature_rows(of, "of", over.shape[1])
    n_over, n_of, d = over.shape[0], of.shape[0], over.shape[1]
    need = L.lib().xp_retrieval_dsl_stats_workspace_bytes(n_over, n_of, d)
    if need == 0:
        raise ValueError(f"xp_retrieval_dsl_stats_workspace_bytes: {L.lib().xp_last_error().decode()}")
    if out is None:
        mx, sm = (torch.empty(n_of, dtype=torch.float32, device=of.device) for _ in range(2))
    else:
        mx, sm = _stat_pair(out, "out", n_of, "one entry per row of `of`", of.device)
    ws = workspace(need, of.device, "retrieval_dsl_stats")
    L.check(L.lib().xp_retrieval_dsl_stats(_p(over), _p(of), n_over, n_of, d, float(theta), int(out is not None), _p(mx), _p(sm), _p(ws),
                                           ws.numel(), _stream()), "xp_retrieval_dsl_stats")
    return mx, sm


def retrieval_topk(q: torch.Tensor, g: torch.Tensor, k: int, index_base: int = 0, out=None, *, dsl=None, dsl_of="gallery", theta=100.0):
    """(vals [nq, k] fp32, idx [nq, k] int64): each query's k best gallery rows, score descending, ties to the lowest index;
    ``out`` = (vals, idx) of an earlier call: its entries compete as candidates and the pair is updated in place.
    ``dsl`` = (mx, sum): rank by s * exp(theta s - mx) / sum with the statistics of the gallery row (``dsl_of="gallery"``, length ng)
    or of the query row (``dsl_of="queries"``, length nq) -- xp_retrieval_topk_dsl; None: the plain call"""
    _feature_rows(q, "q")
    _feature_rows(g, "g", q.shape[1])
    nq, ng, d = q.shape[0], g.shape[0], q.shape[1]
    k = int(k)
    if dsl is not None:
        if dsl_of not in DSL_OF:
            raise ValueError(f"dsl_of: expected 'gallery' or 'queries', got {dsl_of!r}")
        n, what = (ng, "dsl_of='gallery': one entry per gallery row") if dsl_of == "gallery" else (nq, "dsl_of='queries': one entry per query")
        mx, sm = _stat_pair(dsl, "dsl", n, what, q.device)
    need = L.lib().xp_retrieval_topk_workspace_bytes(nq, ng, d, k)
    if need == 0:
        raise ValueError(f"xp_retrieval_topk_workspace_bytes: {L.lib().xp_last_error().decode()}")
    if out is None:
        vals = torch.empty((nq, k), dtype=torch.float32, device=q.device)
        idx = torch.empty((nq, k), dtype=torch.int64, device=q.device)
    else:
        vals, idx = out
        _chk(vals, "out[0]", torch.float32)
        _chk(idx, "out[1]", torch.int64)
        if tuple(vals.shape) != (nq, k) or tuple(idx.shape) != (nq, k) or not (vals.is_contiguous() and idx.is_contiguous()):
            raise ValueError(f"out: expected contiguous ([{nq}, {k}] fp32, [{nq}, {k}] int64), got {tuple(vals.shape)}, {tuple(idx.shape)}")
    ws = workspace(need, q.device, "retrieval_topk")
    if dsl is None:
        L.check(L.lib().xp_retrieval_topk(_p(q), _p(g), nq, ng, d, k, int(index_base), int(out is not None), _p(vals), _p(idx), _p(ws),
                                          ws.numel(), _stream()), "xp_retrieval_topk")
    else:
        L.check(L.lib().xp_retrieval_topk_dsl(_p(q), _p(g), nq, ng, d, k, int(index_base), int(out is not None), float(theta),
                                              DSL_OF[dsl_of], _p(mx), _p(sm), _p(vals), _p(idx), _p(ws), ws.numel(), _stream()),
                "xp_retrieval_topk_dsl")
    return vals, idx
