// One CLIPEncoderLayer pass per C-ABI call (modeling/CLIP_ViP.py:444-460 with CLIPAttention.forward2 :332-381 or
// .forward :266-330 and CLIPMLP :392-396): the 8 forward / ~21 backward kernel launches of a layer are issued from native
// code.  Pure host-side sequencing over the public entry points of this library (xp_layernorm_*, xp_gemm, xp_attn_*,
// and reduce.hip's xp_colsum_partials, xp_splitk_reduce, xp_reduce_rows_batch) -- no kernel of its own -- so the arithmetic is identical,
// launch for launch, to driving those entry points one by one (the Python op-by-op path, functional.EncoderLayerFn with
// XPRETRAIN_DEBUG=op_by_op; tests compare the two bit for bit).  Why: ~810 launches per training step cost 13.6 ms of
// Python / ctypes time against 16.7 ms of GPU time (BENCH_r01); from C++ a launch costs 3-4 us.
// The dense layer (xp_encoder_layer_fwd / _bwd) and the pooled last layer (xp_encoder_layer_pooled_fwd / _bwd) are the same
// sequence from out_proj onward, over `rows` rows or over the B pooled rows: those stages (out_proj_mlp_fwd, mlp_out_proj_bwd,
// finish_bwd) are written once and read the fields the argument structs have in common; LayerNorm 1, the projections, the
// attention call and their backward stay with each entry point.  Every GEMM of a backward call is described once, as a row of
// the call's BwdGemms table: the workspace carvers, the launch sites and xp_debug_layer_bwd_gemms (which functional._dx3_support
// builds its tile lists from) all read that table.
#include "common.h"
#include <string.h>
#include <stdlib.h>
#include <mutex>

namespace {

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// Bump allocator over a layer call's workspace.  Every call has ONE carve_* function below: the *_workspace_bytes query runs it
// with a null base (nothing is checked, bytes() is the answer), the call runs it over the caller's buffer, where every take is
// checked against `cap` -- so the reported size and the pointers a call uses cannot drift apart; the GEMM shapes that decide the
// sizes are the launched ones (BwdGemms below).
struct Carver {
  char* base; size_t cap, off = 0;
  bool fits = true;          // false: a take went past cap (the pointers are then not to be used)
  template <class T = void>
  T* take(size_t n, size_t* aligned = nullptr) {       // aligned: the piece's size as the callee is told it
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    n = align256(n);
    off += n;
    if (aligned) *aligned = n;
    if (base && off + 256 > cap) fits = false;
    return p;
  }
  size_t bytes() const { return off + 256; }           // the pieces and the 256 bytes of slack the ABI-1 sizes have always had
};
// the refusal of a short workspace, before anything is launched (`w`: what carve_* returned, its Carver in `ws`)
#define XP_REQUIRE_WORKSPACE(name, a, w)                                                                    \
  XP_REQUIRE((a)->workspace && (w).ws.fits, "%s: workspace too small (%zu < %zu)", name, (a)->workspace_bytes, (w).ws.bytes())

// b_kstrided: the dX form, dX[M, N] = dY[M, K] . W[K, N] with W read k-strided
XpGemmDesc gemm_desc(const void* A, const void* B, void* C, int64_t M, int64_t N, int64_t K, int dtype, bool b_kstrided = false) {
  XpGemmDesc d;
  memset(&d, 0, sizeof(d));
  d.A = A; d.B = B; d.C = C; d.M = M; d.N = N; d.K = K;
  d.lda = K; d.ldb = b_kstrided ? N : K; d.ldc = N; d.ldr = N; d.ldaux = N; d.b_kstrided = b_kstrided;
  d.in_dtype = dtype; d.out_dtype = dtype; d.split_k = 1; d.scale = 1.0f;
  return d;
}
// dW[n_out, n_in] = dY[k, n_out]^T . X[k, n_in], fp32: both operands k-strided (row pitches lddy / ldx; 0: dense)
XpGemmDesc wgrad_desc(int64_t k, int64_t n_out, int64_t n_in, int dtype, int64_t lddy = 0, int64_t ldx = 0) {
  XpGemmDesc d = gemm_desc(nullptr, nullptr, nullptr, n_out, n_in, k, dtype);
  d.a_kstrided = d.b_kstrided = 1; d.lda = lddy ? lddy : n_out; d.ldb = ldx ? ldx : n_in; d.out_dtype = XP_F32;
  return d;
}

// ---- the GEMMs of a backward call, described once: one table per call, on the stack ---------------------------------------------
// Row XP_LAYER_GEMM_* is that product's descriptor without its operands.  Three functions write the rows (tail_bwd_gemms,
// dense_bwd_gemms, pooled_bwd_gemms) and nothing else describes a backward GEMM: the carvers size the split-K slabs and fc1's
// bias-gradient partial rows from the table, a launch site copies a row, binds its operands (`bound`) and launches it,
// xp_debug_layer_bwd_gemms hands the table out.  A new product of the layer is one row.
float present_[1];                       // an optional operand of a row: the planning queries test these pointers against null only
struct BwdGemms {
  XpGemmDesc g[XP_LAYER_GEMM_MAX] = {};
  int n = 0;                             // rows in use: XP_LAYER_GEMM_DENSE_COUNT / _POOLED_COUNT
  size_t max_slab_bytes = 0;             // split-K slab space that serves every weight gradient of the table under either split rule
  int64_t db1_fused_rows = 0;            // partial rows of fc1's bias gradient out of dpre's epilogue, 0 = a column-sum pass over dpre
  // a weight gradient's row carries the split its launch uses, asked for once per call.  slack: nothing waits for this launch soon
  // (xp_gemm_auto_split_slack: fewer, longer slabs)
  void wgrad(int i, XpGemmDesc d, bool slack) {
    const int a = xp_gemm_auto_split(&d), b = xp_gemm_auto_split_slack(&d), split = slack ? b : a, most = a > b ? a : b;
    const size_t s = most <= 1 ? 0 : (size_t)most * d.M * d.N * sizeof(float);
    if (s > max_slab_bytes) max_slab_bytes = s;
    d.split_k = split > 1 ? split : 1;
    g[i] = d;
  }
};
XpGemmDesc bound(XpGemmDesc d, const void* A, const void* B, void* C) { d.A = A; d.B = B; d.C = C; return d; }

// sup / w: the k-tile lists of weight gradient w of xp_encoder_layer_bwd_listed (nullptr: dense)
int run_wgrad(XpGemmDesc d, float* slabs, size_t slab_bytes, void* st, const XpDx3Support* sup = nullptr, int w = 0) {
  const int split = d.split_k;
  if (sup) {
    XP_REQUIRE(sup->split[w] == split, "encoder layer backward: dx3_support lists weight gradient %d for split %d, "
               "the library plans %d", w, sup->split[w], split);
    d.k_tiles = sup->k_tiles[w]; d.k_tile_begin = sup->k_tile_begin[w]; d.k_tile_begin_host = sup->k_tile_begin_host[w];
  }
  if (split <= 1) return xp_gemm(&d, st);
  XP_REQUIRE(slab_bytes >= (size_t)split * d.M * d.N * sizeof(float), "encoder layer backward: split-K slab space too small");
  float* dw = (float*)d.C;
  d.C = slabs;
  int rc = xp_gemm(&d, st);
  if (rc) return rc;
  return xp_splitk_reduce(slabs, dw, d.M * d.N, split, 0, st);
}

struct Defer {             // the layer's deferred second-level reductions (bias / LayerNorm-parameter gradients)
  XpReduceSeg segs[XP_REDUCE_MAX_SEGS]; int n = 0;
  void add(const float* in, float* out, int64_t stride, int nrows, int width) {
    if (!out) return;
    XpReduceSeg& s = segs[n++];
    s.in = in; s.out = out; s.stride = stride; s.nrows = nrows; s.width = width; s.accumulate = 0; s.reserved = 0;
  }
};

// ---- weight-gradient GEMMs on a second stream (default; XPRETRAIN_WGRAD_STREAM=0 puts them back on the caller's stream) ------
// The four dW GEMMs of a layer (+ their split-K reduces) are off the critical path of the backward pass: nothing in the layer
// reads them.  On a stream of their own they run BESIDE the dX chain (GEMM -> LayerNorm -> GEMM -> attention -> GEMM -> LayerNorm):
// their workgroups take the CUs the 222-tile dX GEMMs leave idle, the tails / launch boundaries of either stream, and overlap the
// HBM-bound LayerNorm / attention / reduce kernels with MFMA work.  Ordering is by events only; the main stream joins the side
// stream before the call returns, so buffer lifetimes (workspace reuse by the next layer, the caching allocator) are unchanged.
// Measured in the step (interleaved whole-step A/B on one box, profiles/r04a_in_step_ab_wgrad_stream_chunk_major.txt):
// 16.57 -> 16.22 ms per step; results are bit-identical (same kernels, same arguments).
struct WgradSide {
  hipStream_t side = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // main-stream progress marks: entry, dpre, dx2, dqkv
  hipEvent_t done = nullptr;                                  // side stream: last dW of the call finished
  bool ok = false;
};
WgradSide* wgrad_side() {
  static const bool on = !getenv("XPRETRAIN_WGRAD_STREAM") || atoi(getenv("XPRETRAIN_WGRAD_STREAM")) != 0;      // default on
  if (!on) return nullptr;
  static std::mutex mu;
  static WgradSide per_dev[16];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  std::lock_guard<std::mutex> lock(mu);
  WgradSide& w = per_dev[dev];
  if (!w.side) {
    // DEFAULT priority.  Highest priority was worth 0.05 ms per step on one GPU (profiles/r04j_in_step_ab_wgrad_priority_split.txt) and
    // cost 15-30 ms per step as soon as a process group's collectives ran beside it (a ONE-rank RCCL group on one GPU: 36-52 ms per
    // step against 21 with the default priority, profiles/r04v_forced_one_rank_collectives_stream_matrix.txt) -- a high-priority HSA
    // queue beside the collective library's streams starves the queues the critical chain runs on.
    bool good = hipStreamCreateWithPriority(&w.side, hipStreamNonBlocking, 0) == hipSuccess;
    for (int i = 0; i < 4 && good; ++i) good = hipEventCreateWithFlags(&w.ev[i], hipEventDisableTiming) == hipSuccess;
    good = good && hipEventCreateWithFlags(&w.done, hipEventDisableTiming) == hipSuccess;
    w.ok = good;
  }
  return w.ok ? &w : nullptr;
}

// One backward call's ordering against that stream (side == nullptr: the dW GEMMs stay on the caller's stream, nothing to order)
struct WgradOrder {
  WgradSide* side; hipStream_t main; const char* name;      // name: the entry point, for error text
  void* stream() const { return side ? (void*)side->side : (void*)main; }
  int mark(int i) const {           // side stream: everything the main stream has enqueued so far must finish first
    if (!side) return XP_OK;
    if (hipEventRecord(side->ev[i], main) != hipSuccess || hipStreamWaitEvent(side->side, side->ev[i], 0) != hipSuccess) {
      xp_set_error("%s: event hand-off to the weight-gradient stream failed", name);
      return XP_ERR_LAUNCH;
    }
    return XP_OK;
  }
  int join() const {                // the weight gradients (and every workspace the side stream read) belong to the main stream again
    if (!side) return XP_OK;
    if (hipEventRecord(side->done, side->side) != hipSuccess || hipStreamWaitEvent(main, side->done, 0) != hipSuccess) {
      xp_set_error("%s: joining the weight-gradient stream failed", name);
      return XP_ERR_LAUNCH;
    }
    return XP_OK;
  }
};

// ---- the stages a dense and a pooled layer share: out_proj onward, over n rows (n = rows / n = B) --------------------------
// `Args`: XpLayerFwd / XpLayerPooledFwd (XpLayerBwd / XpLayerPooledBwd): only the fields the two have in common are read.
// Side rows: (sS, sM) is the geometry of the n rows' fp32 side rows, stored with stride sM (dense: side_S, side_M; pooled: 1, 1).

// the fc1 / dpre epilogue kinds of the layer's activation (XpLayerDims::act, validated by check_dims)
inline int epi_act_fwd(const XpLayerDims& d) { return d.act == XP_ACT_GELU ? XP_EPI_BIAS_GELU_ERF : XP_EPI_BIAS_GELU; }
inline int epi_act_bwd(const XpLayerDims& d) { return d.act == XP_ACT_GELU ? XP_EPI_GELU_ERF_BWD : XP_EPI_GELU_BWD; }

// x2 = resid + attn_o Wo^T + bo (resid: x with row pitch ldr, its side rows in side_x) ; x3 = x2 + fc2(act(fc1(LN2(x2))))
template <class Args>
int out_proj_mlp_fwd(const Args& a, int64_t n, int64_t ldr, const float* side_x, float* side_x2, float* side_out, int64_t sS,
                     int32_t sM, void* st) {
  const XpLayerDims& d = a.dims;
  const int64_t D = d.D, Dff = d.Dff;
  const int dt = d.dtype;
  int rc;
  XpGemmDesc g = gemm_desc(a.attn_o, a.Wo, a.x2, n, D, D, dt);
  g.epilogue = XP_EPI_BIAS_RESID; g.bias = a.bo; g.resid = a.x; g.ldr = ldr;
  if (side_x) { g.resid_side = side_x; g.out_side = side_x2; g.side_S = sS; g.side_M = sM; }
  if ((rc = xp_gemm(&g, st))) return rc;
  if ((rc = xp_layernorm_fwd_side(a.x2, D, a.ln2_w, a.ln2_b, a.h2, D, a.mean2, a.rstd2, n, D, d.ln_eps, dt,
                                  side_x2, nullptr, sS, sM, sM, st))) return rc;
  // pre = h2 W1^T + b1 ; act = quick_gelu(pre) or gelu(pre)
  g = gemm_desc(a.h2, a.W1, a.act, n, Dff, D, dt);
  g.epilogue = epi_act_fwd(d); g.bias = a.b1; g.aux = a.pre;
  if ((rc = xp_gemm(&g, st))) return rc;
  // x3 = x2 + act W2^T + b2
  g = gemm_desc(a.act, a.W2, a.x3, n, D, Dff, dt);
  g.epilogue = XP_EPI_BIAS_RESID; g.bias = a.b2; g.resid = a.x2;
  if (side_x) { g.resid_side = side_x2; g.out_side = side_out; g.side_S = sS; g.side_M = sM; }
  return xp_gemm(&g, st);
}

// The part of a backward workspace the shared stages use, for n rows: [dpre | dh2 | dx2 | dattn] activation-gradient temporaries,
// fc1's bias-gradient partial rows, the second LayerNorm's partial rows, the batched-reduce scratch.
struct TailBwd {
  void *dpre, *dh2, *dx2, *dattn, *red; float *cs_pre, *ln2_part;
  size_t esz, cs_pre_bytes, ln2_bytes, red_bytes;
  int64_t cs_pre_rows, ln_rows;
};
// the shared stages' rows of the table, over n rows.  fuse_db1: fc1's bias gradient comes out of the dpre GEMM's epilogue where the
// library offers it (xp_gemm_colsum_rows), else -- and always without fuse_db1 -- from a column-sum pass over dpre
void tail_bwd_gemms(BwdGemms& t, const XpLayerDims& d, int64_t n, bool fuse_db1) {
  const int64_t D = d.D, Dff = d.Dff;
  const int dt = d.dtype;
  XpGemmDesc& g = t.g[XP_LAYER_GEMM_DPRE] = gemm_desc(nullptr, nullptr, nullptr, n, Dff, D, dt, true);      // (dx3 . W2) * act'(pre)
  g.epilogue = epi_act_bwd(d); g.resid = present_;
  t.db1_fused_rows = fuse_db1 ? xp_gemm_colsum_rows(&g) : 0;
  if (t.db1_fused_rows > 0) g.colsum_partials = present_;
  t.wgrad(XP_LAYER_GEMM_DW2, wgrad_desc(n, D, Dff, dt), true);
  t.g[XP_LAYER_GEMM_DH2] = gemm_desc(nullptr, nullptr, nullptr, n, D, Dff, dt, true);                       // dpre . W1
  t.wgrad(XP_LAYER_GEMM_DW1, wgrad_desc(n, Dff, D, dt), true);
  t.g[XP_LAYER_GEMM_DATTN] = gemm_desc(nullptr, nullptr, nullptr, n, D, D, dt, true);                       // dx2 . Wo
  t.wgrad(XP_LAYER_GEMM_DWO, wgrad_desc(n, D, D, dt), true);
}
TailBwd carve_tail_bwd(Carver& ws, const BwdGemms& gm) {
  TailBwd t;
  const XpGemmDesc& dpre = gm.g[XP_LAYER_GEMM_DPRE];
  const int64_t n = dpre.M, Dff = dpre.N, D = dpre.K;
  t.esz = dpre.in_dtype == XP_BF16 ? 2 : 4;
  t.dpre = ws.take(n * Dff * t.esz); t.dh2 = ws.take(n * D * t.esz); t.dx2 = ws.take(n * D * t.esz); t.dattn = ws.take(n * D * t.esz);
  t.cs_pre_rows = gm.db1_fused_rows > 0 ? gm.db1_fused_rows : xp_colsum_partial_rows(n, Dff);
  t.cs_pre = ws.take<float>(t.cs_pre_rows * Dff * sizeof(float), &t.cs_pre_bytes);
  t.ln_rows = xp_layernorm_bwd_partial_rows(n);
  t.ln2_part = ws.take<float>(xp_layernorm_bwd_workspace_bytes(n, D), &t.ln2_bytes);
  t.red = ws.take((size_t)XP_REDUCE_MAX_SEGS * 32 * (size_t)(3 * D > Dff ? 3 * D : Dff) * sizeof(float) + 16, &t.red_bytes);
  return t;
}

// x3 = x2 + fc2(act(fc1(LN2(x2)))) and x2 = resid + out_proj(attn_o), backwards: leaves dx2 and dattn in the workspace,
// issues dW2, dW1, dWo and defers db1, dln2_w, dln2_b, dbo, db2.  Marks 1 and 2 of the weight-gradient stream.
// sup (xp_encoder_layer_bwd_listed only): dx3 is zero outside the listed tiles.  The three dX GEMMs then run over
// sup->m_tiles and the three dW GEMMs over their k-tile lists; what the dense GEMMs would have written elsewhere -- +0: dh2,
// dattn, fc1's bias-gradient partial rows -- is a fill on the launching stream in front of the listed launch.  dpre's unlisted
// tiles are neither written nor read (dh2 and dW1 walk the same tiles).  LayerNorm 2' stays dense: it reads the filled dh2.
template <class Args>
int mlp_out_proj_bwd(const Args& a, int64_t n, const BwdGemms& gm, const TailBwd& t, float* slabs, size_t slab_bytes, int64_t sS,
                     int32_t sM, Defer& df, const WgradOrder& wg, void* st, const XpDx3Support* sup = nullptr) {
  const int64_t D = a.dims.D, Dff = a.dims.Dff;
  const int dt = a.dims.dtype;
  int rc;
  auto listed = [&](XpGemmDesc& g, void* fill, size_t bytes) -> int {         // g over sup->m_tiles, its output pre-filled with +0
    if (!sup) return XP_OK;
    g.m_tiles = sup->m_tiles; g.n_m_tiles = sup->n_m_tiles;
    if (fill && hipMemsetAsync(fill, 0, bytes, (hipStream_t)st) != hipSuccess) {
      xp_set_error("%s: zero fill in front of a listed GEMM failed", wg.name);
      return XP_ERR_LAUNCH;
    }
    return XP_OK;
  };
  XpGemmDesc g = bound(gm.g[XP_LAYER_GEMM_DPRE], a.dx3, a.W2, t.dpre);        // dpre = (dx3 . W2) * act'(pre)
  g.resid = a.pre; g.colsum_partials = a.db1 && gm.db1_fused_rows > 0 ? t.cs_pre : nullptr;
  if ((rc = listed(g, g.colsum_partials, (size_t)t.cs_pre_rows * Dff * sizeof(float)))) return rc;
  if ((rc = xp_gemm(&g, st))) return rc;
  if (a.db1) {
    if (gm.db1_fused_rows == 0 && (rc = xp_colsum_partials(t.dpre, n, Dff, Dff, dt, t.cs_pre, t.cs_pre_bytes, st))) return rc;
    df.add(t.cs_pre, a.db1, Dff, (int)t.cs_pre_rows, (int)Dff);
  }
  if (a.dw2 && (rc = run_wgrad(bound(gm.g[XP_LAYER_GEMM_DW2], a.dx3, a.act, a.dw2), slabs, slab_bytes, wg.stream(), sup, 0))) return rc;
  if ((rc = wg.mark(1))) return rc;                                           // dpre is ready for dW1
  g = bound(gm.g[XP_LAYER_GEMM_DH2], t.dpre, a.W1, t.dh2);                    // dh2 = dpre . W1
  if ((rc = listed(g, t.dh2, (size_t)n * D * t.esz))) return rc;
  if ((rc = xp_gemm(&g, st))) return rc;
  if (a.dw1 && (rc = run_wgrad(bound(gm.g[XP_LAYER_GEMM_DW1], t.dpre, a.h2, a.dw1), slabs, slab_bytes, wg.stream(), sup, 1))) return rc;
  // dx2 = dx3 + LN2'(dh2); partial rows [dgamma | dbeta | colsum(dx2) | colsum(dx3)] -- out_proj's and fc2's bias gradients
  if ((rc = xp_layernorm_bwd_partials_side(t.dh2, D, a.x2, D, a.ln2_w, a.mean2, a.rstd2, a.dx3, D, t.dx2, D, 2, n, D, dt,
                                           a.side_x2, sS, sM, sM, t.ln2_part, t.ln2_bytes, st))) return rc;
  df.add(t.ln2_part, a.dln2_w, 4 * D, (int)t.ln_rows, (int)D);
  df.add(t.ln2_part + D, a.dln2_b, 4 * D, (int)t.ln_rows, (int)D);
  df.add(t.ln2_part + 2 * D, a.dbo, 4 * D, (int)t.ln_rows, (int)D);
  df.add(t.ln2_part + 3 * D, a.db2, 4 * D, (int)t.ln_rows, (int)D);
  if ((rc = wg.mark(2))) return rc;                                           // dx2 is ready for dWo
  g = bound(gm.g[XP_LAYER_GEMM_DATTN], t.dx2, a.Wo, t.dattn);                 // dattn = dx2 . Wo
  if ((rc = listed(g, t.dattn, (size_t)n * D * t.esz))) return rc;
  if ((rc = xp_gemm(&g, st))) return rc;
  if (a.dwo && (rc = run_wgrad(bound(gm.g[XP_LAYER_GEMM_DWO], t.dx2, a.attn_o, a.dwo), slabs, slab_bytes, wg.stream(), sup, 2))) return rc;
  return XP_OK;
}

// the layer's deferred reductions in one batched launch pair, then the weight-gradient stream joins the caller's
int finish_bwd(const Defer& df, void* red_ws, size_t red_bytes, const WgradOrder& wg, void* st) {
  if (df.n) {
    XP_REQUIRE(xp_reduce_rows_batch_workspace_bytes(df.segs, df.n) <= red_bytes, "%s: reduce scratch too small", wg.name);
    int rc = xp_reduce_rows_batch(df.segs, df.n, red_ws, red_bytes, st);
    if (rc) return rc;
  }
  return wg.join();
}

int check_dims(const char* name, const XpLayerDims& d) {
  XP_REQUIRE(d.rows > 0 && d.D > 0 && d.Dff > 0 && d.B > 0 && d.S > 0 && d.heads > 0, "%s: empty dimension", name);
  XP_REQUIRE(d.rows == d.B * d.S && d.D == d.heads * 64, "%s: rows != B*S or D != heads*64", name);
  XP_REQUIRE(d.dtype == XP_BF16 || d.dtype == XP_F32, "%s: bad dtype %d", name, d.dtype);
  XP_REQUIRE(d.act == XP_ACT_QUICK_GELU || d.act == XP_ACT_GELU, "%s: bad XpLayerDims::act %d (XP_ACT_QUICK_GELU = 0, XP_ACT_GELU = 1)",
             name, d.act);
  return XP_OK;
}

}  // namespace

// Every device pointer of a layer call's argument struct is 16-byte aligned (the GEMM, attention and LayerNorm entries the call
// sequences ask it of their operands; checked here once, under the struct's field names, before anything is launched).
#define XP_A(f) XpPtrName{"args." #f, (const void*)a->f}

extern "C" void* xp_side_stream(void) {
  WgradSide* w = wgrad_side();
  return w ? (void*)w->side : nullptr;
}

// workspace of the forward: the attention workspace, then `side_rows` fp32 side rows of x2 (where XpLayerFwd::side_x2 is not given)
namespace {
struct FwdWs { Carver ws; void* attn; float* side_x2; size_t attn_bytes; };
FwdWs carve_fwd(const XpLayerDims& d, int64_t side_rows, void* base, size_t cap) {
  FwdWs w;
  Carver& ws = w.ws = Carver{(char*)base, cap};
  w.attn = ws.take(xp_attn_workspace_bytes(d.attn_mode, d.B, d.heads, d.M, d.N, d.L), &w.attn_bytes);
  w.side_x2 = ws.take<float>((size_t)side_rows * d.D * sizeof(float));
  return w;
}
}  // namespace

extern "C" size_t xp_encoder_layer_fwd_workspace_bytes(const XpLayerDims* d) {
  if (!d) return 0;
  // the side rows a caller may pass: the proxy tokens of every sample (video), every row (text)
  return carve_fwd(*d, d->attn_mode == XP_ATTN_PROXY ? d->B * d->M : d->rows, nullptr, 0).ws.bytes();
}

extern "C" int xp_encoder_layer_fwd(const XpLayerFwd* a, void* st) {
  XP_REQUIRE(a, "xp_encoder_layer_fwd: null argument");
  XP_REQUIRE_ALIGNED("xp_encoder_layer_fwd", 16, XP_A(x), XP_A(Wqkv), XP_A(Wo), XP_A(W1), XP_A(W2), XP_A(ln1_w), XP_A(ln1_b), XP_A(bqkv), XP_A(bo), XP_A(ln2_w), XP_A(ln2_b), XP_A(b1), XP_A(b2), XP_A(pad_mask), XP_A(h1), XP_A(qkv), XP_A(attn_o), XP_A(x2), XP_A(h2), XP_A(pre), XP_A(act), XP_A(x3), XP_A(mean1), XP_A(rstd1), XP_A(mean2), XP_A(rstd2), XP_A(stats), XP_A(workspace), XP_A(side_in), XP_A(side_out), XP_A(side_x2));
  const XpLayerDims& d = a->dims;
  int rc = check_dims("xp_encoder_layer_fwd", d);
  if (rc) return rc;
  XP_REQUIRE(a->x && a->Wqkv && a->Wo && a->W1 && a->W2 && a->ln1_w && a->ln1_b && a->bqkv && a->bo && a->ln2_w && a->ln2_b &&
             a->b1 && a->b2 && a->h1 && a->qkv && a->attn_o && a->x2 && a->h2 && a->act && a->x3 && a->mean1 &&
             a->rstd1 && a->mean2 && a->rstd2 && a->stats, "xp_encoder_layer_fwd: null pointer");
  const int64_t rows = d.rows, D = d.D;
  const int dt = d.dtype;
  // fp32 side rows of the residual stream (the M proxy tokens of every sample): x rows in side_in, x2 rows in the workspace,
  // x3 rows in side_out
  const bool sided = a->side_in != nullptr;
  XP_REQUIRE(!sided || (a->side_out && dt == XP_BF16 && a->side_S > 0 && a->side_M > 0 && a->side_M <= a->side_S),
             "xp_encoder_layer_fwd: side rows need side_in and side_out, bf16 and 0 < side_M <= side_S");
  const int64_t sS = a->side_S;
  const int32_t sM = a->side_M;
  const FwdWs w = carve_fwd(d, sided ? cdiv(rows, sS) * sM : 0, a->workspace, a->workspace_bytes);
  XP_REQUIRE_WORKSPACE("xp_encoder_layer_fwd", a, w);
  float* side_x2 = !sided ? nullptr : a->side_x2 ? a->side_x2 : w.side_x2;
  // h1 = LN1(x)
  if ((rc = xp_layernorm_fwd_side(a->x, D, a->ln1_w, a->ln1_b, a->h1, D, a->mean1, a->rstd1, rows, D, d.ln_eps, dt,
                                  a->side_in, nullptr, sS, sM, sM, st))) return rc;
  // qkv = (h1 Wqkv^T + b), q columns scaled by dh^-0.5 (:341)
  XpGemmDesc g = gemm_desc(a->h1, a->Wqkv, a->qkv, rows, 3 * D, D, dt);
  g.epilogue = XP_EPI_BIAS_QSCALE; g.bias = a->bqkv; g.scale = d.q_scale; g.scale_cols = D;
  if ((rc = xp_gemm(&g, st))) return rc;
  if ((rc = xp_attn_fwd(a->qkv, 3 * D, a->attn_o, D, a->stats, a->pad_mask, d.attn_mode, d.B, d.heads, d.S, d.M, d.N, d.L, dt,
                        w.attn, w.attn_bytes, st))) return rc;
  return out_proj_mlp_fwd(*a, rows, D, a->side_in, side_x2, a->side_out, sS, sM, st);
}

// workspace of the backward: the shared stages' part (TailBwd), [dqkv | dh1], split-K slabs, the q/k/v bias-gradient and first
// LayerNorm's partial rows, the attention workspace
namespace {
struct BwdWs {
  Carver ws; BwdGemms gm; TailBwd t;
  void *dqkv, *dh1, *attn; float *slabs, *cs_qkv, *ln1_part;
  size_t slab_bytes, cs_qkv_bytes, ln1_bytes, attn_bytes;
  int64_t cs_qkv_rows;
  bool cs_qkv_fused;
};
// the dense backward's table: the shared stages over every row, then dh1 = dqkv . Wqkv and dWqkv -- the last launch of the layer,
// the one the join waits for: the general split rule
BwdGemms dense_bwd_gemms(const XpLayerDims& d) {
  BwdGemms t;
  t.n = XP_LAYER_GEMM_DENSE_COUNT;
  tail_bwd_gemms(t, d, d.rows, true);
  t.g[XP_LAYER_GEMM_DH1] = gemm_desc(nullptr, nullptr, nullptr, d.rows, d.D, 3 * d.D, d.dtype, true);
  t.wgrad(XP_LAYER_GEMM_DWQKV, wgrad_desc(d.rows, 3 * d.D, d.D, d.dtype), false);
  return t;
}
BwdWs carve_bwd(const XpLayerDims& d, void* base, size_t cap) {
  BwdWs w;
  Carver& ws = w.ws = Carver{(char*)base, cap};
  const int64_t rows = d.rows, D = d.D;
  w.gm = dense_bwd_gemms(d);
  w.t = carve_tail_bwd(ws, w.gm);
  // (fc2's bias gradient = column sums of dx3: taken by the second LayerNorm's backward)
  w.dqkv = ws.take(rows * 3 * D * w.t.esz); w.dh1 = ws.take(rows * D * w.t.esz);
  w.slabs = ws.take<float>(w.gm.max_slab_bytes, &w.slab_bytes);
  // the q/k/v bias gradients: out of the attention backward kernels where they offer it, else a column-sum pass over dqkv
  w.cs_qkv_rows = xp_attn_bwd_colsum_rows(d.attn_mode, d.B, d.heads, d.S, d.M, d.N, d.L, d.dtype);
  w.cs_qkv_fused = w.cs_qkv_rows > 0;
  if (!w.cs_qkv_fused) w.cs_qkv_rows = xp_colsum_partial_rows(rows, 3 * D);
  w.cs_qkv = ws.take<float>(w.cs_qkv_rows * 3 * D * sizeof(float), &w.cs_qkv_bytes);
  w.ln1_part = ws.take<float>(w.t.ln2_bytes, &w.ln1_bytes);      // (both LayerNorms run over the same [rows, D])
  w.attn = ws.take(xp_attn_workspace_bytes(d.attn_mode, d.B, d.heads, d.M, d.N, d.L), &w.attn_bytes);
  return w;
}
}  // namespace

extern "C" size_t xp_encoder_layer_bwd_workspace_bytes(const XpLayerDims* d) {
  if (!d || d->rows <= 0) return 0;
  return carve_bwd(*d, nullptr, 0).ws.bytes();
}

static int encoder_layer_bwd(const XpLayerBwd* a, const XpDx3Support* sup, void* st);
extern "C" int xp_encoder_layer_bwd(const XpLayerBwd* a, void* st) { return encoder_layer_bwd(a, nullptr, st); }
extern "C" int xp_encoder_layer_bwd_listed(const XpLayerBwd* a, const XpDx3Support* sup, void* st) {
  XP_REQUIRE(sup, "xp_encoder_layer_bwd_listed: null dx3_support");
  return encoder_layer_bwd(a, sup, st);
}

static int encoder_layer_bwd(const XpLayerBwd* a, const XpDx3Support* sup, void* st) {
  XP_REQUIRE(a, "xp_encoder_layer_bwd: null argument");
  const char* const fn = sup ? "xp_encoder_layer_bwd_listed" : "xp_encoder_layer_bwd";
  XP_REQUIRE_ALIGNED(fn, 16, XP_A(x), XP_A(h1), XP_A(qkv), XP_A(attn_o), XP_A(x2), XP_A(h2), XP_A(pre), XP_A(act), XP_A(Wqkv), XP_A(Wo), XP_A(W1), XP_A(W2), XP_A(ln1_w), XP_A(ln2_w), XP_A(mean1), XP_A(rstd1), XP_A(mean2), XP_A(rstd2), XP_A(stats), XP_A(pad_mask), XP_A(dx3), XP_A(dx), XP_A(dln1_w), XP_A(dln1_b), XP_A(dwqkv), XP_A(dbqkv), XP_A(dwo), XP_A(dbo), XP_A(dln2_w), XP_A(dln2_b), XP_A(dw1), XP_A(db1), XP_A(dw2), XP_A(db2), XP_A(workspace), XP_A(side_in), XP_A(side_x2));
  if (sup)
    XP_REQUIRE_ALIGNED(fn, 16, XpPtrName{"dx3_support.m_tiles", sup->m_tiles}, XpPtrName{"dx3_support.k_tiles[0]", sup->k_tiles[0]},
                       XpPtrName{"dx3_support.k_tiles[1]", sup->k_tiles[1]}, XpPtrName{"dx3_support.k_tiles[2]", sup->k_tiles[2]},
                       XpPtrName{"dx3_support.k_tile_begin[0]", sup->k_tile_begin[0]}, XpPtrName{"dx3_support.k_tile_begin[1]", sup->k_tile_begin[1]},
                       XpPtrName{"dx3_support.k_tile_begin[2]", sup->k_tile_begin[2]});
  const XpLayerDims& d = a->dims;
  int rc = check_dims("xp_encoder_layer_bwd", d);
  if (rc) return rc;
  XP_REQUIRE(a->x && a->h1 && a->qkv && a->attn_o && a->x2 && a->h2 && a->pre && a->act && a->Wqkv && a->Wo && a->W1 && a->W2 &&
             a->ln1_w && a->ln2_w && a->mean1 && a->rstd1 && a->mean2 && a->rstd2 && a->stats && a->dx3 && a->dx,
             "xp_encoder_layer_bwd: null pointer");
  XP_REQUIRE((!a->side_in && !a->side_x2) || (a->side_in && a->side_x2 && d.dtype == XP_BF16 && a->side_S > 0 && a->side_M > 0 &&
                                               a->side_M <= a->side_S),
             "xp_encoder_layer_bwd: side rows need side_in and side_x2, bf16 and 0 < side_M <= side_S");
  const BwdWs w = carve_bwd(d, a->workspace, a->workspace_bytes);
  XP_REQUIRE_WORKSPACE("xp_encoder_layer_bwd", a, w);
  const int64_t rows = d.rows, D = d.D;
  const int dt = d.dtype;
  Defer df;
  // dW GEMMs beside the dX chain (video tower only: the text tower is 256 rows on a side stream of its own already)
  const WgradOrder wg{(d.attn_mode == XP_ATTN_PROXY && rows >= 4096) ? wgrad_side() : nullptr, (hipStream_t)st, "xp_encoder_layer_bwd"};
  if ((rc = wg.mark(0))) return rc;
  // ---- MLP: x3 = x2 + fc2(act(fc1(LN2(x2)))), then dattn = dx2 . Wo of x2 = x + out_proj(attn(qkv(LN1(x))))
  if (sup) {
    XP_REQUIRE(w.gm.db1_fused_rows > 0 && sup->m_tiles && sup->n_m_tiles >= 1, "xp_encoder_layer_bwd: dx3_support needs the 256-wide "
               "GEMM plans of this shape (fused fc1 bias sums) and a non-empty m_tiles");
    for (int i = 0; i < 3; ++i)
      XP_REQUIRE(sup->k_tiles[i] && sup->k_tile_begin[i] && sup->k_tile_begin_host[i], "xp_encoder_layer_bwd: dx3_support list %d is null", i);
  }
  if ((rc = mlp_out_proj_bwd(*a, rows, w.gm, w.t, w.slabs, w.slab_bytes, a->side_S, a->side_M, df, wg, st, sup))) return rc;
  // ---- attention
  if ((rc = xp_attn_bwd2(a->qkv, 3 * D, a->attn_o, w.t.dattn, D, a->stats, a->pad_mask, w.dqkv, d.q_scale, d.attn_mode, d.B, d.heads,
                         d.S, d.M, d.N, d.L, dt, w.attn, w.attn_bytes, (a->dbqkv && w.cs_qkv_fused) ? w.cs_qkv : nullptr, st))) return rc;
  if ((rc = wg.mark(3))) return rc;                                           // dqkv is ready for dWqkv
  const XpGemmDesc g = bound(w.gm.g[XP_LAYER_GEMM_DH1], w.dqkv, a->Wqkv, w.dh1);      // dh1 = dqkv . Wqkv
  if ((rc = xp_gemm(&g, st))) return rc;
  if (a->dwqkv && (rc = run_wgrad(bound(w.gm.g[XP_LAYER_GEMM_DWQKV], w.dqkv, a->h1, a->dwqkv), w.slabs, w.slab_bytes, wg.stream()))) return rc;
  if (a->dbqkv) {
    if (!w.cs_qkv_fused && (rc = xp_colsum_partials(w.dqkv, rows, 3 * D, 3 * D, dt, w.cs_qkv, w.cs_qkv_bytes, st))) return rc;
    df.add(w.cs_qkv, a->dbqkv, 3 * D, (int)w.cs_qkv_rows, (int)(3 * D));
  }
  if ((rc = xp_layernorm_bwd_partials_side(w.dh1, D, a->x, D, a->ln1_w, a->mean1, a->rstd1, w.t.dx2, D, a->dx, D, 0, rows, D, dt,
                                           a->side_in, a->side_S, a->side_M, a->side_M, w.ln1_part, w.ln1_bytes, st))) return rc;
  df.add(w.ln1_part, a->dln1_w, 2 * D, (int)w.t.ln_rows, (int)D);
  df.add(w.ln1_part + D, a->dln1_b, 2 * D, (int)w.t.ln_rows, (int)D);
  return finish_bwd(df, w.t.red, w.t.red_bytes, wg, st);
}

// ================================================================================== pooled last layer (video tower)
// The last layer when only token 0 of every sample (a proxy row) leaves the tower: LayerNorm 1 and the K/V projection on every
// row, everything else on the B pooled rows (include/xpretrain_hip.h: XpLayerPooledFwd).  Host-side sequencing again: the one
// kernel pair of its own is the single-query attention (attention_pooled.hip).  Row b*S of a [rows, .] matrix is addressed as
// row b of a matrix with pitch S*D (LayerNorm, the residual operand) or through the GEMM's A-row remap (1, S, 0).
namespace {

int check_pooled_dims(const char* name, const XpLayerDims& d) {
  int rc = check_dims(name, d);
  if (rc) return rc;
  XP_REQUIRE(d.attn_mode == XP_ATTN_PROXY && d.M >= 1 && d.N >= 1 && d.L >= 1 && d.S == d.M + d.N * d.L,
             "%s: the pooled layer is the video tower's (XP_ATTN_PROXY, M >= 1, S == M + N*L)", name);
  return XP_OK;
}

// workspace of the pooled forward: the attention partials, then two [B, D] fp32 side buffers (the pooled rows of side_in; side_x2
// of a forward-only pass)
struct PooledFwdWs { Carver ws; void* attn; float *side0, *side_x2; size_t attn_bytes; };
PooledFwdWs carve_pooled_fwd(const XpLayerDims& d, void* base, size_t cap) {
  PooledFwdWs w;
  Carver& ws = w.ws = Carver{(char*)base, cap};
  w.attn = ws.take(xp_attn_pooled_workspace_bytes(d.B, d.heads, d.S, d.dtype), &w.attn_bytes);
  w.side0 = ws.take<float>((size_t)d.B * d.D * sizeof(float)); w.side_x2 = ws.take<float>((size_t)d.B * d.D * sizeof(float));
  return w;
}

// workspace of the pooled backward: the shared stages over the B pooled rows (TailBwd), [dqkv | dh1] over every row, split-K slabs,
// the q and k/v bias-gradient partial rows, LayerNorm 1's partial rows of both passes, the attention partials
struct PooledBwdWs {
  Carver ws; BwdGemms gm; TailBwd t;
  char* dqkv; void *dh1, *attn; float *slabs, *cs_q, *cs_kv, *ln1_part, *ln1p_part;
  size_t slab_bytes, cs_q_bytes, ln1_bytes, ln1p_bytes, attn_bytes;
  int64_t cs_q_rows, ln_rows;
};
// the pooled backward's table: the shared stages over the B pooled rows (fc1's bias gradient: always a column-sum pass over dpre),
// then, over dqkv[rows, 3D] (row pitch 3D): dh1 = dkv . Wkv on every row, the pooled rows again with their q columns (row b*S
// through the row remaps), dWq of the pooled rows and dWkv of every row -- the last launch, the general split rule
BwdGemms pooled_bwd_gemms(const XpLayerDims& d) {
  BwdGemms t;
  const int64_t rows = d.rows, D = d.D, B = d.B, S = d.S;
  t.n = XP_LAYER_GEMM_POOLED_COUNT;
  tail_bwd_gemms(t, d, B, false);
  t.g[XP_LAYER_GEMM_DH1_KV] = gemm_desc(nullptr, nullptr, nullptr, rows, D, 2 * D, d.dtype, true);        // dh1 = dkv . Wkv
  t.g[XP_LAYER_GEMM_DH1_KV].lda = 3 * D;
  XpGemmDesc& g = t.g[XP_LAYER_GEMM_DH1_Q] = gemm_desc(nullptr, nullptr, nullptr, B, D, 3 * D, d.dtype, true);   // dh1[b*S] = dqkv[b*S] . Wqkv
  g.a_grp = 1; g.a_grp_stride = S; g.c_grp = 1; g.c_grp_stride = S;
  XpGemmDesc gq = wgrad_desc(B, D, D, d.dtype, 3 * D, D);                     // dWq = dq^T . h1p: dq of the pooled rows of dqkv
  gq.a_grp = 1; gq.a_grp_stride = S;
  t.wgrad(XP_LAYER_GEMM_DWQ, gq, true);
  t.wgrad(XP_LAYER_GEMM_DWKV, wgrad_desc(rows, 2 * D, D, d.dtype, 3 * D, D), false);
  return t;
}
PooledBwdWs carve_pooled_bwd(const XpLayerDims& d, void* base, size_t cap) {
  PooledBwdWs w;
  Carver& ws = w.ws = Carver{(char*)base, cap};
  const int64_t rows = d.rows, D = d.D, B = d.B, S = d.S;
  const int dt = d.dtype;
  w.gm = pooled_bwd_gemms(d);
  w.t = carve_tail_bwd(ws, w.gm);
  w.dqkv = ws.take<char>(rows * 3 * D * w.t.esz); w.dh1 = ws.take(rows * D * w.t.esz);
  w.slabs = ws.take<float>(w.gm.max_slab_bytes, &w.slab_bytes);
  w.cs_q_rows = xp_colsum_partial_rows(B, D);
  w.cs_q = ws.take<float>(w.cs_q_rows * D * sizeof(float), &w.cs_q_bytes);
  w.cs_kv = ws.take<float>(xp_attn_pooled_colsum_rows_max(B, S) * 2 * D * sizeof(float));
  w.ln_rows = xp_layernorm_bwd_partial_rows(rows);
  w.ln1_part = ws.take<float>(xp_layernorm_bwd_workspace_bytes(rows, D), &w.ln1_bytes);
  w.ln1p_part = ws.take<float>(w.t.ln2_bytes, &w.ln1p_bytes);      // (LayerNorm 1 once more over the [B, D] pooled rows)
  w.attn = ws.take(xp_attn_pooled_workspace_bytes(B, d.heads, S, dt), &w.attn_bytes);
  return w;
}

}  // namespace

extern "C" size_t xp_encoder_layer_pooled_fwd_workspace_bytes(const XpLayerDims* d) {
  if (!d || d->B <= 0 || d->D <= 0 || d->S <= 0 || d->heads <= 0) return 0;
  return carve_pooled_fwd(*d, nullptr, 0).ws.bytes();
}

extern "C" int xp_encoder_layer_pooled_fwd(const XpLayerPooledFwd* a, void* st) {
  XP_REQUIRE(a, "xp_encoder_layer_pooled_fwd: null argument");
  XP_REQUIRE_ALIGNED("xp_encoder_layer_pooled_fwd", 16, XP_A(x), XP_A(Wqkv), XP_A(Wo), XP_A(W1), XP_A(W2), XP_A(ln1_w), XP_A(ln1_b), XP_A(bqkv), XP_A(bo), XP_A(ln2_w), XP_A(ln2_b), XP_A(b1), XP_A(b2), XP_A(h1), XP_A(kv), XP_A(mean1), XP_A(rstd1), XP_A(h1p), XP_A(q), XP_A(attn_o), XP_A(x2), XP_A(h2), XP_A(pre), XP_A(act), XP_A(x3), XP_A(mean1p), XP_A(rstd1p), XP_A(mean2), XP_A(rstd2), XP_A(stats), XP_A(workspace), XP_A(side_in), XP_A(side_out), XP_A(side_x2));
  const XpLayerDims& d = a->dims;
  int rc = check_pooled_dims("xp_encoder_layer_pooled_fwd", d);
  if (rc) return rc;
  XP_REQUIRE(a->x && a->Wqkv && a->Wo && a->W1 && a->W2 && a->ln1_w && a->ln1_b && a->bqkv && a->bo && a->ln2_w && a->ln2_b &&
             a->b1 && a->b2 && a->h1 && a->kv && a->mean1 && a->rstd1 && a->h1p && a->q && a->attn_o && a->x2 && a->h2 && a->act &&
             a->x3 && a->mean1p && a->rstd1p && a->mean2 && a->rstd2 && a->stats, "xp_encoder_layer_pooled_fwd: null pointer");
  const int64_t rows = d.rows, D = d.D, B = d.B, S = d.S;
  const int dt = d.dtype;
  const bool sided = a->side_in != nullptr;
  XP_REQUIRE(!sided || (a->side_out && dt == XP_BF16), "xp_encoder_layer_pooled_fwd: side rows need side_in and side_out, and bf16");
  const PooledFwdWs w = carve_pooled_fwd(d, a->workspace, a->workspace_bytes);
  XP_REQUIRE_WORKSPACE("xp_encoder_layer_pooled_fwd", a, w);
  float* side0 = sided ? w.side0 : nullptr;
  float* side_x2 = !sided ? nullptr : a->side_x2 ? a->side_x2 : w.side_x2;
  const int64_t sS = sided ? S : 0;
  const int32_t sM = sided ? (int32_t)d.M : 0, s1 = sided ? 1 : 0;
  const size_t esz = dt == XP_BF16 ? 2 : 4;
  // h1 = LN1(x) on every row; the pooled rows once more as a [B, D] matrix of their own (the Q projection's operand)
  if ((rc = xp_layernorm_fwd_side(a->x, D, a->ln1_w, a->ln1_b, a->h1, D, a->mean1, a->rstd1, rows, D, d.ln_eps, dt,
                                  a->side_in, nullptr, sS, sM, sM, st))) return rc;
  if (sided && (rc = xp_gather_rows(a->side_in, nullptr, side0, B, d.M, D, XP_F32, st))) return rc;
  if ((rc = xp_layernorm_fwd_side(a->x, S * D, a->ln1_w, a->ln1_b, a->h1p, D, a->mean1p, a->rstd1p, B, D, d.ln_eps, dt,
                                  side0, nullptr, s1, s1, s1, st))) return rc;
  // kv = h1 Wkv^T + bkv on every row (token 0 attends all S keys); q = (h1p Wq^T + bq) * dh^-0.5 on the pooled rows
  XpGemmDesc g = gemm_desc(a->h1, static_cast<const char*>(a->Wqkv) + (size_t)D * D * esz, a->kv, rows, 2 * D, D, dt);
  g.epilogue = XP_EPI_BIAS; g.bias = a->bqkv + D;
  if ((rc = xp_gemm(&g, st))) return rc;
  g = gemm_desc(a->h1p, a->Wqkv, a->q, B, D, D, dt);
  g.epilogue = XP_EPI_BIAS_QSCALE; g.bias = a->bqkv; g.scale = d.q_scale; g.scale_cols = D;
  if ((rc = xp_gemm(&g, st))) return rc;
  if ((rc = xp_attn_pooled_fwd(a->q, a->kv, 2 * D, a->attn_o, a->stats, B, d.heads, S, dt, w.attn, w.attn_bytes, st))) return rc;
  // x2 = x[pooled] + attn_o Wo^T + bo, then the MLP
  return out_proj_mlp_fwd(*a, B, S * D, side0, side_x2, a->side_out, s1, s1, st);
}

extern "C" int32_t xp_debug_layer_bwd_gemms(const XpLayerDims* d, int32_t pooled, XpGemmDesc* out, int32_t cap) {
  XP_REQUIRE(d && out, "xp_debug_layer_bwd_gemms: null argument");
  int rc = pooled ? check_pooled_dims("xp_debug_layer_bwd_gemms", *d) : check_dims("xp_debug_layer_bwd_gemms", *d);
  if (rc) return rc;
  const BwdGemms t = pooled ? pooled_bwd_gemms(*d) : dense_bwd_gemms(*d);
  XP_REQUIRE(cap >= t.n, "xp_debug_layer_bwd_gemms: room for %d descriptors, the table has %d", cap, t.n);
  memcpy(out, t.g, t.n * sizeof(XpGemmDesc));
  return t.n;
}

extern "C" size_t xp_encoder_layer_pooled_bwd_workspace_bytes(const XpLayerDims* d) {
  if (!d || d->rows <= 0 || d->B <= 0 || d->D <= 0 || d->Dff <= 0 || d->S <= 0 || d->heads <= 0) return 0;
  return carve_pooled_bwd(*d, nullptr, 0).ws.bytes();
}

extern "C" int xp_encoder_layer_pooled_bwd(const XpLayerPooledBwd* a, void* st) {
  XP_REQUIRE(a, "xp_encoder_layer_pooled_bwd: null argument");
  XP_REQUIRE_ALIGNED("xp_encoder_layer_pooled_bwd", 16, XP_A(x), XP_A(h1), XP_A(kv), XP_A(h1p), XP_A(q), XP_A(attn_o), XP_A(x2), XP_A(h2), XP_A(pre), XP_A(act), XP_A(Wqkv), XP_A(Wo), XP_A(W1), XP_A(W2), XP_A(ln1_w), XP_A(ln2_w), XP_A(mean1), XP_A(rstd1), XP_A(mean1p), XP_A(rstd1p), XP_A(mean2), XP_A(rstd2), XP_A(stats), XP_A(dx3), XP_A(dx), XP_A(dln1_w), XP_A(dln1_b), XP_A(dwqkv), XP_A(dbqkv), XP_A(dwo), XP_A(dbo), XP_A(dln2_w), XP_A(dln2_b), XP_A(dw1), XP_A(db1), XP_A(dw2), XP_A(db2), XP_A(workspace), XP_A(side_in), XP_A(side_x2));
  const XpLayerDims& d = a->dims;
  int rc = check_pooled_dims("xp_encoder_layer_pooled_bwd", d);
  if (rc) return rc;
  XP_REQUIRE(a->x && a->h1 && a->kv && a->h1p && a->q && a->attn_o && a->x2 && a->h2 && a->pre && a->act && a->Wqkv && a->Wo &&
             a->W1 && a->W2 && a->ln1_w && a->ln2_w && a->mean1 && a->rstd1 && a->mean1p && a->rstd1p && a->mean2 && a->rstd2 &&
             a->stats && a->dx3 && a->dx, "xp_encoder_layer_pooled_bwd: null pointer");
  XP_REQUIRE((!a->side_in && !a->side_x2) || (a->side_in && a->side_x2 && d.dtype == XP_BF16),
             "xp_encoder_layer_pooled_bwd: side rows need side_in and side_x2, and bf16");
  const PooledBwdWs w = carve_pooled_bwd(d, a->workspace, a->workspace_bytes);
  XP_REQUIRE_WORKSPACE("xp_encoder_layer_pooled_bwd", a, w);
  char* const dqkv = w.dqkv;
  const int64_t rows = d.rows, D = d.D, B = d.B, S = d.S;
  const int dt = d.dtype;
  const bool sided = a->side_in != nullptr;
  const int64_t sS = sided ? S : 0;
  const int32_t sM = sided ? (int32_t)d.M : 0, s1 = sided ? 1 : 0;
  void* dkv = dqkv + (size_t)D * w.t.esz;    // dqkv[rows, 3D]: the k / v columns of every row, the q columns of the pooled rows only
  Defer df;
  const WgradOrder wg{rows >= 4096 ? wgrad_side() : nullptr, (hipStream_t)st, "xp_encoder_layer_pooled_bwd"};
  if ((rc = wg.mark(0))) return rc;
  // ---- MLP and dattn = dx2 . Wo on the pooled rows
  if ((rc = mlp_out_proj_bwd(*a, B, w.gm, w.t, w.slabs, w.slab_bytes, s1, s1, df, wg, st))) return rc;
  // ---- attention: dq lands in the q columns of the pooled rows of dqkv, dk / dv in the k / v columns of every row
  if ((rc = xp_attn_pooled_bwd(a->q, a->kv, 2 * D, a->attn_o, w.t.dattn, a->stats, dqkv, S * 3 * D, dkv, 3 * D, d.q_scale, B, d.heads,
                               S, dt, w.attn, w.attn_bytes, a->dbqkv ? w.cs_kv : nullptr, st))) return rc;
  if ((rc = wg.mark(3))) return rc;
  // dh1 = dkv . Wkv on every row, then the pooled rows again with their q columns: dqkv[b*S] . Wqkv
  XpGemmDesc g = bound(w.gm.g[XP_LAYER_GEMM_DH1_KV], dkv, static_cast<const char*>(a->Wqkv) + (size_t)D * D * w.t.esz, w.dh1);
  if ((rc = xp_gemm(&g, st))) return rc;
  g = bound(w.gm.g[XP_LAYER_GEMM_DH1_Q], dqkv, a->Wqkv, w.dh1);
  if ((rc = xp_gemm(&g, st))) return rc;
  if (a->dwqkv) {
    if ((rc = run_wgrad(bound(w.gm.g[XP_LAYER_GEMM_DWQ], dqkv, a->h1p, a->dwqkv), w.slabs, w.slab_bytes, wg.stream()))) return rc;
    if ((rc = run_wgrad(bound(w.gm.g[XP_LAYER_GEMM_DWKV], dkv, a->h1, a->dwqkv + D * D), w.slabs, w.slab_bytes, wg.stream()))) return rc;
  }
  if (a->dbqkv) {
    const int64_t kv_rows = xp_attn_pooled_colsum_rows(B, d.heads, S, dt);
    XP_REQUIRE(kv_rows > 0, "xp_encoder_layer_pooled_bwd: no current device");
    if ((rc = xp_colsum_partials(dqkv, B, D, S * 3 * D, dt, w.cs_q, w.cs_q_bytes, st))) return rc;
    df.add(w.cs_q, a->dbqkv, D, (int)w.cs_q_rows, (int)D);
    df.add(w.cs_kv, a->dbqkv + D, 2 * D, (int)kv_rows, (int)(2 * D));
  }
  // dx = LN1'(dh1) on every row; the pooled rows once more with their residual gradient dx2 (the parameter-gradient partial
  // rows of that second pass are dropped: the first pass has counted those rows)
  if ((rc = xp_layernorm_bwd_partials_side(w.dh1, D, a->x, D, a->ln1_w, a->mean1, a->rstd1, nullptr, D, a->dx, D, 0, rows, D, dt,
                                           a->side_in, sS, sM, sM, w.ln1_part, w.ln1_bytes, st))) return rc;
  df.add(w.ln1_part, a->dln1_w, 2 * D, (int)w.ln_rows, (int)D);
  df.add(w.ln1_part + D, a->dln1_b, 2 * D, (int)w.ln_rows, (int)D);
  if ((rc = xp_layernorm_bwd_partials_side(w.dh1, S * D, a->x, S * D, a->ln1_w, a->mean1p, a->rstd1p, w.t.dx2, D, a->dx, S * D, 0, B, D, dt,
                                           a->side_in, s1, s1, sM, w.ln1p_part, w.ln1p_bytes, st))) return rc;
  return finish_bwd(df, w.t.red, w.t.red_bytes, wg, st);
}
#undef XP_A
