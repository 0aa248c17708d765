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
// attention call and their backward stay with each entry point.
#include "common.h"
#include <string.h>
#include <stdlib.h>
#include <initializer_list>
#include <mutex>

namespace {

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

struct Carver {            // bump allocator over the caller's workspace
  char* base; size_t off, cap;
  void* take(size_t n) { void* p = base ? base + off : nullptr; off += align256(n); return p; }
};

XpGemmDesc gemm_desc(const void* A, const void* B, void* C, int64_t M, int64_t N, int64_t K, int dtype) {
  XpGemmDesc d;
  memset(&d, 0, sizeof(d));
  d.A = A; d.B = B; d.C = C; d.M = M; d.N = N; d.K = K;
  d.lda = K; d.ldb = K; d.ldc = N; d.ldr = N; d.ldaux = N;
  d.in_dtype = dtype; d.out_dtype = dtype; d.split_k = 1; d.scale = 1.0f;
  return d;
}

// dW[n_out, n_in] = dY[k, n_out]^T . X[k, n_in], fp32: both operands k-strided (row pitches lddy / ldx), split-K chosen by the library
XpGemmDesc wgrad_desc(const void* dy, int64_t lddy, const void* x, int64_t ldx, float* dw, int64_t k, int64_t n_out, int64_t n_in,
                      int dtype) {
  XpGemmDesc d = gemm_desc(dy, x, dw, n_out, n_in, k, dtype);
  d.a_kstrided = d.b_kstrided = 1; d.lda = lddy; d.ldb = ldx; d.out_dtype = XP_F32;
  return d;
}
// slack: nothing waits for this launch soon (xp_gemm_auto_split_slack: fewer, longer slabs)
int run_wgrad(XpGemmDesc d, float* slabs, size_t slab_bytes, void* st, bool slack) {
  const int split = slack ? xp_gemm_auto_split_slack(&d) : xp_gemm_auto_split(&d);
  if (split <= 1) return xp_gemm(&d, st);
  XP_REQUIRE(slab_bytes >= (size_t)split * d.M * d.N * sizeof(float), "encoder layer backward: split-K slab space too small");
  float* dw = (float*)d.C;
  d.C = slabs; d.split_k = split;
  int rc = xp_gemm(&d, st);
  if (rc) return rc;
  if (xp_debug_flag("skip_splitk_reduce")) return XP_OK;      // measurement only (wrong gradients): what the four reduces of a layer cost the step
  return xp_splitk_reduce(slabs, dw, d.M * d.N, split, 0, st);
}
// both operands dense: dY[k, n_out], X[k, n_in]
XpGemmDesc wgrad_desc(const void* dy, const void* x, float* dw, int64_t k, int64_t n_out, int64_t n_in, int dtype) {
  return wgrad_desc(dy, n_out, x, n_in, dw, k, n_out, n_in, dtype);
}
// split-K slab space that serves every one of `ds` under either split rule (and at least `s` bytes)
size_t max_slab_bytes(size_t s, std::initializer_list<XpGemmDesc> ds) {
  for (XpGemmDesc d : ds) {
    const int a = xp_gemm_auto_split(&d), b = xp_gemm_auto_split_slack(&d), split = a > b ? a : b;
    const size_t t = split <= 1 ? 0 : (size_t)split * d.M * d.N * sizeof(float);
    if (t > s) s = t;
  }
  return s;
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
    // (XPRETRAIN_DEBUG=no_wgrad_join: measurement only -- races on the shared workspace -- what a lazy join could be worth at most)
    if (!side || xp_debug_flag("no_wgrad_join")) return XP_OK;
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
  if (xp_debug_flag("fc1_no_pre")) g.aux = nullptr;      // measurement only (tools/fc1_one_output.py): the backward then reads garbage
  if ((rc = xp_gemm(&g, st))) return rc;
  // x3 = x2 + act W2^T + b2
  g = gemm_desc(a.act, a.W2, a.x3, n, D, Dff, dt);
  g.epilogue = XP_EPI_BIAS_RESID; g.bias = a.b2; g.resid = a.x2;
  if (side_x) { g.resid_side = side_x2; g.out_side = side_out; g.side_S = sS; g.side_M = sM; }
  return xp_gemm(&g, st);
}

// The part of a backward workspace the shared stages use, for n rows: [dpre | dh2 | dx2 | dattn] activation-gradient temporaries,
// fc1's bias-gradient partial rows, the second LayerNorm's partial rows, the batched-reduce scratch.
struct TailBwdPlan {
  size_t esz, dpre, dh, cs_pre, ln2, red, bytes, slabs;     // slabs: what the stage's three dW GEMMs need (not part of bytes)
  int64_t db1_fused_rows, cs_pre_rows, ln_rows;
};
struct TailBwdWs { void *dpre, *dh2, *dx2, *dattn, *red; float *cs_pre, *ln2_part; };
// db1_fused_rows: partial rows of fc1's bias gradient out of the dpre GEMM's epilogue (xp_gemm_colsum_rows), 0 = a separate
// column-sum pass over dpre
TailBwdPlan plan_tail_bwd(int64_t n, int64_t D, int64_t Dff, int dt, int64_t db1_fused_rows) {
  TailBwdPlan p;
  memset(&p, 0, sizeof(p));
  p.esz = dt == XP_BF16 ? 2 : 4;
  p.dpre = align256(n * Dff * p.esz); p.dh = align256(n * D * p.esz);
  p.db1_fused_rows = db1_fused_rows;
  p.cs_pre_rows = db1_fused_rows > 0 ? db1_fused_rows : xp_colsum_partial_rows(n, Dff);
  p.cs_pre = align256(p.cs_pre_rows * Dff * sizeof(float));
  p.ln_rows = xp_layernorm_bwd_partial_rows(n);
  p.ln2 = align256(xp_layernorm_bwd_workspace_bytes(n, D));
  p.red = align256((size_t)XP_REDUCE_MAX_SEGS * 32 * (size_t)(3 * D > Dff ? 3 * D : Dff) * sizeof(float) + 16);
  p.bytes = p.dpre + 3 * p.dh + p.cs_pre + p.ln2 + p.red;
  p.slabs = max_slab_bytes(0, {wgrad_desc(nullptr, nullptr, nullptr, n, D, Dff, dt), wgrad_desc(nullptr, nullptr, nullptr, n, Dff, D, dt),
                               wgrad_desc(nullptr, nullptr, nullptr, n, D, D, dt)});
  return p;
}
TailBwdWs carve_tail_bwd(Carver& ws, const TailBwdPlan& p) {
  TailBwdWs w;
  w.dpre = ws.take(p.dpre); w.dh2 = ws.take(p.dh); w.dx2 = ws.take(p.dh); w.dattn = ws.take(p.dh);
  w.cs_pre = (float*)ws.take(p.cs_pre); w.ln2_part = (float*)ws.take(p.ln2); w.red = ws.take(p.red);
  return w;
}

// x3 = x2 + fc2(act(fc1(LN2(x2)))) and x2 = resid + out_proj(attn_o), backwards: leaves dx2 and dattn in the workspace,
// issues dW2, dW1, dWo and defers db1, dln2_w, dln2_b, dbo, db2.  Marks 1 and 2 of the weight-gradient stream.
template <class Args>
int mlp_out_proj_bwd(const Args& a, int64_t n, const TailBwdPlan& p, const TailBwdWs& w, float* slabs, size_t slab_bytes, int64_t sS,
                     int32_t sM, Defer& df, const WgradOrder& wg, void* st) {
  const int64_t D = a.dims.D, Dff = a.dims.Dff;
  const int dt = a.dims.dtype;
  int rc;
  XpGemmDesc g = gemm_desc(a.dx3, a.W2, w.dpre, n, Dff, D, dt);               // dpre = (dx3 . W2) * act'(pre)
  g.b_kstrided = 1; g.ldb = Dff; g.epilogue = epi_act_bwd(a.dims); g.resid = a.pre; g.ldr = Dff;
  if (a.db1 && p.db1_fused_rows > 0) g.colsum_partials = w.cs_pre;
  if ((rc = xp_gemm(&g, st))) return rc;
  if (a.db1) {
    if (p.db1_fused_rows == 0 && (rc = xp_colsum_partials(w.dpre, n, Dff, Dff, dt, w.cs_pre, p.cs_pre, st))) return rc;
    df.add(w.cs_pre, a.db1, Dff, (int)p.cs_pre_rows, (int)Dff);
  }
  if (a.dw2 && (rc = run_wgrad(wgrad_desc(a.dx3, a.act, a.dw2, n, D, Dff, dt), slabs, slab_bytes, wg.stream(), true))) return rc;
  if ((rc = wg.mark(1))) return rc;                                           // dpre is ready for dW1
  g = gemm_desc(w.dpre, a.W1, w.dh2, n, D, Dff, dt);                          // dh2 = dpre . W1
  g.b_kstrided = 1; g.ldb = D;
  if ((rc = xp_gemm(&g, st))) return rc;
  if (a.dw1 && (rc = run_wgrad(wgrad_desc(w.dpre, a.h2, a.dw1, n, Dff, D, dt), slabs, slab_bytes, wg.stream(), true))) return rc;
  // dx2 = dx3 + LN2'(dh2); partial rows [dgamma | dbeta | colsum(dx2) | colsum(dx3)] -- out_proj's and fc2's bias gradients
  if ((rc = xp_layernorm_bwd_partials_side(w.dh2, D, a.x2, D, a.ln2_w, a.mean2, a.rstd2, a.dx3, D, w.dx2, D, 2, n, D, dt,
                                           a.side_x2, sS, sM, sM, w.ln2_part, p.ln2, st))) return rc;
  df.add(w.ln2_part, a.dln2_w, 4 * D, (int)p.ln_rows, (int)D);
  df.add(w.ln2_part + D, a.dln2_b, 4 * D, (int)p.ln_rows, (int)D);
  df.add(w.ln2_part + 2 * D, a.dbo, 4 * D, (int)p.ln_rows, (int)D);
  df.add(w.ln2_part + 3 * D, a.db2, 4 * D, (int)p.ln_rows, (int)D);
  if ((rc = wg.mark(2))) return rc;                                           // dx2 is ready for dWo
  g = gemm_desc(w.dx2, a.Wo, w.dattn, n, D, D, dt);                           // dattn = dx2 . Wo
  g.b_kstrided = 1; g.ldb = D;
  if ((rc = xp_gemm(&g, st))) return rc;
  if (a.dwo && (rc = run_wgrad(wgrad_desc(w.dx2, a.attn_o, a.dwo, n, D, D, dt), slabs, slab_bytes, wg.stream(), true))) return rc;
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

extern "C" void* xp_side_stream(void) {
  WgradSide* w = wgrad_side();
  return w ? (void*)w->side : nullptr;
}

extern "C" size_t xp_encoder_layer_fwd_workspace_bytes(const XpLayerDims* d) {
  if (!d) return 0;
  // + the fp32 side rows of x2 (video: the proxy tokens; text: every row), used when XpLayerFwd::side_in is given
  const size_t side_rows = d->attn_mode == XP_ATTN_PROXY ? (size_t)d->B * d->M : (size_t)d->rows;
  return align256(xp_attn_workspace_bytes(d->attn_mode, d->B, d->heads, d->M, d->N, d->L)) + align256(side_rows * d->D * sizeof(float)) + 256;
}

extern "C" int xp_encoder_layer_fwd(const XpLayerFwd* a, void* st) {
  XP_REQUIRE(a, "xp_encoder_layer_fwd: null argument");
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
  const size_t attn_ws = align256(xp_attn_workspace_bytes(d.attn_mode, d.B, d.heads, d.M, d.N, d.L));
  const int64_t sS = a->side_S;
  const int32_t sM = a->side_M;
  XP_REQUIRE(!sided || a->workspace_bytes >= attn_ws + align256((size_t)(cdiv(rows, sS) * sM) * D * sizeof(float)),
             "xp_encoder_layer_fwd: workspace too small for the side rows");
  float* side_x2 = !sided ? nullptr : a->side_x2 ? a->side_x2 : reinterpret_cast<float*>(static_cast<char*>(a->workspace) + attn_ws);
  // h1 = LN1(x)
  if ((rc = xp_layernorm_fwd_side(a->x, D, a->ln1_w, a->ln1_b, a->h1, D, a->mean1, a->rstd1, rows, D, d.ln_eps, dt,
                                  a->side_in, nullptr, sS, sM, sM, st))) return rc;
  // qkv = (h1 Wqkv^T + b), q columns scaled by dh^-0.5 (:341)
  XpGemmDesc g = gemm_desc(a->h1, a->Wqkv, a->qkv, rows, 3 * D, D, dt);
  g.epilogue = XP_EPI_BIAS_QSCALE; g.bias = a->bqkv; g.scale = d.q_scale; g.scale_cols = D;
  if ((rc = xp_gemm(&g, st))) return rc;
  if ((rc = xp_attn_fwd(a->qkv, 3 * D, a->attn_o, D, a->stats, a->pad_mask, d.attn_mode, d.B, d.heads, d.S, d.M, d.N, d.L, dt,
                        a->workspace, a->workspace_bytes, st))) return rc;
  return out_proj_mlp_fwd(*a, rows, D, a->side_in, side_x2, a->side_out, sS, sM, st);
}

// workspace of the backward: the shared stages' part (TailBwdPlan), [dqkv | dh1], split-K slabs, the q/k/v bias-gradient and first
// LayerNorm's partial rows, the attention workspace
namespace {
struct BwdPlan {
  TailBwdPlan t;
  size_t dqkv, slabs, cs_qkv, ln1, attn, total;
  int64_t cs_qkv_rows;
  bool cs_qkv_fused;
};
BwdPlan plan_bwd(const XpLayerDims& d) {
  BwdPlan p;
  memset(&p, 0, sizeof(p));
  const int64_t rows = d.rows, D = d.D, Dff = d.Dff;
  // fc1's bias gradient: fused into the dX GEMM epilogue where the library offers it, else a column-sum pass over dpre
  XpGemmDesc g = gemm_desc(nullptr, nullptr, nullptr, rows, Dff, D, d.dtype);
  g.b_kstrided = 1; g.ldb = Dff; g.epilogue = epi_act_bwd(d); g.ldr = Dff;
  g.resid = &g;                          // (only tested for non-NULL by the planning queries)
  p.t = plan_tail_bwd(rows, D, Dff, d.dtype, xp_gemm_colsum_rows(&g));
  // (fc2's bias gradient = column sums of dx3: taken by the second LayerNorm's backward)
  p.dqkv = align256(rows * 3 * D * p.t.esz);
  p.slabs = align256(max_slab_bytes(p.t.slabs, {wgrad_desc(nullptr, nullptr, nullptr, rows, 3 * D, D, d.dtype)}));
  // the q/k/v bias gradients: out of the attention backward kernels where they offer it, else a column-sum pass over dqkv
  p.cs_qkv_rows = xp_attn_bwd_colsum_rows(d.attn_mode, d.B, d.heads, d.S, d.M, d.N, d.L, d.dtype);
  p.cs_qkv_fused = p.cs_qkv_rows > 0;
  if (!p.cs_qkv_fused) p.cs_qkv_rows = xp_colsum_partial_rows(rows, 3 * D);
  p.cs_qkv = align256(p.cs_qkv_rows * 3 * D * sizeof(float));
  p.ln1 = p.t.ln2;                       // (both LayerNorms run over the same [rows, D])
  p.attn = align256(xp_attn_workspace_bytes(d.attn_mode, d.B, d.heads, d.M, d.N, d.L));
  p.total = p.t.bytes + p.dqkv + p.t.dh + p.slabs + p.cs_qkv + p.ln1 + p.attn + 256;
  return p;
}
}  // namespace

extern "C" size_t xp_encoder_layer_bwd_workspace_bytes(const XpLayerDims* d) {
  if (!d || d->rows <= 0) return 0;
  return plan_bwd(*d).total;
}

extern "C" int xp_encoder_layer_bwd(const XpLayerBwd* a, void* st) {
  XP_REQUIRE(a, "xp_encoder_layer_bwd: null argument");
  const XpLayerDims& d = a->dims;
  int rc = check_dims("xp_encoder_layer_bwd", d);
  if (rc) return rc;
  XP_REQUIRE(a->x && a->h1 && a->qkv && a->attn_o && a->x2 && a->h2 && a->pre && a->act && a->Wqkv && a->Wo && a->W1 && a->W2 &&
             a->ln1_w && a->ln2_w && a->mean1 && a->rstd1 && a->mean2 && a->rstd2 && a->stats && a->dx3 && a->dx,
             "xp_encoder_layer_bwd: null pointer");
  XP_REQUIRE((!a->side_in && !a->side_x2) || (a->side_in && a->side_x2 && d.dtype == XP_BF16 && a->side_S > 0 && a->side_M > 0 &&
                                               a->side_M <= a->side_S),
             "xp_encoder_layer_bwd: side rows need side_in and side_x2, bf16 and 0 < side_M <= side_S");
  const BwdPlan p = plan_bwd(d);
  XP_REQUIRE(a->workspace && a->workspace_bytes >= p.total, "xp_encoder_layer_bwd: workspace too small (%zu < %zu)",
             a->workspace_bytes, p.total);
  Carver ws{(char*)a->workspace, 0, a->workspace_bytes};
  const TailBwdWs w = carve_tail_bwd(ws, p.t);
  void* dqkv = ws.take(p.dqkv); void* dh1 = ws.take(p.t.dh);
  float* slabs = (float*)ws.take(p.slabs);
  float* cs_qkv = (float*)ws.take(p.cs_qkv); float* ln1_part = (float*)ws.take(p.ln1);
  void* attn_ws = ws.take(p.attn);
  const int64_t rows = d.rows, D = d.D;
  const int dt = d.dtype;
  Defer df;
  // dW GEMMs beside the dX chain (video tower only: the text tower is 256 rows on a side stream of its own already)
  const WgradOrder wg{(d.attn_mode == XP_ATTN_PROXY && rows >= 4096) ? wgrad_side() : nullptr, (hipStream_t)st, "xp_encoder_layer_bwd"};
  if ((rc = wg.mark(0))) return rc;
  // ---- MLP: x3 = x2 + fc2(act(fc1(LN2(x2)))), then dattn = dx2 . Wo of x2 = x + out_proj(attn(qkv(LN1(x))))
  if ((rc = mlp_out_proj_bwd(*a, rows, p.t, w, slabs, p.slabs, a->side_S, a->side_M, df, wg, st))) return rc;
  // ---- attention
  if ((rc = xp_attn_bwd2(a->qkv, 3 * D, a->attn_o, w.dattn, D, a->stats, a->pad_mask, dqkv, d.q_scale, d.attn_mode, d.B, d.heads,
                         d.S, d.M, d.N, d.L, dt, attn_ws, p.attn, (a->dbqkv && p.cs_qkv_fused) ? cs_qkv : nullptr, st))) return rc;
  if ((rc = wg.mark(3))) return rc;                                           // dqkv is ready for dWqkv
  XpGemmDesc g = gemm_desc(dqkv, a->Wqkv, dh1, rows, D, 3 * D, dt);           // dh1 = dqkv . Wqkv
  g.b_kstrided = 1; g.ldb = D;
  if ((rc = xp_gemm(&g, st))) return rc;
  if (a->dwqkv && (rc = run_wgrad(wgrad_desc(dqkv, a->h1, a->dwqkv, rows, 3 * D, D, dt), slabs, p.slabs, wg.stream(), false))) return rc;
  if (a->dbqkv) {
    if (!p.cs_qkv_fused && (rc = xp_colsum_partials(dqkv, rows, 3 * D, 3 * D, dt, cs_qkv, p.cs_qkv, st))) return rc;
    df.add(cs_qkv, a->dbqkv, 3 * D, (int)p.cs_qkv_rows, (int)(3 * D));
  }
  if ((rc = xp_layernorm_bwd_partials_side(dh1, D, a->x, D, a->ln1_w, a->mean1, a->rstd1, w.dx2, D, a->dx, D, 0, rows, D, dt,
                                           a->side_in, a->side_S, a->side_M, a->side_M, ln1_part, p.ln1, st))) return rc;
  df.add(ln1_part, a->dln1_w, 2 * D, (int)p.t.ln_rows, (int)D);
  df.add(ln1_part + D, a->dln1_b, 2 * D, (int)p.t.ln_rows, (int)D);
  return finish_bwd(df, w.red, p.t.red, wg, st);
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

struct PooledBwdPlan {
  TailBwdPlan t;             // the shared stages over the B pooled rows
  size_t dqkv, dh1, slabs, cs_q, cs_kv, ln1, ln1p, attn, total;
  int64_t cs_q_rows, ln_rows;
};
PooledBwdPlan plan_pooled_bwd(const XpLayerDims& d) {
  PooledBwdPlan p;
  memset(&p, 0, sizeof(p));
  const int64_t rows = d.rows, D = d.D, B = d.B, S = d.S;
  const int dt = d.dtype;
  p.t = plan_tail_bwd(B, D, d.Dff, dt, 0);      // fc1's bias gradient: always a column-sum pass over dpre
  p.dqkv = align256(rows * 3 * D * p.t.esz); p.dh1 = align256(rows * D * p.t.esz);
  XpGemmDesc gq = wgrad_desc(nullptr, 3 * D, nullptr, D, nullptr, B, D, D, dt);       // dWq: dq of the pooled rows of dqkv
  gq.a_grp = 1; gq.a_grp_stride = S;
  p.slabs = align256(max_slab_bytes(p.t.slabs, {gq, wgrad_desc(nullptr, 3 * D, nullptr, D, nullptr, rows, 2 * D, D, dt)}));
  p.cs_q_rows = xp_colsum_partial_rows(B, D);
  p.cs_q = align256(p.cs_q_rows * D * sizeof(float));
  p.cs_kv = align256(xp_attn_pooled_colsum_rows_max(B, S) * 2 * D * sizeof(float));
  p.ln_rows = xp_layernorm_bwd_partial_rows(rows);
  p.ln1 = align256(xp_layernorm_bwd_workspace_bytes(rows, D));
  p.ln1p = p.t.ln2;                             // (LayerNorm 1 once more over the [B, D] pooled rows)
  p.attn = align256(xp_attn_pooled_workspace_bytes(B, d.heads, S, dt));
  p.total = p.t.bytes + p.dqkv + p.dh1 + p.slabs + p.cs_q + p.cs_kv + p.ln1 + p.ln1p + p.attn + 256;
  return p;
}

}  // namespace

extern "C" size_t xp_encoder_layer_pooled_fwd_workspace_bytes(const XpLayerDims* d) {
  if (!d || d->B <= 0 || d->D <= 0 || d->S <= 0 || d->heads <= 0) return 0;
  // the attention partials + two [B, D] fp32 side buffers (the pooled rows of side_in; side_x2 of a forward-only pass)
  return align256(xp_attn_pooled_workspace_bytes(d->B, d->heads, d->S, d->dtype)) + 2 * align256((size_t)d->B * d->D * sizeof(float)) + 256;
}

extern "C" int xp_encoder_layer_pooled_fwd(const XpLayerPooledFwd* a, void* st) {
  XP_REQUIRE(a, "xp_encoder_layer_pooled_fwd: null argument");
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
  const size_t attn_ws = align256(xp_attn_pooled_workspace_bytes(B, d.heads, S, dt)), side_b = align256((size_t)B * D * sizeof(float));
  XP_REQUIRE(a->workspace && a->workspace_bytes >= attn_ws + 2 * side_b, "xp_encoder_layer_pooled_fwd: workspace too small");
  float* side0 = !sided ? nullptr : reinterpret_cast<float*>(static_cast<char*>(a->workspace) + attn_ws);
  float* side_x2 = !sided ? nullptr : a->side_x2 ? a->side_x2 : reinterpret_cast<float*>(static_cast<char*>(a->workspace) + attn_ws + side_b);
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
  if ((rc = xp_attn_pooled_fwd(a->q, a->kv, 2 * D, a->attn_o, a->stats, B, d.heads, S, dt, a->workspace, attn_ws, st))) return rc;
  // x2 = x[pooled] + attn_o Wo^T + bo, then the MLP
  return out_proj_mlp_fwd(*a, B, S * D, side0, side_x2, a->side_out, s1, s1, st);
}

extern "C" size_t xp_encoder_layer_pooled_bwd_workspace_bytes(const XpLayerDims* d) {
  if (!d || d->rows <= 0 || d->B <= 0 || d->D <= 0 || d->Dff <= 0 || d->S <= 0 || d->heads <= 0) return 0;
  return plan_pooled_bwd(*d).total;
}

extern "C" int xp_encoder_layer_pooled_bwd(const XpLayerPooledBwd* a, void* st) {
  XP_REQUIRE(a, "xp_encoder_layer_pooled_bwd: null argument");
  const XpLayerDims& d = a->dims;
  int rc = check_pooled_dims("xp_encoder_layer_pooled_bwd", d);
  if (rc) return rc;
  XP_REQUIRE(a->x && a->h1 && a->kv && a->h1p && a->q && a->attn_o && a->x2 && a->h2 && a->pre && a->act && a->Wqkv && a->Wo &&
             a->W1 && a->W2 && a->ln1_w && a->ln2_w && a->mean1 && a->rstd1 && a->mean1p && a->rstd1p && a->mean2 && a->rstd2 &&
             a->stats && a->dx3 && a->dx, "xp_encoder_layer_pooled_bwd: null pointer");
  XP_REQUIRE((!a->side_in && !a->side_x2) || (a->side_in && a->side_x2 && d.dtype == XP_BF16),
             "xp_encoder_layer_pooled_bwd: side rows need side_in and side_x2, and bf16");
  const PooledBwdPlan p = plan_pooled_bwd(d);
  XP_REQUIRE(a->workspace && a->workspace_bytes >= p.total, "xp_encoder_layer_pooled_bwd: workspace too small (%zu < %zu)",
             a->workspace_bytes, p.total);
  Carver ws{(char*)a->workspace, 0, a->workspace_bytes};
  const TailBwdWs w = carve_tail_bwd(ws, p.t);
  char* dqkv = (char*)ws.take(p.dqkv); void* dh1 = ws.take(p.dh1);
  float* slabs = (float*)ws.take(p.slabs);
  float* cs_q = (float*)ws.take(p.cs_q); float* cs_kv = (float*)ws.take(p.cs_kv);
  float* ln1_part = (float*)ws.take(p.ln1); float* ln1p_part = (float*)ws.take(p.ln1p);
  void* attn_ws = ws.take(p.attn);
  const int64_t rows = d.rows, D = d.D, B = d.B, S = d.S;
  const int dt = d.dtype;
  const bool sided = a->side_in != nullptr;
  const int64_t sS = sided ? S : 0;
  const int32_t sM = sided ? (int32_t)d.M : 0, s1 = sided ? 1 : 0;
  void* dkv = dqkv + (size_t)D * p.t.esz;    // dqkv[rows, 3D]: the k / v columns of every row, the q columns of the pooled rows only
  Defer df;
  const WgradOrder wg{rows >= 4096 ? wgrad_side() : nullptr, (hipStream_t)st, "xp_encoder_layer_pooled_bwd"};
  if ((rc = wg.mark(0))) return rc;
  // ---- MLP and dattn = dx2 . Wo on the pooled rows
  if ((rc = mlp_out_proj_bwd(*a, B, p.t, w, slabs, p.slabs, s1, s1, df, wg, st))) return rc;
  // ---- attention: dq lands in the q columns of the pooled rows of dqkv, dk / dv in the k / v columns of every row
  if ((rc = xp_attn_pooled_bwd(a->q, a->kv, 2 * D, a->attn_o, w.dattn, a->stats, dqkv, S * 3 * D, dkv, 3 * D, d.q_scale, B, d.heads,
                               S, dt, attn_ws, p.attn, a->dbqkv ? cs_kv : nullptr, st))) return rc;
  if ((rc = wg.mark(3))) return rc;
  // dh1 = dkv . Wkv on every row, then the pooled rows again with their q columns: dqkv[b*S] . Wqkv
  XpGemmDesc g = gemm_desc(dkv, static_cast<const char*>(a->Wqkv) + (size_t)D * D * p.t.esz, dh1, rows, D, 2 * D, dt);
  g.lda = 3 * D; g.b_kstrided = 1; g.ldb = D;
  if ((rc = xp_gemm(&g, st))) return rc;
  g = gemm_desc(dqkv, a->Wqkv, dh1, B, D, 3 * D, dt);
  g.a_grp = 1; g.a_grp_stride = S; g.b_kstrided = 1; g.ldb = D; g.c_grp = 1; g.c_grp_stride = S;
  if ((rc = xp_gemm(&g, st))) return rc;
  if (a->dwqkv) {
    g = wgrad_desc(dqkv, 3 * D, a->h1p, D, a->dwqkv, B, D, D, dt);            // dWq = dq^T . h1p
    g.a_grp = 1; g.a_grp_stride = S;
    if ((rc = run_wgrad(g, slabs, p.slabs, wg.stream(), true))) return rc;
    if ((rc = run_wgrad(wgrad_desc(dkv, 3 * D, a->h1, D, a->dwqkv + D * D, rows, 2 * D, D, dt), slabs, p.slabs, wg.stream(), false))) return rc;
  }
  if (a->dbqkv) {
    const int64_t kv_rows = xp_attn_pooled_colsum_rows(B, d.heads, S, dt);
    XP_REQUIRE(kv_rows > 0, "xp_encoder_layer_pooled_bwd: no current device");
    if ((rc = xp_colsum_partials(dqkv, B, D, S * 3 * D, dt, cs_q, p.cs_q, st))) return rc;
    df.add(cs_q, a->dbqkv, D, (int)p.cs_q_rows, (int)D);
    df.add(cs_kv, a->dbqkv + D, 2 * D, (int)kv_rows, (int)(2 * D));
  }
  // dx = LN1'(dh1) on every row; the pooled rows once more with their residual gradient dx2 (the parameter-gradient partial
  // rows of that second pass are dropped: the first pass has counted those rows)
  if ((rc = xp_layernorm_bwd_partials_side(dh1, D, a->x, D, a->ln1_w, a->mean1, a->rstd1, nullptr, D, a->dx, D, 0, rows, D, dt,
                                           a->side_in, sS, sM, sM, ln1_part, p.ln1, st))) return rc;
  df.add(ln1_part, a->dln1_w, 2 * D, (int)p.ln_rows, (int)D);
  df.add(ln1_part + D, a->dln1_b, 2 * D, (int)p.ln_rows, (int)D);
  if ((rc = xp_layernorm_bwd_partials_side(dh1, S * D, a->x, S * D, a->ln1_w, a->mean1p, a->rstd1p, w.dx2, D, a->dx, S * D, 0, B, D, dt,
                                           a->side_in, s1, s1, sM, ln1p_part, p.ln1p, st))) return rc;
  return finish_bwd(df, w.red, p.t.red, wg, st);
}
