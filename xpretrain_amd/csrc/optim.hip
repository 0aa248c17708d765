// On-device optimizer step: global gradient-norm clip + the update of ALL parameter tensors in one
// multi-tensor launch, fp32 master weights, optional compute-dtype shadow copies written in the same pass.  Three updates, one
// per value of the drivers' `optim` key (src/configs/config.py:135-137, src/optimization/utils.py:111-120):
//
//   adam1                   restates  src/optimization/adamw.py:40-103  (AdamW.step: m/v update, denom = sqrt(v) + eps,
//                           bias-corrected step size, decoupled weight decay AFTER the Adam update with the group's lr)
//   opt1<XP_OPT_ADAM>       torch.optim.Adam   as utils.py:119 builds it (single-tensor path, amsgrad = maximize = False)
//   opt1<XP_OPT_ADAMAX>     torch.optim.Adamax likewise
//     both: coupled L2 decay added to the CLIPPED gradient before the moments; the bias corrections applied where torch applies
//     them (Adam: sqrt(v) / sqrt(1-b2^t) + eps; Adamax: eps inside the max operand) -- see opt1 below
//
// and torch.nn.utils.clip_grad_norm_ as called by the training loops (run_video_retrieval.py:390-392):
// coef = min(1, max_norm / (||g||_2 + 1e-6)).
//
// One decomposition for all of them:
//   walk<UPDATE>(tensor, chunk, g, one)   one workgroup over one 64 Ki-element chunk: the 16-byte path where every pointer it touches
//                                         allows it, the scalar tail, the bf16 / fp32 shadow stores.  UPDATE: `one` on (p, g, m, v);
//                                         else the shadows alone, rewritten from p
//   norm_of / clip_coef                   the gradient norm from the per-chunk partials and the clip coefficient, written once
//   update_kernel<KIND, GUARDED>          the six update kernels: norm and coefficient (unguarded: from the partials, when given;
//                                         guarded: from the step's verdict), then walk with adam1 or opt1<KIND>
//   verdict_kernel                        the opt-in step guard: decides once per step whether norm_of is finite.  Behind a verdict
//                                         that is not, a guarded update leaves p, m, v alone and rewrites the shadows from p
// The bits of the three updates are held by tests/test_optim_bits_gpu.py.
//
// HBM-bound: per element 16 B read (p, g, m, v) + 12 B written (p, m, v) + 2 B shadow, the same for all three; the norm pass reads
// g once more.
// Work decomposition: fixed 64 Ki-element CHUNKS of one tensor per workgroup (chunk map built once on the host side of
// the ABI); the gradient pointers, which change every step, travel in the kernel argument block, everything static
// lives in a device table.  All reductions are fixed-order (deterministic): per-chunk partial sums of squares, and
// every workgroup of the update kernel re-derives the same total from the partials array.
#include "common.h"

namespace {

constexpr int NT = 256;                      // threads per workgroup
constexpr int CHUNK = XP_OPT_CHUNK;          // elements per workgroup
constexpr int MAXT = XP_OPT_MAX_TENSORS, MAXG = XP_OPT_MAX_GROUPS;
constexpr int KIND_ADAMW = -1;               // beside XpOptKind, inside this file only

template <typename Group>                    // XpAdamGroup (AdamW) or XpOptGroup (Adam, Adamax)
struct UpdateArgs {
  const float* g[MAXT];
  unsigned char grp[MAXT];
  Group groups[MAXG];
};
struct NormArgs { const float* g[MAXT]; };

__device__ __forceinline__ float block_sum(float v) {
  __shared__ float red[NT / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) s += red[i];
  return s;
}

__global__ __launch_bounds__(NT) void sqnorm_partials_kernel(const XpAdamTensor* __restrict__ table,
                                                             const int32_t* __restrict__ chunk_map, NormArgs a,
                                                             float* __restrict__ partials) {
  const int t = chunk_map[2 * blockIdx.x], c = chunk_map[2 * blockIdx.x + 1];
  const int64_t n = table[t].numel, beg = (int64_t)c * CHUNK;
  const int64_t len = n - beg < CHUNK ? n - beg : CHUNK;
  const float* g = a.g[t] + beg;
  float s = 0.f;
  if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
    const int64_t n4 = len >> 2;
    for (int64_t i = threadIdx.x; i < n4; i += NT) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(g + 4 * i);
      s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    for (int64_t i = (n4 << 2) + threadIdx.x; i < len; i += NT) s += g[i] * g[i];
  } else {
    for (int64_t i = threadIdx.x; i < len; i += NT) s += g[i] * g[i];
  }
  s = block_sum(s);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// One element.  Every rounding point is written out (no compiler-chosen contraction): left to itself hipcc fused  m*b1 + (1-b1)*g  as
// fma(b1, m, [(1-b1)*g]) in this kernel and as fma(1-b1, g, [b1*m]) in a second update kernel built from the same source
// (tools/experiments/adamw_confined.diff).  The form is the one adamw_kernel has compiled to since round 2 (tests/golden/optim.pt: 2e-5).
__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, const XpAdamGroup& h, float coef) {
#pragma clang fp contract(off)
  g = g * coef;
  m = __builtin_fmaf(h.beta1, m, (1.0f - h.beta1) * g);
  v = __builtin_fmaf(h.beta2, v, g * ((1.0f - h.beta2) * g));
  const float denom = sqrtf(v) + h.eps;
  p = __builtin_fmaf(-h.step_size, m / denom, p);
  if (h.weight_decay > 0.f) p = __builtin_fmaf(-(h.lr * h.weight_decay), p, p);
}

// One element of torch.optim.Adam / Adamax (torch/optim/adam.py::_single_tensor_adam, adamax.py::_single_tensor_adamax).  Every
// rounding point is written out, as in adam1.  The form chosen:
//   decay       one fma(wd, p, g)                                  (torch: add with alpha)
//   exp_avg     torch's lerp_, m + w * (g - m), as fma(w, [g - m], m) with w = 1-b1 formed in double on the host, as torch forms it.
//               NOT adam1's fma(b1, m, [(1-b1)*g]) with 1-b1 in fp32: 1 - 0.8f is not 0.2f, and over 8 steps that bias alone put
//               exp_avg 4.6 x torch's own fp32 error away from fp64 torch (lerp with the fp32 difference: 3.1 x; this form: 1.3 x;
//               the unclipped eps = 1e-3 case of tests/test_optim_family_gpu.py: the first figure from a CPU emulation of the
//               kernel's arithmetic, the other two on the MI355X)
//   exp_avg_sq  adam1's fma(b2, v, [g * ((1-b2)*g)])               (torch: mul_ then addcmul_)
//   denominator torch's own rounding points: sqrt, correctly rounded division by sqrt(1-b2^t), then + eps
//   parameter   fma(-step_size, [m / denom], p)                    (torch: addcdiv_)
// Adamax's maximum keeps a NaN from either operand, as torch's amax does (fmaxf would drop it).
template <int KIND>
__device__ __forceinline__ void opt1(float& p, float g, float& m, float& v, const XpOptGroup& h, float coef) {
#pragma clang fp contract(off)
  g = g * coef;
  if (h.weight_decay != 0.f) g = __builtin_fmaf(h.weight_decay, p, g);
  m = __builtin_fmaf(h.one_minus_beta1, g - m, m);
  float denom;
  if (KIND == XP_OPT_ADAM) {
    v = __builtin_fmaf(h.beta2, v, g * ((1.0f - h.beta2) * g));
    denom = sqrtf(v) / h.bias2_sqrt + h.eps;
  } else {
    const float a = h.beta2 * v, b = fabsf(g) + h.eps;
    v = (a >= b || a != a) ? a : b;
    denom = v;
  }
  p = __builtin_fmaf(-h.step_size, m / denom, p);
}

// The gradient norm from the per-chunk partials: thread-strided, then block_sum.  Every workgroup of an unguarded clipped update and
// the verdict kernel call this, so they hold the same bits.  each(i, partials[i]) sees every partial on its way into the sum.
template <typename F>
__device__ __forceinline__ float norm_of(const float* __restrict__ partials, int n, F each) {
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += NT) {
    const float x = partials[i];
    s += x;
    each(i, x);
  }
  return sqrtf(block_sum(s));
}

__device__ __forceinline__ float clip_coef(float norm, float max_norm) {
  if (max_norm > 0.f) { const float c = max_norm / (norm + 1e-6f); return c < 1.0f ? c : 1.0f; }
  return 1.0f;
}

// Chunk c of one tensor.  UPDATE: one(p, g, m, v) on every element, p, m, v stored back, the shadow copy written from the new p.
// Not UPDATE: neither m, v nor g is touched and p is not written; the shadow copy, if there is one, is rewritten from p.
template <bool UPDATE, typename F>
__device__ __forceinline__ void walk(const XpAdamTensor& tt, int c, const float* gt, F one) {
  const int64_t beg = (int64_t)c * CHUNK;
  const int64_t len = tt.numel - beg < CHUNK ? tt.numel - beg : CHUNK;
  float* p = reinterpret_cast<float*>(tt.p) + beg;
  bf16_t* sb = tt.shadow && tt.shadow_dtype == XP_BF16 ? reinterpret_cast<bf16_t*>(tt.shadow) + beg : nullptr;
  float* sf = tt.shadow && tt.shadow_dtype == XP_F32 ? reinterpret_cast<float*>(tt.shadow) + beg : nullptr;
  if (!UPDATE && !sb && !sf) return;
  float* m = UPDATE ? reinterpret_cast<float*>(tt.m) + beg : nullptr;
  float* v = UPDATE ? reinterpret_cast<float*>(tt.v) + beg : nullptr;
  const float* g = UPDATE ? gt + beg : nullptr;
  const uintptr_t align = reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v) |
                          reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(sf) |
                          (reinterpret_cast<uintptr_t>(sb) << 1);
  int64_t done = 0;
  if ((align & 15) == 0) {
    const int64_t n4 = len >> 2;
    for (int64_t i = threadIdx.x; i < n4; i += NT) {
      f32x4 pp = *reinterpret_cast<f32x4*>(p + 4 * i);
      if constexpr (UPDATE) {
        f32x4 mm = *reinterpret_cast<f32x4*>(m + 4 * i), vv = *reinterpret_cast<f32x4*>(v + 4 * i);
        const f32x4 gg = *reinterpret_cast<const f32x4*>(g + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float pe = pp[e], me = mm[e], ve = vv[e];
          one(pe, gg[e], me, ve);
          pp[e] = pe; mm[e] = me; vv[e] = ve;
        }
        *reinterpret_cast<f32x4*>(p + 4 * i) = pp;
        *reinterpret_cast<f32x4*>(m + 4 * i) = mm;
        *reinterpret_cast<f32x4*>(v + 4 * i) = vv;
      }
      if (sb) *reinterpret_cast<bf16x4*>(sb + 4 * i) = bf16x4{(bf16_t)pp[0], (bf16_t)pp[1], (bf16_t)pp[2], (bf16_t)pp[3]};
      if (sf) *reinterpret_cast<f32x4*>(sf + 4 * i) = pp;
    }
    done = n4 << 2;
  }
  for (int64_t i = done + threadIdx.x; i < len; i += NT) {
    float pp = p[i];
    if constexpr (UPDATE) {
      float mm = m[i], vv = v[i];
      one(pp, g[i], mm, vv);
      p[i] = pp; m[i] = mm; v[i] = vv;
    }
    if (sb) sb[i] = (bf16_t)pp;
    if (sf) sf[i] = pp;
  }
}

// The three updates, unguarded and behind a verdict.  Unguarded: the norm and the coefficient from the partials when they are given
// (then norm_out, if not null, gets the norm); the verdict is not read.  GUARDED: both from the verdict xp_step_verdict left (norm_out,
// if not null, always gets its norm); the partials are not touched.  Behind a verdict that is not finite the workgroup touches neither
// m, v nor the gradient and does not write p; it rewrites its chunk of the shadow copy from the unchanged p, so that the weight cache's
// "this step rewrote every entry" holds either way.
template <int KIND, bool GUARDED, typename Group>
__global__ __launch_bounds__(NT) void update_kernel(const XpAdamTensor* __restrict__ table, const int32_t* __restrict__ chunk_map,
                                                    UpdateArgs<Group> a, const float* __restrict__ partials, int n_partials,
                                                    float max_norm, const XpStepVerdict* __restrict__ verdict,
                                                    float* __restrict__ norm_out) {
  float coef = 1.0f;
  if (GUARDED || partials != nullptr) {
    float norm;
    if constexpr (GUARDED) norm = verdict->norm;
    else norm = norm_of(partials, n_partials, [](int, float) {});
    coef = clip_coef(norm, max_norm);
    if (blockIdx.x == 0 && threadIdx.x == 0 && norm_out) norm_out[0] = norm;
  }
  const int t = chunk_map[2 * blockIdx.x], c = chunk_map[2 * blockIdx.x + 1];
  const XpAdamTensor tt = table[t];
  if constexpr (GUARDED) {
    if (verdict->finite == 0) { walk<false>(tt, c, nullptr, nullptr); return; }
  }
  const Group h = a.groups[a.grp[t]];
  walk<true>(tt, c, a.g[t], [&](float& p, float g, float& m, float& v) {
    if constexpr (KIND == KIND_ADAMW) adam1(p, g, m, v, h, coef);
    else opt1<KIND>(p, g, m, v, h, coef);
  });
}

// ---------------------------------------------------------------------------------------------- the step guard (xp_step_verdict)
// One workgroup behind the partials of ALL launch tables of the step.  Launches on one stream are ordered: the counters are a plain
// load and store by one lane.
__global__ __launch_bounds__(NT) void verdict_kernel(const float* __restrict__ partials, int n_partials,
                                                     XpStepVerdict* __restrict__ verdict) {
  __shared__ int first[NT / 64];
  int bad = n_partials;                        // lowest chunk of this thread whose own partial is not finite
  const float norm = norm_of(partials, n_partials, [&](int i, float x) { if (!__builtin_isfinite(x) && i < bad) bad = i; });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const int b = __shfl_xor(bad, o); bad = b < bad ? b : bad; }
  if ((threadIdx.x & 63) == 0) first[threadIdx.x >> 6] = bad;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 1; i < NT / 64; ++i) bad = first[i] < bad ? first[i] : bad;
    const bool finite = __builtin_isfinite(norm);
    verdict->norm = norm;
    verdict->finite = finite ? 1 : 0;
    verdict->first_bad_chunk = bad < n_partials ? bad : -1;
    if (finite) verdict->applied = verdict->applied + 1;
    else verdict->skipped = verdict->skipped + 1;
  }
}

// ---------------------------------------------------------------------------------------------- host side of the four update calls
template <typename Group>
struct UpdateCall {                            // the arguments of xp_adamw_step[_guarded] / xp_optim_step[_guarded], as the ABI names them
  const XpAdamTensor* table; const int32_t* chunk_map; int32_t n_chunks;
  const void* const* grads_host; const uint8_t* group_of_host; int32_t n_tensors;
  const Group* groups_host; int32_t n_groups;
  const float* norm_partials; int32_t n_norm_partials; float max_norm; float* grad_norm_out;
  const XpStepVerdict* verdict; void* stream;
};

// The argument checks and the argument block of an update call.
template <typename Group>
int check_and_fill(const char* name, const UpdateCall<Group>& u, bool guarded, UpdateArgs<Group>& a) {
  XP_REQUIRE(!guarded || u.verdict, "%s: null verdict (xp_step_verdict writes it, behind the partials of the whole step)", name);
  XP_REQUIRE(u.table && u.chunk_map && u.grads_host && u.group_of_host && u.groups_host && u.n_chunks > 0, "%s: null argument", name);
  XP_REQUIRE(u.n_tensors > 0 && u.n_tensors <= MAXT, "%s: n_tensors=%d not in 1..%d", name, u.n_tensors, MAXT);
  if (int rc = xp_check_aligned(name, 16, {XpPtrName{"table", u.table}, XpPtrName{"chunk_map", u.chunk_map}, XpPtrName{"norm_partials", u.norm_partials},
                                           XpPtrName{"grad_norm_out", u.grad_norm_out}, XpPtrName{"verdict", u.verdict}}))
    return rc;
  XP_REQUIRE(u.n_groups > 0 && u.n_groups <= MAXG, "%s: n_groups=%d not in 1..%d", name, u.n_groups, MAXG);
  XP_REQUIRE(u.norm_partials || u.max_norm <= 0.f, "%s: max_norm > 0 needs the gradient-norm partials", name);
  XP_REQUIRE(!u.norm_partials || u.n_norm_partials > 0, "%s: n_norm_partials must be positive", name);
  for (int i = 0; i < MAXT; ++i) { a.g[i] = nullptr; a.grp[i] = 0; }
  for (int i = 0; i < u.n_tensors; ++i) {
    XP_REQUIRE(u.grads_host[i], "%s: gradient %d is null", name, i);
    XP_REQUIRE(u.group_of_host[i] < u.n_groups, "%s: tensor %d has group %d >= %d", name, i, u.group_of_host[i], u.n_groups);
    a.g[i] = reinterpret_cast<const float*>(u.grads_host[i]);
    a.grp[i] = u.group_of_host[i];
  }
  for (int i = 0; i < u.n_groups; ++i) a.groups[i] = u.groups_host[i];
  for (int i = u.n_groups; i < MAXG; ++i) a.groups[i] = u.groups_host[0];
  return XP_OK;
}

template <int KIND, bool GUARDED, typename Group>
int launch_update(const char* name, const UpdateCall<Group>& u) {
  UpdateArgs<Group> a;
  const int rc = check_and_fill(name, u, GUARDED, a);
  if (rc != XP_OK) return rc;
  update_kernel<KIND, GUARDED><<<u.n_chunks, NT, 0, (hipStream_t)u.stream>>>(u.table, u.chunk_map, a, u.norm_partials, u.n_norm_partials,
                                                                             u.max_norm, u.verdict, u.grad_norm_out);
  XP_CHECK_LAUNCH(name);
  return XP_OK;
}

template <bool GUARDED>
int launch_optim(const char* name, int32_t kind, const UpdateCall<XpOptGroup>& u) {
  XP_REQUIRE(kind == XP_OPT_ADAM || kind == XP_OPT_ADAMAX, "%s: unknown kind %d (XP_OPT_ADAM = %d, XP_OPT_ADAMAX = %d)", name, kind,
             (int)XP_OPT_ADAM, (int)XP_OPT_ADAMAX);
  return kind == XP_OPT_ADAM ? launch_update<XP_OPT_ADAM, GUARDED>(name, u) : launch_update<XP_OPT_ADAMAX, GUARDED>(name, u);
}

}  // namespace

extern "C" int xp_grad_sqnorm_partials(const XpAdamTensor* table, const int32_t* chunk_map, int32_t n_chunks,
                                       const void* const* grads_host, int32_t n_tensors, float* partials, void* stream) {
  XP_REQUIRE(table && chunk_map && grads_host && partials && n_chunks > 0, "xp_grad_sqnorm_partials: null argument");
  XP_REQUIRE(n_tensors > 0 && n_tensors <= MAXT, "xp_grad_sqnorm_partials: n_tensors=%d not in 1..%d", n_tensors, MAXT);
  // (the gradients and the tensors the table names: alignment class `any` -- the kernels take their 16-byte path per chunk only where
  //  every pointer of the chunk allows it, else one float per access; partials: one float per workgroup, and a launch table of
  //  optimization/multi_tensor.py writes its slice of the step's array from an arbitrary chunk on)
  XP_REQUIRE_ALIGNED("xp_grad_sqnorm_partials", 16, XP_P(table), XP_P(chunk_map));
  NormArgs a;
  for (int i = 0; i < n_tensors; ++i) {
    XP_REQUIRE(grads_host[i], "xp_grad_sqnorm_partials: gradient %d is null", i);
    a.g[i] = reinterpret_cast<const float*>(grads_host[i]);
  }
  for (int i = n_tensors; i < MAXT; ++i) a.g[i] = nullptr;
  sqnorm_partials_kernel<<<n_chunks, NT, 0, (hipStream_t)stream>>>(table, chunk_map, a, partials);
  XP_CHECK_LAUNCH("xp_grad_sqnorm_partials");
  return XP_OK;
}

extern "C" int xp_adamw_step(const XpAdamTensor* table, const int32_t* chunk_map, int32_t n_chunks,
                             const void* const* grads_host, const uint8_t* group_of_host, int32_t n_tensors,
                             const XpAdamGroup* groups_host, int32_t n_groups, const float* norm_partials,
                             int32_t n_norm_partials, float max_norm, float* grad_norm_out, void* stream) {
  return launch_update<KIND_ADAMW, false, XpAdamGroup>(
      "xp_adamw_step", {table, chunk_map, n_chunks, grads_host, group_of_host, n_tensors, groups_host, n_groups, norm_partials,
                        n_norm_partials, max_norm, grad_norm_out, nullptr, stream});
}

extern "C" int xp_optim_step(int32_t kind, const XpAdamTensor* table, const int32_t* chunk_map, int32_t n_chunks,
                             const void* const* grads_host, const uint8_t* group_of_host, int32_t n_tensors,
                             const XpOptGroup* groups_host, int32_t n_groups, const float* norm_partials,
                             int32_t n_norm_partials, float max_norm, float* grad_norm_out, void* stream) {
  return launch_optim<false>("xp_optim_step", kind, {table, chunk_map, n_chunks, grads_host, group_of_host, n_tensors, groups_host,
                                                     n_groups, norm_partials, n_norm_partials, max_norm, grad_norm_out, nullptr, stream});
}

extern "C" int xp_step_verdict(const float* partials, int32_t n_partials, XpStepVerdict* verdict, void* stream) {
  XP_REQUIRE(partials && verdict, "xp_step_verdict: null argument");
  XP_REQUIRE(n_partials > 0, "xp_step_verdict: n_partials=%d must be positive", n_partials);
  XP_REQUIRE_ALIGNED("xp_step_verdict", 16, XP_P(partials), XP_P(verdict));
  verdict_kernel<<<1, NT, 0, (hipStream_t)stream>>>(partials, n_partials, verdict);
  XP_CHECK_LAUNCH("xp_step_verdict");
  return XP_OK;
}

extern "C" int xp_adamw_step_guarded(const XpAdamTensor* table, const int32_t* chunk_map, int32_t n_chunks,
                                     const void* const* grads_host, const uint8_t* group_of_host, int32_t n_tensors,
                                     const XpAdamGroup* groups_host, int32_t n_groups, const float* norm_partials,
                                     int32_t n_norm_partials, float max_norm, float* grad_norm_out,
                                     const XpStepVerdict* verdict, void* stream) {
  return launch_update<KIND_ADAMW, true, XpAdamGroup>(
      "xp_adamw_step_guarded", {table, chunk_map, n_chunks, grads_host, group_of_host, n_tensors, groups_host, n_groups, norm_partials,
                                n_norm_partials, max_norm, grad_norm_out, verdict, stream});
}

extern "C" int xp_optim_step_guarded(int32_t kind, const XpAdamTensor* table, const int32_t* chunk_map, int32_t n_chunks,
                                     const void* const* grads_host, const uint8_t* group_of_host, int32_t n_tensors,
                                     const XpOptGroup* groups_host, int32_t n_groups, const float* norm_partials,
                                     int32_t n_norm_partials, float max_norm, float* grad_norm_out,
                                     const XpStepVerdict* verdict, void* stream) {
  return launch_optim<true>("xp_optim_step_guarded", kind, {table, chunk_map, n_chunks, grads_host, group_of_host, n_tensors, groups_host,
                                                            n_groups, norm_partials, n_norm_partials, max_norm, grad_norm_out, verdict,
                                                            stream});
}
