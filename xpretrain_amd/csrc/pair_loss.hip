// The fixed-temperature pair losses (optimization/loss.py:13-124; include/xpretrain_hip.h gives the maths of every kind), forward
// AND gradient in one call (xp_pair_loss), fp32 throughout, in the style of loss_family.hip.
//   A = V T^T [n, m], m = n * bag, UNSCALED (or order_sim); the kernels below read x = c A with c = 1 / temp or 1 as an argument
//   one wave per line: the row pass (n blocks) WRITES row i of G = d loss / d A, the column pass (n blocks, next launch) ADDS its
//   share to column j -- two launches on one stream, so every G_ij is (row share) + (column share) in that order, no atomics
//   part[0..n) row shares of the loss, part[n..2n) column shares; summed by reduce.hip's fixed tree
#include "common.h"

namespace {

struct PairArgs {
  float c, margin;              // x = c A ; the triplet margin
  int max_violation, k, bag;
};

// offset of element t of line idx: row idx of an [n, n] matrix, or its column idx
template <bool COL> __device__ __forceinline__ int64_t line_off(int idx, int t, int n) {
  return COL ? (int64_t)t * n + idx : (int64_t)idx * n + t;
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// max(x, 0) as torch.clamp(min=0) has it: a NaN stays a NaN (fmaxf would return the 0), so that a non-finite feature reaches the loss
__device__ __forceinline__ float relu_nan(float x) { return !(x <= 0.f) ? x : 0.f; }

// a > b in the order in which a NaN is the largest value, as torch.max() has it: a line that holds a NaN has it for its maximum
__device__ __forceinline__ bool gt_nan(float a, float b) { return a != a ? b == b : a > b; }

// S_ij = -|max(0, t_j - v_i)|_2 (order_sim, loss.py:13-19): one wave per (i, j), a fixed butterfly
__global__ __launch_bounds__(256) void order_sim_kernel(const float* __restrict__ V, const float* __restrict__ T,
                                                        float* __restrict__ S, int n, int d) {
  const int lane = threadIdx.x & 63;
  const int pair = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= n * n) return;
  const int i = pair / n, j = pair - i * n;
  const float* v = V + (int64_t)i * d;
  const float* t = T + (int64_t)j * d;
  float s = 0.f;
  for (int k = lane; k < d; k += 64) {
    const float r = relu_nan(t[k] - v[k]);
    s += r * r;
  }
  s = wave_sum(s);
  if (lane == 0) S[(int64_t)i * n + j] = -sqrtf(s);
}

// the order measure's backward: dS_ij/dv_i = max(0, t_j - v_i) / (-S_ij) = -dS_ij/dt_j ; a pair at distance 0 gives nothing.
// blocks 0..n-1: row i of dV = sum_j G_ij dS_ij/dv_i ; blocks n..2n-1: row j of dT = sum_i G_ij dS_ij/dt_j   (j, i ascending)
__global__ void order_bwd_kernel(const float* __restrict__ V, const float* __restrict__ T, const float* __restrict__ S,
                                 const float* __restrict__ G, float* __restrict__ dV, float* __restrict__ dT, int n, int d) {
  const bool col = (int)blockIdx.x >= n;
  const int a = col ? blockIdx.x - n : blockIdx.x;
  const float* own = (col ? T : V) + (int64_t)a * d;
  const float* other = col ? V : T;
  float* out = (col ? dT : dV) + (int64_t)a * d;
  for (int k = threadIdx.x; k < d; k += 64) {
    const float x = own[k];
    float acc = 0.f;
    for (int b = 0; b < n; ++b) {
      const int64_t o = col ? (int64_t)b * n + a : (int64_t)a * n + b;
      const float g = G[o], s = S[o];
      if (g != 0.f && s != 0.f) {                                             // (uniform over the block)
        const float y = other[(int64_t)b * d + k];
        const float r = relu_nan(col ? x - y : y - x);                        // max(0, t_j - v_i)
        acc += g * r / (col ? s : -s);
      }
    }
    out[k] = acc;
  }
}

// x = c a as ONE rounded product wherever it is formed: contracted into fma(c, a, -lse) the exponent would see the exact product and
// the lse the rounded one, and a saturated line (n = 1: lse = x) would leave c * 2^-24-sized residue where the gradient is exactly 0
__device__ __forceinline__ float scaled(float c, float a) {
#pragma clang fp contract(off)
  return c * a;
}

// NCEContrastiveLoss: line lse of x = c A ; G share = c (softmax - delta) / n ; loss share = (lse - x_diag) / n
template <bool COL>
__global__ void pair_nce_kernel(const float* __restrict__ A, float* __restrict__ G, float* __restrict__ part, int n, PairArgs p) {
  const int lane = threadIdx.x, idx = blockIdx.x;
  const float inv = 1.0f / (float)n;
  float mx = -INFINITY;
  for (int t = lane; t < n; t += 64) mx = fmaxf(mx, scaled(p.c, A[line_off<COL>(idx, t, n)]));
  mx = wave_max(mx);
  float s = 0.f;
  for (int t = lane; t < n; t += 64) s += expf(scaled(p.c, A[line_off<COL>(idx, t, n)]) - mx);
  s = wave_sum(s);
  const float lse = mx + logf(s);
  for (int t = lane; t < n; t += 64) {
    const int64_t o = line_off<COL>(idx, t, n);
    const float g = p.c * (expf(scaled(p.c, A[o]) - lse) - (t == idx ? 1.0f : 0.0f)) * inv;
    G[o] = COL ? G[o] + g : g;
  }
  if (lane == 0) part[(COL ? n : 0) + idx] = (lse - scaled(p.c, A[(int64_t)idx * n + idx])) * inv;
}

// TripletContrastiveLoss: the costs of line idx against ITS diagonal entry -- row i: cs_ij = margin + S_ij - S_ii (j != i),
// column j: ci_ij = margin + S_ij - S_jj (i != j); active where > 0 -- or NaN: the reference's clamp(min=0) and max() hand a NaN on to
// the loss, and so does this kernel (a NaN cost counts as active, and as the largest).  G share: +1 on every active entry (max_violation: on the
// largest one only, lowest index on a tie) and minus their number on the diagonal entry.
template <bool COL>
__global__ void pair_triplet_kernel(const float* __restrict__ S, float* __restrict__ G, float* __restrict__ part, int n, PairArgs p) {
  const int lane = threadIdx.x, idx = blockIdx.x;
  const int64_t dg = (int64_t)idx * n + idx;
  const float base = p.margin - S[dg];
  if (p.max_violation) {
    float best = 0.f;
    int bi = -1;
    for (int t = lane; t < n; t += 64) {
      const float cst = base + S[line_off<COL>(idx, t, n)];
      if (t != idx && gt_nan(cst, best)) { best = cst; bi = t; }              // (t ascending per lane: the first of equals stays)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      const bool same = ob == best || (ob != ob && best != best);
      if (gt_nan(ob, best) || (same && oi >= 0 && (bi < 0 || oi < bi))) { best = ob; bi = oi; }
    }
    for (int t = lane; t < n; t += 64) {
      const int64_t o = line_off<COL>(idx, t, n);
      const float g = bi < 0 ? 0.f : (t == bi ? 1.0f : (t == idx ? -1.0f : 0.f));
      G[o] = COL ? G[o] + g : g;
    }
    if (lane == 0) part[(COL ? n : 0) + idx] = best;
  } else {
    float sum = 0.f;
    int cnt = 0;
    for (int t = lane; t < n; t += 64) {
      if (t == idx) continue;                                                 // (lane 0 writes the diagonal entry below)
      const int64_t o = line_off<COL>(idx, t, n);
      const float cst = base + S[o];
      const bool act = !(cst <= 0.f);                                         // (true for a NaN)
      sum += act ? cst : 0.f;
      cnt += act;
      const float g = act ? 1.0f : 0.f;
      G[o] = COL ? G[o] + g : g;
    }
    sum = wave_sum(sum);
    cnt = wave_sum_int(cnt);
    if (lane == 0) {
      G[dg] = COL ? G[dg] - (float)cnt : -(float)cnt;
      part[(COL ? n : 0) + idx] = sum;
    }
  }
}

// order-preserving image of an fp32 key: a < b  <=>  ordered_key(a) < ordered_key(b)
__device__ __forceinline__ uint32_t ordered_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

// HardNegLoss: line idx of A with its diagonal entry lowered by 10000, held in LDS (n floats); the k-th largest key by a
// bitwise (radix-2) select on the ordered keys -- 32 counting passes over LDS, no atomics --, then everything above it and the
// lowest-index (k - above) entries equal to it.  sample = [A_diag, the selected]; loss share = (lse(sample) - A_diag) / n;
// G share = softmax(sample) / n on the selected entries and (softmax_0 - 1) / n on the diagonal entry.
// Every pass maps element t to lane t % 64, so each lane re-reads only the LDS words it wrote itself.
template <bool COL>
__global__ void pair_hardneg_kernel(const float* __restrict__ A, float* __restrict__ G, float* __restrict__ part, int n, PairArgs p) {
  extern __shared__ __attribute__((aligned(16))) float line[];
  const int lane = threadIdx.x, idx = blockIdx.x;
  const float inv = 1.0f / (float)n;
  const float dg = A[(int64_t)idx * n + idx];
  float mx = -INFINITY;
  for (int t = lane; t < n; t += 64) {
    float v = A[line_off<COL>(idx, t, n)] + 0.0f;                             // (-0 -> +0: equal floats, equal keys)
    if (t == idx) v -= 10000.0f;
    line[t] = v;
    mx = fmaxf(mx, v);
  }
  mx = wave_max(mx);
  uint32_t kth = 0;                                                           // the largest key with count(key >= it) >= k
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t cand = kth | (1u << bit);
    int cnt = 0;
    for (int t = lane; t < n; t += 64) cnt += ordered_key(line[t]) >= cand;
    if (wave_sum_int(cnt) >= p.k) kth = cand;
  }
  int above = 0;
  for (int t = lane; t < n; t += 64) above += ordered_key(line[t]) > kth;
  const int need = p.k - wave_sum_int(above);                                 // how many of the entries equal to the k-th are taken
  const float m0 = fmaxf(mx, dg);
  float s = lane == 0 ? expf(dg - m0) : 0.f;
  int eq_before = 0;
  for (int t0 = 0; t0 < n; t0 += 64) {                                        // in index order: the rank among equals is a prefix count
    const int t = t0 + lane;
    const bool valid = t < n;
    const float v = valid ? line[t] : 0.f;
    const uint32_t key = ordered_key(v);
    const bool eq = valid && key == kth;
    const unsigned long long eqs = __ballot(eq);
    const int rank = eq_before + __popcll(eqs & ((1ull << lane) - 1ull));
    const bool sel = valid && (key > kth || (eq && rank < need));
    const float e = sel ? expf(v - m0) : 0.f;
    if (valid) line[t] = e;
    s += e;
    eq_before += __popcll(eqs);
  }
  s = wave_sum(s);
  const float lse = m0 + logf(s);
  for (int t = lane; t < n; t += 64) {
    const int64_t o = line_off<COL>(idx, t, n);
    float g = line[t] / s * inv;
    if (t == idx) g += (expf(dg - lse) - 1.0f) * inv;
    G[o] = COL ? G[o] + g : g;
  }
  if (lane == 0) part[(COL ? n : 0) + idx] = (lse - dg) * inv;
}

// MILNCEContrastiveLoss, x = c A viewed as [n, n, bag] (m = n * bag columns).  Row pass, block i: nom_i = lse_b x[i,i,b],
// den_i = lse({x[i,j,b] : j != i} U {x[j,i,b] : all j}) -> den[i]; row i of G = (c / n) (j != i ? exp(x - den_i) : -exp(x - nom_i)).
__global__ void pair_milnce_row_kernel(const float* __restrict__ A, float* __restrict__ G, float* __restrict__ den,
                                       float* __restrict__ part, int n, PairArgs p) {
  const int lane = threadIdx.x, i = blockIdx.x, bag = p.bag, m = n * bag;
  const float* row = A + (int64_t)i * m;
  const float* blk = A + (int64_t)i * bag;                                    // x[j,i,b] = c blk[j * m + b]
  float mn = -INFINITY, md = -INFINITY;
  for (int t = lane; t < m; t += 64) {
    const float x = scaled(p.c, row[t]);
    if (t / bag == i) mn = fmaxf(mn, x); else md = fmaxf(md, x);
    md = fmaxf(md, scaled(p.c, blk[(int64_t)(t / bag) * m + t % bag]));
  }
  mn = wave_max(mn); md = wave_max(md);
  float sn = 0.f, sd = 0.f;
  for (int t = lane; t < m; t += 64) {
    const float x = scaled(p.c, row[t]);
    if (t / bag == i) sn += expf(x - mn); else sd += expf(x - md);
    sd += expf(scaled(p.c, blk[(int64_t)(t / bag) * m + t % bag]) - md);
  }
  sn = wave_sum(sn); sd = wave_sum(sd);
  const float nom = mn + logf(sn), dn = md + logf(sd), scale = p.c / (float)n;
  for (int t = lane; t < m; t += 64) {
    const float x = scaled(p.c, row[t]);
    G[(int64_t)i * m + t] = scaled(scale, t / bag == i ? -expf(x - nom) : expf(x - dn));
  }
  if (lane == 0) { den[i] = dn; part[i] = (dn - nom) / (float)n; }
}

// column pass, block i: G[j, i, b] += (c / n) exp(x[j,i,b] - den_i) for every j, b ; no loss share of its own
__global__ void pair_milnce_col_kernel(const float* __restrict__ A, float* __restrict__ G, const float* __restrict__ den,
                                       float* __restrict__ part, int n, PairArgs p) {
  const int lane = threadIdx.x, i = blockIdx.x, bag = p.bag, m = n * bag;
  const float dn = den[i], scale = p.c / (float)n;
  for (int t = lane; t < m; t += 64) {
    const int64_t o = (int64_t)(t / bag) * m + (int64_t)i * bag + t % bag;
    G[o] += scaled(scale, expf(scaled(p.c, A[o]) - dn));     // (rounded as the row pass rounds its share: at n = 1 the two cancel exactly)
  }
  if (lane == 0) part[n + i] = 0.f;
}

const char* const kPairKinds[] = {"nce", "triplet", "hardneg", "milnce"};
constexpr int kNumPairKinds = 4;

// what the entry refuses; nullptr when the arguments are fine
const char* pair_refusal(int32_t kind, const XpPairLossParams* p, int64_t n, int64_t d) {
  if (kind < 0 || kind >= kNumPairKinds) return "unknown kind";
  if (!p) return "null pointer";
  if (n <= 0 || d <= 0 || d > (1 << 24)) return "bad sizes";
  if (p->bag < 1 || (kind != XP_PAIR_MILNCE && p->bag != 1)) return "bag must be 1 (at least 1 for milnce)";
  if (n > 16384 || n * p->bag > 16384) return "n * bag above 16384";
  if ((kind == XP_PAIR_NCE || kind == XP_PAIR_MILNCE) && !(p->temp > 0.f)) return "temp must be > 0";
  if (kind == XP_PAIR_HARDNEG && (p->hard_negative_num < 1 || p->hard_negative_num > n)) return "hard_negative_num outside [1, n]";
  return nullptr;
}

// the workspace, as float offsets: A, G [n, n * bag] ; part[2n] ; milnce: den[n]
struct PairPlan { size_t A, G, part, den, bytes; };
PairPlan pair_plan(int32_t kind, int64_t n, int64_t bag) {
  const size_t mat = (size_t)(n * n * bag), A = 0, G = A + mat, part = G + mat, den = part + (size_t)(2 * n);
  return {A, G, part, den, (den + (size_t)(kind == XP_PAIR_MILNCE ? n : 0)) * sizeof(float)};
}

}  // namespace

extern "C" size_t xp_pair_loss_workspace_bytes(int32_t kind, const XpPairLossParams* params, int64_t n, int64_t d) {
  if (pair_refusal(kind, params, n, d)) return 0;
  return pair_plan(kind, n, params->bag).bytes;
}

extern "C" int xp_pair_loss(int32_t kind, const XpPairLossParams* params, const float* vis, const float* txt, float* loss,
                            float* d_vis, float* d_txt, int64_t n, int64_t d, void* workspace, size_t workspace_bytes, void* stream) {
  const char* why = pair_refusal(kind, params, n, d);
  const char* name = kind >= 0 && kind < kNumPairKinds ? kPairKinds[kind] : "?";
  XP_REQUIRE(!why, "xp_pair_loss(%s): %s (kind=%d n=%lld d=%lld)", name, why, (int)kind, (long long)n, (long long)d);
  XP_REQUIRE(vis && txt && loss && d_vis && d_txt, "xp_pair_loss(%s): null pointer", name);
  XP_REQUIRE_ALIGNED("xp_pair_loss", 16, XP_P(vis), XP_P(txt), XP_P(loss), XP_P(d_vis), XP_P(d_txt), XP_P(workspace));
  const int64_t bag = params->bag, m = n * bag;
  const PairPlan plan = pair_plan(kind, n, bag);
  XP_REQUIRE(workspace && workspace_bytes >= plan.bytes, "xp_pair_loss(%s): workspace too small", name);
  const char* who = "xp_pair_loss";
  hipStream_t st = (hipStream_t)stream;
  const int N = (int)n, M = (int)m, D = (int)d;
  const bool order = kind == XP_PAIR_TRIPLET && params->order_measure != 0;
  float* ws = (float*)workspace;
  float* A = ws + plan.A; float* G = ws + plan.G; float* part = ws + plan.part; float* den = ws + plan.den;
  PairArgs a;
  a.c = (kind == XP_PAIR_NCE || kind == XP_PAIR_MILNCE) ? 1.0f / params->temp : 1.0f;
  a.margin = params->margin; a.max_violation = params->max_violation != 0; a.k = params->hard_negative_num; a.bag = (int)bag;

  if (order) {
    order_sim_kernel<<<(unsigned)cdiv(n * n, 4), 256, 0, st>>>(vis, txt, A, N, D);
  } else if (m == n) {
    xp_launch_logits(vis, txt, A, n, d, nullptr, st);
  } else {
    xp_launch_small_gemm(vis, d, 1, txt, 1, d, A, m, N, M, D, nullptr, 0, st);
  }
  XP_CHECK_LAUNCH(who);
  const unsigned rows = (unsigned)n;
  switch (kind) {
    case XP_PAIR_NCE:
      pair_nce_kernel<false><<<rows, 64, 0, st>>>(A, G, part, N, a);
      pair_nce_kernel<true><<<rows, 64, 0, st>>>(A, G, part, N, a);
      break;
    case XP_PAIR_TRIPLET:
      pair_triplet_kernel<false><<<rows, 64, 0, st>>>(A, G, part, N, a);
      pair_triplet_kernel<true><<<rows, 64, 0, st>>>(A, G, part, N, a);
      break;
    case XP_PAIR_HARDNEG:
      pair_hardneg_kernel<false><<<rows, 64, (size_t)n * sizeof(float), st>>>(A, G, part, N, a);
      pair_hardneg_kernel<true><<<rows, 64, (size_t)n * sizeof(float), st>>>(A, G, part, N, a);
      break;
    default:
      pair_milnce_row_kernel<<<rows, 64, 0, st>>>(A, G, den, part, N, a);
      pair_milnce_col_kernel<<<rows, 64, 0, st>>>(A, G, den, part, N, a);
      break;
  }
  XP_CHECK_LAUNCH(who);
  xp_launch_rows_reduce(part, loss, 2 * N, 2 * N, 1, 0, st);
  XP_CHECK_LAUNCH(who);
  if (order) {
    order_bwd_kernel<<<(unsigned)(2 * n), 64, 0, st>>>(vis, txt, A, G, d_vis, d_txt, N, D);
  } else {
    xp_launch_small_gemm(G, m, 1, txt, d, 1, d_vis, d, N, D, M, nullptr, 0, st);     // dV = G T
    xp_launch_small_gemm(G, 1, m, vis, d, 1, d_txt, d, M, D, N, nullptr, 0, st);     // dT = G^T V
  }
  XP_CHECK_LAUNCH(who);
  return XP_OK;
}
