// The learnable-temperature contrastive losses of optimization/loss.py, forward AND gradient in one call, fp32 throughout
// (xp_contrastive_loss; include/xpretrain_hip.h gives the maths of every kind).  The simplest, NCELearnableTempLoss (:134-141):
//   A = exp(ls) * V T^T                     [n,n]   (V, T: gathered unit-norm features [n,d])
//   loss = mean_i(lse_j A_ij - A_ii) + mean_j(lse_i A_ij - A_jj)
//   G = dloss/dA = (softmax_rows(A) + softmax_cols(A) - 2 I) / n
//   dV = exp(ls) G T ;  dT = exp(ls) G^T V ;  d ls = sum(G * A)
// n = world_size * local_batch is small (64 at 8 GPUs x 8 pairs), so this is latency- not FLOP-bound:
// plain fp32 FMA tiles (bit-stable, no bf16 rounding on the logits that are multiplied by ~100), one wave per row / column
// for the statistics, a fixed reduction order and no atomics anywhere.
// The logits and the feature gradients are products of small_gemm.hip; the four fixed-temperature losses of the same reference
// file (:13-124; xp_pair_loss) have a file of their own, in the same style.
#include "common.h"

namespace {

__global__ void finish_kernel(const float* __restrict__ part, float* loss, float* d_ls, int n) {
  const int lane = threadIdx.x;
  float a = 0.f, b = 0.f;
  for (int i = lane; i < n; i += 64) { a += part[2 * i]; b += part[2 * i + 1]; }
  a = wave_sum(a); b = wave_sum(b);
  if (lane == 0) { *loss = a; *d_ls = b; }
}

// ---- the cross-entropy family over up to three [n,n] logit matrices -------------------------------------------------------
//   S1 = s V T^T (video-subtitle), S2 = s V C^T (video-caption, HAS2), S3 = s I C^T (frame-caption, HAS3), s = exp(ls)
//   c*_j = lse over column j of S*;  r3_i = lse over row i of S3;
//   plain:   ra_i = lse over row i of S1, rb_i = lse over row i of S2                       (loss.py:134-141, :212-254)
//   merged:  ra_i = lse(S1[i,:] U S2[i,j!=i])   (loss.py:280/:311 [pos, neg, neg_2] with pos = S1_ii)
//            rb_i = lse(S1[i,j!=i] U S2[i,:])   (loss.py:281/:312 with pos = S2_ii)
//            The lse kernel has two forms of it (MERGE): 1 takes ONE maximum over the whole rows of S1 and S2 -- the form
//            XP_LOSS_VSC_FC has always had, kept bit for bit; 2 reduces the shared negatives alone and folds each positive
//            in at the end, so that an empty negative set (n = 1) gives ra_i = S1_ii exactly and a gradient of exact zero,
//            where form 1 leaves the rounding of max(S1_ii, S2_ii) + log(.) behind (1e-4 on d vis at s = 100).
//   loss = mean_i [ (c1_i - S1_ii) + (c2_i - S2_ii) + (ra_i - S1_ii) + (rb_i - S2_ii) + (c3_i - S3_ii) + (r3_i - S3_ii) ]
//   (the terms of a matrix that is not there drop out).  <0,0,0> is NCELearnableTempLoss, <1,1,1> NCELearnableTempLoss_vsc_fc.
// statistics st: the row vectors ra, (rb), (r3), then the column vectors c1, (c2), (c3), n floats each
template <bool HAS2, bool HAS3>
struct FamStats {
  static constexpr int NM = 1 + (HAS2 ? 1 : 0) + (HAS3 ? 1 : 0);          // matrices; 2 NM statistic vectors
  template <typename P> __device__ static P ra(P st, int n) { return st; }
  template <typename P> __device__ static P rb(P st, int n) { return st + n; }
  template <typename P> __device__ static P r3(P st, int n) { return st + (NM - 1) * n; }
  template <typename P> __device__ static P c1(P st, int n) { return st + NM * n; }
  template <typename P> __device__ static P c2(P st, int n) { return st + (NM + 1) * n; }
  template <typename P> __device__ static P c3(P st, int n) { return st + (2 * NM - 1) * n; }
};

// blocks 0..n-1: row i -> ra, rb, r3 ; blocks n..2n-1: column j -> c1, c2, c3   (one wave each)
template <int MERGE, bool HAS2, bool HAS3>
__global__ void fam_lse_kernel(const float* __restrict__ S1, const float* __restrict__ S2, const float* __restrict__ S3,
                               float* __restrict__ st, int n) {
  static_assert(HAS2 || (MERGE == 0 && !HAS3), "merged negatives and the third matrix come with the second");
  using F = FamStats<HAS2, HAS3>;
  const int lane = threadIdx.x;
  float* ra = F::ra(st, n); float* rb = F::rb(st, n); float* r3 = F::r3(st, n);
  float* c1 = F::c1(st, n); float* c2 = F::c2(st, n); float* c3 = F::c3(st, n);
  if ((int)blockIdx.x < n) {
    const int i = blockIdx.x;
    const float* a = S1 + (int64_t)i * n; const float* b = S2 + (int64_t)i * n; const float* c = S3 + (int64_t)i * n;
    if constexpr (MERGE == 2) {
      float mo = -INFINITY, m3 = -INFINITY;                                 // the shared negatives: S1[i,j!=i] U S2[i,j!=i]
      for (int j = lane; j < n; j += 64) {
        if (j != i) mo = fmaxf(mo, fmaxf(a[j], b[j]));
        if constexpr (HAS3) m3 = fmaxf(m3, c[j]);
      }
      mo = wave_max(mo); if constexpr (HAS3) m3 = wave_max(m3);
      float so = 0.f, s3 = 0.f;
      for (int j = lane; j < n; j += 64) {
        if (j != i) so += expf(a[j] - mo) + expf(b[j] - mo);
        if constexpr (HAS3) s3 += expf(c[j] - m3);
      }
      so = wave_sum(so); if constexpr (HAS3) s3 = wave_sum(s3);
      if (lane == 0) {
        const float pa = a[i], pb = b[i], ma = fmaxf(mo, pa), mb = fmaxf(mo, pb);
        ra[i] = ma + logf(expf(pa - ma) + so * expf(mo - ma));              // n = 1: so = 0, exp(-inf) = 0 -> ra = pa exactly
        rb[i] = mb + logf(expf(pb - mb) + so * expf(mo - mb));
        if constexpr (HAS3) r3[i] = m3 + logf(s3);
      }
    } else if constexpr (MERGE == 1) {
      float mab = -INFINITY, m3 = -INFINITY;
      for (int j = lane; j < n; j += 64) { mab = fmaxf(mab, fmaxf(a[j], b[j])); if constexpr (HAS3) m3 = fmaxf(m3, c[j]); }
      mab = wave_max(mab); if constexpr (HAS3) m3 = wave_max(m3);
      float sa = 0.f, sb = 0.f, s3 = 0.f;
      for (int j = lane; j < n; j += 64) {
        const float ea = expf(a[j] - mab), eb = expf(b[j] - mab);
        sa += ea + (j == i ? 0.f : eb);
        sb += (j == i ? 0.f : ea) + eb;
        if constexpr (HAS3) s3 += expf(c[j] - m3);
      }
      sa = wave_sum(sa); sb = wave_sum(sb); if constexpr (HAS3) s3 = wave_sum(s3);
      if (lane == 0) { ra[i] = mab + logf(sa); rb[i] = mab + logf(sb); if constexpr (HAS3) r3[i] = m3 + logf(s3); }
    } else {
      float m1 = -INFINITY, m2 = -INFINITY, m3 = -INFINITY;
      for (int j = lane; j < n; j += 64) {
        m1 = fmaxf(m1, a[j]); if constexpr (HAS2) m2 = fmaxf(m2, b[j]); if constexpr (HAS3) m3 = fmaxf(m3, c[j]);
      }
      m1 = wave_max(m1); if constexpr (HAS2) m2 = wave_max(m2); if constexpr (HAS3) m3 = wave_max(m3);
      float s1 = 0.f, s2 = 0.f, s3 = 0.f;
      for (int j = lane; j < n; j += 64) {
        s1 += expf(a[j] - m1); if constexpr (HAS2) s2 += expf(b[j] - m2); if constexpr (HAS3) s3 += expf(c[j] - m3);
      }
      s1 = wave_sum(s1); if constexpr (HAS2) s2 = wave_sum(s2); if constexpr (HAS3) s3 = wave_sum(s3);
      if (lane == 0) {
        ra[i] = m1 + logf(s1); if constexpr (HAS2) rb[i] = m2 + logf(s2); if constexpr (HAS3) r3[i] = m3 + logf(s3);
      }
    }
  } else {
    const int j = blockIdx.x - n;
    float m1 = -INFINITY, m2 = -INFINITY, m3 = -INFINITY;
    for (int i = lane; i < n; i += 64) {
      m1 = fmaxf(m1, S1[(int64_t)i * n + j]);
      if constexpr (HAS2) m2 = fmaxf(m2, S2[(int64_t)i * n + j]);
      if constexpr (HAS3) m3 = fmaxf(m3, S3[(int64_t)i * n + j]);
    }
    m1 = wave_max(m1); if constexpr (HAS2) m2 = wave_max(m2); if constexpr (HAS3) m3 = wave_max(m3);
    float s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (int i = lane; i < n; i += 64) {
      s1 += expf(S1[(int64_t)i * n + j] - m1);
      if constexpr (HAS2) s2 += expf(S2[(int64_t)i * n + j] - m2);
      if constexpr (HAS3) s3 += expf(S3[(int64_t)i * n + j] - m3);
    }
    s1 = wave_sum(s1); if constexpr (HAS2) s2 = wave_sum(s2); if constexpr (HAS3) s3 = wave_sum(s3);
    if (lane == 0) {
      c1[j] = m1 + logf(s1); if constexpr (HAS2) c2[j] = m2 + logf(s2); if constexpr (HAS3) c3[j] = m3 + logf(s3);
    }
  }
}

// block i: rows i of G1, G2, G3 (d loss / d S*) ; part[i] = (loss_i, dls_i)
template <bool MERGED, bool HAS2, bool HAS3>
__global__ void fam_grad_kernel(const float* __restrict__ S1, const float* __restrict__ S2, const float* __restrict__ S3,
                                const float* __restrict__ st, float* __restrict__ G1, float* __restrict__ G2,
                                float* __restrict__ G3, float* __restrict__ part, int n) {
  using F = FamStats<HAS2, HAS3>;
  const int lane = threadIdx.x, i = blockIdx.x;
  const float* c1 = F::c1(st, n); const float* c2 = F::c2(st, n); const float* c3 = F::c3(st, n);
  const float inv = 1.0f / (float)n, rai = F::ra(st, n)[i];
  float rbi = 0.f, r3i = 0.f;
  if constexpr (HAS2) rbi = F::rb(st, n)[i];
  if constexpr (HAS3) r3i = F::r3(st, n)[i];
  float dls = 0.f;
  for (int j = lane; j < n; j += 64) {
    const int64_t o = (int64_t)i * n + j;
    const bool dg = i == j;
    const float a = S1[o];
    float g1;
    if constexpr (MERGED) g1 = (expf(a - c1[j]) + expf(a - rai) + (dg ? -2.0f : expf(a - rbi))) * inv;
    else g1 = (expf(a - c1[j]) + expf(a - rai) - (dg ? 2.0f : 0.0f)) * inv;
    G1[o] = g1;
    if constexpr (HAS2) {
      const float b = S2[o];
      float g2;
      if constexpr (MERGED) g2 = (expf(b - c2[j]) + expf(b - rbi) + (dg ? -2.0f : expf(b - rai))) * inv;
      else g2 = (expf(b - c2[j]) + expf(b - rbi) - (dg ? 2.0f : 0.0f)) * inv;
      G2[o] = g2;
      if constexpr (HAS3) {
        const float c = S3[o];
        const float g3 = (expf(c - c3[j]) + expf(c - r3i) - (dg ? 2.0f : 0.0f)) * inv;
        G3[o] = g3;
        dls += g1 * a + g2 * b + g3 * c;
      } else {
        dls += g1 * a + g2 * b;
      }
    } else {
      dls += g1 * a;
    }
  }
  dls = wave_sum(dls);
  if (lane == 0) {
    const int64_t d = (int64_t)i * n + i;
    float l;
    if constexpr (HAS2 && HAS3)
      l = (c1[i] - S1[d]) + (c2[i] - S2[d]) + (rai - S1[d]) + (rbi - S2[d]) + (c3[i] - S3[d]) + (r3i - S3[d]);
    else if constexpr (HAS2)
      l = (c1[i] - S1[d]) + (c2[i] - S2[d]) + (rai - S1[d]) + (rbi - S2[d]);
    else
      l = (c1[i] - S1[d]) + (rai - S1[d]);
    part[2 * i] = l * inv;
    part[2 * i + 1] = dls;
  }
}

// ---- NCELearnableTempDSLLoss (optimization/loss.py:193-202): a softmax prior INSIDE the cross-entropy, not detached -----
//   A = s V T^T ; Pc = softmax over i of A (per column), Pr = softmax over j of A (per row) ; B1 = A o Pc, B2 = A o Pr
//   loss = mean_i [ lse_j B1_ij - B1_ii ] + mean_j [ lse_i B2_ij - B2_jj ]
//   G1 = (softmax_rows(B1) - I) / n ; G2 = (softmax_cols(B2) - I) / n ; u_j = sum_k G1_kj B1_kj ; w_i = sum_k G2_ik B2_ik
//   G = dloss/dA = Pc o (G1 o (1 + A) - u_j) + Pr o (G2 o (1 + A) - w_i)        (the -u, -w terms: the softmax Jacobians)
// Three reduction rounds: lse of A (fam_lse_kernel<0, false, false>: lr = ra, lc = c1), then the two kernels below, then the gradient.
// statistics st: lr, lc, R1 (row lse of B1), C2 (column lse of B2), u, w -- n floats each.
// blocks 0..n-1: row i of B1 and R1[i] ; blocks n..2n-1: column j of B2 and C2[j]   (one wave each)
__global__ void dsl_prior_kernel(const float* __restrict__ A, float* __restrict__ st, float* __restrict__ B1,
                                 float* __restrict__ B2, int n) {
  const int lane = threadIdx.x;
  const bool col = (int)blockIdx.x >= n;
  const int idx = col ? blockIdx.x - n : blockIdx.x;
  const float* other = col ? st : st + n;                       // column j scales by Pr (lr_i), row i by Pc (lc_j)
  float* B = col ? B2 : B1;
  const int64_t step = col ? n : 1, base = col ? idx : (int64_t)idx * n;
  float m = -INFINITY;
  for (int t = lane; t < n; t += 64) {
    const float a = A[base + t * step];
    const float b = a * expf(a - other[t]);
    B[base + t * step] = b;
    m = fmaxf(m, b);
  }
  m = wave_max(m);
  float s = 0.f;
  for (int t = lane; t < n; t += 64) s += expf(B[base + t * step] - m);          // each lane re-reads what it wrote itself
  s = wave_sum(s);
  if (lane == 0) st[(col ? 3 : 2) * (int64_t)n + idx] = m + logf(s);
}

// blocks 0..n-1: row i -> w_i = sum_k G2_ik B2_ik ; blocks n..2n-1: column j -> u_j = sum_k G1_kj B1_kj   (one wave each)
__global__ void dsl_jacobian_kernel(const float* __restrict__ B1, const float* __restrict__ B2, float* __restrict__ st, int n) {
  const int lane = threadIdx.x;
  const bool col = (int)blockIdx.x >= n;
  const int idx = col ? blockIdx.x - n : blockIdx.x;
  const float* B = col ? B1 : B2;
  const float* lse = col ? st + 2 * (int64_t)n : st + 3 * (int64_t)n;       // G1_kj needs R1[k], G2_ik needs C2[k]
  const int64_t step = col ? n : 1, base = col ? idx : (int64_t)idx * n;
  const float inv = 1.0f / (float)n;
  float s = 0.f;
  for (int t = lane; t < n; t += 64) {
    const float b = B[base + t * step];
    const float g = (expf(b - lse[t]) - (t == idx ? 1.0f : 0.0f)) * inv;
    s += g * b;
  }
  s = wave_sum(s);
  if (lane == 0) st[(col ? 4 : 5) * (int64_t)n + idx] = s;
}

// block i: row i of G ; part[i] = (loss_i, dls_i)
__global__ void dsl_grad_kernel(const float* __restrict__ A, const float* __restrict__ B1, const float* __restrict__ B2,
                                const float* __restrict__ st, float* __restrict__ G, float* __restrict__ part, int n) {
  const int lane = threadIdx.x, i = blockIdx.x;
  const float* lc = st + n; const float* C2 = st + 3 * (int64_t)n; const float* u = st + 4 * (int64_t)n;
  const float inv = 1.0f / (float)n, lri = st[i], R1i = st[2 * (int64_t)n + i], wi = st[5 * (int64_t)n + i];
  float dls = 0.f;
  for (int j = lane; j < n; j += 64) {
    const int64_t o = (int64_t)i * n + j;
    const float a = A[o], dgl = i == j ? 1.0f : 0.0f;
    const float g1 = (expf(B1[o] - R1i) - dgl) * inv, g2 = (expf(B2[o] - C2[j]) - dgl) * inv;
    const float g = expf(a - lc[j]) * (g1 * (1.0f + a) - u[j]) + expf(a - lri) * (g2 * (1.0f + a) - wi);
    G[o] = g;
    dls += g * a;
  }
  dls = wave_sum(dls);
  if (lane == 0) {
    const int64_t d = (int64_t)i * n + i;
    part[2 * i] = ((R1i - B1[d]) + (C2[i] - B2[d])) * inv;
    part[2 * i + 1] = dls;
  }
}

// out[na + nb, d] = [a ; b]  (VidImgNCELearnableTempLoss concatenates its operands, loss.py:152-153)
__global__ void concat_rows_kernel(const float* __restrict__ a, int64_t na, const float* __restrict__ b, int64_t nb,
                                   float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < na) out[e] = a[e];
  else if (e < na + nb) out[e] = b[e - na];
}

// ---- the loss family: one path, described per kind -------------------------------------------------------------------------
struct LossKindDesc {
  const char* name;
  int merge;                    // fam_lse_kernel's MERGE: 0 plain rows, 1 / 2 merged negatives (the vsc_fc form / exact at n = 1)
  bool has2, has3;              // S2 = V C^T, S3 = I C^T
  bool dsl, concat, divide;     // DSL prior ; NCE over [V;I], [T;C] ; NCE(V,T) + NCE(I,C)
  bool reads_img, reads_cap;
};
const LossKindDesc kLossKinds[] = {
    /* XP_LOSS_NCE           */ {"nce", 0, false, false, false, false, false, false, false},
    /* XP_LOSS_VSC_FC        */ {"vsc_fc", 1, true, true, false, false, false, true, true},
    /* XP_LOSS_DSL           */ {"dsl", 0, false, false, true, false, false, false, false},
    /* XP_LOSS_VS_VC         */ {"vs_vc", 0, true, false, false, false, false, false, true},
    /* XP_LOSS_VS_VC_FC      */ {"vs_vc_fc", 0, true, true, false, false, false, true, true},
    /* XP_LOSS_VSC           */ {"vsc", 2, true, false, false, false, false, false, true},
    /* XP_LOSS_VIDIMG        */ {"vidimg", 0, false, false, false, true, false, true, true},
    /* XP_LOSS_VIDIMG_DIVIDE */ {"vidimg_divide", 0, false, false, false, false, true, true, true},
};
constexpr int kNumLossKinds = (int)(sizeof(kLossKinds) / sizeof(kLossKinds[0]));

const char* const kWho = "xp_contrastive_loss";                 // names the entry in launch errors

// The workspace of one call, as float offsets: xp_contrastive_loss_workspace_bytes reports `bytes`, every launch points into these.
// A pass over `rows` rows holds its [rows, rows] matrices S* (dsl: A, B1, B2), their gradients G* and its statistic vectors.
struct PassPlan { size_t S, G, stats; };
struct LossPlan {
  size_t X, Y;                  // concat: [V;I], [T;C], (n + m) x d each
  PassPlan first, second;       // second: divide's pass over (img, cap) at m rows
  size_t part;                  // part[2 * parts]: (loss_i, dls_i) per row of every pass, in pass order
  int64_t parts;
  size_t bytes;
};

LossPlan loss_plan(const LossKindDesc& k, int64_t n, int64_t m, int64_t d) {
  LossPlan p = {};
  size_t at = 0;
  auto take = [&at](int64_t floats) { const size_t o = at; at += (size_t)floats; return o; };
  auto pass = [&take](int64_t rows, int mats, int grads, int vectors) {
    return PassPlan{take(mats * rows * rows), take(grads * rows * rows), take(vectors * rows)};
  };
  const int nm = 1 + k.has2 + k.has3;
  p.parts = k.concat || k.divide ? n + m : n;
  if (k.concat) { p.X = take(p.parts * d); p.Y = take(p.parts * d); }
  if (k.dsl) p.first = pass(n, 3, 1, 6);                                   // A, B1, B2 ; G ; lr, lc, R1, C2, u, w
  else if (k.concat) p.first = pass(n + m, 1, 1, 2);                       // NCE at n + m rows
  else p.first = pass(n, nm, nm, 2 * nm);                                  // NCE: 2n^2 + 2n ; vsc_fc: 6n^2 + 6n
  if (k.divide) p.second = pass(m, 1, 1, 2);
  p.part = take(2 * p.parts);
  p.bytes = at * sizeof(float);
  return p;
}

// the matrices of a pass over 1 + has2 + has3 logit matrices of n rows (nullptr for one that is not there)
struct FamMats { float *S1, *S2, *S3, *G1, *G2, *G3, *stats; };
FamMats fam_mats(float* ws, const PassPlan& q, int64_t n, bool has2, bool has3) {
  float* S = ws + q.S; float* G = ws + q.G;
  return {S, has2 ? S + n * n : nullptr, has3 ? S + 2 * n * n : nullptr, G, has2 ? G + n * n : nullptr, has3 ? G + 2 * n * n : nullptr,
          ws + q.stats};
}

// The front of a pass over nm = 1 + HAS2 + HAS3 logit matrices of n rows: logits, statistics, G*, part[2n].
// (X, Y, Y2, X3) = (vis, txt, cap, img).
template <int MERGE, bool HAS2, bool HAS3>
int fam_front(const float* X, const float* Y, const float* Y2, const float* X3, const float* log_scale, int64_t n, int64_t d,
              const FamMats& w, float* part, hipStream_t st) {
  const int N = (int)n;
  xp_launch_logits(X, Y, w.S1, n, d, log_scale, st);
  if (HAS2) xp_launch_logits(X, Y2, w.S2, n, d, log_scale, st);
  if (HAS3) xp_launch_logits(X3, Y2, w.S3, n, d, log_scale, st);
  XP_CHECK_LAUNCH(kWho);
  fam_lse_kernel<MERGE, HAS2, HAS3><<<(unsigned)(2 * n), 64, 0, st>>>(w.S1, w.S2, w.S3, w.stats, N);
  XP_CHECK_LAUNCH(kWho);
  fam_grad_kernel<(MERGE != 0), HAS2, HAS3><<<(unsigned)n, 64, 0, st>>>(w.S1, w.S2, w.S3, w.stats, w.G1, w.G2, w.G3, part, N);
  XP_CHECK_LAUNCH(kWho);
  return XP_OK;
}

// The whole pass: the front, then the feature gradients
//   dX = s (G1 Y + G2 Y2) ; dY = s G1^T X ; dY2 = s (G2^T X + G3^T X3) ; dX3 = s G3 Y2
template <int MERGE, bool HAS2, bool HAS3>
int fam_pass(const float* X, const float* Y, const float* Y2, const float* X3, const float* log_scale, float* dX, float* dY,
             float* dY2, float* dX3, int64_t n, int64_t d, float* ws, const PassPlan& q, float* part, hipStream_t st) {
  const FamMats w = fam_mats(ws, q, n, HAS2, HAS3);
  const int rc = fam_front<MERGE, HAS2, HAS3>(X, Y, Y2, X3, log_scale, n, d, w, part, st);
  if (rc != XP_OK) return rc;
  const int N = (int)n, D = (int)d;
  xp_launch_small_gemm(w.G1, n, 1, Y, d, 1, dX, d, N, D, N, log_scale, 0, st);
  if (HAS2) xp_launch_small_gemm(w.G2, n, 1, Y2, d, 1, dX, d, N, D, N, log_scale, 1, st);
  xp_launch_small_gemm(w.G1, 1, n, X, d, 1, dY, d, N, D, N, log_scale, 0, st);
  if (HAS2) xp_launch_small_gemm(w.G2, 1, n, X, d, 1, dY2, d, N, D, N, log_scale, 0, st);
  if (HAS3) xp_launch_small_gemm(w.G3, 1, n, X3, d, 1, dY2, d, N, D, N, log_scale, 1, st);
  if (HAS3) xp_launch_small_gemm(w.G3, n, 1, Y2, d, 1, dX3, d, N, D, N, log_scale, 0, st);
  XP_CHECK_LAUNCH(kWho);
  return XP_OK;
}

int dsl_pass(const float* vis, const float* txt, const float* log_scale, float* d_vis, float* d_txt, int64_t n, int64_t d,
             float* ws, const PassPlan& q, float* part, hipStream_t st) {
  float* A = ws + q.S; float* B1 = A + n * n; float* B2 = B1 + n * n; float* G = ws + q.G; float* stats = ws + q.stats;
  const int N = (int)n, D = (int)d;
  xp_launch_logits(vis, txt, A, n, d, log_scale, st);
  XP_CHECK_LAUNCH(kWho);
  fam_lse_kernel<0, false, false><<<(unsigned)(2 * n), 64, 0, st>>>(A, nullptr, nullptr, stats, N);   // lr, lc
  XP_CHECK_LAUNCH(kWho);
  dsl_prior_kernel<<<(unsigned)(2 * n), 64, 0, st>>>(A, stats, B1, B2, N);                                // B1, B2, R1, C2
  XP_CHECK_LAUNCH(kWho);
  dsl_jacobian_kernel<<<(unsigned)(2 * n), 64, 0, st>>>(B1, B2, stats, N);                                // u, w
  XP_CHECK_LAUNCH(kWho);
  dsl_grad_kernel<<<(unsigned)n, 64, 0, st>>>(A, B1, B2, stats, G, part, N);
  XP_CHECK_LAUNCH(kWho);
  xp_launch_small_gemm(G, n, 1, txt, d, 1, d_vis, d, N, D, N, log_scale, 0, st);
  xp_launch_small_gemm(G, 1, n, vis, d, 1, d_txt, d, N, D, N, log_scale, 0, st);
  XP_CHECK_LAUNCH(kWho);
  return XP_OK;
}

}  // namespace

extern "C" size_t xp_contrastive_loss_workspace_bytes(int32_t kind, int64_t n, int64_t m, int64_t d) {
  if (kind < 0 || kind >= kNumLossKinds || n <= 0 || m <= 0 || d <= 0) return 0;
  return loss_plan(kLossKinds[kind], n, m, d).bytes;
}

extern "C" int xp_contrastive_loss_operands(int32_t kind, int32_t* reads_img, int32_t* reads_cap) {
  XP_REQUIRE(kind >= 0 && kind < kNumLossKinds, "xp_contrastive_loss: unknown kind %d", (int)kind);
  XP_REQUIRE(reads_img && reads_cap, "xp_contrastive_loss_operands: null pointer");
  *reads_img = kLossKinds[kind].reads_img;
  *reads_cap = kLossKinds[kind].reads_cap;
  return XP_OK;
}

extern "C" int xp_contrastive_loss(int32_t kind, const float* vis, const float* txt, const float* img, const float* cap,
                                   const float* log_scale, float* loss, float* d_vis, float* d_txt, float* d_img, float* d_cap,
                                   float* d_log_scale, int64_t n, int64_t m, int64_t d,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  XP_REQUIRE(kind >= 0 && kind < kNumLossKinds, "xp_contrastive_loss: unknown kind %d", (int)kind);
  const LossKindDesc& k = kLossKinds[kind];
  XP_REQUIRE(vis && txt && log_scale && loss && d_vis && d_txt && d_log_scale, "xp_contrastive_loss(%s): null pointer", k.name);
  XP_REQUIRE((!k.reads_img || (img && d_img)) && (!k.reads_cap || (cap && d_cap)),
             "xp_contrastive_loss(%s): null pointer (this kind reads %s)", k.name, k.reads_img ? "img and cap" : "cap");
  XP_REQUIRE_ALIGNED("xp_contrastive_loss", 16, XP_P(vis), XP_P(txt), XP_P(img), XP_P(cap), XP_P(log_scale), XP_P(loss), XP_P(d_vis), XP_P(d_txt),
                     XP_P(d_img), XP_P(d_cap), XP_P(d_log_scale), XP_P(workspace));
  XP_REQUIRE(n > 0 && m > 0 && d > 0 && (k.concat ? n + m : (n > m ? n : m)) <= 16384,
             "xp_contrastive_loss(%s): bad sizes n=%lld m=%lld d=%lld", k.name, (long long)n, (long long)m, (long long)d);
  XP_REQUIRE(m == n || k.concat || k.divide, "xp_contrastive_loss(%s): this kind needs m == n, got n=%lld m=%lld", k.name,
             (long long)n, (long long)m);
  const LossPlan p = loss_plan(k, n, m, d);
  XP_REQUIRE(workspace && workspace_bytes >= p.bytes, "xp_contrastive_loss(%s): workspace too small", k.name);
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)workspace;
  float* part = ws + p.part;
  int rc;
  if (k.dsl) {
    rc = dsl_pass(vis, txt, log_scale, d_vis, d_txt, n, d, ws, p.first, part, st);
  } else if (k.concat) {
    // [V;I] against [T;C]: one NCE front at n + m rows; the gradients are row ranges of G times the concatenated operands
    const int64_t N = n + m;
    float* X = ws + p.X; float* Y = ws + p.Y;
    const unsigned gc = (unsigned)cdiv(N * d, 256);
    concat_rows_kernel<<<gc, 256, 0, st>>>(vis, n * d, img, m * d, X);
    concat_rows_kernel<<<gc, 256, 0, st>>>(txt, n * d, cap, m * d, Y);
    XP_CHECK_LAUNCH(kWho);
    const FamMats w = fam_mats(ws, p.first, N, false, false);
    rc = fam_front<0, false, false>(X, Y, nullptr, nullptr, log_scale, N, d, w, part, st);
    if (rc != XP_OK) return rc;
    const float* G = w.G1;
    const int D = (int)d;
    xp_launch_small_gemm(G, N, 1, Y, d, 1, d_vis, d, (int)n, D, (int)N, log_scale, 0, st);             // rows 0..n-1
    xp_launch_small_gemm(G + n * N, N, 1, Y, d, 1, d_img, d, (int)m, D, (int)N, log_scale, 0, st);     // rows n..
    xp_launch_small_gemm(G, 1, N, X, d, 1, d_txt, d, (int)n, D, (int)N, log_scale, 0, st);             // columns 0..n-1
    xp_launch_small_gemm(G + n, 1, N, X, d, 1, d_cap, d, (int)m, D, (int)N, log_scale, 0, st);         // columns n..
    XP_CHECK_LAUNCH(kWho);
  } else if (k.divide) {
    rc = fam_pass<0, false, false>(vis, txt, nullptr, nullptr, log_scale, d_vis, d_txt, nullptr, nullptr, n, d, ws, p.first, part, st);
    if (rc != XP_OK) return rc;
    rc = fam_pass<0, false, false>(img, cap, nullptr, nullptr, log_scale, d_img, d_cap, nullptr, nullptr, m, d, ws, p.second,
                                   part + 2 * n, st);
  } else {
#define XP_FAM(MG, H2, H3) fam_pass<MG, H2, H3>(vis, txt, cap, img, log_scale, d_vis, d_txt, d_cap, d_img, n, d, ws, p.first, part, st)
    if (k.merge == 1) rc = XP_FAM(1, true, true);                          // vsc_fc
    else if (k.merge == 2) rc = XP_FAM(2, true, false);                    // vsc
    else if (k.has2) rc = k.has3 ? XP_FAM(0, true, true) : XP_FAM(0, true, false);
    else rc = XP_FAM(0, false, false);
#undef XP_FAM
  }
  if (rc != XP_OK) return rc;
  finish_kernel<<<1, 64, 0, st>>>(part, loss, d_log_scale, (int)p.parts);
  XP_CHECK_LAUNCH(kWho);
  return XP_OK;
}
