// The learnable-temperature contrastive losses of optimization/loss.py, forward AND gradient in one call, fp32 throughout
// (xp_contrastive_loss; include/xpretrain_hip.h gives the maths of every kind).  The simplest, NCELearnableTempLoss (:134-141):
//   A = exp(ls) * V T^T                     [n,n]   (V, T: gathered unit-norm features [n,d])
//   loss = mean_i(lse_j A_ij - A_ii) + mean_j(lse_i A_ij - A_jj)
//   G = dloss/dA = (softmax_rows(A) + softmax_cols(A) - 2 I) / n
//   dV = exp(ls) G T ;  dT = exp(ls) G^T V ;  d ls = sum(G * A)
// n = world_size * local_batch is small (64 at 8 GPUs x 8 pairs), so this is latency- not FLOP-bound:
// plain fp32 FMA tiles (bit-stable, no bf16 rounding on the logits that are multiplied by ~100), one wave per row / column
// for the statistics, a fixed reduction order and no atomics anywhere.
// The four fixed-temperature losses of the same file (:13-124; xp_pair_loss) follow at the end, in the same style.
#include "common.h"

namespace {

// C[i][j] = alpha * sum_k X(i,k) Y(k,j), generic strides; 32x32 tile, 256 threads, 2x2 per thread.
__global__ __launch_bounds__(256) XP_NO_PK_F32 void sgemm_strided_kernel(const float* __restrict__ X, int64_t sxi, int64_t sxk,
                                                            const float* __restrict__ Y, int64_t syk, int64_t syj,
                                                            float* __restrict__ C, int64_t ldc, int I, int J, int K,
                                                            const float* __restrict__ log_scale, int accumulate = 0) {
  __shared__ float xs[32][33], ys[32][33];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
  float acc[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
  for (int k0 = 0; k0 < K; k0 += 32) {
    for (int e = threadIdx.x; e < 1024; e += 256) {
      const int r = e >> 5, c = e & 31;
      // xs[r][c] = X(i0 + r, k0 + c) ; ys[r][c] = Y(k0 + r, j0 + c)
      xs[r][c] = (i0 + r < I && k0 + c < K) ? X[(int64_t)(i0 + r) * sxi + (int64_t)(k0 + c) * sxk] : 0.f;
      ys[r][c] = (k0 + r < K && j0 + c < J) ? Y[(int64_t)(k0 + r) * syk + (int64_t)(j0 + c) * syj] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < 32; ++k) {
      const float a0 = xs[ty][k], a1 = xs[ty + 16][k], b0 = ys[k][tx], b1 = ys[k][tx + 16];
      acc[0][0] += a0 * b0; acc[0][1] += a0 * b1; acc[1][0] += a1 * b0; acc[1][1] += a1 * b1;
    }
    __syncthreads();
  }
  const float alpha = log_scale ? expf(*log_scale) : 1.0f;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
      if (i < I && j < J) {
        float* c = C + (int64_t)i * ldc + j;
        *c = accumulate ? *c + alpha * acc[a][b] : alpha * acc[a][b];
      }
    }
}

// Small similarity matrices (n <= 128: the local batch of one to a few GPUs): C[i][j] = alpha * <X[i,:], Y[j,:]> with ONE WAVE per
// (i, j) -- 16-byte loads along d, 8 independent accumulator lanes per wave step, a fixed butterfly.  The 32x32-tile kernel above
// runs a [8 x 512] x [512 x 8] problem as one workgroup walking 16 dependent k-steps of strided loads: 39 us of load latency on the
// serial stretch between the forward and the backward (nothing else runs there); this one takes one load round trip.
__global__ __launch_bounds__(256) XP_NO_PK_F32 void logits_small_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                                        float* __restrict__ C, int n, int d,
                                                                        const float* __restrict__ log_scale) {
  const int lane = threadIdx.x & 63;
  const int pair = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= n * n) return;
  const int i = pair / n, j = pair - i * n;
  const float* x = X + (int64_t)i * d;
  const float* y = Y + (int64_t)j * d;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  for (int k = lane * 4; k < d; k += 256) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(x + k), b = *reinterpret_cast<const f32x4*>(y + k);
    s0 += a[0] * b[0]; s1 += a[1] * b[1]; s2 += a[2] * b[2]; s3 += a[3] * b[3];
  }
  float s = (s0 + s1) + (s2 + s3);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) C[(int64_t)i * n + j] = (log_scale ? expf(*log_scale) : 1.0f) * s;
}

// logits A[n][n] = e^ls V T^T: the small form up to n = 128 (d a multiple of 4, 16-byte aligned rows), the tiled form beyond
static void launch_logits(const float* vis, const float* txt, float* A, int64_t n, int64_t d, const float* log_scale, hipStream_t st) {
  if (n <= 128 && d % 4 == 0 && ((uintptr_t)vis & 15) == 0 && ((uintptr_t)txt & 15) == 0) {
    logits_small_kernel<<<(unsigned)cdiv(n * n, 4), 256, 0, st>>>(vis, txt, A, (int)n, (int)d, log_scale);
  } else {
    dim3 gnn((unsigned)cdiv(n, 32), (unsigned)cdiv(n, 32));
    sgemm_strided_kernel<<<gnn, 256, 0, st>>>(vis, d, 1, txt, 1, d, A, n, (int)n, (int)n, (int)d, log_scale);
  }
}

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
//            xp_vsc_fc_loss has always had, kept bit for bit; 2 reduces the shared negatives alone and folds each positive
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

// ---- retrieval evaluation (tasks/run_video_retrieval.py:150-171, utils/metrics.py) --------------------------------
// DSL re-rank: sim[i][j] *= softmax_i(theta * sim[i][j])   (np_softmax(sim * 100, axis=0), metrics.py:7-39); one wave per column
__global__ void dsl_rerank_kernel(float* __restrict__ sim, int n, int m, float theta, int multiply) {
  const int lane = threadIdx.x, j = blockIdx.x;
  float mx = -INFINITY;
  for (int i = lane; i < n; i += 64) mx = fmaxf(mx, sim[(int64_t)i * m + j] * theta);
  mx = wave_max(mx);
  float sum = 0.f;
  for (int i = lane; i < n; i += 64) sum += expf(sim[(int64_t)i * m + j] * theta - mx);
  sum = wave_sum(sum);
  for (int i = lane; i < n; i += 64) {
    const float x = sim[(int64_t)i * m + j];
    const float sm = expf(x * theta - mx) / sum;
    sim[(int64_t)i * m + j] = multiply ? x * sm : sm;
  }
}

// per query row i: how many entries beat / tie the labelled entry (compute_metrics: position of the label in the
// descending sort, metrics.py:41-53; ties occupy `equal` consecutive positions there).  transpose != 0 ranks columns.
__global__ void retrieval_ranks_kernel(const float* __restrict__ sim, const int64_t* __restrict__ labels, int n, int m,
                                       int transpose, int* __restrict__ greater, int* __restrict__ equal) {
  const int lane = threadIdx.x, i = blockIdx.x;
  const int cnt = transpose ? n : m;                       // candidates per query
  const int64_t qs = transpose ? 1 : m, cs = transpose ? m : 1;
  const int64_t lab = labels ? labels[i] : i;
  const float d = sim[(int64_t)i * qs + lab * cs];
  int g = 0, e = 0;
  for (int j = lane; j < cnt; j += 64) {
    const float x = sim[(int64_t)i * qs + (int64_t)j * cs];
    g += x > d; e += x == d;
  }
  g = (int)wave_sum((float)g); e = (int)wave_sum((float)e);
  if (lane == 0) { greater[i] = g; equal[i] = e; }
}

}  // namespace

extern "C" int xp_sim_matrix(const float* a, const float* b, float* sim, int64_t na, int64_t nb, int64_t d, void* stream) {
  XP_REQUIRE(a && b && sim && na > 0 && nb > 0 && d > 0, "xp_sim_matrix: bad arguments");
  dim3 g((unsigned)cdiv(nb, 32), (unsigned)cdiv(na, 32));
  sgemm_strided_kernel<<<g, 256, 0, (hipStream_t)stream>>>(a, d, 1, b, 1, d, sim, nb, (int)na, (int)nb, (int)d, nullptr);
  XP_CHECK_LAUNCH("xp_sim_matrix");
  return XP_OK;
}

extern "C" int xp_dsl_rerank(float* sim, int64_t n, int64_t m, float theta, int32_t multiply, void* stream) {
  XP_REQUIRE(sim && n > 0 && m > 0, "xp_dsl_rerank: bad arguments");
  dsl_rerank_kernel<<<(unsigned)m, 64, 0, (hipStream_t)stream>>>(sim, (int)n, (int)m, theta, multiply);
  XP_CHECK_LAUNCH("xp_dsl_rerank");
  return XP_OK;
}

extern "C" int xp_retrieval_ranks(const float* sim, const int64_t* labels, int64_t n, int64_t m, int32_t transpose,
                                  int32_t* greater, int32_t* equal, void* stream) {
  XP_REQUIRE(sim && greater && equal && n > 0 && m > 0 && n < (1 << 24) && m < (1 << 24), "xp_retrieval_ranks: bad arguments");
  XP_REQUIRE(labels || n == m || (transpose ? m <= n : n <= m), "xp_retrieval_ranks: diagonal labels need a label for every query");
  const int64_t queries = transpose ? m : n;
  retrieval_ranks_kernel<<<(unsigned)queries, 64, 0, (hipStream_t)stream>>>(sim, labels, (int)n, (int)m, transpose, greater, equal);
  XP_CHECK_LAUNCH("xp_retrieval_ranks");
  return XP_OK;
}

// ---- the loss family: one path, described per kind -------------------------------------------------------------------------
namespace {

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

// floats of one fam pass over nm [n,n] matrices: S*, G*, 2 nm statistic vectors   (part[] is counted by the caller)
size_t fam_floats(int64_t n, int nm) { return (size_t)(2 * nm * n * n + 2 * nm * n); }

size_t loss_workspace_floats(const LossKindDesc& k, int64_t n, int64_t m, int64_t d) {
  if (k.dsl) return (size_t)(4 * n * n + 6 * n + 2 * n);                           // A, B1, B2, G, 6 vectors, part[2n]
  if (k.concat) return (size_t)(2 * (n + m) * d) + fam_floats(n + m, 1) + (size_t)(2 * (n + m));   // [V;I], [T;C], NCE at n+m
  if (k.divide) return fam_floats(n, 1) + fam_floats(m, 1) + (size_t)(2 * (n + m));
  return fam_floats(n, 1 + k.has2 + k.has3) + (size_t)(2 * n);                     // NCE: 2n^2 + 4n ; vsc_fc: 6n^2 + 8n
}

// One pass over nm = 1 + HAS2 + HAS3 logit matrices of n rows: logits, statistics, G*, part[2n], and the feature gradients
//   dX = s (G1 Y + G2 Y2) ; dY = s G1^T X ; dY2 = s (G2^T X + G3^T X3) ; dX3 = s G3 Y2
// (X, Y, Y2, X3) = (vis, txt, cap, img).  ws: fam_floats(n, nm) floats.
template <int MERGE, bool HAS2, bool HAS3>
int fam_pass(const char* who, const float* X, const float* Y, const float* Y2, const float* X3, const float* log_scale,
             float* dX, float* dY, float* dY2, float* dX3, int64_t n, int64_t d, float* ws, float* part, hipStream_t st) {
  constexpr int NM = 1 + (HAS2 ? 1 : 0) + (HAS3 ? 1 : 0);
  float* S1 = ws; float* S2 = HAS2 ? S1 + n * n : nullptr; float* S3 = HAS3 ? S1 + 2 * n * n : nullptr;
  float* G1 = S1 + NM * n * n; float* G2 = HAS2 ? G1 + n * n : nullptr; float* G3 = HAS3 ? G1 + 2 * n * n : nullptr;
  float* stats = G1 + NM * n * n;
  const int N = (int)n, D = (int)d;
  dim3 gnd((unsigned)cdiv(d, 32), (unsigned)cdiv(n, 32));
  launch_logits(X, Y, S1, n, d, log_scale, st);
  if (HAS2) launch_logits(X, Y2, S2, n, d, log_scale, st);
  if (HAS3) launch_logits(X3, Y2, S3, n, d, log_scale, st);
  XP_CHECK_LAUNCH(who);
  fam_lse_kernel<MERGE, HAS2, HAS3><<<(unsigned)(2 * n), 64, 0, st>>>(S1, S2, S3, stats, N);
  XP_CHECK_LAUNCH(who);
  fam_grad_kernel<(MERGE != 0), HAS2, HAS3><<<(unsigned)n, 64, 0, st>>>(S1, S2, S3, stats, G1, G2, G3, part, N);
  XP_CHECK_LAUNCH(who);
  sgemm_strided_kernel<<<gnd, 256, 0, st>>>(G1, n, 1, Y, d, 1, dX, d, N, D, N, log_scale, 0);
  if (HAS2) sgemm_strided_kernel<<<gnd, 256, 0, st>>>(G2, n, 1, Y2, d, 1, dX, d, N, D, N, log_scale, 1);
  sgemm_strided_kernel<<<gnd, 256, 0, st>>>(G1, 1, n, X, d, 1, dY, d, N, D, N, log_scale, 0);
  if (HAS2) sgemm_strided_kernel<<<gnd, 256, 0, st>>>(G2, 1, n, X, d, 1, dY2, d, N, D, N, log_scale, 0);
  if (HAS3) sgemm_strided_kernel<<<gnd, 256, 0, st>>>(G3, 1, n, X3, d, 1, dY2, d, N, D, N, log_scale, 1);
  if (HAS3) sgemm_strided_kernel<<<gnd, 256, 0, st>>>(G3, n, 1, Y2, d, 1, dX3, d, N, D, N, log_scale, 0);
  XP_CHECK_LAUNCH(who);
  return XP_OK;
}

int dsl_pass(const char* who, const float* vis, const float* txt, const float* log_scale, float* d_vis, float* d_txt,
             int64_t n, int64_t d, float* ws, float* part, hipStream_t st) {
  float* A = ws; float* B1 = A + n * n; float* B2 = B1 + n * n; float* G = B2 + n * n; float* stats = G + n * n;
  const int N = (int)n, D = (int)d;
  dim3 gnd((unsigned)cdiv(d, 32), (unsigned)cdiv(n, 32));
  launch_logits(vis, txt, A, n, d, log_scale, st);
  XP_CHECK_LAUNCH(who);
  fam_lse_kernel<0, false, false><<<(unsigned)(2 * n), 64, 0, st>>>(A, nullptr, nullptr, stats, N);   // lr, lc
  XP_CHECK_LAUNCH(who);
  dsl_prior_kernel<<<(unsigned)(2 * n), 64, 0, st>>>(A, stats, B1, B2, N);                                // B1, B2, R1, C2
  XP_CHECK_LAUNCH(who);
  dsl_jacobian_kernel<<<(unsigned)(2 * n), 64, 0, st>>>(B1, B2, stats, N);                                // u, w
  XP_CHECK_LAUNCH(who);
  dsl_grad_kernel<<<(unsigned)n, 64, 0, st>>>(A, B1, B2, stats, G, part, N);
  XP_CHECK_LAUNCH(who);
  sgemm_strided_kernel<<<gnd, 256, 0, st>>>(G, n, 1, txt, d, 1, d_vis, d, N, D, N, log_scale, 0);
  sgemm_strided_kernel<<<gnd, 256, 0, st>>>(G, 1, n, vis, d, 1, d_txt, d, N, D, N, log_scale, 0);
  XP_CHECK_LAUNCH(who);
  return XP_OK;
}

// arguments already checked by the entry point (`who` names it in launch errors)
int contrastive_loss_run(const char* who, const LossKindDesc& k, const float* vis, const float* txt, const float* img,
                         const float* cap, const float* log_scale, float* loss, float* d_vis, float* d_txt, float* d_img,
                         float* d_cap, float* d_log_scale, int64_t n, int64_t m, int64_t d, float* ws, hipStream_t st) {
  int rc;
  int64_t parts = n;
  float* part;
  if (k.dsl) {
    part = ws + 4 * n * n + 6 * n;
    rc = dsl_pass(who, vis, txt, log_scale, d_vis, d_txt, n, d, ws, part, st);
  } else if (k.concat) {
    // [V;I] against [T;C]: one NCE at n + m rows; the gradients are row ranges of G times the concatenated operands
    const int64_t N = n + m;
    float* X = ws; float* Y = X + N * d; float* fam = Y + N * d;
    part = fam + fam_floats(N, 1);
    parts = N;
    const unsigned gc = (unsigned)cdiv(N * d, 256);
    concat_rows_kernel<<<gc, 256, 0, st>>>(vis, n * d, img, m * d, X);
    concat_rows_kernel<<<gc, 256, 0, st>>>(txt, n * d, cap, m * d, Y);
    XP_CHECK_LAUNCH(who);
    float* A = fam; float* G = A + N * N; float* stats = G + N * N;
    launch_logits(X, Y, A, N, d, log_scale, st);
    XP_CHECK_LAUNCH(who);
    fam_lse_kernel<0, false, false><<<(unsigned)(2 * N), 64, 0, st>>>(A, nullptr, nullptr, stats, (int)N);
    XP_CHECK_LAUNCH(who);
    fam_grad_kernel<false, false, false><<<(unsigned)N, 64, 0, st>>>(A, nullptr, nullptr, stats, G, nullptr, nullptr, part, (int)N);
    XP_CHECK_LAUNCH(who);
    const int D = (int)d;
    dim3 gn((unsigned)cdiv(d, 32), (unsigned)cdiv(n, 32)), gm((unsigned)cdiv(d, 32), (unsigned)cdiv(m, 32));
    sgemm_strided_kernel<<<gn, 256, 0, st>>>(G, N, 1, Y, d, 1, d_vis, d, (int)n, D, (int)N, log_scale, 0);             // rows 0..n-1
    sgemm_strided_kernel<<<gm, 256, 0, st>>>(G + n * N, N, 1, Y, d, 1, d_img, d, (int)m, D, (int)N, log_scale, 0);     // rows n..
    sgemm_strided_kernel<<<gn, 256, 0, st>>>(G, 1, N, X, d, 1, d_txt, d, (int)n, D, (int)N, log_scale, 0);             // columns 0..n-1
    sgemm_strided_kernel<<<gm, 256, 0, st>>>(G + n, 1, N, X, d, 1, d_cap, d, (int)m, D, (int)N, log_scale, 0);         // columns n..
    XP_CHECK_LAUNCH(who);
    rc = XP_OK;
  } else if (k.divide) {
    float* fam2 = ws + fam_floats(n, 1);
    part = fam2 + fam_floats(m, 1);
    parts = n + m;
    rc = fam_pass<0, false, false>(who, vis, txt, nullptr, nullptr, log_scale, d_vis, d_txt, nullptr, nullptr, n, d, ws, part, st);
    if (rc != XP_OK) return rc;
    rc = fam_pass<0, false, false>(who, img, cap, nullptr, nullptr, log_scale, d_img, d_cap, nullptr, nullptr, m, d, fam2,
                                       part + 2 * n, st);
  } else {
    part = ws + fam_floats(n, 1 + k.has2 + k.has3);
#define XP_FAM(MG, H2, H3) \
    fam_pass<MG, H2, H3>(who, vis, txt, cap, img, log_scale, d_vis, d_txt, d_cap, d_img, n, d, ws, part, st)
    if (k.merge == 1) rc = XP_FAM(1, true, true);                          // vsc_fc
    else if (k.merge == 2) rc = XP_FAM(2, true, false);                    // vsc
    else if (k.has2) rc = k.has3 ? XP_FAM(0, true, true) : XP_FAM(0, true, false);
    else rc = XP_FAM(0, false, false);
#undef XP_FAM
  }
  if (rc != XP_OK) return rc;
  finish_kernel<<<1, 64, 0, st>>>(part, loss, d_log_scale, (int)parts);
  XP_CHECK_LAUNCH(who);
  return XP_OK;
}

}  // namespace

extern "C" size_t xp_contrastive_loss_workspace_bytes(int32_t kind, int64_t n, int64_t m, int64_t d) {
  if (kind < 0 || kind >= kNumLossKinds || n <= 0 || m <= 0 || d <= 0) return 0;
  return loss_workspace_floats(kLossKinds[kind], n, m, d) * sizeof(float);
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
  XP_REQUIRE(n > 0 && m > 0 && d > 0 && (k.concat ? n + m : (n > m ? n : m)) <= 16384,
             "xp_contrastive_loss(%s): bad sizes n=%lld m=%lld d=%lld", k.name, (long long)n, (long long)m, (long long)d);
  XP_REQUIRE(m == n || k.concat || k.divide, "xp_contrastive_loss(%s): this kind needs m == n, got n=%lld m=%lld", k.name,
             (long long)n, (long long)m);
  XP_REQUIRE(workspace && workspace_bytes >= xp_contrastive_loss_workspace_bytes(kind, n, m, d),
             "xp_contrastive_loss(%s): workspace too small", k.name);
  return contrastive_loss_run("xp_contrastive_loss", k, vis, txt, img, cap, log_scale, loss, d_vis, d_txt, d_img, d_cap,
                              d_log_scale, n, m, d, (float*)workspace, (hipStream_t)stream);
}

extern "C" size_t xp_vsc_fc_loss_workspace_bytes(int64_t n, int64_t d) {
  return loss_workspace_floats(kLossKinds[XP_LOSS_VSC_FC], n, n, d) * sizeof(float);   // S1..S3, G1..G3, 6 lse vectors, part[2n]
}

extern "C" int xp_vsc_fc_loss(const float* vis, const float* txt, const float* img, const float* cap, const float* log_scale,
                              float* loss, float* d_vis, float* d_txt, float* d_img, float* d_cap, float* d_log_scale,
                              int64_t n, int64_t d, void* workspace, size_t workspace_bytes, void* stream) {
  XP_REQUIRE(vis && txt && img && cap && log_scale && loss && d_vis && d_txt && d_img && d_cap && d_log_scale,
             "xp_vsc_fc_loss: null pointer");
  XP_REQUIRE(n > 0 && d > 0 && n <= 16384, "xp_vsc_fc_loss: bad sizes n=%lld d=%lld", (long long)n, (long long)d);
  XP_REQUIRE(workspace && workspace_bytes >= xp_vsc_fc_loss_workspace_bytes(n, d), "xp_vsc_fc_loss: workspace too small");
  return contrastive_loss_run("xp_vsc_fc_loss", kLossKinds[XP_LOSS_VSC_FC], vis, txt, img, cap, log_scale, loss, d_vis, d_txt,
                              d_img, d_cap, d_log_scale, n, n, d, (float*)workspace, (hipStream_t)stream);
}

extern "C" size_t xp_nce_loss_workspace_bytes(int64_t n, int64_t d) {
  return loss_workspace_floats(kLossKinds[XP_LOSS_NCE], n, n, d) * sizeof(float);      // A, G, lse_r, lse_c, part[2n]
}

extern "C" int xp_nce_loss(const float* vis, const float* txt, const float* log_scale, float* loss,
                           float* d_vis, float* d_txt, float* d_log_scale, int64_t n, int64_t d,
                           void* workspace, size_t workspace_bytes, void* stream) {
  XP_REQUIRE(vis && txt && log_scale && loss && d_vis && d_txt && d_log_scale, "xp_nce_loss: null pointer");
  XP_REQUIRE(n > 0 && d > 0 && n <= 16384, "xp_nce_loss: bad sizes n=%lld d=%lld", (long long)n, (long long)d);
  XP_REQUIRE(workspace && workspace_bytes >= xp_nce_loss_workspace_bytes(n, d), "xp_nce_loss: workspace too small");
  return contrastive_loss_run("xp_nce_loss", kLossKinds[XP_LOSS_NCE], vis, txt, nullptr, nullptr, log_scale, loss, d_vis, d_txt,
                              nullptr, nullptr, d_log_scale, n, n, d, (float*)workspace, (hipStream_t)stream);
}

// ---- the fixed-temperature pair losses (optimization/loss.py:13-124; include/xpretrain_hip.h gives the maths of every kind) ----
//   A = V T^T [n, m], m = n * bag, UNSCALED (or order_sim); the kernels below read x = c A with c = 1 / temp or 1 as an argument
//   one wave per line: the row pass (n blocks) WRITES row i of G = d loss / d A, the column pass (n blocks, next launch) ADDS its
//   share to column j -- two launches on one stream, so every G_ij is (row share) + (column share) in that order, no atomics
//   part[0..n) row shares of the loss, part[n..2n) column shares; summed by reduce.hip's fixed tree
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

// floats: A, G [n, n * bag] ; part[2n] ; milnce: den[n]
size_t pair_workspace_floats(int32_t kind, int64_t n, int64_t bag) {
  return (size_t)(2 * n * n * bag + 2 * n + (kind == XP_PAIR_MILNCE ? n : 0));
}

}  // namespace

extern "C" size_t xp_pair_loss_workspace_bytes(int32_t kind, const XpPairLossParams* params, int64_t n, int64_t d) {
  if (pair_refusal(kind, params, n, d)) return 0;
  return pair_workspace_floats(kind, n, params->bag) * sizeof(float);
}

extern "C" int xp_pair_loss(int32_t kind, const XpPairLossParams* params, const float* vis, const float* txt, float* loss,
                            float* d_vis, float* d_txt, int64_t n, int64_t d, void* workspace, size_t workspace_bytes, void* stream) {
  const char* why = pair_refusal(kind, params, n, d);
  const char* name = kind >= 0 && kind < kNumPairKinds ? kPairKinds[kind] : "?";
  XP_REQUIRE(!why, "xp_pair_loss(%s): %s (kind=%d n=%lld d=%lld)", name, why, (int)kind, (long long)n, (long long)d);
  XP_REQUIRE(vis && txt && loss && d_vis && d_txt, "xp_pair_loss(%s): null pointer", name);
  XP_REQUIRE(workspace && workspace_bytes >= xp_pair_loss_workspace_bytes(kind, params, n, d), "xp_pair_loss(%s): workspace too small",
             name);
  const char* who = "xp_pair_loss";
  hipStream_t st = (hipStream_t)stream;
  const int64_t bag = params->bag, m = n * bag;
  const int N = (int)n, M = (int)m, D = (int)d;
  const bool order = kind == XP_PAIR_TRIPLET && params->order_measure != 0;
  float* A = (float*)workspace; float* G = A + n * m; float* part = G + n * m; float* den = part + 2 * n;
  PairArgs a;
  a.c = (kind == XP_PAIR_NCE || kind == XP_PAIR_MILNCE) ? 1.0f / params->temp : 1.0f;
  a.margin = params->margin; a.max_violation = params->max_violation != 0; a.k = params->hard_negative_num; a.bag = (int)bag;

  if (order) {
    order_sim_kernel<<<(unsigned)cdiv(n * n, 4), 256, 0, st>>>(vis, txt, A, N, D);
  } else if (m == n) {
    launch_logits(vis, txt, A, n, d, nullptr, st);
  } else {
    dim3 gnm((unsigned)cdiv(m, 32), (unsigned)cdiv(n, 32));
    sgemm_strided_kernel<<<gnm, 256, 0, st>>>(vis, d, 1, txt, 1, d, A, m, N, M, D, nullptr);
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
    dim3 gnd((unsigned)cdiv(d, 32), (unsigned)cdiv(n, 32)), gmd((unsigned)cdiv(d, 32), (unsigned)cdiv(m, 32));
    sgemm_strided_kernel<<<gnd, 256, 0, st>>>(G, m, 1, txt, d, 1, d_vis, d, N, D, M, nullptr, 0);     // dV = G T
    sgemm_strided_kernel<<<gmd, 256, 0, st>>>(G, 1, m, vis, d, 1, d_txt, d, M, D, N, nullptr, 0);     // dT = G^T V
  }
  XP_CHECK_LAUNCH(who);
  return XP_OK;
}
