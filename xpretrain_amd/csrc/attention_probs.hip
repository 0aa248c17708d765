// The attention weights themselves (output_attentions): the softmax matrices the fused kernels of attention.hip / attention_f32.hip
// never store, rebuilt from what they leave behind -- the packed qkv (q pre-scaled) and stats[B,H,S,2] = (row max, log row sum).
// A weight is one independent expression per (query, key), exp((s' - m) - log l), the one attention_f32.hip's backward evaluates:
// no reduction, no online softmax, so any decomposition gives the same bits.  PROXY: CLIPAttention.forward2's two attn_weights
// (modeling/CLIP_ViP.py:332-381), which the reference computes and drops; CAUSAL: CLIPAttention.forward's attn_weights_reshaped
// (:266-330).  Not on the training step's path.
//
// The stores dominate the bytes (cfg #2: 184 MB of fp32 weights per layer against 87 MB of qkv read once, 5.8 GFLOP of scores), so
// the form is the plain fp32 VALU one of attention_f32.hip, for bf16 storage too, turned so that every store of a row is contiguous
// across lanes (measured: DESIGN.md 4.2 -- 9x the time the stores alone need; the serial chain inside a row, not the arithmetic):
//   wave = one PANEL: 64 consecutive key columns x up to RW consecutive query rows of one (sample, head[, frame]).  Lane j keeps
//   its key row (64 floats) in registers for the whole panel; the query row is wave-uniform (scalar loads feed the FMAs from SGPRs),
//   its two statistics are fetched for the whole panel by one vector load and read back lane by lane; per query row the wave
//   stores 64 consecutive floats (256 B).  Rows have any length (6, 53, 74, 212 ... floats), so the stores are 4 bytes per lane: a
//   row start is 4-byte aligned only.  The last panel of a row is partly masked; nothing assumes M <= 16 or M + L <= 208.
//   workgroup = four panels side by side (256 columns of the same rows): rows are not multiples of a 128-byte line, so neighbouring
//   panels write into the same lines -- from one CU they merge in one L2 before they leave it (workgroups land on different XCDs,
//   each with an L2 of its own), and the four waves read the same query rows through the same scalar cache.
//   No LDS, no workspace, no atomics.
#include "common.h"
#include <math.h>

namespace {

constexpr int DH = 64;
constexpr int RW = 32;                               // query rows per panel (<= 64): the key row's load is amortised over RW stores
constexpr float F32_MIN = -3.4028234663852886e38f;   // torch.finfo(float32).min, _expand_mask (:50-61)

enum { FRAME_ROWS = 0, PROXY_ROWS = 1, CAUSAL_ROWS = 2 };

// rows x cols of one problem's matrix, cut into panels; one workgroup per (problem, group of 4 panels side by side, row block)
struct PG {
  int64_t ldqkv;
  int kind, H, S, M, N, L;
  int rows, cols, chunk_groups, row_blocks;
};

// dot(q, k): k is the lane's key row in registers, q a wave-uniform query row in memory.  Read in 16-byte words (ldqkv % 8 == 0 keeps
// every row 16-byte aligned) so that the compiler can take the row through scalar loads and feed the FMAs from SGPRs; a bf16 pair
// is unpacked with a shift and a mask (on the scalar unit then), which is what the conversion to fp32 is.
__device__ __forceinline__ float qdot(const float* q, const float* k) {
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < DH; d += 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(q + d);
    s = fmaf(v[0], k[d], s); s = fmaf(v[1], k[d + 1], s); s = fmaf(v[2], k[d + 2], s); s = fmaf(v[3], k[d + 3], s);
  }
  return s;
}
__device__ __forceinline__ float qdot(const bf16_t* q, const float* k) {
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < DH; d += 8) {
    const u32x4 w = *reinterpret_cast<const u32x4*>(q + d);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s = fmaf(__builtin_bit_cast(float, w[e] << 16), k[d + 2 * e], s);
      s = fmaf(__builtin_bit_cast(float, w[e] & 0xffff0000u), k[d + 2 * e + 1], s);
    }
  }
  return s;
}

template <typename T>
__global__ __launch_bounds__(256) XP_NO_PK_F32 void attn_probs_kernel(const T* __restrict__ qkv, const float* __restrict__ stats,
                                                                       const int64_t* __restrict__ pad, float* __restrict__ out, PG g) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int rb = (int)(blockIdx.x % g.row_blocks);
  const int c0 = ((int)((blockIdx.x / g.row_blocks) % g.chunk_groups) * 4 + wave) * 64;
  if (c0 >= g.cols) return;
  const int64_t prob = blockIdx.x / ((unsigned)g.row_blocks * g.chunk_groups);    // (b, h, n) for FRAME_ROWS, (b, h) otherwise
  const int n = g.kind == FRAME_ROWS ? (int)(prob % g.N) : 0;
  const int64_t bh = g.kind == FRAME_ROWS ? prob / g.N : prob;
  const int h = (int)(bh % g.H);
  const int64_t b = bh / g.H;
  const int r0 = rb * RW;
  const int nrows = g.rows - r0 < RW ? g.rows - r0 : RW;
  const int q0 = (g.kind == FRAME_ROWS ? g.M + n * g.L : 0) + r0;       // token of the panel's first query row
  const int col = c0 + lane;
  const bool ok = col < g.cols;
  // token of this lane's key: FRAME_ROWS columns are [M proxies | the L tokens of frame n]
  const int key = !ok ? 0 : (g.kind == FRAME_ROWS && col >= g.M) ? g.M + n * g.L + (col - g.M) : col;
  const T* base = qkv + b * g.S * g.ldqkv + h * DH;
  const float* st = stats + bh * g.S * 2;
  float* o = out + (prob * g.rows + r0) * g.cols + col;

  if (g.kind == CAUSAL_ROWS && c0 > q0 + nrows - 1) {                   // the whole panel lies above the diagonal: written, not skipped
    if (ok)
      for (int i = 0; i < nrows; ++i) o[(int64_t)i * g.cols] = 0.f;
    return;
  }
  float k[DH];
  {
    const T* krow = base + (int64_t)key * g.ldqkv + g.H * DH;
#pragma unroll
    for (int d = 0; d < DH; d += 4) { const f32x4 v = load4(krow + d); k[d] = v[0]; k[d + 1] = v[1]; k[d + 2] = v[2]; k[d + 3] = v[3]; }
  }
  // the reference's masking: a padded key's score is finfo.min (added to the score; finfo.min absorbs it)
  const bool kpad = pad && pad[b * g.S + key] == 0;
  // (row max, log row sum) of the panel's rows: row i in lane i (RW <= 64)
  float row_m = 0.f, row_lg = 0.f;
  if (lane < nrows) { row_m = st[2 * (q0 + lane)]; row_lg = st[2 * (q0 + lane) + 1]; }
  for (int i = 0; i < nrows; ++i) {
    const int qt = q0 + i;
    const T* q = base + (int64_t)qt * g.ldqkv;                          // wave-uniform
    float s = qdot(q, k);
    if (kpad) s = F32_MIN;
    const float m = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, row_m), i));
    const float lg = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, row_lg), i));
    float p = __expf((s - m) - lg);
    if (g.kind == CAUSAL_ROWS && key > qt) p = 0.f;
    if (ok) o[(int64_t)i * g.cols] = p;
  }
}

template <typename T>
int launch(const void* qkv, const float* stats, const int64_t* pad, float* out, PG g, int64_t problems, hipStream_t st, const char* what) {
  g.chunk_groups = (int)cdiv(g.cols, 4 * 64);
  g.row_blocks = (int)cdiv(g.rows, RW);
  const int64_t grid = problems * g.chunk_groups * g.row_blocks;
  XP_REQUIRE(grid <= 0x7fffffff, "xp_attn_probs: too many panels");
  attn_probs_kernel<T><<<(unsigned)grid, 256, 0, st>>>((const T*)qkv, stats, pad, out, g);
  XP_CHECK_LAUNCH(what);
  return XP_OK;
}

}  // namespace

extern "C" int xp_attn_probs(const void* qkv, int64_t ldqkv, const float* stats, const int64_t* pad_mask,
                             float* probs, float* probs_proxy, int32_t mode, int64_t B, int64_t H, int64_t S,
                             int64_t M, int64_t N, int64_t L, int32_t dtype, void* stream) {
  XP_REQUIRE(qkv && stats && probs, "xp_attn_probs: null pointer");
  XP_REQUIRE_ALIGNED("xp_attn_probs", 16, XP_P(qkv), XP_P(stats), XP_P(pad_mask), XP_P(probs), XP_P(probs_proxy));
  XP_REQUIRE(dtype == XP_BF16 || dtype == XP_F32, "xp_attn_probs: bad dtype %d", dtype);
  XP_REQUIRE(mode == XP_ATTN_PROXY || mode == XP_ATTN_CAUSAL, "xp_attn_probs: bad mode %d", mode);
  XP_REQUIRE(B > 0 && H > 0 && S > 0, "xp_attn_probs: empty problem");
  if (mode == XP_ATTN_CAUSAL) {
    XP_REQUIRE(!probs_proxy, "xp_attn_probs: XP_ATTN_CAUSAL writes probs alone (probs_proxy must be NULL)");
    M = 0; N = 1; L = S;
  } else {
    XP_REQUIRE(M >= 1 && N >= 1 && L >= 1 && S == M + N * L, "xp_attn_probs: S=%lld != M+N*L (%lld,%lld,%lld)",
               (long long)S, (long long)M, (long long)N, (long long)L);
    XP_REQUIRE(probs_proxy, "xp_attn_probs: null pointer (probs_proxy)");
    XP_REQUIRE(!pad_mask, "xp_attn_probs: XP_ATTN_PROXY takes no padding mask");
  }
  XP_REQUIRE(ldqkv >= 3 * H * DH && ldqkv % 8 == 0, "xp_attn_probs: bad leading dimension");
  XP_REQUIRE(S <= 0x3fffffff && H <= 0x7fffffff / DH / 3 && B * H * N <= 0x7fffffff, "xp_attn_probs: problem too large");
  PG g{};
  g.ldqkv = ldqkv; g.H = (int)H; g.S = (int)S; g.M = (int)M; g.N = (int)N; g.L = (int)L;
  hipStream_t st = (hipStream_t)stream;
  const bool bf = dtype == XP_BF16;
  if (mode == XP_ATTN_CAUSAL) {
    g.kind = CAUSAL_ROWS; g.rows = (int)S; g.cols = (int)S;
    return bf ? launch<bf16_t>(qkv, stats, pad_mask, probs, g, B * H, st, "xp_attn_probs")
              : launch<float>(qkv, stats, pad_mask, probs, g, B * H, st, "xp_attn_probs");
  }
  g.kind = FRAME_ROWS; g.rows = (int)L; g.cols = (int)(M + L);
  int rc = bf ? launch<bf16_t>(qkv, stats, nullptr, probs, g, B * H * N, st, "xp_attn_probs(frame rows)")
              : launch<float>(qkv, stats, nullptr, probs, g, B * H * N, st, "xp_attn_probs(frame rows)");
  if (rc) return rc;
  g.kind = PROXY_ROWS; g.rows = (int)M; g.cols = (int)S;
  return bf ? launch<bf16_t>(qkv, stats, nullptr, probs_proxy, g, B * H, st, "xp_attn_probs(proxy rows)")
            : launch<float>(qkv, stats, nullptr, probs_proxy, g, B * H, st, "xp_attn_probs(proxy rows)");
}
