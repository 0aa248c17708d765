// Retrieval at gallery scale (xp_retrieval_ranks_streamed / xp_retrieval_topk / xp_retrieval_dsl_stats / xp_retrieval_topk_dsl;
// include/xpretrain_hip.h states the contract, the numpy references are tests/retrieval_stream_ref.py and retrieval_dsl_ref.py).
// One fp32 score core, s_ij = sum_k q[i,k] g[j,k], and three consumers that never write a score to global memory: column
// statistics of the dual-softmax re-rank, rank counts in both directions, top-k.
//
// DSL-weighted search connects them: the statistics are an entry of their own (launch_col_stats: the launches the rank call makes,
// so the bits it forms internally; an earlier result may lead the fold), and topk_kernel's MODE turns the score into
// x = dsl_x(s, theta, mx, sum) -- the function the counting kernels use -- with the statistics of the candidate's gallery row or of
// the query row, at the one place where the accumulators go to the LDS score tile.  The list is exact GIVEN the statistics: x
// depends on the two rows, d, theta and (mx, sum) alone, so shards fed the same statistics give the one-shot bits.
//
// Score core: a 128 x 128 tile of scores per 256-thread workgroup; both operand tiles are staged in LDS in 32-column chunks
// (rows of 36 floats: 16-byte aligned rows, a stride of 36 banks), the next chunk's global loads are in flight while the current
// one is multiplied.  Each of the 4 waves owns 64 x 64 scores as 2 x 2 v_mfma_f32_32x32x2_f32 accumulators: f32 in, f32 out, one
// rounding per product -- bit for bit the fmaf chain over k in the order   for c8 in chunks of 8: for e in 0..3: k = c8+e, c8+4+e
// starting from +0.  Rows and columns beyond the operands and k >= d are zeros: fma(0, 0, acc) == acc.  So the bits of s_ij depend
// on row i of q, row j of g and d alone -- not on the tile, the grid, the split or nq / ng (POSITION INDEPENDENCE): duplicate rows
// tie exactly, and the labelled entry's value, computed by label_scores_kernel through the same instruction in the same k order,
// equals the candidate's value the counting pass sees for the label's own column (equal >= 1).
//
// Determinism: no float atomics.  Column statistics are folded lane-locally over the query tiles in ascending order, then across
// the two row halves of the accumulator layout, the two waves and the query splits in a fixed order.  Counts are int32 and meet
// in atomicAdd (exact in any order).  Top-k lists are merged under a total order (value descending, index ascending).
#include "common.h"
#include <limits.h>
#include <math.h>
#include <algorithm>
#include <cmath>

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int TILE = XP_RETRIEVAL_TILE;          // scores per workgroup: TILE x TILE
constexpr int BK = 32, LDT = 36;                 // staged k chunk; floats per staged row
constexpr int THREADS = 256;
constexpr int STAGE_FLOATS = 2 * TILE * LDT;     // the q tile, then the g tile
constexpr int TARGET_BLOCKS = 512;               // a launch that has fewer tiles than this splits its streamed dimension
constexpr int TOPK_TARGET_BLOCKS = 512;          // two workgroups per CU: one selects while the other multiplies
constexpr int64_t NO_INDEX = INT64_MAX;          // the index of an empty top-k slot (value -inf): it loses against every candidate
static_assert(TILE == 128, "the wave / accumulator maps below are written for 128 x 128 tiles");

__device__ __forceinline__ int64_t cdiv_dev(int64_t n) { return (n + TILE - 1) / TILE; }      // tiles of an extent
__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// elements k .. k+3 of row `row` of a [nrows, d] matrix; zeros beyond either extent.  VEC: d % 4 == 0 and a 16-byte aligned base
template <bool VEC>
__device__ __forceinline__ f32x4 load_row4(const float* __restrict__ base, int64_t row, int64_t nrows, int d, int k) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (row < nrows && k < d) {
    const float* p = base + row * (int64_t)d + k;
    if (VEC) {
      v = load4(p);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (k + e < d) v[e] = p[e];
    }
  }
  return v;
}

// the row of accumulator register `reg` of 32 x 32 block `a` (of the wave's two) in lane half h; the column is lane & 31
__device__ __forceinline__ int acc_row(int a, int reg, int h) { return a * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// acc[a][b] = the scores of query rows i0 + wm*64 + a*32 .. and gallery rows j0 + wn*64 + b*32 .. (wave w: wm = w >> 1, wn = w & 1).
// `lds`: STAGE_FLOATS floats.  Ends behind a __syncthreads(): the caller may reuse the staging area at once.
template <bool VEC>
__device__ __forceinline__ void score_tile(const float* __restrict__ q, const float* __restrict__ g, int64_t i0, int64_t j0, int64_t nq,
                                           int64_t ng, int d, float* lds, f32x16 (&acc)[2][2]) {
  float* const qa = lds;
  float* const gb = lds + TILE * LDT;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w >> 1, wn = w & 1;
  const int lr = t >> 3, lk = (t & 7) * 4;               // this thread stages rows lr + 32 p, columns lk .. lk+3 of each chunk
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
  f32x4 ra[4], rb[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    ra[p] = load_row4<VEC>(q, i0 + lr + 32 * p, nq, d, lk);
    rb[p] = load_row4<VEC>(g, j0 + lr + 32 * p, ng, d, lk);
  }
  for (int k0 = 0; k0 < d; k0 += BK) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      store4(qa + (lr + 32 * p) * LDT + lk, ra[p]);
      store4(gb + (lr + 32 * p) * LDT + lk, rb[p]);
    }
    __syncthreads();
    if (k0 + BK < d) {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        ra[p] = load_row4<VEC>(q, i0 + lr + 32 * p, nq, d, k0 + BK + lk);
        rb[p] = load_row4<VEC>(g, j0 + lr + 32 * p, ng, d, k0 + BK + lk);
      }
    }
#pragma unroll
    for (int c = 0; c < BK / 8; ++c) {
      if (k0 + c * 8 < d) {                                  // (uniform) a chunk of zeros leaves every accumulator as it is
        const f32x4 a0 = load4(qa + (wm * 64 + r) * LDT + c * 8 + h * 4), a1 = load4(qa + (wm * 64 + 32 + r) * LDT + c * 8 + h * 4);
        const f32x4 b0 = load4(gb + (wn * 64 + r) * LDT + c * 8 + h * 4), b1 = load4(gb + (wn * 64 + 32 + r) * LDT + c * 8 + h * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          acc[0][0] = mfma32(a0[e], b0[e], acc[0][0]);
          acc[0][1] = mfma32(a0[e], b1[e], acc[0][1]);
          acc[1][0] = mfma32(a1[e], b0[e], acc[1][0]);
          acc[1][1] = mfma32(a1[e], b1[e], acc[1][1]);
        }
      }
    }
    __syncthreads();
  }
}

// the re-ranked score: s * softmax_i(theta s)_ij with the column's statistics -- ONE function for candidates and labels
__device__ __forceinline__ float dsl_x(float s, float theta, float mx, float sum) { return s * (expf(fmaf(s, theta, -mx)) / sum); }

// ---------------------------------------------------------------------------------------------------------- labelled entries
// One wave per 32 (query row, gallery row) pairs: blocks [0, nbq) the row direction (i, labels_q[i] or i) -> xlab_q[i], blocks
// [nbq, ..) the column direction (labels_g[j] or j, j) -> xlab_g[j].  The 32 query rows and the 32 gallery rows go through the
// score core's instruction in its k order, straight from global memory; pair p is the diagonal element (p, p) of the block.
// A label outside its range gives NaN (it compares false with everything: greater = equal = 0) and reads nothing.
template <bool VEC>
XP_NO_PK_F32 __global__ __launch_bounds__(64) void label_scores_kernel(const float* __restrict__ q, const float* __restrict__ g,
                                                                       const int64_t* __restrict__ labels_q,
                                                                       const int64_t* __restrict__ labels_g, int64_t nq, int64_t ng, int d,
                                                                       int nbq, int dsl, float theta, const float* __restrict__ col_mx,
                                                                       const float* __restrict__ col_sum, float* __restrict__ xlab_q,
                                                                       float* __restrict__ xlab_g) {
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const bool rows = (int)blockIdx.x < nbq;
  const int64_t p = (int64_t)(rows ? blockIdx.x : blockIdx.x - nbq) * 32 + r;       // the pair this lane loads operands for
  int64_t i = -1, j = -1;
  if (rows) {
    if (p < nq) { i = p; j = labels_q ? labels_q[p] : p; }
  } else {
    if (p < ng) { j = p; i = labels_g ? labels_g[p] : p; }
  }
  const bool ok = i >= 0 && i < nq && j >= 0 && j < ng;
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  for (int c8 = 0; c8 < d; c8 += 8) {
    const f32x4 a = load_row4<VEC>(q, ok ? i : nq, nq, d, c8 + 4 * h), b = load_row4<VEC>(g, ok ? j : ng, ng, d, c8 + 4 * h);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = mfma32(a[e], b[e], acc);
  }
  // element (r, r): column r is lanes r and r + 32; row r is register (r & 3) + 4 (r >> 3) of lane half (r >> 2) & 1
  if (h != ((r >> 2) & 1)) return;
  const int reg = (r & 3) + 4 * (r >> 3);
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e)
    if (e == reg) s = acc[e];
  const bool in_range = rows ? p < nq : p < ng;
  if (!in_range) return;
  float x = NAN;
  if (ok) x = dsl ? dsl_x(s, theta, col_mx[j], col_sum[j]) : s;
  (rows ? xlab_q : xlab_g)[p] = x;
}

// ---------------------------------------------------------------------------------------------------------- column statistics
// (m, s) of a set of logits v: m = max v, s = sum exp(v - m); the empty set is (-inf, 0)
__device__ __forceinline__ void stat_merge(float& m, float& s, float m2, float s2) {
  const float mm = fmaxf(m, m2);
  if (mm == -INFINITY) { m = mm; s = 0.f; return; }
  s = s * expf(m - mm) + s2 * expf(m2 - mm);
  m = mm;
}

// grid (gallery tiles, query splits): the block folds the query tiles [y * tiles_per_split, ..) into its 128 columns' (m, s)
template <bool VEC>
XP_NO_PK_F32 __global__ __launch_bounds__(THREADS) void col_stats_kernel(const float* __restrict__ q, const float* __restrict__ g, int64_t nq,
                                                                         int64_t ng, int d, float theta, int tiles_per_split,
                                                                         float* __restrict__ part_mx, float* __restrict__ part_sum) {
  __shared__ __attribute__((aligned(16))) float lds[STAGE_FLOATS];
  __shared__ float x_m[2][64], x_s[2][64];                          // the wm = 1 waves' results, per wn and column
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w >> 1, wn = w & 1, r = lane & 31, h = lane >> 5;
  const int64_t j0 = (int64_t)blockIdx.x * TILE;
  const int64_t qtiles = cdiv_dev(nq);
  const int64_t t0 = (int64_t)blockIdx.y * tiles_per_split, t1 = min(t0 + tiles_per_split, qtiles);
  float m[2] = {-INFINITY, -INFINITY}, s[2] = {0.f, 0.f};
  f32x16 acc[2][2];
  for (int64_t qt = t0; qt < t1; ++qt) {
    const int64_t i0 = qt * TILE;
    score_tile<VEC>(q, g, i0, j0, nq, ng, d, lds, acc);
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      float tm = -INFINITY;
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const bool valid = i0 + wm * 64 + acc_row(a, e, h) < nq;
          const float v = valid ? acc[a][b][e] * theta : -INFINITY;
          acc[a][b][e] = v;
          tm = fmaxf(tm, v);
        }
      const float mm = fmaxf(m[b], tm);
      if (mm != -INFINITY) {
        float sum = s[b] * expf(m[b] - mm);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int e = 0; e < 16; ++e) sum += expf(acc[a][b][e] - mm);
        s[b] = sum;
        m[b] = mm;
      }
    }
  }
#pragma unroll
  for (int b = 0; b < 2; ++b) {                                      // lane half 0, then lane half 1 (the same bits in both)
    const float om = __shfl_xor(m[b], 32, 64), os = __shfl_xor(s[b], 32, 64);
    float m0 = h ? om : m[b], s0 = h ? os : s[b];
    stat_merge(m0, s0, h ? m[b] : om, h ? s[b] : os);
    m[b] = m0; s[b] = s0;
  }
  if (wm == 1 && h == 0) {
#pragma unroll
    for (int b = 0; b < 2; ++b) { x_m[wn][b * 32 + r] = m[b]; x_s[wn][b * 32 + r] = s[b]; }
  }
  __syncthreads();
  if (wm == 0 && h == 0) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int64_t j = j0 + wn * 64 + b * 32 + r;
      if (j < ng) {
        stat_merge(m[b], s[b], x_m[wn][b * 32 + r], x_s[wn][b * 32 + r]);
        part_mx[(int64_t)blockIdx.y * ng + j] = m[b];
        part_sum[(int64_t)blockIdx.y * ng + j] = s[b];
      }
    }
  }
}

// the query splits of column j, ascending; `prev_mx` / `prev_sum` (null, or an earlier call's result: they may BE col_mx / col_sum)
// lead the fold as one more operand -- an `over` set that arrives in shards folds in shard order
__global__ void col_stats_combine_kernel(const float* __restrict__ part_mx, const float* __restrict__ part_sum, int64_t ng, int splits,
                                         const float* prev_mx, const float* prev_sum, float* col_mx, float* col_sum) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= ng) return;
  float m = prev_mx ? prev_mx[j] : part_mx[j], s = prev_mx ? prev_sum[j] : part_sum[j];
  for (int y = prev_mx ? 0 : 1; y < splits; ++y) stat_merge(m, s, part_mx[(int64_t)y * ng + j], part_sum[(int64_t)y * ng + j]);
  col_mx[j] = m;
  col_sum[j] = s;
}

// ---------------------------------------------------------------------------------------------------------- counts
// grid (gallery tiles, query tiles).  x = the score or its re-ranked form; per query row i the candidates above / equal to
// xlab_q[i], per gallery column j those above / equal to xlab_g[j], both from the same accumulators.  Row counts: one ballot per
// accumulator register covers 32 columns of two rows (the lane halves); lane (a * 16 + reg, h) keeps the sum for its row.
template <bool VEC, bool DSL>
XP_NO_PK_F32 __global__ __launch_bounds__(THREADS) void counts_kernel(const float* __restrict__ q, const float* __restrict__ g, int64_t nq,
                                                                      int64_t ng, int d, float theta, const float* __restrict__ col_mx,
                                                                      const float* __restrict__ col_sum, const float* __restrict__ xlab_q,
                                                                      const float* __restrict__ xlab_g, int* __restrict__ greater_q,
                                                                      int* __restrict__ equal_q, int* __restrict__ greater_g,
                                                                      int* __restrict__ equal_g) {
  __shared__ __attribute__((aligned(16))) float lds[STAGE_FLOATS];
  __shared__ float s_lq[TILE], s_lg[TILE], s_mx[TILE], s_sum[TILE];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w >> 1, wn = w & 1, r = lane & 31, h = lane >> 5;
  const int64_t j0 = (int64_t)blockIdx.x * TILE, i0 = (int64_t)blockIdx.y * TILE;
  const bool want_q = greater_q != nullptr, want_g = greater_g != nullptr;
  if (t < TILE) {
    s_lq[t] = (want_q && i0 + t < nq) ? xlab_q[i0 + t] : NAN;
    s_lg[t] = (want_g && j0 + t < ng) ? xlab_g[j0 + t] : NAN;
    s_mx[t] = (DSL && j0 + t < ng) ? col_mx[j0 + t] : 0.f;
    s_sum[t] = (DSL && j0 + t < ng) ? col_sum[j0 + t] : 1.f;
  }
  f32x16 acc[2][2];
  score_tile<VEC>(q, g, i0, j0, nq, ng, d, lds, acc);                  // (its barriers order the loads above before the reads below)
  bool cvalid[2];
  float lg[2], mx[2], sum[2];
  int cg[2] = {0, 0}, ce[2] = {0, 0}, rg = 0, re = 0;
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int c = wn * 64 + b * 32 + r;
    cvalid[b] = j0 + c < ng;
    lg[b] = s_lg[c]; mx[b] = s_mx[c]; sum[b] = s_sum[c];
  }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int rowl = wm * 64 + acc_row(a, e, h);
      const bool rvalid = i0 + rowl < nq;
      const float lq = s_lq[rowl];
      int ng_row[2] = {0, 0}, ne_row[2] = {0, 0};                  // per lane half, wave-uniform
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const float sc = acc[a][b][e];
        const float x = DSL ? dsl_x(sc, theta, mx[b], sum[b]) : sc;
        const bool valid = rvalid && cvalid[b];
        if (want_q) {
          const unsigned long long bg = __ballot(valid && x > lq), be = __ballot(valid && x == lq);
          ng_row[0] += __popc((unsigned)bg); ng_row[1] += __popc((unsigned)(bg >> 32));
          ne_row[0] += __popc((unsigned)be); ne_row[1] += __popc((unsigned)(be >> 32));
        }
        cg[b] += valid && x > lg[b];
        ce[b] += valid && x == lg[b];
      }
      if (r == a * 16 + e) { rg += ng_row[h]; re += ne_row[h]; }
    }
  if (want_q) {
    const int64_t i = i0 + wm * 64 + acc_row(r >> 4, r & 15, h);
    if (i < nq) {
      if (rg) atomicAdd(greater_q + i, rg);
      if (re) atomicAdd(equal_q + i, re);
    }
  }
  if (want_g) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int gsum = cg[b] + __shfl_xor(cg[b], 32, 64), esum = ce[b] + __shfl_xor(ce[b], 32, 64);
      if (h == 0 && cvalid[b]) {
        const int64_t j = j0 + wn * 64 + b * 32 + r;
        if (gsum) atomicAdd(greater_g + j, gsum);
        if (esum) atomicAdd(equal_g + j, esum);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------- top-k
// A list of up to 128 (value, index) pairs, best first, lives in one wave's registers: lane l holds positions l and l + 64.
__device__ __forceinline__ bool better(float v, int64_t i, float w, int64_t j) { return v > w || (v == w && i < j); }
// (uniform src) lane src's value in every lane: v_readlane_b32
__device__ __forceinline__ int lane_i32(int x, int src) { return __builtin_amdgcn_readlane(x, src); }
__device__ __forceinline__ float lane_f32(float x, int src) { return __int_as_float(lane_i32(__float_as_int(x), src)); }
__device__ __forceinline__ int64_t lane_i64(int64_t x, int src) {
  return ((int64_t)lane_i32((int)(x >> 32), src) << 32) | (unsigned)lane_i32((int)(x & 0xffffffffll), src);
}
// lane l takes lane l - 1's value (DPP wave_shr:1); lane 0 keeps its own
__device__ __forceinline__ int up1_i32(int x) { return __builtin_amdgcn_update_dpp(x, x, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ float up1_f32(float x) { return __int_as_float(up1_i32(__float_as_int(x))); }
__device__ __forceinline__ int64_t up1_i64(int64_t x) {
  return ((int64_t)up1_i32((int)(x >> 32)) << 32) | (unsigned)up1_i32((int)(x & 0xffffffffll));
}
struct TopList {
  float v0, v1;
  int64_t i0, i1;
  __device__ __forceinline__ void load(const float* vals, const int64_t* idx, int k, int lane) {
    v0 = lane < k ? vals[lane] : -INFINITY;           i0 = lane < k ? idx[lane] : NO_INDEX;
    v1 = lane + 64 < k ? vals[lane + 64] : -INFINITY; i1 = lane + 64 < k ? idx[lane + 64] : NO_INDEX;
  }
  __device__ __forceinline__ void store(float* vals, int64_t* idx, int k, int lane) const {
    if (lane < k) { vals[lane] = v0; idx[lane] = i0; }
    if (lane + 64 < k) { vals[lane + 64] = v1; idx[lane + 64] = i1; }
  }
  // (wave-uniform candidate) the candidate goes behind every entry that is better than it; the last entry drops out
  __device__ __forceinline__ void insert(float cv, int64_t ci, int lane) {
    const int p = __popcll(__ballot(better(v0, i0, cv, ci))) + __popcll(__ballot(better(v1, i1, cv, ci)));
    const float u0 = up1_f32(v0), u1 = up1_f32(v1), e0 = lane_f32(v0, 63);
    const int64_t w0 = up1_i64(i0), w1 = up1_i64(i1), f0 = lane_i64(i0, 63);
    if (lane == p) { v0 = cv; i0 = ci; }
    else if (lane > p) { v0 = u0; i0 = w0; }
    if (lane + 64 == p) { v1 = cv; i1 = ci; }
    else if (lane + 64 > p) { v1 = lane == 0 ? e0 : u1; i1 = lane == 0 ? f0 : w1; }
  }
  __device__ __forceinline__ void entry(int pos, float& v, int64_t& i) const {     // (uniform pos)
    v = pos < 64 ? lane_f32(v0, pos) : lane_f32(v1, pos - 64);
    i = pos < 64 ? lane_i64(i0, pos) : lane_i64(i1, pos - 64);
  }
};

// grid (query tiles, gallery splits).  Split y streams the gallery tiles [y * tiles_per_split, ..) past its 128 queries; the scores
// of a tile go to LDS, wave w then owns rows 32 w .. 32 w + 31: a row's 128 candidates are tested against the row's k-th best
// (lane rr of the wave keeps it for row rr), and only for a row with a candidate that passes is the list fetched (split 0: the
// output itself, so that `accumulate` is "do not clear it"; split y > 0: lists in the workspace), updated in registers and put back.
//
// MODE: what a candidate's value is.  PLAIN: the score s.  DSL_GALLERY / DSL_QUERIES: dsl_x(s, theta, mx, sum) with the statistics
// of the candidate's gallery row (mx / sum [ng]: a lane's two columns, loaded per gallery tile) or of the query row (mx / sum [nq]:
// the block's 128 queries, loaded once into LDS).  The mode acts where the accumulators go to the LDS score tile and nowhere else:
// thresholds, the first tile's ranking, the lists and their merge see x.
enum { PLAIN = 0, DSL_GALLERY = XP_DSL_OF_GALLERY, DSL_QUERIES = XP_DSL_OF_QUERIES };
template <bool VEC, int MODE>
XP_NO_PK_F32 __global__ __launch_bounds__(THREADS) void topk_kernel(const float* __restrict__ q, const float* __restrict__ g, int64_t nq,
                                                                    int64_t ng, int d, int k, int64_t index_base, int accumulate,
                                                                    int tiles_per_split, float* __restrict__ vals, int64_t* __restrict__ idx,
                                                                    float* __restrict__ ws_vals, int64_t* __restrict__ ws_idx, float theta,
                                                                    const float* __restrict__ dsl_mx, const float* __restrict__ dsl_sum) {
  __shared__ __attribute__((aligned(16))) float lds[TILE * TILE];     // staging (STAGE_FLOATS), then the tile's scores
  static_assert(STAGE_FLOATS <= TILE * TILE, "the staging area lies inside the score tile");
  __shared__ float q_mx[MODE == DSL_QUERIES ? TILE : 1], q_sum[MODE == DSL_QUERIES ? TILE : 1];
  static_assert(sizeof(lds) + 2 * TILE * sizeof(float) <= 80 << 10, "two workgroups per CU (TOPK_TARGET_BLOCKS) on 160 KiB of LDS");
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w >> 1, wn = w & 1, r = lane & 31, h = lane >> 5;
  const int64_t i0 = (int64_t)blockIdx.x * TILE;
  const int split = blockIdx.y;
  float* const lv = split == 0 ? vals : ws_vals + (int64_t)(split - 1) * nq * k;
  int64_t* const li = split == 0 ? idx : ws_idx + (int64_t)(split - 1) * nq * k;
  const bool fresh = split > 0 || !accumulate;
  // the k-th best of row 32 w + lane (lanes 0..31), and the lists' initial state
  float thr_v = -INFINITY;
  int64_t thr_i = NO_INDEX;
  for (int rr = 0; rr < 32; ++rr) {
    const int64_t i = i0 + w * 32 + rr;
    if (i >= nq) break;
    if (fresh) {
      for (int p = lane; p < k; p += 64) { lv[i * k + p] = -INFINITY; li[i * k + p] = NO_INDEX; }
    } else if (lane == rr) {
      thr_v = lv[i * k + k - 1];
      thr_i = li[i * k + k - 1];
    }
  }
  if (MODE == DSL_QUERIES && t < TILE) {          // rows beyond nq: the neutral pair (score_tile's barriers are in front of the reads)
    q_mx[t] = i0 + t < nq ? dsl_mx[i0 + t] : 0.f;
    q_sum[t] = i0 + t < nq ? dsl_sum[i0 + t] : 1.f;
  }
  const int64_t gtiles = cdiv_dev(ng);
  const int64_t t0 = (int64_t)split * tiles_per_split, t1 = min(t0 + tiles_per_split, gtiles);
  f32x16 acc[2][2];
  for (int64_t gt = t0; gt < t1; ++gt) {
    const int64_t j0 = gt * TILE;
    float cmx[2] = {0.f, 0.f}, csum[2] = {1.f, 1.f};        // DSL_GALLERY: this lane's two columns (the neutral pair beyond ng)
    if (MODE == DSL_GALLERY) {
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int64_t j = j0 + wn * 64 + b * 32 + r;
        if (j < ng) { cmx[b] = dsl_mx[j]; csum[b] = dsl_sum[j]; }
      }
    }
    score_tile<VEC>(q, g, i0, j0, nq, ng, d, lds, acc);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = wm * 64 + acc_row(a, e, h);
        float rmx = 0.f, rsum = 1.f;
        if (MODE == DSL_QUERIES) { rmx = q_mx[row]; rsum = q_sum[row]; }
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const float s = acc[a][b][e];
          lds[row * TILE + wn * 64 + b * 32 + r] = MODE == PLAIN         ? s
                                                   : MODE == DSL_GALLERY ? dsl_x(s, theta, cmx[b], csum[b])
                                                                         : dsl_x(s, theta, rmx, rsum);
        }
      }
    __syncthreads();
    for (int rr = 0; rr < 32; ++rr) {
      const int row = w * 32 + rr;
      const int64_t i = i0 + row;
      if (i >= nq) break;
      float tv = lane_f32(thr_v, rr);
      int64_t ti = lane_i64(thr_i, rr);
      const float c0 = lds[row * TILE + lane], c1 = lds[row * TILE + 64 + lane];
      const int64_t x0 = index_base + j0 + lane, x1 = x0 + 64;
      if (fresh && gt == t0) {
        // an empty list: the tile's candidates, ranked among themselves under the same order, ARE the list -- each lane counts
        // the candidates that beat its two and puts those of rank < k at their position (the __syncthreads() below is in front
        // of the next tile's reads of the list); 128 candidates one by one through the insertion below cost ten times this
        const bool ok0 = j0 + lane < ng, ok1 = j0 + 64 + lane < ng;
        int r0 = 0, r1 = 0;
#pragma unroll 8
        for (int src = 0; src < 64; ++src) {
          const float a = lane_f32(c0, src), b = lane_f32(c1, src);
          const bool va = j0 + src < ng, vb = j0 + 64 + src < ng;
          r0 += (int)(va && (a > c0 || (a == c0 && src < lane))) + (int)(vb && b > c0);
          r1 += (int)(va && a >= c1) + (int)(vb && (b > c1 || (b == c1 && src < lane)));
        }
        if (ok0 && r0 < k) { lv[i * k + r0] = c0; li[i * k + r0] = x0; }
        if (ok1 && r1 < k) { lv[i * k + r1] = c1; li[i * k + r1] = x1; }
        const unsigned long long h0 = __ballot(ok0 && r0 == k - 1), h1 = __ballot(ok1 && r1 == k - 1);
        if (h0 | h1) {                                    // the tile filled the list: its last entry is the row's k-th best
          const int src = __ffsll((long long)(h0 ? h0 : h1)) - 1;
          tv = h0 ? lane_f32(c0, src) : lane_f32(c1, src);
          ti = index_base + j0 + (h0 ? 0 : 64) + src;
          if (lane == rr) { thr_v = tv; thr_i = ti; }
        }
        continue;
      }
      unsigned long long m0 = __ballot(j0 + lane < ng && better(c0, x0, tv, ti));
      unsigned long long m1 = __ballot(j0 + 64 + lane < ng && better(c1, x1, tv, ti));
      if (!(m0 | m1)) continue;
      TopList L;
      L.load(lv + i * k, li + i * k, k, lane);
      for (int half = 0; half < 2; ++half) {
        unsigned long long m = half ? m1 : m0;
        while (m) {
          const int src = __ffsll((long long)m) - 1;
          m &= m - 1;
          const float cv = lane_f32(half ? c1 : c0, src);
          const int64_t ci = index_base + j0 + half * 64 + src;
          if (better(cv, ci, tv, ti)) {
            L.insert(cv, ci, lane);
            L.entry(k - 1, tv, ti);
          }
        }
      }
      L.store(lv + i * k, li + i * k, k, lane);
      if (lane == rr) { thr_v = tv; thr_i = ti; }
    }
    __syncthreads();
  }
}

// one wave per query: the workspace lists of splits 1 .. splits-1, in order, into the output list
__global__ __launch_bounds__(64) void topk_merge_kernel(int64_t nq, int k, int splits, float* __restrict__ vals, int64_t* __restrict__ idx,
                                                        const float* __restrict__ ws_vals, const int64_t* __restrict__ ws_idx) {
  const int lane = threadIdx.x;
  const int64_t i = blockIdx.x;
  TopList L, S;
  L.load(vals + i * k, idx + i * k, k, lane);
  float tv;
  int64_t ti;
  L.entry(k - 1, tv, ti);
  for (int y = 1; y < splits; ++y) {
    S.load(ws_vals + ((int64_t)(y - 1) * nq + i) * k, ws_idx + ((int64_t)(y - 1) * nq + i) * k, k, lane);
    for (int p = 0; p < k; ++p) {
      float cv;
      int64_t ci;
      S.entry(p, cv, ci);
      if (!better(cv, ci, tv, ti)) break;          // S is sorted: nothing behind p can enter either
      L.insert(cv, ci, lane);
      L.entry(k - 1, tv, ti);
    }
  }
  L.store(vals + i * k, idx + i * k, k, lane);
}

// ---------------------------------------------------------------------------------------------------------- host side
int64_t tiles(int64_t n) { return cdiv(n, TILE); }
size_t pad256(size_t n) { return (n + 255) & ~(size_t)255; }

// the streamed dimension's tiles per split: as many splits as bring the launch to `target` blocks, never an empty one
int64_t tiles_per_split(int64_t fixed_tiles, int64_t streamed_tiles, int target) {
  const int64_t splits = std::min<int64_t>(streamed_tiles, std::max<int64_t>(1, target / fixed_tiles));
  return cdiv(streamed_tiles, splits);
}

struct RanksPlan {
  int64_t stat_tiles_per_split, stat_splits;
  size_t off_labels_q, off_labels_g, off_xlab_q, off_xlab_g, off_mx, off_sum, off_part, bytes;
};
RanksPlan ranks_plan(int64_t nq, int64_t ng, int dsl) {
  RanksPlan p;
  p.stat_tiles_per_split = tiles_per_split(tiles(ng), tiles(nq), TARGET_BLOCKS);
  p.stat_splits = cdiv(tiles(nq), p.stat_tiles_per_split);
  size_t o = 0;
  p.off_labels_q = o; o += pad256((size_t)nq * 8);
  p.off_labels_g = o; o += pad256((size_t)ng * 8);
  p.off_xlab_q = o;   o += pad256((size_t)nq * 4);
  p.off_xlab_g = o;   o += pad256((size_t)ng * 4);
  p.off_mx = o;       o += dsl ? pad256((size_t)ng * 4) : 0;
  p.off_sum = o;      o += dsl ? pad256((size_t)ng * 4) : 0;
  p.off_part = o;     o += dsl && p.stat_splits > 1 ? 2 * pad256((size_t)p.stat_splits * ng * 4) : 0;
  p.bytes = o;
  return p;
}

struct TopkPlan {
  int64_t tiles_per_split, splits;
  size_t off_idx, bytes;
};
TopkPlan topk_plan(int64_t nq, int64_t ng, int k) {
  TopkPlan p;
  p.tiles_per_split = tiles_per_split(tiles(nq), tiles(ng), TOPK_TARGET_BLOCKS);
  p.splits = cdiv(tiles(ng), p.tiles_per_split);
  p.off_idx = pad256((size_t)(p.splits - 1) * nq * k * 4);
  p.bytes = std::max<size_t>(256, p.off_idx + pad256((size_t)(p.splits - 1) * nq * k * 8));
  return p;
}

constexpr int64_t MAX_ROWS = (int64_t)INT32_MAX - TILE;       // counts and the block grid stay inside int32
constexpr int64_t MAX_FIXED_TILES = 65535;                    // gridDim.y

int check_shape(const char* fn, int64_t nq, int64_t ng, int64_t d) {
  XP_REQUIRE(nq > 0 && ng > 0 && d > 0, "%s: nq=%lld, ng=%lld and d=%lld must all be positive", fn, (long long)nq, (long long)ng, (long long)d);
  XP_REQUIRE(nq <= MAX_ROWS && ng <= MAX_ROWS && d <= (1 << 24), "%s: nq=%lld / ng=%lld / d=%lld beyond the supported extent (2^31 - 129 rows, "
             "2^24 columns)", fn, (long long)nq, (long long)ng, (long long)d);
  return XP_OK;
}

// labels the host can read are checked here; returns the pointer the kernels read (labels in ordinary host memory are staged)
int prepare_labels(const char* fn, const char* name, const int64_t* labels, int64_t n, int64_t range, void* stage, hipStream_t st,
                   const int64_t** out) {
  *out = labels;
  if (!labels) return XP_OK;
  hipPointerAttribute_t at;
  const hipError_t e = hipPointerGetAttributes(&at, labels);
  if (e != hipSuccess) (void)hipGetLastError();
  if (e == hipSuccess && at.type == hipMemoryTypeDevice) return XP_OK;          // device memory: the range is the caller's duty
  for (int64_t i = 0; i < n; ++i)
    XP_REQUIRE(labels[i] >= 0 && labels[i] < range, "%s: %s[%lld] = %lld is not in [0, %lld)", fn, name, (long long)i, (long long)labels[i],
               (long long)range);
  if (e == hipSuccess && (at.type == hipMemoryTypeHost || at.type == hipMemoryTypeManaged)) return XP_OK;
  if (hipMemcpyAsync(stage, labels, (size_t)n * 8, hipMemcpyHostToDevice, st) != hipSuccess) {
    xp_set_error("%s: copying %s to the device failed: %s", fn, name, hipGetErrorString(hipGetLastError()));
    return XP_ERR_LAUNCH;
  }
  *out = (const int64_t*)stage;
  return XP_OK;
}

// the column statistics of g's rows over q's rows under plan p -> col_mx / col_sum [ng]: the ONE launch sequence of
// xp_retrieval_ranks_streamed and xp_retrieval_dsl_stats.  `part`: the per-split (mx, then sum) partials, 2 * part_bytes(p, ng) bytes,
// touched when the plan splits the query tiles or `merge` is set.  merge: col_mx / col_sum hold an earlier result, which leads the
// fold of this call's splits.
size_t part_bytes(const RanksPlan& p, int64_t ng) { return pad256((size_t)p.stat_splits * ng * 4); }
int launch_col_stats(const char* fn, const float* q, const float* g, int64_t nq, int64_t ng, int D, float theta, bool vec, const RanksPlan& p,
                     float* part, bool merge, float* col_mx, float* col_sum, hipStream_t st) {
  const bool direct = p.stat_splits == 1 && !merge;
  float* const pm = direct ? col_mx : part;
  float* const ps = direct ? col_sum : (float*)((char*)part + part_bytes(p, ng));
  dim3 grid((unsigned)tiles(ng), (unsigned)p.stat_splits);
  if (vec) col_stats_kernel<true><<<grid, THREADS, 0, st>>>(q, g, nq, ng, D, theta, (int)p.stat_tiles_per_split, pm, ps);
  else col_stats_kernel<false><<<grid, THREADS, 0, st>>>(q, g, nq, ng, D, theta, (int)p.stat_tiles_per_split, pm, ps);
  XP_CHECK_LAUNCH(fn);
  if (!direct) {
    col_stats_combine_kernel<<<(unsigned)cdiv(ng, 256), 256, 0, st>>>(pm, ps, ng, (int)p.stat_splits, merge ? col_mx : nullptr,
                                                                      merge ? col_sum : nullptr, col_mx, col_sum);
    XP_CHECK_LAUNCH(fn);
  }
  return XP_OK;
}

}  // namespace

extern "C" int xp_retrieval_stream_plan(int64_t nq, int64_t ng, int32_t k, int32_t* stat_tiles_per_split, int32_t* topk_tiles_per_split) {
  if (int rc = check_shape("xp_retrieval_stream_plan", nq, ng, 1)) return rc;
  XP_REQUIRE(stat_tiles_per_split && topk_tiles_per_split, "xp_retrieval_stream_plan: null output");
  *stat_tiles_per_split = (int32_t)ranks_plan(nq, ng, 1).stat_tiles_per_split;
  *topk_tiles_per_split = (int32_t)topk_plan(nq, ng, k > 0 ? k : 1).tiles_per_split;
  return XP_OK;
}

extern "C" size_t xp_retrieval_ranks_streamed_workspace_bytes(int64_t nq, int64_t ng, int64_t d, int32_t dsl) {
  if (check_shape("xp_retrieval_ranks_streamed_workspace_bytes", nq, ng, d)) return 0;
  return ranks_plan(nq, ng, dsl).bytes;
}

extern "C" int xp_retrieval_ranks_streamed(const float* q, const float* g, const int64_t* labels_q, const int64_t* labels_g, int64_t nq,
                                           int64_t ng, int64_t d, int32_t dsl, float theta, int32_t* greater_q, int32_t* equal_q,
                                           int32_t* greater_g, int32_t* equal_g, void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "xp_retrieval_ranks_streamed";
  XP_REQUIRE(q && g, "%s: q or g is null", fn);
  // (q and g: alignment class `any` -- load_row4<false> reads one float per access wherever `vec` below is false)
  XP_REQUIRE_ALIGNED(fn, 16, XP_P(labels_q), XP_P(labels_g), XP_P(greater_q), XP_P(equal_q), XP_P(greater_g), XP_P(equal_g), XP_P(workspace));
  if (int rc = check_shape(fn, nq, ng, d)) return rc;
  XP_REQUIRE((greater_q != nullptr) == (equal_q != nullptr) && (greater_g != nullptr) == (equal_g != nullptr),
             "%s: a direction's greater and equal outputs come together", fn);
  XP_REQUIRE(greater_q || greater_g, "%s: no direction asked for (both pairs of outputs are null)", fn);
  XP_REQUIRE(!greater_q || labels_q || nq <= ng, "%s: diagonal labels need a label for every query (nq=%lld > ng=%lld without labels_q)", fn,
             (long long)nq, (long long)ng);
  XP_REQUIRE(!greater_g || labels_g || ng <= nq, "%s: diagonal labels need a label for every query (ng=%lld > nq=%lld without labels_g)", fn,
             (long long)ng, (long long)nq);
  XP_REQUIRE(tiles(nq) <= MAX_FIXED_TILES, "%s: nq=%lld beyond %lld query tiles of one launch", fn, (long long)nq, (long long)MAX_FIXED_TILES);
  XP_REQUIRE(!dsl || std::isfinite(theta), "%s: theta is not finite", fn);
  const RanksPlan p = ranks_plan(nq, ng, dsl);
  XP_REQUIRE(workspace && workspace_bytes >= p.bytes, "%s: workspace of %zu bytes, %zu needed", fn, workspace ? workspace_bytes : (size_t)0,
             p.bytes);
  hipStream_t st = (hipStream_t)stream;
  char* const ws = (char*)workspace;
  const int64_t *lq = nullptr, *lgl = nullptr;
  if (greater_q)
    if (int rc = prepare_labels(fn, "labels_q", labels_q, nq, ng, ws + p.off_labels_q, st, &lq)) return rc;
  if (greater_g)
    if (int rc = prepare_labels(fn, "labels_g", labels_g, ng, nq, ws + p.off_labels_g, st, &lgl)) return rc;
  float* const xlab_q = (float*)(ws + p.off_xlab_q);
  float* const xlab_g = (float*)(ws + p.off_xlab_g);
  float* const col_mx = dsl ? (float*)(ws + p.off_mx) : nullptr;
  float* const col_sum = dsl ? (float*)(ws + p.off_sum) : nullptr;
  const bool vec = d % 4 == 0 && ((uintptr_t)q & 15) == 0 && ((uintptr_t)g & 15) == 0;
  const int D = (int)d;
  if (dsl)
    if (int rc = launch_col_stats(fn, q, g, nq, ng, D, theta, vec, p, (float*)(ws + p.off_part), false, col_mx, col_sum, st)) return rc;
  const int nbq = greater_q ? (int)cdiv(nq, 32) : 0, nbg = greater_g ? (int)cdiv(ng, 32) : 0;
  if (vec) label_scores_kernel<true><<<(unsigned)(nbq + nbg), 64, 0, st>>>(q, g, lq, lgl, nq, ng, D, nbq, dsl, theta, col_mx, col_sum, xlab_q, xlab_g);
  else label_scores_kernel<false><<<(unsigned)(nbq + nbg), 64, 0, st>>>(q, g, lq, lgl, nq, ng, D, nbq, dsl, theta, col_mx, col_sum, xlab_q, xlab_g);
  XP_CHECK_LAUNCH(fn);
  hipError_t e = hipSuccess;
  if (greater_q) {
    if (e == hipSuccess) e = hipMemsetAsync(greater_q, 0, (size_t)nq * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(equal_q, 0, (size_t)nq * 4, st);
  }
  if (greater_g) {
    if (e == hipSuccess) e = hipMemsetAsync(greater_g, 0, (size_t)ng * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(equal_g, 0, (size_t)ng * 4, st);
  }
  if (e != hipSuccess) {
    xp_set_error("%s: clearing the counts failed: %s", fn, hipGetErrorString(e));
    return XP_ERR_LAUNCH;
  }
  dim3 grid((unsigned)tiles(ng), (unsigned)tiles(nq));
#define XP_COUNTS(V, S) counts_kernel<V, S><<<grid, THREADS, 0, st>>>(q, g, nq, ng, D, theta, col_mx, col_sum, xlab_q, xlab_g, greater_q, equal_q, greater_g, equal_g)
  if (vec) { if (dsl) XP_COUNTS(true, true); else XP_COUNTS(true, false); }
  else { if (dsl) XP_COUNTS(false, true); else XP_COUNTS(false, false); }
#undef XP_COUNTS
  XP_CHECK_LAUNCH(fn);
  return XP_OK;
}

extern "C" size_t xp_retrieval_topk_workspace_bytes(int64_t nq, int64_t ng, int64_t d, int32_t k) {
  const char* fn = "xp_retrieval_topk_workspace_bytes";
  if (check_shape(fn, nq, ng, d)) return 0;
  if (k < 1 || k > XP_RETRIEVAL_MAX_K || k > ng) {
    xp_set_error("%s: k=%d is not in 1..min(%d, ng=%lld)", fn, k, XP_RETRIEVAL_MAX_K, (long long)ng);
    return 0;
  }
  return topk_plan(nq, ng, k).bytes;
}

// both top-k entries: every refusal, the plan, the launches.  mode PLAIN: theta, mx and sum are not looked at
static int topk_call(const char* fn, const float* q, const float* g, int64_t nq, int64_t ng, int64_t d, int32_t k, int64_t index_base,
                     int32_t accumulate, int mode, float theta, const float* mx, const float* sum, float* vals, int64_t* idx, void* workspace,
                     size_t workspace_bytes, void* stream) {
  XP_REQUIRE(q && g && vals && idx, "%s: q, g, vals or idx is null", fn);
  // (q, g: class `any`, as above; mx, sum too: topk_kernel reads them one float per lane, and a gallery fed shard by shard gets
  //  its slice of the per-gallery statistics -- utils/metrics.py callers pass st[a:b])
  XP_REQUIRE_ALIGNED(fn, 16, XP_P(vals), XP_P(idx), XP_P(workspace));
  if (int rc = check_shape(fn, nq, ng, d)) return rc;
  XP_REQUIRE(k >= 1 && k <= XP_RETRIEVAL_MAX_K && k <= ng, "%s: k=%d is not in 1..min(%d, ng=%lld)", fn, k, XP_RETRIEVAL_MAX_K, (long long)ng);
  XP_REQUIRE(index_base >= 0 && index_base <= INT64_MAX - ng - 1, "%s: index_base=%lld out of range", fn, (long long)index_base);
  XP_REQUIRE(tiles(ng) <= MAX_FIXED_TILES * (int64_t)MAX_FIXED_TILES, "%s: ng=%lld beyond one launch", fn, (long long)ng);
  if (mode != PLAIN) {
    XP_REQUIRE(mode == DSL_GALLERY || mode == DSL_QUERIES, "%s: stats_of=%d is neither XP_DSL_OF_GALLERY (%d) nor XP_DSL_OF_QUERIES (%d)", fn,
               mode, XP_DSL_OF_GALLERY, XP_DSL_OF_QUERIES);
    XP_REQUIRE(mx && sum, "%s: mx or sum is null", fn);
    XP_REQUIRE(std::isfinite(theta), "%s: theta is not finite", fn);
  }
  const TopkPlan p = topk_plan(nq, ng, k);
  XP_REQUIRE(p.splits <= MAX_FIXED_TILES, "%s: ng=%lld beyond one launch", fn, (long long)ng);
  XP_REQUIRE(workspace && workspace_bytes >= p.bytes, "%s: workspace of %zu bytes, %zu needed", fn, workspace ? workspace_bytes : (size_t)0,
             p.bytes);
  hipStream_t st = (hipStream_t)stream;
  float* const ws_vals = (float*)workspace;
  int64_t* const ws_idx = (int64_t*)((char*)workspace + p.off_idx);
  const bool vec = d % 4 == 0 && ((uintptr_t)q & 15) == 0 && ((uintptr_t)g & 15) == 0;
  dim3 grid((unsigned)tiles(nq), (unsigned)p.splits);
#define XP_TOPK(V, M) topk_kernel<V, M><<<grid, THREADS, 0, st>>>(q, g, nq, ng, (int)d, k, index_base, accumulate, (int)p.tiles_per_split, vals, idx, ws_vals, ws_idx, theta, mx, sum)
  if (mode == PLAIN) { if (vec) XP_TOPK(true, PLAIN); else XP_TOPK(false, PLAIN); }
  else if (mode == DSL_GALLERY) { if (vec) XP_TOPK(true, DSL_GALLERY); else XP_TOPK(false, DSL_GALLERY); }
  else { if (vec) XP_TOPK(true, DSL_QUERIES); else XP_TOPK(false, DSL_QUERIES); }
#undef XP_TOPK
  XP_CHECK_LAUNCH(fn);
  if (p.splits > 1) {
    topk_merge_kernel<<<(unsigned)nq, 64, 0, st>>>(nq, k, (int)p.splits, vals, idx, ws_vals, ws_idx);
    XP_CHECK_LAUNCH(fn);
  }
  return XP_OK;
}

extern "C" int xp_retrieval_topk(const float* q, const float* g, int64_t nq, int64_t ng, int64_t d, int32_t k, int64_t index_base,
                                 int32_t accumulate, float* vals, int64_t* idx, void* workspace, size_t workspace_bytes, void* stream) {
  return topk_call("xp_retrieval_topk", q, g, nq, ng, d, k, index_base, accumulate, PLAIN, 0.f, nullptr, nullptr, vals, idx, workspace,
                   workspace_bytes, stream);
}

extern "C" int xp_retrieval_topk_dsl(const float* q, const float* g, int64_t nq, int64_t ng, int64_t d, int32_t k, int64_t index_base,
                                     int32_t accumulate, float theta, int32_t stats_of, const float* mx, const float* sum, float* vals,
                                     int64_t* idx, void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "xp_retrieval_topk_dsl";
  XP_REQUIRE(stats_of == XP_DSL_OF_GALLERY || stats_of == XP_DSL_OF_QUERIES, "%s: stats_of=%d is neither XP_DSL_OF_GALLERY (%d) nor "
             "XP_DSL_OF_QUERIES (%d)", fn, stats_of, XP_DSL_OF_GALLERY, XP_DSL_OF_QUERIES);
  return topk_call(fn, q, g, nq, ng, d, k, index_base, accumulate, stats_of, theta, mx, sum, vals, idx, workspace, workspace_bytes, stream);
}

extern "C" size_t xp_retrieval_dsl_stats_workspace_bytes(int64_t n_over, int64_t n_of, int64_t d) {
  if (check_shape("xp_retrieval_dsl_stats_workspace_bytes", n_over, n_of, d)) return 0;
  return std::max<size_t>(256, 2 * part_bytes(ranks_plan(n_over, n_of, 1), n_of));
}

extern "C" int xp_retrieval_dsl_stats(const float* over, const float* of, int64_t n_over, int64_t n_of, int64_t d, float theta,
                                      int32_t accumulate, float* mx, float* sum, void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "xp_retrieval_dsl_stats";
  XP_REQUIRE(over && of && mx && sum, "%s: over, of, mx or sum is null", fn);
  XP_REQUIRE_ALIGNED(fn, 16, XP_P(mx), XP_P(sum), XP_P(workspace));                              // (over, of: class `any`, as above)
  if (int rc = check_shape(fn, n_over, n_of, d)) return rc;
  XP_REQUIRE(std::isfinite(theta), "%s: theta is not finite", fn);
  const RanksPlan p = ranks_plan(n_over, n_of, 1);
  const size_t need = std::max<size_t>(256, 2 * part_bytes(p, n_of));
  XP_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace of %zu bytes, %zu needed", fn, workspace ? workspace_bytes : (size_t)0, need);
  const bool vec = d % 4 == 0 && ((uintptr_t)over & 15) == 0 && ((uintptr_t)of & 15) == 0;
  return launch_col_stats(fn, over, of, n_over, n_of, (int)d, theta, vec, p, (float*)workspace, accumulate != 0, mx, sum, (hipStream_t)stream);
}

