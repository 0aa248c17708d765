// Deterministic fp32 row reductions for gfx950: the split-K slab sum and the column sums every bias gradient, LayerNorm-parameter
// gradient and fused-epilogue partial of a training step ends in.  HBM- / launch-bound; adds only, in a fixed order, so results are
// reproducible bit for bit (tests/reduce_emulation.py restates every order below on the CPU, tests/test_reduce_gpu.py holds the
// kernels to it with torch.equal).
//
// TREE A, the one summation loop of the column sums (tree_a): a workgroup of 4 waves sums rows [r0, r1) for 64 * V columns.
//   wave w takes rows r0+w, r0+w+8, ... into s0 and rows r0+w+4, r0+w+12, ... into s1 (two independent chains of loads);
//   the wave result is s0 + s1; the four wave results are combined through LDS as ((W0 + W1) + W2) + W3.
// (xp_layernorm_bwd's last level, layernorm.hip::ln_param_reduce2_kernel, is NOT tree A: one accumulator per wave.)
//
// Which rows one tree-A workgroup gets -- two partition rules, kept apart on purpose:
//   xp_reduce_rows_batch   n <= RB_DIRECT (64) rows: ONE tree over all n rows.
//                          n > 64: nsum = ceil(n / 32); one tree per nsum consecutive rows, then one tree over the ceil(n / nsum) sums.
//   xp_colsum              n chunk partials (one tree per cs_rows() rows of X), ALWAYS two levels: lvl = ceil(n / 32); one tree per
//   (xp_layernorm_bwd's    lvl consecutive partials, then one tree over the ceil(n / lvl) sums.
//    first level too)
// A tree over one row returns that row, so the rules give the same bits for n <= 32, and nsum == lvl makes them the same for n > 64.
// For 33..64 rows they differ (batch: direct; colsum: pairs first) in about two thirds of the columns: routing xp_colsum through the
// batch path would change its results.
#include "common.h"

namespace {

// ---- split-K slab reduce ----------------------------------------------------------------------------
__global__ void splitk_reduce_kernel(const float* __restrict__ slabs, float* __restrict__ out, int64_t n4,
                                     int splits, int accumulate) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const f32x4* sl = reinterpret_cast<const f32x4*>(slabs);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    f32x4 s = accumulate ? reinterpret_cast<const f32x4*>(out)[i] : f32x4{0.f, 0.f, 0.f, 0.f};
    int z = 0;
    for (; z + 4 <= splits; z += 4) {         // 4 independent 16-byte loads in flight per lane
      const f32x4 a = sl[(int64_t)z * n4 + i], b = sl[(int64_t)(z + 1) * n4 + i];
      const f32x4 c = sl[(int64_t)(z + 2) * n4 + i], d = sl[(int64_t)(z + 3) * n4 + i];
      s += (a + b) + (c + d);
    }
    for (; z < splits; ++z) s += sl[(int64_t)z * n4 + i];
    reinterpret_cast<f32x4*>(out)[i] = s;
  }
}

// ---- tree A -----------------------------------------------------------------------------------------
// V adjacent columns per lane: one float, or an f32x4 (8-byte bf16 / 16-byte fp32 loads, 512 B / 1 KiB contiguous per wave instruction)
template <int V> struct ColsOf { typedef float type; };
template <> struct ColsOf<4> { typedef f32x4 type; };
template <int V> using cols_t = typename ColsOf<V>::type;
template <int V, typename T> __device__ __forceinline__ cols_t<V> load_cols(const T* p) {
  if constexpr (V == 4) return load4(p); else return to_f(*p);
}
template <int V> __device__ __forceinline__ void store_cols(float* p, cols_t<V> v) {
  if constexpr (V == 4) store4(p, v); else *p = v;
}

// Sum of rows [r0, r1) of `in` (row pitch `stride` elements) for the V columns at c, in the order of the head comment.  Called by
// all 256 threads of the workgroup (it contains the barrier); lanes with !ok load nothing.  Every wave returns the combined sum.
// R, C: the caller's row / column index types (int, or int64_t for the rows and columns of X).
template <int V, typename T, typename R, typename C>
__device__ __forceinline__ cols_t<V> tree_a(const T* __restrict__ in, int64_t stride, R r0, R r1, C c, bool ok,
                                            cols_t<V> (*red)[64]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  cols_t<V> s0{}, s1{};
  if (ok) {
    R r = r0 + w;
    for (; r + 4 < r1; r += 8) {
      s0 += load_cols<V>(in + (int64_t)r * stride + c);
      s1 += load_cols<V>(in + (int64_t)(r + 4) * stride + c);
    }
    if (r < r1) s0 += load_cols<V>(in + (int64_t)r * stride + c);
  }
  red[w][lane] = s0 + s1;
  __syncthreads();
  return ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// Column sums of X (bias gradients), first level: one partial row per CS_ROWS-row chunk, 256 columns per workgroup.
// Grid: (cols/256, rows/CS_ROWS).
// rows per chunk: narrow matrices need many chunks to fill the chip, wide ones can take longer chunks (fewer partial rows
// for the second level): aim at >= ~2048 workgroups, 32..128 rows each
inline int cs_rows(int64_t rows, int64_t cols) {
  const int64_t per = rows * cdiv(cols, 256) / 2048;
  return per >= 128 ? 128 : (per >= 64 ? 64 : 32);
}
template <typename T>
__global__ __launch_bounds__(256) void colsum_partial_kernel(const T* __restrict__ X, int64_t rows, int64_t cols, int64_t ldx,
                                                             float* __restrict__ part, int CS_ROWS) {
  __shared__ f32x4 red[4][64];
  const int64_t c = ((int64_t)blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
  const int64_t r0 = (int64_t)blockIdx.y * CS_ROWS;
  const int64_t r1 = r0 + CS_ROWS < rows ? r0 + CS_ROWS : rows;
  const f32x4 t = tree_a<4>(X, ldx, r0, r1, c, c < cols, red);
  if (threadIdx.x < 64 && c < cols) store4(part + (int64_t)blockIdx.y * cols + c, t);
}

// out[y][c] (+)= sum of `nsum` consecutive rows of in[.][width] starting at y*nsum; 64 columns per workgroup.
__global__ __launch_bounds__(256) void rows_reduce_kernel(const float* __restrict__ in, float* __restrict__ out, int nrows,
                                                          int nsum, int width, int accumulate) {
  __shared__ float red[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int r0 = blockIdx.y * nsum, r1 = r0 + nsum < nrows ? r0 + nsum : nrows;
  const float t = tree_a<1>(in, width, r0, r1, c, c < width, red);
  if (threadIdx.x < 64 && c < width) {
    float* o = out + (int64_t)blockIdx.y * width + c;
    *o = accumulate ? *o + t : t;
  }
}

// ---- batched two-level row reduction (bias / LayerNorm-parameter gradients of one encoder layer in two launches) ----
struct BatchArgs {
  XpReduceSeg seg[XP_REDUCE_MAX_SEGS];
  float* part2[XP_REDUCE_MAX_SEGS];        // level-1 output [<=32][width] per segment
  int cb0[XP_REDUCE_MAX_SEGS + 1];         // prefix sum of the segments' column blocks (64 * V columns each)
  int n;
};
constexpr int RB_DIRECT = 64;              // segments with <= this many rows skip level 1

__device__ __forceinline__ int batch_find(const BatchArgs& a, int bx) {
  int s = 0;
  while (s + 1 < a.n && bx >= a.cb0[s + 1]) ++s;
  return s;
}

// LEVEL 1 (grid (blocks, 32)): group y of a segment with more than RB_DIRECT rows -> row y of its part2.
// LEVEL 2 (grid (blocks)): the group sums -- or, for a direct segment, its rows -- -> out.
// V = 4 (16-byte accesses, a quarter of the workgroups: the scalar level 1 of a ViT-B layer is 4992 workgroups of ~4 KB each, 20 us
// of workgroup dispatch on the backward's critical stream for 14 MB) when every segment allows it, else V = 1: per column the same
// tree, bit-identical results.
template <int V, int LEVEL>
__global__ __launch_bounds__(256) void reduce_batch_kernel(BatchArgs a) {
  __shared__ cols_t<V> red[4][64];
  const int s = batch_find(a, blockIdx.x);
  const XpReduceSeg sg = a.seg[s];
  const bool direct = sg.nrows <= RB_DIRECT;
  const int nsum = (sg.nrows + 31) / 32;
  const int c = (blockIdx.x - a.cb0[s]) * (64 * V) + (threadIdx.x & 63) * V;
  const bool ok = c < sg.width;
  if constexpr (LEVEL == 1) {
    const int r0 = blockIdx.y * nsum;
    if (direct || r0 >= sg.nrows) return;
    const int r1 = r0 + nsum < sg.nrows ? r0 + nsum : sg.nrows;
    const cols_t<V> t = tree_a<V>(sg.in, sg.stride, r0, r1, c, ok, red);
    if (threadIdx.x < 64 && ok) store_cols<V>(a.part2[s] + (int64_t)blockIdx.y * sg.width + c, t);
  } else {
    const int n2 = direct ? sg.nrows : (sg.nrows + nsum - 1) / nsum;
    const cols_t<V> t = tree_a<V>(direct ? sg.in : a.part2[s], direct ? sg.stride : (int64_t)sg.width, 0, n2, c, ok, red);
    if (threadIdx.x < 64 && ok) store_cols<V>(sg.out + c, sg.accumulate ? load_cols<V>(sg.out + c) + t : t);
  }
}

}  // namespace

void xp_launch_rows_reduce(const float* in, float* out, int nrows, int nsum, int width, int accumulate, hipStream_t st) {
  rows_reduce_kernel<<<dim3((unsigned)cdiv(width, 64), (unsigned)cdiv(nrows, nsum)), 256, 0, st>>>(in, out, nrows, nsum, width, accumulate);
}

extern "C" int xp_splitk_reduce(const float* slabs, float* out, int64_t n, int32_t splits, int32_t accumulate,
                                void* stream) {
  XP_REQUIRE(slabs && out && n > 0 && n % 4 == 0 && splits >= 1, "xp_splitk_reduce: bad arguments");
  XP_REQUIRE_ALIGNED("xp_splitk_reduce", 16, XP_P(slabs), XP_P(out));
  const int64_t n4 = n / 4;
  int blocks = (int)(cdiv(n4, 256) < 8192 ? cdiv(n4, 256) : 8192);
  splitk_reduce_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(slabs, out, n4, splits, accumulate);
  XP_CHECK_LAUNCH("xp_splitk_reduce");
  return XP_OK;
}

extern "C" int64_t xp_colsum_partial_rows(int64_t rows, int64_t cols) { return cdiv(rows, cs_rows(rows, cols)); }

extern "C" int xp_colsum_partials(const void* X, int64_t rows, int64_t cols, int64_t ldx, int32_t dtype, float* partials,
                                  size_t partials_bytes, void* stream) {
  XP_REQUIRE(X && partials && rows > 0 && cols > 0 && cols % 4 == 0 && ldx % 4 == 0, "xp_colsum_partials: bad arguments");
  XP_REQUIRE_ALIGNED("xp_colsum_partials", 16, XP_P(X), XP_P(partials));
  const int csr = cs_rows(rows, cols), chunks = (int)cdiv(rows, csr);
  XP_REQUIRE(partials_bytes >= (size_t)chunks * cols * sizeof(float), "xp_colsum_partials: partials buffer too small");
  dim3 grid((unsigned)cdiv(cols, 256), chunks);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == XP_BF16) colsum_partial_kernel<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)X, rows, cols, ldx, partials, csr);
  else if (dtype == XP_F32) colsum_partial_kernel<float><<<grid, 256, 0, st>>>((const float*)X, rows, cols, ldx, partials, csr);
  else XP_REQUIRE(false, "xp_colsum_partials: bad dtype %d", dtype);
  XP_CHECK_LAUNCH("xp_colsum_partials");
  return XP_OK;
}

extern "C" size_t xp_colsum_workspace_bytes(int64_t rows, int64_t cols) {
  return (size_t)((cdiv(rows, 32) + 32) * cols * sizeof(float));
}

extern "C" int xp_colsum(const void* X, int64_t rows, int64_t cols, int64_t ldx, int32_t dtype, float* out,
                         int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream) {
  XP_REQUIRE(X && out && rows > 0 && cols > 0 && cols % 4 == 0 && ldx % 4 == 0, "xp_colsum: bad arguments");
  XP_REQUIRE_ALIGNED("xp_colsum", 16, XP_P(X), XP_P(out), XP_P(workspace));
  XP_REQUIRE(workspace && workspace_bytes >= xp_colsum_workspace_bytes(rows, cols), "xp_colsum: workspace too small");
  const int csr = cs_rows(rows, cols), chunks = (int)cdiv(rows, csr);
  dim3 grid((unsigned)cdiv(cols, 256), chunks);
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)workspace;
  if (dtype == XP_BF16) colsum_partial_kernel<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)X, rows, cols, ldx, part, csr);
  else                  colsum_partial_kernel<float><<<grid, 256, 0, st>>>((const float*)X, rows, cols, ldx, part, csr);
  XP_CHECK_LAUNCH("xp_colsum(partial)");
  // two-level deterministic reduce of the chunk partials (chunks -> <=32 -> 1): no thread walks hundreds of rows.  Its own
  // partition, not the batch path's (head comment)
  const int lvl = (int)cdiv(chunks, 32), n2 = (int)cdiv(chunks, lvl);
  float* part2 = part + (int64_t)chunks * cols;
  xp_launch_rows_reduce(part, part2, chunks, lvl, (int)cols, 0, st);
  XP_CHECK_LAUNCH("xp_colsum(reduce1)");
  xp_launch_rows_reduce(part2, out, n2, n2, (int)cols, accumulate, st);
  XP_CHECK_LAUNCH("xp_colsum(reduce2)");
  return XP_OK;
}

extern "C" size_t xp_reduce_rows_batch_workspace_bytes(const XpReduceSeg* segs_host, int32_t n) {
  size_t b = 0;
  for (int i = 0; segs_host && i < n; ++i) b += (size_t)32 * (size_t)(segs_host[i].width > 0 ? segs_host[i].width : 0) * sizeof(float);
  return b + 16;
}

extern "C" int xp_reduce_rows_batch(const XpReduceSeg* segs_host, int32_t n, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  XP_REQUIRE(segs_host && n > 0 && n <= XP_REDUCE_MAX_SEGS, "xp_reduce_rows_batch: n=%d not in 1..%d", n, XP_REDUCE_MAX_SEGS);
  XP_REQUIRE(workspace && workspace_bytes >= xp_reduce_rows_batch_workspace_bytes(segs_host, n), "xp_reduce_rows_batch: workspace too small");
  BatchArgs a;
  a.n = n;
  float* ws = (float*)workspace;
  // (alignment class `any` for workspace, in and out: reduce_batch_kernel<1, .> moves one float per lane and access)
  // four columns per lane when every segment allows 16-byte accesses (widths, pitches and addresses multiples of 4 floats: every
  // segment the encoder layers pass); XPRETRAIN_DEBUG=rows_reduce_scalar keeps the one-column kernels (bit-identity test)
  bool vec = ((uintptr_t)workspace & 15) == 0 && !xp_debug_flag("rows_reduce_scalar");
  for (int i = 0; i < n && vec; ++i) {
    const XpReduceSeg& sg = segs_host[i];
    vec = sg.width % 4 == 0 && sg.stride % 4 == 0 && ((uintptr_t)sg.in & 15) == 0 && ((uintptr_t)sg.out & 15) == 0;
  }
  const int cw = vec ? 256 : 64;
  int cb = 0;
  bool any_l1 = false;
  for (int i = 0; i < n; ++i) {
    const XpReduceSeg& sg = segs_host[i];
    XP_REQUIRE(sg.in && sg.out && sg.nrows > 0 && sg.width > 0 && sg.stride >= sg.width, "xp_reduce_rows_batch: bad segment %d", i);
    a.seg[i] = sg; a.part2[i] = ws; a.cb0[i] = cb;
    ws += (size_t)32 * sg.width;
    cb += (int)cdiv(sg.width, cw);
    any_l1 = any_l1 || sg.nrows > RB_DIRECT;
  }
  for (int i = n; i <= XP_REDUCE_MAX_SEGS; ++i) a.cb0[i] = cb;
  hipStream_t st = (hipStream_t)stream;
  if (any_l1) {
    if (vec) reduce_batch_kernel<4, 1><<<dim3((unsigned)cb, 32), 256, 0, st>>>(a);
    else     reduce_batch_kernel<1, 1><<<dim3((unsigned)cb, 32), 256, 0, st>>>(a);
    XP_CHECK_LAUNCH("xp_reduce_rows_batch(level 1)");
  }
  if (vec) reduce_batch_kernel<4, 2><<<(unsigned)cb, 256, 0, st>>>(a);
  else     reduce_batch_kernel<1, 2><<<(unsigned)cb, 256, 0, st>>>(a);
  XP_CHECK_LAUNCH("xp_reduce_rows_batch(level 2)");
  return XP_OK;
}
