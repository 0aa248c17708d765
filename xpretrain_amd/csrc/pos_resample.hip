// The vision tower's position table [1 + g0*g0, D] fp32 resampled to a patch grid gh x gw it was not trained for, and the transpose
// of that map for the gradient (xp_pos_resample_fwd / xp_pos_resample_bwd; the arithmetic is stated in include/xpretrain_hip.h and,
// in fp64, in tests/pos_resample_ref.py).  transformers' CLIPVisionEmbeddings.interpolate_pos_encoding: row 0 (the class position)
// is copied, rows 1.. are F.interpolate(mode="bicubic", align_corners=False) of the g0 x g0 grid of D-vectors.
//
// Both kernels are flat maps over (row, group of 4 columns): a thread owns one float4 of one row, consecutive lanes consecutive
// column groups, so a wave reads and writes whole 256-byte .. 1 KiB row segments.  The tables are small (14 -> 28 x 28 at D = 768:
// 0.6 MB in, 2.4 MB out) and the launch runs once per forward / backward: nothing is staged or tuned.
//
// The tap arithmetic is csrc/frames.hip's cubic_axis without the source box (a second copy on purpose: frames.hip's bits are pinned
// by its tests): floor and fraction of ((2 d + 1) g0 - g) / (2 g) from integer division, t = rem / den ONE correctly
// rounded fp32 division, the Keys weights (A = -0.75) in the factored forms that are exactly 0 / 1 at t = 0.
//
// Forward: the four row sums first, then their combination, fixed order.  Backward: a GATHER -- the thread of source row (sy, sx)
// walks the destination rows y ascending, x ascending, and adds (Wy[y,sy] Wx[x,sx]) d_out[1 + y gw + x], where Wy[y,sy] is the sum
// (taps ascending) of row y's tap weights whose clamped index is sy; zero weights are skipped.  No atomics, one thread per output
// element, one summation order: bit-reproducible.
#include "common.h"

namespace {

constexpr float KEYS_A = -0.75f;
constexpr int THREADS = 256;
constexpr int MAX_GRID = 16384;               // g0, gh, gw: keeps (2 d + 1) * g0 inside int32 and 2 g below 2^24

// d: coordinate in the resampled axis of length `out` over a source axis of length `in`
__device__ __forceinline__ void cubic_axis(int d, int in, int out, int (&tap)[4], float (&w)[4]) {
  const int num = (2 * d + 1) * in - out, den = 2 * out;
  int i = num / den, rem = num - i * den;
  if (rem < 0) { rem += den; --i; }          // C division truncates: make it a floor
  const float t = (float)rem / (float)den, s = (float)(den - rem) / (float)den;
  w[0] = KEYS_A * t * (s * s);
  w[1] = ((KEYS_A + 2.0f) * t - (KEYS_A + 3.0f)) * (t * t) + 1.0f;
  w[2] = ((KEYS_A + 2.0f) * s - (KEYS_A + 3.0f)) * (s * s) + 1.0f;
  w[3] = KEYS_A * s * (t * t);
#pragma unroll
  for (int k = 0; k < 4; ++k) tap[k] = min(max(i - 1 + k, 0), in - 1);
}

// W[d, src]: the sum, taps ascending, of coordinate d's tap weights whose clamped index is `src` (0 where none is)
__device__ __forceinline__ float axis_weight(int d, int in, int out, int src) {
  int tap[4];
  float w[4];
  cubic_axis(d, in, out, tap, w);
  float sum = 0.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (tap[k] == src) sum += w[k];
  return sum;
}

__device__ __forceinline__ f32x4 fma4(float w, f32x4 v, f32x4 acc) {
  return f32x4{fmaf(w, v[0], acc[0]), fmaf(w, v[1], acc[1]), fmaf(w, v[2], acc[2]), fmaf(w, v[3], acc[3])};
}
__device__ __forceinline__ f32x4 mul4(float w, f32x4 v) { return f32x4{w * v[0], w * v[1], w * v[2], w * v[3]}; }

XP_NO_PK_F32 __global__ __launch_bounds__(THREADS) void pos_resample_fwd_kernel(const float* __restrict__ pos, float* __restrict__ out,
                                                                               int g0, int gh, int gw, int D4, int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= total) return;
  const int row = (int)(idx / D4), c = (int)(idx - (int64_t)row * D4) * 4;
  const int64_t D = 4 * (int64_t)D4;
  if (row == 0) {
    store4(out + c, load4(pos + c));
    return;
  }
  const int y = (row - 1) / gw, x = (row - 1) - y * gw;
  int ty[4], tx[4];
  float wy[4], wx[4];
  cubic_axis(y, g0, gh, ty, wy);
  cubic_axis(x, g0, gw, tx, wx);
  f32x4 h[4];                                  // the four row sums
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float* const r = pos + (1 + (int64_t)ty[j] * g0) * D + c;
    h[j] = fma4(wx[3], load4(r + tx[3] * D), fma4(wx[2], load4(r + tx[2] * D), fma4(wx[1], load4(r + tx[1] * D), mul4(wx[0], load4(r + tx[0] * D)))));
  }
  store4(out + row * D + c, fma4(wy[3], h[3], fma4(wy[2], h[2], fma4(wy[1], h[1], mul4(wy[0], h[0])))));
}

XP_NO_PK_F32 __global__ __launch_bounds__(THREADS) void pos_resample_bwd_kernel(const float* __restrict__ d_out, float* __restrict__ d_pos,
                                                                               int g0, int gh, int gw, int D4, int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= total) return;
  const int row = (int)(idx / D4), c = (int)(idx - (int64_t)row * D4) * 4;
  const int64_t D = 4 * (int64_t)D4;
  if (row == 0) {
    store4(d_pos + c, load4(d_out + c));
    return;
  }
  const int sy = (row - 1) / g0, sx = (row - 1) - sy * g0;
  f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int y = 0; y < gh; ++y) {
    const float wy = axis_weight(y, g0, gh, sy);
    if (wy == 0.0f) continue;
    const float* const r = d_out + (1 + (int64_t)y * gw) * D + c;
    for (int x = 0; x < gw; ++x) {
      const float wx = axis_weight(x, g0, gw, sx);
      if (wx == 0.0f) continue;
      acc = fma4(wy * wx, load4(r + x * D), acc);
    }
  }
  store4(d_pos + row * D + c, acc);
}

int check_args(const char* fn, const void* in, const char* in_name, const void* out, const char* out_name, int g0, int gh, int gw,
               int D, int64_t rows, unsigned* blocks, int64_t* total) {
  XP_REQUIRE(in, "%s: %s is null", fn, in_name);
  XP_REQUIRE(out, "%s: %s is null", fn, out_name);
  if (int rc = xp_check_aligned(fn, 16, {XpPtrName{in_name, in}, XpPtrName{out_name, out}})) return rc;      // float4 rows
  XP_REQUIRE(g0 >= 1 && g0 <= MAX_GRID, "%s: g0=%d not in 1..%d", fn, g0, MAX_GRID);
  XP_REQUIRE(gh >= 1 && gh <= MAX_GRID, "%s: gh=%d not in 1..%d", fn, gh, MAX_GRID);
  XP_REQUIRE(gw >= 1 && gw <= MAX_GRID, "%s: gw=%d not in 1..%d", fn, gw, MAX_GRID);
  XP_REQUIRE(D >= 4 && D % 4 == 0, "%s: D=%d is not a positive multiple of 4 (rows are read as float4)", fn, D);
  *total = rows * (D / 4);
  const int64_t nb = cdiv(*total, THREADS);
  XP_REQUIRE(nb <= INT32_MAX, "%s: %lld rows of %d columns exceed one launch", fn, (long long)rows, D);
  *blocks = (unsigned)nb;
  return XP_OK;
}

}  // namespace

extern "C" int xp_pos_resample_fwd(const float* pos, float* out, int32_t g0, int32_t gh, int32_t gw, int32_t D, void* stream) {
  unsigned blocks;
  int64_t total;
  if (int rc = check_args("xp_pos_resample_fwd", pos, "pos", out, "out", g0, gh, gw, D, 1 + (int64_t)gh * gw, &blocks, &total)) return rc;
  pos_resample_fwd_kernel<<<blocks, THREADS, 0, (hipStream_t)stream>>>(pos, out, g0, gh, gw, D / 4, total);
  XP_CHECK_LAUNCH("xp_pos_resample_fwd");
  return XP_OK;
}

extern "C" int xp_pos_resample_bwd(const float* d_out, float* d_pos, int32_t g0, int32_t gh, int32_t gw, int32_t D, void* stream) {
  unsigned blocks;
  int64_t total;
  if (int rc = check_args("xp_pos_resample_bwd", d_out, "d_out", d_pos, "d_pos", g0, gh, gw, D, 1 + (int64_t)g0 * g0, &blocks, &total))
    return rc;
  pos_resample_bwd_kernel<<<blocks, THREADS, 0, (hipStream_t)stream>>>(d_out, d_pos, g0, gh, gw, D / 4, total);
  XP_CHECK_LAUNCH("xp_pos_resample_bwd");
  return XP_OK;
}
