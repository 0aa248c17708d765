// CLIPTextEmbeddings.forward with caller-given position_ids (reference: modeling/CLIP_ViP.py:210-227, position_embedding(position_ids)):
// xp_text_embed_fwd_pos / xp_text_embed_bwd_pos.  The default map (position t for column t) stays with xp_text_embed_fwd / _bwd in
// embed.hip, whose kernels are not touched; what is shared with them is restated here on purpose (their bits are pinned by their own
// tests).
//
// pos_ids is int64 [pos_B, Lt], pos_B 1 (one map for every sample) or B (a map per sample): row r = b * Lt + t reads entry
// r % (pos_B * Lt).  An id outside [0, n_pos) is decided on the device, per row, without a host synchronisation: the forward reads
// no table row for it and writes NaN into the whole output row; the backward skips the row (it adds to nothing and writes nowhere).
//
// Forward: the flat map of text_embed_fwd_kernel -- a thread owns one float4 of one row, one fp32 add, one rounding to T.
// Backward: both table gradients by the first-occurrence-owns-the-row scheme of text_embed_bwd_tok_kernel: one workgroup per row r;
// only the FIRST row that holds a key works, and adds the dx rows of all the key's occurrences in row order, found 256 rows at a
// time (one compare per thread, a ballot per wave, every thread walks the set bits of the four masks in order).  No atomics, one
// summation order: bit-reproducible.  Rows of the table that no key names are cleared (accumulate == 0: one hipMemsetAsync of the
// whole table in front) or left alone (accumulate != 0).
#include "common.h"

namespace {

constexpr int TPB = 256;
inline int grid_for(int64_t work) { int64_t b = cdiv(work, TPB); return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b)); }

__device__ __forceinline__ bool in_table(int64_t id, int64_t n) { return (uint64_t)id < (uint64_t)n; }

template <typename T>
__global__ void text_embed_fwd_pos_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ pos_ids, int64_t pos_rows,
                                          const float* __restrict__ tok, const float* __restrict__ pos, T* __restrict__ x,
                                          int64_t rows, int D, int64_t n_pos) {
  const int D4 = D / 4;
  const int64_t total = rows * D4;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int d = (int)(idx % D4) * 4;
    const int64_t r = idx / D4;
    const int64_t p = pos_ids[r % pos_rows];
    const float nan = __builtin_nanf("");
    f32x4 v = {nan, nan, nan, nan};
    if (in_table(p, n_pos)) v = load4(tok + ids[r] * D + d) + load4(pos + p * D + d);
    store4(x + r * D + d, v);
  }
}

// table[key] (+)= sum of dx[r] over the rows r whose key it is, in row order.  The key of row q is keys[q % key_rows]; CHECKED: a
// key outside [0, n_keys) belongs to no table row (the position table); otherwise keys are trusted, as xp_text_embed_bwd trusts ids.
template <typename T, bool CHECKED>
__global__ __launch_bounds__(256) void embed_bwd_rows_kernel(const int64_t* __restrict__ keys, int64_t key_rows, int64_t n_keys,
                                                             const T* __restrict__ dx, float* table, int64_t rows, int D, int acc) {
  __shared__ unsigned long long masks[4];
  const int64_t r = blockIdx.x, id = keys[r % key_rows];
  if (CHECKED && !in_table(id, n_keys)) return;                // block-uniform
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int earlier = 0;
  for (int64_t q = threadIdx.x; q < r; q += 256) earlier |= keys[q % key_rows] == id;
  if (__syncthreads_or(earlier)) return;                       // block-uniform
  const int D4 = D / 4;
  for (int d40 = 0; d40 < D4; d40 += 256) {
    const int d = (d40 + threadIdx.x) * 4;
    const bool ok = d < D;
    f32x4 s = ok ? load4(dx + r * D + d) : f32x4{0, 0, 0, 0};
    for (int64_t base = r + 1; base < rows; base += 256) {
      const int64_t q = base + threadIdx.x;
      const unsigned long long m = __ballot(q < rows && keys[q % key_rows] == id);
      __syncthreads();                                          // previous chunk's masks are consumed
      if (lane == 0) masks[wave] = m;
      __syncthreads();
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        unsigned long long mm = masks[w];
        while (mm) {
          const int j = __builtin_ctzll(mm);
          mm &= mm - 1;
          if (ok) s += load4(dx + (base + w * 64 + j) * D + d);
        }
      }
    }
    if (ok) {
      float* o = table + id * D + d;
      if (acc) s += load4(o);
      store4(o, s);
    }
  }
}

// everything both entries refuse, before any launch
int check_args(const char* fn, bool pointers, int64_t pos_B, int64_t B, int64_t Lt, int64_t D, int64_t vocab, int64_t n_pos, int32_t dtype) {
  XP_REQUIRE(pointers, "%s: null pointer", fn);
  XP_REQUIRE(B > 0 && Lt > 0 && vocab > 0, "%s: bad sizes (B=%lld Lt=%lld vocab=%lld)", fn, (long long)B, (long long)Lt, (long long)vocab);
  XP_REQUIRE(pos_B == 1 || pos_B == B, "%s: pos_B=%lld is neither 1 nor B=%lld", fn, (long long)pos_B, (long long)B);
  XP_REQUIRE(D >= 4 && D % 4 == 0, "%s: D=%lld is not a positive multiple of 4 (rows are read as float4)", fn, (long long)D);
  XP_REQUIRE(n_pos >= 1, "%s: n_pos=%lld: the position table is empty", fn, (long long)n_pos);
  XP_REQUIRE(B * Lt <= INT32_MAX, "%s: %lld rows exceed one launch", fn, (long long)(B * Lt));
  XP_REQUIRE(dtype == XP_BF16 || dtype == XP_F32, "%s: bad dtype %d", fn, (int)dtype);
  return XP_OK;
}

}  // namespace

extern "C" int xp_text_embed_fwd_pos(const int64_t* ids, const int64_t* pos_ids, int64_t pos_B, const float* tok, const float* pos,
                                     void* x, int64_t B, int64_t Lt, int64_t D, int64_t vocab, int64_t n_pos, int32_t dtype,
                                     void* stream) {
  if (int rc = check_args("xp_text_embed_fwd_pos", ids && pos_ids && tok && pos && x, pos_B, B, Lt, D, vocab, n_pos, dtype)) return rc;
  XP_REQUIRE_ALIGNED("xp_text_embed_fwd_pos", 16, XP_P(ids), XP_P(pos_ids), XP_P(tok), XP_P(pos), XP_P(x));
  hipStream_t st = (hipStream_t)stream;
  const int g = grid_for(B * Lt * D / 4);
  if (dtype == XP_BF16)
    text_embed_fwd_pos_kernel<bf16_t><<<g, TPB, 0, st>>>(ids, pos_ids, pos_B * Lt, tok, pos, (bf16_t*)x, B * Lt, (int)D, n_pos);
  else
    text_embed_fwd_pos_kernel<float><<<g, TPB, 0, st>>>(ids, pos_ids, pos_B * Lt, tok, pos, (float*)x, B * Lt, (int)D, n_pos);
  XP_CHECK_LAUNCH("xp_text_embed_fwd_pos");
  return XP_OK;
}

extern "C" int xp_text_embed_bwd_pos(const int64_t* ids, const int64_t* pos_ids, int64_t pos_B, const void* dx, float* d_tok,
                                     float* d_pos, int64_t B, int64_t Lt, int64_t D, int64_t vocab, int64_t n_pos, int32_t dtype,
                                     int32_t accumulate, void* stream) {
  if (int rc = check_args("xp_text_embed_bwd_pos", ids && pos_ids && dx && d_tok && d_pos, pos_B, B, Lt, D, vocab, n_pos, dtype)) return rc;
  XP_REQUIRE_ALIGNED("xp_text_embed_bwd_pos", 16, XP_P(ids), XP_P(pos_ids), XP_P(dx), XP_P(d_tok), XP_P(d_pos));
  hipStream_t st = (hipStream_t)stream;
  if (!accumulate) {
    hipError_t e = hipMemsetAsync(d_tok, 0, (size_t)vocab * D * sizeof(float), st);
    if (e == hipSuccess) e = hipMemsetAsync(d_pos, 0, (size_t)n_pos * D * sizeof(float), st);
    XP_REQUIRE(e == hipSuccess, "xp_text_embed_bwd_pos: memset failed: %s", hipGetErrorString(e));
  }
  const int64_t rows = B * Lt;
  const unsigned g = (unsigned)rows;               // one workgroup per row (fixed-order sums, no atomics)
  if (dtype == XP_BF16) {
    embed_bwd_rows_kernel<bf16_t, false><<<g, 256, 0, st>>>(ids, rows, vocab, (const bf16_t*)dx, d_tok, rows, (int)D, accumulate);
    embed_bwd_rows_kernel<bf16_t, true><<<g, 256, 0, st>>>(pos_ids, pos_B * Lt, n_pos, (const bf16_t*)dx, d_pos, rows, (int)D, accumulate);
  } else {
    embed_bwd_rows_kernel<float, false><<<g, 256, 0, st>>>(ids, rows, vocab, (const float*)dx, d_tok, rows, (int)D, accumulate);
    embed_bwd_rows_kernel<float, true><<<g, 256, 0, st>>>(pos_ids, pos_B * Lt, n_pos, (const float*)dx, d_pos, rows, (int)D, accumulate);
  }
  XP_CHECK_LAUNCH("xp_text_embed_bwd_pos");
  return XP_OK;
}
