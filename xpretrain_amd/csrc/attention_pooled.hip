// Single-query proxy attention: the pooled last layer of the video tower (modeling/CLIP_ViP.py: pooled_output =
// last_hidden_state[:, 0]; CLIPAttention.forward2 in XP_ATTN_PROXY mode, where a proxy query attends all S = M + N*L keys).
// Only query row b*S + 0 of each sample reaches the contrastive loss, so the last layer's attention is B*H problems of ONE
// query against S keys: a decode-shaped, memory-bound pass over K and V, for which the MFMA kernels of attention.hip (112-row
// query tiles) are the wrong tool.
//
//   layout   q[B, H*64] (already scaled); kv = the packed K/V projection output [B, S, 2, H, 64] with a row stride (ldkv
//            elements per token); out[B, H*64]; stats[B, H, 2] = (row max, log row sum) as xp_attn_fwd writes them.
//   grid     one 4-wave workgroup per (b, h, chunk of keys); the planner cuts S into chunks so that B*H*chunks fills the chip.
//   wave     streams its keys straight into registers with 16-byte loads -- no LDS round trip for an operand nobody shares:
//            a key row (64 elements) is spread over 8 lanes (bf16) / 16 lanes (fp32), so one load instruction of a wave
//            fetches 8 / 4 whole rows; the row's score is finished with 3 / 4 lane exchanges.  Every group of lanes keeps its
//            own online softmax (m, l, acc) in fp32 over the keys it sees; groups, waves and finally chunks are merged in a
//            FIXED order (lane butterflies, then wave 0..3, then chunk 0..n-1 in the combine kernel).  No atomics, no
//            arrival-order dependence: the result is bit-identical run to run.
//   backward one pass over K/V, one write of dkv: p_j = exp(q.k_j - lse), dV_j = p_j dO, dS_j = p_j (dO.v_j - dO.O),
//            dK_j = dS_j q, dq = sum_j dS_j k_j (per-chunk partial rows, summed in chunk order by the combine kernel and
//            multiplied by q_scale as xp_attn_bwd defines dq).  The column sums of the dkv rows AS STORED (rounded) are left
//            as one partial row per (b, chunk) for the k/v bias gradients (finish with xp_reduce_rows_batch), the way
//            xp_attn_bwd2 does.
//   dtypes   bf16 storage or fp32 (a template parameter on the load / store type); the arithmetic is fp32 VALU either way.
//
// head_dim is fixed at 64 like the rest of the attention ABI.  Padding masks and XP_ATTN_CAUSAL are out of scope: the text
// tower pools at a per-sample EOS index and costs 0.6 % of the step's FLOPs.
#include "common.h"
#include <math.h>

namespace {

constexpr int DH = 64;
constexpr int PW = 4;                 // waves per workgroup
constexpr int UNROLL = 4;             // key steps in flight per wave (K and V: 8 16-byte loads per lane)
constexpr int CHUNK_ALIGN = 32;       // chunk lengths are multiples of the keys one workgroup step covers (bf16: 4 waves x 8 keys)
constexpr int MIN_CHUNK_KEYS = 64;    // never cut finer than this
constexpr int MAX_CHUNKS = 64;
constexpr int WGS_PER_CU = 2;         // workgroups the planner aims to keep on every CU

template <typename T> struct Geo;
template <> struct Geo<bf16_t> { typedef bf16x8 raw; static constexpr int EPL = 8; };     // elements per lane = one 16-byte load
template <> struct Geo<float>  { typedef f32x4 raw;  static constexpr int EPL = 4; };

__device__ __forceinline__ void cvt(const bf16x8& v, float* r) {
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = (float)v[e];
}
__device__ __forceinline__ void cvt(const f32x4& v, float* r) {
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] = v[e];
}
__device__ __forceinline__ void st_seg(bf16_t* p, const float* r) {
  bf16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (bf16_t)r[e];
  *reinterpret_cast<bf16x8*>(p) = o;
}
__device__ __forceinline__ void st_seg(float* p, const float* r) { *reinterpret_cast<f32x4*>(p) = f32x4{r[0], r[1], r[2], r[3]}; }
// what a stored value reads back as (the column sums are those of the stored rows)
__device__ __forceinline__ float stored(bf16_t, float x) { return (float)(bf16_t)x; }
__device__ __forceinline__ float stored(float, float x) { return x; }

struct PP {
  const void* q; const void* kv; int64_t ldkv;
  void* out; float* stats;
  const void* dout; void* dq; int64_t lddq; void* dkv; int64_t lddkv; float* cs; float q_scale;
  float* ws_ml; float* ws_acc; float* ws_dq;
  int B, H, S, chunks, chunk_keys;
};

// sum over the LPR lanes that share a key row (lanes differing in the low bits)
template <int LPR> __device__ __forceinline__ float row_sum(float v) {
#pragma unroll
  for (int o = LPR >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// sum over the key slots of a wave (lanes differing in the high bits): same order in every run
template <int LPR> __device__ __forceinline__ float slot_sum(float v) {
#pragma unroll
  for (int o = LPR; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// weight of a partial softmax with maximum m in a merge whose maximum is mm (an empty partial has m = -inf)
__device__ __forceinline__ float merge_w(float m, float mm) { return m == -INFINITY ? 0.f : __expf(m - mm); }

template <typename T>
__global__ __launch_bounds__(PW * 64) XP_NO_PK_F32 void attn_pooled_fwd_kernel(PP p) {
  typedef typename Geo<T>::raw raw;
  constexpr int EPL = Geo<T>::EPL, LPR = DH / EPL, KPW = 64 / LPR;
  __shared__ float sm[PW][2 + DH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x % p.chunks, bh = blockIdx.x / p.chunks, h = bh % p.H, b = bh / p.H;
  const int seg = (lane % LPR) * EPL, slot = lane / LPR;
  const int k0 = c * p.chunk_keys, k1 = min(p.S, k0 + p.chunk_keys);
  float q[EPL];
  cvt(*reinterpret_cast<const raw*>(reinterpret_cast<const T*>(p.q) + (int64_t)bh * DH + seg), q);
  const T* kbase = reinterpret_cast<const T*>(p.kv) + (int64_t)b * p.S * p.ldkv + h * DH + seg;
  const int64_t voff = (int64_t)p.H * DH;
  float m = -INFINITY, l = 0.f, acc[EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) acc[e] = 0.f;
  for (int jb = k0; jb < k1; jb += UNROLL * PW * KPW) {
    raw rk[UNROLL], rv[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {                // loads of past-the-end keys are redirected to the chunk's last key
      const int j = min(jb + (u * PW + wave) * KPW + slot, k1 - 1);
      const T* row = kbase + (int64_t)j * p.ldkv;
      rk[u] = *reinterpret_cast<const raw*>(row);
      rv[u] = *reinterpret_cast<const raw*>(row + voff);
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const bool valid = jb + (u * PW + wave) * KPW + slot < k1;
      float k[EPL], v[EPL], s = 0.f;
      cvt(rk[u], k); cvt(rv[u], v);
#pragma unroll
      for (int e = 0; e < EPL; ++e) s = fmaf(q[e], k[e], s);
      s = row_sum<LPR>(s);
      if (valid) {
        const float mnew = fmaxf(m, s);
        const float alpha = __expf(m - mnew);         // m = -inf at the first key -> 0
        const float pj = __expf(s - mnew);
        l = fmaf(l, alpha, pj);
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc[e] = fmaf(acc[e], alpha, pj * v[e]);
        m = mnew;
      }
    }
  }
  // merge the key slots of the wave (butterfly over the high lane bits) ...
#pragma unroll
  for (int o = LPR; o < 64; o <<= 1) {
    const float m2 = __shfl_xor(m, o, 64), l2 = __shfl_xor(l, o, 64);
    const float mm = fmaxf(m, m2);
    const float w1 = merge_w(m, mm), w2 = merge_w(m2, mm);
    l = l * w1 + l2 * w2;
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[e] = acc[e] * w1 + __shfl_xor(acc[e], o, 64) * w2;
    m = mm;
  }
  // ... then the waves, in wave order
  if (slot == 0) {
    if (lane == 0) { sm[wave][0] = m; sm[wave][1] = l; }
#pragma unroll
    for (int e = 0; e < EPL; ++e) sm[wave][2 + seg + e] = acc[e];
  }
  __syncthreads();
  if (wave == 0) {
    float mm = sm[0][0];
#pragma unroll
    for (int w = 1; w < PW; ++w) mm = fmaxf(mm, sm[w][0]);
    float ls = 0.f, a = 0.f;
#pragma unroll
    for (int w = 0; w < PW; ++w) {
      const float wt = merge_w(sm[w][0], mm);
      ls = fmaf(sm[w][1], wt, ls);
      a = fmaf(sm[w][2 + lane], wt, a);
    }
    p.ws_acc[(int64_t)blockIdx.x * DH + lane] = a;
    if (lane < 2) p.ws_ml[(int64_t)blockIdx.x * 2 + lane] = lane ? ls : mm;
  }
}

// out[b, h*64 + d] and stats from the chunk partials, in chunk order.  One wave per (b, h).
template <typename T>
__global__ __launch_bounds__(64) XP_NO_PK_F32 void attn_pooled_fwd_combine_kernel(PP p) {
  const int lane = threadIdx.x, bh = blockIdx.x;
  const float* ml = p.ws_ml + (int64_t)bh * p.chunks * 2;
  const float* acc = p.ws_acc + (int64_t)bh * p.chunks * DH;
  float mm = ml[0];
  for (int c = 1; c < p.chunks; ++c) mm = fmaxf(mm, ml[c * 2]);
  float ls = 0.f, a = 0.f;
  for (int c = 0; c < p.chunks; ++c) {
    const float wt = merge_w(ml[c * 2], mm);
    ls = fmaf(ml[c * 2 + 1], wt, ls);
    a = fmaf(acc[c * DH + lane], wt, a);
  }
  reinterpret_cast<T*>(p.out)[(int64_t)bh * DH + lane] = from_f<T>(a / ls);
  if (lane < 2) p.stats[(int64_t)bh * 2 + lane] = lane ? __logf(ls) : mm;
}

template <typename T>
__global__ __launch_bounds__(PW * 64) XP_NO_PK_F32 void attn_pooled_bwd_kernel(PP p) {
  typedef typename Geo<T>::raw raw;
  constexpr int EPL = Geo<T>::EPL, LPR = DH / EPL, KPW = 64 / LPR;
  __shared__ float sm[PW][3][DH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x % p.chunks, bh = blockIdx.x / p.chunks, h = bh % p.H, b = bh / p.H;
  const int seg = (lane % LPR) * EPL, slot = lane / LPR;
  const int k0 = c * p.chunk_keys, k1 = min(p.S, k0 + p.chunk_keys);
  float q[EPL], go[EPL], o[EPL];
  cvt(*reinterpret_cast<const raw*>(reinterpret_cast<const T*>(p.q) + (int64_t)bh * DH + seg), q);
  cvt(*reinterpret_cast<const raw*>(reinterpret_cast<const T*>(p.dout) + (int64_t)bh * DH + seg), go);
  cvt(*reinterpret_cast<const raw*>(reinterpret_cast<const T*>(p.out) + (int64_t)bh * DH + seg), o);
  float delta = 0.f;
#pragma unroll
  for (int e = 0; e < EPL; ++e) delta = fmaf(go[e], o[e], delta);
  delta = row_sum<LPR>(delta);
  const float mx = p.stats[(int64_t)bh * 2], lg = p.stats[(int64_t)bh * 2 + 1];
  const T* kbase = reinterpret_cast<const T*>(p.kv) + (int64_t)b * p.S * p.ldkv + h * DH + seg;
  T* dbase = reinterpret_cast<T*>(p.dkv) + (int64_t)b * p.S * p.lddkv + h * DH + seg;
  const int64_t voff = (int64_t)p.H * DH;
  float dq[EPL], csk[EPL], csv[EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) dq[e] = csk[e] = csv[e] = 0.f;
  for (int jb = k0; jb < k1; jb += UNROLL * PW * KPW) {
    raw rk[UNROLL], rv[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int j = min(jb + (u * PW + wave) * KPW + slot, k1 - 1);
      const T* row = kbase + (int64_t)j * p.ldkv;
      rk[u] = *reinterpret_cast<const raw*>(row);
      rv[u] = *reinterpret_cast<const raw*>(row + voff);
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int j = jb + (u * PW + wave) * KPW + slot;
      float k[EPL], v[EPL], s = 0.f, dov = 0.f;
      cvt(rk[u], k); cvt(rv[u], v);
#pragma unroll
      for (int e = 0; e < EPL; ++e) { s = fmaf(q[e], k[e], s); dov = fmaf(go[e], v[e], dov); }
      s = row_sum<LPR>(s);
      dov = row_sum<LPR>(dov);
      if (j < k1) {                                    // (stores of past-the-end keys are skipped: j < k1 <= S)
        const float pj = __expf((s - mx) - lg);
        const float ds = pj * (dov - delta);
        float dk[EPL], dv[EPL];
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          dk[e] = ds * q[e]; dv[e] = pj * go[e];
          dq[e] = fmaf(ds, k[e], dq[e]);
          csk[e] += stored(T(), dk[e]); csv[e] += stored(T(), dv[e]);
        }
        T* row = dbase + (int64_t)j * p.lddkv;
        st_seg(row, dk);
        st_seg(row + voff, dv);
      }
    }
  }
  // key slots of the wave, then the waves in wave order
#pragma unroll
  for (int e = 0; e < EPL; ++e) { dq[e] = slot_sum<LPR>(dq[e]); csk[e] = slot_sum<LPR>(csk[e]); csv[e] = slot_sum<LPR>(csv[e]); }
  if (slot == 0) {
#pragma unroll
    for (int e = 0; e < EPL; ++e) { sm[wave][0][seg + e] = dq[e]; sm[wave][1][seg + e] = csk[e]; sm[wave][2][seg + e] = csv[e]; }
  }
  __syncthreads();
  if (wave == 0) {
    float a = sm[0][0][lane], ck = sm[0][1][lane], cv = sm[0][2][lane];
#pragma unroll
    for (int w = 1; w < PW; ++w) { a += sm[w][0][lane]; ck += sm[w][1][lane]; cv += sm[w][2][lane]; }
    p.ws_dq[(int64_t)blockIdx.x * DH + lane] = a;
    if (p.cs) {                                        // partial row (b, chunk): [k columns of every head | v columns]
      float* row = p.cs + ((int64_t)b * p.chunks + c) * 2 * p.H * DH + h * DH + lane;
      row[0] = ck;
      row[voff] = cv;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(64) XP_NO_PK_F32 void attn_pooled_bwd_combine_kernel(PP p) {
  const int lane = threadIdx.x, bh = blockIdx.x, h = bh % p.H, b = bh / p.H;
  const float* part = p.ws_dq + (int64_t)bh * p.chunks * DH + lane;
  float a = 0.f;
  for (int c = 0; c < p.chunks; ++c) a += part[c * DH];
  reinterpret_cast<T*>(p.dq)[(int64_t)b * p.lddq + h * DH + lane] = from_f<T>(a * p.q_scale);
}

// ============================================================================================ planning
struct Region { int64_t off, bytes; };
struct PooledPlan {
  int chunks, chunk_keys;
  unsigned grid, combine_grid;
  Region ml, acc, dq;
  int64_t ws_bytes, colsum_rows;
};
inline int64_t a256(int64_t n) { return (n + 255) & ~(int64_t)255; }
inline int64_t max_chunks_of(int64_t S) { const int64_t c = cdiv(S, MIN_CHUNK_KEYS); return c < MAX_CHUNKS ? c : MAX_CHUNKS; }

// Chunks: as many as give every CU WGS_PER_CU workgroups, never finer than MIN_CHUNK_KEYS keys, at most MAX_CHUNKS; the chunk
// length is rounded up to CHUNK_ALIGN keys and the count recomputed, so no chunk is empty and only the last one is short.
PooledPlan plan_pooled(int64_t B, int64_t H, int64_t S, bool bwd, int cus) {
  PooledPlan p{};
  const int64_t P = B * H;
  int64_t chunks = cdiv((int64_t)WGS_PER_CU * cus, P);
  const int64_t cap = max_chunks_of(S);
  if (chunks > cap) chunks = cap;
  if (chunks < 1) chunks = 1;
  const int64_t keys = cdiv(cdiv(S, chunks), CHUNK_ALIGN) * CHUNK_ALIGN;
  chunks = cdiv(S, keys);
  p.chunks = (int)chunks; p.chunk_keys = (int)keys;
  p.grid = (unsigned)(P * chunks); p.combine_grid = (unsigned)P;
  if (!bwd) {
    p.ml = {0, P * chunks * 2 * 4};
    p.acc = {a256(p.ml.bytes), P * chunks * DH * 4};
    p.ws_bytes = p.acc.off + p.acc.bytes;
  } else {
    p.dq = {0, P * chunks * DH * 4};
    p.ws_bytes = p.dq.bytes;
  }
  p.colsum_rows = B * chunks;
  return p;
}
int plan_pooled_for(int64_t B, int64_t H, int64_t S, bool bwd, int cus, PooledPlan& p) {
  if (cus <= 0 && !(cus = xp_device_cus())) return XP_ERR_LAUNCH;
  p = plan_pooled(B, H, S, bwd, cus);
  return XP_OK;
}

int check_pooled(const char* name, int64_t B, int64_t H, int64_t S, int64_t ldkv, int32_t dtype) {
  XP_REQUIRE(dtype == XP_BF16 || dtype == XP_F32, "%s: bad dtype %d", name, dtype);
  XP_REQUIRE(B > 0 && H > 0 && S > 0, "%s: empty problem B=%lld H=%lld S=%lld", name, (long long)B, (long long)H, (long long)S);
  XP_REQUIRE(B * H * MAX_CHUNKS < (1LL << 31) && B * S < (1LL << 31) && S < (1LL << 30), "%s: problem too large", name);
  const int epl = dtype == XP_BF16 ? 8 : 4;
  XP_REQUIRE(ldkv >= 2 * H * DH && ldkv % epl == 0, "%s: row stride %lld must be >= 2*H*64 and a multiple of %d", name, (long long)ldkv, epl);
  return XP_OK;
}

}  // namespace

extern "C" size_t xp_attn_pooled_workspace_bytes(int64_t B, int64_t H, int64_t S, int32_t dtype) {
  if (B <= 0 || H <= 0 || S <= 0) return 0;
  // the larger direction at the most chunks any device is planned (the forward: (m, l) and 64 accumulators per chunk)
  const int64_t P = B * H, c = max_chunks_of(S);
  return (size_t)(a256(P * c * 2 * 4) + a256(P * c * DH * 4));
}

extern "C" int64_t xp_attn_pooled_colsum_rows(int64_t B, int64_t H, int64_t S, int32_t dtype) {
  PooledPlan pl;
  if (B <= 0 || H <= 0 || S <= 0 || plan_pooled_for(B, H, S, true, 0, pl)) return 0;
  return pl.colsum_rows;
}

extern "C" int64_t xp_attn_pooled_colsum_rows_max(int64_t B, int64_t S) { return B <= 0 || S <= 0 ? 0 : B * max_chunks_of(S); }

extern "C" int xp_attn_pooled_fwd(const void* q, const void* kv, int64_t ldkv, void* out, float* stats, int64_t B, int64_t H,
                                  int64_t S, int32_t dtype, void* workspace, size_t workspace_bytes, void* stream) {
  XP_REQUIRE(q && kv && out && stats, "xp_attn_pooled_fwd: null pointer");
  int rc = check_pooled("xp_attn_pooled_fwd", B, H, S, ldkv, dtype);
  if (rc) return rc;
  XP_REQUIRE_ALIGNED("xp_attn_pooled_fwd", 16, XP_P(q), XP_P(kv), XP_P(out), XP_P(stats), XP_P(workspace));
  PooledPlan pl;
  if ((rc = plan_pooled_for(B, H, S, false, 0, pl))) return rc;
  XP_REQUIRE(workspace && workspace_bytes >= (size_t)pl.ws_bytes, "xp_attn_pooled_fwd: workspace too small");
  PP p{};
  p.q = q; p.kv = kv; p.ldkv = ldkv; p.out = out; p.stats = stats;
  p.ws_ml = reinterpret_cast<float*>(static_cast<char*>(workspace) + pl.ml.off);
  p.ws_acc = reinterpret_cast<float*>(static_cast<char*>(workspace) + pl.acc.off);
  p.B = (int)B; p.H = (int)H; p.S = (int)S; p.chunks = pl.chunks; p.chunk_keys = pl.chunk_keys;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == XP_BF16) attn_pooled_fwd_kernel<bf16_t><<<pl.grid, PW * 64, 0, st>>>(p);
  else                  attn_pooled_fwd_kernel<float><<<pl.grid, PW * 64, 0, st>>>(p);
  XP_CHECK_LAUNCH("xp_attn_pooled_fwd");
  if (dtype == XP_BF16) attn_pooled_fwd_combine_kernel<bf16_t><<<pl.combine_grid, 64, 0, st>>>(p);
  else                  attn_pooled_fwd_combine_kernel<float><<<pl.combine_grid, 64, 0, st>>>(p);
  XP_CHECK_LAUNCH("xp_attn_pooled_fwd(combine)");
  return XP_OK;
}

extern "C" int xp_attn_pooled_bwd(const void* q, const void* kv, int64_t ldkv, const void* out, const void* dout,
                                  const float* stats, void* dq, int64_t lddq, void* dkv, int64_t lddkv, float q_scale,
                                  int64_t B, int64_t H, int64_t S, int32_t dtype, void* workspace, size_t workspace_bytes,
                                  float* dkv_colsum_partials, void* stream) {
  XP_REQUIRE(q && kv && out && dout && stats && dq && dkv, "xp_attn_pooled_bwd: null pointer");
  int rc = check_pooled("xp_attn_pooled_bwd", B, H, S, ldkv, dtype);
  if (rc) return rc;
  if ((rc = check_pooled("xp_attn_pooled_bwd(dkv)", B, H, S, lddkv, dtype))) return rc;
  XP_REQUIRE(lddq >= H * DH, "xp_attn_pooled_bwd: dq row stride %lld < H*64", (long long)lddq);
  XP_REQUIRE_ALIGNED("xp_attn_pooled_bwd", 16, XP_P(q), XP_P(kv), XP_P(out), XP_P(dout), XP_P(stats), XP_P(dq), XP_P(dkv), XP_P(workspace),
                     XP_P(dkv_colsum_partials));
  PooledPlan pl;
  if ((rc = plan_pooled_for(B, H, S, true, 0, pl))) return rc;
  XP_REQUIRE(workspace && workspace_bytes >= (size_t)pl.ws_bytes, "xp_attn_pooled_bwd: workspace too small");
  PP p{};
  p.q = q; p.kv = kv; p.ldkv = ldkv; p.out = const_cast<void*>(out); p.stats = const_cast<float*>(stats); p.dout = dout;
  p.dq = dq; p.lddq = lddq; p.dkv = dkv; p.lddkv = lddkv; p.cs = dkv_colsum_partials; p.q_scale = q_scale;
  p.ws_dq = reinterpret_cast<float*>(static_cast<char*>(workspace) + pl.dq.off);
  p.B = (int)B; p.H = (int)H; p.S = (int)S; p.chunks = pl.chunks; p.chunk_keys = pl.chunk_keys;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == XP_BF16) attn_pooled_bwd_kernel<bf16_t><<<pl.grid, PW * 64, 0, st>>>(p);
  else                  attn_pooled_bwd_kernel<float><<<pl.grid, PW * 64, 0, st>>>(p);
  XP_CHECK_LAUNCH("xp_attn_pooled_bwd");
  if (dtype == XP_BF16) attn_pooled_bwd_combine_kernel<bf16_t><<<pl.combine_grid, 64, 0, st>>>(p);
  else                  attn_pooled_bwd_combine_kernel<float><<<pl.combine_grid, 64, 0, st>>>(p);
  XP_CHECK_LAUNCH("xp_attn_pooled_bwd(combine)");
  return XP_OK;
}

extern "C" int xp_debug_attn_pooled_plan(int64_t B, int64_t H, int64_t S, int32_t dtype, int32_t backward, int32_t cus,
                                         XpAttnPooledPlanInfo* out) {
  XP_REQUIRE(out, "xp_debug_attn_pooled_plan: null argument");
  XP_REQUIRE(dtype == XP_BF16 || dtype == XP_F32, "xp_debug_attn_pooled_plan: bad dtype %d", dtype);
  XP_REQUIRE(B > 0 && H > 0 && S > 0, "xp_debug_attn_pooled_plan: empty problem B=%lld H=%lld S=%lld", (long long)B, (long long)H, (long long)S);
  PooledPlan p;
  const int rc = plan_pooled_for(B, H, S, backward != 0, cus, p);
  if (rc) return rc;
  *out = XpAttnPooledPlanInfo{p.chunks, p.chunk_keys, (int32_t)p.grid, (int32_t)p.combine_grid, {p.ml.off, p.ml.bytes},
                              {p.acc.off, p.acc.bytes}, {p.dq.off, p.dq.bytes}, p.ws_bytes, p.colsum_rows};
  return XP_OK;
}
