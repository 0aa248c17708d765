// Shared device/host helpers for the gfx950 kernels of libxpretrain_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <initializer_list>
#include "../../include/xpretrain_hip.h"

typedef __bf16 bf16_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) short i16x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

// ------------------------------------------------------------------------------------------ errors
void xp_set_error(const char* fmt, ...);   // thread-local message (common.cpp)
bool xp_debug_flag(const char* name);      // XPRETRAIN_DEBUG=flag[,flag...] (common.cpp)
int xp_device_cus(const void* kernel = nullptr, int lds_bytes = 0);     // CUs of the current device, a kernel's LDS opt-in (common.cpp)

#define XP_REQUIRE(cond, ...)                                  \
  do {                                                         \
    if (!(cond)) { xp_set_error(__VA_ARGS__); return XP_ERR_ARG; } \
  } while (0)

// The pointer-alignment rule of the ABI (include/xpretrain_hip.h, "Pointer alignment"): every device pointer an entry receives is
// checked on the host before the entry's first HIP call.  `bytes` is the operand's class there (need 4 / 8 / 16: the widest access
// any kernel of the entry makes through that pointer); operands of class `any` are not checked, their kernels are element-wide.
// A null pointer passes: whether an operand may be absent is the entry's own check.  The message names entry, operand and bytes.
struct XpPtrName { const char* name; const void* ptr; };
inline int xp_check_aligned(const char* fn, unsigned bytes, std::initializer_list<XpPtrName> ptrs) {
  for (const XpPtrName& p : ptrs)
    if (((uintptr_t)p.ptr & (bytes - 1)) != 0) {
      xp_set_error("%s: %s=%p is not %u-byte aligned", fn, p.name, p.ptr, bytes);
      return XP_ERR_ARG;
    }
  return XP_OK;
}
#define XP_P(p) XpPtrName{#p, (const void*)(p)}                    /* a parameter, under its header name */
#define XP_REQUIRE_ALIGNED(fn, bytes, ...)                                           \
  do {                                                                               \
    if (int rc_al__ = xp_check_aligned(fn, bytes, {__VA_ARGS__})) return rc_al__;    \
  } while (0)

#define XP_CHECK_LAUNCH(name)                                                   \
  do {                                                                          \
    hipError_t e__ = hipGetLastError();                                         \
    if (e__ != hipSuccess) {                                                    \
      xp_set_error("%s: launch failed: %s", name, hipGetErrorString(e__));      \
      return XP_ERR_LAUNCH;                                                     \
    }                                                                           \
  } while (0)

static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// reduce.hip, rows_reduce_kernel: out[y][c] (+)= the sum of rows [y * nsum, min((y + 1) * nsum, nrows)) of the dense fp32 matrix
// in[nrows][width], for every y < ceil(nrows / nsum), in that file's fixed order (tree A).  The caller checks the launch.
void xp_launch_rows_reduce(const float* in, float* out, int nrows, int nsum, int width, int accumulate, hipStream_t st);

// small_gemm.hip: C[i][j] (+)= alpha * sum_k X[i * sxi + k * sxk] Y[k * syk + j * syj] for i < I, j < J over K terms, fp32, with
// alpha = exp(*log_scale), or 1 where log_scale is null; xp_launch_logits: A[n][n] = alpha * vis txt^T of two [n,d] operands, by the
// kernel that suits n and d.  The caller checks the launch.
void xp_launch_small_gemm(const float* X, int64_t sxi, int64_t sxk, const float* Y, int64_t syk, int64_t syj, float* C, int64_t ldc,
                          int I, int J, int K, const float* log_scale, int accumulate, hipStream_t st);
void xp_launch_logits(const float* vis, const float* txt, float* A, int64_t n, int64_t d, const float* log_scale, hipStream_t st);

// ------------------------------------------------------------------------------------------ scalars
template <typename T> struct DT;
template <> struct DT<bf16_t> { static constexpr int id = XP_BF16; };
template <> struct DT<float>  { static constexpr int id = XP_F32; };

__device__ __forceinline__ float to_f(float x) { return x; }
__device__ __forceinline__ float to_f(bf16_t x) { return (float)x; }
template <typename T> __device__ __forceinline__ T from_f(float x);
template <> __device__ __forceinline__ float from_f<float>(float x) { return x; }
template <> __device__ __forceinline__ bf16_t from_f<bf16_t>(float x) { return (bf16_t)x; }

// 4 consecutive elements <-> f32x4
__device__ __forceinline__ f32x4 load4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 load4(const bf16_t* p) {
  bf16x4 v = *reinterpret_cast<const bf16x4*>(p);
  return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}
__device__ __forceinline__ void store4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ void store4(bf16_t* p, f32x4 v) {
  bf16x4 o = {(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
  *reinterpret_cast<bf16x4*>(p) = o;
}

// 8 consecutive elements <-> two f32x4 (16-byte bf16 / 2 x 16-byte f32 accesses)
struct f32x8 { f32x4 lo, hi; };
__device__ __forceinline__ f32x8 load8(const float* p) { return f32x8{load4(p), load4(p + 4)}; }
__device__ __forceinline__ f32x8 load8(const bf16_t* p) {
  const bf16x8 v = *reinterpret_cast<const bf16x8*>(p);
  return f32x8{f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]}, f32x4{(float)v[4], (float)v[5], (float)v[6], (float)v[7]}};
}
__device__ __forceinline__ void store8(float* p, f32x8 v) { store4(p, v.lo); store4(p + 4, v.hi); }
__device__ __forceinline__ void store8(bf16_t* p, f32x8 v) {
  bf16x8 o = {(bf16_t)v.lo[0], (bf16_t)v.lo[1], (bf16_t)v.lo[2], (bf16_t)v.lo[3],
              (bf16_t)v.hi[0], (bf16_t)v.hi[1], (bf16_t)v.hi[2], (bf16_t)v.hi[3]};
  *reinterpret_cast<bf16x8*>(p) = o;
}

// v_rcp_f32 (1 ulp) instead of the IEEE division sequence (~10 instructions): the GELU epilogues run 128 of these per
// lane per 256x256 tile and were VALU-bound on the divide.
__device__ __forceinline__ float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float quick_gelu_f(float x) { return x * fast_rcp(1.0f + __expf(-1.702f * x)); }
__device__ __forceinline__ float quick_gelu_grad_f(float x) {
  float s = fast_rcp(1.0f + __expf(-1.702f * x));
  return s * (1.0f + 1.702f * x * (1.0f - s));
}

// erf GELU (hidden_act "gelu": x * Phi(x), Phi the standard normal CDF) and its derivative Phi(x) + x * phi(x).
// Phi(-|x|) = erfc(|x| / sqrt 2) / 2 by Abramowitz & Stegun 7.1.26: erfc(z) = t (a1 + t (a2 + t (a3 + t (a4 + t a5)))) exp(-z^2),
// t = 1 / (1 + p z), |error| <= 1.5e-7 ABSOLUTE for every z >= 0 -- the rounding of an fp32 value near 1, which is what Phi is where
// the error matters (x * Phi(-|x|) has its extremum 0.17 at |x| = 0.75; the tail's relative error is irrelevant: its absolute size
// is).  Branch-free, one v_rcp_f32 and one v_exp_f32 as the quick_gelu pair above -- the device library's erff branches per lane
// on |x| < 1 -- and exp(-z^2) = exp(-x^2 / 2) = sqrt(2 pi) phi(x) is the very factor the derivative needs.
struct NormalCdfPdf { float cdf, pdf; };
__device__ __forceinline__ NormalCdfPdf normal_cdf_pdf(float x) {
  const float z = fabsf(x) * 0.70710678118654752f;
  const float t = fast_rcp(1.0f + 0.3275911f * z);
  const float e = __expf(-z * z);
  float q = 1.061405429f;
  q = q * t - 1.453152027f;
  q = q * t + 1.421413741f;
  q = q * t - 0.284496736f;
  q = q * t + 0.254829592f;
  const float h = 0.5f * q * t * e;                    // Phi(-|x|)
  return NormalCdfPdf{x < 0.0f ? h : 1.0f - h, 0.39894228040143268f * e};
}
__device__ __forceinline__ float gelu_erf_f(float x) { return x * normal_cdf_pdf(x).cdf; }
__device__ __forceinline__ float gelu_erf_grad_f(float x) {
  const NormalCdfPdf n = normal_cdf_pdf(x);
  return n.cdf + x * n.pdf;
}
// the MLP activation of a GEMM kernel instantiation (gemm_common.h: ACT template parameters): XP_ACT_QUICK_GELU / XP_ACT_GELU
template <int ACT> __device__ __forceinline__ float act_f(float x) { return ACT == 0 ? quick_gelu_f(x) : gelu_erf_f(x); }
template <int ACT> __device__ __forceinline__ float act_grad_f(float x) { return ACT == 0 ? quick_gelu_grad_f(x) : gelu_erf_grad_f(x); }

// ------------------------------------------------------------------------------------------ gfx950 packed-fp32 hazard
// Measured on MI355X (tools/race_repro.py, csrc/probe.hip::probe_pk_kernel): a `v_pk_add_f32` whose LOW
// result half takes the HIGH dword of a source pair (`op_sel:[0,1]`, the form hipcc emits for `x - m[1]` when it keeps two
// row scalars {m0, m1} in one register pair) returns a wrong low half in lanes 48..63 while a wave of ANOTHER kernel issues
// MFMAs on the same SIMD (kernels of two streams sharing a CU).  Alone on the GPU the instruction is exact, so single-stream
// tests never see it.  Kernels in which hipcc forms such operands are compiled without packed fp32 arithmetic (they are
// HBM- or latency-bound), and the build lints the generated code of every kernel for the form (tools/check_isa.py).
#if defined(__HIP_DEVICE_COMPILE__)
#define XP_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define XP_NO_PK_F32
#endif

// ------------------------------------------------------------------------------------------ wave ops
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// ------------------------------------------------------------------------------------------ MFMA
// D[i][j] += sum_k A[i][k] B[k][j] on 16x16 tiles.  Lane l = (i16 = l & 15, g = l >> 4).
//   bf16 (16x16x32): the lane's 16-byte fragment holds k = 8g .. 8g+7 for row/col i16.
//   f32  (16x16x4, issued 4x): fragment holds 4 floats; MFMA e uses element e, i.e. k = 4g + e.
// Any k permutation is fine as long as A and B fragments use the same one -- every loader below does.
// C/D layout (both): lane holds D[row = 4g + r][col = i16], r = 0..3.
template <typename T> struct Frag;
template <> struct Frag<bf16_t> { typedef bf16x8 type; };
template <> struct Frag<float>  { typedef f32x4 type; };

__device__ __forceinline__ f32x4 mma16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mma16(f32x4 a, f32x4 b, f32x4 c) {
#pragma unroll
  for (int e = 0; e < 4; ++e) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[e], c, 0, 0, 0);
  return c;
}

// ------------------------------------------------------------------------------------------ LDS tiles
// Row-major tiles with 128-byte rows ([rows][8 x 16 B chunks]).  XOR swizzle on the 16-byte chunk
// index, conflict-free both for ds_read_b128 of a 16-row x 16-byte column (MFMA k-contiguous
// fragments) and for ds_read_b64_tr_b16 of 8 consecutive rows x 32 bytes (transposed fragments).
__device__ __forceinline__ int swz128(int row) { return ((row >> 1) & 3) << 1; }
__device__ __forceinline__ int tile128_off(int row, int chunk16) { return row * 128 + ((chunk16 ^ swz128(row)) << 4); }

// LDS transpose read: each lane passes the address of 4 contiguous 16-bit elements; within each
// 16-lane group the 16x4 elements form a [4][16] matrix (lanes 4j..4j+3 supply row j) and lane i gets
// column i: result[j] = element (i & 3) of the chunk supplied by lane 4j + (i >> 2).   (probe.hip pins it)
__device__ __forceinline__ i16x4 lds_read_tr16(const void* lds_ptr) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) i16x4*)(lds_ptr));
}
// The same read as inline asm, for loops that keep `buffer_load ... lds` DMA in flight: hipcc's waitcnt pass puts
// `s_waitcnt vmcnt(0)` in front of every ds_read_tr builtin while an LDS-DMA is outstanding (plain ds_read_b128 is not
// affected), which drains the whole prefetch pipeline once per phase.  The asm form is invisible to that pass -- and to
// its lgkmcnt bookkeeping: the CALLER must execute `s_waitcnt lgkmcnt(0)` before the first use of the result, and
// tools/check_isa.py (run by the build) verifies in the generated code that nothing touches the destination registers
// before that wait.  OFF = immediate byte offset (< 65536).
template <int OFF>
__device__ __forceinline__ i16x4 lds_read_tr16_async(const void* lds_ptr) {
  const unsigned addr = (unsigned)(size_t)((__attribute__((address_space(3))) char*)(lds_ptr));
  i16x4 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}
