// The small fp32 products of the losses and of retrieval evaluation: similarity matrices of gathered unit-norm features and the
// feature gradients that follow from them (common.h: xp_launch_small_gemm, xp_launch_logits; xp_sim_matrix is the C entry).
// Latency- not FLOP-bound (n is a few hundred at most): plain fp32 FMA tiles, a fixed reduction order and no atomics.
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
// (The butterfly carries no `#pragma unroll`: it compiles to a six-trip loop here whatever it is told.  XP_NO_PK_F32 keeps
// __shfl_xor out of line, this is its only call site in the file, and the unroller leaves a loop alone whose callee has one use --
// it expects the inliner to take it -- and then warns about the pragma.  Same six shuffle-adds, 32 down to 1.)
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
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) C[(int64_t)i * n + j] = (log_scale ? expf(*log_scale) : 1.0f) * s;
}

}  // namespace

void xp_launch_small_gemm(const float* X, int64_t sxi, int64_t sxk, const float* Y, int64_t syk, int64_t syj, float* C, int64_t ldc,
                          int I, int J, int K, const float* log_scale, int accumulate, hipStream_t st) {
  dim3 grid((unsigned)cdiv(J, 32), (unsigned)cdiv(I, 32));
  sgemm_strided_kernel<<<grid, 256, 0, st>>>(X, sxi, sxk, Y, syk, syj, C, ldc, I, J, K, log_scale, accumulate);
}

// logits A[n][n] = e^ls V T^T: the small form up to n = 128 (d a multiple of 4, 16-byte aligned rows), the tiled form beyond
// (Both callers, xp_contrastive_loss and xp_pair_loss, refuse a vis / txt off 16 bytes before they get here, and their concatenated
// operands are 256-byte aligned workspace pieces: the two address terms are always true today.  They stay as the kernel's own
// precondition, next to d % 4, for a caller inside the library that does not come through those checks.)
void xp_launch_logits(const float* vis, const float* txt, float* A, int64_t n, int64_t d, const float* log_scale, hipStream_t st) {
  if (n <= 128 && d % 4 == 0 && ((uintptr_t)vis & 15) == 0 && ((uintptr_t)txt & 15) == 0) {
    logits_small_kernel<<<(unsigned)cdiv(n * n, 4), 256, 0, st>>>(vis, txt, A, (int)n, (int)d, log_scale);
  } else {
    xp_launch_small_gemm(vis, d, 1, txt, 1, d, A, n, (int)n, (int)n, (int)d, log_scale, 0, st);
  }
}

extern "C" int xp_sim_matrix(const float* a, const float* b, float* sim, int64_t na, int64_t nb, int64_t d, void* stream) {
  XP_REQUIRE(a && b && sim && na > 0 && nb > 0 && d > 0, "xp_sim_matrix: bad arguments");
  // alignment class `any` for a, b and sim: sgemm_strided_kernel reads and writes one float per lane and access
  xp_launch_small_gemm(a, d, 1, b, 1, d, sim, nb, (int)na, (int)nb, (int)d, nullptr, 0, (hipStream_t)stream);
  XP_CHECK_LAUNCH("xp_sim_matrix");
  return XP_OK;
}
