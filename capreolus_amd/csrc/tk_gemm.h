// The fp32 GEMM of the encoders that run in fp32 throughout (tk.hip, posit.hip): C = A W^T + bias on the exact-f32 MFMA
// (v_mfma_f32_16x16x4_f32: one rounding per product, f32 accumulation).  Weights are in nn.Linear layout [N][K], zero-padded by the
// caller so that N is a multiple of 64 and K a multiple of 64: no GEMM has edge code in N or K.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kEpiBias = 0, kEpiRelu = 1;
constexpr int kKC = 64;          // K chunk of the A tile staged in LDS

__device__ __forceinline__ f32x4 mfma4(float4 a, float4 b, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, c, 0, 0, 0);
  return c;
}

// The shared main loop: acc[rt][ct] += A[r0 + 16 rt + ., :] W[cw + 16 ct + ., :]^T over K (a multiple of 64).  The workgroup's
// 16 RT rows of A are staged in LDS, 64 k at a time (the next chunk is loaded into registers while this one is consumed); the
// wave's own 16 CT rows of W (nn.Linear layout [N][K]) are read from global memory, where every workgroup finds them in L2.  A lane
// loads 4 consecutive k of its row of A and of W and feeds them to 4 MFMAs: lane l holds A[row l & 15][k] and B[k][col l & 15] for
// the SAME k in both operands, so the k order inside a 16-wide step is permuted alike on both sides.  Rows >= M are clamped on load.
template <int RT, int CT>
__device__ __forceinline__ void gemm_mainloop(const float* __restrict__ A, int64_t lda, int M, int K, const float* __restrict__ W, int r0, int cw,
                                              float (*As)[kKC + 4], f32x4 (&acc)[RT][CT]) {
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lk = (lane >> 4) * 4;
#pragma unroll
  for (int i = 0; i < RT; ++i)
#pragma unroll
    for (int j = 0; j < CT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // staging: RT float4 per thread per chunk (16 RT rows x 64 k)
  // thread tid stages k 4 (tid & 15) .. + 3 of rows tid >> 4 + 16 i
  const int sr = tid >> 4, sk = (tid & 15) * 4;
  const float* a[RT];
#pragma unroll
  for (int i = 0; i < RT; ++i) a[i] = A + (int64_t)min(r0 + sr + 16 * i, M - 1) * lda + sk;
  float4 st[RT];
#pragma unroll
  for (int i = 0; i < RT; ++i) st[i] = *reinterpret_cast<const float4*>(a[i]);
  const float* w[CT];
#pragma unroll
  for (int j = 0; j < CT; ++j) w[j] = W + (int64_t)(cw + 16 * j + li) * K + lk;
  for (int k0 = 0; k0 < K; k0 += kKC) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < RT; ++i) *reinterpret_cast<float4*>(&As[sr + 16 * i][sk]) = st[i];
    __syncthreads();
    if (k0 + kKC < K) {
#pragma unroll
      for (int i = 0; i < RT; ++i) st[i] = *reinterpret_cast<const float4*>(a[i] + k0 + kKC);
    }
    float4 wv[CT];
#pragma unroll
    for (int j = 0; j < CT; ++j) wv[j] = *reinterpret_cast<const float4*>(w[j] + k0);
#pragma unroll
    for (int kk = 0; kk < kKC; kk += 16) {
      float4 wn[CT];
      if (kk + 16 < kKC) {
#pragma unroll
        for (int j = 0; j < CT; ++j) wn[j] = *reinterpret_cast<const float4*>(w[j] + k0 + kk + 16);
      }
#pragma unroll
      for (int i = 0; i < RT; ++i) {
        const float4 av = *reinterpret_cast<const float4*>(&As[16 * i + li][kk + lk]);
#pragma unroll
        for (int j = 0; j < CT; ++j) acc[i][j] = mfma4(av, wv[j], acc[i][j]);
      }
      if (kk + 16 < kKC) {
#pragma unroll
        for (int j = 0; j < CT; ++j) wv[j] = wn[j];
      }
    }
  }
}

// C[i][n] = A[i] . W[n] + bias[n] (ReLU'd for kEpiRelu).  256 threads; a workgroup computes 16 RT rows x 64 CT columns, wave w the
// columns 16 CT w .. 16 CT (w + 1).  N % (64 CT) == 0, K % 64 == 0.
template <int RT, int CT, int EPI>
__global__ __launch_bounds__(256) void gemm_kernel(const float* __restrict__ A, int64_t lda, int M, int K, const float* __restrict__ W,
                                                   const float* __restrict__ bias, float* __restrict__ C, int64_t ldc) {
  __shared__ float As[16 * RT][kKC + 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15;
  const int r0 = blockIdx.x * 16 * RT, cw = blockIdx.y * 64 * CT + wave * 16 * CT;
  f32x4 acc[RT][CT];
  gemm_mainloop<RT, CT>(A, lda, M, K, W, r0, cw, As, acc);
  // C/D map of the 16x16 f32 tile: column lane & 15, row 4 (lane >> 4) + register
#pragma unroll
  for (int j = 0; j < CT; ++j) {
    const int col = cw + 16 * j + li;
    const float b = bias[col];
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = r0 + 16 * i + 4 * (lane >> 4) + r;
        if (row >= M) continue;
        float v = acc[i][j][r] + b;
        if (EPI == kEpiRelu) v = fmaxf(v, 0.f);
        C[(int64_t)row * ldc + col] = v;
      }
  }
}

// C [M][N] = A [M][lda] W [N][K]^T + bias: the widest column tile that divides N
template <int EPI>
void launch_gemm(const float* A, int64_t lda, int M, int N, int K, const float* W, const float* bias, float* C, hipStream_t s) {
  const unsigned gx = (unsigned)((M + 31) / 32);
  const int n64 = N / 64;
  if (n64 % 3 == 0)
    hipLaunchKernelGGL((gemm_kernel<2, 3, EPI>), dim3(gx, (unsigned)(n64 / 3)), dim3(256), 0, s, A, lda, M, K, W, bias, C, (int64_t)N);
  else if (n64 % 2 == 0)
    hipLaunchKernelGGL((gemm_kernel<2, 2, EPI>), dim3(gx, (unsigned)(n64 / 2)), dim3(256), 0, s, A, lda, M, K, W, bias, C, (int64_t)N);
  else
    hipLaunchKernelGGL((gemm_kernel<2, 1, EPI>), dim3(gx, (unsigned)n64), dim3(256), 0, s, A, lda, M, K, W, bias, C, (int64_t)N);
}

}  // namespace
