// PARADE's aggregation head (reference capreolus/reranker/ptparade.py:53-65, 78) on the fp32 [CLS] rows capamd_parade_passage_cls
// leaves behind.  fp32 operands and fp32 accumulation throughout, as the reference computes it: the head is ~0.3 GFLOP per document
// against ~730 GFLOP of encoder work, so 16-bit operands would buy nothing and add an error of their own.
//
// Rows of all documents form one M (B * (P + 1) rows for the first layer), so every weight tile is read once per call.  Launches:
//   x0_kernel                       X0 = [initial_cls; cls rows] + position embeddings
//   layer 1:  gemm (Q, K, V in one launch) -> attention (all P + 1 queries) -> gemm + residual -> LayerNorm
//             -> gemm + GELU -> gemm + residual -> LayerNorm
//   layer 2:  gemm (K, V over all rows) + gemm (Q of row 0 only) -> attention (row 0) -> the same row-wise tail on B rows
//             -> LayerNorm + linear (the score)
// Layer 2's output is read at row 0 only: its K and V need every row, its Q / attention / projections / FFN only row 0 (exact).
#include "capreolus_amd.h"
#include "workspace.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kEpiPlain = 0, kEpiGelu = 1, kEpiResid = 2;
constexpr int kMaxRows = 64;   // P + 1: the keys of one document fit one wave

struct GemmJob {
  const float* W;     // [N, K] (nn.Linear.weight)
  const float* bias;  // [N]
  float* out;         // [M, N]
};
struct GemmJobs {
  GemmJob j[3];       // blockIdx.z selects one: the Q, K, V projections share their A operand and run as one launch
};

// out[i][n] = sum_k A[i * lda + k] W[n][k] + bias[n]  (+ erf-GELU | + resid[i * ldr + n]).
// 256 threads, a 32 x 32 output tile per workgroup; wave w sums its quarter of K on __builtin_amdgcn_mfma_f32_16x16x4f32 (exact f32
// products, f32 accumulation), the four partial tiles are added through LDS in fixed order.  A lane loads 4 consecutive k of its
// row of A and of W (one 16-byte load each) and feeds them to 4 MFMAs: lane l holds A[row l & 15][k] and B[k][col l & 15] for the
// SAME k in both operands, so the k order inside a 16-wide step is permuted alike on both sides and the sum is the product's.
// K % 64 == 0, N % 32 == 0; rows >= M are clamped on load and never stored.
template <int EPI>
__global__ __launch_bounds__(256) void gemm_f32_kernel(const float* __restrict__ A, int64_t lda, int M, int N, int K, GemmJobs jobs,
                                                       const float* __restrict__ resid, int64_t ldr) {
  __shared__ float red[4][32][33];
  const GemmJob jb = jobs.j[blockIdx.z];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int li = lane & 15, lk = (lane >> 4) * 4;
  const float* a[2];
  const float* w[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int row = min(r0 + 16 * t + li, M - 1);
    a[t] = A + (int64_t)row * lda + lk;
    w[t] = jb.W + (int64_t)(c0 + 16 * t + li) * K + lk;
  }
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int kq = K >> 2, kb = wave * kq;
  for (int k = kb; k < kb + kq; k += 16) {
    float4 av[2], wv[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      av[t] = *reinterpret_cast<const float4*>(a[t] + k);
      wv[t] = *reinterpret_cast<const float4*>(w[t] + k);
    }
#pragma unroll
    for (int ta = 0; ta < 2; ++ta)
#pragma unroll
      for (int tw = 0; tw < 2; ++tw) {
        acc[ta][tw] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ta].x, wv[tw].x, acc[ta][tw], 0, 0, 0);
        acc[ta][tw] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ta].y, wv[tw].y, acc[ta][tw], 0, 0, 0);
        acc[ta][tw] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ta].z, wv[tw].z, acc[ta][tw], 0, 0, 0);
        acc[ta][tw] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ta].w, wv[tw].w, acc[ta][tw], 0, 0, 0);
      }
  }
  // C/D map of the 16x16 f32 tile: column lane & 15, row 4 (lane >> 4) + register
#pragma unroll
  for (int ta = 0; ta < 2; ++ta)
#pragma unroll
    for (int tw = 0; tw < 2; ++tw)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave][16 * ta + 4 * (lane >> 4) + r][16 * tw + li] = acc[ta][tw][r];
  __syncthreads();
  for (int e = tid; e < 32 * 32; e += 256) {
    const int rr = e >> 5, cc = e & 31, row = r0 + rr, col = c0 + cc;
    if (row >= M) continue;
    float v = ((red[0][rr][cc] + red[1][rr][cc]) + (red[2][rr][cc] + red[3][rr][cc])) + jb.bias[col];
    if (EPI == kEpiGelu) v = 0.5f * v * (1.f + erff(v * 0.70710678118654752f));
    if (EPI == kEpiResid) v += resid[(int64_t)row * ldr + col];
    jb.out[(int64_t)row * N + col] = v;
  }
}

// X0[b * R + r] = (r == 0 ? initial_cls : cls[b * P + r - 1]) + pos[r]   (ptparade.py:55-60)
__global__ __launch_bounds__(256) void x0_kernel(const float* __restrict__ cls, const float* __restrict__ init, const float* __restrict__ pos, int P,
                                                 int H, float* __restrict__ x0) {
  const int R = P + 1, b = blockIdx.x / R, r = blockIdx.x - b * R;
  const float* src = r == 0 ? init : cls + ((int64_t)b * P + r - 1) * H;
  for (int i = threadIdx.x; i < H; i += 256) x0[(int64_t)blockIdx.x * H + i] = src[i] + pos[(int64_t)r * H + i];
}

// Self-attention of one (document, head) over its R <= 64 rows, no mask (ptparade.py:62-63 passes none): one wave, lane i = query
// row i of the document (nq = R: every row; nq = 1: row 0, whose Q is row b of q).  K and V of the head in LDS; an online softmax
// over the keys in order, scores scaled by 1/8 = 1/sqrt(64).  ctx row layout as q's.
__global__ __launch_bounds__(64) void attn_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int R, int nq,
                                                  int H, float* __restrict__ ctx) {
  __shared__ float ks[kMaxRows][65], vs[kMaxRows][65];
  const int b = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
  for (int e = lane; e < R * 64; e += 64) {
    const int j = e >> 6, d = e & 63;
    const int64_t src = ((int64_t)b * R + j) * H + h * 64 + d;
    ks[j][d] = k[src];
    vs[j][d] = v[src];
  }
  __syncthreads();
  if (lane >= nq) return;
  const int64_t row = ((int64_t)b * nq + lane) * H + h * 64;
  float qv[64], acc[64];
#pragma unroll
  for (int d = 0; d < 64; ++d) {
    qv[d] = q[row + d];
    acc[d] = 0.f;
  }
  float mx = -INFINITY, l = 0.f;
  for (int j = 0; j < R; ++j) {
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < 64; ++d) s = __builtin_fmaf(qv[d], ks[j][d], s);
    s *= 0.125f;
    const float mn = fmaxf(mx, s), c = expf(mx - mn), p = expf(s - mn);
    l = l * c + p;
#pragma unroll
    for (int d = 0; d < 64; ++d) acc[d] = __builtin_fmaf(p, vs[j][d], acc[d] * c);
    mx = mn;
  }
  const float inv = 1.f / l;
#pragma unroll
  for (int d = 0; d < 64; ++d) ctx[row + d] = acc[d] * inv;
}

// y[i] = LayerNorm(x[i]) * gamma + beta, one workgroup per row (H <= 1024: four elements per thread).  lin_w != NULL: also
// score[i] = lin_w . y[i] + lin_b[0] (ptparade.py:78).
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, int H, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        float eps, float* __restrict__ y, const float* __restrict__ lin_w,
                                                        const float* __restrict__ lin_b, float* __restrict__ score) {
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t i = blockIdx.x;
  auto block_sum = [&](float s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    __syncthreads();
    if (lane == 0) red[wave] = s;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
  };
  float v[4];
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int j = tid + 256 * c;
    v[c] = j < H ? x[i * H + j] : 0.f;
    s += v[c];
  }
  const float mean = block_sum(s) / (float)H;
  float q = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (tid + 256 * c < H) q += (v[c] - mean) * (v[c] - mean);
  const float rstd = rsqrtf(block_sum(q) / (float)H + eps);
  float dot = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int j = tid + 256 * c;
    if (j < H) {
      const float o = (v[c] - mean) * rstd * gamma[j] + beta[j];
      y[i * H + j] = o;
      if (lin_w) dot = __builtin_fmaf(lin_w[j], o, dot);
    }
  }
  if (lin_w) {
    const float d = block_sum(dot);
    if (tid == 0) score[i] = d + lin_b[0];
  }
}

bool geometry_ok(const capamd_parade_head_model* hm, int B, int P) {
  return hm && hm->hidden >= 64 && hm->hidden <= 1024 && hm->heads * 64 == hm->hidden && hm->ffn >= 64 && hm->ffn % 64 == 0 && hm->ln_eps >= 0.f &&
         B >= 0 && P >= 1 && P + 1 <= kMaxRows;
}

struct Ws {
  float *x0, *q, *k, *v, *ctx, *t, *xa, *x1, *mid;
  size_t bytes;
};

// workspace: x0, q, k, v, ctx, t, xa, x1 ([M, H] each) and mid [M, F], M = B (P + 1)
Ws carve(int64_t M, int H, int F, void* base) {
  Carver c(base);
  return {c.take(M * H), c.take(M * H), c.take(M * H), c.take(M * H), c.take(M * H), c.take(M * H), c.take(M * H), c.take(M * H), c.take(M * F), c.bytes()};
}

template <int EPI>
void gemm(const float* A, int64_t lda, int M, int N, int K, GemmJobs jobs, int nz, const float* resid, int64_t ldr, hipStream_t s) {
  hipLaunchKernelGGL(gemm_f32_kernel<EPI>, dim3((unsigned)((M + 31) / 32), (unsigned)(N / 32), (unsigned)nz), dim3(256), 0, s, A, lda, M, N, K, jobs,
                     resid, ldr);
}

GemmJobs one(const float* W, const float* bias, float* out) {
  GemmJobs j{};
  j.j[0] = GemmJob{W, bias, out};
  return j;
}

}  // namespace

extern "C" {

int64_t capamd_parade_workspace_bytes(const capamd_parade_head_model* hm, int B, int P) {
  if (!geometry_ok(hm, B, P)) return -1;
  return (int64_t)carve((int64_t)B * (P + 1), hm->hidden, hm->ffn, nullptr).bytes;
}

int capamd_parade_head(const float* cls_rows, int B, int P, const capamd_parade_head_model* hm, void* workspace, int64_t workspace_bytes,
                       float* out, float* aggregated_out, void* stream) {
  if (!cls_rows || !geometry_ok(hm, B, P) || !workspace || !out) return CAPAMD_ERR_ARG;
  if (!hm->initial_cls || !hm->pos_emb || !hm->linear_w || !hm->linear_b) return CAPAMD_ERR_ARG;
  for (int i = 0; i < 16; ++i)
    if (!hm->layer1[i] || !hm->layer2[i]) return CAPAMD_ERR_ARG;
  if (B == 0) return CAPAMD_OK;
  const int H = hm->hidden, F = hm->ffn, R = P + 1, heads = hm->heads;
  const int64_t M = (int64_t)B * R;
  if (M > (1 << 30)) return CAPAMD_ERR_ARG;
  if ((int64_t)carve(M, H, F, nullptr).bytes > workspace_bytes) return CAPAMD_ERR_WORKSPACE;
  // the GEMMs load 16 bytes at a time from the activations and the weight rows
  if ((reinterpret_cast<uintptr_t>(workspace) & 255) != 0 || !aligned16(cls_rows)) return CAPAMD_ERR_ALIGN;
  for (int i = 0; i < 16; i += 2)
    if (!aligned16(hm->layer1[i]) || !aligned16(hm->layer2[i])) return CAPAMD_ERR_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  (void)hipGetLastError();
  const auto [x0, q, k, v, ctx, t, xa, x1, mid, carved] = carve(M, H, F, workspace);
  const float eps = hm->ln_eps;
  const int Mi = (int)M;

  hipLaunchKernelGGL(x0_kernel, dim3((unsigned)M), dim3(256), 0, s, cls_rows, hm->initial_cls, hm->pos_emb, P, H, x0);

  // transformer_layer_1 on every row of every document
  const float* const* L = hm->layer1;
  GemmJobs qkv{};
  qkv.j[0] = GemmJob{L[0], L[1], q};
  qkv.j[1] = GemmJob{L[2], L[3], k};
  qkv.j[2] = GemmJob{L[4], L[5], v};
  gemm<kEpiPlain>(x0, H, Mi, H, H, qkv, 3, nullptr, 0, s);
  hipLaunchKernelGGL(attn_kernel, dim3((unsigned)B, (unsigned)heads), dim3(64), 0, s, q, k, v, R, R, H, ctx);
  gemm<kEpiResid>(ctx, H, Mi, H, H, one(L[6], L[7], t), 1, x0, H, s);
  hipLaunchKernelGGL(layernorm_kernel, dim3((unsigned)M), dim3(256), 0, s, t, H, L[8], L[9], eps, xa, nullptr, nullptr, nullptr);
  gemm<kEpiGelu>(xa, H, Mi, F, H, one(L[10], L[11], mid), 1, nullptr, 0, s);
  gemm<kEpiResid>(mid, F, Mi, H, F, one(L[12], L[13], t), 1, xa, H, s);
  hipLaunchKernelGGL(layernorm_kernel, dim3((unsigned)M), dim3(256), 0, s, t, H, L[14], L[15], eps, x1, nullptr, nullptr, nullptr);

  // transformer_layer_2: K and V of every row, everything else for row 0 of each document only (B rows, row stride R * H in x1)
  L = hm->layer2;
  GemmJobs kv{};
  kv.j[0] = GemmJob{L[2], L[3], k};
  kv.j[1] = GemmJob{L[4], L[5], v};
  gemm<kEpiPlain>(x1, H, Mi, H, H, kv, 2, nullptr, 0, s);
  gemm<kEpiPlain>(x1, (int64_t)R * H, B, H, H, one(L[0], L[1], q), 1, nullptr, 0, s);
  hipLaunchKernelGGL(attn_kernel, dim3((unsigned)B, (unsigned)heads), dim3(64), 0, s, q, k, v, R, 1, H, ctx);
  gemm<kEpiResid>(ctx, H, B, H, H, one(L[6], L[7], t), 1, x1, (int64_t)R * H, s);
  hipLaunchKernelGGL(layernorm_kernel, dim3((unsigned)B), dim3(256), 0, s, t, H, L[8], L[9], eps, xa, nullptr, nullptr, nullptr);
  gemm<kEpiGelu>(xa, H, B, F, H, one(L[10], L[11], mid), 1, nullptr, 0, s);
  gemm<kEpiResid>(mid, F, B, H, F, one(L[12], L[13], t), 1, xa, H, s);
  hipLaunchKernelGGL(layernorm_kernel, dim3((unsigned)B), dim3(256), 0, s, t, H, L[14], L[15], eps, aggregated_out ? aggregated_out : x0, hm->linear_w,
                     hm->linear_b, out);
  return hipGetLastError() == hipSuccess ? CAPAMD_OK : CAPAMD_ERR_LAUNCH;
}

}  // extern "C"
