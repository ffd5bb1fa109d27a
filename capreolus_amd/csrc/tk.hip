// TK (reference capreolus/reranker/TK.py, TK_class.forward) in fp32 throughout: the reference's arithmetic on the exact-f32 MFMA
// (v_mfma_f32_16x16x4_f32: one rounding per product, f32 accumulation).
//
// Per micro-batch of documents, the query side (B x Q rows) and then the document side (B x L rows) run through the same kernels:
//   embed_kernel                 X = emb[id] + pe[pos] (pad columns 0), key mask = "embedding row not all zeros"
//   per layer (post-norm TransformerEncoderLayer, ReLU, no dropout):
//     gemm  QKV = X Wqkv^T + b                     [rows, 3 Hs]   (each head in its own 16-multiple slot, pad columns 0)
//     attn_kernel                                   [rows, Hs]     flash-style: K/V tiles through LDS, online softmax, no L x L matrix
//     gemm_ln  X1 = LN1(CTX Wo^T + bo + X)          [rows, Dp]     one workgroup owns whole rows: bias, residual, LayerNorm fused
//     gemm  FF = relu(X1 W1^T + b1)                 [rows, Fp]
//     gemm_ln  X = LN2(FF W2^T + b2 + X1)           [rows, Dp]
//   pool_kernel: mix a*emb + (1-a)*ctx, cosine against the Q query rows, 11 kernels (pads in closed form), log2 / sum, the three linears.
// Padded layouts (built once per set of weights by the caller, include/capreolus_amd.h): Dp, Fp and Hs = heads * hs are multiples of
// 64 and every pad row / column of the weights is zero, so no GEMM has edge code in N or K and the pad columns of every activation
// stay exactly 0 (LayerNorm normalises over the D real columns and writes 0 to the rest).
#include "capreolus_amd.h"
#include "tk_gemm.h"
#include "workspace.h"
#include <math.h>

namespace {

constexpr int kMaxQ = 32, kMaxDim = 512, kMaxFf = 512, kMaxHeadDim = 64, kNumKernels = 11;

// (gemm_mainloop, gemm_kernel and launch_gemm: tk_gemm.h)
// Y[i] = LayerNorm(A[i] . W^T + bias + R[i]) over the first `nreal` columns (gamma, beta; biased variance, eps), 0 in the pad columns.
// N = 64 CT (the whole padded width: one workgroup owns 32 whole rows).  Two-pass statistics in fp32, reduced in a fixed order.
template <int CT>
__global__ __launch_bounds__(256) void gemm_ln_kernel(const float* __restrict__ A, int64_t lda, int M, int K, const float* __restrict__ W,
                                                      const float* __restrict__ bias, const float* __restrict__ R, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, int nreal, float eps, float* __restrict__ Y) {
  constexpr int RT = 2, N = 64 * CT;
  __shared__ float As[16 * RT][kKC + 4];
  __shared__ float red[4][16 * RT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, g = lane >> 4;
  const int r0 = blockIdx.x * 16 * RT, cw = wave * 16 * CT;
  f32x4 acc[RT][CT];
  gemm_mainloop<RT, CT>(A, lda, M, K, W, r0, cw, As, acc);
  float s[RT][4];
#pragma unroll
  for (int i = 0; i < RT; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = min(r0 + 16 * i + 4 * g + r, M - 1);
      float t = 0.f;
#pragma unroll
      for (int j = 0; j < CT; ++j) {
        const int col = cw + 16 * j + li;
        const float v = acc[i][j][r] + bias[col] + R[(int64_t)row * N + col];
        acc[i][j][r] = v;
        t += v;
      }
      s[i][r] = t;
    }
  // row sums: over the 16 lanes of a row group, then over the 4 waves (fixed order)
  auto row_reduce = [&](float (&v)[RT][4]) {
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float t = v[i][r];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) t += __shfl_xor(t, o, 64);
        v[i][r] = t;
      }
    __syncthreads();
    if (li == 0) {
#pragma unroll
      for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave][16 * i + 4 * g + r] = v[i][r];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rr = 16 * i + 4 * g + r;
        v[i][r] = (red[0][rr] + red[1][rr]) + (red[2][rr] + red[3][rr]);
      }
  };
  row_reduce(s);
  const float inv_n = 1.f / (float)nreal;
  float mean[RT][4], q[RT][4];
#pragma unroll
  for (int i = 0; i < RT; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      mean[i][r] = s[i][r] * inv_n;
      float t = 0.f;
#pragma unroll
      for (int j = 0; j < CT; ++j) {
        const int col = cw + 16 * j + li;
        const float d = acc[i][j][r] - mean[i][r];
        if (col < nreal) t += d * d;
      }
      q[i][r] = t;
    }
  row_reduce(q);
#pragma unroll
  for (int i = 0; i < RT; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r0 + 16 * i + 4 * g + r;
      if (row >= M) continue;
      const float rstd = 1.f / sqrtf(q[i][r] * inv_n + eps);
#pragma unroll
      for (int j = 0; j < CT; ++j) {
        const int col = cw + 16 * j + li;
        Y[(int64_t)row * N + col] = col < nreal ? (acc[i][j][r] - mean[i][r]) * rstd * gamma[col] + beta[col] : 0.f;
      }
    }
}

// X[row] = emb[id] + pe[row % S] in the first D of Dp columns (0 beyond); valid[row] = 1 if the embedding row has a non-zero element
// (the reference's mask: decided before pe is added, not from id == pad).  One wave per row.  Ids outside [0, V) are scored as a zero
// row and set `bad_bit` in status (nn.Embedding raises).
__global__ __launch_bounds__(256) void embed_kernel(const int64_t* __restrict__ ids, int64_t rows, int S, const float* __restrict__ emb, int64_t V,
                                                    int D, int Dp, const float* __restrict__ pe, float* __restrict__ X, float* __restrict__ valid,
                                                    int* status, int bad_bit) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int64_t id = ids[row];
  const bool ok = id >= 0 && id < V;
  if (!ok && lane == 0) atomicOr(status, bad_bit);
  const float* e = emb + (ok ? id : 0) * (int64_t)D;
  const float* p = pe + (int64_t)(row % S) * D;
  int nz = 0;
  for (int c = lane; c < Dp; c += 64) {
    float v = 0.f;
    if (c < D) {
      const float x = ok ? e[c] : 0.f;
      nz |= x != 0.f;
      v = x + p[c];
    }
    X[row * Dp + c] = v;
  }
  nz = __any(nz);
  if (lane == 0) valid[row] = nz ? 1.f : 0.f;
}

// Self-attention of one (sequence, head, block of 64 query rows): 4 waves x 16 query rows.  K and V of the head stream through LDS
// 64 keys at a time.  The wave computes S^T = K Q^T (a 16-key x 16-query tile per MFMA chain; lane l then holds the scores of query
// l & 15 for keys 4 (l >> 4) + r), so the online softmax's max / sum per query are lane-local plus two shuffles, and P^T is already
// the B operand of O^T = V^T P^T (the k order inside each 4-key step permuted alike in V's rows).  valid (NULL: no mask): a key with
// valid == 0 is excluded; a query with valid == 0, or with every key excluded, gets a zero output (what the reference's attention
// gives a row of -inf scores).  qkv rows: [Q of head h at h HS | K at Hs + h HS | V at 2 Hs + h HS]; ctx rows [Hs].
template <int HS>
__global__ __launch_bounds__(256) void attn_kernel(const float* __restrict__ qkv, int Hs, int S, const float* __restrict__ valid, float scale,
                                                   float* __restrict__ ctx) {
  __shared__ float ks[64][HS + 4], vs[64][HS + 4], kb_add[64];
  constexpr int NC = HS / 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4, lk = g * 4;
  const int h = blockIdx.y;
  const int64_t seq = blockIdx.z, base = seq * S;
  const int64_t ld = 3 * (int64_t)Hs;
  const int q = blockIdx.x * 64 + wave * 16 + li;
  const int qc = min(q, S - 1);
  float4 qf[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) qf[c] = *reinterpret_cast<const float4*>(qkv + (base + qc) * ld + h * HS + 16 * c + lk);
  f32x4 o[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) o[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;
  for (int k0 = 0; k0 < S; k0 += 64) {
    __syncthreads();
    for (int e = tid; e < 64 * (HS / 4); e += 256) {
      const int j = e / (HS / 4), d = (e % (HS / 4)) * 4;
      float4 kv = float4{0.f, 0.f, 0.f, 0.f}, vv = kv;
      if (k0 + j < S) {
        const float* src = qkv + (base + k0 + j) * ld + h * HS + d;
        kv = *reinterpret_cast<const float4*>(src + Hs);
        vv = *reinterpret_cast<const float4*>(src + 2 * Hs);
      }
      *reinterpret_cast<float4*>(&ks[j][d]) = kv;
      *reinterpret_cast<float4*>(&vs[j][d]) = vv;
    }
    if (tid < 64) {
      const int j = k0 + tid;
      kb_add[tid] = (j < S && (!valid || valid[base + j] != 0.f)) ? 0.f : -INFINITY;
    }
    __syncthreads();
    f32x4 s[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < NC; ++c) s[t] = mfma4(*reinterpret_cast<const float4*>(&ks[16 * t + li][16 * c + lk]), qf[c], s[t]);
    }
    float mb = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[t][r] = s[t][r] * scale + kb_add[16 * t + 4 * g + r];
        mb = fmaxf(mb, s[t][r]);
      }
    mb = fmaxf(mb, __shfl_xor(mb, 16, 64));
    mb = fmaxf(mb, __shfl_xor(mb, 32, 64));
    const float mn = fmaxf(m, mb);
    // every key so far excluded for this query (mn = -inf): exponents against 0 give p = 0 and corr = 0 (o and l are still 0) - no
    // branch, the MFMAs below run with the whole wave
    const float mref = mn == -INFINITY ? 0.f : mn;
    const float corr = expf(m - mref);
    float ps = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[t][r] = expf(s[t][r] - mref);
        ps += s[t][r];
      }
    l = l * corr + ps;
    m = mn;
#pragma unroll
    for (int c = 0; c < NC; ++c) o[c] *= corr;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < NC; ++c)
          o[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(vs[16 * t + 4 * g + r][16 * c + li], s[t][r], o[c], 0, 0, 0);
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (q >= S) return;
  const bool live = l > 0.f && (!valid || valid[base + q] != 0.f);
  const float inv = live ? 1.f / l : 0.f;
  float* dst = ctx + (base + q) * (int64_t)Hs + h * HS;
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) dst[16 * c + 4 * g + r] = live ? o[c][r] * inv : 0.f;
  // the pad columns past the last head slot (Hs = heads HS rounded up to 64; fewer than 64, a multiple of 16): the out-proj GEMM reads
  // them against zero weights, so they must be 0 and not whatever the workspace held (0 x NaN = NaN)
  if (h == (int)gridDim.y - 1)
    for (int c = (h + 1) * HS + 4 * g; c < Hs; c += 16)
#pragma unroll
      for (int r = 0; r < 4; ++r) ctx[(base + q) * (int64_t)Hs + c + r] = 0.f;
}

// One document per workgroup: e_j = a emb[d_j] + (1 - a) xd_j (likewise the query rows, into LDS 8 at a time), cos[i][j] =
// q_i . e_j / ((|q_i| + 1e-9)(|e_j| + 1e-9)), 0 where either id is the pad; k = exp(-(cos - mu)^2) / (2 sigma^2) (the reference's
// precedence); ksum[i] = sum over all L positions (a pad position's term exp(-mu^2) / (2 sigma^2) in closed form); s_log = sum_i
// log2(ksum[i]), s_len = sum_i ksum[i] / L; score = comb . [s_log_w . s_log, s_len_w . s_len].  cos goes through `scratch` [Q][L].
__global__ __launch_bounds__(256) void pool_kernel(const int64_t* __restrict__ q_ids, const int64_t* __restrict__ d_ids, int Q, int L,
                                                   const float* __restrict__ xq, const float* __restrict__ xd, int Dp, const float* __restrict__ emb,
                                                   int64_t V, int D, int64_t pad, const float* __restrict__ mixer, float alpha,
                                                   const float* __restrict__ w_log, const float* __restrict__ w_len, const float* __restrict__ w_comb,
                                                   float* __restrict__ scratch, float* __restrict__ out, float* __restrict__ feats) {
  __shared__ float qs[8][kMaxDim];
  __shared__ float qden[kMaxQ], ksum[kMaxQ][kNumKernels];
  __shared__ int npad_s[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  const float a = mixer ? mixer[0] : alpha, ia = 1.f - a;
  const int64_t* qi_ids = q_ids + b * Q;
  const int64_t* di_ids = d_ids + b * L;
  float* cs = scratch + b * (int64_t)Q * L;
  int npad = 0;
  for (int i0 = 0; i0 < Q; i0 += 8) {
    const int nq = min(8, Q - i0);
    __syncthreads();
    for (int e = tid; e < nq * D; e += 256) {
      const int i = e / D, c = e - i * D;
      const int64_t id = qi_ids[i0 + i];
      const float x = (id >= 0 && id < V) ? emb[id * D + c] : 0.f;
      qs[i][c] = a * x + ia * xq[((b * Q) + i0 + i) * (int64_t)Dp + c];
    }
    __syncthreads();
    if (wave < nq) {     // |q_i| + 1e-9, one wave per row
      float t = 0.f;
      for (int c = lane; c < D; c += 64) t += qs[wave][c] * qs[wave][c];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
      if (lane == 0) qden[i0 + wave] = sqrtf(t) + 1e-9f;
    }
    if (wave + 4 < nq) {
      float t = 0.f;
      for (int c = lane; c < D; c += 64) t += qs[wave + 4][c] * qs[wave + 4][c];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
      if (lane == 0) qden[i0 + wave + 4] = sqrtf(t) + 1e-9f;
    }
    __syncthreads();
    for (int j = tid; j < L; j += 256) {
      const int64_t id = di_ids[j];
      if (id == pad) {
        if (i0 == 0) ++npad;
        continue;
      }
      const float* er = emb + ((id >= 0 && id < V) ? id : 0) * (int64_t)D;
      const bool ok = id >= 0 && id < V;
      const float* xr = xd + (b * L + j) * (int64_t)Dp;
      float dot[8], nrm = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) dot[i] = 0.f;
      for (int c = 0; c < D; ++c) {
        const float e = a * (ok ? er[c] : 0.f) + ia * xr[c];
        nrm += e * e;
#pragma unroll
        for (int i = 0; i < 8; ++i) dot[i] += qs[i][c] * e;
      }
      const float dden = sqrtf(nrm) + 1e-9f;
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (i < nq) cs[(int64_t)(i0 + i) * L + j] = qi_ids[i0 + i] == pad ? 0.f : dot[i] / (qden[i0 + i] * dden);
    }
  }
  // pads of the document
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) npad += __shfl_xor(npad, o, 64);
  if (lane == 0) npad_s[wave] = npad;
  __syncthreads();
  npad = (npad_s[0] + npad_s[1]) + (npad_s[2] + npad_s[3]);
  const float two_s2 = 2.f * (0.1f * 0.1f);     // 2 sigma^2 as the reference rounds it (fp32 sigma = 0.1)
  const float mu[kNumKernels] = {-0.9f, -0.7f, -0.5f, -0.3f, -0.1f, 0.1f, 0.3f, 0.5f, 0.7f, 0.9f, 1.0f};
  for (int i = wave; i < Q; i += 4) {
    const bool qpad = qi_ids[i] == pad;
    float acc[kNumKernels];
#pragma unroll
    for (int k = 0; k < kNumKernels; ++k) acc[k] = 0.f;
    if (!qpad) {
      for (int j = lane; j < L; j += 64) {
        if (di_ids[j] == pad) continue;
        const float c = cs[(int64_t)i * L + j];
#pragma unroll
        for (int k = 0; k < kNumKernels; ++k) acc[k] += expf(-(c - mu[k]) * (c - mu[k])) / two_s2;
      }
    }
    const int nzero = qpad ? L : npad;     // positions whose cosine is 0 (a pad on either side)
#pragma unroll
    for (int k = 0; k < kNumKernels; ++k) {
      float t = acc[k];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
      if (lane == 0) ksum[i][k] = t + (float)nzero * (expf(-mu[k] * mu[k]) / two_s2);
    }
  }
  __syncthreads();
  if (wave == 0) {
    float sl = 0.f, sn = 0.f;
    if (lane < kNumKernels) {
      for (int i = 0; i < Q; ++i) {
        sl += log2f(ksum[i][lane]);
        sn += ksum[i][lane];
      }
      sn /= (float)L;
      if (feats) {
        feats[b * 2 * kNumKernels + lane] = sl;
        feats[b * 2 * kNumKernels + kNumKernels + lane] = sn;
      }
    }
    float vl = lane < kNumKernels ? w_log[lane] * sl : 0.f, vn = lane < kNumKernels ? w_len[lane] * sn : 0.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      vl += __shfl_xor(vl, o, 64);
      vn += __shfl_xor(vn, o, 64);
    }
    if (lane == 0) out[b] = w_comb[0] * vl + w_comb[1] * vn;
  }
}

int head_slot(int hd) { return (hd + 15) / 16 * 16; }

struct Geo {
  int D, Dp, heads, hd, hs, Hs, F, Fp;
};

bool geometry(const capamd_tk_model* m, Geo* g) {
  if (!m || m->dim < 1 || m->dim > kMaxDim || m->heads < 1 || m->dim % m->heads != 0 || m->dim / m->heads > kMaxHeadDim || m->ffdim < 1 ||
      m->ffdim > kMaxFf || m->numlayers < 1 || m->vocab < 1 || m->max_len < 1)
    return false;
  g->D = m->dim;
  g->Dp = up64(m->dim);
  g->heads = m->heads;
  g->hd = m->dim / m->heads;
  g->hs = head_slot(g->hd);
  g->Hs = up64(g->heads * g->hs);
  g->F = m->ffdim;
  g->Fp = up64(m->ffdim);
  return true;
}

bool shape_ok(const capamd_tk_model* m, int Q, int L) { return Q >= 1 && Q <= kMaxQ && L >= 1 && L <= m->max_len; }

struct Ws {
  float *xq, *xd, *qkv, *ctx, *x1, *ff, *valid, *cos;
  size_t bytes;
};

// workspace for nb documents: final rows of both sides, and one set of layer buffers for the longer side
Ws carve(const Geo& g, int64_t nb, int Q, int L, void* base) {
  const int64_t rows = nb * (int64_t)(L > Q ? L : Q);
  Carver c(base);
  return {c.take(nb * Q * g.Dp), c.take(nb * L * g.Dp), c.take(rows * 3 * g.Hs), c.take(rows * g.Hs), c.take(rows * g.Dp),
          c.take(rows * g.Fp),   c.take(rows),          c.take(nb * Q * L),      c.bytes()};
}

void launch_gemm_ln(const float* A, int64_t lda, int M, int N, int K, const float* W, const float* bias, const float* R, const float* gamma,
                    const float* beta, int nreal, float eps, float* Y, hipStream_t s) {
  const dim3 grid((unsigned)((M + 31) / 32)), block(256);
#define TK_LN(CT) hipLaunchKernelGGL(gemm_ln_kernel<CT>, grid, block, 0, s, A, lda, M, K, W, bias, R, gamma, beta, nreal, eps, Y)
  switch (N / 64) {
    case 1: TK_LN(1); break;
    case 2: TK_LN(2); break;
    case 3: TK_LN(3); break;
    case 4: TK_LN(4); break;
    case 5: TK_LN(5); break;
    case 6: TK_LN(6); break;
    case 7: TK_LN(7); break;
    default: TK_LN(8); break;
  }
#undef TK_LN
}

void launch_attn(const Geo& g, const float* qkv, int S, int64_t nseq, const float* valid, float* ctx, hipStream_t s) {
  const dim3 grid((unsigned)((S + 63) / 64), (unsigned)g.heads, (unsigned)nseq), block(256);
  const float scale = 1.f / sqrtf((float)g.hd);
  switch (g.hs) {
    case 16: hipLaunchKernelGGL(attn_kernel<16>, grid, block, 0, s, qkv, g.Hs, S, valid, scale, ctx); break;
    case 32: hipLaunchKernelGGL(attn_kernel<32>, grid, block, 0, s, qkv, g.Hs, S, valid, scale, ctx); break;
    case 48: hipLaunchKernelGGL(attn_kernel<48>, grid, block, 0, s, qkv, g.Hs, S, valid, scale, ctx); break;
    default: hipLaunchKernelGGL(attn_kernel<64>, grid, block, 0, s, qkv, g.Hs, S, valid, scale, ctx); break;
  }
}

// the encoder over nseq sequences of S ids -> X [nseq S, Dp] (its final hidden rows)
void encode(const capamd_tk_model* m, const Geo& g, const int64_t* ids, int64_t nseq, int S, const Ws& w, float* X, int* status, int bad_bit,
            hipStream_t s) {
  const int64_t rows = nseq * S;
  const int M = (int)rows;
  hipLaunchKernelGGL(embed_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, ids, rows, S, m->emb, m->vocab, g.D, g.Dp, m->pe, X, w.valid,
                     status, bad_bit);
  for (int li = 0; li < m->numlayers; ++li) {
    const capamd_tk_layer& L = m->layers_host[li];
    launch_gemm<kEpiBias>(X, g.Dp, M, 3 * g.Hs, g.Dp, L.wqkv, L.bqkv, w.qkv, s);
    launch_attn(g, w.qkv, S, nseq, m->usemask ? w.valid : nullptr, w.ctx, s);
    launch_gemm_ln(w.ctx, g.Hs, M, g.Dp, g.Hs, L.wo, L.bo, X, L.ln1_g, L.ln1_b, g.D, m->ln_eps, w.x1, s);
    launch_gemm<kEpiRelu>(w.x1, g.Dp, M, g.Fp, g.Dp, L.w1, L.b1, w.ff, s);
    launch_gemm_ln(w.ff, g.Fp, M, g.Dp, g.Fp, L.w2, L.b2, w.x1, L.ln2_g, L.ln2_b, g.D, m->ln_eps, X, s);
  }
}

}  // namespace

extern "C" {

int64_t capamd_tk_workspace_bytes(const capamd_tk_model* m, int docs_per_microbatch, int Q, int L) {
  Geo g;
  if (!geometry(m, &g) || !shape_ok(m, Q, L) || docs_per_microbatch < 1) return -1;
  return (int64_t)carve(g, docs_per_microbatch, Q, L, nullptr).bytes;
}

int capamd_tk_forward(const int64_t* q_ids, const int64_t* d_ids, int B, int Q, int L, const capamd_tk_model* m, int docs_per_microbatch,
                      void* workspace, int64_t workspace_bytes, float* out, float* features_out, int* status, void* stream) {
  Geo g;
  if (!q_ids || !d_ids || !m || !workspace || !out || !status || !geometry(m, &g) || !shape_ok(m, Q, L) || B < 0 || docs_per_microbatch < 1)
    return CAPAMD_ERR_ARG;
  if (!m->emb || !m->pe || !m->layers_host || !m->s_log_w || !m->s_len_w || !m->comb_w || !(m->ln_eps >= 0.f)) return CAPAMD_ERR_ARG;
  for (int i = 0; i < m->numlayers; ++i) {
    const capamd_tk_layer& l = m->layers_host[i];
    const float* p[12] = {l.wqkv, l.bqkv, l.wo, l.bo, l.ln1_g, l.ln1_b, l.w1, l.b1, l.w2, l.b2, l.ln2_g, l.ln2_b};
    for (const float* x : p)
      if (!x) return CAPAMD_ERR_ARG;
    if (!aligned16(l.wqkv) || !aligned16(l.wo) || !aligned16(l.w1) || !aligned16(l.w2)) return CAPAMD_ERR_ALIGN;
  }
  if (B == 0) return CAPAMD_OK;
  const int64_t nb = docs_per_microbatch < B ? docs_per_microbatch : B;
  if (nb * (int64_t)(L > Q ? L : Q) > (int64_t)1 << 30) return CAPAMD_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  return run_microbatches(
      B, docs_per_microbatch, workspace, workspace_bytes, [&](int64_t n, void* base) { return carve(g, n, Q, L, base); },
      [&](int64_t b0, int64_t n, const Ws& w) {
        encode(m, g, q_ids + b0 * Q, n, Q, w, w.xq, status, CAPAMD_STATUS_QUERY_ID_RANGE, s);
        encode(m, g, d_ids + b0 * L, n, L, w, w.xd, status, CAPAMD_STATUS_DOC_ID_RANGE, s);
        hipLaunchKernelGGL(pool_kernel, dim3((unsigned)n), dim3(256), 0, s, q_ids + b0 * Q, d_ids + b0 * L, Q, L, w.xq, w.xd, g.Dp, m->emb, m->vocab,
                           g.D, m->pad, m->mixer, m->alpha, m->s_log_w, m->s_len_w, m->comb_w, w.cos, out + b0,
                           features_out ? features_out + b0 * 2 * kNumKernels : nullptr);
        return CAPAMD_OK;
      });
}

}  // extern "C"
