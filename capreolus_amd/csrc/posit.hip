// POSITDRMM (reference capreolus/reranker/POSITDRMM.py: POSITDRMM_class.test_forward -> POSITDRMM_basic.forward) in fp32 throughout.
// Sequences are laid out time-major, [position][sequence][padded width], so that a range of positions of every sequence of the
// micro-batch is one contiguous block of GEMM rows.  Per micro-batch of n pairs:
//   front_kernel   one workgroup per pair: the Q query rows normalised into LDS (q / (|q| + 1e-7)); 16 lanes per document term read its
//                  row once per four query terms, write it to X (zero in the pad columns of the padded width Dp) and form the Q cosines
//                  dot(qn_i, d) / (|d| + 1e-7) -> mcos [n][Q][L]; from the ids alone the three match statistics of
//                  get_exact_match_stats (integer counts; the reference's divisions).
//   encode         the 2-layer bidirectional LSTM (hidden = dim) from zero state over ALL positions, pads included, for the query side
//                  (S = Q) and the document side (S = L).  Per layer the positions are walked in chunks of T steps:
//       gemm       (tk_gemm.h) P_dir = A W_ih^T + (b_ih + b_hh) for the chunk's T n rows, once per direction (the backward direction's
//                  chunk is the mirrored range of positions); layer 0: A = X, K = Dp; layer 1: A = Y0, K = 2 Dp
//       rec_kernel the recurrence: one workgroup owns 16 sequences of one direction for the chunk's T steps.  h lives in LDS (double
//                  buffered: one barrier per step), c in registers, the step's h W_hh^T runs on v_mfma_f32_16x16x4_f32 with W_hh read
//                  from global memory every step (all workgroups of a direction find it in L2; even workgroup ids, i.e. even XCDs,
//                  take the forward direction and odd ones the backward direction, so one XCD's L2 holds one direction's weights).
//                  Gate rows are packed so that the i, f, g, o pre-activations of one hidden unit of one sequence land in one lane.
//                  The backward direction walks t downwards in place.  Between chunks c goes through a small state buffer and h is
//                  read back from the layer's output.  No step depends on another workgroup.
//   pool_kernel    one workgroup per pair: context rows [fwd + x, bwd + x], the query's normalised into LDS, the cosines of every
//                  document position (no epsilon) -> mctx; per query term one wave pools max and mean-of-top-5 of mcos and mctx (top 5
//                  per lane in registers, merged by five rounds of wave-max) and the exact-match row in closed form from the count;
//                  Q1, LeakyReLU, softmax(idf), Wg over [ans, extras].
// A pair's results do not depend on its tile mates, on the micro-batch size or on the chunk length, bit for bit.
#include "capreolus_amd.h"
#include "cos_front.h"
#include "tk_gemm.h"
#include "workspace.h"
#include <math.h>

namespace {

constexpr int kMaxQ = 16, kMaxDim = 320, kMaxL = 8192, kSeqTile = 16;
constexpr int64_t kProjBytes = (int64_t)512 << 20;     // the two directions' projection buffers of one chunk

struct Ws {
  float *X, *QX, *Y0, *Y1, *QY1, *P, *cst, *mcos, *mctx, *stats;
  int T;          // positions per chunk of the recurrence: what P is sized for
  size_t bytes;
};

int chunk_steps(int64_t nb, int Dp, int Q, int L) {
  const int64_t S = L > Q ? L : Q, t = kProjBytes / (nb * 8 * Dp * 4);
  return (int)(t < 1 ? 1 : t > S ? S : t);
}

Ws carve(int64_t nb, int Dp, int Q, int L, void* base) {
  const int64_t S = L > Q ? L : Q, T = chunk_steps(nb, Dp, Q, L);
  Carver c(base);
  return {c.take(L * nb * Dp),     c.take(Q * nb * Dp), c.take(S * nb * 2 * Dp), c.take(L * nb * 2 * Dp), c.take(Q * nb * 2 * Dp),
          c.take(T * nb * 8 * Dp), c.take(2 * nb * Dp), c.take(nb * Q * L),      c.take(nb * Q * L),      c.take(nb * 4),
          (int)T,                  c.bytes()};
}

// One pass of a 16-lane group over a row val(0 .. W - 1) against the rows i0 .. i0 + 3 of qn [Q][W] (normalised, in LDS): the dot
// products divided by the row's norm + eps to out[i * stride].  FIRST: the norm is formed here (returned with eps added, and handed to
// the later passes).
template <bool FIRST, class F>
__device__ __forceinline__ float cos_pass(F val, int W, const float* qn, int i0, int Q, int l, float eps, float* __restrict__ out, int64_t stride,
                                          float den) {
  const int nq = Q - i0 < 4 ? Q - i0 : 4;
  const float* q0 = qn + i0 * W;
  const float* q1 = qn + (i0 + (nq > 1 ? 1 : 0)) * W;
  const float* q2 = qn + (i0 + (nq > 2 ? 2 : 0)) * W;
  const float* q3 = qn + (i0 + (nq > 3 ? 3 : 0)) * W;
  float ss = 0.f, a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (int k = l; k < W; k += 16) {
    const float v = val(k);
    if (FIRST) ss = fmaf(v, v, ss);
    a0 = fmaf(v, q0[k], a0);
    a1 = fmaf(v, q1[k], a1);
    a2 = fmaf(v, q2[k], a2);
    a3 = fmaf(v, q3[k], a3);
  }
  a0 = group16_sum(a0);
  a1 = group16_sum(a1);
  a2 = group16_sum(a2);
  a3 = group16_sum(a3);
  if (FIRST) den = sqrtf(group16_sum(ss)) + eps;
  if (l < nq) {
    const float a = l == 0 ? a0 : l == 1 ? a1 : l == 2 ? a2 : a3;
    out[(int64_t)(i0 + l) * stride] = a / den;
  }
  return den;
}

// c + a b with the product rounded before the sum.  (__fmul_rn / __fadd_rn are plain * and + in HIP's headers, and under hipcc's
// default -ffp-contract=fast the pair became one fma: the idf sum of a document that matches two query terms was an ulp off.)
__device__ __forceinline__ float mul_then_add(float a, float b, float c) {
#pragma clang fp contract(off)
  const float p = a * b;
  return c + p;
}

// ---- stage 1 ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void front_kernel(const int64_t* __restrict__ q_ids, const float* __restrict__ q_idf, const int64_t* __restrict__ d_ids,
                                                    int Q, int L, const float* __restrict__ emb, int64_t V, int D, int Dp, int64_t pad, int64_t n,
                                                    float* __restrict__ X, float* __restrict__ QX, float* __restrict__ mcos,
                                                    float* __restrict__ stats, int* status) {
  extern __shared__ float lds[];
  const FrontLds at(Q, D, Q + 2);
  float* qn = lds;                                          // [Q][D]
  int64_t* qid = reinterpret_cast<int64_t*>(lds + at.qid);  // [Q]
  int* cnt = reinterpret_cast<int*>(lds + at.cnt);          // [Q] matches per query term, [1] bigrams, [1] length
  const int tid = threadIdx.x, g = tid >> 4, l = tid & 15;
  const int64_t b = blockIdx.x;
  if (tid < Q + 2) cnt[tid] = 0;
  // the query: 16 lanes per row
  for (int i = g; i < Q; i += 16) {
    const int64_t id = q_ids[b * Q + i];
    const bool ok = id >= 0 && id < V;
    if (!ok && l == 0) atomicOr(status, CAPAMD_STATUS_QUERY_ID_RANGE);
    const float* e = emb + (ok ? id : 0) * (int64_t)D;
    float ss = 0.f;
    for (int k = l; k < D; k += 16) {
      const float v = ok ? e[k] : 0.f;
      ss = fmaf(v, v, ss);
    }
    const float den = sqrtf(group16_sum(ss)) + 1e-7f;
    float* qx = QX + ((int64_t)i * n + b) * Dp;
    for (int k = l; k < Dp; k += 16) {
      const float v = (ok && k < D) ? e[k] : 0.f;
      qx[k] = v;
      if (k < D) qn[i * D + k] = v / den;
    }
    if (l == 0) qid[i] = id;
  }
  __syncthreads();
  // the document: 16 lanes per term, the row read once per group of four query terms
  for (int t = g; t < L; t += 16) {
    const int64_t id = d_ids[b * L + t];
    const bool ok = id >= 0 && id < V;
    if (!ok && l == 0) atomicOr(status, CAPAMD_STATUS_DOC_ID_RANGE);
    const float* e = emb + (ok ? id : 0) * (int64_t)D;
    float* x = X + ((int64_t)t * n + b) * Dp;
    for (int k = l; k < Dp; k += 16) x[k] = (ok && k < D) ? e[k] : 0.f;
    auto val = [&](int k) { return ok ? e[k] : 0.f; };
    float* out = mcos + (b * Q) * (int64_t)L + t;
    const float den = cos_pass<true>(val, D, qn, 0, Q, l, 1e-7f, out, L, 0.f);
    for (int i0 = 4; i0 < Q; i0 += 4) cos_pass<false>(val, D, qn, i0, Q, l, 1e-7f, out, L, den);
  }
  // get_exact_match_stats: the query as it is, the document without its pads (so a bigram spans a pad inside the document)
  for (int t = tid; t < L; t += 256) {
    const int64_t id = d_ids[b * L + t];
    if (id == pad) continue;
    atomicAdd(&cnt[Q + 1], 1);
    int nx = t + 1;
    while (nx < L && d_ids[b * L + nx] == pad) ++nx;
    const int64_t idn = nx < L ? d_ids[b * L + nx] : pad;
    for (int i = 0; i < Q; ++i) {
      if (qid[i] != id) continue;
      atomicAdd(&cnt[i], 1);
      if (i + 1 < Q && nx < L && qid[i + 1] == idn) atomicAdd(&cnt[Q], 1);
    }
  }
  __syncthreads();
  if (tid == 0) {
    const int len = cnt[Q + 1];
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    if (len < 2) {
      atomicOr(status, CAPAMD_STATUS_SHORT_DOC);
    } else {
      int64_t em = 0;
      float widf = 0.f;
      for (int i = 0; i < Q; ++i) {          // in query order, the product and the sum each rounded as the reference's tensor arithmetic does
        em += cnt[i];
        widf = mul_then_add((float)cnt[i], q_idf[b * Q + i], widf);
      }
      s0 = (float)((double)em / (double)len);
      s1 = widf / (float)len;
      s2 = (float)((double)cnt[Q] / (double)(len - 1));
    }
    stats[b * 4 + 0] = s0;
    stats[b * 4 + 1] = s1;
    stats[b * 4 + 2] = s2;
    stats[b * 4 + 3] = 0.f;
  }
}

// ---- stage 2 ---------------------------------------------------------------------------------------------------------------------------
// Steps s0 .. s0 + Tc - 1 of one layer's recurrence for 16 sequences of one direction.  P [2][Tc n][4 Dp]: the chunk's input
// projections with both biases, rows in ascending position; Y [S][n][2 Dp]; cst [2][n][Dp].  Packed gate order: row
// ub 64 + gate 16 + j = gate (i, f, g, o) of hidden unit ub 16 + j.  Wave w owns the unit blocks w NB .. w NB + NB - 1; in the MFMA's
// C layout lane l then holds column (unit) l & 15 of the four gate tiles for the sequences 4 (l >> 4) .. + 3.  Whh [2][4 Dp x Dp] is
// stored fragment-major, [unit block][k / 16][gate][lane][4]: lane l's four floats are row ub 64 + gate 16 + (l & 15), columns
// 16 (k / 16) + 4 (l >> 4) .. + 3 - what the lane feeds to four MFMAs -, so a wave's load is 1 KiB in a row.  (Read in nn.Linear
// layout, as the GEMM reads its weights, a load instruction touched 64 cache lines: 52 us per step instead of 40 at dim 300.)
template <int NB>
__global__ __launch_bounds__(256) void rec_kernel(const float* __restrict__ P, const float* __restrict__ Whh, float* __restrict__ Y,
                                                  float* __restrict__ cst, int n, int S, int s0, int Tc) {
  constexpr int Dp = 64 * NB, LD = Dp + 4;
  __shared__ float hbuf[2][kSeqTile][LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lq = lane >> 4, lk = lq * 4;
  const int dir = blockIdx.x & 1, seq0 = (blockIdx.x >> 1) * kSeqTile;
  const float* W = Whh + (int64_t)dir * 4 * Dp * Dp;
  const float* Pd = P + (int64_t)dir * Tc * n * 4 * Dp;
  // the state behind the previous chunk: h is the layer's output at the step before, c comes from the state buffer
  const int tprev = dir ? S - s0 : s0 - 1;
  for (int e = tid; e < kSeqTile * Dp; e += 256) {
    const int r = e / Dp, k = e - r * Dp;
    const int seq = min(seq0 + r, n - 1);
    hbuf[0][r][k] = s0 ? Y[((int64_t)tprev * n + seq) * 2 * Dp + dir * Dp + k] : 0.f;
  }
  float c[NB][4];
#pragma unroll
  for (int ub = 0; ub < NB; ++ub)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int seq = min(seq0 + 4 * lq + j, n - 1);
      c[ub][j] = s0 ? cst[((int64_t)dir * n + seq) * Dp + (wave * NB + ub) * 16 + li] : 0.f;
    }
  // fragment-major W_hh: the wave's unit blocks are NB x NB groups of 4096 floats in a row; a load instruction reads 1 KiB in a row
  const float* w0 = W + (int64_t)wave * NB * (64 * Dp) + lane * 4;
  float4 wv[4][4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk)
#pragma unroll
    for (int gt = 0; gt < 4; ++gt) wv[kk][gt] = *reinterpret_cast<const float4*>(w0 + (kk * 4 + gt) * 256);
  __syncthreads();
  for (int s = 0; s < Tc; ++s) {
    const int t = dir ? S - 1 - s0 - s : s0 + s;
    const int prow = dir ? Tc - 1 - s : s;
    const float(*h)[LD] = hbuf[s & 1];
    float(*hn)[LD] = hbuf[(s & 1) ^ 1];
#pragma unroll
    for (int ub = 0; ub < NB; ++ub) {
      const int ubg = wave * NB + ub, u = ubg * 16 + li;
      // the pre-activations are asked for before the products
      float p[4][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int seq = min(seq0 + 4 * lq + j, n - 1);
        const float* pr = Pd + ((int64_t)prow * n + seq) * 4 * Dp + ubg * 64 + li;
#pragma unroll
        for (int gt = 0; gt < 4; ++gt) p[j][gt] = pr[gt * 16];
      }
      f32x4 acc[4];
#pragma unroll
      for (int gt = 0; gt < 4; ++gt) acc[gt] = f32x4{0.f, 0.f, 0.f, 0.f};
      // W_hh in groups of 64 k, the next group loaded while this one is consumed.  The wave's NB x NB groups are one contiguous stream
      // that wraps around: the group behind a unit block's last is the next block's first, and behind the step's last the next step's
      // first, so no load is waited for at a block's or a step's start.  (A rolled loop: unrolled, the compiler asks for all of W_hh's
      // rows at once and spills.)
#pragma unroll 1
      for (int kg = 0; kg < NB; ++kg) {
        const int gn = ub * NB + kg + 1 == NB * NB ? 0 : ub * NB + kg + 1;
        float4 wn[4][4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
          for (int gt = 0; gt < 4; ++gt) wn[kk][gt] = *reinterpret_cast<const float4*>(w0 + gn * 4096 + (kk * 4 + gt) * 256);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const float4 av = *reinterpret_cast<const float4*>(&h[li][kg * 64 + 16 * kk + lk]);
#pragma unroll
          for (int gt = 0; gt < 4; ++gt) acc[gt] = mfma4(av, wv[kk][gt], acc[gt]);
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
          for (int gt = 0; gt < 4; ++gt) wv[kk][gt] = wn[kk][gt];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float gi = acc[0][j] + p[j][0], gf = acc[1][j] + p[j][1], gg = acc[2][j] + p[j][2], go = acc[3][j] + p[j][3];
        const float cc = sigmoidf_(gf) * c[ub][j] + sigmoidf_(gi) * tanhf(gg);
        const float hv = sigmoidf_(go) * tanhf(cc);
        c[ub][j] = cc;
        hn[4 * lq + j][u] = hv;
        const int seq = seq0 + 4 * lq + j;
        if (seq < n) Y[((int64_t)t * n + seq) * 2 * Dp + dir * Dp + u] = hv;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int ub = 0; ub < NB; ++ub)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int seq = seq0 + 4 * lq + j;
      if (seq < n) cst[((int64_t)dir * n + seq) * Dp + (wave * NB + ub) * 16 + li] = c[ub][j];
    }
}

// ---- stage 3 ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// max and mean of the 5 largest of row[0 .. L - 1] (L >= 5) by one wave: every lane keeps the 5 largest of its share, sorted, in
// registers; five rounds take the largest head of all lanes and pop it in the lowest lane that holds it (ties change nothing: only the
// sum is used).  Summed largest first, as torch.sum over the sorted topk does.
__device__ __forceinline__ void pool_row(const float* __restrict__ row, int L, int lane, float* mx, float* mean5) {
  const float ninf = -INFINITY;
  float t0 = ninf, t1 = ninf, t2 = ninf, t3 = ninf, t4 = ninf;
  for (int t = lane; t < L; t += 64) {
    const float v = row[t];
    if (v > t4) {
      t4 = v;
      if (t4 > t3) { const float x = t3; t3 = t4; t4 = x; }
      if (t3 > t2) { const float x = t2; t2 = t3; t3 = x; }
      if (t2 > t1) { const float x = t1; t1 = t2; t2 = x; }
      if (t1 > t0) { const float x = t0; t0 = t1; t1 = x; }
    }
  }
  float sum = 0.f;
  for (int r = 0; r < 5; ++r) {
    const float m = wave_max(t0);
    const unsigned long long have = __ballot(t0 == m);
    if (have && lane == __ffsll(have) - 1) {
      t0 = t1;
      t1 = t2;
      t2 = t3;
      t3 = t4;
      t4 = ninf;
    }
    if (r == 0) *mx = m;
    sum += m;
  }
  *mean5 = sum / 5.f;
}

__global__ __launch_bounds__(256) void pool_kernel(const int64_t* __restrict__ q_ids, const float* __restrict__ q_idf, const int64_t* __restrict__ d_ids,
                                                   int Q, int L, int D, int Dp, int64_t pad, int64_t n, const float* __restrict__ X,
                                                   const float* __restrict__ QX, const float* __restrict__ Y1, const float* __restrict__ QY1,
                                                   const float* __restrict__ mcos, float* __restrict__ mctx, const float* __restrict__ stats,
                                                   const float* __restrict__ extras, const float* __restrict__ bm25, const float* __restrict__ q1_w,
                                                   const float* __restrict__ q1_b, const float* __restrict__ wg_w, const float* __restrict__ wg_b,
                                                   float* __restrict__ out, float* __restrict__ feat_out, float* __restrict__ stats_out,
                                                   float* __restrict__ qctx_out, float* __restrict__ dctx_out) {
  extern __shared__ float lds[];
  float* qcn = lds;                        // [Q][2 D] the query's context rows, normalised
  float* feat = lds + (size_t)Q * 2 * D;   // [Q][6]
  const int tid = threadIdx.x, g = tid >> 4, l = tid & 15, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  const int W = 2 * D;
  for (int i = g; i < Q; i += 16) {
    const float* y = QY1 + ((int64_t)i * n + b) * 2 * Dp;
    const float* x = QX + ((int64_t)i * n + b) * Dp;
    auto val = [&](int k) { return k < D ? y[k] + x[k] : y[Dp + k - D] + x[k - D]; };      // the residual per direction
    float ss = 0.f;
    for (int k = l; k < W; k += 16) {
      const float v = val(k);
      ss = fmaf(v, v, ss);
    }
    const float den = sqrtf(group16_sum(ss));
    for (int k = l; k < W; k += 16) {
      const float v = val(k);
      qcn[i * W + k] = v / den;
      if (qctx_out) qctx_out[(b * Q + i) * W + k] = v;
    }
  }
  __syncthreads();
  for (int t = g; t < L; t += 16) {
    const float* y = Y1 + ((int64_t)t * n + b) * 2 * Dp;
    const float* x = X + ((int64_t)t * n + b) * Dp;
    auto val = [&](int k) { return k < D ? y[k] + x[k] : y[Dp + k - D] + x[k - D]; };
    if (dctx_out)
      for (int k = l; k < W; k += 16) dctx_out[(b * L + t) * W + k] = val(k);
    float* o = mctx + (b * Q) * (int64_t)L + t;
    const float den = cos_pass<true>(val, W, qcn, 0, Q, l, 0.f, o, L, 0.f);
    for (int i0 = 4; i0 < Q; i0 += 4) cos_pass<false>(val, W, qcn, i0, Q, l, 0.f, o, L, den);
  }
  __threadfence();
  __syncthreads();
  for (int i = wave; i < Q; i += 4) {
    float f[6];
    pool_row(mcos + (b * Q + i) * (int64_t)L, L, lane, &f[0], &f[1]);
    pool_row(mctx + (b * Q + i) * (int64_t)L, L, lane, &f[2], &f[3]);
    // the exact-match row holds only 0 and 1 (all 0 for a pad query term): its max and its top-5 sum follow from the count
    const int64_t qid = q_ids[b * Q + i];
    int hits = 0;
    if (qid != pad)
      for (int t = lane; t < L; t += 64) hits += d_ids[b * L + t] == qid;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) hits += __shfl_xor(hits, o, 64);
    f[4] = hits > 0 ? 1.f : 0.f;
    f[5] = (float)(hits < 5 ? hits : 5) / 5.f;
    if (lane < 6) {
      const float v = lane == 0 ? f[0] : lane == 1 ? f[1] : lane == 2 ? f[2] : lane == 3 ? f[3] : lane == 4 ? f[4] : f[5];
      feat[i * 6 + lane] = v;
      if (feat_out) feat_out[(b * Q + i) * 6 + lane] = v;
    }
  }
  __syncthreads();
  if (tid == 0) {
    float mx = -INFINITY;
    for (int i = 0; i < Q; ++i) mx = fmaxf(mx, q_idf[b * Q + i]);
    float den = 0.f;
    for (int i = 0; i < Q; ++i) den += expf(q_idf[b * Q + i] - mx);
    float ans = 0.f;
    for (int i = 0; i < Q; ++i) {
      float a = q1_b[0];
      for (int k = 0; k < 6; ++k) a = fmaf(q1_w[k], feat[i * 6 + k], a);
      a = a > 0.f ? a : 0.01f * a;                                        // LeakyReLU's default slope
      ans += expf(q_idf[b * Q + i] - mx) / den * a;
    }
    float ex[4];
    for (int k = 0; k < 4; ++k) ex[k] = extras ? extras[b * 4 + k] : k < 3 ? stats[b * 4 + k] : bm25[b];
    float sc = wg_b[0];
    sc = fmaf(wg_w[0], ans, sc);
    for (int k = 0; k < 4; ++k) sc = fmaf(wg_w[1 + k], ex[k], sc);
    out[b] = sc;
    if (stats_out)
      for (int k = 0; k < 3; ++k) stats_out[b * 3 + k] = stats[b * 4 + k];
  }
}

bool shape_ok(const capamd_posit_model* m, int Q, int L) {
  return m && m->dim >= 1 && m->dim <= kMaxDim && m->vocab >= 1 && Q >= 1 && Q <= kMaxQ && L >= 5 && L <= kMaxL;
}

void launch_rec(int NB, unsigned grid, hipStream_t s, const float* P, const float* Whh, float* Y, float* cst, int n, int S, int s0, int Tc) {
#define POSIT_REC(N) hipLaunchKernelGGL(rec_kernel<N>, dim3(grid), dim3(256), 0, s, P, Whh, Y, cst, n, S, s0, Tc)
  switch (NB) {
    case 1: POSIT_REC(1); break;
    case 2: POSIT_REC(2); break;
    case 3: POSIT_REC(3); break;
    case 4: POSIT_REC(4); break;
    default: POSIT_REC(5); break;
  }
#undef POSIT_REC
}

// the two LSTM layers over n sequences of S positions: X [S][n][Dp] -> Yout [S][n][2 Dp] (forward half, backward half)
void encode(const capamd_posit_model* m, int Dp, int n, int S, const Ws& w, const float* X, float* Yout, hipStream_t s) {
  const int T = w.T;
  const unsigned grid = 2u * (unsigned)((n + kSeqTile - 1) / kSeqTile);
  for (int layer = 0; layer < 2; ++layer) {
    const float* A = layer ? w.Y0 : X;
    const int K = layer ? 2 * Dp : Dp;
    float* Y = layer ? Yout : w.Y0;
    for (int s0 = 0; s0 < S; s0 += T) {
      const int Tc = S - s0 < T ? S - s0 : T, M = Tc * n;
      launch_gemm<kEpiBias>(A + (int64_t)s0 * n * K, K, M, 4 * Dp, K, m->w_ih[layer], m->bias[layer], w.P, s);
      launch_gemm<kEpiBias>(A + (int64_t)(S - s0 - Tc) * n * K, K, M, 4 * Dp, K, m->w_ih[layer] + (int64_t)4 * Dp * K, m->bias[layer] + 4 * Dp,
                            w.P + (int64_t)M * 4 * Dp, s);
      launch_rec(Dp / 64, grid, s, w.P, m->w_hh[layer], Y, w.cst, n, S, s0, Tc);
    }
  }
}

}  // namespace

extern "C" {

int64_t capamd_posit_workspace_bytes(const capamd_posit_model* m, int docs_per_microbatch, int Q, int L) {
  if (!shape_ok(m, Q, L) || docs_per_microbatch < 1 || docs_per_microbatch > (1 << 20)) return -1;
  return (int64_t)carve(docs_per_microbatch, up64(m->dim), Q, L, nullptr).bytes;
}

int capamd_posit_forward(const int64_t* q_ids, const float* q_idf, const int64_t* d_ids, const float* extras, const float* bm25, int B, int Q, int L,
                         const capamd_posit_model* m, int docs_per_microbatch, void* workspace, int64_t workspace_bytes, float* out,
                         float* features_out, float* stats_out, float* qctx_out, float* dctx_out, int* status, void* stream) {
  if (!q_ids || !q_idf || !d_ids || (!extras && !bm25) || !m || !workspace || !out || !status || !shape_ok(m, Q, L) || B < 0 ||
      docs_per_microbatch < 1 || docs_per_microbatch > (1 << 20))
    return CAPAMD_ERR_ARG;
  if (!m->emb || !m->q1_w || !m->q1_b || !m->wg_w || !m->wg_b) return CAPAMD_ERR_ARG;
  for (int i = 0; i < 2; ++i) {
    if (!m->w_ih[i] || !m->w_hh[i] || !m->bias[i]) return CAPAMD_ERR_ARG;
    if (!aligned16(m->w_ih[i]) || !aligned16(m->w_hh[i])) return CAPAMD_ERR_ALIGN;
  }
  if (B == 0) return CAPAMD_OK;
  const int D = m->dim, Dp = up64(D);
  const size_t front_lds = FrontLds(Q, D, Q + 2).bytes;
  const size_t pool_lds = (size_t)Q * 2 * D * 4 + (size_t)Q * 6 * 4;
  hipStream_t s = (hipStream_t)stream;
  return run_microbatches(
      B, docs_per_microbatch, workspace, workspace_bytes, [&](int64_t nb, void* base) { return carve(nb, Dp, Q, L, base); },
      [&](int64_t b0, int64_t nn, const Ws& w) {
        const int n = (int)nn;
        const int64_t* q = q_ids + b0 * Q;
        const int64_t* d = d_ids + b0 * L;
        const float* idf = q_idf + b0 * Q;
        hipLaunchKernelGGL(front_kernel, dim3((unsigned)n), dim3(256), front_lds, s, q, idf, d, Q, L, m->emb, m->vocab, D, Dp, m->pad, (int64_t)n, w.X,
                           w.QX, w.mcos, w.stats, status);
        encode(m, Dp, n, Q, w, w.QX, w.QY1, s);
        encode(m, Dp, n, L, w, w.X, w.Y1, s);
        hipLaunchKernelGGL(pool_kernel, dim3((unsigned)n), dim3(256), pool_lds, s, q, idf, d, Q, L, D, Dp, m->pad, (int64_t)n, w.X, w.QX, w.Y1, w.QY1,
                           w.mcos, w.mctx, w.stats, extras ? extras + b0 * 4 : nullptr, bm25 ? bm25 + b0 : nullptr, m->q1_w, m->q1_b, m->wg_w, m->wg_b,
                           out + b0, features_out ? features_out + b0 * Q * 6 : nullptr, stats_out ? stats_out + b0 * 3 : nullptr,
                           qctx_out ? qctx_out + b0 * Q * 2 * D : nullptr, dctx_out ? dctx_out + b0 * (int64_t)L * 2 * D : nullptr);
        return CAPAMD_OK;
      });
}

}  // extern "C"
