// DUET (reference capreolus/reranker/DUET.py: DUET_class.forward = LocalModel + DistributedModel) in fp32 throughout, two kernels per
// micro-batch of documents.  Q = 4 query terms, H = nfilters, M = lmhidden, NP = L - 101 pooled positions (= nhidden).
//   proj_kernel   one LANE per document term, the terms of the micro-batch laid end to end (a wave owns 64 of them): the (3, dim)
//                 convolution of d_conv1 is three per-token projections, P[t][j H + h] = sum_k W1[h][j][k] emb[d_t][k], so a row is read
//                 ONCE per document: in 32-float pieces (128 bytes, float4 per lane when dim % 4 == 0; asked for one piece ahead, into
//                 registers), 64 rows' pieces into the wave's LDS image (stride 36 floats: the b128 reads of a lane's own row are
//                 conflict-free); lane t then walks its piece with
//                 the weights of one k for all 3 H outputs as ONE wave-uniform run of W1^T [k][3 H padded to 16] (scalar loads, the fmaf's
//                 second operand a scalar register), the 16 NB accumulators in registers.  One fmaf chain per output in the order of k:
//                 a term's projections depend on its row alone.  Its floors are the fp32 fmaf rate (3 H dim per term) and the row gather
//                 (4 dim bytes per term); measured, the fixed cost around each piece is what bounds it.  Ids outside
//                 the table are rows of zeros, nothing is read for them.
//   doc_kernel    one workgroup per document.
//                 local model: the [Q, L] match matrix is never formed.  A byte per position holds which query terms equal the id (ids
//                 compared as they are, pads included); wave q walks it 64 positions at a time (ballot) and, for every match in ascending
//                 d, lanes h < H add idf_q x W^T[d][h] - one contiguous read of H floats.  Then Linear(4 H -> M), act, Linear(M -> 1), one
//                 wave per output unit, the 64 partial products added by the xor butterfly.
//                 query side: the 4 rows in LDS, the two windows' 2 H convolution outputs one wave each, max, q_ffw.
//                 document side, in tiles of 256 pooled positions (355 convolution positions): c = act(b + P0[t] + P1[t + 1] + P2[t + 2])
//                 into LDS; the sliding maximum of 100 by doubling - windows of 2, 4, .., 64 in six passes between two buffers, then
//                 max(w64[t], w64[t + 36]): 7 compares per output, exact; thread t then forms e[g] = act(b2 + W2[g] . p[:, t]) and adds
//                 W1[t] (q[g] e[g]) to its own H sums (tiles in ascending order).  The 256 threads' sums are added by the butterfly and
//                 then wave 0 .. 3 in order: every order is a function of the document alone - no float atomics, and a document's bits
//                 do not depend on its neighbours, the batch or the micro-batch.
// Limits (shape_ok): Q == 4, 2 <= H <= 32, 1 <= M <= 256, 1 <= dim <= 512, 103 <= L <= 8192, nhidden == L - 101, maxdoclen == L.
#include "capreolus_amd.h"
#include "workspace.h"
#include <math.h>
#include <type_traits>

namespace {

constexpr int kQ = 4, kPool = 100, kMaxH = 32, kMaxM = 256, kMaxDim = 512, kMinL = kPool + 3, kMaxL = 8192;
constexpr int kWaves = 4, kThreads = 64 * kWaves;
constexpr int kChunk = 32, kRowStride = kChunk + 4;                 // proj_kernel: floats of a row per piece, and between rows in LDS
constexpr int kTile = kThreads, kWd = kTile + kPool - 1, kStride = kWd + 2;      // doc_kernel: an odd stride between filter rows

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float act(float x, int tanh_) { return tanh_ ? tanhf(x) : fmaxf(x, 0.f); }

inline int up16(int n) { return (n + 15) / 16 * 16; }

// ---- stage 1: the three per-token projections ------------------------------------------------------------------------------------------
template <int NB, bool VEC4>
__global__ __launch_bounds__(kThreads) void proj_kernel(const int64_t* __restrict__ d_ids, int64_t ntok, const float* __restrict__ emb, int64_t V, int D,
                                                        const float* __restrict__ w1t, float* __restrict__ P, int* status) {
  constexpr int OP = 16 * NB;
  __shared__ __attribute__((aligned(16))) float tiles[kWaves][64 * kRowStride];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* tile = tiles[wave];
  const int64_t g = ((int64_t)blockIdx.x * kWaves + wave) * 64 + lane;
  long long my_id = -1;                                  // -1: behind the last term, or an id outside the table - a row of zeros
  if (g < ntok) {
    my_id = d_ids[g];
    if (my_id < 0 || my_id >= V) {
      atomicOr(status, CAPAMD_STATUS_DOC_ID_RANGE);
      my_id = -1;
    }
  }
  float acc[OP];
#pragma unroll
  for (int o = 0; o < OP; ++o) acc[o] = 0.f;
  // the pieces of the wave's 64 rows for the columns k0 .. k0 + 31, into registers: asked for one piece ahead, so that the trip to
  // memory runs under the arithmetic of the piece before
  constexpr int NR = VEC4 ? 8 : 32;
  typename std::conditional<VEC4, float4, float>::type nxt[NR];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if constexpr (VEC4) {
        const int tok = r * 8 + (lane >> 3), pc = 4 * (lane & 7);
        const long long id = __shfl(my_id, tok, 64);
        nxt[r] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (id >= 0 && k0 + pc < D) nxt[r] = *reinterpret_cast<const float4*>(emb + id * (int64_t)D + k0 + pc);
      } else {
        const int tok = r * 2 + (lane >> 5), pc = lane & 31;
        const long long id = __shfl(my_id, tok, 64);
        nxt[r] = (id >= 0 && k0 + pc < D) ? emb[id * (int64_t)D + k0 + pc] : 0.f;
      }
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < D; k0 += kChunk) {               // (the same trip count in every wave: the barriers below are uniform)
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if constexpr (VEC4)
        *reinterpret_cast<float4*>(tile + (r * 8 + (lane >> 3)) * kRowStride + 4 * (lane & 7)) = nxt[r];
      else
        tile[(r * 2 + (lane >> 5)) * kRowStride + (lane & 31)] = nxt[r];
    }
    __syncthreads();
    if (k0 + kChunk < D) fetch(k0 + kChunk);
    // (w1t has D rounded up to 32 rows, the ones behind D zeros like the piece's columns behind D: no test in the loop)
#pragma unroll 2
    for (int k4 = 0; k4 < kChunk / 4; ++k4) {
      const float4 x = *reinterpret_cast<const float4*>(tile + lane * kRowStride + 4 * k4);
      const float* w = w1t + (int64_t)(k0 + 4 * k4) * OP;
#pragma unroll
      for (int o = 0; o < OP; ++o) acc[o] = fmaf(w[o], x.x, acc[o]);
#pragma unroll
      for (int o = 0; o < OP; ++o) acc[o] = fmaf(w[OP + o], x.y, acc[o]);
#pragma unroll
      for (int o = 0; o < OP; ++o) acc[o] = fmaf(w[2 * OP + o], x.z, acc[o]);
#pragma unroll
      for (int o = 0; o < OP; ++o) acc[o] = fmaf(w[3 * OP + o], x.w, acc[o]);
    }
    __syncthreads();
  }
  if (g < ntok) {
    float4* dst = reinterpret_cast<float4*>(P + g * OP);
#pragma unroll
    for (int o = 0; o < OP; o += 4) dst[o / 4] = make_float4(acc[o], acc[o + 1], acc[o + 2], acc[o + 3]);
  }
}

template <int NB>
void launch_proj(bool vec4, int64_t ntok, hipStream_t s, const int64_t* d_ids, const float* emb, int64_t V, int D, const float* w1t, float* P, int* status) {
  const dim3 grid((unsigned)((ntok + kThreads - 1) / kThreads));
  if (vec4)
    hipLaunchKernelGGL((proj_kernel<NB, true>), grid, dim3(kThreads), 0, s, d_ids, ntok, emb, V, D, w1t, P, status);
  else
    hipLaunchKernelGGL((proj_kernel<NB, false>), grid, dim3(kThreads), 0, s, d_ids, ntok, emb, V, D, w1t, P, status);
}

// ---- stage 2: everything else, per document ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void doc_kernel(const int64_t* __restrict__ q_ids, const int64_t* __restrict__ d_ids, const float* __restrict__ idf,
                                                       const capamd_duet_model m, const float* __restrict__ P, int L, int OP, float* __restrict__ out,
                                                       float* __restrict__ parts, float* __restrict__ ev, int* status) {
  extern __shared__ __attribute__((aligned(16))) float dyn[];                 // [2][H][kStride]: the two buffers of the sliding maximum
  __shared__ unsigned char mask[kMaxL];                                        // bit q: d_ids[d] == q_ids[q]
  __shared__ float qrow[kQ * kMaxDim];                                         // the query's rows, back to back
  __shared__ float x[kQ * kMaxH], hid[kMaxM], qc[2 * kMaxH], qv[kMaxH], red[kWaves][kMaxH], fin[kMaxH];
  __shared__ float lm_s;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t b = blockIdx.x;
  const int H = m.nfilters, M = m.lmhidden, D = m.dim, tanh_ = m.activation;
  const int NP = L - (kPool + 1), NC = L - 2;
  const int64_t* qi = q_ids + b * kQ;
  const int64_t* di = d_ids + b * L;

  // ---- local model ----
  const int64_t q0 = qi[0], q1 = qi[1], q2 = qi[2], q3 = qi[3];
  for (int d = tid; d < L; d += kThreads) {
    const int64_t id = di[d];
    mask[d] = (unsigned char)((id == q0) | ((id == q1) << 1) | ((id == q2) << 2) | ((id == q3) << 3));
  }
  // the query's rows for the distributed model (an id outside the table: a row of zeros)
  for (int i = 0; i < kQ; ++i) {
    const int64_t id = qi[i];
    const bool ok = id >= 0 && id < m.vocab;
    if (!ok && tid == 0) atomicOr(status, CAPAMD_STATUS_QUERY_ID_RANGE);
    const float* e = m.emb + (ok ? id : 0) * (int64_t)D;
    for (int k = tid; k < D; k += kThreads) qrow[i * D + k] = ok ? e[k] : 0.f;
  }
  __syncthreads();
  {
    const int q = wave;                                  // kWaves == kQ: one wave per query term
    const float w = m.idfweight ? idf[b * kQ + q] : 1.f;
    float a = 0.f;
    for (int d0 = 0; d0 < L; d0 += 64) {
      const int d = d0 + lane;
      unsigned long long hits = __ballot(d < L && ((mask[d] >> q) & 1));
      while (hits) {                                     // ascending d
        const int dd = d0 + __builtin_ctzll(hits);
        hits &= hits - 1;
        if (lane < H) a = fmaf(m.lm_wt[(int64_t)dd * H + lane], w, a);
      }
    }
    if (lane < H) x[lane * kQ + q] = act(a + m.lm_b[lane], tanh_);
  }
  __syncthreads();
  for (int o = wave; o < M; o += kWaves) {
    const float* wr = m.lm_w0 + (int64_t)o * (kQ * H);
    float s = 0.f;
    for (int k = lane; k < kQ * H; k += 64) s = fmaf(wr[k], x[k], s);
    s = wave_sum(s);
    if (lane == 0) hid[o] = act(s + m.lm_b0[o], tanh_);
  }
  // ---- distributed model, query side: outputs (window w, filter h) = w H + h, one wave each ----
  for (int o = wave; o < 2 * H; o += kWaves) {
    const int w = o >= H, h = o - w * H;
    const float* wr = m.q_w + (int64_t)h * 3 * D;
    const float* xr = qrow + w * D;
    float s = 0.f;
#pragma unroll 4
    for (int k = lane; k < 3 * D; k += 64) s = fmaf(wr[k], xr[k], s);
    s = wave_sum(s);
    if (lane == 0) qc[o] = act(s + m.q_b[h], tanh_);
  }
  __syncthreads();
  if (wave == 0) {
    float s = 0.f;
    for (int k = lane; k < M; k += 64) s = fmaf(m.lm_w3[k], hid[k], s);
    s = wave_sum(s);
    if (lane == 0) lm_s = s + m.lm_b3[0];
  } else if (wave == 1 && lane < H) {
    float s = m.qf_b[lane];
    for (int h = 0; h < H; ++h) s = fmaf(m.qf_w[lane * H + h], fmaxf(qc[h], qc[H + h]), s);
    qv[lane] = s;
    if (ev) ev[(b * H + lane) * (int64_t)(NP + 1)] = s;
  }
  __syncthreads();

  // ---- distributed model, document side ----
  const float* Pd = P + b * (int64_t)L * OP;
  float facc[kMaxH];
#pragma unroll
  for (int g = 0; g < kMaxH; ++g) facc[g] = 0.f;
  for (int t0 = 0; t0 < NP; t0 += kTile) {
    float* a = dyn;
    float* o = dyn + H * kStride;
#pragma unroll 4
    for (int i = tid; i < H * kWd; i += kThreads) {      // h fastest: a term's H projections are contiguous; four trips to memory at once
      const int u = i / H, h = i - u * H, t = t0 + u;
      const float* p = Pd + (int64_t)(t < NC ? t : NC - 1) * OP;                 // (no branch around the reads: they go out together)
      const float v = act(((m.d_b1[h] + p[h]) + p[OP + H + h]) + p[2 * OP + 2 * H + h], tanh_);
      a[h * kStride + u] = t < NC ? v : -INFINITY;       // behind the last convolution position: never the maximum of a window in use
    }
    __syncthreads();
    for (int s = 1; s < 64; s <<= 1) {                   // windows of 2 s from windows of s; six passes, the last leaves windows of 64 in `a`
      for (int i = tid; i < H * kWd; i += kThreads) {
        const int h = i / kWd, u = i - h * kWd;
        float v = a[h * kStride + u];
        if (u + s < kWd) v = fmaxf(v, a[h * kStride + u + s]);
        o[h * kStride + u] = v;
      }
      __syncthreads();
      float* sw = a;
      a = o;
      o = sw;
    }
    const int t = t0 + tid;
    if (t < NP) {
      // windows of 64 are whole up to u = kWd - 64 = 291 >= 255 + 36
      for (int h = 0; h < H; ++h) {
        const float pv = fmaxf(a[h * kStride + tid], a[h * kStride + tid + (kPool - 64)]);
        o[h * kStride + tid] = pv;                       // (column tid of `o` is this thread's alone)
        if (ev) ev[(b * H + h) * (int64_t)(NP + 1) + 1 + t] = pv;
      }
      const float wt = m.f1_w[t];
#pragma unroll
      for (int g = 0; g < kMaxH; ++g)
        if (g < H) {
          float s = m.d_b2[g];
          for (int h = 0; h < H; ++h) s = fmaf(m.d_w2[g * H + h], o[h * kStride + tid], s);
          facc[g] = fmaf(wt, qv[g] * act(s, tanh_), facc[g]);
        }
    }
    __syncthreads();
  }
#pragma unroll
  for (int g = 0; g < kMaxH; ++g)
    if (g < H) {
      const float s = wave_sum(facc[g]);
      if (lane == 0) red[wave][g] = s;
    }
  __syncthreads();
  if (tid < H) fin[tid] = act((((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid]) + m.f1_b[0], tanh_);
  __syncthreads();
  if (tid == 0) {
    float dm = m.f2_b[0];
    for (int g = 0; g < H; ++g) dm = fmaf(m.f2_w[g], fin[g], dm);
    out[b] = lm_s + dm;
    if (parts) {
      parts[2 * b] = lm_s;
      parts[2 * b + 1] = dm;
    }
  }
}

bool shape_ok(const capamd_duet_model* m, int Q, int L) {
  if (!m || Q != kQ || L < kMinL || L > kMaxL) return false;
  if (m->nfilters < 2 || m->nfilters > kMaxH || m->lmhidden < 1 || m->lmhidden > kMaxM || m->dim < 1 || m->dim > kMaxDim || m->vocab < 1) return false;
  return m->maxdoclen == L && m->nhidden == L - (kPool + 1) && (m->activation == 0 || m->activation == 1);
}

struct Ws {
  float* P;
  size_t bytes;
};

Ws carve(int64_t nb, int L, int OP, void* base) {
  Carver c(base);
  return {c.take((size_t)nb * L * OP), c.bytes()};
}

}  // namespace

extern "C" {

int64_t capamd_duet_workspace_bytes(const capamd_duet_model* m, int docs_per_microbatch, int Q, int L) {
  if (!shape_ok(m, Q, L) || docs_per_microbatch < 1) return -1;
  return (int64_t)carve(docs_per_microbatch, L, up16(3 * m->nfilters), nullptr).bytes;
}

int capamd_duet_forward(const int64_t* q_ids, const int64_t* d_ids, const float* idf, int B, int Q, int L, const capamd_duet_model* m,
                        int docs_per_microbatch, void* workspace, int64_t workspace_bytes, float* out, float* parts_out, float* evidence_out, int* status,
                        void* stream) {
  if (!q_ids || !d_ids || !m || !workspace || !out || !status || !shape_ok(m, Q, L) || B < 0 || docs_per_microbatch < 1) return CAPAMD_ERR_ARG;
  if (m->idfweight && !idf) return CAPAMD_ERR_ARG;
  const float* need[19] = {m->emb,  m->lm_wt, m->lm_b, m->lm_w0, m->lm_b0, m->lm_w3, m->lm_b3, m->q_w,  m->q_b, m->qf_w,
                           m->qf_b, m->d_w1t, m->d_b1, m->d_w2,  m->d_b2,  m->f1_w,  m->f1_b,  m->f2_w, m->f2_b};
  for (const float* p : need)
    if (!p) return CAPAMD_ERR_ARG;
  if (!aligned16(m->emb) || !aligned16(m->d_w1t)) return CAPAMD_ERR_ALIGN;
  if (B == 0) return CAPAMD_OK;
  const int H = m->nfilters, OP = up16(3 * H), NB = OP / 16, NP = L - (kPool + 1);
  const bool vec4 = m->dim % 4 == 0;
  const size_t doc_lds = (size_t)2 * H * kStride * sizeof(float);
  hipStream_t s = (hipStream_t)stream;
  return run_microbatches(
      B, docs_per_microbatch, workspace, workspace_bytes, [&](int64_t n, void* base) { return carve(n, L, OP, base); },
      [&](int64_t b0, int64_t n, const Ws& w) {
        // (beside the kernel's 19 KB of fixed arrays, H > 16 passes the 64 KiB a kernel gets without asking: 110 KB at H = 32)
        if (b0 == 0 && doc_lds > 40 * 1024 &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(doc_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)doc_lds) != hipSuccess)
          return CAPAMD_ERR_LAUNCH;
        const int64_t ntok = n * L;
        const int64_t* d = d_ids + b0 * L;
        switch (NB) {
          case 1: launch_proj<1>(vec4, ntok, s, d, m->emb, m->vocab, m->dim, m->d_w1t, w.P, status); break;
          case 2: launch_proj<2>(vec4, ntok, s, d, m->emb, m->vocab, m->dim, m->d_w1t, w.P, status); break;
          case 3: launch_proj<3>(vec4, ntok, s, d, m->emb, m->vocab, m->dim, m->d_w1t, w.P, status); break;
          case 4: launch_proj<4>(vec4, ntok, s, d, m->emb, m->vocab, m->dim, m->d_w1t, w.P, status); break;
          case 5: launch_proj<5>(vec4, ntok, s, d, m->emb, m->vocab, m->dim, m->d_w1t, w.P, status); break;
          default: launch_proj<6>(vec4, ntok, s, d, m->emb, m->vocab, m->dim, m->d_w1t, w.P, status); break;
        }
        hipLaunchKernelGGL(doc_kernel, dim3((unsigned)n), dim3(kThreads), doc_lds, s, q_ids + b0 * kQ, d, idf ? idf + b0 * kQ : nullptr, *m, w.P, L, OP,
                           out + b0, parts_out ? parts_out + 2 * b0 : nullptr,
                           evidence_out ? evidence_out + b0 * H * (int64_t)(NP + 1) : nullptr, status);
        return CAPAMD_OK;
      });
}

}  // extern "C"
