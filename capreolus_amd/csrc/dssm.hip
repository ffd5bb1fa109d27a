// DSSM and CDSSM (reference capreolus/reranker/DSSM.py, CDSSM.py), fp32 throughout.  Neither model looks at a (query, document) pair before
// the final cosine: each side runs through a tower on its own, once per distinct row, and pairs are scored from the tower outputs.
//   cdssm_tower_kernel  one workgroup per id row, one WAVE per window of W terms: the window's W embedding rows (their ids fetched one window
//                       ahead) are read once, coalesced (float4 when dim % 4 == 0), into the wave's LDS image of W dim floats (ids outside the table and the appended
//                       pads of the last window as zeros, nothing read for them); lane t then forms, per filter, the fixed chain
//                       a = b_f; a = fmaf(w[f][j], x[t + j], a), j = 0 .. nkernel - 1, and keeps max(acc[t], relu(a)) in the wave's own
//                       accumulator row in LDS.  A whole window of zeros (T % W == 0 appends one) is the closed form max_f relu(b_f),
//                       the accumulators' initial value.  The four rows are merged by max at the end: max is exact, so the result
//                       does not depend on which wave saw which window.
//   dssm_tower_kernel   one workgroup per bag: wave w takes the bag's entries w, w + 4, ... in order, lane l the columns l + 64 u of
//                       the padded row W1^T[idx] (a whole-row gather, one 256-byte piece per wave-instruction, the rows of several
//                       entries in flight), a = fmaf(val, row, a) in the order of the entries;
//                       the four partial sums are added as ((p0 + p1) + p2) + p3 onto the bias: the order is a function of the bag
//                       alone, no float atomics.  ReLU, then the later layers from LDS, one wave per output unit, its 64 partial dot
//                       products added by the xor butterfly.
//   cos_sigmoid_kernel  one wave per pair: |q|, |d| (sum of squares by the butterfly, sqrtf, + 1e-7), then the dot product of the two
//                       normalised rows in the same lane order, sigmoid.  A pair's bits depend on its two rows alone.
#include "capreolus_amd.h"
#include "cos_front.h"
#include <math.h>

namespace {

constexpr int kMaxDim = 512, kMaxWindow = 8, kMaxSpan = 4096, kMaxKernel = 16, kMaxFilter = 16;
constexpr int kWaves = 4, kThreads = 64 * kWaves;
constexpr int kMaxLayers = 4, kMaxWidth = 512;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- CDSSM tower -----------------------------------------------------------------------------------------------------------------------
// dynamic LDS, floats: win [kWaves][S4] | acc [kWaves][R] | wgt [F][nk] | bias [F];  S = W dim, S4 = S rounded up to 4
struct CdssmLds {
  int S4, R;
  size_t acc, wgt, bias, bytes;
  __host__ __device__ CdssmLds(int S, int nk, int F)
      : S4((S + 3) / 4 * 4), R(S - nk + 1), acc((size_t)kWaves * S4), wgt(acc + (size_t)kWaves * R), bias(wgt + (size_t)F * nk),
        bytes((bias + F) * 4) {}
};

template <bool VEC4>
__global__ __launch_bounds__(kThreads) void cdssm_tower_kernel(const int64_t* __restrict__ ids, int T, const float* __restrict__ emb, int64_t V,
                                                               int D, int W, const float* __restrict__ conv_w, const float* __restrict__ conv_b,
                                                               int nk, int F, int bad_bit, float* __restrict__ rep, int* status) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int S = W * D;
  const CdssmLds at(S, nk, F);
  const int R = at.R;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  float* win = lds + (size_t)wave * at.S4;
  float* acc = lds + at.acc + (size_t)wave * R;
  float* wgt = lds + at.wgt;
  float* bias = lds + at.bias;
  const int64_t n = blockIdx.x;
  const int64_t* row_ids = ids + n * T;
  for (int k = tid; k < F * nk; k += kThreads) wgt[k] = conv_w[k];
  for (int k = tid; k < F; k += kThreads) bias[k] = conv_b[k];
  // an appended window of zeros gives max_f relu(b_f) at every position; every other window gives values >= 0
  float init = 0.f;
  if (T % W == 0)
    for (int f = 0; f < F; ++f) init = fmaxf(init, conv_b[f]);
  for (int t = lane; t < R; t += 64) acc[t] = init;
  const int windows = (T + W - 1) / W;                   // the windows that hold a term of the row
  // lane r < W holds the id of row r of the wave's window, fetched one window ahead of its use; -1: an appended pad or an id outside
  // the table - a row of zeros either way, for which nothing is read
  auto window_id = [&](int i) -> long long {
    const long long p = (long long)i * W + lane;
    long long id = -1;
    if (lane < W && i < windows && p < T) {
      id = row_ids[p];
      if (id < 0 || id >= V) {
        atomicOr(status, bad_bit);
        id = -1;
      }
    }
    return id;
  };
  long long next_id = window_id(wave);
  for (int i0 = 0; i0 < windows; i0 += kWaves) {         // (the same trip count in every wave: the barriers below are uniform)
    const int i = i0 + wave;
    const long long cur_id = next_id;
    next_id = window_id(i + kWaves);
    if (i < windows) {
      for (int r = 0; r < W; ++r) {
        const long long id = __shfl(cur_id, r, 64);
        float* dst = win + r * D;
        if (VEC4) {
          const float4* e = reinterpret_cast<const float4*>(emb + (id < 0 ? 0 : id) * (int64_t)D);
          float4* d4 = reinterpret_cast<float4*>(dst);
          for (int k = lane; k < D / 4; k += 64) d4[k] = id < 0 ? make_float4(0.f, 0.f, 0.f, 0.f) : e[k];
        } else {
          const float* e = emb + (id < 0 ? 0 : id) * (int64_t)D;
          for (int k = lane; k < D; k += 64) dst[k] = id < 0 ? 0.f : e[k];
        }
      }
    }
    __syncthreads();
    if (i < windows) {
      for (int t = lane; t < R; t += 64) {
        float m = acc[t];
        for (int f = 0; f < F; ++f) {
          float a = bias[f];
          const float* wf = wgt + f * nk;
          for (int j = 0; j < nk; ++j) a = fmaf(wf[j], win[t + j], a);
          m = fmaxf(m, a);                               // (acc >= 0 already: max(acc, relu(a)) = max(acc, a))
        }
        acc[t] = m;
      }
    }
    __syncthreads();
  }
  __syncthreads();
  const float* a0 = lds + at.acc;
  for (int t = tid; t < R; t += kThreads) rep[n * R + t] = fmaxf(fmaxf(a0[t], a0[R + t]), fmaxf(a0[2 * R + t], a0[3 * R + t]));
}

template <bool VEC4>
int launch_cdssm(const CdssmLds& at, int64_t N, hipStream_t s, const int64_t* ids, int T, const float* emb, int64_t V, int D, int W, const float* conv_w,
                 const float* conv_b, int nk, int F, int bad_bit, float* rep, int* status) {
  // (the widest geometry, W dim = 4096, takes 128 KiB: more than the 64 KiB a kernel gets without asking)
  if (at.bytes > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(cdssm_tower_kernel<VEC4>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   (int)at.bytes) != hipSuccess)
    return CAPAMD_ERR_LAUNCH;
  hipLaunchKernelGGL(cdssm_tower_kernel<VEC4>, dim3((unsigned)N), dim3(kThreads), at.bytes, s, ids, T, emb, V, D, W, conv_w, conv_b, nk, F, bad_bit, rep,
                     status);
  return hipGetLastError() == hipSuccess ? CAPAMD_OK : CAPAMD_ERR_LAUNCH;
}

// ---- DSSM tower ------------------------------------------------------------------------------------------------------------------------
struct DssmDims {
  int layers, h1p;
  int width[kMaxLayers];
};

// NUMAX: the 64-float pieces of a padded row a lane may hold (1: the widths up to 64, the reference's default 56 among them; 8: any width).
// The rows of kRows entries are in flight at once: an entry's row is one dependent trip to memory, and a wave has nothing else to do.
template <int NUMAX>
__global__ __launch_bounds__(kThreads) void dssm_tower_kernel(const int64_t* __restrict__ indptr, const int* __restrict__ idx, const float* __restrict__ val,
                                                              int64_t nnz, const float* __restrict__ w1t, const float* __restrict__ b1,
                                                              const float* __restrict__ w2, const float* __restrict__ b2, const float* __restrict__ w3,
                                                              const float* __restrict__ b3, const float* __restrict__ w4, const float* __restrict__ b4,
                                                              int64_t nvocab, DssmDims dm, int bad_bit, float* __restrict__ rep, int* status) {
  constexpr int kRows = NUMAX == 1 ? 8 : 4;
  __shared__ float part[kWaves][kMaxWidth];
  __shared__ float act[2][kMaxWidth];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t n = blockIdx.x;
  // an indptr pair that decreases or leaves [0, nnz] is clamped: nothing outside idx / val is read
  const int64_t raw_lo = indptr[n], raw_hi = indptr[n + 1];
  int64_t lo = raw_lo < 0 ? 0 : (raw_lo > nnz ? nnz : raw_lo);
  int64_t hi = raw_hi < lo ? lo : (raw_hi > nnz ? nnz : raw_hi);
  if ((lo != raw_lo || hi != raw_hi) && tid == 0) atomicOr(status, CAPAMD_STATUS_BAG_RANGE);
  const int64_t len = hi - lo;
  const int64_t mine = len > wave ? (len - wave + kWaves - 1) / kWaves : 0;      // this wave's entries: lo + wave + 4 e
  const int NU = dm.h1p >> 6;
  float a[NUMAX];
#pragma unroll
  for (int u = 0; u < NUMAX; ++u) a[u] = 0.f;
  for (int64_t base = 0; base < mine; base += 64) {
    // lane e of the wave fetches the wave's entry base + e; -1: no entry (behind the bag's end) or an index outside the table (skipped)
    const int64_t e = base + lane;
    int my_idx = -1;
    float my_val = 0.f;
    if (e < mine) {
      const int64_t k = lo + wave + kWaves * e;
      my_idx = idx[k];
      my_val = val[k];
      if (my_idx < 0 || my_idx >= nvocab) {
        atomicOr(status, bad_bit);
        my_idx = -1;
      }
    }
    const int m = mine - base < 64 ? (int)(mine - base) : 64;
    for (int j0 = 0; j0 < m; j0 += kRows) {              // (64 is a multiple of kRows: j0 + k stays a lane of the wave)
      int id[kRows];
      float v[kRows], r[kRows][NUMAX];
#pragma unroll
      for (int k = 0; k < kRows; ++k) {
        id[k] = __shfl(my_idx, j0 + k, 64);
        v[k] = __shfl(my_val, j0 + k, 64);
        const float* row = w1t + (int64_t)(id[k] < 0 ? 0 : id[k]) * dm.h1p + lane;
#pragma unroll
        for (int u = 0; u < NUMAX; ++u) r[k][u] = (id[k] >= 0 && u < NU) ? row[64 * u] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < kRows; ++k)                    // added in the order of the entries, whatever came back first
        if (id[k] >= 0) {
#pragma unroll
          for (int u = 0; u < NUMAX; ++u) a[u] = fmaf(v[k], r[k][u], a[u]);
        }
    }
  }
#pragma unroll
  for (int u = 0; u < NUMAX; ++u)
    if (u < NU) part[wave][lane + 64 * u] = a[u];
  __syncthreads();
  int h = dm.width[0];
  for (int c = tid; c < h; c += kThreads) act[0][c] = fmaxf(b1[c] + (((part[0][c] + part[1][c]) + part[2][c]) + part[3][c]), 0.f);
  __syncthreads();
  int cur = 0;
  for (int l = 1; l < dm.layers; ++l) {
    const float* w = l == 1 ? w2 : (l == 2 ? w3 : w4);
    const float* b = l == 1 ? b2 : (l == 2 ? b3 : b4);
    const int ho = dm.width[l];
    for (int o = wave; o < ho; o += kWaves) {
      const float* wr = w + (int64_t)o * h;
      float s = 0.f;
      for (int k = lane; k < h; k += 64) s = fmaf(wr[k], act[cur][k], s);
      s = wave_sum(s);
      if (lane == 0) act[cur ^ 1][o] = fmaxf(s + b[o], 0.f);
    }
    __syncthreads();
    cur ^= 1;
    h = ho;
  }
  for (int c = tid; c < h; c += kThreads) rep[n * h + c] = act[cur][c];
}

// ---- cosine + sigmoid of pairs ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void cos_sigmoid_kernel(const float* __restrict__ qrep, const float* __restrict__ drep,
                                                               const int* __restrict__ pair_q, const int* __restrict__ pair_d, int64_t Nq, int64_t Nd,
                                                               int64_t n_pairs, int R, float* __restrict__ out, int* status) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * kWaves + wave;
  if (i >= n_pairs) return;
  int64_t iq = pair_q ? pair_q[i] : i, id = pair_d ? pair_d[i] : i;
  const bool okq = iq >= 0 && iq < Nq, okd = id >= 0 && id < Nd;       // a row outside its table counts as a zero row
  if (lane == 0 && !okq) atomicOr(status, CAPAMD_STATUS_QUERY_ID_RANGE);
  if (lane == 0 && !okd) atomicOr(status, CAPAMD_STATUS_DOC_ID_RANGE);
  const float* q = qrep + (okq ? iq : 0) * R;
  const float* d = drep + (okd ? id : 0) * R;
  float qq = 0.f, dd = 0.f;
  for (int t = lane; t < R; t += 64) {
    const float x = okq ? q[t] : 0.f, y = okd ? d[t] : 0.f;
    qq = fmaf(x, x, qq);
    dd = fmaf(y, y, dd);
  }
  const float nq = sqrtf(wave_sum(qq)) + 1e-7f, nd = sqrtf(wave_sum(dd)) + 1e-7f;
  float dot = 0.f;
  for (int t = lane; t < R; t += 64) {
    const float x = okq ? q[t] : 0.f, y = okd ? d[t] : 0.f;
    dot = fmaf(x / nq, y / nd, dot);
  }
  dot = wave_sum(dot);
  if (lane == 0) out[i] = sigmoidf_(dot);
}

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int side_bit(int side) { return side == 0 ? CAPAMD_STATUS_QUERY_ID_RANGE : CAPAMD_STATUS_DOC_ID_RANGE; }

}  // namespace

extern "C" {

int capamd_cdssm_tower(const int64_t* ids, int64_t N, int T, const float* emb, int64_t vocab, int dim, int windowsize, const float* conv_w,
                       const float* conv_b, int nkernel, int nfilter, int side, float* rep, int* status, void* stream) {
  if (!ids || !emb || !conv_w || !conv_b || !rep || !status) return CAPAMD_ERR_ARG;
  if (N < 0 || N > 0x7fffffffLL || T < 1 || vocab < 1 || dim < 1 || dim > kMaxDim || windowsize < 1 || windowsize > kMaxWindow) return CAPAMD_ERR_ARG;
  const int S = windowsize * dim;
  if (S > kMaxSpan || nkernel < 1 || nkernel > kMaxKernel || nkernel > S || nfilter < 1 || nfilter > kMaxFilter) return CAPAMD_ERR_ARG;
  if (side != 0 && side != 1) return CAPAMD_ERR_ARG;
  if (!aligned(ids, 8) || !aligned(emb, 16) || !aligned(conv_w, 4) || !aligned(conv_b, 4) || !aligned(rep, 4) || !aligned(status, 4)) return CAPAMD_ERR_ALIGN;
  if (N == 0) return CAPAMD_OK;
  const CdssmLds at(S, nkernel, nfilter);
  hipStream_t s = (hipStream_t)stream;
  if (dim % 4 == 0) return launch_cdssm<true>(at, N, s, ids, T, emb, vocab, dim, windowsize, conv_w, conv_b, nkernel, nfilter, side_bit(side), rep, status);
  return launch_cdssm<false>(at, N, s, ids, T, emb, vocab, dim, windowsize, conv_w, conv_b, nkernel, nfilter, side_bit(side), rep, status);
}

int capamd_dssm_tower(const int64_t* indptr, const int* idx, const float* val, int64_t N, int64_t nnz, const capamd_dssm_model* m, int side, float* rep,
                      int* status, void* stream) {
  if (!indptr || !m || !rep || !status || N < 0 || N > 0x7fffffffLL || nnz < 0 || (nnz > 0 && (!idx || !val))) return CAPAMD_ERR_ARG;
  if (m->layers < 1 || m->layers > kMaxLayers || m->nvocab < 1 || m->nvocab > 0x7fffffffLL || !m->w1t || !m->b1) return CAPAMD_ERR_ARG;
  if (side != 0 && side != 1) return CAPAMD_ERR_ARG;
  DssmDims dm;
  dm.layers = m->layers;
  for (int l = 0; l < kMaxLayers; ++l) {
    dm.width[l] = l < m->layers ? m->width[l] : 0;
    if (l < m->layers && (m->width[l] < 1 || m->width[l] > kMaxWidth)) return CAPAMD_ERR_ARG;
    if (l >= 1 && l < m->layers && (!m->w[l - 1] || !m->b[l - 1])) return CAPAMD_ERR_ARG;
  }
  dm.h1p = (dm.width[0] + 63) / 64 * 64;
  if (!aligned(indptr, 8) || !aligned(idx, 4) || !aligned(val, 4) || !aligned(m->w1t, 16) || !aligned(m->b1, 4) || !aligned(rep, 4) || !aligned(status, 4))
    return CAPAMD_ERR_ALIGN;
  for (int l = 1; l < m->layers; ++l)
    if (!aligned(m->w[l - 1], 4) || !aligned(m->b[l - 1], 4)) return CAPAMD_ERR_ALIGN;
  if (N == 0) return CAPAMD_OK;
  if (dm.h1p == 64)
    hipLaunchKernelGGL(dssm_tower_kernel<1>, dim3((unsigned)N), dim3(kThreads), 0, (hipStream_t)stream, indptr, idx, val, nnz, m->w1t, m->b1, m->w[0],
                       m->b[0], m->w[1], m->b[1], m->w[2], m->b[2], m->nvocab, dm, side_bit(side), rep, status);
  else
    hipLaunchKernelGGL(dssm_tower_kernel<kMaxWidth / 64>, dim3((unsigned)N), dim3(kThreads), 0, (hipStream_t)stream, indptr, idx, val, nnz, m->w1t, m->b1,
                       m->w[0], m->b[0], m->w[1], m->b[1], m->w[2], m->b[2], m->nvocab, dm, side_bit(side), rep, status);
  return hipGetLastError() == hipSuccess ? CAPAMD_OK : CAPAMD_ERR_LAUNCH;
}

int capamd_cos_sigmoid_pairs(const float* qrep, const float* drep, const int* pair_q, const int* pair_d, int64_t Nq, int64_t Nd, int64_t n_pairs, int R,
                             float* out, int* status, void* stream) {
  if (!qrep || !drep || !out || !status || Nq < 1 || Nd < 1 || n_pairs < 0 || R < 1) return CAPAMD_ERR_ARG;
  if ((!pair_q && n_pairs > Nq) || (!pair_d && n_pairs > Nd)) return CAPAMD_ERR_ARG;
  if (!aligned(qrep, 4) || !aligned(drep, 4) || !aligned(pair_q, 4) || !aligned(pair_d, 4) || !aligned(out, 4) || !aligned(status, 4)) return CAPAMD_ERR_ALIGN;
  if (n_pairs == 0) return CAPAMD_OK;
  const int64_t blocks = (n_pairs + kWaves - 1) / kWaves;
  if (blocks > 0x7fffffffLL) return CAPAMD_ERR_ARG;
  hipLaunchKernelGGL(cos_sigmoid_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, qrep, drep, pair_q, pair_d, Nq, Nd, n_pairs, R,
                     out, status);
  return hipGetLastError() == hipSuccess ? CAPAMD_OK : CAPAMD_ERR_LAUNCH;
}

}  // extern "C"
