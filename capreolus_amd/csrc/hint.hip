// HINT (reference capreolus/reranker/HINT.py: HiNT_main.test_forward -> HiNT.forward) in fp32 throughout, three kernels per micro-batch
// of documents (P = L / 100 windows of 100 terms each; the terms behind P x 100 are never read):
//   front_kernel   one workgroup per document: the Q query rows normalised into LDS (q / (|q| + 1e-7)), X_i = Ws q_i + b; then 16 lanes
//                  per document term read its row (once per four query terms) and form |d|, Y_j = Ws d_j + b and the Q cosines dot(qn_i, d) / (|d| + 1e-7),
//                  and from the ids alone two bit rows over the query terms: eq (q_i == d_j) and mk (q_i == 0 and d_j == 0, the
//                  reference's both-pad mask: where d_j == 0 it IS the eq row).  Everything is written window-transposed,
//                  [column j][window w = doc * P + p], so that the lanes of the next kernel read consecutive words.
//   gru_kernel     the spatial GRU: one LANE per chain (window x {xor, cos}), one grid row per direction, so a wave's lanes share one
//                  GRUCell2d's 162 weights (read once per wave, held in registers).  The recurrence h[i][j] <- h[i-1][j], h[i][j-1],
//                  h[i-1][j-1] is walked column by column (j outside, the Q query rows inside): every cell sees the same three neighbours and does the same
//                  arithmetic as the reference's row-by-row walk, and what has to be remembered is one column (Q x 2 floats per lane,
//                  in LDS, lane-interleaved: conflict-free) instead of one row of 100.  The reversed direction (GRU2d3 on matrix_inv)
//                  is the index map (Q-1-i, 99-j) on the same buffers.  Only the last cell's 2-vector is written.
//   head_kernel    one wave per document: the bidirectional LSTM over the P windows from zero state (lane = gate x direction),
//                  forward + backward, tanh(Wv .), the sorted top-kmax of the 2P values per hidden unit (by rank counting), fc.
// Each document's result is independent of the other documents and of the micro-batch size, bit for bit.
#include "capreolus_amd.h"
#include "cos_front.h"
#include "workspace.h"
#include <math.h>

namespace {

constexpr int kWin = 100;        // the reference's hard-coded window width
constexpr int kMaxQ = 32, kMaxP = 64, kMaxDim = 512, kMaxK = 32, kH = 6, kEv = 8;

struct Ws {
  float *Y, *cos, *X, *ev;
  uint32_t *eq, *mk;
  size_t bytes;
};

// the window-transposed inputs of the GRU for nb documents, and its evidence
Ws carve(int64_t nb, int Q, int P, void* base) {
  const int64_t NW = nb * P;
  Carver c(base);
  return {c.take(kWin * NW), c.take((size_t)(kWin * NW) * Q), c.take(nb * Q), c.take(NW * kEv), c.take<uint32_t>(kWin * NW), c.take<uint32_t>(kWin * NW),
          c.bytes()};
}

// One pass of a 16-lane group over a document term's row e against the query rows i0 .. i0 + 3 (normalised, in LDS): their cosines to
// cos_out[i * NW].  FIRST: also the row's norm (returned as |d| + 1e-7, which the later passes are handed) and Ws d + b to *y_out.
template <bool FIRST>
__device__ __forceinline__ float term_pass(const float* __restrict__ e, bool ok, const float* qn, int i0, int Q, int D, int l,
                                           const float* __restrict__ ws_w, float bias, float* __restrict__ y_out, float* __restrict__ cos_out,
                                           int64_t NW, float den) {
  const int n = Q - i0 < 4 ? Q - i0 : 4;
  const float* q0 = qn + i0 * D;
  const float* q1 = qn + (i0 + (n > 1 ? 1 : 0)) * D;
  const float* q2 = qn + (i0 + (n > 2 ? 2 : 0)) * D;
  const float* q3 = qn + (i0 + (n > 3 ? 3 : 0)) * D;
  float ss = 0.f, ys = 0.f, a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (int k = l; k < D; k += 16) {
    const float v = ok ? e[k] : 0.f;
    if (FIRST) {
      ss = fmaf(v, v, ss);
      ys = fmaf(v, ws_w[k], ys);
    }
    a0 = fmaf(v, q0[k], a0);
    a1 = fmaf(v, q1[k], a1);
    a2 = fmaf(v, q2[k], a2);
    a3 = fmaf(v, q3[k], a3);
  }
  a0 = group16_sum(a0);
  a1 = group16_sum(a1);
  a2 = group16_sum(a2);
  a3 = group16_sum(a3);
  if (FIRST) {
    ss = group16_sum(ss);
    ys = group16_sum(ys);
    den = sqrtf(ss) + 1e-7f;
    if (l == 0) *y_out = ys + bias;
  }
  if (l < n) {
    const float a = l == 0 ? a0 : l == 1 ? a1 : l == 2 ? a2 : a3;
    cos_out[l * NW] = a / den;
  }
  return den;
}

// ---- stage 1 ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void front_kernel(const int64_t* __restrict__ q_ids, const int64_t* __restrict__ d_ids, int Q, int L, int P,
                                                    const float* __restrict__ emb, int64_t V, int D, const float* __restrict__ ws_w,
                                                    const float* __restrict__ ws_b, int64_t NW, float* __restrict__ Yt, float* __restrict__ cost,
                                                    uint32_t* __restrict__ eqt, uint32_t* __restrict__ mkt, float* __restrict__ X, int* status) {
  extern __shared__ float lds[];
  float* qn = lds;                                                           // [Q][D]
  int64_t* qid = reinterpret_cast<int64_t*>(lds + FrontLds(Q, D, 0).qid);    // [Q]
  const int tid = threadIdx.x, g = tid >> 4, l = tid & 15;
  const int64_t b = blockIdx.x;
  const float bias = ws_b[0];
  // the query: 16 lanes per row
  for (int i = g; i < Q; i += 16) {
    const int64_t id = q_ids[b * Q + i];
    const bool ok = id >= 0 && id < V;
    if (!ok && l == 0) atomicOr(status, CAPAMD_STATUS_QUERY_ID_RANGE);
    const float* e = emb + (ok ? id : 0) * (int64_t)D;
    float ss = 0.f, xs = 0.f;
    for (int k = l; k < D; k += 16) {
      const float v = ok ? e[k] : 0.f;
      ss = fmaf(v, v, ss);
      xs = fmaf(v, ws_w[k], xs);
    }
    ss = group16_sum(ss);
    xs = group16_sum(xs);
    const float den = sqrtf(ss) + 1e-7f;
    for (int k = l; k < D; k += 16) qn[i * D + k] = (ok ? e[k] : 0.f) / den;
    if (l == 0) {
      X[b * Q + i] = xs + bias;
      qid[i] = id;
    }
  }
  __syncthreads();
  // the document: 16 lanes per term, the row read once per group of four query terms
  const int T = P * kWin;
  for (int t = g; t < T; t += 16) {
    const int64_t id = d_ids[b * L + t];
    const bool ok = id >= 0 && id < V;
    if (!ok && l == 0) atomicOr(status, CAPAMD_STATUS_DOC_ID_RANGE);
    const float* e = emb + (ok ? id : 0) * (int64_t)D;
    const int p = t / kWin, j = t - p * kWin;
    const int64_t w = b * P + p, at = (int64_t)j * NW + w;
    // the first pass over the row also forms its norm and Ws product; queries of more than four terms take further passes
    const float den = term_pass<true>(e, ok, qn, 0, Q, D, l, ws_w, bias, Yt + at, cost + ((int64_t)j * Q) * NW + w, NW, 0.f);
    for (int i0 = 4; i0 < Q; i0 += 4) term_pass<false>(e, ok, qn, i0, Q, D, l, ws_w, bias, Yt + at, cost + ((int64_t)j * Q + i0) * NW + w, NW, den);
    if (l == 0) {
      uint32_t eq = 0;
      for (int i = 0; i < Q; ++i) eq |= (uint32_t)(qid[i] == id) << i;
      eqt[at] = eq;
      mkt[at] = id == 0 ? eq : 0u;
    }
  }
}

// ---- stage 2 ---------------------------------------------------------------------------------------------------------------------------
struct GruPtrs {
  const float *wrz_w, *wrz_b, *w_w, *w_b, *u_w, *u_b;
};

// softmax over the four gates of one hidden unit, as F.softmax does (max subtracted)
__device__ __forceinline__ void softmax4(float& a, float& b, float& c, float& d) {
  const float m = fmaxf(fmaxf(a, b), fmaxf(c, d));
  a = expf(a - m);
  b = expf(b - m);
  c = expf(c - m);
  d = expf(d - m);
  const float r = 1.f / ((a + b) + (c + d));
  a *= r;
  b *= r;
  c *= r;
  d *= r;
}

__global__ __launch_bounds__(64) void gru_kernel(GruPtrs g1, GruPtrs g3, const float* __restrict__ Yt, const float* __restrict__ cost,
                                                 const uint32_t* __restrict__ eqt, const uint32_t* __restrict__ mkt, const float* __restrict__ X,
                                                 int Q, int P, int64_t NW, float* __restrict__ ev) {
  extern __shared__ float lds[];
  float2* hcol = reinterpret_cast<float2*>(lds);        // [Q][64]: h[i][j - 1] of this lane's chain
  float* xs = lds + 128 * Q;                             // [Q][64]: X_i in walking order
  const int lane = threadIdx.x, dir = blockIdx.y;
  const int64_t c0 = (int64_t)blockIdx.x * 64 + lane;
  const bool live = c0 < 2 * NW;
  const int64_t c = live ? c0 : 2 * NW - 1;
  const int mat = c >= NW;                                // 0: the exact-match matrix, 1: the cosine matrix
  const int64_t w = c - (int64_t)mat * NW;
  const int64_t b = w / P;
  const GruPtrs g = dir ? g3 : g1;
  // Wrz and its bias (140 floats) go through LDS into vector registers: as wave-uniform loads they would not all fit the scalar
  // registers, and what does not fit is read back lane by lane in every cell; the 22 floats of W and U stay scalar
  float wrz[14][9], brz[14], ww[2][3], bw[2], wu[2][6], bu[2];
  float* wl = xs + 64 * Q;                               // [140]
  for (int k = lane; k < 126; k += 64) wl[k] = g.wrz_w[k];
  if (lane < 14) wl[126 + lane] = g.wrz_b[lane];
  __syncthreads();
#pragma unroll
  for (int o = 0; o < 14; ++o) {
#pragma unroll
    for (int k = 0; k < 9; ++k) wrz[o][k] = wl[o * 9 + k];
    brz[o] = wl[126 + o];
  }
#pragma unroll
  for (int o = 0; o < 2; ++o) {
#pragma unroll
    for (int k = 0; k < 3; ++k) ww[o][k] = g.w_w[o * 3 + k];
#pragma unroll
    for (int k = 0; k < 6; ++k) wu[o][k] = g.u_w[o * 6 + k];
    bw[o] = g.w_b[o];
    bu[o] = g.u_b[o];
  }
  for (int ii = 0; ii < Q; ++ii) {
    hcol[ii * 64 + lane] = make_float2(0.f, 0.f);
    xs[ii * 64 + lane] = X[b * Q + (dir ? Q - 1 - ii : ii)];
  }
  float2 h = make_float2(0.f, 0.f);
  const int i_first = dir ? Q - 1 : 0;
  float cos_next = cost[((int64_t)(dir ? kWin - 1 : 0) * Q + i_first) * NW + w];
  for (int jj = 0; jj < kWin; ++jj) {
    const int j = dir ? kWin - 1 - jj : jj;
    const int jn = jj + 1 < kWin ? (dir ? j - 1 : j + 1) : j;
    const float Y = Yt[(int64_t)j * NW + w];
    const uint32_t eq = eqt[(int64_t)j * NW + w], mk = mkt[(int64_t)j * NW + w];
    float2 top = make_float2(0.f, 0.f), diag = make_float2(0.f, 0.f);
    for (int ii = 0; ii < Q; ++ii) {
      const int i = dir ? Q - 1 - ii : ii;
      const float cosv = cos_next;
      // the next cell's cosine is asked for before this cell's arithmetic
      cos_next = ii + 1 < Q ? cost[((int64_t)j * Q + (dir ? i - 1 : i + 1)) * NW + w] : cost[((int64_t)jn * Q + i_first) * NW + w];
      const float keep = ((mk >> i) & 1u) ? 0.f : 1.f;
      const float m = mat ? cosv : (float)((eq >> i) & 1u);
      const float2 left = hcol[ii * 64 + lane];
      const float q[9] = {top.x, top.y, left.x, left.y, diag.x, diag.y, xs[ii * 64 + lane] * keep, Y * keep, m * keep};
      float rz[14];
#pragma unroll
      for (int o = 0; o < 14; ++o) {
        float a = brz[o];
#pragma unroll
        for (int k = 0; k < 9; ++k) a = fmaf(wrz[o][k], q[k], a);
        rz[o] = a;
      }
      float rt[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) rt[k] = sigmoidf_(rz[k]) * q[k];        // [rl top, rt left, rd diag]
      softmax4(rz[6], rz[8], rz[10], rz[12]);                             // zi, zl, zt, zd of unit 0
      softmax4(rz[7], rz[9], rz[11], rz[13]);                             // ... of unit 1
      float h1[2];
#pragma unroll
      for (int o = 0; o < 2; ++o) {
        float a = bw[o], u = bu[o];
#pragma unroll
        for (int k = 0; k < 3; ++k) a = fmaf(ww[o][k], q[6 + k], a);
#pragma unroll
        for (int k = 0; k < 6; ++k) u = fmaf(wu[o][k], rt[k], u);
        h1[o] = tanhf(a + u);
      }
      h.x = rz[8] * left.x + rz[10] * top.x + rz[12] * diag.x + rz[6] * h1[0];
      h.y = rz[9] * left.y + rz[11] * top.y + rz[13] * diag.y + rz[7] * h1[1];
      hcol[ii * 64 + lane] = h;
      diag = left;
      top = h;
    }
  }
  if (live) *reinterpret_cast<float2*>(ev + w * kEv + dir * 4 + mat * 2) = h;
}

// ---- stage 3 ---------------------------------------------------------------------------------------------------------------------------
struct HeadPtrs {
  const float *w_ih[2], *w_hh[2], *b_ih[2], *b_hh[2], *wv_w, *wv_b, *fc_w, *fc_b;
};

__global__ __launch_bounds__(64) void head_kernel(HeadPtrs hp, const float* __restrict__ ev, int P, int kmax, float* __restrict__ out,
                                                  float* __restrict__ ev_out) {
  __shared__ float x[kMaxP][kEv], hs[2][kMaxP][kH], gates[2][4 * kH], hcur[2][kH], vals[kH][2 * kMaxP];
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  for (int t = lane; t < P * kEv; t += 64) {
    const float v = ev[b * P * kEv + t];
    x[t / kEv][t % kEv] = v;
    if (ev_out) ev_out[b * P * kEv + t] = v;
  }
  const int d = lane / 24, gt = lane % 24;               // lanes 0..47: gate gt (i, f, g, o blocks of 6) of direction d
  const bool gate_lane = lane < 48;
  float wih[kEv], whh[kH], bi = 0.f, bh = 0.f, cst = 0.f;
  if (gate_lane) {
#pragma unroll
    for (int k = 0; k < kEv; ++k) wih[k] = hp.w_ih[d][gt * kEv + k];
#pragma unroll
    for (int k = 0; k < kH; ++k) whh[k] = hp.w_hh[d][gt * kH + k];
    bi = hp.b_ih[d][gt];
    bh = hp.b_hh[d][gt];
  }
  if (lane < 2 * kH) (&hcur[0][0])[lane] = 0.f;
  __syncthreads();
  for (int s = 0; s < P; ++s) {
    const int t = d ? P - 1 - s : s;
    if (gate_lane) {
      float a = bi, r = bh;
#pragma unroll
      for (int k = 0; k < kEv; ++k) a = fmaf(wih[k], x[t][k], a);
#pragma unroll
      for (int k = 0; k < kH; ++k) r = fmaf(whh[k], hcur[d][k], r);
      a += r;
      gates[d][gt] = (gt >= 2 * kH && gt < 3 * kH) ? tanhf(a) : sigmoidf_(a);
    }
    __syncthreads();
    if (gate_lane && gt < kH) {
      cst = gates[d][kH + gt] * cst + gates[d][gt] * gates[d][2 * kH + gt];
      const float hv = gates[d][3 * kH + gt] * tanhf(cst);
      hcur[d][gt] = hv;
      hs[d][t][gt] = hv;
    }
    __syncthreads();
  }
  const int R = 2 * P;
  for (int idx = lane; idx < kH * R; idx += 64) {
    const int u = idx / R, r = idx - u * R;
    float v;
    if (r < P) {
      float a = hp.wv_b[u];
#pragma unroll
      for (int k = 0; k < kEv; ++k) a = fmaf(hp.wv_w[u * kEv + k], x[r][k], a);
      v = tanhf(a);
    } else {
      v = hs[0][r - P][u] + hs[1][r - P][u];
    }
    vals[u][r] = v;
  }
  __syncthreads();
  // sorted top-kmax per unit by rank counting: the value of rank r < kmax meets fc's weight u * kmax + r
  float acc = 0.f;
  for (int idx = lane; idx < kH * R; idx += 64) {
    const int u = idx / R, r = idx - u * R;
    const float v = vals[u][r];
    int rank = 0;
    for (int o = 0; o < R; ++o) {
      const float vo = vals[u][o];
      rank += (vo > v) || (vo == v && o < r);
    }
    if (rank < kmax) acc = fmaf(hp.fc_w[u * kmax + rank], v, acc);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) out[b] = acc + hp.fc_b[0];
}

bool shape_ok(const capamd_hint_model* m, int Q, int L) {
  if (!m || m->dim < 1 || m->dim > kMaxDim || m->vocab < 1) return false;
  if (Q < 1 || Q > kMaxQ || L < kWin || L / kWin > kMaxP) return false;
  const int P = L / kWin;
  return m->kmax >= 1 && m->kmax <= kMaxK && m->kmax <= 2 * P;
}

}  // namespace

extern "C" {

int64_t capamd_hint_workspace_bytes(const capamd_hint_model* m, int docs_per_microbatch, int Q, int L) {
  if (!shape_ok(m, Q, L) || docs_per_microbatch < 1) return -1;
  return (int64_t)carve(docs_per_microbatch, Q, L / kWin, nullptr).bytes;
}

int capamd_hint_forward(const int64_t* q_ids, const int64_t* d_ids, int B, int Q, int L, const capamd_hint_model* m, int docs_per_microbatch,
                        void* workspace, int64_t workspace_bytes, float* out, float* evidence_out, int* status, void* stream) {
  if (!q_ids || !d_ids || !m || !workspace || !out || !status || !shape_ok(m, Q, L) || B < 0 || docs_per_microbatch < 1) return CAPAMD_ERR_ARG;
  const float* need[25] = {m->emb,        m->ws_w,       m->ws_b,       m->gru1.wrz_w, m->gru1.wrz_b, m->gru1.w_w,   m->gru1.w_b,
                           m->gru1.u_w,   m->gru1.u_b,   m->gru3.wrz_w, m->gru3.wrz_b, m->gru3.w_w,   m->gru3.w_b,   m->gru3.u_w,
                           m->gru3.u_b,   m->lstm_w_ih,  m->lstm_w_hh,  m->lstm_b_ih,  m->lstm_b_hh,  m->lstm_w_ih_r, m->lstm_w_hh_r,
                           m->lstm_b_ih_r, m->lstm_b_hh_r, m->wv_w,     m->wv_b};
  for (const float* p : need)
    if (!p) return CAPAMD_ERR_ARG;
  if (!m->fc_w || !m->fc_b) return CAPAMD_ERR_ARG;
  if (B == 0) return CAPAMD_OK;
  const int P = L / kWin;
  const int64_t nb = docs_per_microbatch < B ? docs_per_microbatch : B;
  if (nb * P * (int64_t)kWin * Q > (int64_t)1 << 40) return CAPAMD_ERR_ARG;
  const size_t front_lds = FrontLds(Q, m->dim, 0).bytes;
  const GruPtrs g1 = {m->gru1.wrz_w, m->gru1.wrz_b, m->gru1.w_w, m->gru1.w_b, m->gru1.u_w, m->gru1.u_b};
  const GruPtrs g3 = {m->gru3.wrz_w, m->gru3.wrz_b, m->gru3.w_w, m->gru3.w_b, m->gru3.u_w, m->gru3.u_b};
  const HeadPtrs hp = {{m->lstm_w_ih, m->lstm_w_ih_r}, {m->lstm_w_hh, m->lstm_w_hh_r}, {m->lstm_b_ih, m->lstm_b_ih_r}, {m->lstm_b_hh, m->lstm_b_hh_r},
                       m->wv_w, m->wv_b, m->fc_w, m->fc_b};
  hipStream_t s = (hipStream_t)stream;
  return run_microbatches(
      B, docs_per_microbatch, workspace, workspace_bytes, [&](int64_t n, void* base) { return carve(n, Q, P, base); },
      [&](int64_t b0, int64_t n, const Ws& w) {
        // (only Q = 32 with dim = 512, the two limits together, passes the 64 KiB a kernel gets without asking: 64 KiB + 256 bytes)
        if (b0 == 0 && front_lds > 64 * 1024 &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(front_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)front_lds) != hipSuccess)
          return CAPAMD_ERR_LAUNCH;
        const int64_t NW = n * P;
        hipLaunchKernelGGL(front_kernel, dim3((unsigned)n), dim3(256), front_lds, s, q_ids + b0 * Q, d_ids + b0 * L, Q, L, P, m->emb, m->vocab, m->dim,
                           m->ws_w, m->ws_b, NW, w.Y, w.cos, w.eq, w.mk, w.X, status);
        hipLaunchKernelGGL(gru_kernel, dim3((unsigned)((2 * NW + 63) / 64), 2), dim3(64), (size_t)Q * 64 * 12 + 140 * 4, s, g1, g3, w.Y, w.cos, w.eq, w.mk,
                           w.X, Q, P, NW, w.ev);
        hipLaunchKernelGGL(head_kernel, dim3((unsigned)n), dim3(64), 0, s, hp, w.ev, P, m->kmax, out + b0,
                           evidence_out ? evidence_out + b0 * P * kEv : nullptr);
        return CAPAMD_OK;
      });
}

}  // extern "C"
