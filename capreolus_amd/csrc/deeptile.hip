// DeepTileBar (reference capreolus/extractor/deeptileextractor.py: create_visualization_matrix -> color_grid, and
// capreolus/reranker/DeepTileBar.py: DeepTileBar_class.test_forward -> DeepTileBar_nn.forward), fp32 throughout, one kernel each:
//   color_kernel   one workgroup per document: the Q query rows (as they are, not normalised) in LDS, the P + 1 segment offsets clamped
//                  into a non-decreasing walk inside [0, L]; then 16 lanes per document token of [start[0], start[P]) read its row ONCE
//                  into registers and form, for every live query term, the squared distance from the differences, sim = exp(-d2 / 2),
//                  and whether the ids are equal.  Per (query term, segment) the max of sim and the count live in LDS: the max as an
//                  unsigned integer max over the bits of the (non-negative) floats, the count as an integer add - both independent of
//                  the order the tokens arrive in, no float atomics.  The tile [Q][P][C] is written at the end:
//                    pad query term (id 0) or empty segment: zeros;  tf = tokens of the segment whose id equals the term's;
//                    C = 3: [tf, idf if tf else 0, sim];  C = 2: [idf if tf else 0, sim];
//                    a token with a negative id (the literal "<pad>" token) contributes 0 and is never counted; a token with id 0 (every
//                    word the vocabulary does not know) is looked up like any other and contributes exp(-|emb[q]|^2 / 2).
//   model_kernel   one workgroup per document, the tile as [C][Q][P] in LDS:
//                  (1) the ten convolutions conv_w (kernel Q x w, 3 filters, no activation) as items (w, column t, filter f, channel c)
//                      spread over all threads, then summed over c with the bias: the sequences x_w [T_w = P - w + 1][3];
//                  (2) the ten LSTMs (gates i, f, g, o, both biases, zero state) side by side, one LANE per gate row of a chain, its
//                      3 + H weights in registers, two barriers per step; only the last h is kept (evidence [10][H]);
//                  (3) relu(W1 .), relu(W2 .), W3.
//                  The parameters are read from one packed buffer (capamd_deeptile_model), laid out by the caller once per parameter
//                  version: a lane picks its chain's weights by an offset, not by one of sixty pointers.
// Each document's result is independent of the other documents of the call, bit for bit.
#include "capreolus_amd.h"
#include "cos_front.h"
#include <math.h>

namespace {

constexpr int kMaxQ = 32, kMaxP = 64, kMaxDim = 512, kMinP = 10;
constexpr int kW = 10, kF = 3;                      // the reference's ten kernel widths; nn.LSTM(input_size=3) fixes the filters
constexpr int kMaxH = 16, kMaxLin = 128;

// ---- colouring -------------------------------------------------------------------------------------------------------------------------
// dynamic LDS in 4-byte words: qrow [Q][D] | qid [Q] int64 (8-byte aligned) | seg [P + 1] | raw [P + 1] | simbits [Q][P] | tf [Q][P]
struct ColorLds {
  size_t qid, seg, raw, sim, tf, bytes;
  __host__ __device__ ColorLds(int Q, int D, int P)
      : qid((size_t)((Q * D + 1) / 2 * 2)), seg(qid + 2 * Q), raw(seg + P + 1), sim(raw + P + 1), tf(sim + (size_t)Q * P), bytes((tf + (size_t)Q * P) * 4) {}
};

// NJ: the row's floats per lane (dim <= 16 NJ), held in registers
template <int NJ>
__global__ __launch_bounds__(256) void color_kernel(const int64_t* __restrict__ q_ids, const int64_t* __restrict__ d_ids,
                                                    const int* __restrict__ seg_start, const float* __restrict__ idf, int Q, int L, int P,
                                                    const float* __restrict__ emb, int64_t V, int D, int C, float* __restrict__ tiles, int* status) {
  extern __shared__ float lds[];
  const ColorLds at(Q, D, P);
  float* qrow = lds;
  int64_t* qid = reinterpret_cast<int64_t*>(lds + at.qid);
  int* seg = reinterpret_cast<int*>(lds + at.seg);
  int* raw = reinterpret_cast<int*>(lds + at.raw);
  unsigned* simbits = reinterpret_cast<unsigned*>(lds + at.sim);
  int* tf = reinterpret_cast<int*>(lds + at.tf);
  const int tid = threadIdx.x, g = tid >> 4, l = tid & 15;
  const int64_t b = blockIdx.x;
  for (int i = g; i < Q; i += 16) {
    const int64_t id = q_ids[b * Q + i];
    const bool ok = id >= 0 && id < V;
    if (!ok && l == 0) atomicOr(status, CAPAMD_STATUS_QUERY_ID_RANGE);
    const float* e = emb + (ok ? id : 0) * (int64_t)D;
    for (int k = l; k < D; k += 16) qrow[i * D + k] = ok ? e[k] : 0.f;
    if (l == 0) qid[i] = id;
  }
  for (int p = tid; p <= P; p += 256) raw[p] = seg_start[b * (P + 1) + p];
  for (int k = tid; k < Q * P; k += 256) {
    simbits[k] = 0u;
    tf[k] = 0;
  }
  __syncthreads();
  // offsets that decrease or leave [0, L] are clamped: seg[p] = min(L, max(0, raw[0], ..., raw[p])), so nothing is read outside the row
  for (int p = tid; p <= P; p += 256) {
    int m = 0;
    for (int k = 0; k <= p; ++k) m = raw[k] > m ? raw[k] : m;
    m = m < L ? m : L;
    if (m != raw[p]) atomicOr(status, CAPAMD_STATUS_SEGMENT_RANGE);
    seg[p] = m;
  }
  __syncthreads();
  const int t0 = seg[0], t1 = seg[P];
  for (int t = t0 + g; t < t1; t += 16) {
    const int64_t id = d_ids[b * L + t];
    if (id < 0) continue;                                  // the literal pad token: contributes 0, never counted
    const bool ok = id < V;
    if (!ok && l == 0) atomicOr(status, CAPAMD_STATUS_DOC_ID_RANGE);
    const float* e = emb + (ok ? id : 0) * (int64_t)D;
    float v[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int k = l + 16 * j;
      v[j] = (ok && k < D) ? e[k] : 0.f;
    }
    // the segment of t: the last p with seg[p] <= t (empty segments before it are stepped over)
    int lo = 0, hi = P;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (seg[mid] <= t) lo = mid; else hi = mid;
    }
    for (int i = 0; i < Q; ++i) {
      const int64_t qi = qid[i];
      if (qi == 0) continue;                               // a pad query term: its tiles stay zero
      const float* q = qrow + i * D;
      float ss = 0.f;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int k = l + 16 * j;
        const float df = k < D ? v[j] - q[k] : 0.f;
        ss = fmaf(df, df, ss);
      }
      ss = group16_sum(ss);
      if (l == 0) {
        atomicMax(&simbits[i * P + lo], __float_as_uint(expf(-0.5f * ss)));
        if (qi == id) atomicAdd(&tf[i * P + lo], 1);
      }
    }
  }
  __syncthreads();
  float* out = tiles + b * (int64_t)Q * P * C;
  for (int k = tid; k < Q * P; k += 256) {
    const int n = tf[k];
    const float w = n ? idf[b * Q + k / P] : 0.f, s = __uint_as_float(simbits[k]);
    float* o = out + (int64_t)k * C;
    if (C == 3) {
      o[0] = (float)n;
      o[1] = w;
      o[2] = s;
    } else {
      o[0] = w;
      o[1] = s;
    }
  }
}

// ---- the model -------------------------------------------------------------------------------------------------------------------------
// The packed parameters, in floats: per width w = 1 .. 10 a chunk [conv weight [3][C][Q][w] | conv bias [3] | w_ih [4H][3] | w_hh [4H][H] |
// b_ih [4H] | b_hh [4H]], then W1 [N1][10 H] | b1 [N1] | W2 [N2][N1] | b2 [N2] | W3 [N2] | b3 [1].
struct Layout {
  int Q, C, H, N1, N2;
  __host__ __device__ int64_t lstm_floats() const { return 12 * H + 4 * H * H + 8 * H; }
  __host__ __device__ int64_t chunk(int w) const { return (int64_t)kF * C * Q * (w - 1) * w / 2 + (int64_t)(w - 1) * (kF + lstm_floats()); }
  __host__ __device__ int64_t conv_b(int w) const { return chunk(w) + (int64_t)kF * C * Q * w; }
  __host__ __device__ int64_t w_ih(int w) const { return conv_b(w) + kF; }
  __host__ __device__ int64_t w_hh(int w) const { return w_ih(w) + 12 * H; }
  __host__ __device__ int64_t b_ih(int w) const { return w_hh(w) + 4 * H * H; }
  __host__ __device__ int64_t b_hh(int w) const { return b_ih(w) + 4 * H; }
  __host__ __device__ int64_t w1() const { return chunk(kW + 1); }
  __host__ __device__ int64_t b1() const { return w1() + (int64_t)N1 * kW * H; }
  __host__ __device__ int64_t w2() const { return b1() + N1; }
  __host__ __device__ int64_t b2() const { return w2() + (int64_t)N2 * N1; }
  __host__ __device__ int64_t w3() const { return b2() + N2; }
  __host__ __device__ int64_t b3() const { return w3() + N2; }
  __host__ __device__ int64_t total() const { return b3() + 1; }
};

// columns of all ten sequences: sum over w of T_w = P - w + 1
__host__ __device__ inline int seq_columns(int P) { return kW * P - kW * (kW - 1) / 2; }
// the first column of width w's sequence among them
__device__ __forceinline__ int seq_first(int P, int w) { return (w - 1) * P - (w - 1) * (w - 2) / 2; }

// dynamic LDS in floats: tile [C][Q][P] | part [columns][3][C] (x_w[t][f] ends up in its c = 0 slot) | gates [10][4H] | h [10][H] | x1 [N1] | x2 [N2]
struct ModelLds {
  size_t part, gates, h, x1, x2, bytes;
  __host__ __device__ ModelLds(const Layout& y, int P)
      : part((size_t)y.C * y.Q * P), gates(part + (size_t)seq_columns(P) * kF * y.C), h(gates + kW * 4 * y.H), x1(h + kW * y.H), x2(x1 + y.N1),
        bytes((x2 + y.N2) * 4) {}
};

__global__ __launch_bounds__(640) void model_kernel(const float* __restrict__ tiles, int P, Layout y, const float* __restrict__ w, float* __restrict__ out,
                                                    float* __restrict__ ev_out) {
  extern __shared__ float lds[];
  const ModelLds at(y, P);
  const int Q = y.Q, C = y.C, H = y.H, N1 = y.N1, N2 = y.N2;
  float* tile = lds;
  float* part = lds + at.part;
  float* gates = lds + at.gates;
  float* hcur = lds + at.h;
  float* x1 = lds + at.x1;
  float* x2 = lds + at.x2;
  const int tid = threadIdx.x, NT = blockDim.x;
  const int64_t b = blockIdx.x;
  const int QP = Q * P;
  for (int k = tid; k < QP * C; k += NT) {                 // [q][p][c] -> [c][q][p]
    const int c = k % C, qp = k / C;
    tile[c * QP + qp] = tiles[b * QP * C + k];
  }
  for (int k = tid; k < kW * H; k += NT) hcur[k] = 0.f;
  __syncthreads();
  // (1) the convolutions: item n = ((column, f), c) with the columns of width 1 first
  const int items = seq_columns(P) * kF * C;
  for (int n = tid; n < items; n += NT) {
    const int c = n % C, cf = n / C, f = cf % kF, col = cf / kF;
    int wd = 1;
    while (wd < kW && col >= seq_first(P, wd + 1)) ++wd;
    const int t = col - seq_first(P, wd);
    const float* k = w + y.chunk(wd) + (int64_t)(f * C + c) * Q * wd;
    const float* x = tile + c * QP + t;
    float a = 0.f;
    for (int q = 0; q < Q; ++q)
      for (int dw = 0; dw < wd; ++dw) a = fmaf(k[q * wd + dw], x[q * P + dw], a);
    part[n] = a;
  }
  __syncthreads();
  for (int cf = tid; cf < items / C; cf += NT) {
    int wd = 1;
    const int col = cf / kF;
    while (wd < kW && col >= seq_first(P, wd + 1)) ++wd;
    float a = w[y.conv_b(wd) + cf % kF];
    for (int c = 0; c < C; ++c) a += part[cf * C + c];
    part[cf * C] = a;
  }
  // (2) the LSTMs: lane = (chain wd, gate row r)
  const int G = 4 * H;
  const bool gate_lane = tid < kW * G;
  const int wd = gate_lane ? tid / G + 1 : 1, r = gate_lane ? tid % G : 0;
  const int T = P - wd + 1;
  float wih[kF], whh[kMaxH], bi = 0.f, bh = 0.f, cst = 0.f;
#pragma unroll
  for (int k = 0; k < kF; ++k) wih[k] = w[y.w_ih(wd) + r * kF + k];
#pragma unroll
  for (int k = 0; k < kMaxH; ++k) whh[k] = k < H ? w[y.w_hh(wd) + r * H + k] : 0.f;
  bi = w[y.b_ih(wd) + r];
  bh = w[y.b_hh(wd) + r];
  const float* xs = part + (size_t)seq_first(P, wd) * kF * C;
  float* hw = hcur + (wd - 1) * H;
  float* gw = gates + (wd - 1) * G;
  __syncthreads();
  for (int s = 0; s < P; ++s) {
    const bool on = gate_lane && s < T;
    if (on) {
      float a = bi, rr = bh;
#pragma unroll
      for (int k = 0; k < kF; ++k) a = fmaf(wih[k], xs[(s * kF + k) * C], a);
#pragma unroll
      for (int k = 0; k < kMaxH; ++k)
        if (k < H) rr = fmaf(whh[k], hw[k], rr);
      a += rr;
      gw[r] = (r >= 2 * H && r < 3 * H) ? tanhf(a) : sigmoidf_(a);
    }
    __syncthreads();
    if (on && r < H) {
      cst = gw[H + r] * cst + gw[r] * gw[2 * H + r];
      hw[r] = gw[3 * H + r] * tanhf(cst);
    }
    __syncthreads();
  }
  // (3) the head
  if (ev_out)
    for (int k = tid; k < kW * H; k += NT) ev_out[b * kW * H + k] = hcur[k];
  for (int o = tid; o < N1; o += NT) {
    float a = w[y.b1() + o];
    const float* row = w + y.w1() + (int64_t)o * kW * H;
    for (int k = 0; k < kW * H; ++k) a = fmaf(row[k], hcur[k], a);
    x1[o] = fmaxf(a, 0.f);
  }
  __syncthreads();
  for (int o = tid; o < N2; o += NT) {
    float a = w[y.b2() + o];
    const float* row = w + y.w2() + (int64_t)o * N1;
    for (int k = 0; k < N1; ++k) a = fmaf(row[k], x1[k], a);
    x2[o] = fmaxf(a, 0.f);
  }
  __syncthreads();
  if (tid < 64) {
    float a = 0.f;
    for (int o = tid; o < N2; o += 64) a = fmaf(w[y.w3() + o], x2[o], a);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if (tid == 0) out[b] = a + w[y.b3()];
  }
}

bool model_ok(const capamd_deeptile_model* m) {
  return m && m->filters == kF && m->maxqlen >= 1 && m->maxqlen <= kMaxQ && (m->channels == 2 || m->channels == 3) && m->hidden >= 1 &&
         m->hidden <= kMaxH && m->lin1 >= 1 && m->lin1 <= kMaxLin && m->lin2 >= 1 && m->lin2 <= kMaxLin;
}

Layout layout_of(const capamd_deeptile_model* m) { return {m->maxqlen, m->channels, m->hidden, m->lin1, m->lin2}; }

template <int NJ>
int launch_color(const ColorLds& at, int B, hipStream_t s, const int64_t* q_ids, const int64_t* d_ids, const int* seg_start, const float* idf, int Q, int L,
                 int P, const float* emb, int64_t V, int D, int C, float* tiles, int* status) {
  // (Q = 32 rows of dim 512 with P = 64 segments pass the 64 KiB a kernel gets without asking)
  if (at.bytes > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(color_kernel<NJ>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   (int)at.bytes) != hipSuccess)
    return CAPAMD_ERR_LAUNCH;
  hipLaunchKernelGGL(color_kernel<NJ>, dim3((unsigned)B), dim3(256), at.bytes, s, q_ids, d_ids, seg_start, idf, Q, L, P, emb, V, D, C, tiles, status);
  return hipGetLastError() == hipSuccess ? CAPAMD_OK : CAPAMD_ERR_LAUNCH;
}

}  // namespace

extern "C" {

int capamd_deeptile_color(const int64_t* q_ids, const int64_t* d_ids, const int* seg_start, const float* idf, int B, int Q, int L, int P,
                          const float* emb, int64_t V, int D, int C, float* tiles_out, int* status, void* stream) {
  if (!q_ids || !d_ids || !seg_start || !idf || !emb || !tiles_out || !status) return CAPAMD_ERR_ARG;
  if (B < 0 || Q < 1 || Q > kMaxQ || P < 1 || P > kMaxP || D < 1 || D > kMaxDim || L < 1 || V < 1 || (C != 2 && C != 3)) return CAPAMD_ERR_ARG;
  if (B == 0) return CAPAMD_OK;
  const ColorLds at(Q, D, P);
  hipStream_t s = (hipStream_t)stream;
  const int nj = (D + 15) / 16;
  if (nj <= 8) return launch_color<8>(at, B, s, q_ids, d_ids, seg_start, idf, Q, L, P, emb, V, D, C, tiles_out, status);
  if (nj <= 16) return launch_color<16>(at, B, s, q_ids, d_ids, seg_start, idf, Q, L, P, emb, V, D, C, tiles_out, status);
  if (nj <= 24) return launch_color<24>(at, B, s, q_ids, d_ids, seg_start, idf, Q, L, P, emb, V, D, C, tiles_out, status);
  return launch_color<32>(at, B, s, q_ids, d_ids, seg_start, idf, Q, L, P, emb, V, D, C, tiles_out, status);
}

int64_t capamd_deeptile_packed_floats(const capamd_deeptile_model* m) { return model_ok(m) ? layout_of(m).total() : -1; }

int capamd_deeptile_forward(const float* tiles, int B, int Q, int P, int C, const capamd_deeptile_model* m, float* out, float* evidence_out,
                            void* stream) {
  if (!tiles || !m || !out || !model_ok(m) || !m->packed || B < 0) return CAPAMD_ERR_ARG;
  if (Q != m->maxqlen || C != m->channels || P < kMinP || P > kMaxP) return CAPAMD_ERR_ARG;
  const Layout y = layout_of(m);
  if (m->packed_floats != y.total()) return CAPAMD_ERR_ARG;
  if (B == 0) return CAPAMD_OK;
  const ModelLds at(y, P);
  const int lanes = kW * 4 * y.H;
  const int nt = lanes > 256 ? (lanes + 63) / 64 * 64 : 256;
  hipLaunchKernelGGL(model_kernel, dim3((unsigned)B), dim3(nt), at.bytes, (hipStream_t)stream, tiles, P, y, m->packed, out, evidence_out);
  return hipGetLastError() == hipSuccess ? CAPAMD_OK : CAPAMD_ERR_LAUNCH;
}

}  // extern "C"
