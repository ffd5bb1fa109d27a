// Birch (reference capreolus/reranker/birch.py:72-127) around the passage encoder of bert.hip: what comes before it (which passages are
// encoded, in which sub-batch, cut where; capamd_birch_plan) and what comes behind it (fill, top-k, combine; capamd_birch_head).
// Integers and fp32 only; no float atomics: every float sum runs in an order that is a function of the document alone.
//
// capamd_birch_plan, four launches:
//   row_kernel       one wave per passage row: the count of (seg + mask == 2) and the first position of the maximum of seg + mask
//   doc_kernel       one wave per document, lane = passage: valid flags (slot 0 forced when none is valid), ranks among the valid
//                    passages, the cut of every sub-batch of `subbatch` consecutive ranks
//   scan_kernel      one wave: the exclusive scan of the documents' valid counts, in document order -> doc_first, n_enc
//   compact_kernel   one wave per passage row: a valid row is copied to row doc_first[b] + rank, its mask cleared behind the cut
// capamd_birch_head, one launch: one wave per document, lane = passage slot.
#include "capreolus_amd.h"
#include "workspace.h"
#include <limits.h>

namespace {

constexpr int kMaxP = 64;        // a document's passages are the lanes of one wave
constexpr int kMaxHidden = 256;  // combine's hidden layer
constexpr int kWaves = 4;        // waves (rows / documents) per workgroup

bool length_ok(int S) { return (S >= 32 && S <= 256 && S % 32 == 0) || S == 384 || S == 512; }

__device__ inline int64_t shfl_xor64(int64_t v, int o) {
  const int lo = __shfl_xor((int)(v & 0xffffffffll), o, 64), hi = __shfl_xor((int)(v >> 32), o, 64);
  return ((int64_t)hi << 32) | (uint32_t)lo;
}

struct PlanWs {
  int* cnt2;    // [B P]  tokens with seg + mask == 2
  int* first;   // [B P]  first position of the maximum of seg + mask
  int* rank;    // [B P]  rank among the document's valid passages, -1: not encoded
  int* cut;     // [B P]  last position whose mask is kept
  int* nvalid;  // [B]
  size_t bytes;
};

PlanWs plan_layout(int64_t B, int64_t P, void* base) {
  Carver c(base);
  return {c.take<int>(B * P), c.take<int>(B * P), c.take<int>(B * P), c.take<int>(B * P), c.take<int>(B), c.bytes()};
}

__global__ __launch_bounds__(64 * kWaves) void row_kernel(const int64_t* __restrict__ mask, const int64_t* __restrict__ seg, int64_t rows, int S,
                                                         int* __restrict__ cnt2, int* __restrict__ first) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int64_t* m = mask + row * S;
  const int64_t* g = seg + row * S;
  int n2 = 0, pos = INT_MAX;
  int64_t best = LLONG_MIN;
  for (int j = lane; j < S; j += 64) {
    const int64_t v = g[j] + m[j];
    n2 += v == 2;
    if (pos == INT_MAX || v > best) {    // (ascending j: an equal value keeps the earlier position)
      best = v;
      pos = j;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n2 += __shfl_xor(n2, o, 64);
    const int64_t ob = shfl_xor64(best, o);
    const int op = __shfl_xor(pos, o, 64);
    if (op != INT_MAX && (pos == INT_MAX || ob > best || (ob == best && op < pos))) {
      best = ob;
      pos = op;
    }
  }
  if (lane == 0) {
    cnt2[row] = n2;
    first[row] = pos;
  }
}

__global__ __launch_bounds__(64 * kWaves) void doc_kernel(const int* __restrict__ cnt2, const int* __restrict__ first, int B, int P, int S, int subbatch,
                                                         int truncate, int* __restrict__ rank, int* __restrict__ cut, int* __restrict__ nvalid) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (b >= B) return;
  const int64_t at = (int64_t)b * P + lane;
  const bool in = lane < P;
  bool valid = in && cnt2[at] > 2;
  if (__ballot(valid) == 0ull) valid = lane == 0;            // birch.py:93-94
  const unsigned long long bal = __ballot(valid);
  const int r = __popcll(bal & ((1ull << lane) - 1ull));
  const int f = in ? first[at] : 0;
  const int grp = r / subbatch;
  int c = 0;
  for (int q = 0; q < P; ++q) {                              // the cut of a sub-batch: the largest first-maximum of its rows (:106)
    const int fq = __shfl(f, q, 64), gq = __shfl(grp, q, 64);
    if (((bal >> q) & 1ull) && gq == grp && fq > c) c = fq;
  }
  if (in) {
    rank[at] = valid ? r : -1;
    cut[at] = truncate ? c : S - 1;
  }
  if (lane == 0) nvalid[b] = __popcll(bal);
}

__global__ __launch_bounds__(64) void scan_kernel(const int* __restrict__ nvalid, int B, int* __restrict__ doc_first, int* __restrict__ n_enc) {
  const int lane = threadIdx.x;
  int carry = 0;
  for (int b0 = 0; b0 < B; b0 += 64) {
    const int v = b0 + lane < B ? nvalid[b0 + lane] : 0;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(inc, o, 64);
      if (lane >= o) inc += up;
    }
    if (b0 + lane < B) doc_first[b0 + lane] = carry + inc - v;
    carry += __shfl(inc, 63, 64);
  }
  if (lane == 0) {
    doc_first[B] = carry;
    *n_enc = carry;
  }
}

__global__ __launch_bounds__(64 * kWaves) void compact_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ mask,
                                                             const int64_t* __restrict__ seg, int64_t rows, int P, int S, const int* __restrict__ rank,
                                                             const int* __restrict__ cut, const int* __restrict__ doc_first,
                                                             int64_t* __restrict__ enc_ids, int64_t* __restrict__ enc_mask,
                                                             int64_t* __restrict__ enc_seg) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int r = rank[row];
  if (r < 0) return;
  const int64_t dst = (int64_t)doc_first[row / P] + r;       // < the document's valid count summed up: at most `rows`
  if (dst >= rows) return;
  const int c = cut[row];
  const int64_t from = row * S, to = dst * S;
  for (int j = lane; j < S; j += 64) {
    enc_ids[to + j] = ids[from + j];
    enc_seg[to + j] = seg[from + j];
    enc_mask[to + j] = j <= c ? mask[from + j] : 0;
  }
}

// An order-preserving integer image of a float (-inf < ... < -0 < +0 < ... < +inf < NaN, as torch.topk ranks them).
__device__ inline uint32_t order_key(float v) {
  if (v != v) return 0xffffffffu;
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(64 * kWaves) void head_kernel(const float* __restrict__ logits, int64_t n_logits, const int* __restrict__ doc_first, int B, int P,
                                                          int topk, int hidden, const float* __restrict__ w1, const float* __restrict__ b1,
                                                          const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ out,
                                                          float* __restrict__ topk_out, float* __restrict__ scores_out) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (b >= B) return;                                        // (whole waves leave; no workgroup barrier below)
  const int64_t f0 = doc_first[b];
  int64_t n = (int64_t)doc_first[b + 1] - f0;
  if (f0 < 0 || n < 0) n = 0;
  if (n > P) n = P;
  if (f0 + n > n_logits) n = n_logits > f0 ? n_logits - f0 : 0;
  const bool have = lane < n;
  float v = have ? logits[f0 + lane] : 0.f;
  // the fill: the minimum of the encoded logits (birch.py:124), a NaN among them as torch.min has it; the value's own bits
  uint32_t k = have ? order_key(v) : 0xffffffffu;
  uint32_t kmin = k;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) kmin = min(kmin, (uint32_t)__shfl_xor((int)kmin, o, 64));
  const unsigned long long nan_at = __ballot(have && v != v), min_at = __ballot(have && k == kmin);
  const unsigned long long src_at = nan_at ? nan_at : min_at;
  const float fill = src_at ? __shfl(v, __ffsll((long long)src_at) - 1, 64) : 0.f;
  if (!have) v = fill;
  if (scores_out && lane < P) scores_out[(int64_t)b * P + lane] = v;
  // top-k by selection: a slot's place is the number of slots that come before it (larger, or equal and earlier)
  k = lane < P ? order_key(v) : 0u;
  int place = 0;
  for (int q = 0; q < P; ++q) {
    const uint32_t kq = (uint32_t)__shfl((int)k, q, 64);
    place += kq > k || (kq == k && q < lane);
  }
  if (topk_out && lane < P && place < topk) topk_out[(int64_t)b * topk + place] = v;
  float sorted = 0.f;                                        // lane i: the i-th largest value
  for (int q = 0; q < P; ++q) {
    const int pq = __shfl(place, q, 64);
    const float vq = __shfl(v, q, 64);
    if (pq == lane) sorted = vq;
  }
  // combine (birch.py:41-47, 82) on the live parameters; every lane runs every shuffle, the sums in the order of i (and of the lanes)
  if (hidden == 0) {
    float a = 0.f;
    for (int i = 0; i < topk; ++i) a = fmaf(w1[i], __shfl(sorted, i, 64), a);
    if (lane == 0) out[b] = a;
    return;
  }
  float part = 0.f;
  for (int j0 = 0; j0 < hidden; j0 += 64) {
    const int j = j0 + lane;
    const bool on = j < hidden;
    const float* row = w1 + (int64_t)(on ? j : 0) * topk;
    float a = on ? b1[j] : 0.f;
    for (int i = 0; i < topk; ++i) a = fmaf(row[i], __shfl(sorted, i, 64), a);
    if (on) part = fmaf(w2[j], fmaxf(a, 0.f), part);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
  if (lane == 0) out[b] = part + b2[0];
}

bool plan_dims_ok(int B, int P, int S, int subbatch) {
  return B >= 0 && P >= 1 && P <= kMaxP && length_ok(S) && subbatch >= 1 && (int64_t)B * P <= INT_MAX;
}

unsigned blocks_of(int64_t n) { return (unsigned)((n + kWaves - 1) / kWaves); }

}  // namespace

extern "C" {

int64_t capamd_birch_workspace_bytes(int B, int P) {
  if (B < 0 || P < 1 || P > kMaxP || (int64_t)B * P > INT_MAX) return -1;
  return (int64_t)plan_layout(B, P, nullptr).bytes;
}

int capamd_birch_plan(const int64_t* ids, const int64_t* mask, const int64_t* seg, int B, int P, int S, int subbatch, int truncate, void* workspace,
                      int64_t workspace_bytes, int64_t* enc_ids, int64_t* enc_mask, int64_t* enc_seg, int* doc_first, int* n_enc, void* stream) {
  if (!ids || !mask || !seg || !workspace || !enc_ids || !enc_mask || !enc_seg || !doc_first || !n_enc) return CAPAMD_ERR_ARG;
  if (!plan_dims_ok(B, P, S, subbatch) || (truncate != 0 && truncate != 1)) return CAPAMD_ERR_ARG;
  if ((int64_t)plan_layout(B, P, nullptr).bytes > workspace_bytes) return CAPAMD_ERR_WORKSPACE;
  if ((reinterpret_cast<uintptr_t>(workspace) & 255) != 0) return CAPAMD_ERR_ALIGN;
  const PlanWs ws = plan_layout(B, P, workspace);
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = (int64_t)B * P;
  (void)hipGetLastError();
  if (B > 0) {
    hipLaunchKernelGGL(row_kernel, dim3(blocks_of(rows)), dim3(64 * kWaves), 0, s, mask, seg, rows, S, ws.cnt2, ws.first);
    hipLaunchKernelGGL(doc_kernel, dim3(blocks_of(B)), dim3(64 * kWaves), 0, s, ws.cnt2, ws.first, B, P, S, subbatch, truncate, ws.rank, ws.cut, ws.nvalid);
  }
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(64), 0, s, ws.nvalid, B, doc_first, n_enc);
  if (B > 0)
    hipLaunchKernelGGL(compact_kernel, dim3(blocks_of(rows)), dim3(64 * kWaves), 0, s, ids, mask, seg, rows, P, S, ws.rank, ws.cut, doc_first, enc_ids,
                       enc_mask, enc_seg);
  return hipGetLastError() == hipSuccess ? CAPAMD_OK : CAPAMD_ERR_LAUNCH;
}

int capamd_birch_head(const float* enc_logits, int64_t n_logits, const int* doc_first, int B, int P, int topk, int hidden, const float* w1,
                      const float* b1, const float* w2, const float* b2, float* out, float* topk_out, float* passage_scores_out, void* stream) {
  if (!enc_logits || !doc_first || !w1 || !out) return CAPAMD_ERR_ARG;
  if (B < 0 || n_logits < 0 || P < 1 || P > kMaxP || topk < 1 || topk > P || hidden < 0 || hidden > kMaxHidden) return CAPAMD_ERR_ARG;
  if (hidden > 0 && (!b1 || !w2 || !b2)) return CAPAMD_ERR_ARG;
  if (B == 0) return CAPAMD_OK;
  (void)hipGetLastError();
  hipLaunchKernelGGL(head_kernel, dim3(blocks_of(B)), dim3(64 * kWaves), 0, (hipStream_t)stream, enc_logits, n_logits, doc_first, B, P, topk, hidden, w1, b1,
                     w2, b2, out, topk_out, passage_scores_out);
  return hipGetLastError() == hipSuccess ? CAPAMD_OK : CAPAMD_ERR_LAUNCH;
}

}  // extern "C"
