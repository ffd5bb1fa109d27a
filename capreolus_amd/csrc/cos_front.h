// Device pieces shared by the front ends that form cosines of embedding rows against a query held in LDS (hint.hip, posit.hip),
// 16 lanes per row.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// The dynamic LDS of a front_kernel, in 4-byte words: qn [Q][D] floats at 0, the query's ids [Q] int64 at qid (8-byte aligned), ncnt
// ints at cnt behind them.  The kernel carves by it and the host sizes the launch by it.
struct FrontLds {
  size_t qid, cnt, bytes;
  __host__ __device__ FrontLds(int Q, int D, int ncnt) : qid((size_t)((Q * D + 1) / 2 * 2)), cnt(qid + 2 * Q), bytes((cnt + ncnt) * 4) {}
};

}  // namespace
