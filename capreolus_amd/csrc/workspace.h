// Host-side pieces shared by the entries that run on a caller's workspace (tk.hip, hint.hip, posit.hip, parade.hip): the roundings, the
// carver that states a workspace's layout once - its size and its pointers come from the same sequence of take() calls -, and the
// micro-batch loop of the per-document rerankers.
#pragma once
#include "capreolus_amd.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

inline int up64(int n) { return (n + 63) / 64 * 64; }
inline size_t up256(size_t n) { return (n + 255) / 256 * 256; }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Buffers of 4-byte elements in a row, each rounded up to 256 bytes.  With a null base nothing is pointed to and only bytes() counts.
struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(void* b) : base(static_cast<char*>(b)) {}
  template <class T = float>
  T* take(size_t n) {
    static_assert(sizeof(T) == 4, "4-byte elements");
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += up256(4 * n);
    return p;
  }
  size_t bytes() const { return off; }      // (as the last initialiser of a braced list: the total of the takes before it)
};

// The tail of capamd_{tk,hint,posit}_forward behind the model's own argument checks: B documents in micro-batches of
// nb = min(docs_per_microbatch, B).  layout(nb, base) carves the model's buffers for nb documents (its result has .bytes; base may be
// null); body(b0, n, ws) launches the documents b0 .. b0 + n - 1 and returns CAPAMD_OK, or the code the call ends with.
template <class Layout, class Body>
int run_microbatches(int B, int docs_per_microbatch, void* workspace, int64_t workspace_bytes, Layout layout, Body body) {
  const int64_t nb = docs_per_microbatch < B ? docs_per_microbatch : B;
  if ((int64_t)layout(nb, nullptr).bytes > workspace_bytes) return CAPAMD_ERR_WORKSPACE;
  if ((reinterpret_cast<uintptr_t>(workspace) & 255) != 0) return CAPAMD_ERR_ALIGN;
  const auto ws = layout(nb, workspace);
  (void)hipGetLastError();
  for (int64_t b0 = 0; b0 < B; b0 += nb)
    if (const int rc = body(b0, B - b0 < nb ? B - b0 : nb, ws)) {
      (void)hipGetLastError();
      return rc;
    }
  return hipGetLastError() == hipSuccess ? CAPAMD_OK : CAPAMD_ERR_LAUNCH;
}

}  // namespace
