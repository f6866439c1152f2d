// Document-masked causal attention for head dim 128: the DOC instantiations of flash_attn.hip's
// kernels, and the kernel that turns document ids into the bounds they read.
//
// A row of S tokens is several documents packed together; a document is a maximal run of equal
// consecutive ids. Query i attends to key j iff j <= i and both are in one run:
//   lo[b, s] = first index of s's run, hi[b, s] = one past its last   (int32 [B, S])
//   query-major kernels (forward, dQ):  lo[b, i] <= j <= i
//   key-major kernel (dK dV):           j <= i < hi[b, j]
// Both are non-decreasing along s, so the extreme of a block or a wave sits at its first or last
// row: whole tiles outside [lo, hi) are neither staged nor computed, and the element mask runs
// only on tiles that straddle a boundary (see the DOC branches in flash_attn.hip).
//
// This file compiles flash_attn.hip a second time for those instantiations alone, with scalar
// fp32 VALU only (_build.py SRC_FLAGS), and leaves the plain kernels' object as it was.
#define CML_FA_DOC_TU 1
#include "flash_attn.hip"

#include <limits.h>

namespace cml {
namespace {

constexpr int kBT = 256;   // threads = elements per chunk of the bounds kernel

// inclusive max / min scan of one value per thread, in thread order: shuffles inside a wave,
// the 4 wave totals through LDS. Returns the scanned value; tot = the workgroup's total.
template <bool MAX>
__device__ __forceinline__ int wg_scan(int v, int* part, int lane, int w, int& tot) {
  auto op = [](int x, int y) { return MAX ? max(x, y) : min(x, y); };
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(v, d, 64);
    if (lane >= d) v = op(v, u);
  }
  __syncthreads();   // the previous chunk's totals are read
  if (lane == 63) part[w] = v;
  __syncthreads();
  tot = part[0];
#pragma unroll
  for (int i = 1; i < kBT / 64; ++i) {
    if (i == w) v = op(v, tot);
    tot = op(tot, part[i]);
  }
  return v;
}

// One workgroup per batch row, chunks of 256 tokens with a carry. Forward pass: a run starts at
// s == 0 or ids[s] != ids[s - 1]; lo[s] = the last start at or before s (inclusive max-scan of
// the start indices). Backward pass, mirrored: a run ends after s == S - 1 or
// ids[s + 1] != ids[s]; hi[s] = the first end at or after s (min-scan from the right).
template <typename I>
__global__ __launch_bounds__(kBT) void doc_bounds_kernel(const I* ids, int* lo, int* hi, int S) {
  __shared__ int part[kBT / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const I* row = ids + static_cast<int64_t>(blockIdx.x) * S;
  int* lor = lo + static_cast<int64_t>(blockIdx.x) * S;
  int* hir = hi + static_cast<int64_t>(blockIdx.x) * S;
  int carry = 0, tot;
  for (int c0 = 0; c0 < S; c0 += kBT) {
    const int s = c0 + tid;
    int v = -1;
    if (s < S && (s == 0 || row[s] != row[s - 1])) v = s;
    v = max(wg_scan<true>(v, part, lane, w, tot), carry);
    if (s < S) lor[s] = v;
    carry = max(carry, tot);
  }
  carry = S;
  for (int c0 = 0; c0 < S; c0 += kBT) {
    const int s = S - 1 - (c0 + tid);
    int v = INT_MAX;
    if (s >= 0 && (s == S - 1 || row[s + 1] != row[s])) v = s + 1;
    v = min(wg_scan<false>(v, part, lane, w, tot), carry);
    if (s >= 0) hir[s] = v;
    carry = min(carry, tot);
  }
}

}  // namespace

hipError_t launch_doc_bounds(const void* ids, int id_bytes, int* lo, int* hi, int B, int S,
                             hipStream_t st) {
  if (B < 1 || S < 1 || (id_bytes != 4 && id_bytes != 8)) return hipErrorInvalidValue;
  if (id_bytes == 4)
    doc_bounds_kernel<<<B, kBT, 0, st>>>(static_cast<const int32_t*>(ids), lo, hi, S);
  else
    doc_bounds_kernel<<<B, kBT, 0, st>>>(static_cast<const int64_t*>(ids), lo, hi, S);
  return hipGetLastError();
}

}  // namespace cml
