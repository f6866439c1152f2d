// Counter-based dropout masks: the keep decision of an element is a pure function of
// (seed, offset, linear element index), so no mask tensor lives in HBM and a backward regenerates
// exactly what its forward used.
//
// Mapping. Elements are taken in groups of 8 consecutive linear indices (group g = index >> 3;
// every user's rows are multiples of 8 elements, so a 16-B bf16 chunk is one group). Group g draws
//     (w0, w1, w2, w3) = Philox4x32-10(counter = (g lo, g hi, offset lo, offset hi),
//                                      key     = (seed lo, seed hi))
// and element 8 g + 2 i + j (i = 0..3, j = 0..1) takes the 16-bit draw (w_i >> 16 j) & 0xffff.
// It is KEPT iff draw >= thr, thr = round(p * 65536) in [1, 65535]: the effective rate is
// p_eff = thr / 65536 and kept values are scaled by 1 / (1 - p_eff) = 65536 / (65536 - thr).
// Linear indices: hidden sites row * D + col; attention ((b * H + h) * S + q) * S + k.
// Philox4x32-10 is Salmon et al., "Parallel random numbers: as easy as 1, 2, 3" (SC 2011).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace cml {

struct DropArgs {
  uint32_t k0, k1, o0, o1, thr;
  float scale;
};

inline DropArgs drop_args(const DropSpec& s) {
  return {static_cast<uint32_t>(s.seed), static_cast<uint32_t>(s.seed >> 32),
          static_cast<uint32_t>(s.offset), static_cast<uint32_t>(s.offset >> 32), s.thr,
          65536.f / static_cast<float>(65536u - s.thr)};
}
inline bool drop_valid(const DropSpec& s) { return s.thr >= 1 && s.thr <= 65535; }

__device__ __forceinline__ uint4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                               uint32_t k0, uint32_t k1) {
  constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u, kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(kM0, c0), l0 = kM0 * c0;
    const uint32_t h1 = __umulhi(kM1, c2), l1 = kM1 * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += kW0;
    k1 += kW1;
  }
  return make_uint4(c0, c1, c2, c3);
}

// keep bits of the 8 elements of group g: bit e set <=> element 8 g + e is kept
__device__ __forceinline__ uint32_t drop_keep8(const DropArgs& d, uint64_t g) {
  const uint4 w = philox4x32_10(static_cast<uint32_t>(g), static_cast<uint32_t>(g >> 32), d.o0,
                                d.o1, d.k0, d.k1);
  const uint32_t w4[4] = {w.x, w.y, w.z, w.w};
  uint32_t bits = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    bits |= ((w4[i] & 0xffffu) >= d.thr ? 1u : 0u) << (2 * i);
    bits |= ((w4[i] >> 16) >= d.thr ? 1u : 0u) << (2 * i + 1);
  }
  return bits;
}

// v[e] <- keep(e) ? v[e] / (1 - p_eff) : 0 for the 8 elements of group g
__device__ __forceinline__ void drop_apply8(const DropArgs& d, uint64_t g, float (&v)[8]) {
  const uint32_t bits = drop_keep8(d, g);
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (bits >> e) & 1u ? v[e] * d.scale : 0.f;
}

}  // namespace cml
