// MFMA fragment helpers shared by the pixel-reduction kernels (wgrad1x1.hip, gram1x1.hip): operands
// staged as [pixel][channel] rows in LDS and read through ds_read_b64_tr_b16 (k = pixel).
#pragma once
#include "common.h"

namespace cml {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

__device__ __forceinline__ f32x16 mfma(bf16x8_t a, bf16x8_t b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ s16x4 ld_tr(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p));
}
__device__ __forceinline__ bf16x8_t cat(s16x4 a, s16x4 b) {
  return __builtin_bit_cast(bf16x8_t, __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7));
}
// component-wise select: a select of whole uint4 values becomes a select of their addresses and
// pushes the prefetch registers into scratch memory
__device__ __forceinline__ uint4 keep_if(bool ok, uint4 v) {
  return make_uint4(ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u);
}
// byte offset of 16-B chunk ch of row `row` in a [rows][ROWB] image; the XOR spreads the 4 rows x
// 64 B of each transposed read over all 64 banks. 256-B (and 512-B) rows: every row starts on the
// same bank, so chunk bits 0..3 are permuted by the row. 128-B rows (64 channels): row parity
// already selects the bank half, and rows 2-3 of each group of 4 take the other 64 B of it.
template <int ROWB>
__device__ __forceinline__ int img_off(int row, int ch) {
  if constexpr (ROWB == 128) return ROWB * row + 16 * (ch ^ (((row >> 1) & 1) << 2));
  return ROWB * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

}  // namespace cml
