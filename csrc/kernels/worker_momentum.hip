// Worker-side momentum (optim.worker_momentum, parallel/engine.py): every local worker keeps an
// fp32 momentum row m <- beta m + g and sends m, rounded to the comm dtype, in place of its
// gradient, so the robust rule sees rows averaged over the momentum window (Karimireddy, He,
// Jaggi 2021).
//
// One launch updates an [R, L] window in place: a column range of the flat gradient buffer (bf16
// or fp32 rows, row stride ldr >= L) and the same range of the fp32 state (row stride ldm). Per
// element: m' = fmaf(beta, m, float(g)); the state gets m', the row bf16-RNE(m') (fp32 rows: m'
// itself). Non-finite values propagate as the arithmetic dictates. Traffic with bf16 rows: 2 + 4
// read, 2 + 4 written = 12 B per element.
//
// A streaming kernel in the idiom of multi_copy.hip: a workgroup row (blockIdx.y) per window row,
// its workgroups stride over the row's 8-element vectors (one 16-B vector of bf16 against two of
// fp32) with kMU vectors per lane in flight, all loads of an iteration before its stores; the
// L mod 8 tail of each row is done element-wise by the first lanes of the row's first workgroup.
// A base pointer or row stride that is not 16-B aligned takes the same kernel at VEC = 1 (scalar
// accesses, no tail). Plain vector stores only: every element has exactly one writer.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace cml {
namespace {

constexpr int kMB = 256;
constexpr int kMU = 4;                   // vectors in flight per lane and iteration
constexpr int kMGrid = 8192;             // most workgroups of a launch (all rows together) unless
                                         // the caller sets grid_cap (tests: a few workgroups
                                         // that make several passes over a short row)

template <typename T, int VEC>
__device__ __forceinline__ void store_row(T* __restrict__ p, const float (&v)[VEC]) {
  if constexpr (sizeof(T) == 2) store_bf16<VEC>(p, v);
  else store_f32<VEC>(p, v);
}

template <typename T, int VEC>
__global__ __launch_bounds__(kMB) void worker_momentum_kernel(T* rows, int64_t ldr, float* mom,
                                                              int64_t ldm, int64_t L, float beta) {
  T* x = rows + static_cast<int64_t>(blockIdx.y) * ldr;
  float* m = mom + static_cast<int64_t>(blockIdx.y) * ldm;
  const int64_t nv = L / VEC;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kMB;
  for (int64_t i0 = static_cast<int64_t>(blockIdx.x) * kMB + threadIdx.x; i0 < nv;
       i0 += kMU * stride) {
    float g[kMU][VEC], s[kMU][VEC];
#pragma unroll
    for (int u = 0; u < kMU; ++u) {
      const int64_t i = i0 + u * stride;
      if (i < nv) {
        load_vec<T, VEC>(x + i * VEC, g[u]);
        load_vec<float, VEC>(m + i * VEC, s[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < kMU; ++u) {
      const int64_t i = i0 + u * stride;
      if (i < nv) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) s[u][k] = fmaf(beta, s[u][k], g[u][k]);
        store_f32<VEC>(m + i * VEC, s[u]);
        store_row<T, VEC>(x + i * VEC, s[u]);
      }
    }
  }
  if constexpr (VEC > 1) {   // elements [nv * VEC, L) of the row
    const int64_t j = nv * VEC + threadIdx.x;
    if (blockIdx.x == 0 && j < L) {
      float g[1], s[1];
      load_vec<T, 1>(x + j, g);
      s[0] = fmaf(beta, m[j], g[0]);
      m[j] = s[0];
      store_row<T, 1>(x + j, s);
    }
  }
}

template <typename T, int VEC>
hipError_t launch_t(void* rows, int64_t ldr, float* mom, int64_t ldm, int R, int64_t L, float beta,
                    int cap, hipStream_t st) {
  // workgroups per row: one per kMB * kMU vectors (a workgroup then makes one pass), at most
  // cap over all rows (then they stride), at least one (the tail)
  const int64_t nv = L / VEC;
  const int64_t need = (nv + kMB * kMU - 1) / (kMB * kMU);
  const int64_t gx = std::max<int64_t>(1, std::min<int64_t>(need, std::max(1, cap / R)));
  worker_momentum_kernel<T, VEC><<<dim3(static_cast<unsigned>(gx), static_cast<unsigned>(R)), kMB,
                                   0, st>>>(reinterpret_cast<T*>(rows), ldr, mom, ldm, L, beta);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_worker_momentum(int dtype, void* rows, int64_t ldr, float* mom, int64_t ldm,
                                  int R, int64_t L, float beta, int grid_cap, hipStream_t st) {
  if (R < 0 || R > 65535 || L < 0 || (R > 1 && (ldr < L || ldm < L))) return hipErrorInvalidValue;
  if (dtype != DT_BF16 && dtype != DT_F32) return hipErrorInvalidValue;
  if (R == 0 || L == 0) return hipSuccess;
  const int cap = grid_cap > 0 ? grid_cap : kMGrid;
  const int64_t esz = dtype == DT_BF16 ? 2 : 4;
  const bool vec = ((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(mom)) & 15) == 0 &&
                   (R == 1 || ((ldr * esz) % 16 == 0 && (ldm * 4) % 16 == 0));
  if (dtype == DT_BF16)
    return vec ? launch_t<bf16, 8>(rows, ldr, mom, ldm, R, L, beta, cap, st)
               : launch_t<bf16, 1>(rows, ldr, mom, ldm, R, L, beta, cap, st);
  return vec ? launch_t<float, 8>(rows, ldr, mom, ldm, R, L, beta, cap, st)
             : launch_t<float, 1>(rows, ldr, mom, ldm, R, L, beta, cap, st);
}

}  // namespace cml
