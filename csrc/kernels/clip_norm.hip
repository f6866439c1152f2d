// Global-norm gradient clipping of the aggregate (optim.clip_norm, parallel/engine.py;
// max_grad_norm of optim/fused.py): the squared L2 norm of a set of vectors and, from it, the
// clipping coefficient as a DEVICE weight that the weighted combine of agg_update.hip reads, so
// no value of the norm ever travels to the host.
//
// sq_norm_partial  a read-only stream over up to kSqNormMaxSegs contiguous segments (blockIdx.y =
//                  segment, as agg_multi), bf16 or fp32. Per element v = float(x) * scale rounded
//                  to fp32 (what the update's fp32 multiply produces), then v * v accumulated in
//                  fp64 per thread: the square of a 24-bit significand is exact in fp64, the terms
//                  are non-negative, so the relative error of the sum is at most (terms) * 2^-53.
//                  16 B per lane on the 16-B aligned middle of a segment, kSU vectors per lane in
//                  flight (all loads of an iteration ahead of its arithmetic); the unaligned head
//                  and the tail (fewer than one vector each) are done element-wise by the first
//                  lanes of the segment's first workgroup. A fixed-order reduction (xor shuffles
//                  inside a wave, the four wave sums added in wave order by thread 0) and ONE
//                  fp64 store per workgroup, to work[segment * gridDim.x + blockIdx.x]. Every
//                  slot is written on every launch: nothing to clear, no atomics, and two runs
//                  over the same data give the same bits.
// clip_finalize    one wave: the partials summed in index order (lane l takes the contiguous
//                  chunk l, the 64 chunk sums are added in lane order), then norm, coefficient,
//                  the device weight and the statistics (kernels.h).
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace cml {
namespace {

constexpr int kSB = 256;
constexpr int kSU = 4;          // 16-B vectors in flight per lane and iteration
// Most workgroups of a launch (all segments together), 4 per CU. Measured over one fp32 / bf16 row
// of 25.6 M and 109.5 M elements: 1024 read 5-16 % faster than 2048 and 10-65 % faster than 4096 /
// 8192 (profiles/clip_norm/README.md); fewer partials also shorten clip_finalize.
constexpr int kSGrid = 1024;

struct SqSegTable {
  const void* x[kSqNormMaxSegs];
  int64_t len[kSqNormMaxSegs];
};

template <typename T>
__global__ __launch_bounds__(kSB) void sq_norm_partial(SqSegTable t, float scale,
                                                       double* __restrict__ work) {
  constexpr int VEC = 16 / sizeof(T);
  const int sg = blockIdx.y;
  const T* __restrict__ x = reinterpret_cast<const T*>(t.x[sg]);
  const int64_t L = t.len[sg];
  // elements ahead of the first 16-B boundary (x is aligned to its element size)
  const int64_t mis = static_cast<int64_t>(reinterpret_cast<uintptr_t>(x) & 15) / sizeof(T);
  const int64_t head = std::min<int64_t>(L, mis ? VEC - mis : 0);
  const int64_t nv = (L - head) / VEC;
  const T* __restrict__ xv = x + head;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kSB;
  double acc = 0.0;
  for (int64_t i0 = static_cast<int64_t>(blockIdx.x) * kSB + threadIdx.x; i0 < nv;
       i0 += kSU * stride) {
    float v[kSU][VEC];
#pragma unroll
    for (int u = 0; u < kSU; ++u) {
      const int64_t i = i0 + u * stride;
      if (i < nv) {
        load_vec<T, VEC>(xv + i * VEC, v[u]);
      } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) v[u][k] = 0.0f;
      }
    }
#pragma unroll
    for (int u = 0; u < kSU; ++u) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const double d = static_cast<double>(v[u][k] * scale);
        acc = fma(d, d, acc);
      }
    }
  }
  if (blockIdx.x == 0) {   // head [0, head) and tail [head + nv * VEC, L): < VEC elements each
    const int64_t tail0 = head + nv * VEC;
    const int64_t ntail = L - tail0;
    int64_t j = -1;
    if (threadIdx.x < head) j = threadIdx.x;
    else if (threadIdx.x - head < ntail) j = tail0 + (threadIdx.x - head);
    if (j >= 0) {
      float e[1];
      load_vec<T, 1>(x + j, e);
      const double d = static_cast<double>(e[0] * scale);
      acc = fma(d, d, acc);
    }
  }
  __shared__ double s_part[kSB / kWave];
  acc = wave_sum(acc);
  if ((threadIdx.x & (kWave - 1)) == 0) s_part[threadIdx.x / kWave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = s_part[0];
#pragma unroll
    for (int w = 1; w < kSB / kWave; ++w) s += s_part[w];
    work[static_cast<int64_t>(sg) * gridDim.x + blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(kWave) void clip_finalize(const double* __restrict__ partials,
                                                       int npart, double* norm2,
                                                       const double* reduced,
                                                       double max_norm, float base,
                                                       float* __restrict__ w_out,
                                                       double* __restrict__ stats) {
  const int lane = threadIdx.x;
  __shared__ double s_lane[kWave];
  if (npart > 0) {
    const int per = (npart + kWave - 1) / kWave;
    const int a = lane * per;
    const int b = a + per < npart ? a + per : npart;
    double s = 0.0;
    for (int i = a; i < b; ++i) s += partials[i];
    s_lane[lane] = s;
  }
  __syncthreads();
  if (lane != 0) return;
  if (npart > 0) {
    double s = 0.0;
    for (int l = 0; l < kWave; ++l) s += s_lane[l];
    norm2[0] = s;
  }
  if (w_out == nullptr) return;
  const double s = reduced ? reduced[0] : norm2[0];
  const bool ok = s == s && s >= 0.0 && s != __builtin_inf();
  const double norm = ok ? sqrt(s) : s;
  double coef = 0.0;
  if (ok) {
    coef = max_norm / (norm + 1e-6);
    coef = coef < 1.0 ? coef : 1.0;
  }
  w_out[0] = static_cast<float>(static_cast<double>(base) * coef);
  stats[0] = norm;
  stats[1] = coef;
  if (!ok) stats[2] += 1.0;
  stats[3] = s;
}

}  // namespace

int sq_norm_grid(int dtype, int64_t maxlen, int nseg, int grid_cap) {
  const int cap = grid_cap > 0 ? grid_cap : kSGrid;
  // one workgroup per kSB * kSU vectors of 16 B (it then makes one pass), at most cap over all
  // segments (then they stride), at least one (head and tail)
  const int64_t per = static_cast<int64_t>(kSB) * kSU * (dtype == DT_BF16 ? 8 : 4);
  const int64_t need = (maxlen + per - 1) / per;
  const int64_t lim = std::max(1, cap / std::max(1, nseg));
  return static_cast<int>(std::max<int64_t>(1, std::min(need, lim)));
}

hipError_t launch_sq_norm_partial(int dtype, const SqNormSeg* segs, int nseg, float scale,
                                  double* work, int grid_cap, hipStream_t st) {
  if (nseg < 1 || nseg > kSqNormMaxSegs || work == nullptr) return hipErrorInvalidValue;
  if (dtype != DT_BF16 && dtype != DT_F32) return hipErrorInvalidValue;
  const uintptr_t esz = dtype == DT_BF16 ? 2 : 4;
  SqSegTable t{};
  int64_t maxlen = 0;
  for (int i = 0; i < nseg; ++i) {
    if (segs[i].len < 0 || (segs[i].len > 0 && segs[i].x == nullptr)) return hipErrorInvalidValue;
    if (reinterpret_cast<uintptr_t>(segs[i].x) % esz) return hipErrorInvalidValue;
    t.x[i] = segs[i].x;
    t.len[i] = segs[i].len;
    maxlen = std::max(maxlen, segs[i].len);
  }
  const dim3 g(static_cast<unsigned>(sq_norm_grid(dtype, maxlen, nseg, grid_cap)),
               static_cast<unsigned>(nseg));
  if (dtype == DT_BF16) sq_norm_partial<bf16><<<g, kSB, 0, st>>>(t, scale, work);
  else sq_norm_partial<float><<<g, kSB, 0, st>>>(t, scale, work);
  return hipGetLastError();
}

hipError_t launch_clip_finalize(const double* partials, int npart, double* norm2,
                                const double* reduced, double max_norm, float base, float* w_out,
                                double* stats, hipStream_t st) {
  if (npart < 0 || (npart > 0 && (partials == nullptr || norm2 == nullptr)))
    return hipErrorInvalidValue;
  if (w_out != nullptr && (stats == nullptr || (norm2 == nullptr && reduced == nullptr)))
    return hipErrorInvalidValue;
  if (npart == 0 && w_out == nullptr) return hipSuccess;
  clip_finalize<<<1, kWave, 0, st>>>(partials, npart, norm2, reduced, max_norm, base, w_out, stats);
  return hipGetLastError();
}

}  // namespace cml
