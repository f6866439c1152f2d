// LAMB (optim.name=lamb, parallel/engine.py; FusedLAMB of optim/fused.py; You et al. 2020): Adam's
// moments with a per-tensor trust ratio on the Adam DIRECTION u, not on the gradient. Two kernels
// over ONE state vector (the fp32 master p, the fp32 moments m and v, and the co-indexed gradient
// row: the materialised fp32 aggregate, or a bf16 / fp32 gradient row times an fp32 scale) whose
// parameter tensors sit at starts that are multiples of 8 elements; the ratios between them are
// lars_finalize of lars.hip with trust = 1, wd = 0, eps = 0 (q = wn / un, 1 or 0), unchanged.
//
// lamb_dir         THE formula, once: (x, p, m, v) -> (m', v', u) per element, every contraction
//                  written as fmaf and the compiler's own contraction off, so the u whose norm
//                  lamb_norm_partial takes and the u lamb_update applies agree bit for bit (one
//                  function, one translation unit, the same instruction sequence at VEC 8 and 1).
// lamb_norm_partial  one read-only pass over lars_plan's item table (tensor, start, len):
//                  workgroups of 256 threads stride over the items; a lane loads 8 elements of all
//                  four rows (16 B of bf16, 2 x 16 B of fp32 each; m and v are not read on the
//                  first step), kNU steps in flight, all loads of an iteration ahead of its
//                  arithmetic. kNU = 2: 64 VGPRs of loads per lane, which with the fp64
//                  accumulators and the division's temporaries stays under the 128 VGPRs that
//                  keep four workgroups on a CU (the compiler's count is in
//                  profiles/lamb/README.md). Per element fma(d, d, acc) in fp64 for d = p and
//                  d = u. The ragged tail (< 8 elements) is done element-wise and the alignment
//                  padding behind it is never read into a norm. The reduction is
//                  seg_sq_norm_partial's: xor shuffles inside a wave, the four wave sums in wave
//                  order, ONE fp64 pair per item, work[2 it] = sum p^2, work[2 it + 1] = sum u^2;
//                  every slot written on every launch, no atomics, the same data gives the same
//                  bits. An item that does not lie inside the vector reads nothing and writes
//                  zeros. It writes NO state: the moments are recomputed by the update.
// lamb_update      the streaming update: reads g, p, m, v, calls lamb_dir, p' = fmaf(-(lr q[t]),
//                  u, p), writes m', v', p' and the parameter output (bf16 / fp32). Up to
//                  kLarsMaxSegs output segments per launch, blockIdx.y = segment; a lane finds its
//                  tensor as lars_update_k does (one binary search, then a bounded linear advance,
//                  then a fresh search). q[t] == 0 (a non-finite norm) skips every store of state
//                  for that vector: p, m and v stay bit for bit, the parameter output is rewritten
//                  from the unchanged master.
//
// Traffic (derived, not measured): read-only norms followed by the full update move 44 B per
// element with an fp32 aggregate (16 B read for the norms; 16 B read and 12 B written by the
// update) plus 2 B for a bf16 parameter. Storing m', v' in the first pass would move 40 B, but it
// would make a non-finite tensor's moments unrecoverable (the ratio is known only after the pass)
// and make the first pass a writer. The 44 B form is taken for the guarantee that a NaN in the
// aggregate poisons no state. The fused AdamW kernel moves 28 - 30 B per element, so where both
// are bandwidth-bound the two LAMB stages cost about 1.5 x the AdamW n = 1 step on the same rows.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace cml {
namespace {

constexpr int kLB = 256;
constexpr int kNU = 2;          // steps of 8 elements per lane in flight (norm pass): 4 rows each
constexpr int kLV = 8;          // elements per lane and step: 16 B of bf16, 2 x 16 B of fp32
constexpr int kUpdGrid = 4096;  // most workgroups of the update over all segments
constexpr int kUpdSteps = 4;    // vectors per lane a workgroup of the default launch covers

// VEC co-indexed elements of the four rows at state index e; x is the gradient row as stored
// (before the scale). Loads only: the first step reads no moments (m = v = 0). The zeros are
// written first and the loads overwrite them: with a store in either branch the compiler joins
// the stores through a pointer and the arrays leave the registers for scratch.
template <typename T, int VEC>
__device__ __forceinline__ void lamb_load(const T* __restrict__ g, const float* __restrict__ master,
                                          const float* __restrict__ s1,
                                          const float* __restrict__ s2, bool first, int64_t e,
                                          float (&x)[VEC], float (&p)[VEC], float (&m)[VEC],
                                          float (&v)[VEC]) {
  load_vec<T, VEC>(g + e, x);
  load_vec<float, VEC>(master + e, p);
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    m[k] = 0.0f;
    v[k] = 0.0f;
  }
  if (!first) {
    load_vec<float, VEC>(s1 + e, m);
    load_vec<float, VEC>(s2 + e, v);
  }
}

// x = fp32(x * scale); m' = fma(b1, m, (1 - b1) x); v' = fma(b2, v, (1 - b2) x x) (AdamW's forms
// in agg_update.hip); denom = fma(sqrt(v'), inv_sqrt_bc2, eps); r = (m' / denom) inv_bc1;
// u = fma(wd, p, r). m and v become m' and v'.
template <int VEC>
__device__ __forceinline__ void lamb_dir(const float (&xs)[VEC], float scale,
                                         const float (&p)[VEC], float (&m)[VEC], float (&v)[VEC],
                                         const LambUpd& a, float (&u)[VEC]) {
#pragma clang fp contract(off)
  const float c1 = 1.0f - a.beta1, c2 = 1.0f - a.beta2;
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    const float x = xs[k] * scale;
    m[k] = fmaf(a.beta1, m[k], c1 * x);
    v[k] = fmaf(a.beta2, v[k], c2 * x * x);
    const float denom = fmaf(sqrtf(v[k]), a.inv_sqrt_bc2, a.eps);
    const float d = (m[k] / denom) * a.inv_bc1;
    u[k] = fmaf(a.weight_decay, p[k], d);
  }
}

template <typename T>
__global__ __launch_bounds__(kLB) void lamb_norm_partial(const float* __restrict__ master,
                                                         const T* __restrict__ g, float scale,
                                                         const float* __restrict__ s1,
                                                         const float* __restrict__ s2,
                                                         const int64_t* __restrict__ items,
                                                         int64_t nitems, int64_t vec_len, LambUpd a,
                                                         double* __restrict__ work) {
  __shared__ double s_part[2][kLB / kWave];
  const bool first = a.first != 0;
  for (int64_t it = blockIdx.x; it < nitems; it += gridDim.x) {
    const int64_t start = items[3 * it + 1];
    const int64_t len = items[3 * it + 2];
    double aw = 0.0, au = 0.0;
    const bool inside = start >= 0 && len >= 0 && (start & (kLV - 1)) == 0 && start <= vec_len &&
                        len <= vec_len - start;
    if (inside) {
      const int64_t nv = len / kLV;
      for (int64_t i0 = threadIdx.x; i0 < nv; i0 += kNU * kLB) {
        float x[kNU][kLV], p[kNU][kLV], m[kNU][kLV], v[kNU][kLV];
#pragma unroll
        for (int s = 0; s < kNU; ++s) {
          const int64_t i = i0 + s * kLB;
          if (i < nv)
            lamb_load<T, kLV>(g, master, s1, s2, first, start + i * kLV, x[s], p[s], m[s], v[s]);
        }
#pragma unroll
        for (int s = 0; s < kNU; ++s) {
          if (i0 + s * kLB < nv) {   // (an absent step is skipped, not zero-filled: eps may be 0)
            float u[kLV];
            lamb_dir<kLV>(x[s], scale, p[s], m[s], v[s], a, u);
#pragma unroll
            for (int k = 0; k < kLV; ++k) {
              const double dp = static_cast<double>(p[s][k]);
              aw = fma(dp, dp, aw);
              const double du = static_cast<double>(u[k]);
              au = fma(du, du, au);
            }
          }
        }
      }
      const int64_t j = nv * kLV + threadIdx.x;   // the ragged tail: fewer than kLV elements
      if (j < len) {
        float x[1], p[1], m[1], v[1], u[1];
        lamb_load<T, 1>(g, master, s1, s2, first, start + j, x, p, m, v);
        lamb_dir<1>(x, scale, p, m, v, a, u);
        const double dp = static_cast<double>(p[0]);
        aw = fma(dp, dp, aw);
        const double du = static_cast<double>(u[0]);
        au = fma(du, du, au);
      }
    }
    aw = wave_sum(aw);
    au = wave_sum(au);
    if ((threadIdx.x & (kWave - 1)) == 0) {
      s_part[0][threadIdx.x / kWave] = aw;
      s_part[1][threadIdx.x / kWave] = au;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double sw = s_part[0][0], su = s_part[1][0];
#pragma unroll
      for (int w = 1; w < kLB / kWave; ++w) {
        sw += s_part[0][w];
        su += s_part[1][w];
      }
      work[2 * it] = sw;
      work[2 * it + 1] = su;
    }
    __syncthreads();   // s_part is reused by the next item
  }
}

struct LambSegTable {
  void* pout[kLarsMaxSegs];
  int64_t off[kLarsMaxSegs];
  int64_t len[kLarsMaxSegs];
};

// the last t in [0, T) with starts[t] <= e (0 where there is none); lars.hip keeps its own copy
__device__ __forceinline__ int lamb_find(const int64_t* __restrict__ starts, int T, int64_t e) {
  int lo = 0, hi = T - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (starts[mid] <= e) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// VEC elements at state index e with the factor qt of their tensor; pe = the element's index in
// the output segment. qt == 0: no state is stored, the parameters are rewritten from the master.
template <typename T, int VEC, bool PF32>
__device__ __forceinline__ void lamb_apply(const T* __restrict__ g, float scale,
                                           float* __restrict__ master, float* __restrict__ s1,
                                           float* __restrict__ s2, const LambUpd& a, float qt,
                                           int64_t e, void* pout, int64_t pe) {
  float x[VEC], p[VEC], m[VEC], v[VEC];
  lamb_load<T, VEC>(g, master, s1, s2, a.first != 0, e, x, p, m, v);
  if (qt != 0.0f) {
    float u[VEC];
    lamb_dir<VEC>(x, scale, p, m, v, a, u);
    const float step = -(a.lr * qt);
#pragma unroll
    for (int k = 0; k < VEC; ++k) p[k] = fmaf(step, u[k], p[k]);
    store_f32<VEC>(s1 + e, m);
    store_f32<VEC>(s2 + e, v);
    store_f32<VEC>(master + e, p);
  }
  if (pout != nullptr) {
    if constexpr (PF32) store_f32<VEC>(reinterpret_cast<float*>(pout) + pe, p);
    else store_bf16<VEC>(reinterpret_cast<bf16*>(pout) + pe, p);
  }
}

template <typename T, bool PF32>
__global__ __launch_bounds__(kLB) void lamb_update_k(const T* __restrict__ g, float scale,
                                                     float* __restrict__ master,
                                                     float* __restrict__ s1,
                                                     float* __restrict__ s2,
                                                     const float* __restrict__ q,
                                                     const int64_t* __restrict__ starts, int T_,
                                                     LambSegTable seg, LambUpd a, int64_t per) {
  const int sg = blockIdx.y;
  const int64_t off = seg.off[sg];
  const int64_t len = seg.len[sg];
  void* pout = seg.pout[sg];
  const int64_t nv = len / kLV;
  const int64_t i1 = std::min<int64_t>((static_cast<int64_t>(blockIdx.x) + 1) * per, nv);
  int64_t i = static_cast<int64_t>(blockIdx.x) * per + threadIdx.x;
  if (i < i1) {
    // the lane's tensor, the start of the next one and its factor stay in registers: the table is
    // read again only where the lane crosses into another tensor
    constexpr int64_t kNone = INT64_MAX;
    int t = lamb_find(starts, T_, off + i * kLV);
    int64_t next = t + 1 < T_ ? starts[t + 1] : kNone;
    float qt = q[t];
    for (; i < i1; i += kLB) {
      const int64_t e = off + i * kLV;
      if (e >= next) {
        for (int k = 0; k < 4 && e >= next; ++k) {
          ++t;
          next = t + 1 < T_ ? starts[t + 1] : kNone;
        }
        if (e >= next) {
          t = lamb_find(starts, T_, e);
          next = t + 1 < T_ ? starts[t + 1] : kNone;
        }
        qt = q[t];
      }
      lamb_apply<T, kLV, PF32>(g, scale, master, s1, s2, a, qt, e, pout, i * kLV);
    }
  }
  if (blockIdx.x == 0) {   // the segment's ragged tail: fewer than kLV elements
    const int64_t j = nv * kLV + threadIdx.x;
    if (j < len) {
      const int t = lamb_find(starts, T_, off + j);
      lamb_apply<T, 1, PF32>(g, scale, master, s1, s2, a, q[t], off + j, pout, j);
    }
  }
}

bool lamb_hyper_ok(const LambUpd& a) {
  return a.beta1 >= 0.0f && a.beta1 < 1.0f && a.beta2 >= 0.0f && a.beta2 < 1.0f && a.eps >= 0.0f;
}

}  // namespace

hipError_t launch_lamb_norm_partial(int dtype, const float* master, const void* g, float scale,
                                    const float* s1, const float* s2, const int64_t* items,
                                    int64_t nitems, int64_t vec_len, const LambUpd& a, double* work,
                                    int grid_cap, hipStream_t st) {
  if (nitems < 0 || vec_len < 0) return hipErrorInvalidValue;
  if (nitems == 0) return hipSuccess;
  if (master == nullptr || g == nullptr || items == nullptr || work == nullptr)
    return hipErrorInvalidValue;
  if (!a.first && (s1 == nullptr || s2 == nullptr)) return hipErrorInvalidValue;
  if (dtype != DT_BF16 && dtype != DT_F32) return hipErrorInvalidValue;
  if (!lamb_hyper_ok(a)) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(master) | reinterpret_cast<uintptr_t>(g) |
       reinterpret_cast<uintptr_t>(s1) | reinterpret_cast<uintptr_t>(s2)) & 15)
    return hipErrorInvalidValue;
  const int gx = seg_sq_norm_grid(nitems, grid_cap);
  if (dtype == DT_BF16)
    lamb_norm_partial<bf16><<<gx, kLB, 0, st>>>(master, reinterpret_cast<const bf16*>(g), scale, s1,
                                                s2, items, nitems, vec_len, a, work);
  else
    lamb_norm_partial<float><<<gx, kLB, 0, st>>>(master, reinterpret_cast<const float*>(g), scale,
                                                 s1, s2, items, nitems, vec_len, a, work);
  return hipGetLastError();
}

hipError_t launch_lamb_update(int dtype, const void* g, float scale, float* master, float* s1,
                              float* s2, const float* q, const int64_t* starts, int T,
                              const LarsSeg* segs, int nseg, const LambUpd& a, int grid_cap,
                              hipStream_t st) {
  if (nseg < 1 || nseg > kLarsMaxSegs || T < 1) return hipErrorInvalidValue;
  if (g == nullptr || master == nullptr || s1 == nullptr || s2 == nullptr || q == nullptr ||
      starts == nullptr || segs == nullptr)
    return hipErrorInvalidValue;
  if (dtype != DT_BF16 && dtype != DT_F32) return hipErrorInvalidValue;
  if (!lamb_hyper_ok(a)) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(master) |
       reinterpret_cast<uintptr_t>(s1) | reinterpret_cast<uintptr_t>(s2)) & 15)
    return hipErrorInvalidValue;
  LambSegTable tb{};
  int64_t maxlen = 0;
  const bool has_out = segs[0].param_out != nullptr;
  for (int i = 0; i < nseg; ++i) {
    if (segs[i].off < 0 || segs[i].len < 0 || (segs[i].off & (kLV - 1))) return hipErrorInvalidValue;
    if ((segs[i].param_out != nullptr) != has_out) return hipErrorInvalidValue;
    if (reinterpret_cast<uintptr_t>(segs[i].param_out) & 15) return hipErrorInvalidValue;
    tb.pout[i] = segs[i].param_out;
    tb.off[i] = segs[i].off;
    tb.len[i] = segs[i].len;
    maxlen = std::max(maxlen, segs[i].len);
  }
  if (maxlen == 0) return hipSuccess;
  const int64_t nv = maxlen / kLV;
  const int cap = std::max(1, (grid_cap > 0 ? grid_cap : kUpdGrid) / nseg);
  const int64_t want = (nv + static_cast<int64_t>(kLB) * kUpdSteps - 1) / (kLB * kUpdSteps);
  const int64_t gx = std::max<int64_t>(1, std::min<int64_t>(want, cap));
  int64_t per = (nv + gx - 1) / gx;
  per = std::max<int64_t>(kLB, (per + kLB - 1) / kLB * kLB);   // whole steps of the workgroup
  const dim3 grid(static_cast<unsigned>(gx), static_cast<unsigned>(nseg));
  const bool pf32 = a.param_f32 != 0;
#define CML_LAMB_LAUNCH(TT, PF)                                                                  \
  lamb_update_k<TT, PF><<<grid, kLB, 0, st>>>(reinterpret_cast<const TT*>(g), scale, master, s1, \
                                              s2, q, starts, T, tb, a, per)
  if (dtype == DT_BF16) {
    if (pf32) CML_LAMB_LAUNCH(bf16, true);
    else CML_LAMB_LAUNCH(bf16, false);
  } else {
    if (pf32) CML_LAMB_LAUNCH(float, true);
    else CML_LAMB_LAUNCH(float, false);
  }
#undef CML_LAMB_LAUNCH
  return hipGetLastError();
}

}  // namespace cml
