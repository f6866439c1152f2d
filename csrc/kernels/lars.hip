// LARS (optim.name=lars, parallel/engine.py; FusedLARS of optim/fused.py): layer-wise trust ratios
// on the aggregate. Three kernels over ONE state vector (the fp32 master, the momentum buffer and
// the co-indexed gradient row: the materialised fp32 aggregate, or a bf16 / fp32 gradient row
// times an fp32 scale), whose parameter tensors sit at starts that are multiples of 8 elements:
//
// seg_sq_norm_partial  one read-only pass that gives both norms of every tensor. The work is a
//                  device table of items (tensor, start, len): a tensor's range cut into chunks of
//                  at most C elements (C a multiple of 8, ops/kernels.py lars_plan), so a 2.4 M
//                  element tensor and a 64 element one cost what they hold. Workgroups of 256
//                  threads stride over the items; both rows load 16 B per lane, kLU steps of 8
//                  elements per lane in flight (all loads of an iteration ahead of its
//                  arithmetic). Per element d = p and d = float(x) * scale rounded to fp32 (what
//                  the update's multiply produces), fma(d, d, acc) in fp64 per thread: squares of
//                  24-bit significands are exact, the terms are non-negative, so the relative
//                  error of a sum is at most (terms) * 2^-53. A tensor's last item ends at its
//                  exact numel: the ragged tail (< 8 elements) is done element-wise, and the
//                  alignment padding behind it is never read into a norm. A fixed-order
//                  reduction (xor shuffles inside a wave, the four wave sums in wave order) and
//                  ONE fp64 pair per item, work[2 item] = sum p^2, work[2 item + 1] = sum g^2.
//                  Every slot is written on every launch: nothing to clear, no atomics, the same
//                  data gives the same bits. An item that does not lie inside the vector (a
//                  corrupt table) reads nothing and writes zeros.
// lars_finalize    one wave per tensor: the tensor's contiguous items' pairs summed as
//                  clip_finalize does (lane l takes the contiguous chunk l, the lane sums added
//                  in lane order) into pairs[t] = (sum p^2, sum g^2); with a q output, from that
//                  pair (or from ``reduced``, the pairs all-reduced over ranks) the trust ratio
//                  q[t] and stats[t] = (wn, gn, q, non-finite count) as kernels.h defines them.
// lars_update      the streaming SGD-momentum update with one inserted multiply, g <- q[t] g
//                  after the weight-decay term (and g <- 0, not 0 * g, where q[t] == 0). 8
//                  elements per lane and step; up to kLarsMaxSegs output segments, blockIdx.y =
//                  segment as in agg_multi. A workgroup owns a contiguous run of its segment's
//                  vectors. How a lane finds its tensor: one binary search over the ascending
//                  starts for the lane's first vector, then, per step of 256 vectors, a linear
//                  advance of at most 4 tensors and a fresh binary search beyond that (a run of
//                  tiny tensors). Starts are multiples of 8, so a vector never straddles two
//                  tensors; padding takes the preceding tensor's q. Measured: see
//                  profiles/lars/README.md (the update against the weighted n = 1 kernel of
//                  agg_update.hip on the same rows; the per-lane search was the only variant
//                  timed).
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace cml {
namespace {

constexpr int kLB = 256;
constexpr int kLU = 2;           // steps of 8 elements per lane in flight (norm pass)
constexpr int kLV = 8;           // elements per lane and step: 16 B of bf16, 2 x 16 B of fp32
constexpr int kNormGrid = 2048;  // most workgroups of the norm pass (8 per CU); they stride
constexpr int kUpdGrid = 4096;   // most workgroups of the update over all segments
constexpr int kUpdSteps = 4;     // vectors per lane a workgroup of the default launch covers

template <typename T>
__global__ __launch_bounds__(kLB) void seg_sq_norm_partial(const float* __restrict__ master,
                                                           const T* __restrict__ g, float scale,
                                                           const int64_t* __restrict__ items,
                                                           int64_t nitems, int64_t vec_len,
                                                           double* __restrict__ work) {
  __shared__ double s_part[2][kLB / kWave];
  for (int64_t it = blockIdx.x; it < nitems; it += gridDim.x) {
    const int64_t start = items[3 * it + 1];
    const int64_t len = items[3 * it + 2];
    double aw = 0.0, ag = 0.0;
    const bool inside = start >= 0 && len >= 0 && (start & (kLV - 1)) == 0 && start <= vec_len &&
                        len <= vec_len - start;
    if (inside) {
      const float* __restrict__ pm = master + start;
      const T* __restrict__ pg = g + start;
      const int64_t nv = len / kLV;
      for (int64_t i0 = threadIdx.x; i0 < nv; i0 += kLU * kLB) {
        float p[kLU][kLV], x[kLU][kLV];
#pragma unroll
        for (int u = 0; u < kLU; ++u) {
          const int64_t i = i0 + u * kLB;
          if (i < nv) {
            load_vec<float, kLV>(pm + i * kLV, p[u]);
            load_vec<T, kLV>(pg + i * kLV, x[u]);
          } else {
#pragma unroll
            for (int k = 0; k < kLV; ++k) p[u][k] = x[u][k] = 0.0f;
          }
        }
#pragma unroll
        for (int u = 0; u < kLU; ++u) {
#pragma unroll
          for (int k = 0; k < kLV; ++k) {
            const double dp = static_cast<double>(p[u][k]);
            aw = fma(dp, dp, aw);
            const double dg = static_cast<double>(x[u][k] * scale);
            ag = fma(dg, dg, ag);
          }
        }
      }
      const int64_t j = nv * kLV + threadIdx.x;   // the ragged tail: fewer than kLV elements
      if (j < len) {
        float e[1];
        const double dp = static_cast<double>(pm[j]);
        aw = fma(dp, dp, aw);
        load_vec<T, 1>(pg + j, e);
        const double dg = static_cast<double>(e[0] * scale);
        ag = fma(dg, dg, ag);
      }
    }
    aw = wave_sum(aw);
    ag = wave_sum(ag);
    if ((threadIdx.x & (kWave - 1)) == 0) {
      s_part[0][threadIdx.x / kWave] = aw;
      s_part[1][threadIdx.x / kWave] = ag;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double sw = s_part[0][0], sg = s_part[1][0];
#pragma unroll
      for (int w = 1; w < kLB / kWave; ++w) {
        sw += s_part[0][w];
        sg += s_part[1][w];
      }
      work[2 * it] = sw;
      work[2 * it + 1] = sg;
    }
    __syncthreads();   // s_part is reused by the next item
  }
}

__device__ __forceinline__ bool finite_sum(double s) {
  return s == s && s >= 0.0 && s != __builtin_inf();
}

__global__ __launch_bounds__(kWave) void lars_finalize(const double* __restrict__ work,
                                                       const int64_t* __restrict__ item_off,
                                                       int64_t nitems, double* pairs,
                                                       const double* reduced,
                                                       const uint8_t* __restrict__ adapt,
                                                       double trust, double wd, double eps,
                                                       float* __restrict__ q,
                                                       double* __restrict__ stats) {
  const int t = blockIdx.x;
  const int lane = threadIdx.x;
  __shared__ double s_lane[2][kWave];
  if (work != nullptr) {
    const int64_t a0 = std::min(std::max<int64_t>(item_off[t], 0), nitems);
    const int64_t a1 = std::min(std::max<int64_t>(item_off[t + 1], a0), nitems);
    const int64_t per = (a1 - a0 + kWave - 1) / kWave;
    const int64_t a = a0 + lane * per;
    const int64_t b = std::min(a + per, a1);
    double sw = 0.0, sg = 0.0;
    for (int64_t i = a; i < b; ++i) {
      sw += work[2 * i];
      sg += work[2 * i + 1];
    }
    s_lane[0][lane] = sw;
    s_lane[1][lane] = sg;
  }
  __syncthreads();
  if (lane != 0) return;
  if (work != nullptr) {
    double sw = 0.0, sg = 0.0;
    for (int l = 0; l < kWave; ++l) {
      sw += s_lane[0][l];
      sg += s_lane[1][l];
    }
    pairs[2 * t] = sw;
    pairs[2 * t + 1] = sg;
  }
  if (q == nullptr) return;
  const double* src = reduced != nullptr ? reduced : pairs;
  const double sw = src[2 * t], sg = src[2 * t + 1];
  const bool ok = finite_sum(sw) && finite_sum(sg);
  const double wn = finite_sum(sw) ? sqrt(sw) : sw;
  const double gn = finite_sum(sg) ? sqrt(sg) : sg;
  float qt = 0.0f;
  if (ok) {
    qt = 1.0f;
    if (adapt[t] != 0 && wn > 0.0 && gn > 0.0)
      qt = static_cast<float>(trust * wn / (gn + wd * wn + eps));
  }
  q[t] = qt;
  stats[kLarsStats * t] = wn;
  stats[kLarsStats * t + 1] = gn;
  stats[kLarsStats * t + 2] = static_cast<double>(qt);
  if (!ok) stats[kLarsStats * t + 3] += 1.0;
}

struct LarsSegTable {
  void* pout[kLarsMaxSegs];
  int64_t off[kLarsMaxSegs];
  int64_t len[kLarsMaxSegs];
};

// the last t in [0, T) with starts[t] <= e (0 where there is none)
__device__ __forceinline__ int lars_find(const int64_t* __restrict__ starts, int T, int64_t e) {
  int lo = 0, hi = T - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (starts[mid] <= e) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// The OPT_SGD sequence of agg_update.hip's update_and_store over VEC elements at state index e,
// with g <- qt g after the weight-decay term; pe = the element's index in the output segment.
template <typename T, int VEC, bool PF32>
__device__ __forceinline__ void lars_apply(const T* __restrict__ g, float scale,
                                           float* __restrict__ master, float* __restrict__ s1,
                                           const LarsUpd& u, float qt, int64_t e, void* pout,
                                           int64_t pe) {
  float x[VEC], p[VEC], b[VEC];
  load_vec<T, VEC>(g + e, x);
  load_vec<float, VEC>(master + e, p);
  const bool mom = u.momentum != 0.0f;
  if (mom && !u.first) load_vec<float, VEC>(s1 + e, b);
  float gv[VEC];
  if (qt == 0.0f) {   // a zero gradient, not 0 * g: a NaN in the row poisons no state
#pragma unroll
    for (int v = 0; v < VEC; ++v) gv[v] = 0.0f;
  } else {
#pragma unroll
    for (int v = 0; v < VEC; ++v) gv[v] = x[v] * scale;
    if (u.weight_decay != 0.0f) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) gv[v] = fmaf(u.weight_decay, p[v], gv[v]);
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) gv[v] = qt * gv[v];
  }
  if (mom) {
    if (u.first) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) b[v] = gv[v];
    } else {
#pragma unroll
      for (int v = 0; v < VEC; ++v) b[v] = fmaf(u.momentum, b[v], gv[v]);
    }
    store_f32<VEC>(s1 + e, b);
    if (u.nesterov) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) gv[v] = fmaf(u.momentum, b[v], gv[v]);
    } else {
#pragma unroll
      for (int v = 0; v < VEC; ++v) gv[v] = b[v];
    }
  }
#pragma unroll
  for (int v = 0; v < VEC; ++v) p[v] = fmaf(-u.lr, gv[v], p[v]);
  store_f32<VEC>(master + e, p);
  if (pout != nullptr) {
    if constexpr (PF32) store_f32<VEC>(reinterpret_cast<float*>(pout) + pe, p);
    else store_bf16<VEC>(reinterpret_cast<bf16*>(pout) + pe, p);
  }
}

template <typename T, bool PF32>
__global__ __launch_bounds__(kLB) void lars_update_k(const T* __restrict__ g, float scale,
                                                     float* __restrict__ master,
                                                     float* __restrict__ s1,
                                                     const float* __restrict__ q,
                                                     const int64_t* __restrict__ starts, int T_,
                                                     LarsSegTable seg, LarsUpd u, int64_t per) {
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
    int t = lars_find(starts, T_, off + i * kLV);
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
          t = lars_find(starts, T_, e);
          next = t + 1 < T_ ? starts[t + 1] : kNone;
        }
        qt = q[t];
      }
      lars_apply<T, kLV, PF32>(g, scale, master, s1, u, qt, e, pout, i * kLV);
    }
  }
  if (blockIdx.x == 0) {   // the segment's ragged tail: fewer than kLV elements
    const int64_t j = nv * kLV + threadIdx.x;
    if (j < len) {
      const int t = lars_find(starts, T_, off + j);
      lars_apply<T, 1, PF32>(g, scale, master, s1, u, q[t], off + j, pout, j);
    }
  }
}

}  // namespace

int seg_sq_norm_grid(int64_t nitems, int grid_cap) {
  const int cap = grid_cap > 0 ? grid_cap : kNormGrid;
  return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(nitems, cap)));
}

hipError_t launch_seg_sq_norm_partial(int dtype, const float* master, const void* g, float scale,
                                      const int64_t* items, int64_t nitems, int64_t vec_len,
                                      double* work, int grid_cap, hipStream_t st) {
  if (nitems < 0 || vec_len < 0) return hipErrorInvalidValue;
  if (nitems == 0) return hipSuccess;
  if (master == nullptr || g == nullptr || items == nullptr || work == nullptr)
    return hipErrorInvalidValue;
  if (dtype != DT_BF16 && dtype != DT_F32) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(master) | reinterpret_cast<uintptr_t>(g)) & 15)
    return hipErrorInvalidValue;
  const int gx = seg_sq_norm_grid(nitems, grid_cap);
  if (dtype == DT_BF16)
    seg_sq_norm_partial<bf16><<<gx, kLB, 0, st>>>(master, reinterpret_cast<const bf16*>(g), scale,
                                                  items, nitems, vec_len, work);
  else
    seg_sq_norm_partial<float><<<gx, kLB, 0, st>>>(master, reinterpret_cast<const float*>(g),
                                                   scale, items, nitems, vec_len, work);
  return hipGetLastError();
}

hipError_t launch_lars_finalize(const double* work, const int64_t* item_off, int64_t nitems, int T,
                                double* pairs, const double* reduced, const uint8_t* adapt,
                                double trust, double wd, double eps, float* q, double* stats,
                                hipStream_t st) {
  if (T < 0 || nitems < 0) return hipErrorInvalidValue;
  if (T == 0) return hipSuccess;
  if (work != nullptr && (item_off == nullptr || pairs == nullptr)) return hipErrorInvalidValue;
  if (q != nullptr && (stats == nullptr || adapt == nullptr ||
                       (pairs == nullptr && reduced == nullptr)))
    return hipErrorInvalidValue;
  if (work == nullptr && q == nullptr) return hipSuccess;
  lars_finalize<<<T, kWave, 0, st>>>(work, item_off, nitems, pairs, reduced, adapt, trust, wd, eps,
                                     q, stats);
  return hipGetLastError();
}

hipError_t launch_lars_update(int dtype, const void* g, float scale, float* master, float* s1,
                              const float* q, const int64_t* starts, int T, const LarsSeg* segs,
                              int nseg, const LarsUpd& u, int grid_cap, hipStream_t st) {
  if (nseg < 1 || nseg > kLarsMaxSegs || T < 1) return hipErrorInvalidValue;
  if (g == nullptr || master == nullptr || q == nullptr || starts == nullptr)
    return hipErrorInvalidValue;
  if (u.momentum != 0.0f && s1 == nullptr) return hipErrorInvalidValue;
  if (dtype != DT_BF16 && dtype != DT_F32) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(master) |
       reinterpret_cast<uintptr_t>(s1)) & 15)
    return hipErrorInvalidValue;
  LarsSegTable tb{};
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
  const bool pf32 = u.param_f32 != 0;
#define CML_LARS_LAUNCH(TT, PF)                                                              \
  lars_update_k<TT, PF><<<grid, kLB, 0, st>>>(reinterpret_cast<const TT*>(g), scale, master, s1, \
                                              q, starts, T, tb, u, per)
  if (dtype == DT_BF16) {
    if (pf32) CML_LARS_LAUNCH(bf16, true);
    else CML_LARS_LAUNCH(bf16, false);
  } else {
    if (pf32) CML_LARS_LAUNCH(float, true);
    else CML_LARS_LAUNCH(float, false);
  }
#undef CML_LARS_LAUNCH
  return hipGetLastError();
}

}  // namespace cml
