// Fused robust aggregation + optimizer update (N04/N05/N08 of SURVEY.md §2.4).
//
// One pass over the n worker vectors of a coordinate shard: per coordinate either
//   * SORTED   : a compile-time Batcher network over NP >= n values held in VGPRs (padding rows
//                are +inf), then the mean of sorted ranks [lo, lo+cnt) -> median / trimmed mean
//                / Bulyan's coordinate phase, or
//   * WEIGHTED : sum_i w_i x_i over the non-zero weights only (Krum, Multi-Krum, Weiszfeld,
//                centered clipping, plain mean) — zero-weight rows are never read,
// and then SGD(momentum, nesterov, wd) or Adam/AdamW on the fp32 master, rewriting the bf16
// parameters in the same pass. The aggregated gradient never round-trips through HBM.
//
// The SORTED combine has a second form, NEAREST (SrcArgs::keep > 0; MeaMed / Phocas): the mean of
// the keep sorted values nearest to a centre c = mean of ranks [lo, lo+cnt). Those values are a
// contiguous rank window whose position varies per coordinate (near_combine below). bf16 rows
// take the fp32 network there, as the mixed combine does: the predicate needs floats. The other
// form, the packed u16 sort and a decode of all NP keys after it, was not built or measured; by
// instruction count it would save about a tenth of the vector ALU work at NP = 16 and a quarter
// at NP = 32.
//
// Memory-bound streaming kernel: up to 16 B per lane per worker row (Form::vec below), workgroups
// of 256 threads. A single-segment launch has no grid cap by default, one vector per thread
// (CML_AGG_GRID_CAP, grid_for below); a multi-segment launch strides at most 2048 / nseg
// workgroups over each segment. Row addresses are hoisted out of the loop; padded rows load a
// clamped (valid) row and are replaced by +inf with a select, so no per-row branch sits between
// the loads (hipcc would otherwise wait vmcnt(0) per row).
//
// Every kernel is one (Form, NP, VEC, OPT) instance of agg_kernel / agg_multi; Form is the only
// table of padded row counts and elements per lane, read by the launch ladder and by the
// run-time alignment checks alike (dispatch, at the end of the file).
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace cml {

constexpr int kBlock = 256;
constexpr int kMaxRows = 64;
constexpr int kMaxSegs = 16;   // segments of one multi-segment launch
constexpr int kMaxMixRows = 32;   // rows of the mixed sorted combine (x and y live in VGPRs)

// ----------------------------------------------------------------------------- dispatch space
// One kernel form: the row type, the sorted combine's variants (NEAR: SrcArgs::keep > 0, MIX: a
// pre-mix matrix) or the weighted combine. np(n) is the padded row count of the sorting network
// (0: no network) and vec(NP, vector) the elements per lane; both are evaluated at compile time
// by the launch ladder and at run time by the alignment checks.
template <typename T_, bool NEAR, bool MIX, bool WEIGHTED = false>
struct Form {
  using T = T_;
  static constexpr bool near = NEAR, mix = MIX, weighted = WEIGHTED;
  static constexpr bool bf = sizeof(T) == 2;

  // The mixed forms start at 4 rows (n <= 4 pads to 4, not 2) and end at kMaxMixRows.
  static constexpr int np(int n) {
    if (WEIGHTED) return 0;
    int p = MIX ? 4 : 2;
    while (p < n && p < (MIX ? kMaxMixRows : kMaxRows)) p *= 2;
    return p;
  }

  static constexpr int vec(int NP, bool vector) {
    if (!vector) return 1;   // scalar tail, or unaligned inputs
    const int full = bf ? 8 : 4;   // 16 B per lane per row
    if (WEIGHTED) return full;
    // Mixed: x and y (fp32) are live together, 2 NP VEC VGPRs: 64 at NP <= 8 (NP = 4 keeps 16-B
    // bf16 loads), 128 at NP = 16 / 32. The nearest-mixed form takes the same widths.
    if (MIX) return NP <= 4 ? full : NP <= 16 ? 4 : 2;
    // Nearest to centre: fp32 values for both row types plus the copy of the low half (1.5 NP VEC
    // live fp32). bf16 rows keep 16 B loads up to NP = 4 only: at NP = 8, 8 elements per lane take
    // 172-206 VGPRs (2 waves per SIMD) and ran 1.13-1.21x the plain median kernel, 4 elements per
    // lane 86-121 VGPRs (4-5 waves) and 0.98-1.02x. At NP = 16 / 32, 2 elements per lane ran
    // 9-12 % / 25-26 % faster than 4 (bf16 rows; fp32 rows take the same widths, not timed).
    // All in profiles/meamed/README.md.
    if (NEAR) return NP <= 4 ? full : NP <= 8 ? 4 : 2;
    // Plain: bf16 keys take half a VGPR per value, so bf16 keeps 16 B loads up to NP = 32;
    // NP = 64 drops to 2 elements per lane.
    return NP <= 32 ? full : 2;
  }

  // bf16 rows of the plain form sort packed u16 keys, two coordinates per word
  static constexpr bool packed(int VEC) { return bf && !NEAR && !MIX && !WEIGHTED && VEC >= 2; }
};

// Optimizer state of VEC coordinates, loaded BEFORE the combine so those HBM reads are in flight
// while the sort / weighted sum runs (hipcc does not hoist them above the VALU work by itself).
template <int VEC>
struct OptState {
  float p[VEC];   // fp32 master
  float a[VEC];   // momentum buffer / Adam m
  float b[VEC];   // Adam v
};

template <int VEC>
__device__ __forceinline__ void load_state(const UpdArgs& u, int opt, int64_t e, OptState<VEC>& st) {
  if (opt == OPT_NONE) return;
  load_vec<float, VEC>(u.master + e, st.p);
  if (opt == OPT_SGD) {
    if (u.momentum != 0.0f && !u.first) load_vec<float, VEC>(u.s1 + e, st.a);
  } else {
    load_vec<float, VEC>(u.s1 + e, st.a);
    load_vec<float, VEC>(u.s2 + e, st.b);
  }
}

template <int VEC>
__device__ __forceinline__ void update_and_store(const UpdArgs& u, int opt, int64_t e,
                                                 float (&g)[VEC], OptState<VEC>& st) {
  if (u.gscale != 1.0f) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) g[v] *= u.gscale;
  }
  if (u.gout) store_f32<VEC>(u.gout + e, g);
  if (opt == OPT_NONE) return;
  float (&p)[VEC] = st.p;
  if (opt == OPT_SGD) {
    if (u.weight_decay != 0.0f) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) g[v] = fmaf(u.weight_decay, p[v], g[v]);
    }
    if (u.momentum != 0.0f) {
      float (&b)[VEC] = st.a;
      if (u.first) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) b[v] = g[v];
      } else {
#pragma unroll
        for (int v = 0; v < VEC; ++v) b[v] = fmaf(u.momentum, b[v], g[v]);
      }
      store_f32<VEC>(u.s1 + e, b);
      if (u.nesterov) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) g[v] = fmaf(u.momentum, b[v], g[v]);
      } else {
#pragma unroll
        for (int v = 0; v < VEC; ++v) g[v] = b[v];
      }
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) p[v] = fmaf(-u.lr, g[v], p[v]);
  } else {  // OPT_ADAM: decoupled weight decay (AdamW), or the L2 term of Adam (adam_l2)
    float (&m)[VEC] = st.a;
    float (&s)[VEC] = st.b;
    float decay = 1.0f - u.lr * u.weight_decay;
    if (u.adam_l2) {   // wave-uniform kernel argument
      decay = 1.0f;
#pragma unroll
      for (int v = 0; v < VEC; ++v) g[v] = fmaf(u.weight_decay, p[v], g[v]);
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      m[v] = fmaf(u.beta1, m[v], (1.0f - u.beta1) * g[v]);
      s[v] = fmaf(u.beta2, s[v], (1.0f - u.beta2) * g[v] * g[v]);
      const float denom = fmaf(sqrtf(s[v]), u.inv_sqrt_bc2, u.eps);
      p[v] = fmaf(-u.step_size, m[v] / denom, p[v] * decay);
    }
    store_f32<VEC>(u.s1 + e, m);
    store_f32<VEC>(u.s2 + e, s);
  }
  store_f32<VEC>(u.master + e, p);
  if (u.param_out) {
    if (u.param_f32) store_f32<VEC>(reinterpret_cast<float*>(u.param_out) + e, p);
    else store_bf16<VEC>(reinterpret_cast<bf16*>(u.param_out) + e, p);
  }
}

// ----------------------------------------------------------------------------- nearest to centre
// a: NP sorted values per coordinate (+inf padding on top). k = keep, f = n - k (launchers ensure
// 1 <= f <= k, so f <= NP / 2). Every window [j, j+k), j <= f, holds the core ranks [f, k); of each
// pair (s_j, s_{j+k}), j < f, it holds s_{j+k} where (s_{j+k} - c) < (c - s_j) and s_j otherwise
// (the true predicates are a prefix: the left side does not decrease with j, the right side does
// not increase, in fp32 as in exact arithmetic). The pair distance k is a runtime value and the
// register array takes static indices only, so the upper partners come from a copy shifted down
// by k in log2(NP) conditional static shifts, one scalar branch per bit of k, high bit first;
// only ranks [0, NP/2) of the result are needed, so stage b moves NP/2 + b - 1 rows at most. The
// shift is in place after a copy of the low NP/2 rows: 1.5 NP VEC live values at the peak.
template <int B, int NP, int VEC>
__device__ __forceinline__ void shift_down(float (&a)[NP][VEC], int k) {
  if constexpr (B >= 1) {
    if (k & B) {   // wave-uniform
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        if (i + B < NP && i < NP / 2 + B - 1) {
#pragma unroll
          for (int v = 0; v < VEC; ++v) a[i][v] = a[i + B][v];
        }
      }
    }
    shift_down<B / 2, NP, VEC>(a, k);
  }
}

template <int NP, int VEC>
__device__ __forceinline__ void near_combine(float (&a)[NP][VEC], const SrcArgs& s, float inv,
                                             float (&g)[VEC]) {
  constexpr int H = NP / 2;
  const int k = s.keep, f = s.n - k;
  float c[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) c[v] = 0.0f;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    if (i >= s.lo && i < s.lo + s.cnt) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) c[v] += a[i][v];
    }
  }
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    c[v] *= inv;
    g[v] = 0.0f;
  }
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    if (i >= f && i < k) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) g[v] += a[i][v];
    }
  }
  float low[H][VEC];
#pragma unroll
  for (int j = 0; j < H; ++j) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) low[j][v] = a[j][v];
  }
  shift_down<H, NP, VEC>(a, k);   // a[j] = s_{j+k} for j < f
#pragma unroll
  for (int j = 0; j < H; ++j) {
    if (j < f) {
#pragma unroll
      for (int v = 0; v < VEC; ++v)
        g[v] += (a[j][v] - c[v]) < (c[v] - low[j][v]) ? a[j][v] : low[j][v];
    }
  }
  const float invk = 1.0f / static_cast<float>(k);
#pragma unroll
  for (int v = 0; v < VEC; ++v) g[v] *= invk;
}

// ----------------------------------------------------------------------------- mixed sorted combine
// A linear pre-mix of the rows ahead of the sort (nearest-neighbour mixing for the coordinate
// rules): per coordinate y_i = sum_j M_ij x_j in fp32 (an fmaf chain in j order), then the
// sanitising, network and rank window of agg_sorted_body on y. M (fp32 [n, n]) is staged once per
// workgroup into LDS, zero-padded to NP x NP, and read back as broadcasts (every lane the same
// address). x and y are both live during the mix, so VEC is chosen per NP to keep 2 NP VEC fp32
// in registers (Form::vec); the mixed values are fp32, so bf16 rows take the fp32 network.
//
// "M_ij == 0 contributes nothing even where x_j is NaN / inf": with every loaded value finite a
// zero entry adds an exact zero, so the fast path is plain (packed) FMAs. One extra FMA per loaded
// value (x * 0 accumulates to NaN iff some x is non-finite) detects the other case, and a wave
// that saw a non-finite value redoes its mix with the zero entries skipped by a select.
template <int NP, int VEC>
__device__ __forceinline__ void mix_rows(const float (&sM)[NP * NP], const float (&x)[NP][VEC],
                                         float (&y)[NP][VEC], int n) {
  // M is re-read from LDS as it is used: its NP^2 values are loop invariant, and hipcc would
  // otherwise hoist all of them into VGPRs (NP = 16: 256 registers, spilling). An offset it
  // cannot see through (always 0) keeps the broadcast reads inside the iteration.
  int z = 0;
  asm volatile("" : "+v"(z));
  float probe = 0.0f;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) probe = fmaf(x[j][v], 0.0f, probe);
  }
  if (__builtin_amdgcn_ballot_w64(probe != probe) == 0) {   // wave-uniform
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      if (i < n) {   // n is a kernel argument: a scalar branch per row
        if constexpr (VEC % 2 == 0) {
          f32x2 acc[VEC / 2];
#pragma unroll
          for (int v = 0; v < VEC / 2; ++v) acc[v] = f32x2{0.0f, 0.0f};
#pragma unroll
          for (int j = 0; j < NP; ++j) {
            const float mij = sM[z + i * NP + j];
            const f32x2 mm = {mij, mij};
#pragma unroll
            for (int v = 0; v < VEC / 2; ++v)
              acc[v] = __builtin_elementwise_fma(mm, f32x2{x[j][2 * v], x[j][2 * v + 1]}, acc[v]);
          }
#pragma unroll
          for (int v = 0; v < VEC / 2; ++v) {
            y[i][2 * v] = acc[v].x;
            y[i][2 * v + 1] = acc[v].y;
          }
        } else {
#pragma unroll
          for (int v = 0; v < VEC; ++v) y[i][v] = 0.0f;
#pragma unroll
          for (int j = 0; j < NP; ++j) {
            const float mij = sM[z + i * NP + j];
#pragma unroll
            for (int v = 0; v < VEC; ++v) y[i][v] = fmaf(mij, x[j][v], y[i][v]);
          }
        }
      } else {   // padding row: replaced by +inf in the caller
#pragma unroll
        for (int v = 0; v < VEC; ++v) y[i][v] = 0.0f;
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      if (i < n) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) y[i][v] = 0.0f;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
          const float mij = sM[z + i * NP + j];
#pragma unroll
          for (int v = 0; v < VEC; ++v)
            y[i][v] = mij != 0.0f ? fmaf(mij, x[j][v], y[i][v]) : y[i][v];
        }
      } else {
#pragma unroll
        for (int v = 0; v < VEC; ++v) y[i][v] = 0.0f;
      }
    }
  }
}

// ----------------------------------------------------------------------------- sorted combine
// fp32 rows, the bf16 scalar tail, and bf16 rows of the NEAR and MIX forms: sort fp32 values. The
// rank window [lo, lo+cnt) is wave-uniform (kernel arguments), so the per-rank test is a scalar
// branch, not a VALU select. MIX: the rows are mixed (mix_rows) between the loads and the
// sanitising pass.
//
// The row offsets, the sanitising pass and the window mean are written out here (and the first
// and the last again in the packed-key body and in near_combine's centre) rather than factored
// into __forceinline__ helpers: a helper is simplified on its own before it is inlined, and each
// of the three then moves registers or code in kernels that must not move -- the sanitising pass
// over the whole array turns its selects into branches (fp32, NP = 8, 4 per lane, SGD: 3800 ->
// 7312 bytes, 108 -> 112 VGPRs), the window mean moves 68 -> 65 VGPRs at fp32 NP = 4 and as
// near_combine's centre 152 -> 162 at NP = 32, the row offsets move code size alone
// (profiles/agg_dispatch/README.md).
template <typename T, int NP, int VEC, int OPT, bool MIX, bool NEAR>
__device__ __forceinline__ void agg_sorted_body(const SrcArgs& s, const UpdArgs& u, int64_t base,
    int64_t nvec, int blk, int nblk, const float* __restrict__ mix = nullptr) {
  __shared__ float sM[MIX ? NP * NP : 1];
  if constexpr (MIX) {
    for (int k = threadIdx.x; k < NP * NP; k += kBlock) {
      const int i = k / NP, j = k % NP;
      sM[k] = (i < s.n && j < s.n) ? mix[i * s.n + j] : 0.0f;
    }
    __syncthreads();
  }
  const T* X = reinterpret_cast<const T*>(s.X);
  int64_t roff[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int r = i < s.n ? i : s.n - 1;
    roff[i] = static_cast<int64_t>(s.rows ? s.rows[r] : r) * s.ld + base;
  }
  const float inf = __builtin_inff();
  const float inv = 1.0f / static_cast<float>(s.cnt);
  const int64_t stride = static_cast<int64_t>(nblk) * kBlock;
  for (int64_t t = static_cast<int64_t>(blk) * kBlock + threadIdx.x; t < nvec; t += stride) {
    const int64_t e = t * VEC;
    float a[NP][VEC];
    OptState<VEC> st;
    if constexpr (MIX) {
      float x[NP][VEC];
#pragma unroll
      for (int i = 0; i < NP; ++i) load_vec<T, VEC>(X + roff[i] + e, x[i]);
      load_state<VEC>(u, OPT, base + e, st);
      mix_rows<NP, VEC>(sM, x, a, s.n);
    } else {
#pragma unroll
      for (int i = 0; i < NP; ++i) load_vec<T, VEC>(X + roff[i] + e, a[i]);
      load_state<VEC>(u, OPT, base + e, st);
    }
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const bool pad = i >= s.n;
#pragma unroll
      for (int v = 0; v < VEC; ++v) a[i][v] = (pad || a[i][v] != a[i][v]) ? inf : a[i][v];
    }
    sort_columns<float, NP, VEC>(a);
    float g[VEC];
    if constexpr (NEAR) {
      near_combine<NP, VEC>(a, s, inv, g);
    } else {
#pragma unroll
      for (int v = 0; v < VEC; ++v) g[v] = 0.0f;
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        if (i >= s.lo && i < s.lo + s.cnt) {
#pragma unroll
          for (int v = 0; v < VEC; ++v) g[v] += a[i][v];
        }
      }
#pragma unroll
      for (int v = 0; v < VEC; ++v) g[v] *= inv;
    }
    update_and_store<VEC>(u, OPT, base + e, g, st);
  }
}

// bf16 rows: sort packed u16 keys (two coordinates per v_pk_min/max_u16, see bf16_key), decode
// only the cnt window ranks. VEC bf16 = VEC/2 32-bit words per row.
template <int W> struct Words;
template <> struct Words<4> {
  static __device__ __forceinline__ void load(const bf16* p, uint32_t (&w)[4]) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    w[0] = u.x; w[1] = u.y; w[2] = u.z; w[3] = u.w;
  }
};
template <> struct Words<2> {
  static __device__ __forceinline__ void load(const bf16* p, uint32_t (&w)[2]) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    w[0] = u.x; w[1] = u.y;
  }
};
template <> struct Words<1> {
  static __device__ __forceinline__ void load(const bf16* p, uint32_t (&w)[1]) {
    w[0] = *reinterpret_cast<const uint32_t*>(p);
  }
};

template <int NP, int VEC, int OPT>
__device__ __forceinline__ void agg_sorted_bf16_body(const SrcArgs& s, const UpdArgs& u, int64_t base,
    int64_t nvec, int blk, int nblk) {
  constexpr int W = VEC / 2;
  const bf16* X = reinterpret_cast<const bf16*>(s.X);
  int64_t roff[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int r = i < s.n ? i : s.n - 1;
    roff[i] = static_cast<int64_t>(s.rows ? s.rows[r] : r) * s.ld + base;
  }
  const float inv = 1.0f / static_cast<float>(s.cnt);
  const u16x2 kinf = {kKeyInf, kKeyInf};
  const int64_t stride = static_cast<int64_t>(nblk) * kBlock;
  for (int64_t t = static_cast<int64_t>(blk) * kBlock + threadIdx.x; t < nvec; t += stride) {
    const int64_t e = t * VEC;
    uint32_t raw[NP][W];
#pragma unroll
    for (int i = 0; i < NP; ++i) Words<W>::load(X + roff[i] + e, raw[i]);
    OptState<VEC> st;
    load_state<VEC>(u, OPT, base + e, st);
    u16x2 k[NP][W];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const bool pad = i >= s.n;
#pragma unroll
      for (int w = 0; w < W; ++w) k[i][w] = pad ? kinf : bf16_key(raw[i][w]);
    }
    sort_columns<u16x2, NP, W>(k);
    float g[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) g[v] = 0.0f;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      if (i >= s.lo && i < s.lo + s.cnt) {
#pragma unroll
        for (int w = 0; w < W; ++w) {
          float lo, hi;
          bf16_unkey(k[i][w], lo, hi);
          g[2 * w] += lo;
          g[2 * w + 1] += hi;
        }
      }
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) g[v] *= inv;
    update_and_store<VEC>(u, OPT, base + e, g, st);
  }
}

// ----------------------------------------------------------------------------- weighted combine
template <typename T, int VEC, int OPT>
__device__ __forceinline__ void agg_weighted_body(const SrcArgs& s, const UpdArgs& u, int64_t base,
    int64_t nvec, int blk, int nblk) {
  // Compact the non-zero weights once per workgroup (LDS, broadcast reads in the loop).
  __shared__ int64_t s_off[kMaxRows];
  __shared__ float s_w[kMaxRows];
  __shared__ int s_nz;
  if (threadIdx.x == 0) {
    int nz = 0;
    for (int i = 0; i < s.n; ++i) {
      const float wi = s.w ? s.w[i] : 1.0f;
      if (wi != 0.0f) {
        s_off[nz] = static_cast<int64_t>(s.rows ? s.rows[i] : i) * s.ld + base;
        s_w[nz] = wi;
        ++nz;
      }
    }
    s_nz = nz;
  }
  __syncthreads();
  const int nz = s_nz;
  const T* X = reinterpret_cast<const T*>(s.X);
  const int64_t stride = static_cast<int64_t>(nblk) * kBlock;
  for (int64_t t = static_cast<int64_t>(blk) * kBlock + threadIdx.x; t < nvec; t += stride) {
    const int64_t e = t * VEC;
    OptState<VEC> st;
    load_state<VEC>(u, OPT, base + e, st);
    float g[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) g[v] = 0.0f;
    int i = 0;
    for (; i + 4 <= nz; i += 4) {  // four rows in flight before the FMAs
      float x0[VEC], x1[VEC], x2[VEC], x3[VEC];
      load_vec<T, VEC>(X + s_off[i] + e, x0);
      load_vec<T, VEC>(X + s_off[i + 1] + e, x1);
      load_vec<T, VEC>(X + s_off[i + 2] + e, x2);
      load_vec<T, VEC>(X + s_off[i + 3] + e, x3);
      const float w0 = s_w[i], w1 = s_w[i + 1], w2 = s_w[i + 2], w3 = s_w[i + 3];
#pragma unroll
      for (int v = 0; v < VEC; ++v)
        g[v] = fmaf(w3, x3[v], fmaf(w2, x2[v], fmaf(w1, x1[v], fmaf(w0, x0[v], g[v]))));
    }
    for (; i < nz; ++i) {
      float x0[VEC];
      load_vec<T, VEC>(X + s_off[i] + e, x0);
      const float w0 = s_w[i];
#pragma unroll
      for (int v = 0; v < VEC; ++v) g[v] = fmaf(w0, x0[v], g[v]);
    }
    update_and_store<VEC>(u, OPT, base + e, g, st);
  }
}

// ----------------------------------------------------------------------------- kernels
// A mixed form's kernels take the matrix as one more argument after u: Mix = {MixPtr}; the other
// forms' kernels take none: Mix = {}. Both kernels pick the body of form F themselves: one more
// __forceinline__ layer between kernel and body moves code in the largest scalar-tail kernels
// (NP = 64, no optimizer: up to 252 bytes and one VGPR).
using MixPtr = const float* __restrict__;

// Single segment (one bucket / one vector): grid-stride over nvec vectors.
template <class F, int NP, int VEC, int OPT, class... Mix>
__global__ __launch_bounds__(kBlock) void agg_kernel(SrcArgs s, UpdArgs u, Mix... mix, int64_t base,
                                                     int64_t nvec) {
  using T = typename F::T;
  const int blk = blockIdx.x, nblk = gridDim.x;
  if constexpr (F::weighted) agg_weighted_body<T, VEC, OPT>(s, u, base, nvec, blk, nblk);
  else if constexpr (F::packed(VEC)) agg_sorted_bf16_body<NP, VEC, OPT>(s, u, base, nvec, blk, nblk);
  else agg_sorted_body<T, NP, VEC, OPT, F::mix, F::near>(s, u, base, nvec, blk, nblk, mix...);
}

// Several segments in ONE launch (the sharded engine's buckets: per-bucket worker matrices and
// parameter shards, one fp32 optimizer-state vector): blockIdx.y = segment. Every segment is on
// the vector path (checked by the launcher).
struct SegTable {
  const void* X[kMaxSegs];
  int64_t ld[kMaxSegs];
  int64_t nvec[kMaxSegs];
  int64_t off[kMaxSegs];     // element offset into master / s1 / s2 / gout
  void* pout[kMaxSegs];
};

// The shared rule and state bases (s, u) become those of segment sg: in the multi kernel, and on
// the host for the per-segment fallback.
__host__ __device__ __forceinline__ void seg_args(const SegTable& t, int sg, SrcArgs& s,
                                                  UpdArgs& u) {
  s.X = t.X[sg];
  s.ld = t.ld[sg];
  const int64_t o = t.off[sg];
  if (u.master) u.master += o;
  if (u.s1) u.s1 += o;
  if (u.s2) u.s2 += o;
  if (u.gout) u.gout += o;
  u.param_out = t.pout[sg];
}

template <class F, int NP, int VEC, int OPT, class... Mix>
__global__ __launch_bounds__(kBlock) void agg_multi(SrcArgs s, UpdArgs u, Mix... mix, SegTable t) {
  seg_args(t, blockIdx.y, s, u);
  using T = typename F::T;
  const int64_t nvec = t.nvec[blockIdx.y];
  const int blk = blockIdx.x, nblk = gridDim.x;
  if constexpr (F::weighted) agg_weighted_body<T, VEC, OPT>(s, u, 0, nvec, blk, nblk);
  else if constexpr (F::packed(VEC)) agg_sorted_bf16_body<NP, VEC, OPT>(s, u, 0, nvec, blk, nblk);
  else agg_sorted_body<T, NP, VEC, OPT, F::mix, F::near>(s, u, 0, nvec, blk, nblk, mix...);
}

// ----------------------------------------------------------------------------- dispatch
// Run-time values to compile-time ones: each calls fn with a std::integral_constant (with_form:
// with a Form). These are the only ladder over n and the only switch over opt in the file.
template <int V> using IC = std::integral_constant<int, V>;

template <class Fn>
static void with_np(int n, Fn&& fn) {   // the least power of two >= n; Form::np maps it further
  if (n <= 2) fn(IC<2>{});
  else if (n <= 4) fn(IC<4>{});
  else if (n <= 8) fn(IC<8>{});
  else if (n <= 16) fn(IC<16>{});
  else if (n <= 32) fn(IC<32>{});
  else fn(IC<64>{});
}

template <class Fn>
static void with_opt(int opt, Fn&& fn) {
  switch (opt) {
    case OPT_NONE: fn(IC<OPT_NONE>{}); break;
    case OPT_SGD: fn(IC<OPT_SGD>{}); break;
    default: fn(IC<OPT_ADAM>{}); break;
  }
}

template <class Fn>
static void with_form(int dtype, int combine, bool mix, bool near, Fn&& fn) {
  auto rows = [&](auto t) {
    using T = decltype(t);
    if (combine == CMB_WEIGHTED) fn(Form<T, false, false, true>{});
    else if (mix && near) fn(Form<T, true, true>{});
    else if (mix) fn(Form<T, false, true>{});
    else if (near) fn(Form<T, true, false>{});
    else fn(Form<T, false, false>{});
  };
  if (dtype == DT_BF16) rows(bf16{});
  else rows(float{});
}

// fn(IC<NP>, IC<VEC>, IC<OPT>) of form F for n rows on the vector or the scalar path.
template <class F, bool VECTOR, class Fn>
static void with_kernel(int n, int opt, Fn&& fn) {
  with_np(n, [&](auto np) {
    with_opt(opt, [&](auto o) {
      constexpr int NP = F::np(decltype(np)::value);
      fn(IC<NP>{}, IC<F::vec(NP, VECTOR)>{}, o);
    });
  });
}

// CML_AGG_GRID_CAP: the most workgroups of an update launch (default 0 = no cap: one vector per
// thread, the form that streams fastest on MI355X -- tools/diag/hbm_copy.py: a one-pass copy
// 6.0-6.6 TB/s vs 4.7-5.7 for grid-stride loops; the fused rule + SGD update 8.6-12.7 % faster
// than at the former cap of 2048 workgroups, profiles/r06_13/agg_*.jsonl).
static inline int grid_for(int64_t nvec) {
  static const int cap = [] {
    const char* e = getenv("CML_AGG_GRID_CAP");
    return e ? atoi(e) : 0;
  }();
  int64_t b = (nvec + kBlock - 1) / kBlock;
  if (cap > 0 && b > cap) b = cap;
  if (b > (1LL << 30)) b = 1LL << 30;
  if (b < 1) b = 1;
  return static_cast<int>(b);
}

// D elements from element base on; VECTOR: D is a multiple of F::vec and all pointers aligned.
template <class F, bool VECTOR>
static void launch(int opt, const SrcArgs& s, const UpdArgs& u, const float* mix, int64_t base,
                   int64_t D, hipStream_t st) {
  with_kernel<F, VECTOR>(s.n, opt, [&](auto np, auto vec, auto o) {
    constexpr int NP = decltype(np)::value, VEC = decltype(vec)::value, OPT = decltype(o)::value;
    const int64_t nvec = D / VEC;
    const int g = grid_for(nvec);
    if constexpr (F::mix) agg_kernel<F, NP, VEC, OPT, MixPtr><<<g, kBlock, 0, st>>>(s, u, mix, base, nvec);
    else agg_kernel<F, NP, VEC, OPT><<<g, kBlock, 0, st>>>(s, u, base, nvec);
  });
}

static inline bool aligned(const void* p, int bytes) {
  return p == nullptr || (reinterpret_cast<uintptr_t>(p) % bytes) == 0;
}

// The vector path needs every state pointer aligned to vec elements (and every row start, which
// the callers check with the row pointer and stride of each segment).
static bool state_aligned(const UpdArgs& u, const void* param_out, int vec) {
  return aligned(u.master, vec * 4) && aligned(u.s1, vec * 4) && aligned(u.s2, vec * 4) &&
         aligned(u.gout, vec * 4) && aligned(param_out, vec * (u.param_f32 ? 4 : 2));
}

template <class F>
static hipError_t agg_update_f(int opt, const SrcArgs& s, const UpdArgs& u, int64_t D,
                               hipStream_t st, const float* mix) {
  if (D <= 0) return hipSuccess;
  constexpr int esz = sizeof(typename F::T);
  const int vec = F::vec(F::np(s.n), true);
  const bool ok = (s.ld % vec) == 0 && aligned(s.X, vec * esz) && state_aligned(u, u.param_out, vec);
  const int64_t Dv = ok ? (D / vec) * vec : 0;
  if (Dv > 0) launch<F, true>(opt, s, u, mix, 0, Dv, st);
  if (D > Dv) launch<F, false>(opt, s, u, mix, Dv, D - Dv, st);   // scalar tail (or unaligned inputs)
  return hipGetLastError();
}

static void set_seg(SegTable& t, int i, const AggSeg& g, int vec) {
  t.X[i] = g.X;
  t.ld[i] = g.ld;
  t.nvec[i] = g.D / vec;
  t.off[i] = g.off;
  t.pout[i] = g.param_out;
}

template <class F>
static hipError_t agg_update_multi_f(int opt, const SrcArgs& s, const UpdArgs& u,
                                     const AggSeg* segs, int nseg, hipStream_t st,
                                     const float* mix) {
  constexpr int esz = sizeof(typename F::T);
  const int vec = F::vec(F::np(s.n), true);
  bool ok = nseg <= kMaxSegs;
  SegTable t{};
  int64_t maxv = 0;
  for (int i = 0; ok && i < nseg; ++i) {
    const AggSeg& g = segs[i];
    ok = g.D > 0 && g.D % vec == 0 && (g.ld % vec) == 0 && aligned(g.X, vec * esz) &&
         g.off % vec == 0 && state_aligned(u, g.param_out, vec);
    set_seg(t, i, g, vec);
    maxv = t.nvec[i] > maxv ? t.nvec[i] : maxv;
  }
  if (!ok) {   // per-segment launches (unaligned / ragged segments)
    for (int i = 0; i < nseg; ++i) {
      SegTable one;
      set_seg(one, 0, segs[i], vec);
      SrcArgs s1 = s;
      UpdArgs u1 = u;
      seg_args(one, 0, s1, u1);
      hipError_t e = agg_update_f<F>(opt, s1, u1, segs[i].D, st, mix);
      if (e != hipSuccess) return e;
    }
    return hipGetLastError();
  }
  int gx = grid_for(maxv);
  const int cap = 2048 / nseg;
  if (gx > cap) gx = cap < 1 ? 1 : cap;
  const dim3 g(static_cast<unsigned>(gx), static_cast<unsigned>(nseg));
  with_kernel<F, true>(s.n, opt, [&](auto np, auto v, auto o) {
    constexpr int NP = decltype(np)::value, VEC = decltype(v)::value, OPT = decltype(o)::value;
    if constexpr (F::mix) agg_multi<F, NP, VEC, OPT, MixPtr><<<g, kBlock, 0, st>>>(s, u, mix, t);
    else agg_multi<F, NP, VEC, OPT><<<g, kBlock, 0, st>>>(s, u, t);
  });
  return hipGetLastError();
}

// The n, window, mix and keep checks of both entry points. keep: 0, or a sorted combine keeping at
// least half of the rows (near_combine's window needs f = n - keep <= keep). keep == n is the
// plain mean of all n rows: the fixed window [0, n).
static bool check_rule(int combine, SrcArgs& s, const float* mix) {
  if (s.n < 1 || s.n > kMaxRows) return false;
  if (combine == CMB_SORTED && (s.cnt < 1 || s.lo < 0 || s.lo + s.cnt > s.n)) return false;
  if (mix && (combine != CMB_SORTED || s.n > kMaxMixRows)) return false;
  if (s.keep == 0) return true;
  if (combine != CMB_SORTED || s.keep < 0 || s.keep > s.n || 2 * s.keep < s.n) return false;
  if (s.keep == s.n) {
    s.lo = 0;
    s.cnt = s.n;
    s.keep = 0;
  }
  return true;
}

hipError_t launch_agg_update_multi(int dtype, int combine, int opt, const SrcArgs& src,
                                   const UpdArgs& upd, const AggSeg* segs, int nseg,
                                   hipStream_t stream, const float* mix) {
  SrcArgs s = src;
  if (!check_rule(combine, s, mix) || nseg < 1) return hipErrorInvalidValue;
  hipError_t e = hipSuccess;
  with_form(dtype, combine, mix != nullptr, s.keep > 0, [&](auto f) {
    e = agg_update_multi_f<decltype(f)>(opt, s, upd, segs, nseg, stream, mix);
  });
  return e;
}

hipError_t launch_agg_update(int dtype, int combine, int opt, const SrcArgs& src,
                             const UpdArgs& upd, int64_t D, hipStream_t stream, const float* mix) {
  SrcArgs s = src;
  if (!check_rule(combine, s, mix)) return hipErrorInvalidValue;
  hipError_t e = hipSuccess;
  with_form(dtype, combine, mix != nullptr, s.keep > 0, [&](auto f) {
    e = agg_update_f<decltype(f)>(opt, s, upd, D, stream, mix);
  });
  return e;
}

}  // namespace cml
