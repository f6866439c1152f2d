// Gram matrix of an NHWC bf16 activation over its pixels, G = y^T y (fp32 [p][p]) with
// y = bf16(max(z sc + bi, 0)) (or y = z), and the column sums of y: the BN statistics of the
// recompute tails (ops.conv._RecomputeTailFn). The general weight-gradient kernel (wgrad1x1.hip)
// computes the same product as dW of (z, z): it loads, transforms and stages the tensor twice and
// multiplies both triangles. Here every element of z is loaded once, transformed once and written
// to LDS once; both MFMA operands come from that one image through ds_read_b64_tr_b16 (k = pixel),
// a workgroup covers all p channels of a range of pixels, and no tile below the diagonal is
// multiplied. Split-K partials hold the tiles that were; one fold launch sums them in a fixed
// order and writes G, its mirror and the column sums (no atomics: bit-reproducible).
//   p = 64        4 independent waves per workgroup: each has its own two-stage LDS region, its
//                 own interleaved 64-pixel chunks and three accumulators (the 32 x 32 blocks 00, 01,
//                 11), so the loop has no workgroup barrier; the waves' sums are added through LDS
//                 at the end
//   p = 128, 256  one [64 px][p] image per stage shared by the workgroup (one barrier per chunk);
//                 one wave per 64 x 64 tile on or above the diagonal: 3 of 4 tiles at p = 128,
//                 10 of 16 at p = 256
// Measurements: profiles/gram_syrk/README.md (bench/gram.py).
#include <cstdlib>

#include "common.h"
#include "kernels.h"
#include "wgrad_frag.h"

namespace cml {
namespace {

constexpr int kKC = 64;     // pixels per chunk
constexpr int kNW64 = 4;    // waves per workgroup at p = 64

// the staged values of 8 channels: max(z sc + bi, 0) rounded to bf16 as wgrad1x1.hip's prologues
// round it
template <bool PRO>
__device__ __forceinline__ uint4 bnrelu8(uint4 v, const float (&sc)[8], const float (&bi)[8]) {
  if constexpr (PRO) {
    uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float lo = fmaxf(fmaf(__uint_as_float(w4[i] << 16), sc[2 * i], bi[2 * i]), 0.f);
      const float hi =
          fmaxf(fmaf(__uint_as_float(w4[i] & 0xffff0000u), sc[2 * i + 1], bi[2 * i + 1]), 0.f);
      w4[i] = static_cast<uint32_t>(f2bf(lo)) | (static_cast<uint32_t>(f2bf(hi)) << 16);
    }
    return make_uint4(w4[0], w4[1], w4[2], w4[3]);
  }
  return v;
}

__device__ __forceinline__ void colsum8(uint4 v, float (&cs)[8]) {
  const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    cs[2 * i] += __uint_as_float(w4[i] << 16);
    cs[2 * i + 1] += __uint_as_float(w4[i] & 0xffff0000u);
  }
}

// orders this wave's LDS stores and its transposed reads of other lanes' stores in the compiled
// code; the LDS executes one wave's instructions in order, so no wait is needed
__device__ __forceinline__ void wave_order() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
}

// the two 32-channel operand fragments of 64-channel tile t at k step ks of a staged image
template <int ROWB>
__device__ __forceinline__ void frag2(const char* img, int t, int ks, int lane, bf16x8_t (&A)[2]) {
  const int h = lane >> 5, gi = lane & 15, grp = lane >> 4, q = gi >> 2, pq = gi & 3;
  const int r0 = 16 * ks + 8 * h + q;
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int ch = 8 * t + 4 * b + 2 * (grp & 1) + (pq >> 1);
    A[b] = cat(ld_tr(img + img_off<ROWB>(r0, ch) + 8 * (pq & 1)),
               ld_tr(img + img_off<ROWB>(r0 + 4, ch) + 8 * (pq & 1)));
  }
}

// the column sums of the workgroup: the threads of each 8-channel group (tid % CA), fixed order
template <int NT, int CA>
__device__ __forceinline__ void fold_colsums(float* red, const float (&cs)[8], int tid,
                                             float* __restrict__ out) {
#pragma unroll
  for (int q = 0; q < 8; ++q) red[tid * 8 + q] = cs[q];
  __syncthreads();
  if (tid < CA) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      float v = 0.f;
      for (int k = tid; k < NT; k += CA) v += red[k * 8 + q];
      out[8 * tid + q] = v;
    }
  }
}

// p = 64. part [split][64][64]: blocks (0,0), (0,1), (1,1) written, (1,0) left alone.
template <bool PRO>
__global__ __launch_bounds__(kNW64 * 64) void gram64_kernel(
    const uint16_t* __restrict__ z, float* __restrict__ part, int M, int cps,
    const float* __restrict__ sc, const float* __restrict__ bi, float* __restrict__ cs_part) {
  constexpr int ROWB = 128, STG = kKC * ROWB, NT = kNW64 * 64;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // kNW64 waves x 2 stages
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nchunk = (M + kKC - 1) / kKC;
  // this wave's chunks: c_lo, c_lo + kNW64, ... below c_hi
  const int c_lo = blockIdx.x * cps + wave;
  const int c_hi = min(nchunk, (static_cast<int>(blockIdx.x) + 1) * cps);
  char* my = smem + wave * 2 * STG;
  // item j of a chunk: row row0 + 8 j, 16-B chunk ch (the same 8 channels for every item)
  const int ch = lane & 7, row0 = lane >> 3;
  float psc[8], pbi[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    psc[q] = PRO ? sc[8 * ch + q] : 0.f;
    pbi[q] = PRO ? bi[8 * ch + q] : 0.f;
  }
  // prefetch registers: unconditional loads of a clamped pixel, zeroed at use
  uint4 pv[8];
  auto fetch = [&](int c) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int p = min(c * kKC + row0 + 8 * j, M - 1);
      pv[j] = *reinterpret_cast<const uint4*>(z + static_cast<int64_t>(p) * 64 + 8 * ch);
    }
  };
  const bool csum = cs_part != nullptr;
  float cs[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) cs[q] = 0.f;
  auto stage = [&](int c, int sb) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int row = row0 + 8 * j;
      // rows at or beyond M are zeroed after the transform: relu(0 sc + bi) is not 0
      const uint4 v = keep_if(c * kKC + row < M, bnrelu8<PRO>(pv[j], psc, pbi));
      *reinterpret_cast<uint4*>(my + sb * STG + img_off<ROWB>(row, ch)) = v;
      if (csum) colsum8(v, cs);
    }
  };
  f32x16 acc[3] = {};
  if (c_lo < c_hi) {
    fetch(c_lo);
    stage(c_lo, 0);
    fetch(c_lo + kNW64 < c_hi ? c_lo + kNW64 : c_lo);
  }
  int sb = 0;
  for (int c = c_lo; c < c_hi; c += kNW64, sb ^= 1) {
    wave_order();
    const char* img = my + sb * STG;
#pragma unroll
    for (int ks = 0; ks < kKC / 16; ++ks) {
      bf16x8_t A[2];
      frag2<ROWB>(img, 0, ks, lane, A);
      acc[0] = mfma(A[0], A[0], acc[0]);
      acc[1] = mfma(A[0], A[1], acc[1]);
      acc[2] = mfma(A[1], A[1], acc[2]);
    }
    wave_order();
    if (c + kNW64 < c_hi) stage(c + kNW64, sb ^ 1);            // uniform branch
    fetch(c + 2 * kNW64 < c_hi ? c + 2 * kNW64 : c);           // past the end: a valid chunk
  }
  // the waves' accumulators through LDS (their stage regions are free once every wave is done),
  // added in wave order
  __syncthreads();
  float* red = reinterpret_cast<float*>(smem);   // [wave][block][register][lane]
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int k = 0; k < 16; ++k) red[((wave * 3 + t) * 16 + k) * 64 + lane] = acc[t][k];
  __syncthreads();
  float* pw = part + static_cast<int64_t>(blockIdx.x) * 64 * 64;
#pragma unroll
  for (int u = 0; u < 3 * 16 * 64 / NT; ++u) {
    const int idx = tid + NT * u;
    float v = red[idx];
#pragma unroll
    for (int w = 1; w < kNW64; ++w) v += red[w * 3 * 16 * 64 + idx];
    // lane l = column l & 31, register k = row (k & 3) + 8 (k >> 2) + 4 (l >> 5)
    const int t = idx >> 10, k = (idx >> 6) & 15, l = idx & 63;
    const int row = (t == 2 ? 32 : 0) + (k & 3) + 8 * (k >> 2) + 4 * (l >> 5);
    const int col = (t >= 1 ? 32 : 0) + (l & 31);
    pw[row * 64 + col] = v;
  }
  if (csum) {
    __syncthreads();
    fold_colsums<NT, 8>(red, cs, tid, cs_part + static_cast<int64_t>(blockIdx.x) * 64);
  }
}

// p = PC in {128, 256}. Wave w owns the w-th 64 x 64 tile (ti, tj) with ti <= tj, in row-major order
// ((0,0) (0,1) (1,1) at 128, where a fourth wave only stages; ten waves at 256); a diagonal tile is
// multiplied whole. part [split][PC][PC]: those tiles written, the others left alone.
template <int PC>
constexpr int gram_wide_threads() { return PC == 256 ? 640 : 256; }

template <int PC, bool PRO>
__global__ __launch_bounds__(gram_wide_threads<PC>(), 3) void gram_wide_kernel(
    const uint16_t* __restrict__ z, float* __restrict__ part, int M, int cps,
    const float* __restrict__ sc, const float* __restrict__ bi, float* __restrict__ cs_part) {
  constexpr int NT = gram_wide_threads<PC>(), ROWB = PC * 2, CA = PC / 8, STG = kKC * ROWB;
  constexpr int ITEMS = kKC * CA, IA = (ITEMS + NT - 1) / NT;   // 16-B items per chunk, per thread
  constexpr int T = PC / 64;
  static_assert(NT % CA == 0 && NT / 64 >= T * (T + 1) / 2, "staged items / one wave per tile");
  extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 stages of [kKC][PC]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, r = lane & 31;
  const bool work = wave < T * (T + 1) / 2;             // uniform per wave
  int ti = 0, tj = 0;
  if (work) {
    int w = wave;
    while (w >= T - ti) w -= T - ti++;
    tj = ti + w;
  }
  const int nchunk = (M + kKC - 1) / kKC;
  const int c_lo = blockIdx.x * cps;
  const int c_hi = min(nchunk, c_lo + cps);
  // every staged item of this thread covers the same 8 channels (NT is a multiple of CA)
  const int ch = tid % CA;
  float psc[8], pbi[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    psc[q] = PRO ? sc[8 * ch + q] : 0.f;
    pbi[q] = PRO ? bi[8 * ch + q] : 0.f;
  }
  // prefetch registers: unconditional loads of a clamped pixel (items past the chunk included,
  // where NT does not divide ITEMS), zeroed or dropped at use
  uint4 pv[IA];
  auto fetch = [&](int c) {
#pragma unroll
    for (int j = 0; j < IA; ++j) {
      const int row = (tid + NT * j) / CA;
      const int p = min(c * kKC + row, M - 1);
      pv[j] = *reinterpret_cast<const uint4*>(z + static_cast<int64_t>(p) * PC + 8 * ch);
    }
  };
  const bool csum = cs_part != nullptr;
  float cs[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) cs[q] = 0.f;
  auto stage = [&](int c, int sb) {
#pragma unroll
    for (int j = 0; j < IA; ++j) {
      const int row = (tid + NT * j) / CA;
      if (ITEMS % NT == 0 || row < kKC) {
        // rows at or beyond M are zeroed after the transform: relu(0 sc + bi) is not 0
        const uint4 v = keep_if(c * kKC + row < M, bnrelu8<PRO>(pv[j], psc, pbi));
        *reinterpret_cast<uint4*>(smem + sb * STG + img_off<ROWB>(row, ch)) = v;
        if (csum) colsum8(v, cs);
      }
    }
  };
  f32x16 acc[2][2] = {};
  if (c_lo < c_hi) {
    fetch(c_lo);
    stage(c_lo, 0);
    fetch(c_lo + 1 < c_hi ? c_lo + 1 : c_lo);
  }
  __syncthreads();
  // two LDS stages: chunk c is multiplied out of stage c & 1 while chunk c + 1 is written into the
  // other stage from registers and chunk c + 2 is in flight -> one barrier per chunk
  for (int c = c_lo; c < c_hi; ++c) {
    const int sb = (c - c_lo) & 1;
    const char* img = smem + sb * STG;
    if (work) {
#pragma unroll
      for (int ks = 0; ks < kKC / 16; ++ks) {
        bf16x8_t A[2], B[2];
        frag2<ROWB>(img, ti, ks, lane, A);
        frag2<ROWB>(img, tj, ks, lane, B);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = mfma(A[i], B[j], acc[i][j]);
      }
    }
    if (c + 1 < c_hi) stage(c + 1, sb ^ 1);            // uniform branch; loads stay unconditional
    fetch(c + 2 < c_hi ? c + 2 : c);                   // past the end: reload a valid chunk
    __syncthreads();
  }
  if (csum)
    fold_colsums<NT, CA>(reinterpret_cast<float*>(smem), cs, tid,
                         cs_part + static_cast<int64_t>(blockIdx.x) * PC);
  if (!work) return;
  // lane r = column, register k = row (k & 3) + 8 (k >> 2) + 4 h of each 32 x 32 block
  float* pw = part + static_cast<int64_t>(blockIdx.x) * PC * PC;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int k = 0; k < 16; ++k)
        pw[(64 * ti + 32 * i + (k & 3) + 8 * (k >> 2) + 4 * h) * PC + 64 * tj + 32 * j + r] =
            acc[i][j][k];
}

// G = sum over the S partials (fixed order) of the blocks on or above the diagonal, written with
// its mirror (of a diagonal block only the elements on or above the diagonal are taken, so G is
// bitwise symmetric), and cy = sum of the S column-sum rows, in one launch: blocks [0, b1) fold
// 64 elements of G each, the others 64 of cy. 16 split lanes per 4 outputs, as wgrad1x1.hip's
// wide fold: lane sl sums splits sl, sl + 16, ..., then lane 0 adds the 16 sums in lane order.
__global__ __launch_bounds__(256) void gram_fold_kernel(const float* __restrict__ part, int S,
                                                        int p, float* __restrict__ G,
                                                        const float* __restrict__ cs_part,
                                                        float* __restrict__ cy, int b1) {
  __shared__ float4 red[16][17];
  const int cg = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int b = blockIdx.x;
  const bool gram = b < b1;
  const float* __restrict__ src = gram ? part : cs_part;
  const int n = gram ? p * p : p;
  const int e = ((gram ? b : b - b1) * 16 + cg) * 4;
  const int row = e / p, col = e - row * p;
  const bool live = e < n && (!gram || (row >> 5) <= (col >> 5));
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) {
    int k = sl;
    for (; k + 7 * 16 < S; k += 8 * 16) {
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        v[u] = *reinterpret_cast<const float4*>(src + static_cast<int64_t>(k + 16 * u) * n + e);
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        s.x += v[u].x;
        s.y += v[u].y;
        s.z += v[u].z;
        s.w += v[u].w;
      }
    }
    for (; k < S; k += 16) {
      const float4 v = *reinterpret_cast<const float4*>(src + static_cast<int64_t>(k) * n + e);
      s.x += v.x;
      s.y += v.y;
      s.z += v.z;
      s.w += v.w;
    }
  }
  red[sl][cg] = s;
  __syncthreads();
  if (sl != 0 || !live) return;
#pragma unroll
  for (int j = 1; j < 16; ++j) {
    const float4 v = red[j][cg];
    s.x += v.x;
    s.y += v.y;
    s.z += v.z;
    s.w += v.w;
  }
  if (!gram) {
    *reinterpret_cast<float4*>(cy + e) = s;
    return;
  }
  const float v[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = col + i;
    if (c >= row) {
      G[row * p + c] = v[i];
      G[c * p + row] = v[i];
    }
  }
}

// CML_GRAM_SYRK=0 keeps the Gram calls on the weight-gradient kernel (A/B)
bool syrk_enabled() {
  static const bool on = [] {
    const char* e = getenv("CML_GRAM_SYRK");
    return !(e && e[0] == '0');
  }();
  return on;
}

}  // namespace

bool gram1x1_route(const void* dy, const void* x, int Co, int Ci, const float* pro_sc,
                   const float* pro_bi, int dmode, const float* dz_a, const float* dz_b,
                   bool dw_bf16) {
  if (!syrk_enabled() || dy != x || Co != Ci || dw_bf16) return false;
  if (Co != 64 && Co != 128 && Co != 256) return false;
  if (dmode == 3) return pro_sc != nullptr && dz_a == pro_sc && dz_b == pro_bi;
  return dmode == 0 && pro_sc == nullptr && pro_bi == nullptr;
}

void gram1x1_plan(int64_t M, int p, int* splits, int* cps) {
  const int nchunk = static_cast<int>((M + kKC - 1) / kKC);
  // p = 64, 128: two workgroups per CU (64 / 32 KiB of LDS each); p = 256: one, its partial is
  // 160 KiB per split
  const int target = p == 256 ? 256 : 512;
  int c = (nchunk + target - 1) / target;
  if (p == 64) c = (c + kNW64 - 1) / kNW64 * kNW64;   // whole rounds of the interleaved waves
  *cps = c;
  *splits = (nchunk + c - 1) / c;
}

hipError_t launch_gram1x1(const void* z, float* part, float* G, int64_t M, int p, const float* sc,
                          const float* bi, float* cs_part, float* cy, hipStream_t st) {
  if (M < 1 || M >= (1ll << 31) - kKC || (p != 64 && p != 128 && p != 256))
    return hipErrorInvalidValue;
  if (!z || !part || !G || (sc == nullptr) != (bi == nullptr) ||
      (cs_part == nullptr) != (cy == nullptr) || reinterpret_cast<uintptr_t>(z) % 16)
    return hipErrorInvalidValue;
  int S, cps;
  gram1x1_plan(M, p, &S, &cps);
  const auto* zp = reinterpret_cast<const uint16_t*>(z);
  const int Mi = static_cast<int>(M);
  const size_t lds = p == 64 ? kNW64 * 2 * kKC * 128 : 2 * static_cast<size_t>(kKC) * p * 2;
  auto go = [&](auto k, int nt) { k<<<S, nt, lds, st>>>(zp, part, Mi, cps, sc, bi, cs_part); };
  if (p == 64) {
    if (sc) go(gram64_kernel<true>, kNW64 * 64);
    else go(gram64_kernel<false>, kNW64 * 64);
  } else if (p == 128) {
    if (sc) go(gram_wide_kernel<128, true>, gram_wide_threads<128>());
    else go(gram_wide_kernel<128, false>, gram_wide_threads<128>());
  } else {
    if (sc) go(gram_wide_kernel<256, true>, gram_wide_threads<256>());
    else go(gram_wide_kernel<256, false>, gram_wide_threads<256>());
  }
  const int b1 = p * p / 64, b2 = cy ? p / 64 : 0;
  gram_fold_kernel<<<b1 + b2, 256, 0, st>>>(part, S, p, G, cs_part, cy, b1);
  return hipGetLastError();
}

}  // namespace cml
