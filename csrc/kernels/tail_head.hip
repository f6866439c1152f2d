// A layer-1 bottleneck's recompute tail with the NEXT block's conv1 inside it. The tail writes the
// block output y (256 channels) and the very next kernel in the stream, the following block's conv1
// (1x1, 256 -> p'), reads it straight back; the tail's workgroup holds the full 256-channel row of
// every pixel of its tile on chip, so conv1 is a second product from that tile and the 4-unit read
// of y disappears (a unit = one 64-channel tensor of the layer).
//   workgroup  8 waves, one per CU, a contiguous range of 64-pixel tiles
//   product 1  y^T = W A^T, A = relu(bn2(z2)) (identity tail, K = 64) or [relu(bn2(z2)) | x] (down
//              tail, K = 128, BN scales folded into W by the caller): wave w owns output channels
//              32 w .. + 31, its W block lives in registers as MFMA fragments for the whole kernel;
//              operand roles, k order and rounding points are those of conv1x1.hip's tail kernels
//              (bf16(acc), then fmaf(v, sc, bi) + res, ReLU, bit mask), so y and the mask are the
//              parent kernels' bit for bit
//   y tile     the bf16 y rows stay in LDS (32 KB) after they are stored
//   product 2  z1n^T = W1n y^T, K = 256, W1n resident in LDS; one 32 x 32 block per wave (p' = 64:
//              four waves multiply)
//   statistics shifted sums of the stored bf16 z1n (conv1x1.hip's SM_BN rule), per lane over the
//              workgroup's tiles, one partial row per workgroup in a fixed order (a workgroup
//              without pixels writes zeros; no atomics), finalized by launch_bn_stats_finalize
// The next tile's z2 / x / residual rows are in flight in registers while a tile is multiplied.
// Measurements: profiles/tail_head/README.md (bench/tail_head.py).
#include "common.h"
#include "kernels.h"
#include "wgrad_frag.h"

namespace cml {
namespace {

constexpr int kTP = 64;     // pixels per tile
constexpr int kNT = 512;    // threads per workgroup
constexpr int kCO = 256;    // output channels of the tail

struct THArgs {
  const uint16_t *z, *x2, *w, *res, *w1n;
  const float *sc2, *bi2, *ep_sc, *ep_bi, *shift;
  uint16_t *y, *z1n;
  uint8_t* ymask;
  float* part;
  int M, tpw;   // tpw: tiles per workgroup
};

// byte offset of 16-B chunk c of row `row` of a [rows][ROWB] image read as MFMA row operands
// (ds_read_b128: the 16 rows of a lane group on 16 distinct bank slots)
template <int ROWB>
__device__ __forceinline__ int roff(int row, int c) {
  if constexpr (ROWB == 128) return row * 128 + 16 * (c ^ ((row >> 1) & 7));
  return img_off<ROWB>(row, c);
}

// K: channels of the staged operand (64: z2; 128: z2 | x2). P2: the next conv1's output channels.
// RES: a residual is added in the first epilogue.
template <int K, int P2, bool RES>
__global__ __launch_bounds__(kNT) void tail_head_kernel(const THArgs a) {
  constexpr int AROWB = 2 * K, YROWB = 2 * kCO, ZROWB = 2 * P2;
  constexpr int KU = K / 64;                  // staged sources: z2 (BN + ReLU), x2 (as is)
  constexpr int XU = kTP * (kCO / 8) / kNT;   // y / residual items per thread and tile (4)
  constexpr int CZ = P2 / 8;                  // 16-B chunks of a z1n row
  constexpr int ZU = kTP * CZ / kNT;          // z1n items per thread and tile, one chunk column
  constexpr int NW2 = P2 / 16;                // waves of the second product
  static_assert(kTP * CZ % kNT == 0 && kNT % CZ == 0, "whole items per thread");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const aimg = smem;                         // [kTP][K] staged operand
  char* const yimg = aimg + kTP * AROWB;           // [kTP][256] bf16 product, then y
  char* const zimg = yimg + kTP * YROWB;           // [kTP][P2] z1n
  char* const wimg = zimg + kTP * ZROWB;           // [P2][256] W1n
  float* const cst = reinterpret_cast<float*>(wimg + P2 * YROWB);   // sc2 bi2 [64] esc ebi [256] sh [P2]
  float* const c_sc2 = cst;
  float* const c_bi2 = cst + 64;
  float* const c_esc = cst + 128;
  float* const c_ebi = c_esc + kCO;
  float* const c_sh = c_ebi + kCO;
  const int tid = threadIdx.x, lane = tid & 63;
  const int cw = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, r = lane & 31;
  const int M = a.M;
  const int ntile = (M + kTP - 1) / kTP;
  const int t_lo = min(ntile, static_cast<int>(blockIdx.x) * a.tpw);
  const int t_hi = min(ntile, t_lo + a.tpw);

  // W's block of this wave: element j of k step ks = W[32 cw + r][16 ks + 8 h + j]
  bf16x8_t wf[K / 16];
#pragma unroll
  for (int ks = 0; ks < K / 16; ++ks)
    wf[ks] = __builtin_bit_cast(
        bf16x8_t, *reinterpret_cast<const uint4*>(a.w + (32 * cw + r) * K + 16 * ks + 8 * h));
#pragma unroll
  for (int i = 0; i < P2 * (kCO / 8) / kNT; ++i) {
    const int row = (tid >> 5) + (kNT / 32) * i, c = tid & 31;
    *reinterpret_cast<uint4*>(wimg + roff<YROWB>(row, c)) =
        *reinterpret_cast<const uint4*>(a.w1n + row * kCO + 8 * c);
  }
  if (tid < 64) {
    c_sc2[tid] = a.sc2[tid];
    c_bi2[tid] = a.bi2[tid];
  }
  if (tid < kCO) {
    c_esc[tid] = a.ep_sc[tid];
    c_ebi[tid] = a.ep_bi[tid];
  }
  if (tid < P2) c_sh[tid] = a.shift ? a.shift[tid] : 0.f;
  __syncthreads();

  // staged items of this thread: row ar, 16-B chunk ac of source u
  const int ar = tid >> 3, ac = tid & 7;
  // y / residual items: rows xr + 16 j, 16-B chunk cx
  const int xr = tid >> 5, cx = tid & 31;
  // z1n items: rows zr + (kNT / CZ) u, 16-B chunk cz
  const int zr = tid / CZ, cz = tid % CZ;

  // prefetch registers: unconditional loads of a clamped pixel, zeroed or dropped at use
  uint4 av[KU], rv[XU];
  auto fetch = [&](int t) {
    const int64_t p = min(t * kTP + ar, M - 1);
    av[0] = *reinterpret_cast<const uint4*>(a.z + p * 64 + 8 * ac);
    if constexpr (KU == 2) av[1] = *reinterpret_cast<const uint4*>(a.x2 + p * 64 + 8 * ac);
    if constexpr (RES) {
#pragma unroll
      for (int j = 0; j < XU; ++j) {
        const int64_t q = min(t * kTP + xr + (kNT / 32) * j, M - 1);
        rv[j] = *reinterpret_cast<const uint4*>(a.res + q * kCO + 8 * cx);
      }
    }
  };
  uint4 rc[XU];
  auto stage = [&](int t) {
    float sc[8], bi[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      sc[q] = c_sc2[8 * ac + q];
      bi[q] = c_bi2[8 * ac + q];
    }
    const bool live = t * kTP + ar < M;
    const uint4 v = av[0];
    // rows at or beyond M are zeroed so that no NaN gets in; their outputs are dropped
    *reinterpret_cast<uint4*>(aimg + roff<AROWB>(ar, ac)) = keep_if(
        live, make_uint4(bnrelu_pk(v.x, f32x2{sc[0], sc[1]}, f32x2{bi[0], bi[1]}),
                         bnrelu_pk(v.y, f32x2{sc[2], sc[3]}, f32x2{bi[2], bi[3]}),
                         bnrelu_pk(v.z, f32x2{sc[4], sc[5]}, f32x2{bi[4], bi[5]}),
                         bnrelu_pk(v.w, f32x2{sc[6], sc[7]}, f32x2{bi[6], bi[7]})));
    if constexpr (KU == 2)
      *reinterpret_cast<uint4*>(aimg + roff<AROWB>(ar, 8 + ac)) = keep_if(live, av[1]);
#pragma unroll
    for (int j = 0; j < XU; ++j) rc[j] = RES ? rv[j] : make_uint4(0u, 0u, 0u, 0u);
  };

  // statistics of z1n: this thread's 8 channels 8 cz .. + 7
  float ss[8], sq[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) ss[q] = sq[q] = 0.f;

  if (t_lo < t_hi) fetch(t_lo);
  for (int t = t_lo; t < t_hi; ++t) {
    stage(t);
    fetch(t + 1 < t_hi ? t + 1 : t);   // past the end: a valid tile, dropped
    __syncthreads();
    // product 1: row = channel 32 cw + .., column = pixel 32 ph + r; ascending k
#pragma unroll
    for (int ph = 0; ph < kTP / 32; ++ph) {
      f32x16 acc = {};
#pragma unroll
      for (int ks = 0; ks < K / 16; ++ks) {
        const bf16x8_t B = *reinterpret_cast<const bf16x8_t*>(
            aimg + roff<AROWB>(32 * ph + r, 2 * ks + h));
        acc = mfma(wf[ks], B, acc);
      }
      // registers 4 g .. 4 g + 3 = channels 8 g + 4 h .. + 3 of the wave's 32: half h of chunk g
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<uint2*>(yimg + roff<YROWB>(32 * ph + r, 4 * cw + g) + 8 * h) =
            make_uint2(pk_bf16(acc[4 * g], acc[4 * g + 1]), pk_bf16(acc[4 * g + 2], acc[4 * g + 3]));
    }
    __syncthreads();
    // epilogue 1 (conv1x1_common.h's SM_BNRES row): y = max(bn(v) + res, 0), its bit mask, and
    // the y tile back into the image
    {
      float esc[8], ebi[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        esc[q] = c_esc[8 * cx + q];
        ebi[q] = c_ebi[8 * cx + q];
      }
#pragma unroll
      for (int j = 0; j < XU; ++j) {
        const int row = xr + (kNT / 32) * j;
        char* const yp = yimg + roff<YROWB>(row, cx);
        const uint4 v = *reinterpret_cast<const uint4*>(yp);
        const uint32_t r4[4] = {rc[j].x, rc[j].y, rc[j].z, rc[j].w};
        uint32_t w4[4] = {v.x, v.y, v.z, v.w};
        uint32_t bits = 0u;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float lo = fmaf(__uint_as_float(w4[q] << 16), esc[2 * q], ebi[2 * q]) +
                           __uint_as_float(r4[q] << 16);
          const float hi =
              fmaf(__uint_as_float(w4[q] & 0xffff0000u), esc[2 * q + 1], ebi[2 * q + 1]) +
              __uint_as_float(r4[q] & 0xffff0000u);
          bits |= (lo > 0.f ? 1u : 0u) << (2 * q);
          bits |= (hi > 0.f ? 1u : 0u) << (2 * q + 1);
          w4[q] = pk_bf16(fmaxf(lo, 0.f), fmaxf(hi, 0.f));
        }
        const uint4 o = make_uint4(w4[0], w4[1], w4[2], w4[3]);
        const int64_t p = static_cast<int64_t>(t) * kTP + row;
        const bool live = p < M;
        *reinterpret_cast<uint4*>(yp) = keep_if(live, o);
        if (live) {
          *reinterpret_cast<uint4*>(a.y + p * kCO + 8 * cx) = o;
          a.ymask[p * (kCO / 8) + cx] = static_cast<uint8_t>(bits);
        }
      }
    }
    __syncthreads();
    // product 2: row = channel 32 cb + .. of p', column = pixel 32 pb + r; ascending k
    if (cw < NW2) {
      const int cb = cw % (P2 / 32), pb = cw / (P2 / 32);
      f32x16 acc = {};
#pragma unroll
      for (int ks = 0; ks < kCO / 16; ++ks) {
        const bf16x8_t A = *reinterpret_cast<const bf16x8_t*>(
            wimg + roff<YROWB>(32 * cb + r, 2 * ks + h));
        const bf16x8_t B = *reinterpret_cast<const bf16x8_t*>(
            yimg + roff<YROWB>(32 * pb + r, 2 * ks + h));
        acc = mfma(A, B, acc);
      }
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<uint2*>(zimg + roff<ZROWB>(32 * pb + r, 4 * cb + g) + 8 * h) =
            make_uint2(pk_bf16(acc[4 * g], acc[4 * g + 1]), pk_bf16(acc[4 * g + 2], acc[4 * g + 3]));
    }
    __syncthreads();
    // z1n rows out as 16-B chunks, and the shifted sums of the stored values
    {
      float sh[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) sh[q] = c_sh[8 * cz + q];
#pragma unroll
      for (int u = 0; u < ZU; ++u) {
        const int row = zr + (kNT / CZ) * u;
        const uint4 v = *reinterpret_cast<const uint4*>(zimg + roff<ZROWB>(row, cz));
        const int64_t p = static_cast<int64_t>(t) * kTP + row;
        if (p < M) {
          *reinterpret_cast<uint4*>(a.z1n + p * P2 + 8 * cz) = v;
          const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float lo = __uint_as_float(w4[q] << 16) - sh[2 * q];
            const float hi = __uint_as_float(w4[q] & 0xffff0000u) - sh[2 * q + 1];
            ss[2 * q] += lo;
            ss[2 * q + 1] += hi;
            sq[2 * q] = fmaf(lo, lo, sq[2 * q]);
            sq[2 * q + 1] = fmaf(hi, hi, sq[2 * q + 1]);
          }
        }
      }
    }
    // the next stage writes aimg (last read before the second barrier); yimg, zimg and the
    // images' next writes all come after the next tile's first barrier or later
  }
  // one partial row [2][P2] per workgroup: the threads of a chunk column summed in thread order
  __syncthreads();
  float* const red = reinterpret_cast<float*>(yimg);   // [kNT][16]
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    red[16 * tid + q] = ss[q];
    red[16 * tid + 8 + q] = sq[q];
  }
  __syncthreads();
  if (tid < 2 * P2) {
    const int which = tid / P2, ch = tid % P2;
    const float* src = red + 16 * (ch >> 3) + 8 * which + (ch & 7);
    float s = 0.f;
    for (int k = 0; k < kNT / CZ; ++k) s += src[16 * CZ * k];
    a.part[static_cast<int64_t>(blockIdx.x) * 2 * P2 + tid] = s;
  }
}

template <int K, int P2, bool RES>
hipError_t launch_k(const THArgs& a, int S, hipStream_t st) {
  constexpr int LDS = kTP * 2 * K + kTP * 2 * kCO + kTP * 2 * P2 + P2 * 2 * kCO +
                      (128 + 2 * kCO + P2) * 4;   // 83 .. 131 KiB: one workgroup per CU
  const hipError_t e =
      hipFuncSetAttribute(reinterpret_cast<const void*>(&tail_head_kernel<K, P2, RES>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, LDS);   // per device
  if (e != hipSuccess) return e;
  tail_head_kernel<K, P2, RES><<<S, kNT, LDS, st>>>(a);
  return hipGetLastError();
}

}  // namespace

bool tail_head_plan(int64_t M, int p, int Cout, int p2, int* wgs, int want) {
  if (p != 64 || Cout != kCO || (p2 != 64 && p2 != 128)) return false;
  if (M < 1 || M >= (1ll << 31) - 2 * kTP || want < 0 || want > 4096) return false;
  const int ntile = static_cast<int>((M + kTP - 1) / kTP);
  // one workgroup per CU; `want` (tests): that many pixel ranges, empty ones included
  int S = want ? want : 256;
  const int tpw = (ntile + S - 1) / S;
  if (!want) S = (ntile + tpw - 1) / tpw;
  *wgs = S;
  return true;
}

hipError_t launch_tail_head(const void* z, const void* x2, const void* w, const float* sc2,
                            const float* bi2, const float* ep_sc, const float* ep_bi,
                            const void* res, void* y, uint8_t* ymask, const void* w1n, void* z1n,
                            const float* shift, float* part, int wgs, float* mean, float* invstd,
                            float* rmean, float* rvar, float eps, float momentum,
                            const BnAffineOut* aff, int64_t M, int p, int Cout, int p2,
                            hipStream_t st) {
  int S;
  if (!tail_head_plan(M, p, Cout, p2, &S, 0) || wgs < 1 || wgs > 4096) return hipErrorInvalidValue;
  if (!z || !w || !sc2 || !bi2 || !ep_sc || !ep_bi || !y || !ymask || !w1n || !z1n || !part ||
      !mean || !invstd)
    return hipErrorInvalidValue;
  if ((x2 != nullptr) == (res != nullptr)) return hipErrorInvalidValue;   // down: no residual
  for (const void* q : {z, x2, w, res, w1n, static_cast<const void*>(y),
                        static_cast<const void*>(z1n)})
    if (reinterpret_cast<uintptr_t>(q) % 16) return hipErrorInvalidValue;
  THArgs a{};
  a.z = reinterpret_cast<const uint16_t*>(z);
  a.x2 = reinterpret_cast<const uint16_t*>(x2);
  a.w = reinterpret_cast<const uint16_t*>(w);
  a.res = reinterpret_cast<const uint16_t*>(res);
  a.w1n = reinterpret_cast<const uint16_t*>(w1n);
  a.sc2 = sc2;
  a.bi2 = bi2;
  a.ep_sc = ep_sc;
  a.ep_bi = ep_bi;
  a.shift = shift;
  a.y = reinterpret_cast<uint16_t*>(y);
  a.z1n = reinterpret_cast<uint16_t*>(z1n);
  a.ymask = ymask;
  a.part = part;
  a.M = static_cast<int>(M);
  const int ntile = static_cast<int>((M + kTP - 1) / kTP);
  a.tpw = (ntile + wgs - 1) / wgs;
  hipError_t e;
  if (x2)
    e = p2 == 64 ? launch_k<128, 64, false>(a, wgs, st) : launch_k<128, 128, false>(a, wgs, st);
  else
    e = p2 == 64 ? launch_k<64, 64, true>(a, wgs, st) : launch_k<64, 128, true>(a, wgs, st);
  if (e != hipSuccess) return e;
  return launch_bn_stats_finalize(part, wgs, p2, p2, M, shift, eps, momentum, mean, invstd, rmean,
                                  rvar, st, nullptr, aff);
}

}  // namespace cml
