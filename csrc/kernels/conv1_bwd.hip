// Backward of a bottleneck's conv1 (1x1, Cin -> p) with bn1's apply pass inside it: bn1's input
// gradient dz1 = bn_bwd_apply(dy1, z1) is read by two products, the data gradient dx = dz1 W1 (+ the
// parked residual gradient) and the weight gradient dW1 = dz1^T x. As three launches dz1 is written
// once and read twice; here one workgroup forms each 64-pixel tile of dz1 once, in LDS, and both
// products take it from there, so the apply pass's traffic (read dy1, read z1, write dz1) shrinks
// to the two reads and the consumers' two reads of dz1 disappear.
//   workgroup  8 waves, one workgroup per CU; one 256-channel slice of Cin (two slices at Cin =
//              512: the second re-reads dy1 / z1, placed on the same XCD so that it hits in L2)
//              and a contiguous range of 64-pixel tiles. Wave w owns channels 32 w .. + 31 of the
//              slice.
//   W1         the wave's p x 32 block lives in registers as MFMA fragments for the whole kernel
//   dW1        p x 32 fp32 accumulators per wave over the workgroup's pixels -> one partial slab
//              per workgroup, folded in a fixed order by launch_wgrad_fold (no atomics; a
//              workgroup without pixels writes zeros)
//   dx         dx^T = W1^T dz1^T per tile (pixel on the lane, 4 consecutive channels per register
//              group), rounded to bf16 into an LDS image and read back as 16-B row chunks for the
//              link epilogue of conv1x1_common.h's EL rule: bf16(bf16(acc) + (bit ? link : 0))
// The next tile's x, dy1, z1 and link rows (about 100 KB per CU) are in flight in registers while
// a tile is multiplied; bn1's per-channel constants stay in LDS to leave room for them.
// Measurements: profiles/conv1_bwd/README.md (bench/conv1_bwd.py).
#include "common.h"
#include "kernels.h"
#include "wgrad_frag.h"

namespace cml {
namespace {

constexpr int kTP = 64;     // pixels per tile
constexpr int kNT = 512;    // threads per workgroup
constexpr int kSL = 256;    // channels per slice of Cin

enum { LK_NONE = 0, LK_MASK = 1, LK_S2 = 2 };

struct C1BArgs {
  const uint16_t *dy, *z, *x, *w, *g;
  const uint8_t* gm;
  const uint16_t *gamma, *beta;
  const float *mean, *invstd, *sdz, *sdzx;
  uint16_t *dx, *dz;
  float* part;
  int M, Cin, tpw, slices;   // tpw: tiles per workgroup
  int W, HW, OW, OHW;        // LK_S2: full-resolution row / image, compact row / image (pixels)
};

// the 32-channel operand fragment (channels of 16-B chunks c0 .. c0 + 3) at k step ks of a
// [pixel][channel] image, k = pixel: gram1x1.hip's frag2 for one block
template <int ROWB>
__device__ __forceinline__ bf16x8_t frag32(const char* img, int c0, int ks, int lane) {
  const int h = lane >> 5, gi = lane & 15, grp = lane >> 4, q = gi >> 2, pq = gi & 3;
  const int r0 = 16 * ks + 8 * h + q;
  const int ch = c0 + 2 * (grp & 1) + (pq >> 1);
  return cat(ld_tr(img + img_off<ROWB>(r0, ch) + 8 * (pq & 1)),
             ld_tr(img + img_off<ROWB>(r0 + 4, ch) + 8 * (pq & 1)));
}

// bf16(bf16 v + (bit ? l : 0)) of 8 channels
__device__ __forceinline__ uint4 add_link8(uint4 v, uint4 l, uint32_t lb) {
  const uint32_t l4[4] = {l.x, l.y, l.z, l.w};
  uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float lo = __uint_as_float(w4[q] << 16) +
                     (((lb >> (2 * q)) & 1u) ? __uint_as_float(l4[q] << 16) : 0.f);
    const float hi = __uint_as_float(w4[q] & 0xffff0000u) +
                     (((lb >> (2 * q + 1)) & 1u) ? __uint_as_float(l4[q] & 0xffff0000u) : 0.f);
    w4[q] = pk_bf16(lo, hi);
  }
  return make_uint4(w4[0], w4[1], w4[2], w4[3]);
}

template <int P, int LK>
__global__ __launch_bounds__(kNT) void conv1_bwd_kernel(const C1BArgs a) {
  constexpr int ZROWB = 2 * P, XROWB = 2 * kSL;
  constexpr int CA = P / 8;               // 16-B chunks of a dz1 row
  constexpr int ZU = kTP * CA / kNT;      // dz1 items per thread and tile (1 or 2), one chunk column
  constexpr int XU = kTP * (kSL / 8) / kNT;   // x / link / dx items per thread and tile
  static_assert(kTP * CA % kNT == 0 && kNT % CA == 0 && kNT % 32 == 0, "whole items per thread");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const ximg = smem;                       // [kTP][256] x
  char* const oimg = ximg + kTP * XROWB;         // [kTP][256] bf16(dx product)
  char* const zimg = oimg + kTP * XROWB;         // [kTP][P] dz1
  float* const cst = reinterpret_cast<float*>(zimg + kTP * ZROWB);   // [6][P] sc bi mu is a b
  const int tid = threadIdx.x, lane = tid & 63;
  const int cw = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, r = lane & 31;
  // two slices: workgroups b and b + 8 (the same XCD) take the two slices of one pixel range
  const int b = blockIdx.x;
  const int slice = a.slices == 2 ? (b >> 3) & 1 : 0;
  const int range = a.slices == 2 ? ((b >> 4) << 3) | (b & 7) : b;
  const int Cin = a.Cin, M = a.M;
  const int cin0 = slice * kSL;
  const int ntile = (M + kTP - 1) / kTP;
  const int t_lo = min(ntile, range * a.tpw);
  const int t_hi = min(ntile, t_lo + a.tpw);

  // W1's block of this wave: element j of k step ks = W1[16 ks + 8 h + j][cin0 + 32 cw + r]
  bf16x8_t wf[P / 16];
#pragma unroll
  for (int ks = 0; ks < P / 16; ++ks) {
    bf16x8 t;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      t[j] = static_cast<short>(
          a.w[static_cast<int64_t>(16 * ks + 8 * h + j) * Cin + cin0 + 32 * cw + r]);
    wf[ks] = __builtin_bit_cast(bf16x8_t, t);
  }
  if (tid < P) {
    const float invM = 1.0f / static_cast<float>(static_cast<int64_t>(M));
    const float m = a.mean[tid], i = a.invstd[tid];
    float s, o;
    bn_chan_affine(m, i, bf2f(a.gamma[tid]), bf2f(a.beta[tid]), s, o);
    cst[tid] = s;
    cst[P + tid] = o;
    cst[2 * P + tid] = m;
    cst[3 * P + tid] = i;
    cst[4 * P + tid] = a.sdz[tid] * invM;
    cst[5 * P + tid] = a.sdzx[tid] * invM;
  }
  __syncthreads();
  // dz1 items of this thread: rows zr + (kNT / CA) u, 16-B chunk cz
  const int zr = tid / CA, cz = tid % CA;
  // x / link / dx items: rows xr + 16 j, 16-B chunk cx of the slice
  const int xr = tid >> 5, cx = tid & 31;

  // prefetch registers: unconditional loads of a clamped pixel, zeroed or dropped at use
  uint4 xv[XU], gv[XU], dyv[ZU], zv[ZU];
  uint32_t gb[XU];
  auto fetch = [&](int t) {
#pragma unroll
    for (int j = 0; j < XU; ++j) {
      const int p = min(t * kTP + xr + (kNT / 32) * j, M - 1);
      const int64_t e0 = static_cast<int64_t>(p) * Cin + cin0 + 8 * cx;
      xv[j] = *reinterpret_cast<const uint4*>(a.x + e0);
      if constexpr (LK == LK_MASK) {
        gv[j] = *reinterpret_cast<const uint4*>(a.g + e0);
        gb[j] = a.gm[e0 >> 3];
      } else if constexpr (LK == LK_S2) {   // compact stride-2 gradient: even pixels only
        const int img = p / a.HW, rem = p - img * a.HW;
        const int hh = rem / a.W, ww = rem - hh * a.W;
        const bool ev = !((hh | ww) & 1);
        const int64_t lrow =
            ev ? static_cast<int64_t>(img) * a.OHW + (hh >> 1) * a.OW + (ww >> 1) : 0;
        gv[j] = *reinterpret_cast<const uint4*>(a.g + lrow * Cin + cin0 + 8 * cx);
        gb[j] = ev ? 0xffu : 0u;
      }
    }
#pragma unroll
    for (int u = 0; u < ZU; ++u) {
      const int p = min(t * kTP + zr + (kNT / CA) * u, M - 1);
      dyv[u] = *reinterpret_cast<const uint4*>(a.dy + static_cast<int64_t>(p) * P + 8 * cz);
      zv[u] = *reinterpret_cast<const uint4*>(a.z + static_cast<int64_t>(p) * P + 8 * cz);
    }
  };
  uint4 gc[XU];
  uint32_t gcb[XU];
  auto stage = [&](int t) {
#pragma unroll
    for (int j = 0; j < XU; ++j) {
      const int row = xr + (kNT / 32) * j;
      // rows at or beyond M multiply a zero dz1 row; zeroed too so that no NaN gets in
      *reinterpret_cast<uint4*>(ximg + img_off<XROWB>(row, cx)) =
          keep_if(t * kTP + row < M, xv[j]);
      if constexpr (LK != LK_NONE) {
        gc[j] = gv[j];
        gcb[j] = gb[j];
      }
    }
    uint32_t o4[ZU][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {   // two channels at a time: few constants live
      const float2 sc = *reinterpret_cast<const float2*>(cst + 8 * cz + 2 * q);
      const float2 bi = *reinterpret_cast<const float2*>(cst + P + 8 * cz + 2 * q);
      const float2 mu = *reinterpret_cast<const float2*>(cst + 2 * P + 8 * cz + 2 * q);
      const float2 is = *reinterpret_cast<const float2*>(cst + 3 * P + 8 * cz + 2 * q);
      const float2 ca = *reinterpret_cast<const float2*>(cst + 4 * P + 8 * cz + 2 * q);
      const float2 cb = *reinterpret_cast<const float2*>(cst + 5 * P + 8 * cz + 2 * q);
#pragma unroll
      for (int u = 0; u < ZU; ++u) {
        const uint32_t dw = q == 0 ? dyv[u].x : q == 1 ? dyv[u].y : q == 2 ? dyv[u].z : dyv[u].w;
        const uint32_t zw = q == 0 ? zv[u].x : q == 1 ? zv[u].y : q == 2 ? zv[u].z : zv[u].w;
        const float d0 = __uint_as_float(dw << 16), d1 = __uint_as_float(dw & 0xffff0000u);
        const float z0 = __uint_as_float(zw << 16), z1 = __uint_as_float(zw & 0xffff0000u);
        const float o0 =
            bn_bwd_elem(bn_relu_keep(d0, z0, sc.x, bi.x), z0, mu.x, is.x, sc.x, ca.x, cb.x);
        const float o1 =
            bn_bwd_elem(bn_relu_keep(d1, z1, sc.y, bi.y), z1, mu.y, is.y, sc.y, ca.y, cb.y);
        o4[u][q] = pk_bf16(o0, o1);
      }
    }
#pragma unroll
    for (int u = 0; u < ZU; ++u) {
      const int row = zr + (kNT / CA) * u;
      const bool live = t * kTP + row < M;
      const uint4 v = keep_if(live, make_uint4(o4[u][0], o4[u][1], o4[u][2], o4[u][3]));
      *reinterpret_cast<uint4*>(zimg + img_off<ZROWB>(row, cz)) = v;
      if (a.dz != nullptr && live && slice == 0)
        *reinterpret_cast<uint4*>(a.dz + static_cast<int64_t>(t * kTP + row) * P + 8 * cz) = v;
    }
  };

  f32x16 accw[P / 32] = {};
  if (t_lo < t_hi) fetch(t_lo);
  for (int t = t_lo; t < t_hi; ++t) {
    stage(t);
    fetch(t + 1 < t_hi ? t + 1 : t);   // past the end: a valid tile, dropped
    __syncthreads();
    // dW1 += dz1^T x over the tile's 64 pixels
#pragma unroll
    for (int ks = 0; ks < kTP / 16; ++ks) {
      const bf16x8_t B = frag32<XROWB>(ximg, 4 * cw, ks, lane);
#pragma unroll
      for (int i = 0; i < P / 32; ++i)
        accw[i] = mfma(frag32<ZROWB>(zimg, 4 * i, ks, lane), B, accw[i]);
    }
    // dx^T = W1^T dz1^T per 32 pixels: row = channel 32 cw + .., column = pixel 32 ph + r;
    // ascending k
#pragma unroll
    for (int ph = 0; ph < kTP / 32; ++ph) {
      f32x16 accx = {};
#pragma unroll
      for (int ks = 0; ks < P / 16; ++ks) {
        const bf16x8_t B = *reinterpret_cast<const bf16x8_t*>(
            zimg + img_off<ZROWB>(32 * ph + r, 2 * ks + h));
        accx = mfma(wf[ks], B, accx);
      }
      // registers 4 g .. 4 g + 3 = channels 8 g + 4 h .. + 3 of the wave's 32: half h of chunk g
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<uint2*>(oimg + img_off<XROWB>(32 * ph + r, 4 * cw + g) + 8 * h) =
            make_uint2(pk_bf16(accx[4 * g], accx[4 * g + 1]),
                       pk_bf16(accx[4 * g + 2], accx[4 * g + 3]));
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < XU; ++j) {
      const int row = xr + (kNT / 32) * j;
      uint4 v = *reinterpret_cast<const uint4*>(oimg + img_off<XROWB>(row, cx));
      if constexpr (LK != LK_NONE) v = add_link8(v, gc[j], gcb[j]);
      const int p = t * kTP + row;
      if (p < M)
        *reinterpret_cast<uint4*>(a.dx + static_cast<int64_t>(p) * Cin + cin0 + 8 * cx) = v;
    }
    // the next stage writes zimg / ximg (every wave is past its reads: second barrier) and the
    // next tile's oimg writes come after the next first barrier
  }
  // lane r = column (channel of Cin), register k = row (k & 3) + 8 (k >> 2) + 4 h of each block
  float* pw = a.part + static_cast<int64_t>(range) * P * Cin + cin0 + 32 * cw + r;
#pragma unroll
  for (int i = 0; i < P / 32; ++i)
#pragma unroll
    for (int k = 0; k < 16; ++k)
      pw[static_cast<int64_t>(32 * i + (k & 3) + 8 * (k >> 2) + 4 * h) * Cin] = accw[i][k];
}

template <int P, int LK>
hipError_t launch_k(const C1BArgs& a, int S, hipStream_t st) {
  constexpr int LDS = 2 * kTP * 2 * kSL + kTP * 2 * P + 6 * P * 4;   // 72 / 82 KiB: one per CU
  const hipError_t e =
      hipFuncSetAttribute(reinterpret_cast<const void*>(&conv1_bwd_kernel<P, LK>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, LDS);   // per device
  if (e != hipSuccess) return e;
  conv1_bwd_kernel<P, LK><<<S * a.slices, kNT, LDS, st>>>(a);
  return hipGetLastError();
}

template <int P>
hipError_t launch_p(const C1BArgs& a, int kind, int S, hipStream_t st) {
  if (kind == LK_MASK) return launch_k<P, LK_MASK>(a, S, st);
  if (kind == LK_S2) return launch_k<P, LK_S2>(a, S, st);
  return launch_k<P, LK_NONE>(a, S, st);
}

}  // namespace

bool conv1_bwd_plan(int64_t M, int p, int Cin, int* splits, int want) {
  if ((p != 64 && p != 128) || (Cin != 256 && Cin != 512)) return false;
  if (M < 1 || M >= (1ll << 31) - 2 * kTP || want < 0 || want > 4096) return false;
  const int slices = Cin / kSL;
  const int ntile = static_cast<int>((M + kTP - 1) / kTP);
  // one workgroup per CU; `want` (tests): that many pixel ranges, empty ones included
  int S = want ? want : 256 / slices;
  const int tpw = (ntile + S - 1) / S;
  if (!want) S = (ntile + tpw - 1) / tpw;
  if (slices == 2) S = (S + 7) / 8 * 8;   // whole groups of 8 ranges x 2 slices
  *splits = S;
  return true;
}

hipError_t launch_conv1_bwd(const void* dy, const void* z, const void* gamma, const void* beta,
                            const float* mean, const float* invstd, const float* sdz,
                            const float* sdzx, const void* x, const void* w, const void* link,
                            const uint8_t* lmask, int link_kind, int Nimg, int H, int W, void* dx,
                            float* part, int splits, void* dw, bool dw_bf16, void* dz_out,
                            int64_t M, int p, int Cin, hipStream_t st) {
  int S;
  if (!conv1_bwd_plan(M, p, Cin, &S, 0) || splits < 1 || splits > 4096)
    return hipErrorInvalidValue;
  const int slices = Cin / kSL;
  if (slices == 2 && splits % 8) return hipErrorInvalidValue;
  if (!dy || !z || !gamma || !beta || !mean || !invstd || !sdz || !sdzx || !x || !w || !dx ||
      !part || !dw)
    return hipErrorInvalidValue;
  if (link_kind < LK_NONE || link_kind > LK_S2 || (link_kind != LK_NONE && !link) ||
      (link_kind == LK_MASK) != (lmask != nullptr))
    return hipErrorInvalidValue;
  if (link_kind == LK_S2 && (Nimg < 1 || H < 1 || W < 1 || static_cast<int64_t>(Nimg) * H * W != M))
    return hipErrorInvalidValue;
  for (const void* q : {dy, z, x, link, static_cast<const void*>(dx),
                        static_cast<const void*>(dz_out)})
    if (reinterpret_cast<uintptr_t>(q) % 16) return hipErrorInvalidValue;
  C1BArgs a{};
  a.dy = reinterpret_cast<const uint16_t*>(dy);
  a.z = reinterpret_cast<const uint16_t*>(z);
  a.x = reinterpret_cast<const uint16_t*>(x);
  a.w = reinterpret_cast<const uint16_t*>(w);
  a.g = reinterpret_cast<const uint16_t*>(link);
  a.gm = lmask;
  a.gamma = reinterpret_cast<const uint16_t*>(gamma);
  a.beta = reinterpret_cast<const uint16_t*>(beta);
  a.mean = mean;
  a.invstd = invstd;
  a.sdz = sdz;
  a.sdzx = sdzx;
  a.dx = reinterpret_cast<uint16_t*>(dx);
  a.dz = reinterpret_cast<uint16_t*>(dz_out);
  a.part = part;
  a.M = static_cast<int>(M);
  a.Cin = Cin;
  a.slices = slices;
  const int ntile = static_cast<int>((M + kTP - 1) / kTP);
  a.tpw = (ntile + splits - 1) / splits;
  if (link_kind == LK_S2) {
    a.W = W;
    a.HW = H * W;
    a.OW = (W + 1) / 2;
    a.OHW = ((H + 1) / 2) * a.OW;
  }
  const hipError_t e =
      p == 64 ? launch_p<64>(a, link_kind, splits, st) : launch_p<128>(a, link_kind, splits, st);
  if (e != hipSuccess) return e;
  return launch_wgrad_fold(part, splits, static_cast<int64_t>(p) * Cin, dw, dw_bf16, st);
}

}  // namespace cml
