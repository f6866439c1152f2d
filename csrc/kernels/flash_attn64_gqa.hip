// Flash attention for head dim 64 with grouped-query heads and head-major operands (the small
// Llamas: Llama-3.2-1B 32 q / 8 kv heads, TinyLlama 32 / 4, Qwen2-0.5B 14 / 2), causal and full,
// any S >= 1, any grp = H / KV >= 1 (grp = 1 is head-major MHA), forward and backward on
// v_mfma_f32_32x32x16_bf16, gfx950 / CDNA4.
//
// Layouts (rope_fwd's output on one side, the output projection's input rows on the other):
//   q [B, H, S, 64], k / v [B, KV, S, 64]     head-major bf16; query head h reads kv head h / grp
//   o, do [B, S, H * 64]
//   lse, dsum [B, H, S] fp32                  log2 domain / D = rowsum(dO * O), as flash_attn64.hip
//   dq [B, H, S, 64]; dk / dv [B, KV, S, 64]  dk / dv ALREADY summed over the group's query heads
//
// The MFMA scheme, the 128-row 16 KB images with the sw64 swizzle on the LDS-DMA source chunk, the
// one-barrier two-buffer staging, the log2-domain online softmax with the deferred rescale and the
// row store are flash_attn64.hip's: this file includes it under CML_F64_GQA_TU, which leaves out
// its launchers, and uses its helpers (mfma, rowfrag, trfrag, acc_frag, stage, store_row,
// work_item). flash_attn64.hip's own kernels are compiled as before; none of them is
// instantiated here.
//
// Forward (g64_fwd_kernel) and dQ (g64_dq_kernel): 4 waves x 32 queries of ONE query head, the
// loops of f64_fwd_kernel<NQ = 1> / f64_dq_kernel without lengths and dropout. What changes is
// the addressing: a head's rows are contiguous 128-B rows, so a staged 128-row K or V tile is one
// contiguous 16 KB block of kv head h / grp (row stride 64 elements; rows past S clamp to S - 1
// of that head); Q rows come from q [B, H, S, 64], dQ goes there. Work order: work_item over
// B * H, so the ids of one XCD (id % 8) take a contiguous (batch, query head) range and the grp
// query heads of a kv head read its K / V through one L2 (when B * H % 8 == 0; otherwise the
// plain order, heads fastest); causal blocks heaviest first. D is computed in dQ's prologue and
// written to dsum. Only the one-query-group forward is built: the NQ = 1 / 2 rule of f64_nq was
// measured on the fused MHA layout at 12 heads and no measurement exists for this layout.
//
// dK / dV (g64_dkdv_kernel) with the group sum inside: one workgroup owns 128 keys of one
// (batch, kv head), 4 waves x 32 keys, the lane's K and V rows in registers. It runs ONE flat loop
// over items (head of the group, query tile of that head): item it is head kvh grp + it / nt,
// tile it % nt, where nt is the number of 128-query tiles that see the block's keys (causal: from
// the key block's first row). Each item's Q / dO images and its lse / D are staged by LDS-DMA
// into buffer it & 1, and the DMA of item it + 1 is issued after the barrier of item it whether
// or not it belongs to the next head: the pipeline never drains at a head change and every wave
// runs exactly grp nt barriers. The dK^T / dV^T fp32 accumulators live across the whole loop and
// are stored once. So dk / dv are written exactly once, already group-summed, in a fixed order
// (heads ascending, tiles ascending within a head): no atomics, bitwise deterministic, and the
// per-query-head dk / dv tensor [B, H, S, 64] and its summing pass do not exist. Grid
// B * KV * ceil(S / 128), heaviest key blocks (the first) first, XCD-contiguous (batch, kv head).
//
// LDS / occupancy: forward and dQ 2 x (K image + V image) = 64 KB; dK / dV 2 x (Q image + dO
// image + lse [128] + D [128]) = 66 KB; two workgroups (8 waves) per CU each.
// (dynamic LDS: the compiler reports 0 static bytes for all six).
// VGPRs (causal / full): forward 126 / 126; dQ 169 / 170; dK / dV 199 / 199; no VGPR or SGPR
// spill and 0 bytes of scratch in any of them (the compiler's kernel-resource-usage remarks with
// the scalar-fp32 flags of _build.py SRC_FLAGS).
//
// Not here: lengths, attention dropout and document bounds on this layout.
#define CML_F64_GQA_TU 1
#include "flash_attn64.hip"

namespace cml {

namespace {

struct G64Args {
  const uint16_t* q;      // [B, H, S, 64]
  const uint16_t* k;      // [B, KV, S, 64]
  const uint16_t* v;
  const uint16_t* o;      // [B, S, H, 64]
  const uint16_t* dout;   // [B, S, H, 64]
  uint16_t* out;          // forward: o; backward: dq [B, H, S, 64]
  uint16_t* dk;           // [B, KV, S, 64]
  uint16_t* dv;
  float* lse;             // [B, H, S]
  float* dsum;            // [B, H, S]
  int B, H, KV, S;
  float c;                // scale * log2(e)
  float scale;
  float thr;              // forward: deferred-rescale threshold (log2 units)
};

// ------------------------------------------------------------------------------------- forward
template <bool CAUSAL>
__global__ __launch_bounds__(kThreads, 2) void g64_fwd_kernel(G64Args a) {
  constexpr int BQ = 128;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 x (K image, V image)
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int S = a.S, H = a.H;
  int qb, bh;
  work_item((S + BQ - 1) / BQ, a.B * H, CAUSAL, qb, bh);
  const int b = bh / H, hh = bh - b * H, kvh = hh / (H / a.KV);
  const int64_t kvoff = (static_cast<int64_t>(b) * a.KV + kvh) * S * kD;
  const uint16_t* kg = a.k + kvoff;   // the kv head's rows: a 128-row tile is 16 KB contiguous
  const uint16_t* vg = a.v + kvoff;
  const int q0 = qb * BQ, qmin = q0 + 32 * w, qrow = qmin + r;
  const int kend = CAUSAL ? min(S, q0 + BQ) : S;
  const int nt = (kend + kBK - 1) / kBK;

  stage(kg, kD, 0, S, smem, w, lane);
  stage(vg, kD, 0, S, smem + kImg, w, lane);
  bf16x8_t qf[4];   // B operand of S^T = K Q^T: Q[qrow][16 ks + 8 h + j]
  {
    const uint16_t* qp = a.q + (static_cast<int64_t>(bh) * S + min(qrow, S - 1)) * kD + 8 * h;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const bf16x8_t*>(qp + 16 * ks);
  }
  f32x16 o[2] = {zero16(), zero16()};
  float m = -INFINITY, l = 0.f;
  for (int t = 0; t < nt; ++t) {
    const char* kimg = smem + (t & 1) * 2 * kImg;
    const char* vimg = kimg + kImg;
    // tile t landed (this wave's DMAs: a barrier does not wait for global_load_lds), then every
    // wave's; every wave is done with tile t - 1's buffer
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t + 1 < nt) {
      char* nb = smem + ((t + 1) & 1) * 2 * kImg;
      stage(kg, kD, (t + 1) * kBK, S, nb, w, lane);
      stage(vg, kD, (t + 1) * kBK, S, nb + kImg, w, lane);
    }
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const int k0 = t * kBK + 64 * hf;
      // no key of the half is visible to any query of the wave (never the first half: key 0 is)
      if (k0 >= S || (CAUSAL && k0 > qmin + 31)) continue;
      // S^T: s0 = keys k0 + 0..31, s1 = keys k0 + 32..63 (rows), query of the lane
      f32x16 s0 = zero16(), s1 = zero16();
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        s0 = mfma(rowfrag(kimg, 64 * hf + r, 2 * ks + h), qf[ks], s0);
        s1 = mfma(rowfrag(kimg, 64 * hf + 32 + r, 2 * ks + h), qf[ks], s1);
      }
      if (CAUSAL ? (k0 + 63 > qmin) : (k0 + 64 > S)) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int key = k0 + acc_row(i, h);
          if ((CAUSAL && key > qrow) || key >= S) s0[i] = -INFINITY;
          if ((CAUSAL && key + 32 > qrow) || key + 32 >= S) s1[i] = -INFINITY;
        }
      }
      float mt = -INFINITY;
#pragma unroll
      for (int i = 0; i < 16; ++i) mt = fmaxf(mt, fmaxf(s0[i], s1[i]));
      mt = fmaxf(mt, __shfl_xor(mt, 32, 64)) * a.c;
      // deferred rescale: the running max moves (and O, l are rescaled) only when some row's tile
      // max exceeds it by more than thr, so exponentiated scores stay <= 2^thr; the first half
      // always sets m (finite from then on: key 0 is visible to every query). A half that is
      // fully masked for these 32 queries has mt = -inf and changes nothing.
      if (__any(mt > m + a.thr)) {
        const float mn = fmaxf(m, mt);
        const float alpha = fexp2(m - mn);
        m = mn;
        l *= alpha;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
          for (int i = 0; i < 16; ++i) o[dt][i] *= alpha;
      }
      float ls = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        s0[i] = fexp2(fmaf(s0[i], a.c, -m));
        s1[i] = fexp2(fmaf(s1[i], a.c, -m));
        ls += s0[i] + s1[i];
      }
      l += ls;
      // O^T += V^T P^T over the 64 keys (4 k-steps of 16)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int ka = 64 * hf + 16 * u + 4 * h;
        const bf16x8_t p0 = acc_frag(s0, u), p1 = acc_frag(s1, u);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          o[dt] = mfma(trfrag(vimg, ka, ka + 8, 32 * dt, lane), p0, o[dt]);
          o[dt] = mfma(trfrag(vimg, 32 + ka, 40 + ka, 32 * dt, lane), p1, o[dt]);
        }
      }
    }
  }
  const float lt = l + __shfl_xor(l, 32, 64);
  uint16_t* orow = a.out + ((static_cast<int64_t>(b) * S + min(qrow, S - 1)) * H + hh) * kD;
  store_row(orow, o, 1.f / lt, h, qrow < S);
  if (h == 0 && qrow < S) a.lse[static_cast<int64_t>(bh) * S + qrow] = m + __log2f(lt);
}

// ------------------------------------------------------------------------------ backward: dQ
template <bool CAUSAL>
__global__ __launch_bounds__(kThreads, 2) void g64_dq_kernel(G64Args a) {
  constexpr int BQ = 128;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 x (K image, V image)
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int S = a.S, H = a.H;
  int qb, bh;
  work_item((S + BQ - 1) / BQ, a.B * H, CAUSAL, qb, bh);
  const int b = bh / H, hh = bh - b * H, kvh = hh / (H / a.KV);
  const int64_t kvoff = (static_cast<int64_t>(b) * a.KV + kvh) * S * kD;
  const uint16_t* kg = a.k + kvoff;
  const uint16_t* vg = a.v + kvoff;
  const int q0 = qb * BQ, qmin = q0 + 32 * w, qrow = qmin + r;
  const int qc = min(qrow, S - 1);   // the row whose Q, dO, O and lse the lane holds
  const int kend = CAUSAL ? min(S, q0 + BQ) : S;
  const int nt = (kend + kBK - 1) / kBK;

  stage(kg, kD, 0, S, smem, w, lane);
  stage(vg, kD, 0, S, smem + kImg, w, lane);
  bf16x8_t qf[4], df[4];
  float dsum;
  {
    const uint16_t* qp = a.q + (static_cast<int64_t>(bh) * S + qc) * kD + 8 * h;
    const int64_t orow = ((static_cast<int64_t>(b) * S + qc) * H + hh) * kD + 8 * h;
    const uint16_t* dp = a.dout + orow;
    const uint16_t* op = a.o + orow;
    float part = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      qf[ks] = *reinterpret_cast<const bf16x8_t*>(qp + 16 * ks);
      const uint4 dv = *reinterpret_cast<const uint4*>(dp + 16 * ks);
      const uint4 ov = *reinterpret_cast<const uint4*>(op + 16 * ks);
      df[ks] = __builtin_bit_cast(bf16x8_t, dv);
      const uint32_t d4[4] = {dv.x, dv.y, dv.z, dv.w}, o4[4] = {ov.x, ov.y, ov.z, ov.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        part = fmaf(__uint_as_float(d4[e] << 16), __uint_as_float(o4[e] << 16), part);
        part = fmaf(__uint_as_float(d4[e] & 0xffff0000u), __uint_as_float(o4[e] & 0xffff0000u), part);
      }
    }
    dsum = part + __shfl_xor(part, 32, 64);
    if (h == 0 && qrow < S) a.dsum[static_cast<int64_t>(bh) * S + qrow] = dsum;
  }
  const float lse = a.lse[static_cast<int64_t>(bh) * S + qc];
  f32x16 dq[2] = {zero16(), zero16()};
  for (int t = 0; t < nt; ++t) {
    const char* kimg = smem + (t & 1) * 2 * kImg;
    const char* vimg = kimg + kImg;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // tile t landed (see g64_fwd_kernel)
    __syncthreads();
    if (t + 1 < nt) {
      char* nb = smem + ((t + 1) & 1) * 2 * kImg;
      stage(kg, kD, (t + 1) * kBK, S, nb, w, lane);
      stage(vg, kD, (t + 1) * kBK, S, nb + kImg, w, lane);
    }
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const int k0 = t * kBK + 64 * hf;
      if (k0 >= S || (CAUSAL && k0 > qmin + 31)) continue;
      f32x16 s0 = zero16(), s1 = zero16(), p0 = zero16(), p1 = zero16();
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        s0 = mfma(rowfrag(kimg, 64 * hf + r, 2 * ks + h), qf[ks], s0);
        s1 = mfma(rowfrag(kimg, 64 * hf + 32 + r, 2 * ks + h), qf[ks], s1);
        p0 = mfma(rowfrag(vimg, 64 * hf + r, 2 * ks + h), df[ks], p0);
        p1 = mfma(rowfrag(vimg, 64 * hf + 32 + r, 2 * ks + h), df[ks], p1);
      }
      const bool edge = CAUSAL ? (k0 + 63 > qmin) : (k0 + 64 > S);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        float e0 = fexp2(fmaf(s0[i], a.c, -lse)), e1 = fexp2(fmaf(s1[i], a.c, -lse));
        if (edge) {
          const int key = k0 + acc_row(i, h);
          if ((CAUSAL && key > qrow) || key >= S) e0 = 0.f;
          if ((CAUSAL && key + 32 > qrow) || key + 32 >= S) e1 = 0.f;
        }
        s0[i] = e0 * (p0[i] - dsum);   // dS^T
        s1[i] = e1 * (p1[i] - dsum);
      }
      // dQ^T += K^T dS^T (K^T by transposed reads of the K rows)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const bf16x8_t d0 = acc_frag(s0, u), d1 = acc_frag(s1, u);
        const int ka = 64 * hf + 16 * u + 4 * h;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          dq[dt] = mfma(trfrag(kimg, ka, ka + 8, 32 * dt, lane), d0, dq[dt]);
          dq[dt] = mfma(trfrag(kimg, 32 + ka, 40 + ka, 32 * dt, lane), d1, dq[dt]);
        }
      }
    }
  }
  store_row(a.out + (static_cast<int64_t>(bh) * S + qc) * kD, dq, a.scale, h, qrow < S);
}

// --------------------------------------------------------------------------- backward: dK, dV
// 4 waves x 32 keys of one (batch, kv head); the lane's K and V rows in registers (B operands of
// S = Q K^T and dP = dO V^T); one flat loop over (query head of the group, query tile), the
// item's Q / dO images with their lse / D in LDS; dK^T / dV^T accumulate over the whole loop.
template <bool CAUSAL>
__global__ __launch_bounds__(kThreads, 2) void g64_dkdv_kernel(G64Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int S = a.S, H = a.H, KV = a.KV, grp = H / KV;
  int kb, bkv;
  work_item((S + kBK - 1) / kBK, a.B * KV, false, kb, bkv);
  const int b = bkv / KV, kvh = bkv - b * KV;
  const int h0 = b * H + kvh * grp;   // (batch, head) index of the group's first query head
  const int64_t ld_o = static_cast<int64_t>(H) * kD;
  const uint16_t* dob = a.dout + static_cast<int64_t>(b) * S * ld_o + kvh * grp * kD;
  const int kb0 = kb * kBK, kmin = kb0 + 32 * w, key = kmin + r;
  const int kc = min(key, S - 1);
  const int qstart = CAUSAL ? kb0 : 0;
  const int nt = (S - qstart + kBK - 1) / kBK;   // query tiles of one head (>= 1: kb0 < S)
  const int nit = grp * nt;

  // item (head g of the group, tile t) into buf: Q rows are the head's contiguous 128-B rows, dO
  // rows the head's 64 columns of the [S, H * 64] rows
  auto stage_all = [&](int g, int t, char* buf) {
    const int row0 = qstart + t * kBK;
    const int64_t hs = static_cast<int64_t>(h0 + g) * S;
    stage(a.q + hs * kD, kD, row0, S, buf, w, lane);
    stage(dob + g * kD, ld_o, row0, S, buf + kImg, w, lane);
    // lse (waves 0, 1) / D (waves 2, 3) of the tile's 128 queries: one 4-B DMA per lane
    const float* src = (w < 2 ? a.lse : a.dsum) + hs + min(row0 + 64 * (w & 1) + lane, S - 1);
    __builtin_amdgcn_global_load_lds((g_void*)src, (lds_void*)(buf + 2 * kImg + 256 * w), 4, 0, 0);
  };
  stage_all(0, 0, smem);
  bf16x8_t kf[4], vf[4];   // B operands K^T / V^T [d][key] = this lane's key rows
  {
    const int64_t off = (static_cast<int64_t>(bkv) * S + kc) * kD + 8 * h;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      kf[ks] = *reinterpret_cast<const bf16x8_t*>(a.k + off + 16 * ks);
      vf[ks] = *reinterpret_cast<const bf16x8_t*>(a.v + off + 16 * ks);
    }
  }
  f32x16 dk[2] = {zero16(), zero16()};
  f32x16 dv[2] = {zero16(), zero16()};
  int t = 0, gn = 0, tn = 0;   // tile of item it; (head, tile) of item it + 1
  for (int it = 0; it < nit; ++it) {
    const char* qimg = smem + (it & 1) * kKVBuf;
    const char* dimg = qimg + kImg;
    const float* lsel = reinterpret_cast<const float*>(qimg + 2 * kImg);
    const float* dsl = lsel + 128;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // item it landed (see g64_fwd_kernel)
    __syncthreads();
    // the next item, across a head change too: the other buffer was item it - 1's, which every
    // wave left before this barrier
    if (++tn == nt) {
      tn = 0;
      ++gn;
    }
    if (it + 1 < nit) stage_all(gn, tn, smem + ((it + 1) & 1) * kKVBuf);
    const int q0 = qstart + t * kBK;
    t = tn;
#pragma unroll 1
    for (int qs = 0; qs < 4; ++qs) {
      const int qq0 = q0 + 32 * qs;
      // no query of the sub-tile sees a key of the wave: past S, or (causal) all before them
      if (qq0 >= S || (CAUSAL && qq0 + 31 < kmin)) continue;
      f32x16 s = zero16(), dp = zero16();
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        s = mfma(rowfrag(qimg, 32 * qs + r, 2 * ks + h), kf[ks], s);
        dp = mfma(rowfrag(dimg, 32 * qs + r, 2 * ks + h), vf[ks], dp);
      }
      // s[i] = S[query qq0 + acc_row(i, h)][key]; registers 4g..4g+3: 4 consecutive queries
      const bool edge = (CAUSAL && qq0 < kmin + 31) || qq0 + 32 > S;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int ql = 32 * qs + 8 * g + 4 * h;
        const float4 Ls = *reinterpret_cast<const float4*>(lsel + ql);
        const float4 Dd = *reinterpret_cast<const float4*>(dsl + ql);
        const float Lv[4] = {Ls.x, Ls.y, Ls.z, Ls.w}, Dv[4] = {Dd.x, Dd.y, Dd.z, Dd.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = 4 * g + e;
          float p = fexp2(fmaf(s[i], a.c, -Lv[e]));
          if (edge) {
            const int qi = qq0 + 8 * g + 4 * h + e;
            if ((CAUSAL && qi < key) || qi >= S) p = 0.f;
          }
          s[i] = p;
          dp[i] = p * (dp[i] - Dv[e]);
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const bf16x8_t pb = acc_frag(s, u), sb = acc_frag(dp, u);
        const int ka = 32 * qs + 16 * u + 4 * h;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          dv[dt] = mfma(trfrag(dimg, ka, ka + 8, 32 * dt, lane), pb, dv[dt]);
          dk[dt] = mfma(trfrag(qimg, ka, ka + 8, 32 * dt, lane), sb, dk[dt]);
        }
      }
    }
  }
  const int64_t row = (static_cast<int64_t>(bkv) * S + kc) * kD;
  store_row(a.dk + row, dk, a.scale, h, key < S);
  store_row(a.dv + row, dv, 1.f, h, key < S);
}

// dynamic LDS at / above the default limit: set once per kernel (six instantiations here)
hipError_t launch_g64(void (*kern)(G64Args), const G64Args& a, int smem, int64_t nwg,
                      hipStream_t st) {
  static const void* done[6] = {};
  const void* f = reinterpret_cast<const void*>(kern);
  bool set = false;
  for (const void* d : done) set = set || d == f;
  if (!set) {
    hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    if (e != hipSuccess) return e;
    for (const void*& d : done)
      if (d == nullptr) {
        d = f;
        break;
      }
  }
  kern<<<dim3(static_cast<unsigned>(nwg)), kThreads, smem, st>>>(a);
  return hipGetLastError();
}

// blocks of 128 rows x (batch, query head): the largest grid of the three kernels
bool g64_shape_ok(int B, int H, int KV, int S) {
  return B >= 1 && KV >= 1 && H >= KV && H % KV == 0 && S >= 1 &&
         static_cast<int64_t>((S + kBK - 1) / kBK) * B * H < (1LL << 31);
}

}  // namespace

hipError_t launch_flash64_gqa_fwd(const void* q, const void* k, const void* v, void* o, float* lse,
                                  int B, int H, int KV, int S, float scale, bool causal,
                                  hipStream_t st, float rescale_thr) {
  if (!g64_shape_ok(B, H, KV, S)) return hipErrorInvalidValue;
  G64Args a{};
  a.q = static_cast<const uint16_t*>(q);
  a.k = static_cast<const uint16_t*>(k);
  a.v = static_cast<const uint16_t*>(v);
  a.out = static_cast<uint16_t*>(o);
  a.lse = lse;
  a.B = B; a.H = H; a.KV = KV; a.S = S;
  a.scale = scale;
  a.c = scale * 1.4426950408889634f;
  a.thr = rescale_thr < 0.f ? 0.f : rescale_thr;
  const int64_t nwg = static_cast<int64_t>((S + kBK - 1) / kBK) * B * H;
  return causal ? launch_g64(g64_fwd_kernel<true>, a, kFwdSmem, nwg, st)
                : launch_g64(g64_fwd_kernel<false>, a, kFwdSmem, nwg, st);
}

hipError_t launch_flash64_gqa_bwd(const void* q, const void* k, const void* v, const void* o,
                                  const void* dout, const float* lse, float* dsum, void* dq,
                                  void* dk, void* dv, int B, int H, int KV, int S, float scale,
                                  bool causal, hipStream_t st) {
  if (!g64_shape_ok(B, H, KV, S)) return hipErrorInvalidValue;
  G64Args a{};
  a.q = static_cast<const uint16_t*>(q);
  a.k = static_cast<const uint16_t*>(k);
  a.v = static_cast<const uint16_t*>(v);
  a.o = static_cast<const uint16_t*>(o);
  a.dout = static_cast<const uint16_t*>(dout);
  a.out = static_cast<uint16_t*>(dq);
  a.dk = static_cast<uint16_t*>(dk);
  a.dv = static_cast<uint16_t*>(dv);
  a.lse = const_cast<float*>(lse);
  a.dsum = dsum;
  a.B = B; a.H = H; a.KV = KV; a.S = S;
  a.scale = scale;
  a.c = scale * 1.4426950408889634f;
  const int64_t nblk = (S + kBK - 1) / kBK;
  // dQ first: it also writes D = rowsum(dO * O), which the dK / dV kernel reads
  hipError_t e = causal ? launch_g64(g64_dq_kernel<true>, a, kFwdSmem, nblk * B * H, st)
                        : launch_g64(g64_dq_kernel<false>, a, kFwdSmem, nblk * B * H, st);
  if (e != hipSuccess) return e;
  return causal ? launch_g64(g64_dkdv_kernel<true>, a, kKVSmem, nblk * B * KV, st)
                : launch_g64(g64_dkdv_kernel<false>, a, kKVSmem, nblk * B * KV, st);
}

}  // namespace cml
