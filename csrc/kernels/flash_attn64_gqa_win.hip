// Sliding-window causal flash attention for head dim 64 with grouped-query heads (Mistral / Qwen2
// local attention, Gemma's local layers) on flash_attn64_gqa.hip's head-major layouts: query i
// attends key j iff max(0, i - W + 1) <= j <= i, 1 <= W (W >= S is the plain causal mask; the
// binding sends that to flash_attn64_gqa.hip). Any S >= 1, any grp = H / KV >= 1, forward and
// backward on v_mfma_f32_32x32x16_bf16, gfx950 / CDNA4. The score work is O(S W), not O(S^2 / 2).
//
// Layouts: q [B, H, S, 64], k / v [B, KV, S, 64], o / do [B, S, H * 64], lse / dsum [B, H, S]
// fp32 (log2 domain / D = rowsum(dO * O)), dq [B, H, S, 64], dk / dv [B, KV, S, 64] already
// summed over the group. Helpers (mfma, rowfrag, trfrag, acc_frag, stage, store_row, work_item)
// are flash_attn64.hip's, included under CML_F64_GQA_TU, which instantiates nothing of that file.
//
// Forward (w64_fwd_kernel) and dQ (w64_dq_kernel): 4 waves x 32 queries of one query head, block
// [q0, q0 + 128). The key-tile loop runs from tile max(0, q0 - W + 1) / 128 to the diagonal tile
// q0 / 128: at most ceil((W - 1) / 128) + 1 tiles are staged, whatever S is; the first one goes
// into the buffer of its own parity, so tile t is always in buffer t & 1. A wave works in halves
// of 64 keys and looks at a half only when it can hold a visible (query, key) pair of ITS 32
// queries: not after the wave's last query, not wholly below the window of its first. The element
// mask (key > query, key < query - W + 1, key >= S) runs only on halves that hold a masked pair:
// those reaching past the wave's first query (diagonal) and those starting below the window of
// the wave's last query (lower edge; W % 64 != 0 makes that two halves). Every other half runs
// the unmasked instruction stream of the plain kernels. The first staged half can be wholly
// masked for a wave's later rows: their running max stays -inf and fin() keeps alpha and the
// exponentials NaN-free (alpha = exp2(-inf - 0) = 0 on O = l = 0, P = exp2(-inf) = 0); a finite
// max passes through fin() bit for bit. Key j = i is visible to every row, so l > 0 at the end.
// Deferred rescale as in the plain kernels. Blocks cost nearly the same (at most W + 127 keys),
// so they run in increasing order, XCD-contiguous (batch, head) ranges (work_item).
//
// dK / dV (w64_dkdv_kernel): a workgroup owns keys [k0, k0 + 128) of one (batch, kv head), 4 waves
// x 32 keys with the lane's K / V rows in registers, and runs the plain kernel's single flat
// double-buffered loop over items (query head of the group, query tile). Key j is seen by queries
// j <= i <= j + W - 1, so every head's tile range is k0 / 128 .. min(S - 1, k0 + 127 + W - 1) / 128:
// nt tiles, the same for each head of the group, and tiles past the window's upper edge are never
// staged. Item it is head it / nt, tile it % nt in buffer it & 1; the DMA of item it + 1 is
// issued after item it's barrier across head changes too, so the parity never resets. A wave
// skips 32-query sub-tiles wholly before its keys or wholly past their windows and masks only the
// sub-tiles on the diagonal or crossing i = j + W - 1. dk / dv accumulate in registers over the
// whole loop and are stored once: fixed order, no atomics, no per-query-head tensor.
//
// LDS: forward / dQ 2 x (K, V image) = 64 KB; dK / dV 2 x (Q, dO image + lse + D) = 66 KB
// (dynamic); two workgroups per CU. VGPRs: forward 144, dQ 176, dK / dV 190; no VGPR or SGPR spill
// and 0 bytes of scratch (kernel-resource-usage remarks with the scalar-fp32 flags of _build.py).
// Measured against the plain causal kernels and SDPA: profiles/flash64_window/README.md.
#define CML_F64_GQA_TU 1
#include "flash_attn64.hip"

namespace cml {

namespace {

struct W64Args {
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
  int W;                  // window: keys i - W + 1 .. i (1 <= W <= S)
  float c;                // scale * log2(e)
  float scale;
  float thr;              // forward: deferred-rescale threshold (log2 units)
};

// a running max that is still -inf (no visible key yet) counts as 0 inside an exp2 argument
__device__ __forceinline__ float fin(float m) { return m == -INFINITY ? 0.f : m; }

// ------------------------------------------------------------------------------------- forward
__global__ __launch_bounds__(kThreads, 2) void w64_fwd_kernel(W64Args a) {
  constexpr int BQ = 128;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 x (K image, V image)
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int S = a.S, H = a.H, W = a.W;
  int qb, bh;
  work_item((S + BQ - 1) / BQ, a.B * H, false, qb, bh);
  const int b = bh / H, hh = bh - b * H, kvh = hh / (H / a.KV);
  const int64_t kvoff = (static_cast<int64_t>(b) * a.KV + kvh) * S * kD;
  const uint16_t* kg = a.k + kvoff;
  const uint16_t* vg = a.v + kvoff;
  const int q0 = qb * BQ, qmin = q0 + 32 * w, qrow = qmin + r;
  const int t0 = max(q0 - W + 1, 0) / kBK;   // first tile with a key some query of the block sees
  const int nt = qb + 1;                     // ... through the diagonal tile
  const int wlo = qmin - W + 1;              // first key of the wave's first query (may be < 0)
  const int rlo = qrow - W + 1;              // first key of the lane's query

  stage(kg, kD, t0 * kBK, S, smem + (t0 & 1) * 2 * kImg, w, lane);
  stage(vg, kD, t0 * kBK, S, smem + (t0 & 1) * 2 * kImg + kImg, w, lane);
  bf16x8_t qf[4];   // B operand of S^T = K Q^T: Q[qrow][16 ks + 8 h + j]
  {
    const uint16_t* qp = a.q + (static_cast<int64_t>(bh) * S + min(qrow, S - 1)) * kD + 8 * h;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const bf16x8_t*>(qp + 16 * ks);
  }
  f32x16 o[2] = {zero16(), zero16()};
  float m = -INFINITY, l = 0.f;
  for (int t = t0; t < nt; ++t) {
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
      // no (query of the wave, key of the half) pair is visible: the half is past S, after the
      // wave's last query, or wholly below the window of its first
      if (k0 >= S || k0 > qmin + 31 || k0 + 63 < wlo) continue;
      // S^T: s0 = keys k0 + 0..31, s1 = keys k0 + 32..63 (rows), query of the lane
      f32x16 s0 = zero16(), s1 = zero16();
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        s0 = mfma(rowfrag(kimg, 64 * hf + r, 2 * ks + h), qf[ks], s0);
        s1 = mfma(rowfrag(kimg, 64 * hf + 32 + r, 2 * ks + h), qf[ks], s1);
      }
      // a masked pair: a key after the wave's first query (that covers keys >= S of live rows),
      // or a key below the window of the wave's last query
      if (k0 + 63 > qmin || k0 < wlo + 31) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int key = k0 + acc_row(i, h);
          if (key > qrow || key >= S || key < rlo) s0[i] = -INFINITY;
          if (key + 32 > qrow || key + 32 >= S || key + 32 < rlo) s1[i] = -INFINITY;
        }
      }
      float mt = -INFINITY;
#pragma unroll
      for (int i = 0; i < 16; ++i) mt = fmaxf(mt, fmaxf(s0[i], s1[i]));
      mt = fmaxf(mt, __shfl_xor(mt, 32, 64)) * a.c;
      // deferred rescale (see g64_fwd_kernel). A row whose window starts after this half has
      // mt = -inf and, until its first visible key, m = -inf: fin() keeps alpha (0 on O = l = 0)
      // and the exponentials (exp2(-inf) = 0) NaN-free; a finite max passes unchanged.
      if (__any(mt > m + a.thr)) {
        const float mn = fmaxf(m, mt);
        const float alpha = fexp2(m - fin(mn));
        m = mn;
        l *= alpha;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
          for (int i = 0; i < 16; ++i) o[dt][i] *= alpha;
      }
      const float ms = fin(m);
      float ls = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        s0[i] = fexp2(fmaf(s0[i], a.c, -ms));
        s1[i] = fexp2(fmaf(s1[i], a.c, -ms));
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
__global__ __launch_bounds__(kThreads, 2) void w64_dq_kernel(W64Args a) {
  constexpr int BQ = 128;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 x (K image, V image)
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int S = a.S, H = a.H, W = a.W;
  int qb, bh;
  work_item((S + BQ - 1) / BQ, a.B * H, false, qb, bh);
  const int b = bh / H, hh = bh - b * H, kvh = hh / (H / a.KV);
  const int64_t kvoff = (static_cast<int64_t>(b) * a.KV + kvh) * S * kD;
  const uint16_t* kg = a.k + kvoff;
  const uint16_t* vg = a.v + kvoff;
  const int q0 = qb * BQ, qmin = q0 + 32 * w, qrow = qmin + r;
  const int qc = min(qrow, S - 1);   // the row whose Q, dO, O and lse the lane holds
  const int t0 = max(q0 - W + 1, 0) / kBK, nt = qb + 1;   // as in w64_fwd_kernel
  const int wlo = qmin - W + 1, rlo = qrow - W + 1;

  stage(kg, kD, t0 * kBK, S, smem + (t0 & 1) * 2 * kImg, w, lane);
  stage(vg, kD, t0 * kBK, S, smem + (t0 & 1) * 2 * kImg + kImg, w, lane);
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
  for (int t = t0; t < nt; ++t) {
    const char* kimg = smem + (t & 1) * 2 * kImg;
    const char* vimg = kimg + kImg;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // tile t landed (see w64_fwd_kernel)
    __syncthreads();
    if (t + 1 < nt) {
      char* nb = smem + ((t + 1) & 1) * 2 * kImg;
      stage(kg, kD, (t + 1) * kBK, S, nb, w, lane);
      stage(vg, kD, (t + 1) * kBK, S, nb + kImg, w, lane);
    }
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const int k0 = t * kBK + 64 * hf;
      if (k0 >= S || k0 > qmin + 31 || k0 + 63 < wlo) continue;
      f32x16 s0 = zero16(), s1 = zero16(), p0 = zero16(), p1 = zero16();
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        s0 = mfma(rowfrag(kimg, 64 * hf + r, 2 * ks + h), qf[ks], s0);
        s1 = mfma(rowfrag(kimg, 64 * hf + 32 + r, 2 * ks + h), qf[ks], s1);
        p0 = mfma(rowfrag(vimg, 64 * hf + r, 2 * ks + h), df[ks], p0);
        p1 = mfma(rowfrag(vimg, 64 * hf + 32 + r, 2 * ks + h), df[ks], p1);
      }
      const bool edge = k0 + 63 > qmin || k0 < wlo + 31;   // diagonal / lower edge of the window
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        float e0 = fexp2(fmaf(s0[i], a.c, -lse)), e1 = fexp2(fmaf(s1[i], a.c, -lse));
        if (edge) {
          const int key = k0 + acc_row(i, h);
          if (key > qrow || key >= S || key < rlo) e0 = 0.f;
          if (key + 32 > qrow || key + 32 >= S || key + 32 < rlo) e1 = 0.f;
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
__global__ __launch_bounds__(kThreads, 2) void w64_dkdv_kernel(W64Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int S = a.S, H = a.H, KV = a.KV, grp = H / KV, W = a.W;
  int kb, bkv;
  work_item((S + kBK - 1) / kBK, a.B * KV, false, kb, bkv);
  const int b = bkv / KV, kvh = bkv - b * KV;
  const int h0 = b * H + kvh * grp;   // (batch, head) index of the group's first query head
  const int64_t ld_o = static_cast<int64_t>(H) * kD;
  const uint16_t* dob = a.dout + static_cast<int64_t>(b) * S * ld_o + kvh * grp * kD;
  const int kb0 = kb * kBK, kmin = kb0 + 32 * w, key = kmin + r;
  const int kc = min(key, S - 1);
  // query tiles kb .. (last query that sees the block's last key) / 128, for every head
  const int nt = min(S - 1, kb0 + kBK - 1 + W - 1) / kBK - kb + 1;
  const int nit = grp * nt;

  // item (head g of the group, tile t of the range) into buf
  auto stage_all = [&](int g, int t, char* buf) {
    const int row0 = kb0 + t * kBK;
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
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // item it landed (see w64_fwd_kernel)
    __syncthreads();
    // the next item, across a head change too (the next head starts again at the diagonal tile):
    // the other buffer was item it - 1's, which every wave left before this barrier
    if (++tn == nt) {
      tn = 0;
      ++gn;
    }
    if (it + 1 < nit) stage_all(gn, tn, smem + ((it + 1) & 1) * kKVBuf);
    const int q0 = kb0 + t * kBK;
    t = tn;
#pragma unroll 1
    for (int qs = 0; qs < 4; ++qs) {
      const int qq0 = q0 + 32 * qs;
      // no query of the sub-tile sees a key of the wave: past S, all before the keys, or all at
      // or past the window's end of the wave's last key (query i sees key j iff 0 <= i - j < W)
      if (qq0 >= S || qq0 + 31 < kmin || qq0 - (kmin + 31) >= W) continue;
      f32x16 s = zero16(), dp = zero16();
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        s = mfma(rowfrag(qimg, 32 * qs + r, 2 * ks + h), kf[ks], s);
        dp = mfma(rowfrag(dimg, 32 * qs + r, 2 * ks + h), vf[ks], dp);
      }
      // s[i] = S[query qq0 + acc_row(i, h)][key]; registers 4g..4g+3: 4 consecutive queries.
      // A masked pair: a query before the wave's last key, past S, or past the window of the
      // wave's first key
      const bool edge = qq0 < kmin + 31 || qq0 + 32 > S || qq0 + 31 - kmin >= W;
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
            if (qi < key || qi >= S || qi - key >= W) p = 0.f;
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

// dynamic LDS at / above the default limit: set once per kernel (three here)
hipError_t launch_w64(void (*kern)(W64Args), const W64Args& a, int smem, int64_t nwg,
                      hipStream_t st) {
  static const void* done[3] = {};
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

// S <= 2^30 keeps every row + window sum inside int; the grid as in flash_attn64_gqa.hip
bool w64_shape_ok(int B, int H, int KV, int S, int window) {
  return B >= 1 && KV >= 1 && H >= KV && H % KV == 0 && S >= 1 && S <= (1 << 30) && window >= 1 &&
         static_cast<int64_t>((S + kBK - 1) / kBK) * B * H < (1LL << 31);
}

}  // namespace

hipError_t launch_flash64_gqa_win_fwd(const void* q, const void* k, const void* v, void* o,
                                      float* lse, int B, int H, int KV, int S, int window,
                                      float scale, hipStream_t st, float rescale_thr) {
  if (!w64_shape_ok(B, H, KV, S, window)) return hipErrorInvalidValue;
  W64Args a{};
  a.q = static_cast<const uint16_t*>(q);
  a.k = static_cast<const uint16_t*>(k);
  a.v = static_cast<const uint16_t*>(v);
  a.out = static_cast<uint16_t*>(o);
  a.lse = lse;
  a.B = B; a.H = H; a.KV = KV; a.S = S;
  a.W = window < S ? window : S;
  a.scale = scale;
  a.c = scale * 1.4426950408889634f;
  a.thr = rescale_thr < 0.f ? 0.f : rescale_thr;
  const int64_t nwg = static_cast<int64_t>((S + kBK - 1) / kBK) * B * H;
  return launch_w64(w64_fwd_kernel, a, kFwdSmem, nwg, st);
}

hipError_t launch_flash64_gqa_win_bwd(const void* q, const void* k, const void* v, const void* o,
                                      const void* dout, const float* lse, float* dsum, void* dq,
                                      void* dk, void* dv, int B, int H, int KV, int S, int window,
                                      float scale, hipStream_t st) {
  if (!w64_shape_ok(B, H, KV, S, window)) return hipErrorInvalidValue;
  W64Args a{};
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
  a.W = window < S ? window : S;
  a.scale = scale;
  a.c = scale * 1.4426950408889634f;
  const int64_t nblk = (S + kBK - 1) / kBK;
  // dQ first: it also writes D = rowsum(dO * O), which the dK / dV kernel reads
  hipError_t e = launch_w64(w64_dq_kernel, a, kFwdSmem, nblk * B * H, st);
  if (e != hipSuccess) return e;
  return launch_w64(w64_dkdv_kernel, a, kKVSmem, nblk * B * KV, st);
}

}  // namespace cml
