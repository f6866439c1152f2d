// Flash attention for head dim 64 straight from the fused QKV projection (BERT-base / GPT-2-small
// shapes past the short kernel's S <= 128), MHA, full and causal, forward and backward on
// v_mfma_f32_32x32x16_bf16, gfx950 / CDNA4.
//
// Layouts (those of attention.hip, so no split / transpose / gather copies exist on either side):
//   qkv  [B, S, 3, H, 64]   row stride ld = 3 H 64; q / k / v of head h at column (j H + h) 64
//   o, do [B, S, H * 64]
//   lse  [B, H, S] fp32     log2 domain: m + log2(l) of the scores times scale * log2(e)
//   dsum [B, H, S] fp32     D = rowsum(dO * O), written by the dQ kernel
//   dqkv [B, S, 3, H, 64]   q section by the dQ kernel, k / v sections by the dK / dV kernel: every
//                           element written exactly once (no zero-fill, no atomics, no group sum)
//
// MFMA 32x32x16 bf16: lane l (r = l & 31, h = l >> 5) holds A[r][8h + j], B[8h + j][r]
// (j = 0..7) and C[(i & 3) + 8 (i >> 2) + 4h][r] (i = 0..15). As in flash_attn.hip every product
// sums over the previous accumulator's ROW index, so accumulators are fed back as B operands with
// no lane movement and the other operand comes from ds_read_b64_tr_b16 on the row images.
//
// What head dim 64 changes against flash_attn.hip:
//   * rows are 128 B: a 16 KB image holds 128 rows. A staged tile is 128 keys (forward, dQ) or 128
//     queries (dK / dV), consumed as two / four independent sub-tiles between ONE pair of barriers
//     (half the barriers per key of the hd-128 kernel)
//   * 4 k-steps per S^T tile, 2 output accumulators per 32 queries: Q is 16 VGPRs, O 32
//   * the swizzle is attention.hip's sw64 (chunk c of row r at 16 (c ^ f((r >> 1) & 7))): LDS-DMA
//     writes lane-linear (8 rows x 128 B per wave instruction), so f goes on each lane's SOURCE
//     chunk; a row's 8 chunks stay inside its one 128-B line, so the global side stays coalesced
//   * dK / dV: the lane's K AND V rows sit in registers (16 VGPRs each), so there is no resident V
//     image: 66 KB of LDS and two workgroups per CU instead of 130 KB and one
//
// Forward (f64_fwd_kernel<CAUSAL, NQ>): 4 waves, a wave owns NQ x 32 queries.
//   S^T = K Q^T, online softmax in the log2 domain with the deferred rescale (threshold = launch
//   argument), O^T += V^T P^T. NQ = 2: every K row fragment and every V^T fragment read from LDS
//   feeds two MFMAs, 256 queries per staged tile (248-250 VGPRs). NQ = 1: 128 queries per
//   workgroup, twice the workgroups (139 VGPRs). Neither wins everywhere: NQ = 1 at BERT's
//   8192-token steps (0.0226 vs 0.0266 ms at 16 x 12 x 512), NQ = 2 once the grid fills the chip
//   several times over (0.076 vs 0.090 ms at 64 x 12 x 512); f64_nq() picks per launch.
// dQ (f64_dq_kernel): 4 waves x 32 queries; D in the prologue; dS^T = P^T (dP^T - D),
//   dQ^T += K^T dS^T. Q, dO fragments (32 VGPRs) + 4 score tiles (64) + dQ (32): a 64-query wave
//   would need ~290 VGPRs and lose the second workgroup per CU, so it was not built.
// dK / dV (f64_dkdv_kernel): 4 waves x 32 keys, Q / dO tiles of 128 queries + their lse / D staged.
// LDS / occupancy: forward and dQ 2 x (K image + V image) = 64 KB; dK / dV 2 x (Q image + dO image
//   + lse [128] + D [128]) = 66 KB; two workgroups (8 waves) per CU each.
// Staging: 16-B global_load_lds from the fused rows into two buffers, one barrier per tile, the DMA
// of tile t + 1 issued after the barrier of tile t. Work order: XCD-contiguous (batch, head)
// ranges, heaviest causal blocks first; causal sub-tiles fully masked for a wave are skipped
// wave-uniformly (barrier count uniform).
//
// Lengths (the VL instantiations, launched when `lens` is given; the others are the same code with
// L = S folded in: same registers, same bits). Sequence b is rows [0, L), L = lens[b] clamped into
// [1, S] by a scalar load per workgroup; the row stride of every tensor stays S.
//   * no padded row is ever read: every row clamp -- the staging DMA, the lse / D DMA, the
//     register loads of Q, dO, O, K, V rows -- is to L - 1, not S - 1. A masked key has p = 0, but
//     0 * NaN inside the P V or dO^T P MFMA is NaN, so masking the scores alone is not enough
//   * loop bounds come from L: kend / nt (forward, dQ) and the query-tile count (dK / dV), so tiles
//     wholly past L are never staged and the t + 1 < nt prefetch follows; the sub-tile skips and
//     the edge masks compare against L. Causal forward / dQ fold both masks into one bound per
//     row, the last visible key min(row, L - 1) (this is what keeps <causal, 2, VL> at 246 VGPRs;
//     with two compares per score it spilled 39)
//   * a block wholly past L (query block in forward / dQ, key block in dK / dV) stores its zeros
//     (and lse = 0 / D = 0) and returns before the first DMA and barrier: the whole workgroup
//     takes the exit. In a partial block a wave wholly past L runs the barriers and its share of
//     the staging but no MFMA: its visible-row bound (kvis / qvis) is 0, which the existing
//     wave-uniform skip then tests (as a separate flag in the skip the full NQ = 2 form spilled
//     34 VGPRs; as a bound it is 252, no scratch). Padded rows of a partial block are stored as
//     +0 bits by store_row (lse, D: 0.f), so dqkv is still written exactly once by the kernels
//   * the forward's first half-tile still sets the running max: L >= 1, so key 0 is visible to
//     every query of a wave that computes at all
//   * grid, f64_nq and work_item are those of S: the launch needs no host knowledge of lens. Dead
//     blocks keep their place in the order (a different order was not tried)
// VGPRs with lengths: forward 141 / 140 (NQ 1 causal / full), 246 / 252 (NQ 2), dQ 176 / 174,
// dK / dV 207 / 207; no scratch, LDS as above, two workgroups per CU.
//
// Dropout (template flag DROP, instantiated only by flash_attn64_drop.hip, which includes this file
// under CML_F64_DROP_TU; the DROP = false instruction streams are those of the file without the
// flag). The arithmetic is attention.hip's: lse, the running max and l come from the undropped
// scores; with M = keep / (1 - p_eff), O = (M P) V (1 / (1 - p_eff) folded into the final 1 / l),
// dV = (M P)^T dO (folded into the store scale), dS = P (M dP - D) with D = rowsum(dO * O). That
// D is taken from o32, the fp32 row the DROP forward stores beside the bf16 one (4 B per element
// more written, and read once by dQ's prologue): O now carries 1 / (1 - p_eff), so for a query
// with one visible key M dP - D = 0 cancels only as far as O is exact, and with the bf16 O the
// remainder (2^-9 of |dO| |O|) was 2.6 times the 1e-3 floor of that sequence's whole gradient.
// Keep bits: dropout.h's mask over ((b H + h) S + q) S + k, S % 8 == 0, regenerated in
// every kernel at one Philox call per 8 scores, after the sub-tile skips (a skipped sub-tile draws
// nothing), applied in the loop that forms the probabilities; no keep image in HBM, no barrier
// added. Forward / dQ: drop_keep64 (registers + one permlane32_swap). dK / dV: drop_keep_patch
// (128 B of wave-private LDS per wave: 66.5 KB per workgroup, still two per CU). The forward is
// built for NQ = 1 only (NQ = 2 sits at 246-252 VGPRs without it).
// VGPRs with DROP (causal / full; plain, then lengths): forward 154 / 154, 153 / 152; dQ
// 220 / 219, 220 / 219; dK / dV 211 / 215, 209 / 213; no scratch, two workgroups per CU.
#include <math.h>

#include <type_traits>

#include "common.h"
#include "dropout.h"
#include "kernels.h"

namespace cml {

struct F64Args {
  const uint16_t* qkv;    // [B, S, 3, H, 64]
  const uint16_t* o;      // [B, S, H, 64]
  const uint16_t* dout;   // [B, S, H, 64]
  uint16_t* out;          // forward: o; backward: dqkv
  float* lse;             // [B, H, S]
  float* dsum;            // [B, H, S]
  int B, H, S;
  float c;                // scale * log2(e)
  float scale;
  float thr;              // forward: deferred-rescale threshold (log2 units)
  const int* lens;        // [B] rows of each sequence (VL kernels only; clamped into [1, S])
};
// the DROP instantiations (flash_attn64_drop.hip): S % 8 == 0, forward with one query group
hipError_t launch_f64_drop_fwd(const F64Args& a, const DropArgs& d, float* o32, bool causal,
                               hipStream_t st);
hipError_t launch_f64_drop_bwd(const F64Args& a, const DropArgs& d, const float* o32, bool causal,
                               hipStream_t st);

namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short v4i16 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4i16 lds_v4i16;
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) void g_void;

constexpr int kD = 64;                  // head dim
constexpr int kBK = 128;                // rows per staged tile
constexpr int kImg = kBK * 128;         // one [128][64] bf16 image: 16 KB
constexpr int kThreads = 256;
constexpr int kFwdSmem = 4 * kImg;              // 2 x (K, V)
constexpr int kKVBuf = 2 * kImg + 1024;         // Q image, dO image, lse [128], D [128]
constexpr int kKVSmem = 2 * kKVBuf;

// kernel argument: F64Args, for the DROP instantiations with the dropout.h arguments appended
struct F64DropArgs : F64Args {
  DropArgs drop;
  float* o32;   // [B, S, H, 64] fp32: the forward's output before its bf16 rounding, read for D
};
template <bool DROP>
using F64A = std::conditional_t<DROP, F64DropArgs, F64Args>;

__device__ __forceinline__ f32x16 mfma(bf16x8_t a, bf16x8_t b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}
// accumulator row of register i for lane half h
__device__ __forceinline__ int acc_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }
__device__ __forceinline__ int swz_f(int row) {
  const int k = (row >> 1) & 7;
  return ((k & 1) << 2) | (k >> 1);
}
// byte offset of 16-B chunk ch / of element col of row `row` in a [rows][128 B] image
__device__ __forceinline__ int sw(int row, int ch) { return row * 128 + 16 * (ch ^ swz_f(row)); }
__device__ __forceinline__ int swe(int row, int col) { return sw(row, col >> 3) + 2 * (col & 7); }
__device__ __forceinline__ bf16x8_t rowfrag(const char* img, int row, int ch) {
  return *reinterpret_cast<const bf16x8_t*>(img + sw(row, ch));
}
__device__ __forceinline__ uint2 tr_rd(const char* p) {
  return __builtin_bit_cast(uint2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)(p)));
}
// transposed operand of an image X [rows = k][64 cols = m]: elements 0-3 = X[ka + q][m],
// 4-7 = X[kb + q][m] (q = 0..3), m = m0 + (lane & 31)
__device__ __forceinline__ bf16x8_t trfrag(const char* img, int ka, int kb, int m0, int lane) {
  const int q = (lane >> 2) & 3, col = m0 + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
  const uint2 lo = tr_rd(img + swe(ka + q, col)), hi = tr_rd(img + swe(kb + q, col));
  return __builtin_bit_cast(bf16x8_t, make_uint4(lo.x, lo.y, hi.x, hi.y));
}
// registers 8u..8u+7 of an accumulator as a bf16 operand fragment
__device__ __forceinline__ bf16x8_t acc_frag(const f32x16& x, int u) {
  const int o = 8 * u;
  return __builtin_bit_cast(bf16x8_t, make_uint4(pk_bf16(x[o], x[o + 1]), pk_bf16(x[o + 2], x[o + 3]),
                                                 pk_bf16(x[o + 4], x[o + 5]),
                                                 pk_bf16(x[o + 6], x[o + 7])));
}
__device__ __forceinline__ float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }

// One row of 64 outputs times sc as bf16: o[dt][4g..4g+3] = elements 32 dt + 8 g + 4 h + 0..3 of
// the lane's row (lanes r and r + 32 hold one row). permlane32_swap pairs groups g, g + 1 so each
// lane stores 16 contiguous bytes. Every lane must execute it: `ok` only gates the stores. `zero`
// (a padded row of a length-variant kernel; lanes r and r + 32 agree on it) stores +0 bits
// whatever the accumulators hold.
__device__ __forceinline__ void store_row(uint16_t* row, const f32x16 (&o)[2], float sc, int h,
                                          bool ok, bool zero = false) {
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g = 0; g < 4; g += 2) {
      uint32_t a0 = pk_bf16(o[dt][4 * g] * sc, o[dt][4 * g + 1] * sc);
      uint32_t a1 = pk_bf16(o[dt][4 * g + 2] * sc, o[dt][4 * g + 3] * sc);
      uint32_t b0 = pk_bf16(o[dt][4 * g + 4] * sc, o[dt][4 * g + 5] * sc);
      uint32_t b1 = pk_bf16(o[dt][4 * g + 6] * sc, o[dt][4 * g + 7] * sc);
      const auto x = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
      const auto y = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
      a0 = x[0]; b0 = x[1];
      a1 = y[0]; b1 = y[1];
      if (ok)
        *reinterpret_cast<uint4*>(row + 32 * dt + 8 * g + 8 * h) =
            zero ? make_uint4(0u, 0u, 0u, 0u) : make_uint4(a0, a1, b0, b1);
    }
}

// rows [row0, row0 + 128) of a [S][ld] bf16 tensor's 64 columns at g (rows past S clamped to
// S - 1; the length-variant kernels pass the sequence's length as S, so no padded row is ever
// read) into an image: 16 LDS-DMA wave-instructions of 8 rows x 128 B, wave w issues w, w + 4, ..
__device__ __forceinline__ void stage(const uint16_t* g, int64_t ld, int row0, int S, char* img,
                                      int w, int lane) {
#pragma unroll
  for (int s = 0; s < kBK / 8 / 4; ++s) {
    const int i = w + 4 * s;
    const int row = 8 * i + (lane >> 3);
    const int ch = (lane & 7) ^ swz_f(row);
    int gr = row0 + row;
    gr = gr < S ? gr : S - 1;
    __builtin_amdgcn_global_load_lds((g_void*)(g + gr * ld + 8 * ch), (lds_void*)(img + 1024 * i),
                                     16, 0, 0);
  }
}

// workgroup id -> (row block, batch * head): ids sharing an XCD (id % 8) take a contiguous head
// range; blocks in decreasing (heavy_last) or increasing order of causal work
__device__ __forceinline__ void work_item(int nblk, int BH, bool heavy_last, int& blk, int& bh) {
  const int id = blockIdx.x;
  int slot, hb;
  if ((BH & 7) == 0) {
    const int hp = BH >> 3;
    slot = (id >> 3) / hp;
    hb = (id & 7) * hp + (id >> 3) % hp;
  } else {
    slot = id / BH;
    hb = id % BH;
  }
  blk = heavy_last ? nblk - 1 - slot : slot;
  bh = hb;
}

// rows of sequence b: S, or (VL) lens[b] clamped into [1, S] -- workgroup-uniform, a scalar load
template <bool VL>
__device__ __forceinline__ int seq_len(const F64Args& a, int b) {
  if constexpr (VL) return min(max(a.lens[b], 1), a.S);
  return a.S;
}
// A block wholly past its sequence's length: +0 into the 64 columns at p of rows [row0, row0 +
// rows) below S (16 B per lane and pass, a row's 128 B contiguous) and 0.f into f[row0 ..] (lse
// or D; nullptr: none). The whole workgroup calls it and returns, before any DMA or barrier.
__device__ __forceinline__ void zero_block(uint16_t* p, int64_t ld, int row0, int rows, int S,
                                           float* f) {
  for (int i = threadIdx.x; i < 8 * rows; i += kThreads) {
    const int row = row0 + (i >> 3);
    if (row < S) *reinterpret_cast<uint4*>(p + row * ld + 8 * (i & 7)) = make_uint4(0u, 0u, 0u, 0u);
  }
  if (f != nullptr)
    for (int i = threadIdx.x; i < rows; i += kThreads)
      if (row0 + i < S) f[row0 + i] = 0.f;
}

// ---------------------------------------------------------------------------- dropout keep bits
// dropout.h group (8 consecutive keys of one query, S % 8 == 0) of query row `row` of head bh at
// key 0; the group of key k is this + (k >> 3)
__device__ __forceinline__ uint64_t drop_row(int bh, int S, int row) {
  return (static_cast<uint64_t>(bh) * S + row) * static_cast<uint32_t>(S >> 3);
}
// Forward / dQ: keep bits of the lane's query against the 64 keys [k0, k0 + 64) of a half-tile
// (g0 = drop_row + (k0 >> 3)). The lane's registers 4j..4j+3 of score tile x are keys
// k0 + 32 x + 8 j + 4 h + 0..3, so group (x, j) is that quad of lane r and of lane r + 32. The
// lane draws the four groups of x = h (byte j of its word = group j), then one permlane32_swap
// hands both lanes of a query both words: every group is drawn once, nothing goes through LDS.
// kw[x] bit 8 j + e = keep of register 4 j + e of tile x (already shifted to the lane's nibble).
__device__ __forceinline__ void drop_keep64(const DropArgs& d, uint64_t g0, int h,
                                            uint32_t (&kw)[2]) {
  uint32_t mine = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) mine |= drop_keep8(d, g0 + 4 * h + j) << (8 * j);
  const auto x = __builtin_amdgcn_permlane32_swap(mine, mine, false, false);
  kw[0] = x[0] >> (4 * h);   // the word of lanes 0-31: tile 0
  kw[1] = x[1] >> (4 * h);   // the word of lanes 32-63: tile 1
}
// dK / dV: keep bits of a 32-query x 32-key sub-tile (queries q0 + 0..31, key groups from kg8 =
// first key >> 3) as one 32-bit word per query (bit r = key r) in a wave-private 128-byte patch.
// 128 groups, two per lane: lane l draws key groups 2 (l & 1) + 0 / 1 of query l >> 1 and writes
// their 16 bits at byte 2 l, i.e. half (l & 1) of word l >> 1. The words of the four queries
// 8 g + 4 h + 0..3 (registers 4g..4g+3 of the lane) are then one ds_read_b128 at 32 g + 16 h.
// Wave-private: the wave's own LDS operations complete in order, so lgkmcnt(0) is the only wait.
__device__ __forceinline__ void drop_keep_patch(const DropArgs& d, uint64_t bh_base, int S, int q0,
                                                int kg8, int lane, char* patch) {
  const uint64_t g = bh_base + static_cast<uint64_t>(q0 + (lane >> 1)) * static_cast<uint32_t>(S >> 3) +
                     static_cast<uint32_t>(kg8 + 2 * (lane & 1));
  const uint32_t bits = drop_keep8(d, g) | (drop_keep8(d, g + 1) << 8);
  *reinterpret_cast<uint16_t*>(patch + 2 * lane) = static_cast<uint16_t>(bits);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// ------------------------------------------------------------------------------------- forward
template <bool CAUSAL, int NQ, bool VL, bool DROP = false>
__global__ __launch_bounds__(kThreads, 2) void f64_fwd_kernel(F64A<DROP> a) {
  static_assert(!DROP || NQ == 1, "the DROP forward is built for one query group per wave");
  constexpr int BQ = 128 * NQ;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 x (K image, V image)
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int S = a.S, H = a.H;
  int qb, bh;
  work_item((S + BQ - 1) / BQ, a.B * H, CAUSAL, qb, bh);
  const int b = bh / H, hh = bh - b * H;
  const int64_t ld = 3LL * H * kD;
  const uint16_t* base = a.qkv + static_cast<int64_t>(b) * S * ld;
  const uint16_t* kg = base + (H + hh) * kD;
  const uint16_t* vg = base + (2 * H + hh) * kD;
  const int q0 = qb * BQ, qmin = q0 + 32 * NQ * w;
  const int L = seq_len<VL>(a, b);   // keys and valid queries: rows [0, L)
  if (VL && q0 >= L) {
    zero_block(a.out + static_cast<int64_t>(b) * S * H * kD + hh * kD, static_cast<int64_t>(H) * kD,
               q0, BQ, S, a.lse + static_cast<int64_t>(bh) * S);
    return;
  }
  // keys visible to the wave: none for a partial block's wave of padded queries (no MFMA)
  const int kvis = VL && qmin >= L ? 0 : L;
  const int kend = CAUSAL ? min(L, q0 + BQ) : L;
  const int nt = (kend + kBK - 1) / kBK;

  stage(kg, ld, 0, L, smem, w, lane);
  stage(vg, ld, 0, L, smem + kImg, w, lane);
  bf16x8_t qf[NQ][4];   // B operand of S^T = K Q^T: Q[qrow][16 ks + 8 h + j]
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    const uint16_t* qp = base + min(qmin + 32 * n + r, L - 1) * ld + hh * kD + 8 * h;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[n][ks] = *reinterpret_cast<const bf16x8_t*>(qp + 16 * ks);
  }
  f32x16 o[NQ][2];
  float m[NQ], l[NQ];
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    o[n][0] = zero16();
    o[n][1] = zero16();
    m[n] = -INFINITY;
    l[n] = 0.f;
  }
  for (int t = 0; t < nt; ++t) {
    const char* kimg = smem + (t & 1) * 2 * kImg;
    const char* vimg = kimg + kImg;
    // tile t landed (this wave's DMAs: a barrier does not wait for global_load_lds), then every
    // wave's; every wave is done with tile t - 1's buffer
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t + 1 < nt) {
      char* nb = smem + ((t + 1) & 1) * 2 * kImg;
      stage(kg, ld, (t + 1) * kBK, L, nb, w, lane);
      stage(vg, ld, (t + 1) * kBK, L, nb + kImg, w, lane);
    }
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const int k0 = t * kBK + 64 * hf;
      // no key of the half is visible to any query of the wave (never the first half: key 0 is,
      // unless the whole wave is padding, kvis = 0)
      if (k0 >= kvis || (CAUSAL && k0 > qmin + 32 * NQ - 1)) continue;
      // S^T: s[n][0] = keys k0 + 0..31, s[n][1] = keys k0 + 32..63 (rows), query of the lane
      f32x16 s[NQ][2];
#pragma unroll
      for (int n = 0; n < NQ; ++n) s[n][0] = s[n][1] = zero16();
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const bf16x8_t ka = rowfrag(kimg, 64 * hf + r, 2 * ks + h);
        const bf16x8_t kb = rowfrag(kimg, 64 * hf + 32 + r, 2 * ks + h);
#pragma unroll
        for (int n = 0; n < NQ; ++n) {
          s[n][0] = mfma(ka, qf[n][ks], s[n][0]);
          s[n][1] = mfma(kb, qf[n][ks], s[n][1]);
        }
      }
#pragma unroll
      for (int n = 0; n < NQ; ++n) {
        // causal with lengths: the last visible key of a row is min(row, L - 1) -- one bound for
        // both masks; a padded query row sees keys [0, L) like row L - 1, whose Q it holds
        const int qlo = (CAUSAL && VL) ? min(qmin + 32 * n, L - 1) : qmin + 32 * n;
        const int qrow = (CAUSAL && VL) ? min(qmin + 32 * n + r, L - 1) : qmin + 32 * n + r;
        if (CAUSAL ? (k0 + 63 > qlo) : (k0 + 64 > L)) {
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int key = k0 + acc_row(i, h);
            constexpr bool kOne = CAUSAL && VL;   // qrow < L already
            if ((CAUSAL && key > qrow) || (!kOne && key >= L)) s[n][0][i] = -INFINITY;
            if ((CAUSAL && key + 32 > qrow) || (!kOne && key + 32 >= L)) s[n][1][i] = -INFINITY;
          }
        }
        float mt = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i) mt = fmaxf(mt, fmaxf(s[n][0][i], s[n][1][i]));
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64)) * a.c;
        // deferred rescale: the running max moves (and O, l are rescaled) only when some row's
        // tile max exceeds it by more than thr, so exponentiated scores stay <= 2^thr; the first
        // half always sets m (finite from then on: key 0 is visible to every query -- with
        // lengths too, since L >= 1 after the clamp and a wave that gets here has qmin < L). A
        // half that is fully masked for this 32-query group has mt = -inf and changes nothing.
        if (__any(mt > m[n] + a.thr)) {
          const float mn = fmaxf(m[n], mt);
          const float alpha = fexp2(m[n] - mn);
          m[n] = mn;
          l[n] *= alpha;
#pragma unroll
          for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int i = 0; i < 16; ++i) o[n][dt][i] *= alpha;
        }
        float ls = 0.f;
        uint32_t kw[2];
        if constexpr (DROP)
          drop_keep64(a.drop, drop_row(bh, S, qmin + 32 * n + r) + (k0 >> 3), h, kw);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          s[n][0][i] = fexp2(fmaf(s[n][0][i], a.c, -m[n]));
          s[n][1][i] = fexp2(fmaf(s[n][1][i], a.c, -m[n]));
          ls += s[n][0][i] + s[n][1][i];
          if constexpr (DROP) {   // l keeps the undropped sum; the P of the P V product is dropped
            const int bit = 8 * (i >> 2) + (i & 3);
            if (!((kw[0] >> bit) & 1u)) s[n][0][i] = 0.f;
            if (!((kw[1] >> bit) & 1u)) s[n][1][i] = 0.f;
          }
        }
        l[n] += ls;
      }
      // O^T += V^T P^T over the 64 keys (4 k-steps of 16); each V^T fragment feeds NQ MFMAs
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int ka = 64 * hf + 16 * u + 4 * h;
        bf16x8_t pf[NQ][2];
#pragma unroll
        for (int n = 0; n < NQ; ++n) {
          pf[n][0] = acc_frag(s[n][0], u);
          pf[n][1] = acc_frag(s[n][1], u);
        }
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          const bf16x8_t v0 = trfrag(vimg, ka, ka + 8, 32 * dt, lane);
          const bf16x8_t v1 = trfrag(vimg, 32 + ka, 40 + ka, 32 * dt, lane);
#pragma unroll
          for (int n = 0; n < NQ; ++n) {
            o[n][dt] = mfma(v0, pf[n][0], o[n][dt]);
            o[n][dt] = mfma(v1, pf[n][1], o[n][dt]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    const int qrow = qmin + 32 * n + r;
    const float lt = l[n] + __shfl_xor(l[n], 32, 64);
    // rows [L, S) of a partial block: +0 and lse = 0 (a dead wave's l is 0: its 1 / lt is never
    // stored)
    const bool pad = VL && qrow >= L;
    uint16_t* orow = a.out + ((static_cast<int64_t>(b) * S + min(qrow, S - 1)) * H + hh) * kD;
    float inv = 1.f / lt;
    if constexpr (DROP) inv *= a.drop.scale;   // kept probabilities / (1 - p_eff)
    store_row(orow, o[n], inv, h, qrow < S, pad);
    if constexpr (DROP) {
      // the unrounded row for the backward's D (registers 4g..4g+3: 16 B per lane, lanes r and
      // r + 32 adjacent); padded rows are never read back, so they are not written
      if (qrow < S && !pad) {
        float* r32 = a.o32 + ((static_cast<int64_t>(b) * S + qrow) * H + hh) * kD + 4 * h;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
          for (int g = 0; g < 4; ++g)
            *reinterpret_cast<float4*>(r32 + 32 * dt + 8 * g) =
                make_float4(o[n][dt][4 * g] * inv, o[n][dt][4 * g + 1] * inv,
                            o[n][dt][4 * g + 2] * inv, o[n][dt][4 * g + 3] * inv);
      }
    }
    if (h == 0 && qrow < S)
      a.lse[static_cast<int64_t>(bh) * S + qrow] = pad ? 0.f : m[n] + __log2f(lt);
  }
}

// ------------------------------------------------------------------------------ backward: dQ
template <bool CAUSAL, bool VL, bool DROP = false>
__global__ __launch_bounds__(kThreads, 2) void f64_dq_kernel(F64A<DROP> a) {
  constexpr int BQ = 128;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 x (K image, V image)
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int S = a.S, H = a.H;
  int qb, bh;
  work_item((S + BQ - 1) / BQ, a.B * H, CAUSAL, qb, bh);
  const int b = bh / H, hh = bh - b * H;
  const int64_t ld = 3LL * H * kD;
  const uint16_t* base = a.qkv + static_cast<int64_t>(b) * S * ld;
  const uint16_t* kg = base + (H + hh) * kD;
  const uint16_t* vg = base + (2 * H + hh) * kD;
  const int q0 = qb * BQ, qmin = q0 + 32 * w, qrow = qmin + r;
  const int L = seq_len<VL>(a, b);
  if (VL && q0 >= L) {
    zero_block(a.out + static_cast<int64_t>(b) * S * ld + hh * kD, ld, q0, BQ, S,
               a.dsum + static_cast<int64_t>(bh) * S);
    return;
  }
  const int kvis = VL && qmin >= L ? 0 : L;   // as in the forward
  const bool pad = VL && qrow >= L;
  const int qc = min(qrow, L - 1);   // the row whose Q, dO, O and lse the lane holds
  const int kend = CAUSAL ? min(L, q0 + BQ) : L;
  const int nt = (kend + kBK - 1) / kBK;

  stage(kg, ld, 0, L, smem, w, lane);
  stage(vg, ld, 0, L, smem + kImg, w, lane);
  bf16x8_t qf[4], df[4];
  float dsum;
  {
    const uint16_t* qp = base + qc * ld + hh * kD + 8 * h;
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
      if constexpr (DROP) {   // D from the fp32 row: see the header comment
        const float* o32 = a.o32 + orow + 16 * ks;
        const float4 oa = *reinterpret_cast<const float4*>(o32);
        const float4 ob = *reinterpret_cast<const float4*>(o32 + 4);
        const float of[8] = {oa.x, oa.y, oa.z, oa.w, ob.x, ob.y, ob.z, ob.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          part = fmaf(__uint_as_float(d4[e] << 16), of[2 * e], part);
          part = fmaf(__uint_as_float(d4[e] & 0xffff0000u), of[2 * e + 1], part);
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          part = fmaf(__uint_as_float(d4[e] << 16), __uint_as_float(o4[e] << 16), part);
          part = fmaf(__uint_as_float(d4[e] & 0xffff0000u), __uint_as_float(o4[e] & 0xffff0000u), part);
        }
      }
    }
    dsum = part + __shfl_xor(part, 32, 64);
    if (h == 0 && qrow < S) a.dsum[static_cast<int64_t>(bh) * S + qrow] = pad ? 0.f : dsum;
  }
  const float lse = a.lse[static_cast<int64_t>(bh) * S + qc];
  f32x16 dq[2] = {zero16(), zero16()};
  for (int t = 0; t < nt; ++t) {
    const char* kimg = smem + (t & 1) * 2 * kImg;
    const char* vimg = kimg + kImg;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // tile t landed (see f64_fwd_kernel)
    __syncthreads();
    if (t + 1 < nt) {
      char* nb = smem + ((t + 1) & 1) * 2 * kImg;
      stage(kg, ld, (t + 1) * kBK, L, nb, w, lane);
      stage(vg, ld, (t + 1) * kBK, L, nb + kImg, w, lane);
    }
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const int k0 = t * kBK + 64 * hf;
      if (k0 >= kvis || (CAUSAL && k0 > qmin + 31)) continue;
      f32x16 s0 = zero16(), s1 = zero16(), p0 = zero16(), p1 = zero16();
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        s0 = mfma(rowfrag(kimg, 64 * hf + r, 2 * ks + h), qf[ks], s0);
        s1 = mfma(rowfrag(kimg, 64 * hf + 32 + r, 2 * ks + h), qf[ks], s1);
        p0 = mfma(rowfrag(vimg, 64 * hf + r, 2 * ks + h), df[ks], p0);
        p1 = mfma(rowfrag(vimg, 64 * hf + 32 + r, 2 * ks + h), df[ks], p1);
      }
      // causal with lengths: one bound, the last visible key min(row, L - 1) = qc (see forward)
      constexpr bool kOne = CAUSAL && VL;
      const int qlast = kOne ? qc : qrow;
      const bool edge = CAUSAL ? (k0 + 63 > (kOne ? min(qmin, L - 1) : qmin)) : (k0 + 64 > L);
      uint32_t kw[2];
      if constexpr (DROP) drop_keep64(a.drop, drop_row(bh, S, qrow) + (k0 >> 3), h, kw);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        float e0 = fexp2(fmaf(s0[i], a.c, -lse)), e1 = fexp2(fmaf(s1[i], a.c, -lse));
        if (edge) {
          const int key = k0 + acc_row(i, h);
          if ((CAUSAL && key > qlast) || (!kOne && key >= L)) e0 = 0.f;
          if ((CAUSAL && key + 32 > qlast) || (!kOne && key + 32 >= L)) e1 = 0.f;
        }
        if constexpr (DROP) {   // dP <- M dP, M = keep / (1 - p_eff); e0 / e1 stay undropped
          const int bit = 8 * (i >> 2) + (i & 3);
          p0[i] = (kw[0] >> bit) & 1u ? p0[i] * a.drop.scale : 0.f;
          p1[i] = (kw[1] >> bit) & 1u ? p1[i] * a.drop.scale : 0.f;
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
  store_row(a.out + (static_cast<int64_t>(b) * S + min(qrow, S - 1)) * ld + hh * kD, dq, a.scale, h,
            qrow < S, pad);
}

// --------------------------------------------------------------------------- backward: dK, dV
// 4 waves x 32 keys; the lane's K and V rows in registers (B operands of S = Q K^T and
// dP = dO V^T), Q / dO tiles of 128 queries with their lse / D in LDS.
template <bool CAUSAL, bool VL, bool DROP = false>
__global__ __launch_bounds__(kThreads, 2) void f64_dkdv_kernel(F64A<DROP> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int S = a.S, H = a.H;
  int kb, bh;
  work_item((S + kBK - 1) / kBK, a.B * H, false, kb, bh);
  const int b = bh / H, hh = bh - b * H;
  const int64_t ld = 3LL * H * kD, ld_o = static_cast<int64_t>(H) * kD;
  const uint16_t* base = a.qkv + static_cast<int64_t>(b) * S * ld;
  const uint16_t* qg = base + hh * kD;
  const uint16_t* dog = a.dout + static_cast<int64_t>(b) * S * ld_o + hh * kD;
  const float* lseg = a.lse + static_cast<int64_t>(bh) * S;
  const float* dsg = a.dsum + static_cast<int64_t>(bh) * S;
  const int kb0 = kb * kBK, kmin = kb0 + 32 * w, key = kmin + r;
  const int L = seq_len<VL>(a, b);   // queries and valid keys: rows [0, L)
  if (VL && kb0 >= L) {
    uint16_t* z = a.out + static_cast<int64_t>(b) * S * ld + (H + hh) * kD;
    zero_block(z, ld, kb0, kBK, S, nullptr);
    zero_block(z + H * kD, ld, kb0, kBK, S, nullptr);
    return;
  }
  // queries that see a key of the wave: none for a partial block's wave of padded keys (no MFMA)
  const int qvis = VL && kmin >= L ? 0 : L;
  const bool pad = VL && key >= L;
  const int kc = min(key, L - 1);
  const int qstart = CAUSAL ? kb0 : 0;
  const int nt = (L - qstart + kBK - 1) / kBK;

  auto stage_all = [&](int t, char* buf) {
    const int row0 = qstart + t * kBK;
    stage(qg, ld, row0, L, buf, w, lane);
    stage(dog, ld_o, row0, L, buf + kImg, w, lane);
    // lse (waves 0, 1) / D (waves 2, 3) of the tile's 128 queries: one 4-B DMA per lane
    const float* src = (w < 2 ? lseg : dsg) + min(row0 + 64 * (w & 1) + lane, L - 1);
    __builtin_amdgcn_global_load_lds((g_void*)src, (lds_void*)(buf + 2 * kImg + 256 * w), 4, 0, 0);
  };
  stage_all(0, smem);
  bf16x8_t kf[4], vf[4];   // B operands K^T / V^T [d][key] = this lane's key rows
  {
    const uint16_t* kp = base + kc * ld + (H + hh) * kD + 8 * h;
    const uint16_t* vp = kp + H * kD;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      kf[ks] = *reinterpret_cast<const bf16x8_t*>(kp + 16 * ks);
      vf[ks] = *reinterpret_cast<const bf16x8_t*>(vp + 16 * ks);
    }
  }
  f32x16 dk[2] = {zero16(), zero16()};
  f32x16 dv[2] = {zero16(), zero16()};
  for (int t = 0; t < nt; ++t) {
    const char* qimg = smem + (t & 1) * kKVBuf;
    const char* dimg = qimg + kImg;
    const float* lsel = reinterpret_cast<const float*>(qimg + 2 * kImg);
    const float* dsl = lsel + 128;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // tile t landed (see f64_fwd_kernel)
    __syncthreads();
    if (t + 1 < nt) stage_all(t + 1, smem + ((t + 1) & 1) * kKVBuf);
    const int q0 = qstart + t * kBK;
#pragma unroll 1
    for (int qs = 0; qs < 4; ++qs) {
      const int qq0 = q0 + 32 * qs;
      // no query of the sub-tile sees a key of the wave: past S, or (causal) all before them
      if (qq0 >= qvis || (CAUSAL && qq0 + 31 < kmin)) continue;
      f32x16 s = zero16(), dp = zero16();
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        s = mfma(rowfrag(qimg, 32 * qs + r, 2 * ks + h), kf[ks], s);
        dp = mfma(rowfrag(dimg, 32 * qs + r, 2 * ks + h), vf[ks], dp);
      }
      // s[i] = S[query qq0 + acc_row(i, h)][key]; registers 4g..4g+3: 4 consecutive queries
      const bool edge = (CAUSAL && qq0 < kmin + 31) || qq0 + 32 > L;
      // the sub-tile's keep words (after the skip: a skipped sub-tile draws nothing); the patch
      // follows the two staging buffers, 128 B per wave
      char* patch = smem + kKVSmem + 128 * w;
      if constexpr (DROP)
        drop_keep_patch(a.drop, drop_row(bh, S, 0), S, qq0, kmin >> 3, lane, patch);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int ql = 32 * qs + 8 * g + 4 * h;
        const float4 Ls = *reinterpret_cast<const float4*>(lsel + ql);
        const float4 Dd = *reinterpret_cast<const float4*>(dsl + ql);
        const float Lv[4] = {Ls.x, Ls.y, Ls.z, Ls.w}, Dv[4] = {Dd.x, Dd.y, Dd.z, Dd.w};
        uint4 kq = {};
        if constexpr (DROP) kq = *reinterpret_cast<const uint4*>(patch + 32 * g + 16 * h);
        const uint32_t Kv[4] = {kq.x, kq.y, kq.z, kq.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = 4 * g + e;
          float p = fexp2(fmaf(s[i], a.c, -Lv[e]));
          if (edge) {
            const int qi = qq0 + 8 * g + 4 * h + e;
            if ((CAUSAL && qi < key) || qi >= L) p = 0.f;
          }
          if constexpr (DROP) {   // dV takes keep * P, dS = P (M dP - D) the undropped P
            const bool keep = (Kv[e] >> r) & 1u;
            s[i] = keep ? p : 0.f;
            dp[i] = p * ((keep ? dp[i] * a.drop.scale : 0.f) - Dv[e]);
          } else {
            s[i] = p;
            dp[i] = p * (dp[i] - Dv[e]);
          }
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
  uint16_t* row = a.out + (static_cast<int64_t>(b) * S + min(key, S - 1)) * ld + (H + hh) * kD;
  store_row(row, dk, a.scale, h, key < S, pad);
  float vs = 1.f;
  if constexpr (DROP) vs = a.drop.scale;   // dV = (keep P)^T dO / (1 - p_eff)
  store_row(row + H * kD, dv, vs, h, key < S, pad);
}

template <typename A>
hipError_t launch_f64(void (*kern)(A), const A& a, int smem, int rows, hipStream_t st) {
  // dynamic LDS at / above the default limit: set once per kernel. One slot per instantiation a
  // compilation launches (the table is per compilation and argument type). flash_attn64.hip:
  // forward {causal, full} x {NQ 1, 2}, dQ and dK / dV {causal, full}, each with and without
  // lengths (8 + 8). flash_attn64_drop.hip: the DROP forward (NQ 1), dQ and dK / dV in the same
  // four forms (4 + 4 + 4). A 17th would just set its attribute on every launch.
  static const void* done[16] = {};
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
  const int nblk = (a.S + rows - 1) / rows;
  const dim3 grid(static_cast<unsigned>(nblk * a.B * a.H));
  kern<<<grid, kThreads, smem, st>>>(a);
  return hipGetLastError();
}

#if !defined(CML_F64_DROP_TU) && !defined(CML_F64_GQA_TU)
// 32-query groups per forward wave: 2 when its grid still gives every CU >= 3 workgroups (causal:
// >= 4) and S wastes no half block of 256 queries, else 1. Measured at 12 heads (256 CUs,
// profiles/flash64/README.md): at 1.5-2 workgroups per CU NQ = 1 is 12-17 % faster; at 3 NQ = 2
// is 8-13 % faster (causal: 3 % slower); at 4.5-6 NQ = 2 is 7-15 % faster (causal at 4.5: level);
// S = 384 (a third of NQ = 2's query rows would be padding) stays 4-7 % slower at every size.
int f64_nq(int B, int H, int S, bool causal) {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      n = 256;
    return n;
  }();
  const int64_t nb2 = (S + 255) / 256;
  return nb2 * B * H >= (causal ? 4LL : 3LL) * cus && 2 * nb2 == (S + 127) / 128 ? 2 : 1;
}

bool f64_shape_ok(int B, int H, int S) {
  return B >= 1 && H >= 1 && S >= 1 &&
         static_cast<int64_t>((S + kBK - 1) / kBK) * B * H < (1LL << 31);
}

#endif  // !CML_F64_DROP_TU && !CML_F64_GQA_TU

}  // namespace

#if defined(CML_F64_GQA_TU)
// flash_attn64_gqa.hip takes the helpers above for its own kernels and launchers: nothing of this
// file is instantiated in that compilation
#elif defined(CML_F64_DROP_TU)
hipError_t launch_f64_drop_fwd(const F64Args& a, const DropArgs& d, float* o32, bool causal,
                               hipStream_t st) {
  const F64DropArgs x{a, d, o32};
  if (a.lens != nullptr)
    return causal ? launch_f64(f64_fwd_kernel<true, 1, true, true>, x, kFwdSmem, 128, st)
                  : launch_f64(f64_fwd_kernel<false, 1, true, true>, x, kFwdSmem, 128, st);
  return causal ? launch_f64(f64_fwd_kernel<true, 1, false, true>, x, kFwdSmem, 128, st)
                : launch_f64(f64_fwd_kernel<false, 1, false, true>, x, kFwdSmem, 128, st);
}

hipError_t launch_f64_drop_bwd(const F64Args& a, const DropArgs& d, const float* o32, bool causal,
                               hipStream_t st) {
  const F64DropArgs x{a, d, const_cast<float*>(o32)};
  constexpr int kv = kKVSmem + 4 * 128;   // + one keep-word patch per wave
  hipError_t e;
  if (a.lens != nullptr) {
    e = causal ? launch_f64(f64_dq_kernel<true, true, true>, x, kFwdSmem, 128, st)
               : launch_f64(f64_dq_kernel<false, true, true>, x, kFwdSmem, 128, st);
    if (e != hipSuccess) return e;
    return causal ? launch_f64(f64_dkdv_kernel<true, true, true>, x, kv, kBK, st)
                  : launch_f64(f64_dkdv_kernel<false, true, true>, x, kv, kBK, st);
  }
  e = causal ? launch_f64(f64_dq_kernel<true, false, true>, x, kFwdSmem, 128, st)
             : launch_f64(f64_dq_kernel<false, false, true>, x, kFwdSmem, 128, st);
  if (e != hipSuccess) return e;
  return causal ? launch_f64(f64_dkdv_kernel<true, false, true>, x, kv, kBK, st)
                : launch_f64(f64_dkdv_kernel<false, false, true>, x, kv, kBK, st);
}
#else
hipError_t launch_flash64_fwd(const void* qkv, void* o, float* lse, int B, int H, int S,
                              float scale, bool causal, hipStream_t st, float rescale_thr,
                              int nq, const int* lens, const DropSpec& drop, float* o32) {
  if (!f64_shape_ok(B, H, S) || nq < 0 || nq > 2) return hipErrorInvalidValue;
  // dropout: a Philox group is 8 keys of one query (S % 8 == 0); one query group per wave only
  if (drop.thr && (!drop_valid(drop) || S % 8 != 0 || nq == 2 || o32 == nullptr))
    return hipErrorInvalidValue;
  F64Args a{};
  a.qkv = static_cast<const uint16_t*>(qkv);
  a.out = static_cast<uint16_t*>(o);
  a.lse = lse;
  a.B = B; a.H = H; a.S = S;
  a.scale = scale;
  a.c = scale * 1.4426950408889634f;
  a.thr = rescale_thr < 0.f ? 0.f : rescale_thr;
  a.lens = lens;
  if (drop.thr) return launch_f64_drop_fwd(a, drop_args(drop), o32, causal, st);   // f64_nq not asked
  // the grid and the pick of NQ come from S with or without lengths: the host never reads lens
  const bool two = (nq ? nq : f64_nq(B, H, S, causal)) == 2;
  if (lens != nullptr) {
    if (two)
      return causal ? launch_f64(f64_fwd_kernel<true, 2, true>, a, kFwdSmem, 256, st)
                    : launch_f64(f64_fwd_kernel<false, 2, true>, a, kFwdSmem, 256, st);
    return causal ? launch_f64(f64_fwd_kernel<true, 1, true>, a, kFwdSmem, 128, st)
                  : launch_f64(f64_fwd_kernel<false, 1, true>, a, kFwdSmem, 128, st);
  }
  if (two)
    return causal ? launch_f64(f64_fwd_kernel<true, 2, false>, a, kFwdSmem, 256, st)
                  : launch_f64(f64_fwd_kernel<false, 2, false>, a, kFwdSmem, 256, st);
  return causal ? launch_f64(f64_fwd_kernel<true, 1, false>, a, kFwdSmem, 128, st)
                : launch_f64(f64_fwd_kernel<false, 1, false>, a, kFwdSmem, 128, st);
}

hipError_t launch_flash64_bwd(const void* qkv, const void* o, const void* dout, const float* lse,
                              float* dsum, void* dqkv, int B, int H, int S, float scale,
                              bool causal, hipStream_t st, const int* lens, const DropSpec& drop,
                              const float* o32) {
  if (!f64_shape_ok(B, H, S)) return hipErrorInvalidValue;
  if (drop.thr && (!drop_valid(drop) || S % 8 != 0 || o32 == nullptr)) return hipErrorInvalidValue;
  F64Args a{};
  a.qkv = static_cast<const uint16_t*>(qkv);
  a.o = static_cast<const uint16_t*>(o);
  a.dout = static_cast<const uint16_t*>(dout);
  a.out = static_cast<uint16_t*>(dqkv);
  a.lse = const_cast<float*>(lse);
  a.dsum = dsum;
  a.B = B; a.H = H; a.S = S;
  a.scale = scale;
  a.c = scale * 1.4426950408889634f;
  a.lens = lens;
  if (drop.thr) return launch_f64_drop_bwd(a, drop_args(drop), o32, causal, st);
  // dQ first: it also writes D = rowsum(dO * O), which the dK / dV kernel reads
  if (lens != nullptr) {
    hipError_t e = causal ? launch_f64(f64_dq_kernel<true, true>, a, kFwdSmem, 128, st)
                          : launch_f64(f64_dq_kernel<false, true>, a, kFwdSmem, 128, st);
    if (e != hipSuccess) return e;
    return causal ? launch_f64(f64_dkdv_kernel<true, true>, a, kKVSmem, kBK, st)
                  : launch_f64(f64_dkdv_kernel<false, true>, a, kKVSmem, kBK, st);
  }
  hipError_t e = causal ? launch_f64(f64_dq_kernel<true, false>, a, kFwdSmem, 128, st)
                        : launch_f64(f64_dq_kernel<false, false>, a, kFwdSmem, 128, st);
  if (e != hipSuccess) return e;
  return causal ? launch_f64(f64_dkdv_kernel<true, false>, a, kKVSmem, kBK, st)
                : launch_f64(f64_dkdv_kernel<false, false>, a, kKVSmem, kBK, st);
}
#endif  // CML_F64_GQA_TU / CML_F64_DROP_TU

}  // namespace cml
