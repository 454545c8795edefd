// Batched decode for the large-codebook VPTQ formats of VECTOR LENGTH 12, 17 - 48 TOKENS in one launch: TB = 2 / 3 blocks of 16 tokens
// over gemm_gather12c.hip's pass.  It is to gemm_gather12.hip / gemm_gather12c.hip what gemm_gatherxw.hip is to gemm_gatherx.hip - with
// BOTH axes of the v = 12 kernels in one kernel: token blocks, and the work split over (row group, column part).
//
// From the 17th token on a v = 12 layer went through vptq_dequant + a dense GEMM: a dense W rebuilt in HBM on every call.  The time of
// both v = 12 kernels hardly depends on the token count (profiles/r37, profiles/r38: gathers, the rebuild and the tile write bound
// them, not the MFMAs), so a further block of 16 tokens adds its A-operand loads and 12 MFMAs per wave and tile to a pass whose cost
// is elsewhere.
//  * WORK ITEM = (ROW GROUP of 4 vector-rows = 48 outputs, COLUMN PART of whole 512-column tiles): gemm_gather12c's walk - it =
//    blockIdx.x, += gridDim.x of n_groups x S; item it is row group it / S, part it % S; part p covers tiles [p tpp, min((p + 1) tpp,
//    n_tiles)).  S >= 1 (gemm_gather12w_decide).  The column split is here from the start because gemm_gather12 alone loses on the
//    4096-output layers of the one published v = 12 checkpoint: 86 row groups cannot fill 512 resident slots.
//  * THE ROW-GROUP BODY IS A COPY of gemm_gather12c.hip's, which is gemm_gather12.hip's (its head describes it: dequant role of 4
//    vector-rows x 64 chunks of 8 columns, the run-time index window, 24-byte entries gathered as 16 + 8 bytes, RES = none / table in LDS /
//    from L2, the reference's three roundings, the 48 KiB tile [N block][chunk][16 outputs][16 bytes] with the slot XOR-ed by chunk & 7,
//    the gathers of tile t + 1 in flight during the MFMAs of tile t, prefetches clamped to the part's last tile).  A copy for the
//    reason given there: as a shared function such bodies have twice cost 3 - 8 % and changed the parents' listings (profiles/r17,
//    profiles/r31).  A CHANGE TO THE BODY HERE BELONGS IN gemm_gather12.hip, gemm_gather12c.hip, gemm_gather12_grouped.hip AND gemm_gather12w_grouped.hip TOO, AND THE OTHER WAY ROUND.
//  * TOKEN BLOCKS.  Lane (token mj, k group mkg) of block b reads row 16 b + mj of x, clamped to the last token and masked past it
//    (gt_load_a1: the uniform base + a 32-bit lane offset, one address register per load).  Per K-step a wave reads the three N
//    blocks' B operands ONCE (three ds_read_b128) and every read feeds all TB token blocks before the next one: 3 x TB
//    v_mfma_f32_16x16x32 per K-step into 3 x TB accumulators (36 registers at TB = 3) - where gemm_gatherxw's third block re-reads B.
//    REGISTER SCHEDULE: block 0's four A operands are requested ahead of the rebuild and held through it, as in the parents.  The
//    4 x (TB - 1) operands of blocks 1 and 2 are requested back to back BEHIND the tile write - when ca / cb / ra / rb, the 48 - 96
//    registers of the rebuilt entries, are dead - and in front of the next tile's gathers, which then fly beside them through the
//    MFMA phase.  A scheduling barrier on either side keeps the compiler from lifting them above the tile write, where they would
//    sit on top of the peak.  Where an instantiation still spilled at 2 workgroups per CU it is relaxed to 1 (g12w_min_wg).
//  * EPILOGUE, once per token block over the tile's first 12 KiB with a barrier between blocks: the 4 waves' three partial D meet in
//    LDS and are added in wave order.  S == 1: the output bias is added in fp32 and the sum rounded once and stored to y, as
//    gemm_gather12 does - no second kernel.  S >= 2: the RAW fp32 sums of every live token and ALL 48 outputs of the group go to
//    partials[part][token][rg x 48 + 0 ... 47] (row length n_groups x 48 >= O), 64-byte runs, plain vector stores; every word
//    gemm_gather12w_sum_kernel reads (p < S, token < tokens, o < O) is written by exactly one item of this launch: what the workspace
//    held before never reaches y.
//  * gemm_gather12w_sum_kernel<DT>, next on the stream when S >= 2: y[token][o] = sum over p ASCENDING of partials[p][token][o] in
//    fp32, then the output bias in fp32, then one rounding (VPTQ_GEMV_OUT_F32: the fp32 sum).  A copy of gemm_gather12c_sum_kernel in
//    this unit, so that gemm_gather12c.hip's device code stays what it is.
// BIT CONTRACT: for every token block the K-step -> wave mapping, the order of the MFMAs into the block's accumulators (the part's
// tiles in order, steps 0 - 3) and the wave-order LDS sum are gemm_gather12c_kernel's; the second kernel's order is its sum kernel's.
// A token's output bits depend neither on its slot nor on the batch size: at S = 1 they are what vptq_quant_gemm_gather12 gives that
// token, at S >= 2 what vptq_quant_gemm_gather12c gives it with the same (S, tpp), in a call of <= 16 tokens.
// There is no form with a permutation (permute_x_tokens in front, vptq_quant_gemm_gather12w).  LDS 48 KiB + the table.  No atomics, no
// scratch in any of the 12 instantiations (profiles/r39/listings.md), plain vector stores only.
// NOT HERE: a fourth token block (49 - 64 tokens), sibling groups (gemm_gather12w_grouped.hip), v = 6, the folded / selective arithmetics.
#include "gemm_gather_tile.h"
#include "launch.h"

namespace vptq {

// (gemm_gather12.hip's constants, copies)
constexpr int kG12wV = 12;
constexpr int kG12wEB = kG12wV * 2;                     // bytes per codebook entry
constexpr int kG12wRows = 4;                            // vector-rows per row group
constexpr int kG12wOut = kG12wRows * kG12wV;            // 48 outputs = 3 N blocks
constexpr int kG12wTile = 512;                          // columns per tile: kGTThreads / 4 chunks of 8
constexpr int kG12wChunks = kG12wTile / 8;
constexpr int kG12wTileBytes = 3 * kG12wChunks * 16 * 16;   // [N block][chunk][16 outputs][16 bytes]: 48 KiB
constexpr int kG12wResLdsMax = 32768;
constexpr int kG12wMaxParts = 16;
constexpr int kG12wSumThreads = 256;

typedef uint32_t u32x4_a8 __attribute__((ext_vector_type(4), aligned(8)));
typedef uint32_t u32x2_a8 __attribute__((ext_vector_type(2), aligned(8)));

// gemm_gather12c's argument block: partials [S][tokens][op] fp32, op = n_groups x 48; tpp tiles per part; n_items = n_groups x S
struct GemmGather12wParams {
  GemmGatherParams g;
  float* partials;
  int S, tpp, n_items, op;
};

// workgroups per CU the register budget is held to: 2 (256 registers), which 8 of the 12 instantiations meet without a spill (183 -
// 236 VGPRs).  The 4 with a residual table AND three token blocks (RES = 1 / 2, TB = 3, both dtypes) spilled 15 registers there (60
// bytes of scratch: the residual entries in flight beside three blocks' A operands and 36 accumulators) and take what they need,
// 230 VGPRs + 52 AGPRs at one workgroup per CU (profiles/r39/listings.md)
constexpr int g12w_min_wg(int res, int tb) { return res != 0 && tb == 3 ? 1 : 2; }

// element E (compile time) of T bits (wave uniform) out of the normalised window n[0..7] (gemm_gatherx.hip: gx_elem, a copy)
template <int E>
static __device__ __forceinline__ uint32_t g12w_elem(const uint32_t (&n)[8], int T, uint32_t mask) {
  if constexpr (E == 0) return n[0] & mask;
  const int p = E * T, wi = p >> 5, s = p & 31;
  uint32_t lo = n[0], hi = n[1];
#pragma unroll
  for (int j = 1; j <= E; ++j) {
    const uint32_t next = j + 1 < 8 ? n[(j + 1) & 7] : 0u;   // (a word 8 only at s = 0: T = 32, E = 7)
    lo = wi == j ? n[j] : lo;
    hi = wi == j ? next : hi;
  }
  return __builtin_amdgcn_alignbit(hi, lo, (uint32_t)s) & mask;
}

// first column of chunk dch of tile t (a chunk past the row end clamps to the last chunk of the row)
static __device__ __forceinline__ int g12w_dcol(int t, int dch, int G) { const int c = t * kG12wTile + dch * 8; return c < G ? c : G - 8; }

static __device__ __forceinline__ u32x4 g12w_masked(const u32x4& v, bool live) {
  return u32x4{live ? v[0] : 0u, live ? v[1] : 0u, live ? v[2] : 0u, live ? v[3] : 0u};
}

template <typename DT, int RES, int TB>
__global__ __launch_bounds__(kGTThreads, g12w_min_wg(RES, TB)) void gemm_gather12w_kernel(const GemmGather12wParams Q) {
  static_assert(RES >= 0 && RES <= 2, "residual: none, LDS, L2");
  static_assert(TB == 2 || TB == 3, "17 - 32 / 33 - 48 tokens");
  extern __shared__ __attribute__((aligned(16))) unsigned char g12w_smem[];
  const GemmGatherParams& P = Q.g;
  u32x4* const tile = (u32x4*)g12w_smem;                               // [N block][chunk][16 outputs]: 48 KiB
  const unsigned char* const rtab = g12w_smem + kG12wTileBytes;        // RES = 1: the residual table
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int G = P.G, N = P.N, O = P.O, tokens = P.tokens;
  const int T = P.ib + P.rb, ib = P.ib;
  const uint32_t tmask = T >= 32 ? 0xffffffffu : ((1u << T) - 1u), mmask = (1u << ib) - 1u;
  // the 9th window word: 8 T bits + the largest offset (24, 16 or 0 bits: T odd, T % 4 == 2, T % 4 == 0) beyond 8 words (T = 31)
  const bool need9 = 8 * T + ((T & 1) ? 24 : (T & 2) ? 16 : 0) > 256;
  const int last = P.row_words - 1;
  const int n_tiles = (G + kG12wTile - 1) / kG12wTile;
  const int S = Q.S, tpp = Q.tpp;
  if constexpr (RES == 1) {   // once per workgroup, not per item
    const int n8 = P.res_bytes >> 3;   // (24-byte entries: the table is whole 8-byte units)
    for (int i = tid; i < n8; i += kGTThreads)
      *(u32x2*)(g12w_smem + kG12wTileBytes + (size_t)i * 8) = *(const u32x2_a8*)(P.rcent + (size_t)i * 8);
    __syncthreads();
  }
  // dequant role: 8 consecutive columns (chunk dch) of the 12 outputs of vector-row dr = wave of the group
  const int dr = wave, dch = lane;
  const uint32_t wx = (uint32_t)(dch & 7);
  // MFMA role: lane (token / output mj, k group mkg); step i reads chunk 16 wave + 4 mkg + i
  const int mj = lane & 15, mkg = lane >> 4;
  const int mch0 = wave * 16 + mkg * 4;
  // block b's row of x, 16 b + mj clamped to the last token, as a byte offset (gt_load_a1); block 0 is whole: 16 < tokens
  uint32_t xoff[TB];
  bool tok_b[TB];
#pragma unroll
  for (int b = 0; b < TB; ++b) {
    const int tk = 16 * b + mj;
    tok_b[b] = tk < tokens;
    xoff[b] = (uint32_t)(tk < tokens ? tk : tokens - 1) * (uint32_t)G * 2u;
  }

  for (int it = blockIdx.x; it < Q.n_items; it += gridDim.x) {
    const int rg = it / S, part = it - rg * S;
    const int t0 = part * tpp, t1 = t0 + tpp < n_tiles ? t0 + tpp : n_tiles;   // the part's tiles: t0 < t1 (the host rule)
    const int row = rg * kG12wRows + dr;
    const uint32_t* const irow = P.idx + (size_t)(row < N ? row : N - 1) * P.row_words;
    auto ptile = [&](int t) { return t < t1 ? t : t1 - 1; };   // a prefetch past the part stays on the part's last tile
    auto dcol = [&](int t) { return g12w_dcol(t, dch, G); };
    // ---- the index window: gemm_gatherx.hip's (see the head of gemm_gather12.hip)
    auto load_idx = [&](int t, uint32_t (&n)[8]) {
      const uint32_t cb = (uint32_t)(dcol(t) >> 3) * (uint32_t)T;   // the chunk's first byte in the row
      const int w0 = (int)(cb >> 2);
      const uint32_t off = (cb & 3u) * 8u;
      uint32_t w[9];
      if (w0 + 8 <= last) {
        const u32x4_a4 a = *(const u32x4_a4*)(irow + w0);
        const u32x4_a4 b = *(const u32x4_a4*)(irow + w0 + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { w[j] = a[j]; w[4 + j] = b[j]; }
        w[8] = need9 ? *(const u32_a4*)(irow + w0 + 8) : 0u;
      } else {
#pragma unroll
        for (int j = 0; j < 9; ++j) w[j] = *(const u32_a4*)(irow + (w0 + j < last ? w0 + j : last));
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) n[j] = __builtin_amdgcn_alignbit(w[j + 1], w[j], off);
    };
    // ---- the gathers: a 24-byte entry as 16 + 8 bytes (ca / cb: outputs 0 - 7 / 8 - 11 of the 8 columns)
    u32x4 ca[8], ra[RES ? 8 : 1];
    u32x2 cb[8], rb[RES ? 8 : 1];
    auto gather1 = [&](int e, uint32_t v) {
      const char* const c = P.cent + (size_t)(v & mmask) * kG12wEB;
      ca[e] = *(const u32x4_a8*)c;
      cb[e] = *(const u32x2_a8*)(c + 16);
      if constexpr (RES == 1) {
        const unsigned char* const r = rtab + (v >> ib) * (uint32_t)kG12wEB;
        ra[e] = *(const u32x4_a8*)r;
        rb[e] = *(const u32x2_a8*)(r + 16);
      }
      if constexpr (RES == 2) {
        const char* const r = P.rcent + (size_t)(v >> ib) * kG12wEB;
        ra[e] = *(const u32x4_a8*)r;
        rb[e] = *(const u32x2_a8*)(r + 16);
      }
    };
    auto gather = [&](const uint32_t (&n)[8]) {
      gather1(0, g12w_elem<0>(n, T, tmask)); gather1(1, g12w_elem<1>(n, T, tmask));
      gather1(2, g12w_elem<2>(n, T, tmask)); gather1(3, g12w_elem<3>(n, T, tmask));
      gather1(4, g12w_elem<4>(n, T, tmask)); gather1(5, g12w_elem<5>(n, T, tmask));
      gather1(6, g12w_elem<6>(n, T, tmask)); gather1(7, g12w_elem<7>(n, T, tmask));
    };
    // ---- the rebuild in place: c + r, * s, + b, each rounded to 16 bits; columns past the row end become 0
    auto rebuild = [&](const uint32_t (&sp)[4], const uint32_t (&bp)[4], bool dvalid) {
      gt_rebuild<DT, RES != 0>(ca, ra, sp, bp, dvalid);
#pragma unroll
      for (int e = 0; e < 8; e += 2) {
        uint32_t v[4] = {cb[e][0], cb[e][1], cb[e + 1][0], cb[e + 1][1]};
        if constexpr (RES != 0) {
          const uint32_t r[4] = {rb[e][0], rb[e][1], rb[e + 1][0], rb[e + 1][1]};
          DT::add4(v, r);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int h = q >> 1;   // column e + h: half h of the pair registers sp / bp[e >> 1]
          v[q] = DT::add2_bcast(DT::mul2_bcast(v[q], sp[e >> 1], h), bp[e >> 1], h);
          v[q] = dvalid ? v[q] : 0u;
        }
        cb[e] = u32x2{v[0], v[1]};
        cb[e + 1] = u32x2{v[2], v[3]};
      }
    };
    // ---- transpose to 12 outputs x 8 k values and write them in B-operand order (head of gemm_gather12.hip: swizzle and banks)
    auto write_tile = [&]() {
#pragma unroll
      for (int p = 0; p < 6; ++p) {
        uint32_t c[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) c[e] = p < 4 ? ca[e][p & 3] : cb[e][p & 1];
        const u32x4 lo = {__builtin_amdgcn_perm(c[1], c[0], 0x05040100u), __builtin_amdgcn_perm(c[3], c[2], 0x05040100u),
                          __builtin_amdgcn_perm(c[5], c[4], 0x05040100u), __builtin_amdgcn_perm(c[7], c[6], 0x05040100u)};
        const u32x4 hi = {__builtin_amdgcn_perm(c[1], c[0], 0x07060302u), __builtin_amdgcn_perm(c[3], c[2], 0x07060302u),
                          __builtin_amdgcn_perm(c[5], c[4], 0x07060302u), __builtin_amdgcn_perm(c[7], c[6], 0x07060302u)};
        const uint32_t g0 = (uint32_t)(dr * kG12wV + 2 * p), g1 = g0 + 1u;   // outputs 2 p, 2 p + 1 of the row, as outputs of the group
        tile[((g0 >> 4) * kG12wChunks + (uint32_t)dch) * 16u + ((g0 & 15u) ^ wx)] = lo;
        tile[((g1 >> 4) * kG12wChunks + (uint32_t)dch) * 16u + ((g1 & 15u) ^ wx)] = hi;
      }
    };
    uint32_t wq[8], sp[4], bp[4], sp_next[4], bp_next[4];
    load_idx(t0, wq);
    gt_load_sb(P, dcol(t0), sp, bp);
    gather(wq);
    load_idx(ptile(t0 + 1), wq);
    gt_load_sb(P, dcol(ptile(t0 + 1)), sp_next, bp_next);
    f32x4 acc[TB][3];
#pragma unroll
    for (int tb = 0; tb < TB; ++tb)
#pragma unroll
      for (int b = 0; b < 3; ++b) acc[tb][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int t = t0; t < t1; ++t) {
      // ---- block 0's A operands of this tile: 4 x 16 bytes of x, 32 consecutive columns of one token, ahead of the rebuild
      u32x4 xa[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) xa[i] = gt_load_a1<false>(nullptr, P.x, xoff[0], G, t * kG12wTile + (mch0 + i) * 8);
      rebuild(sp, bp, t * kG12wTile + dch * 8 < G);
      __syncthreads();   // the previous tile's MFMA reads (and the previous item's sums) are done
      write_tile();
      // ---- blocks 1 and 2: their A operands back to back, once the rebuilt entries have left their registers
      __builtin_amdgcn_sched_barrier(0);
      u32x4 xb[TB - 1][4];
#pragma unroll
      for (int tb = 1; tb < TB; ++tb)
#pragma unroll
        for (int i = 0; i < 4; ++i) xb[tb - 1][i] = gt_load_a1<false>(nullptr, P.x, xoff[tb], G, t * kG12wTile + (mch0 + i) * 8);
      __builtin_amdgcn_sched_barrier(0);
      // ---- the next tile's gathers fly during the MFMA phase; the index window and scale / bias of the one after follow
      if (t + 1 < t1) {
        gather(wq);
#pragma unroll
        for (int q = 0; q < 4; ++q) { sp[q] = sp_next[q]; bp[q] = bp_next[q]; }
        load_idx(ptile(t + 2), wq);
        gt_load_sb(P, dcol(ptile(t + 2)), sp_next, bp_next);
      }
      __syncthreads();   // tile complete
      // ---- this wave's 4 K-steps: three B reads, each feeding every token block before the next read
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool kin = t * kG12wTile + (mch0 + i) * 8 < G;
        u32x4 a[TB];
        a[0] = g12w_masked(xa[i], kin);   // (block 0 is whole)
#pragma unroll
        for (int tb = 1; tb < TB; ++tb) a[tb] = g12w_masked(xb[tb - 1][i], kin && tok_b[tb]);
        const uint32_t slot = (uint32_t)((mch0 + i) * 16) + ((uint32_t)mj ^ (uint32_t)((mch0 + i) & 7));
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          const u32x4 bv = tile[(uint32_t)(b * kG12wChunks * 16) + slot];
#pragma unroll
          for (int tb = 0; tb < TB; ++tb) acc[tb][b] = mfma16x16x32<DT>(a[tb], bv, acc[tb][b]);
        }
      }
    }
    // ---- one epilogue per token block: the 4 waves' partial D of the three N blocks, added in wave order; D element (token of the
    // block = (l >> 4) * 4 + reg, output = l & 15).  The first barrier of a block also ends the reads of the block before
    {
      float* const scr = (float*)g12w_smem;   // [wave][N block][reg][lane]: the tile's first 12 KiB
      const int r = wave;
#pragma unroll
      for (int tb = 0; tb < TB; ++tb) {
        __syncthreads();
#pragma unroll
        for (int b = 0; b < 3; ++b)
#pragma unroll
          for (int q = 0; q < 4; ++q) scr[((wave * 3 + b) * 4 + q) * 64 + lane] = acc[tb][b][q];
        __syncthreads();
        const int token = 16 * tb + (lane >> 4) * 4 + r;
        float* const prow = Q.partials + ((size_t)part * tokens + (token < tokens ? token : 0)) * Q.op + (size_t)rg * kG12wOut + (lane & 15);
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          float sum = scr[(b * 4 + r) * 64 + lane];
#pragma unroll
          for (int w = 1; w < 4; ++w) sum += scr[((w * 3 + b) * 4 + r) * 64 + lane];
          if (S > 1) {   // the raw sums of all 48 outputs: lanes 0 - 15 of a token are one 64-byte run
            if (token < tokens) prow[b * 16] = sum;
          } else {       // the whole row: gemm_gather12's epilogue
            const int o = rg * kG12wOut + b * 16 + (lane & 15);
            if (token < tokens && o < O) {
              if (P.bias) sum += DT::to_float(P.bias[o]);
              if (P.out_f32) ((float*)P.y)[(size_t)token * O + o] = sum;
              else ((uint16_t*)P.y)[(size_t)token * O + o] = DT::from_float(sum);
            }
          }
        }
      }
    }
  }
}

// y[token][o] = sum over the parts in ascending order, + the output bias, one rounding (gemm_gather12c_sum_kernel, a copy)
template <typename DT>
__global__ __launch_bounds__(kG12wSumThreads) void gemm_gather12w_sum_kernel(const float* __restrict__ partials, const uint16_t* __restrict__ bias,
                                                                            void* __restrict__ y, int O, int op, int tokens, int S, int out_f32) {
  const int o = blockIdx.x * kG12wSumThreads + threadIdx.x, token = blockIdx.y;
  if (o >= O || token >= tokens) return;
  const size_t plane = (size_t)tokens * op;
  const float* const p = partials + (size_t)token * op + o;
  float sum = p[0];
  for (int s = 1; s < S; ++s) sum += p[(size_t)s * plane];
  if (bias) sum += DT::to_float(bias[o]);
  if (out_f32) ((float*)y)[(size_t)token * O + o] = sum;
  else ((uint16_t*)y)[(size_t)token * O + o] = DT::from_float(sum);
}

// ---- host side -------------------------------------------------------------------
// what one call IS: gemm_gather12_decide's format decision (template arguments, index widths, LDS) + the token blocks + the split,
// decided once for the launcher, the workspace query and vptq_quant_gemm_gather12w_instance.  wgcu: the RESIDENT workgroups per CU -
// the smaller of the LDS bound and g12w_min_wg(res, tb); the slots the rule counts are CUs x wgcu.
// parts == 1: no split.  parts >= 2 is a request, gemm_gather12c's formula: tpp = ceil(tiles / min(parts, tiles, 16)), S = ceil(tiles /
// tpp) - every part non-empty, S <= 16; a forced split coincides with vptq_quant_gemm_gather12c's.  parts == 0 is the library's rule.
// THE RULE AND ITS EVIDENCE (profiles/r39/sweep.md: forced parts 1 / 2 / 3 / 4 / 6 / 8 / 14 / 16 on 4096 x 4096, 14336 x 4096, 4096 x 1024, 4096 x
// 14336 and 8192 x 8192 (columns x outputs), v12-k65536-4096 and -0, both dtypes, with and without a permutation, 17 / 32 / 48 tokens; one
// MI355X, 256 CUs; 696 rows, 120 cells).  The starting rule was g12c_rule_parts' shape - the smallest tiles-per-part that DIVIDES the
// tile count, gives at most 16 parts and keeps n_groups x S <= 2.5 x slots; if no divisor does, the smallest tiles-per-part that keeps
// the bound - with S = 1 allowed (tiles-per-part = all tiles), S = 1 at once where the row groups alone exceed 1.25 x slots, and slots =
// CUs x wgcu of the instantiation.  With two token blocks, and with three and no residual table, its choice was the fastest measured
// split or within 3 % of it in every cell: the best S does not move with the token count (8192 x 8192 v12-k65536-4096 fp16: S = 4 at
// 67.2 / 70.0 us for 17 / 32 tokens; 14336 x 4096: S = 14 at 63.6 / 66.0; no split: 88.5 - 145.8), so the partials' traffic does not
// shift it.  THE CORRECTION is for the four instantiations relaxed to ONE workgroup per CU (three blocks beside a residual table):
// counted with 256 slots the rule halved the parts and lost - 8192 x 8192 at 48 tokens S = 2 108.3 us against S = 4 91.8; 14336 x 4096
// S = 7 91.0 against S = 14 85.5; 4096 x 14336 S = 2 90.4 against S = 4 85.7 - 16 of the 120 cells more than 3 % (up to 19 %) behind the
// best split.  The items of a row group are short and the walk it += gridDim.x deals them out evenly whatever the residency, so the
// rule counts slots = CUs x the LDS bound's 2 for EVERY instantiation; the grid is still CUs x wgcu.  So corrected, its choice is within
// 3.1 % of the fastest measured split in all 120 cells.
int gemm_gather12w_rule_parts(int tiles, int groups, int slots) {   // (kernels.h: gemm_gather12_grouped.hip reads it too)
  if (4LL * groups > 5LL * slots) return 1;
  for (int pass = 0; pass < 2; ++pass)
    for (int tpp = 1; tpp <= tiles; ++tpp) {
      const int S = (tiles + tpp - 1) / tpp;
      if (S > kG12wMaxParts || (pass == 0 && tiles % tpp != 0)) continue;
      if (2LL * groups * S <= 5LL * slots) return S;
    }
  return 1;
}

bool gemm_gather12w_eligible(const VptqLayerDesc& d, int tokens) {
  return tokens >= 17 && tokens <= 48 && gemm_gather12_eligible(d, 16);   // gemm_gather12's layers
}

GemmGather12wDecision gemm_gather12w_decide(const VptqLayerDesc& d, int tokens, int parts) {
  GemmGather12wDecision D = {};
  D.base = gemm_gather12_decide(d, 16);
  D.base.tok = tokens;
  D.tb = (tokens + 15) / 16;
  const int by_lds = D.base.wgcu, by_regs = g12w_min_wg(D.base.res, D.tb);   // (the parent's: what the LDS leaves, at most 2)
  if (D.base.wgcu > by_regs) D.base.wgcu = by_regs;
  const int tiles = D.base.tiles, slots = device_cus() * D.base.wgcu, groups = D.base.n_groups;
  int want = parts;
  if (parts == 0) want = gemm_gather12w_rule_parts(tiles, groups, device_cus() * by_lds);
  if (want > kG12wMaxParts) want = kG12wMaxParts;
  if (want > tiles) want = tiles;
  if (want < 1) want = 1;
  D.tpp = (tiles + want - 1) / want;
  D.parts = D.tpp > 0 ? (tiles + D.tpp - 1) / D.tpp : 1;
  D.items = groups * D.parts;
  D.grid = D.items < slots ? D.items : slots;
  D.rgs = D.grid > 0 ? (D.items + D.grid - 1) / D.grid : 0;
  D.base.grid = D.grid; D.base.rgs = D.rgs;
  D.op = groups * kG12wOut;
  D.partial_bytes = D.parts >= 2 ? (size_t)D.parts * tokens * D.op * sizeof(float) : 0;
  D.sum_grid_x = (d.out_features + kG12wSumThreads - 1) / kG12wSumThreads;
  D.sum_grid_y = tokens;
  D.serves = parts >= 0 && gemm_gather12w_eligible(d, tokens);
  return D;
}

template <typename DT, int RES>
static hipError_t launch_g12w_tb(const GemmGather12wParams& Q, const GemmGather12wDecision& D, hipStream_t st) {
  const dim3 grid(D.grid), block(kGTThreads);
  if constexpr (RES == 1) {   // 48 KiB + the table: past the 64 KiB a kernel may use unasked
    const hipError_t e = D.tb == 2 ? allow_dynamic_lds<gemm_gather12w_kernel<DT, 1, 2>>(kG12wTileBytes + kG12wResLdsMax)
                                   : allow_dynamic_lds<gemm_gather12w_kernel<DT, 1, 3>>(kG12wTileBytes + kG12wResLdsMax);
    if (e != hipSuccess) return e;
  }
  if (D.tb == 2) hipLaunchKernelGGL((gemm_gather12w_kernel<DT, RES, 2>), grid, block, D.base.lds, st, Q);
  else hipLaunchKernelGGL((gemm_gather12w_kernel<DT, RES, 3>), grid, block, D.base.lds, st, Q);
  return hipGetLastError();
}

template <typename DT>
static hipError_t launch_g12w(const GemmGather12wParams& Q, const GemmGather12wDecision& D, hipStream_t st) {
  hipError_t e = hipErrorInvalidValue;
  switch (D.base.res) {
    case 0: e = launch_g12w_tb<DT, 0>(Q, D, st); break;
    case 1: e = launch_g12w_tb<DT, 1>(Q, D, st); break;
    case 2: e = launch_g12w_tb<DT, 2>(Q, D, st); break;
    default: break;
  }
  if (e != hipSuccess || D.parts < 2) return e;   // one part: the main kernel has written y
  hipLaunchKernelGGL((gemm_gather12w_sum_kernel<DT>), dim3(D.sum_grid_x, D.sum_grid_y), dim3(kG12wSumThreads), 0, st, Q.partials, Q.g.bias, Q.g.y,
                     Q.g.O, Q.op, Q.g.tokens, Q.S, Q.g.out_f32);
  return hipGetLastError();
}

// d: a layer WITHOUT a permutation (a permuted one as gemm_gather_px_plain(d), x = x[perm]); partials: D.partial_bytes of fp32 (S >= 2)
hipError_t launch_gemm_gather12w(const VptqLayerDesc& d, const void* x, void* y, int tokens, bool out_f32, int parts, void* partials,
                                 hipStream_t st) {
  const GemmGather12wDecision D = gemm_gather12w_decide(d, tokens, parts);
  if (d.perm || !D.serves || D.grid < 1 || D.tb < 2 || D.tb > 3 || (D.parts >= 2 && !partials) ||
      D.base.lds > kG12wTileBytes + kG12wResLdsMax)
    return hipErrorInvalidValue;
  GemmGather12wParams Q = {};
  Q.g = gemm_gather_params(d, x, y, tokens, out_f32, D.base.n_groups);
  Q.g.ib = D.base.ib; Q.g.rb = D.base.rb; Q.g.res_bytes = D.base.res_bytes;
  Q.partials = D.parts >= 2 ? (float*)partials : (float*)y;   // (S == 1: never dereferenced)
  Q.S = D.parts; Q.tpp = D.tpp; Q.n_items = D.items; Q.op = D.op;
  return D.base.f16 ? launch_g12w<F16>(Q, D, st) : launch_g12w<BF16>(Q, D, st);
}

}  // namespace vptq
