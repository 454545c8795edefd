// Batched decode of SIBLING layers (q / k / v, gate / up) of the large-codebook VPTQ formats of VECTOR LENGTH 12 ("v12-k65536-4096 / -256 /
// -0": gemm_gather12.hip's layers), 1 - 16 tokens of 2 - 4 members in ONE launch: gemm_gather12c.hip's (row group, column part) item
// behind a member walk in the manner of gemm_gatherx_grouped_kernel (gemm_gatherx_grouped.hip).
//
// Without it every member goes out alone - gemm_gather12, gemm_gather12c (two launches), two gemv_gatherx launches or vptq_dequant + a
// dense GEMM, whichever its size gives it, each behind an x gather of its own when permuted - and k / v of an 8B decoder (1024 outputs
// = 22 row groups of 48) leave most of the 512 resident workgroup slots (256 CUs x 2) empty in every one of those launches.
//  * WORK LIST: the members share ONE list of items; an item is (member, row group of 4 vector-rows = 48 outputs, column part of whole
//    512-column tiles).  The members share in_features, hence the tile count: one split, S parts of tpp tiles, holds for the group.
//    Member m owns the items [first_item[m], first_item[m + 1]), groups[m] x S of them; inside a member item i is row group i / S, part
//    i % S, as in gemm_gather12c: the parts of one row group run side by side on neighbouring workgroups.  A workgroup walks it =
//    blockIdx.x, it += gridDim.x; grid = min(items, CUs x wgcu), wgcu gemm_gather12_decide's of the shared format.
//  * MEMBER SWITCH: it only rises, so a workgroup's member only rises - at most n - 1 switches.  At a switch the workgroup takes the
//    member's argument block (a uniform search over <= 4 entries; the block goes to SGPRs) and, RES = 1, re-stages that member's
//    residual table behind the 48 KiB tile between two barriers (the members' tables differ in content, never in size).  The first
//    item of a workgroup stages its table the same way; there is no table copy except at a member change.
//  * THE ROW-GROUP BODY IS THE FOURTH COPY of gemm_gather12.hip's, taken from gemm_gather12c.hip statement for statement (its head and
//    gemm_gather12.hip's describe it: the part's tile range [t0, t1), prefetches clamped to the part's last tile, the 48 KiB tile
//    [N block][chunk][16 outputs][16 bytes] with the slot XOR-ed by chunk & 7, four K-steps per wave x three mfma16x16x32<DT>, the
//    gathers of tile t + 1 in flight during the MFMAs of tile t).  A copy for the reason given there: as a shared function such bodies
//    have twice cost 3 - 8 % and changed the parents' listings (profiles/r17, profiles/r31).  A CHANGE TO THE BODY HERE BELONGS IN
//    gemm_gather12.hip, gemm_gather12c.hip, gemm_gather12w.hip AND gemm_gather12w_grouped.hip TOO, AND THE OTHER WAY ROUND.
//  * EPILOGUE: the 4 waves' three partial D meet in LDS and are added in wave order.  S == 1: the output bias is added in fp32, the sum
//    rounded once and stored into y[m] (VPTQ_GEMV_OUT_F32: the fp32 sum) - gemm_gather12's epilogue.  S >= 2: the raw fp32 sums of all 48
//    outputs go to partials_m[part][token][rg x 48 + 0 ... 47] in the workspace (plain vector stores; no atomics, no counters, no
//    waiting on another workgroup); then ONE launch of gemm_gather12_grouped_sum_kernel<DT> covers every member: grid.x runs over the
//    members' output blocks of 256, concatenated, grid.y = tokens; y[token][o] = sum over p ASCENDING of the partials in fp32, then the
//    output bias, then one rounding - gemm_gather12c_sum_kernel's arithmetic.  Every word the sum kernel reads is written by exactly one
//    item of the launch in front of it: what the workspace held before never reaches y.
//  * PERMUTATIONS: no permuted form.  A permuted member arrives as its plain descriptor with x[perm] (in the workspace) for its x; one
//    permute_x_tokens launch per DISTINCT perm pointer is the caller's (vptq_quant_gemm_gather12_grouped).
// BIT CONTRACT: an item depends neither on the grid nor on the workgroup that runs it.  For S >= 2, y[m] is bit-identical to
// vptq_quant_gemm_gather12c(descs[m], parts = S); for S == 1 to vptq_quant_gemm_gather12(descs[m]) - at the same token count and x.
// LDS 48 KiB + the table; 2 workgroups per CU as the parents; no instantiation has scratch (profiles/r40/listings.md).
// NOT HERE: 17 - 48 tokens of v = 12 groups (gemm_gather12w_grouped.hip: gemm_gather12w's token-block pass behind this walk), groups of mixed format, v = 6, the
// folded / selective arithmetics.
#include "gemm_gather_tile.h"
#include "launch.h"

namespace vptq {

// (gemm_gather12.hip's constants, copies)
constexpr int kG12gV = 12;
constexpr int kG12gEB = kG12gV * 2;                     // bytes per codebook entry
constexpr int kG12gRows = 4;                            // vector-rows per row group
constexpr int kG12gOut = kG12gRows * kG12gV;            // 48 outputs = 3 N blocks
constexpr int kG12gTile = 512;                          // columns per tile: kGTThreads / 4 chunks of 8
constexpr int kG12gChunks = kG12gTile / 8;
constexpr int kG12gTileBytes = 3 * kG12gChunks * 16 * 16;   // [N block][chunk][16 outputs][16 bytes]: 48 KiB
constexpr int kG12gResLdsMax = 32768;
constexpr int kG12gMaxParts = 16;
constexpr int kG12gSumThreads = 256;
constexpr int kG12gMembers = 4;

typedef uint32_t u32x4_a8 __attribute__((ext_vector_type(4), aligned(8)));
typedef uint32_t u32x2_a8 __attribute__((ext_vector_type(2), aligned(8)));

// every member's argument block (the single kernels') + its partials [S][tokens][op[m]] fp32, op[m] = groups[m] x 48 (S >= 2), and the
// split: S parts of tpp tiles; member m owns the items [first_item[m], first_item[m + 1])
struct GemmGather12GroupedParams {
  GemmGatherParams m[kG12gMembers];
  float* partials[kG12gMembers];
  int op[kG12gMembers];
  int first_item[kG12gMembers + 1];
  int n, S, tpp;
};

// the sum launch: member m owns the blocks [first_block[m], first_block[m + 1]) of 256 outputs
struct GemmGather12GroupedSumParams {
  const float* partials[kG12gMembers];
  const uint16_t* bias[kG12gMembers];
  void* y[kG12gMembers];
  int O[kG12gMembers], op[kG12gMembers];
  int first_block[kG12gMembers + 1];
  int tokens, S, out_f32;
};

// workgroups per CU the register budget is held to: the parents' 2 for every instantiation (profiles/r40/listings.md)
constexpr int g12g_min_wg(int) { return 2; }

// element E (compile time) of T bits (wave uniform) out of the normalised window n[0..7] (gemm_gatherx.hip: gx_elem, a copy)
template <int E>
static __device__ __forceinline__ uint32_t g12g_elem(const uint32_t (&n)[8], int T, uint32_t mask) {
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
static __device__ __forceinline__ int g12g_dcol(int t, int dch, int G) { const int c = t * kG12gTile + dch * 8; return c < G ? c : G - 8; }

// one item of one member: row group rg, part `part` of S parts of tpp tiles.  The body of gemm_gather12c_kernel<DT, RES>'s item loop
// (gemm_gather12c.hip), statement for statement, with gemm_gather12_kernel's epilogue where S == 1.  smem: the tile, behind it (RES = 1)
// the member's residual table, staged at the switch.
template <typename DT, int RES>
static __device__ __forceinline__ void g12g_item(const GemmGatherParams& P, unsigned char* smem, float* partials, int op, int S, int tpp,
                                                 int rg, int part) {
  u32x4* const tile = (u32x4*)smem;                                // [N block][chunk][16 outputs]: 48 KiB
  const unsigned char* const rtab = smem + kG12gTileBytes;         // RES = 1: the residual table
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int G = P.G, N = P.N, O = P.O, tokens = P.tokens;
  const int T = P.ib + P.rb, ib = P.ib;
  const uint32_t tmask = T >= 32 ? 0xffffffffu : ((1u << T) - 1u), mmask = (1u << ib) - 1u;
  // the 9th window word: 8 T bits + the largest offset (24, 16 or 0 bits: T odd, T % 4 == 2, T % 4 == 0) beyond 8 words (T = 31)
  const bool need9 = 8 * T + ((T & 1) ? 24 : (T & 2) ? 16 : 0) > 256;
  const int last = P.row_words - 1;
  const int n_tiles = (G + kG12gTile - 1) / kG12gTile;
  // dequant role: 8 consecutive columns (chunk dch) of the 12 outputs of vector-row dr = wave of the group
  const int dr = wave, dch = lane;
  const uint32_t wx = (uint32_t)(dch & 7);
  // MFMA role: lane (token / output mj, k group mkg); step i reads chunk 16 wave + 4 mkg + i
  const int mj = lane & 15, mkg = lane >> 4;
  const int mch0 = wave * 16 + mkg * 4;
  const uint32_t xoff = (uint32_t)(mj < tokens ? mj : tokens - 1) * (uint32_t)G * 2u;

  const int t0 = part * tpp, t1 = t0 + tpp < n_tiles ? t0 + tpp : n_tiles;   // the part's tiles: t0 < t1 (the host rule)
  const int row = rg * kG12gRows + dr;
  const uint32_t* const irow = P.idx + (size_t)(row < N ? row : N - 1) * P.row_words;
  auto ptile = [&](int t) { return t < t1 ? t : t1 - 1; };   // a prefetch past the part stays on the part's last tile
  auto dcol = [&](int t) { return g12g_dcol(t, dch, G); };
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
    const char* const c = P.cent + (size_t)(v & mmask) * kG12gEB;
    ca[e] = *(const u32x4_a8*)c;
    cb[e] = *(const u32x2_a8*)(c + 16);
    if constexpr (RES == 1) {
      const unsigned char* const r = rtab + (v >> ib) * (uint32_t)kG12gEB;
      ra[e] = *(const u32x4_a8*)r;
      rb[e] = *(const u32x2_a8*)(r + 16);
    }
    if constexpr (RES == 2) {
      const char* const r = P.rcent + (size_t)(v >> ib) * kG12gEB;
      ra[e] = *(const u32x4_a8*)r;
      rb[e] = *(const u32x2_a8*)(r + 16);
    }
  };
  auto gather = [&](const uint32_t (&n)[8]) {
    gather1(0, g12g_elem<0>(n, T, tmask)); gather1(1, g12g_elem<1>(n, T, tmask));
    gather1(2, g12g_elem<2>(n, T, tmask)); gather1(3, g12g_elem<3>(n, T, tmask));
    gather1(4, g12g_elem<4>(n, T, tmask)); gather1(5, g12g_elem<5>(n, T, tmask));
    gather1(6, g12g_elem<6>(n, T, tmask)); gather1(7, g12g_elem<7>(n, T, tmask));
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
      const uint32_t g0 = (uint32_t)(dr * kG12gV + 2 * p), g1 = g0 + 1u;   // outputs 2 p, 2 p + 1 of the row, as outputs of the group
      tile[((g0 >> 4) * kG12gChunks + (uint32_t)dch) * 16u + ((g0 & 15u) ^ wx)] = lo;
      tile[((g1 >> 4) * kG12gChunks + (uint32_t)dch) * 16u + ((g1 & 15u) ^ wx)] = hi;
    }
  };
  uint32_t wq[8], sp[4], bp[4], sp_next[4], bp_next[4];
  load_idx(t0, wq);
  gt_load_sb(P, dcol(t0), sp, bp);
  gather(wq);
  load_idx(ptile(t0 + 1), wq);
  gt_load_sb(P, dcol(ptile(t0 + 1)), sp_next, bp_next);
  f32x4 acc[3];
#pragma unroll
  for (int b = 0; b < 3; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int t = t0; t < t1; ++t) {
    // ---- this tile's A operands: 4 x 16 bytes of x, 32 consecutive columns of one token
    u32x4 xa[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) xa[i] = gt_load_a1<false>(nullptr, P.x, xoff, G, t * kG12gTile + (mch0 + i) * 8);
    rebuild(sp, bp, t * kG12gTile + dch * 8 < G);
    __syncthreads();   // the previous tile's MFMA reads (and the previous item's sums) are done
    write_tile();
    // ---- the next tile's gathers fly during the MFMA phase; the index window and scale / bias of the one after follow
    if (t + 1 < t1) {
      gather(wq);
#pragma unroll
      for (int q = 0; q < 4; ++q) { sp[q] = sp_next[q]; bp[q] = bp_next[q]; }
      load_idx(ptile(t + 2), wq);
      gt_load_sb(P, dcol(ptile(t + 2)), sp_next, bp_next);
    }
    __syncthreads();   // tile complete
    // ---- this wave's 4 K-steps: the A operand once, three B reads and three MFMAs
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool live = mj < tokens && t * kG12gTile + (mch0 + i) * 8 < G;
      const u32x4 a = {live ? xa[i][0] : 0u, live ? xa[i][1] : 0u, live ? xa[i][2] : 0u, live ? xa[i][3] : 0u};
      const uint32_t slot = (uint32_t)((mch0 + i) * 16) + ((uint32_t)mj ^ (uint32_t)((mch0 + i) & 7));
#pragma unroll
      for (int b = 0; b < 3; ++b) acc[b] = mfma16x16x32<DT>(a, tile[(uint32_t)(b * kG12gChunks * 16) + slot], acc[b]);
    }
  }
  // ---- the 4 waves' partial D of the three N blocks, added in wave order; D element (token = (l >> 4) * 4 + reg, output = l & 15).
  // S == 1: gemm_gather12's epilogue (bias in fp32, one rounding, outputs o >= O masked).  S >= 2: gemm_gather12c's - the raw sums of
  // all 48 outputs go to this part's plane of the member's partials: lanes 0 - 15 of a token are one 64-byte run
  {
    float* const scr = (float*)smem;   // [wave][N block][reg][lane]: the tile's first 12 KiB
    __syncthreads();
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) scr[((wave * 3 + b) * 4 + r) * 64 + lane] = acc[b][r];
    __syncthreads();
    const int r = wave, token = (lane >> 4) * 4 + r;
    float* const prow = partials + ((size_t)part * tokens + (token < tokens ? token : 0)) * op + (size_t)rg * kG12gOut + (lane & 15);
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      float sum = scr[(b * 4 + r) * 64 + lane];
#pragma unroll
      for (int w = 1; w < 4; ++w) sum += scr[((w * 3 + b) * 4 + r) * 64 + lane];
      if (S >= 2) {
        if (token < tokens) prow[b * 16] = sum;
      } else {
        const int o = rg * kG12gOut + b * 16 + (lane & 15);
        if (token < tokens && o < O) {
          if (P.bias) sum += DT::to_float(P.bias[o]);
          if (P.out_f32) ((float*)P.y)[(size_t)token * O + o] = sum;
          else ((uint16_t*)P.y)[(size_t)token * O + o] = DT::from_float(sum);
        }
      }
    }
  }
}

// A workgroup walks the items it = blockIdx.x, + gridDim.x, ...: it rises, so the member never falls - the members are visited in
// order, and a member's state (its argument block - pointers, scale / bias, partials -, RES = 1: its residual table in LDS) is set up
// at the switch.  (gemm_gatherx_grouped_kernel's walk over gemm_gather12c's items.)
template <typename DT, int RES>
__global__ __launch_bounds__(kGTThreads, g12g_min_wg(RES)) void gemm_gather12_grouped_kernel(const GemmGather12GroupedParams GP) {
  static_assert(RES >= 0 && RES <= 2, "residual: none, LDS, L2");
  extern __shared__ __attribute__((aligned(16))) unsigned char g12g_smem[];
  const int tid = threadIdx.x;
  const int S = GP.S, tpp = GP.tpp;
  int it = blockIdx.x;
#pragma unroll 1
  for (int m = 0; m < GP.n; ++m) {
    const int first = GP.first_item[m], end = GP.first_item[m + 1];
    if (it >= end) continue;   // (uniform: it is the workgroup's)
    const GemmGatherParams P = GP.m[m];
    float* const partials = GP.partials[m];
    const int op = GP.op[m];
    if constexpr (RES == 1) {
      __syncthreads();   // the other waves' table reads of the previous member's last item are done
      const int n8 = P.res_bytes >> 3;   // (24-byte entries: the table is whole 8-byte units)
      for (int i = tid; i < n8; i += kGTThreads)
        *(u32x2*)(g12g_smem + kG12gTileBytes + (size_t)i * 8) = *(const u32x2_a8*)(P.rcent + (size_t)i * 8);
      __syncthreads();
    }
#pragma unroll 1
    for (; it < end; it += gridDim.x) {
      const int i = it - first, rg = i / S;
      g12g_item<DT, RES>(P, g12g_smem, partials, op, S, tpp, rg, i - rg * S);
    }
  }
}

// every member's y[token][o] = sum over the parts in ascending order, + the output bias, one rounding: gemm_gather12c_sum_kernel's
// arithmetic.  The member of a block is a uniform search over <= 4 entries (first_block[j] = the total for j >= n)
template <typename DT>
__global__ __launch_bounds__(kG12gSumThreads) void gemm_gather12_grouped_sum_kernel(const GemmGather12GroupedSumParams Q) {
  const int bx = blockIdx.x, token = blockIdx.y;
  const float* partials = Q.partials[0];
  const uint16_t* bias = Q.bias[0];
  void* y = Q.y[0];
  int O = Q.O[0], op = Q.op[0], first = 0;
#pragma unroll
  for (int j = 1; j < kG12gMembers; ++j)
    if (bx >= Q.first_block[j]) { partials = Q.partials[j]; bias = Q.bias[j]; y = Q.y[j]; O = Q.O[j]; op = Q.op[j]; first = Q.first_block[j]; }
  const int tokens = Q.tokens, S = Q.S;
  const int o = (bx - first) * kG12gSumThreads + threadIdx.x;
  if (o >= O || token >= tokens) return;
  const size_t plane = (size_t)tokens * op;
  const float* const p = partials + (size_t)token * op + o;
  float sum = p[0];
  for (int s = 1; s < S; ++s) sum += p[(size_t)s * plane];
  if (bias) sum += DT::to_float(bias[o]);
  if (Q.out_f32) ((float*)y)[(size_t)token * O + o] = sum;
  else ((uint16_t*)y)[(size_t)token * O + o] = DT::from_float(sum);
}

// ---- host side -------------------------------------------------------------------
// what one grouped call IS: gemm_gather12_decide's format decision of the first member (the members share dtype, width and format: the
// caller's check) + every member's row groups + the split, decided once for the launcher, the workspace query and
// vptq_quant_gemm_gather12_grouped_instance.
// parts > 0 is a request, gemm_gather12c_decide's formula: tpp = ceil(tiles / min(parts, tiles, 16)), S = ceil(tiles / tpp) - every part
// non-empty, S <= 16; here S == 1 is allowed (no partials, no sum launch).  parts == 0 is the library's rule: gemm_gather12w's
// (gemm_gather12w_rule_parts, the v = 12 rule that allows one part; gemm_gather12w.hip gives its evidence, profiles/r39) fed the group's
// TOTAL row groups and the resident slots CUs x wgcu.  No rule of its own: none has been measured (profiles/r40/README.md).
GemmGather12GroupedDecision gemm_gather12_grouped_decide(const VptqLayerDesc* descs, int n, int tokens, int parts) {
  GemmGather12GroupedDecision D = {};
  if (n < 1 || n > kG12gMembers) return D;
  D.base = gemm_gather12_decide(descs[0], tokens);
  D.n = n;
  int total_groups = 0;
  for (int m = 0; m < n; ++m) {
    D.groups[m] = (descs[m].num_indices + kG12gRows - 1) / kG12gRows;
    total_groups += D.groups[m];
  }
  const int tiles = D.base.tiles, slots = device_cus() * D.base.wgcu;
  int want = parts;
  if (parts == 0) want = gemm_gather12w_rule_parts(tiles, total_groups, slots);
  if (want > kG12gMaxParts) want = kG12gMaxParts;
  if (want > tiles) want = tiles;
  if (want < 1) want = 1;
  D.tpp = (tiles + want - 1) / want;
  D.parts = D.tpp > 0 ? (tiles + D.tpp - 1) / D.tpp : 1;
  for (int m = 0; m < n; ++m) {
    D.first_item[m + 1] = D.first_item[m] + D.groups[m] * D.parts;
    D.op[m] = D.groups[m] * kG12gOut;
    const size_t bytes = D.parts >= 2 ? (size_t)D.parts * tokens * D.op[m] * sizeof(float) : 0;
    D.partial_bytes[m] = (bytes + 255) & ~(size_t)255;
    D.first_block[m + 1] = D.first_block[m] + (descs[m].out_features + kG12gSumThreads - 1) / kG12gSumThreads;
  }
  D.items = D.first_item[n];
  D.grid = D.items < slots ? D.items : slots;
  D.rgs = D.grid > 0 ? (D.items + D.grid - 1) / D.grid : 0;
  D.base.grid = D.grid; D.base.rgs = D.rgs;
  D.sum_grid_x = D.first_block[n];
  D.sum_grid_y = tokens;
  return D;
}

template <typename DT>
static hipError_t launch_g12g(const GemmGather12GroupedParams& GP, const GemmGather12GroupedSumParams& SP, const GemmGather12GroupedDecision& D,
                              hipStream_t st) {
  const dim3 grid(D.grid), block(kGTThreads);
  const int lds = D.base.lds;
  hipError_t e = hipSuccess;
  switch (D.base.res) {
    case 0: hipLaunchKernelGGL((gemm_gather12_grouped_kernel<DT, 0>), grid, block, lds, st, GP); break;
    case 1:   // 48 KiB + the table: past the 64 KiB a kernel may use unasked
      e = allow_dynamic_lds<gemm_gather12_grouped_kernel<DT, 1>>(kG12gTileBytes + kG12gResLdsMax);
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL((gemm_gather12_grouped_kernel<DT, 1>), grid, block, lds, st, GP);
      break;
    case 2: hipLaunchKernelGGL((gemm_gather12_grouped_kernel<DT, 2>), grid, block, lds, st, GP); break;
    default: return hipErrorInvalidValue;
  }
  e = hipGetLastError();
  if (e != hipSuccess || D.parts < 2) return e;   // one part: the main kernel has written every y[m]
  hipLaunchKernelGGL((gemm_gather12_grouped_sum_kernel<DT>), dim3(D.sum_grid_x, D.sum_grid_y), dim3(kG12gSumThreads), 0, st, SP);
  return hipGetLastError();
}

// descs: the members WITHOUT a permutation (a permuted member as its plain form); x[m]: member m's activations in its own column order;
// partials: the sum of D.partial_bytes of fp32, 256-byte aligned (S >= 2)
hipError_t launch_gemm_gather12_grouped(const VptqLayerDesc* descs, int n, const void* const* x, void* const* y, int tokens, bool out_f32,
                                        int parts, void* partials, hipStream_t st) {
  const GemmGather12GroupedDecision D = gemm_gather12_grouped_decide(descs, n, tokens, parts);
  if (D.n < 2 || D.grid < 1 || tokens < 1 || tokens > 16 || parts < 0 || (D.parts >= 2 && !partials) ||
      D.base.lds > kG12gTileBytes + kG12gResLdsMax)
    return hipErrorInvalidValue;
  GemmGather12GroupedParams GP = {};
  GemmGather12GroupedSumParams SP = {};
  char* next = (char*)partials;
  for (int m = 0; m < n; ++m) {
    // (the table copied into LDS is the one D.base.lds has room for: every member's is the first's size; one tile count for all)
    if (descs[m].perm || !x[m] || !y[m] || descs[m].num_res_centroids * kG12gEB != D.base.res_bytes ||
        descs[m].group_size != descs[0].group_size)
      return hipErrorInvalidValue;
    GP.m[m] = gemm_gather_params(descs[m], x[m], y[m], tokens, out_f32, D.groups[m]);
    GP.m[m].ib = D.base.ib; GP.m[m].rb = D.base.rb; GP.m[m].res_bytes = D.base.res_bytes;
    GP.partials[m] = D.parts >= 2 ? (float*)next : (float*)y[m];   // (S == 1: never dereferenced)
    next += D.partial_bytes[m];
    GP.op[m] = D.op[m];
    GP.first_item[m] = D.first_item[m];
    SP.partials[m] = GP.partials[m]; SP.bias[m] = GP.m[m].bias; SP.y[m] = y[m];
    SP.O[m] = descs[m].out_features; SP.op[m] = D.op[m];
    SP.first_block[m] = D.first_block[m];
  }
  for (int m = n; m <= kG12gMembers; ++m) { GP.first_item[m] = D.items; SP.first_block[m] = D.sum_grid_x; }
  GP.n = n; GP.S = D.parts; GP.tpp = D.tpp;
  SP.tokens = tokens; SP.S = D.parts; SP.out_f32 = out_f32 ? 1 : 0;
  return D.base.f16 ? launch_g12g<F16>(GP, SP, D, st) : launch_g12g<BF16>(GP, SP, D, st);
}

}  // namespace vptq
