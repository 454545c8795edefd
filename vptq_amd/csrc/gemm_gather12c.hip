// Batched decode for the large-codebook VPTQ formats of VECTOR LENGTH 12, COLUMN-PARTS form: gemm_gather12.hip's kernel for layers with
// FEW OUTPUTS.  There a workgroup owns a row group (4 vector-rows = 48 outputs) over ALL columns: a 4096-output layer is 86 row groups on
// 512 resident slots (256 CUs x 2), and its time follows the column count - about 5 us per 512-column tile, serially, with five sixths
// of the machine idle (profiles/r37: 4096 x 4096 43.5 us, 14336 x 4096 loses from 9 tokens).  Here the work item is (ROW GROUP, COLUMN
// PART): part p of a row group covers tiles [p tpp, min((p + 1) tpp, n_tiles)), S parts per row group, every part non-empty
// (gemm_gather12c_decide).  A workgroup walks items it = blockIdx.x, it += gridDim.x of n_groups x S; item it is row group it / S, part
// it % S, so the parts of one row group run side by side on neighbouring workgroups.
//  * THE ROW-GROUP BODY IS A COPY of gemm_gather12.hip's (its head describes it: dequant role of 4 vector-rows x 64 chunks of 8
//    columns, the run-time index window, 24-byte entries gathered as 16 + 8 bytes, RES = none / table in LDS / from L2, the reference's
//    three roundings, the 48 KiB tile [N block][chunk][16 outputs][16 bytes] with the slot XOR-ed by chunk & 7, four K-steps per wave x
//    three v_mfma_f32_16x16x32, the gathers of tile t + 1 in flight during the MFMAs of tile t).  A copy for the reason given there:
//    as a shared function such bodies have twice cost 3 - 8 % and changed the parents' listings (profiles/r17, profiles/r31).  A CHANGE
//    TO THE BODY HERE BELONGS IN gemm_gather12.hip, gemm_gather12w.hip (its third copy), gemm_gather12_grouped.hip (its fourth) AND gemm_gather12w_grouped.hip (its fifth) TOO, AND THE OTHER WAY ROUND.
//  * WHAT DIFFERS: the tile loop runs over [t0, t1) of the part; the index window, g12c_dcol, the scale / bias prefetch and the x
//    columns start at tile t0.  The prefetch of "the tile after next" (index window, scale / bias) and the preamble's second window are
//    clamped to the PART's last tile, t1 - 1 (ptile), and then by g12c_dcol inside the row as in the parent: the address is one the
//    part has already fetched and the values are never used - at the row end as in the parent, and at a part end that is not the row
//    end the workgroup does not fetch the next part's lines, which belong to another workgroup.  An LDS-held residual table is copied once per workgroup, in front of the item loop.
//  * EPILOGUE: the 4 waves' three partial D meet in LDS and are added in wave order, as in the parent.  The item then stores its RAW
//    fp32 sums of every live token and ALL 48 outputs of the group into partials[p][token][rg x 48 + 0 ... 47] (row length n_groups x
//    48 >= O): 16 lanes x 4 bytes = 64-byte runs, plain vector stores; no rounding, no output bias, no atomics, no counters, no waiting
//    on another workgroup.  Every word gemm_gather12c_sum_kernel reads (p < S, token < tokens, o < O) is written by exactly one item
//    of this launch: what the workspace held before never reaches y.
//  * gemm_gather12c_sum_kernel<DT>, next on the stream: y[token][o] = sum over p ASCENDING of partials[p][token][o] in fp32, then the
//    output bias in fp32, then one rounding (VPTQ_GEMV_OUT_F32: the fp32 sum) - the parent's epilogue arithmetic; a fixed order: two
//    launches give the same bits.  A thread per output, coalesced 4-byte loads, S <= 16 of them.
// There is no form with a permutation (permute_x_tokens in front, vptq_quant_gemm_gather12c).  LDS 48 KiB + the table; 2 workgroups per
// CU as the parent; no instantiation has scratch (profiles/r38/listings.md).
// NOT HERE: 17 - 48 tokens (gemm_gather12w.hip: token blocks over this walk), sibling groups, v = 6, the folded / selective arithmetics.
#include "gemm_gather_tile.h"
#include "launch.h"

namespace vptq {

// (gemm_gather12.hip's constants, copies)
constexpr int kG12cV = 12;
constexpr int kG12cEB = kG12cV * 2;                     // bytes per codebook entry
constexpr int kG12cRows = 4;                            // vector-rows per row group
constexpr int kG12cOut = kG12cRows * kG12cV;            // 48 outputs = 3 N blocks
constexpr int kG12cTile = 512;                          // columns per tile: kGTThreads / 4 chunks of 8
constexpr int kG12cChunks = kG12cTile / 8;
constexpr int kG12cTileBytes = 3 * kG12cChunks * 16 * 16;   // [N block][chunk][16 outputs][16 bytes]: 48 KiB
constexpr int kG12cResLdsMax = 32768;
constexpr int kG12cMaxParts = 16;
constexpr int kG12cSumThreads = 256;

typedef uint32_t u32x4_a8 __attribute__((ext_vector_type(4), aligned(8)));
typedef uint32_t u32x2_a8 __attribute__((ext_vector_type(2), aligned(8)));

// the parent's argument block + the split: partials [S][tokens][op] fp32, op = n_groups x 48; tpp tiles per part; n_items = n_groups x S
struct GemmGather12cParams {
  GemmGatherParams g;
  float* partials;
  int S, tpp, n_items, op;
};

// workgroups per CU the register budget is held to: the parent's 2 for every instantiation (profiles/r38/listings.md)
constexpr int g12c_min_wg(int) { return 2; }

// element E (compile time) of T bits (wave uniform) out of the normalised window n[0..7] (gemm_gatherx.hip: gx_elem, a copy)
template <int E>
static __device__ __forceinline__ uint32_t g12c_elem(const uint32_t (&n)[8], int T, uint32_t mask) {
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
static __device__ __forceinline__ int g12c_dcol(int t, int dch, int G) { const int c = t * kG12cTile + dch * 8; return c < G ? c : G - 8; }

template <typename DT, int RES>
__global__ __launch_bounds__(kGTThreads, g12c_min_wg(RES)) void gemm_gather12c_kernel(const GemmGather12cParams Q) {
  static_assert(RES >= 0 && RES <= 2, "residual: none, LDS, L2");
  extern __shared__ __attribute__((aligned(16))) unsigned char g12c_smem[];
  const GemmGatherParams& P = Q.g;
  u32x4* const tile = (u32x4*)g12c_smem;                               // [N block][chunk][16 outputs]: 48 KiB
  const unsigned char* const rtab = g12c_smem + kG12cTileBytes;        // RES = 1: the residual table
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int G = P.G, N = P.N, tokens = P.tokens;
  const int T = P.ib + P.rb, ib = P.ib;
  const uint32_t tmask = T >= 32 ? 0xffffffffu : ((1u << T) - 1u), mmask = (1u << ib) - 1u;
  // the 9th window word: 8 T bits + the largest offset (24, 16 or 0 bits: T odd, T % 4 == 2, T % 4 == 0) beyond 8 words (T = 31)
  const bool need9 = 8 * T + ((T & 1) ? 24 : (T & 2) ? 16 : 0) > 256;
  const int last = P.row_words - 1;
  const int n_tiles = (G + kG12cTile - 1) / kG12cTile;
  const int S = Q.S, tpp = Q.tpp;
  if constexpr (RES == 1) {   // once per workgroup, not per item
    const int n8 = P.res_bytes >> 3;   // (24-byte entries: the table is whole 8-byte units)
    for (int i = tid; i < n8; i += kGTThreads)
      *(u32x2*)(g12c_smem + kG12cTileBytes + (size_t)i * 8) = *(const u32x2_a8*)(P.rcent + (size_t)i * 8);
    __syncthreads();
  }
  // dequant role: 8 consecutive columns (chunk dch) of the 12 outputs of vector-row dr = wave of the group
  const int dr = wave, dch = lane;
  const uint32_t wx = (uint32_t)(dch & 7);
  // MFMA role: lane (token / output mj, k group mkg); step i reads chunk 16 wave + 4 mkg + i
  const int mj = lane & 15, mkg = lane >> 4;
  const int mch0 = wave * 16 + mkg * 4;
  const uint32_t xoff = (uint32_t)(mj < tokens ? mj : tokens - 1) * (uint32_t)G * 2u;

  for (int it = blockIdx.x; it < Q.n_items; it += gridDim.x) {
    const int rg = it / S, part = it - rg * S;
    const int t0 = part * tpp, t1 = t0 + tpp < n_tiles ? t0 + tpp : n_tiles;   // the part's tiles: t0 < t1 (the host rule)
    const int row = rg * kG12cRows + dr;
    const uint32_t* const irow = P.idx + (size_t)(row < N ? row : N - 1) * P.row_words;
    auto ptile = [&](int t) { return t < t1 ? t : t1 - 1; };   // a prefetch past the part stays on the part's last tile
    auto dcol = [&](int t) { return g12c_dcol(t, dch, G); };
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
      const char* const c = P.cent + (size_t)(v & mmask) * kG12cEB;
      ca[e] = *(const u32x4_a8*)c;
      cb[e] = *(const u32x2_a8*)(c + 16);
      if constexpr (RES == 1) {
        const unsigned char* const r = rtab + (v >> ib) * (uint32_t)kG12cEB;
        ra[e] = *(const u32x4_a8*)r;
        rb[e] = *(const u32x2_a8*)(r + 16);
      }
      if constexpr (RES == 2) {
        const char* const r = P.rcent + (size_t)(v >> ib) * kG12cEB;
        ra[e] = *(const u32x4_a8*)r;
        rb[e] = *(const u32x2_a8*)(r + 16);
      }
    };
    auto gather = [&](const uint32_t (&n)[8]) {
      gather1(0, g12c_elem<0>(n, T, tmask)); gather1(1, g12c_elem<1>(n, T, tmask));
      gather1(2, g12c_elem<2>(n, T, tmask)); gather1(3, g12c_elem<3>(n, T, tmask));
      gather1(4, g12c_elem<4>(n, T, tmask)); gather1(5, g12c_elem<5>(n, T, tmask));
      gather1(6, g12c_elem<6>(n, T, tmask)); gather1(7, g12c_elem<7>(n, T, tmask));
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
        const uint32_t g0 = (uint32_t)(dr * kG12cV + 2 * p), g1 = g0 + 1u;   // outputs 2 p, 2 p + 1 of the row, as outputs of the group
        tile[((g0 >> 4) * kG12cChunks + (uint32_t)dch) * 16u + ((g0 & 15u) ^ wx)] = lo;
        tile[((g1 >> 4) * kG12cChunks + (uint32_t)dch) * 16u + ((g1 & 15u) ^ wx)] = hi;
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
      for (int i = 0; i < 4; ++i) xa[i] = gt_load_a1<false>(nullptr, P.x, xoff, G, t * kG12cTile + (mch0 + i) * 8);
      rebuild(sp, bp, t * kG12cTile + dch * 8 < G);
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
        const bool live = mj < tokens && t * kG12cTile + (mch0 + i) * 8 < G;
        const u32x4 a = {live ? xa[i][0] : 0u, live ? xa[i][1] : 0u, live ? xa[i][2] : 0u, live ? xa[i][3] : 0u};
        const uint32_t slot = (uint32_t)((mch0 + i) * 16) + ((uint32_t)mj ^ (uint32_t)((mch0 + i) & 7));
#pragma unroll
        for (int b = 0; b < 3; ++b) acc[b] = mfma16x16x32<DT>(a, tile[(uint32_t)(b * kG12cChunks * 16) + slot], acc[b]);
      }
    }
    // ---- the 4 waves' partial D of the three N blocks, added in wave order; D element (token = (l >> 4) * 4 + reg, output = l & 15).
    // The raw sums of all 48 outputs go to this part's plane of the partials: lanes 0 - 15 of a token are one 64-byte run
    {
      float* const scr = (float*)g12c_smem;   // [wave][N block][reg][lane]: the tile's first 12 KiB
      __syncthreads();
#pragma unroll
      for (int b = 0; b < 3; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) scr[((wave * 3 + b) * 4 + r) * 64 + lane] = acc[b][r];
      __syncthreads();
      const int r = wave, token = (lane >> 4) * 4 + r;
      float* const prow = Q.partials + ((size_t)part * tokens + (token < tokens ? token : 0)) * Q.op + (size_t)rg * kG12cOut + (lane & 15);
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        float sum = scr[(b * 4 + r) * 64 + lane];
#pragma unroll
        for (int w = 1; w < 4; ++w) sum += scr[((w * 3 + b) * 4 + r) * 64 + lane];
        if (token < tokens) prow[b * 16] = sum;
      }
    }
  }
}

// y[token][o] = sum over the parts in ascending order, + the output bias, one rounding: the parent's epilogue arithmetic
template <typename DT>
__global__ __launch_bounds__(kG12cSumThreads) void gemm_gather12c_sum_kernel(const float* __restrict__ partials, const uint16_t* __restrict__ bias,
                                                                            void* __restrict__ y, int O, int op, int tokens, int S, int out_f32) {
  const int o = blockIdx.x * kG12cSumThreads + threadIdx.x, token = blockIdx.y;
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
// what one call IS: the parent's decision (gemm_gather12_decide: template arguments, index widths, LDS, wgcu) + the split, decided once
// for the launcher, the workspace query and vptq_quant_gemm_gather12c_instance.
// parts > 0 is a request: tpp = ceil(tiles / min(parts, tiles, 16)), S = ceil(tiles / tpp) - every part non-empty, S <= 16.
// parts == 0 is the library's rule, g12c_rule_parts.
// THE RULE AND ITS EVIDENCE (profiles/r38/sweep.md: forced parts 2 / 3 / 4 / 6 / 8 / 14 / 16 on 4096 x 4096, 14336 x 4096, 4096 x 1024, 4096 x
// 14336 and 8192 x 8192 (columns x outputs), v12-k65536-4096 and -0, both dtypes, with and without a permutation, 5 and 16 tokens; one
// MI355X, 256 CUs x 2 = 512 slots).  The starting rule - the smallest S with n_groups x S >= slots - lost everywhere: 4096 x 4096 (86 row
// groups) S = 4 (344 items) 25.0 us against S = 8 (688 items) 22.7; 8192 x 8192 (171) S = 3 (513 items) 75.1 against S = 4 (684) 64.0.  What
// the sweep shows: (a) the SHORTEST parts win as long as the items stay within about 2.5 x the slots - 4096 x 1024: 32.7 / 25.4 / 19.5 /
// 13.6 us at S = 2 / 3 / 4 / 8; 14336 x 4096: 76.6 / 68.0 / 62.0 / 60.5 at S = 2 / 4 / 7 / 14 (1204 items = 2.35 x) - (b) beyond that
// the per-item prologue (a first gather nothing overlaps) and the partials' traffic cost more than balance gains - 8192 x 8192 fp16:
// 64.0 / 70.9 / 68.9 at S = 4 / 8 / 16 (684 / 1368 / 2736 items), 4096 x 14336 (299 row groups): 58.6 / 63.6 at S = 4 / 8 (1196 / 2392) -
// and (c) UNEVEN parts lose to the even split below them: 8 tiles as 3 + 3 + 2 are slower than 4 + 4 in every cell (4096 x 4096: 29.9
// against 27.4), 16 tiles as 5 x 3 + 1 slower than 4 x 4 (75.2 against 64.0).  So: the smallest tiles-per-part that DIVIDES the tile
// count, gives at most 16 parts and keeps n_groups x S <= 2.5 x slots; if no divisor does, the smallest tiles-per-part that keeps the
// bound; if none does (more than 1.25 x slots row groups: the parent kernel's layers), two parts.  On the 80 swept cells the rule's
// choice is the fastest measured split in 77 and within 1.1 % of it in the other 3.
static int g12c_rule_parts(int tiles, int groups, int slots) {
  for (int pass = 0; pass < 2; ++pass)
    for (int tpp = 1; tpp < tiles; ++tpp) {
      const int S = (tiles + tpp - 1) / tpp;
      if (S > kG12cMaxParts || (pass == 0 && tiles % tpp != 0)) continue;
      if (2LL * groups * S <= 5LL * slots) return S;
    }
  return 2;
}

GemmGather12cDecision gemm_gather12c_decide(const VptqLayerDesc& d, int tokens, int parts) {
  GemmGather12cDecision D = {};
  D.base = gemm_gather12_decide(d, tokens);
  const int tiles = D.base.tiles, slots = device_cus() * D.base.wgcu, groups = D.base.n_groups;
  int want = parts;
  if (parts == 0) want = g12c_rule_parts(tiles, groups, slots);
  if (want > kG12cMaxParts) want = kG12cMaxParts;
  if (want > tiles) want = tiles;
  if (want < 1) want = 1;
  D.tpp = (tiles + want - 1) / want;
  D.parts = D.tpp > 0 ? (tiles + D.tpp - 1) / D.tpp : 1;
  D.items = groups * D.parts;
  D.grid = D.items < slots ? D.items : slots;
  D.rgs = D.grid > 0 ? (D.items + D.grid - 1) / D.grid : 0;
  D.op = groups * kG12cOut;
  D.partial_bytes = (size_t)D.parts * tokens * D.op * sizeof(float);
  D.sum_grid_x = (d.out_features + kG12cSumThreads - 1) / kG12cSumThreads;
  D.sum_grid_y = tokens;
  D.serves = parts >= 0 && gemm_gather12_eligible(d, tokens) && D.parts >= 2;
  return D;
}

template <typename DT>
static hipError_t launch_g12c(const GemmGather12cParams& Q, const GemmGather12cDecision& D, hipStream_t st) {
  const dim3 grid(D.grid), block(kGTThreads);
  const int lds = D.base.lds;
  hipError_t e = hipSuccess;
  switch (D.base.res) {
    case 0: hipLaunchKernelGGL((gemm_gather12c_kernel<DT, 0>), grid, block, lds, st, Q); break;
    case 1:   // 48 KiB + the table: past the 64 KiB a kernel may use unasked
      e = allow_dynamic_lds<gemm_gather12c_kernel<DT, 1>>(kG12cTileBytes + kG12cResLdsMax);
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL((gemm_gather12c_kernel<DT, 1>), grid, block, lds, st, Q);
      break;
    case 2: hipLaunchKernelGGL((gemm_gather12c_kernel<DT, 2>), grid, block, lds, st, Q); break;
    default: return hipErrorInvalidValue;
  }
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((gemm_gather12c_sum_kernel<DT>), dim3(D.sum_grid_x, D.sum_grid_y), dim3(kG12cSumThreads), 0, st, Q.partials, Q.g.bias, Q.g.y,
                     Q.g.O, Q.op, Q.g.tokens, Q.S, Q.g.out_f32);
  return hipGetLastError();
}

// d: a layer WITHOUT a permutation (a permuted one as gemm_gather_px_plain(d), x = x[perm]); partials: D.partial_bytes of fp32
hipError_t launch_gemm_gather12c(const VptqLayerDesc& d, const void* x, void* y, int tokens, bool out_f32, int parts, void* partials,
                                 hipStream_t st) {
  const GemmGather12cDecision D = gemm_gather12c_decide(d, tokens, parts);
  if (d.perm || !D.serves || !partials || D.grid < 1 || D.base.lds > kG12cTileBytes + kG12cResLdsMax) return hipErrorInvalidValue;
  GemmGather12cParams Q = {};
  Q.g = gemm_gather_params(d, x, y, tokens, out_f32, D.base.n_groups);
  Q.g.ib = D.base.ib; Q.g.rb = D.base.rb; Q.g.res_bytes = D.base.res_bytes;
  Q.partials = (float*)partials;
  Q.S = D.parts; Q.tpp = D.tpp; Q.n_items = D.items; Q.op = D.op;
  return D.base.f16 ? launch_g12c<F16>(Q, D, st) : launch_g12c<BF16>(Q, D, st);
}

}  // namespace vptq
