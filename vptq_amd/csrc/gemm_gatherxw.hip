// Batched decode for gemm_gatherx.hip's layers (vector length 8 or 16, 16384 ... 65536 main centroids, ANY residual codebook, i.e. any
// total index width T = index_bits + res_bits <= 32 - "v16-k65536-65536 / -32768 / -1024 / -256 / -64 / -0", "v8-k65536-4096 / -4",
// "v8-k32768-0", "v8-k16384-0"), 17 - 48 tokens in ONE launch: TB = 2 / 3 blocks of 16 tokens over gemm_gatherx_kernel's pass.  It is
// to gemm_gatherx.hip what gemm_gatherw.hip is to gemm_gather.hip.
//
// From the 17th token on these layers went through vptq_dequant + a dense GEMM: a dense W rebuilt in HBM on every call.  Here every
// further block of 16 tokens adds its A-operand loads and 8 MFMAs per wave and tile to gemm_gatherx's pass: one index window, one set
// of gathers, one rebuild and one tile write per 1024-column tile, then per K-step one B-operand read from LDS and one
// v_mfma_f32_16x16x32 per token block into that block's own accumulator (the third block: a second round of B reads, below).
//
// Structure: gemm_gatherx.hip's, through the phases of gemm_gather_tile.h:
//  * row group = 16 outputs.  V = 16: ONE vector-row, the two thread halves (tid >> 7) take the two 16-byte halves of the same
//    32-byte entry and read the same index window.  V = 8: two vector-rows.
//  * the ROW-GROUP BODY (run-time T index window of up to 9 words, clamped tail words, v_alignbit_b32 normalisation, gx_elem<E>,
//    need9; gathers of the main entry and of the residual entry: RES = 0 none, 1 from the table copied once per workgroup into the
//    dynamic LDS behind the tile, 2 from L2) is a COPY of gemm_gatherx.hip's: as a shared function it has twice cost 3 - 8 %
//    (profiles/r17) and changed the parent's listings (profiles/r31).  A CHANGE TO IT HERE BELONGS IN gemm_gatherx.hip TOO (and the
//    other way round; gemm_gatherx_grouped.hip holds the third copy).
//  * token blocks: gemm_gatherw.hip's register schedule.  Lane (token mj, k group mkg) of block b reads row 16 b + mj of x, clamped to
//    the last token and masked past it.  Block 0's eight A operands are requested a whole tile ahead and held through the rebuild;
//    block 1's are requested back to back behind the tile write, when the rebuilt weights have left their registers, in front of the
//    next tile's gathers; block 2 (TB = 3) has no registers of its own: when the 8 K-steps of blocks 0 and 1 are done it takes block
//    0's, and the 8 K-steps run again over the same tile (8 more B reads).  Every x load is the uniform base + a 32-bit lane offset
//    (gt_load_a1): one address register per load.
//  * the epilogue runs once per block over the tile's first 4 KiB, gt_epilogue on the block's rows of y.
// There is no form with a permutation: the in-kernel permuted forms of this family were measured at 1.8 - 6.8 times the dense route
// (profiles/r23/table_perm.md).  A permuted layer comes here as gemm_gather_px_plain(d) with x[perm] for x (vptq_quant_gemm_gatherxw
// runs permute_x_tokens in front).
// BIT CONTRACT: the K-step -> wave mapping, the order of the MFMAs into a block's accumulator (tiles in order, steps 0 - 7) and the
// wave-order sum of the epilogue are gemm_gatherx_kernel's for every block: a token's output bits depend neither on its slot nor on
// the batch size, and equal what vptq_quant_gemm_gatherx gives that token in a launch of <= 16 (vptq_quant_gemm_gather_px for a
// layer with a permutation).
// LDS: 32 KiB tile + the table, gemm_gatherx_decide's size and workgroups-per-CU rule.  Registers: held to 2 workgroups per CU (256
// VGPRs) except where that spilled (gxw_min_wg); none of the 24 instantiations has scratch (profiles/r35/listings.md).  No atomics,
// no scratch, no workspace.
// NOT HERE: row groups of 32 outputs, which would halve the x traffic from L2 (gemm_gatherw's open item (a)); a fourth token block
// (49 - 64 tokens); the grouped (sibling) form; the folded / selective arithmetics - the reference's roundings only, like the parent.
#include "gemm_gather_tile.h"

namespace vptq {

// element E (compile time) of T bits (wave uniform) out of the normalised window n[0..7] (gemm_gatherx.hip: gx_elem, a copy - that
// unit's device code is not to change, and a header both include is a change to it)
template <int E>
static __device__ __forceinline__ uint32_t gxw_elem(const uint32_t (&n)[8], int T, uint32_t mask) {
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

// workgroups per CU the register budget is held to: 2 (256 VGPRs), which 16 of the 24 instantiations meet without a spill.  The 8 with
// a residual table AND three token blocks (RES = 1 / 2, TB = 3; both dtypes, both V) spilled 10 - 12 registers there (44 - 52 bytes of
// scratch: the residual entries in flight beside two blocks' A operands) and take what they need: one workgroup per CU
constexpr int gxw_min_wg(int res, int tb) { return res != 0 && tb == 3 ? 1 : 2; }

template <typename DT, int V, int RES, int TB>
__global__ __launch_bounds__(kGTThreads, gxw_min_wg(RES, TB)) void gemm_gatherxw_kernel(const GemmGatherParams P) {
  static_assert(V == 8 || V == 16, "vector length");
  static_assert(RES >= 0 && RES <= 2, "residual: none, LDS, L2");
  static_assert(TB == 2 || TB == 3, "17 - 32 / 33 - 48 tokens");
  constexpr int kRows = 16 / V;   // vector-rows per row group (16 outputs)
  constexpr int EB = V * 2;       // bytes per codebook entry
  extern __shared__ __attribute__((aligned(16))) unsigned char gxw_smem[];
  u32x4* const tile = (u32x4*)gxw_smem;                             // [chunk][16 outputs]: 32 KiB
  const unsigned char* const rtab = gxw_smem + kGTTileBytes;        // RES = 1: the residual table
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int G = P.G, N = P.N, tokens = P.tokens;
  const int T = P.ib + P.rb, ib = P.ib;
  const uint32_t tmask = T >= 32 ? 0xffffffffu : ((1u << T) - 1u), mmask = (1u << ib) - 1u;
  // the 9th window word: 8 T bits + the largest offset (24, 16 or 0 bits: T odd, T % 4 == 2, T % 4 == 0) beyond 8 words (T = 31)
  const bool need9 = 8 * T + ((T & 1) ? 24 : (T & 2) ? 16 : 0) > 256;
  const int last = P.row_words - 1;
  const int n_tiles = (G + kGTTile - 1) / kGTTile;
  if constexpr (RES == 1) {
    const int n16 = P.res_bytes >> 4;
    for (int i = tid; i < n16; i += kGTThreads)
      *(u32x4*)(gxw_smem + kGTTileBytes + (size_t)i * 16) = *(const u32x4*)(P.rcent + (size_t)i * 16);
    __syncthreads();
  }
  // dequant role: 8 consecutive columns (chunk dch) of 8 outputs: V = 8 vector-row dr of the group, V = 16 half dr of its one entry
  const int dr = tid >> 7, dch = tid & (kGTChunks - 1);
  const uint32_t hoff = V == 16 ? (uint32_t)dr * 16u : 0u;
  const uint32_t wslot = (uint32_t)(dch * 16 + dr * 8), wx = (uint32_t)(dch & 7);
  // MFMA role: lane (token / output mj, k group mkg); step i reads chunk 32 wave + 8 mkg + i
  const int mj = lane & 15, mkg = lane >> 4;
  const int mch0 = wave * 32 + mkg * 8;
  // block b's row of x, 16 b + mj clamped to the last token, as a byte offset (gt_load_a1); block 0 is whole: 16 < tokens
  uint32_t xoff[TB];
  bool tok_b[TB];
#pragma unroll
  for (int b = 0; b < TB; ++b) {
    const int tk = 16 * b + mj;
    tok_b[b] = tk < tokens;
    xoff[b] = (uint32_t)(tk < tokens ? tk : tokens - 1) * (uint32_t)G * 2u;
  }

  for (int rg = blockIdx.x; rg < P.n_groups; rg += gridDim.x) {
    // ---- the row-group body: gemm_gatherx.hip's (see the head of the file)
    const int row = V == 16 ? rg : rg * kRows + dr;
    const uint32_t* const irow = P.idx + (size_t)(row < N ? row : N - 1) * P.row_words;
    auto dcol = [&](int t) { return gt_dcol(t, dch, G); };
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
    u32x4 cv[8], rv[RES ? 8 : 1];
    auto gather1 = [&](int e, uint32_t v) {
      cv[e] = *(const u32x4*)(P.cent + (size_t)(v & mmask) * EB + hoff);
      if constexpr (RES == 1) rv[e] = *(const u32x4*)(rtab + (v >> ib) * (uint32_t)EB + hoff);
      if constexpr (RES == 2) rv[e] = *(const u32x4*)(P.rcent + (size_t)(v >> ib) * EB + hoff);
    };
    auto gather = [&](const uint32_t (&n)[8]) {
      gather1(0, gxw_elem<0>(n, T, tmask)); gather1(1, gxw_elem<1>(n, T, tmask));
      gather1(2, gxw_elem<2>(n, T, tmask)); gather1(3, gxw_elem<3>(n, T, tmask));
      gather1(4, gxw_elem<4>(n, T, tmask)); gather1(5, gxw_elem<5>(n, T, tmask));
      gather1(6, gxw_elem<6>(n, T, tmask)); gather1(7, gxw_elem<7>(n, T, tmask));
    };
    uint32_t wq[8], sp[4], bp[4], sp_next[4], bp_next[4];
    load_idx(0, wq);
    gt_load_sb(P, dcol(0), sp, bp);
    gather(wq);
    load_idx(1, wq);
    gt_load_sb(P, dcol(1), sp_next, bp_next);
    f32x4 acc[TB];
#pragma unroll
    for (int b = 0; b < TB; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int t = 0; t < n_tiles; ++t) {
      // ---- block 0's A operands, a whole tile ahead (gemm_gatherx's gt_load_a in gt_load_a1's addressing)
      u32x4 xa[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) xa[i] = gt_load_a1<false>(nullptr, P.x, xoff[0], G, t * kGTTile + (mch0 + i) * 8);
      gt_rebuild<DT, RES != 0>(cv, rv, sp, bp, t * kGTTile + dch * 8 < G);
      __syncthreads();   // the previous tile's MFMA reads (and the previous row group's sums) are done
      gt_write_tile(tile, wslot, wx, cv);
      // ---- block 1's A operands, whole and back to back, in front of the gathers
      u32x4 xb[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) xb[i] = gt_load_a1<false>(nullptr, P.x, xoff[1], G, t * kGTTile + (mch0 + i) * 8);
      // ---- the next tile's gathers fly during the MFMA phase; the index window and scale / bias of the one after follow
      if (t + 1 < n_tiles) {
        gather(wq);
#pragma unroll
        for (int q = 0; q < 4; ++q) { sp[q] = sp_next[q]; bp[q] = bp_next[q]; }
        load_idx(t + 2, wq);
        gt_load_sb(P, dcol(t + 2), sp_next, bp_next);
      }
      __syncthreads();   // tile complete
      // ---- this wave's 8 K-steps: the B operand once, one MFMA each for blocks 0 and 1
      auto masked = [](const u32x4& v, bool live) { return u32x4{live ? v[0] : 0u, live ? v[1] : 0u, live ? v[2] : 0u, live ? v[3] : 0u}; };
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const bool kin = t * kGTTile + (mch0 + i) * 8 < G;
        const u32x4 b = tile[(mch0 + i) * 16 + (mj ^ i)];   // ((mch0 + i) & 7 == i)
        acc[0] = mfma16x16x32<DT>(masked(xa[i], kin), b, acc[0]);
        acc[1] = mfma16x16x32<DT>(masked(xb[i], kin && tok_b[1]), b, acc[1]);
      }
      if constexpr (TB == 3) {
        // ---- block 2 takes block 0's registers: its 8 loads back to back, then the 8 K-steps again over the same tile
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 8; ++i) xa[i] = gt_load_a1<false>(nullptr, P.x, xoff[2], G, t * kGTTile + (mch0 + i) * 8);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const bool kin = t * kGTTile + (mch0 + i) * 8 < G;
          const u32x4 b = tile[(mch0 + i) * 16 + (mj ^ i)];
          acc[2] = mfma16x16x32<DT>(masked(xa[i], kin && tok_b[2]), b, acc[2]);
        }
      }
    }
    // ---- one epilogue per block, on the block's rows of y (gt_epilogue's first barrier also ends the reads of the block before)
#pragma unroll
    for (int b = 0; b < TB; ++b) {
      GemmGatherParams Pb = P;
      Pb.tokens = tokens - 16 * b;
      Pb.y = (char*)P.y + (size_t)(16 * b) * P.O * (P.out_f32 ? 4 : 2);
      gt_epilogue<DT>(Pb, tid, lane, wave, (float*)gxw_smem, rg, acc[b]);
    }
  }
}

// ---- host side -------------------------------------------------------------------
bool gemm_gatherxw_eligible(const VptqLayerDesc& d, int tokens) {
  return tokens >= 17 && tokens <= 48 && gemm_gatherx_eligible(d, 16);   // gemm_gatherx's layers
}

// what one launch IS: the template arguments of gemm_gatherxw_kernel<DT, V, RES, TB>, the run-time index widths and the launch
// shape, decided once for the launcher and for vptq_quant_gemm_gatherxw_instance.  Format, LDS and workgroups per CU are
// gemm_gatherx_decide's
GemmGatherXWDecision gemm_gatherxw_decide(const VptqLayerDesc& d, int tokens) {
  const GemmGatherXDecision S = gemm_gatherx_decide(d, 16);
  GemmGatherXWDecision D = {};
  D.f16 = S.f16;
  D.v = S.v; D.ib = S.ib; D.rb = S.rb; D.res = S.res; D.res_bytes = S.res_bytes;
  D.tok = tokens;
  D.tb = (tokens + 15) / 16;
  D.tiles = S.tiles; D.lds = S.lds; D.wgcu = S.wgcu;
  D.n_groups = S.n_groups; D.grid = S.grid; D.rgs = S.rgs;
  return D;
}

template <typename DT, int V, int RES>
static hipError_t launch_gxw(const GemmGatherParams& P, const GemmGatherXWDecision& D, hipStream_t st) {
  const dim3 grid(D.grid), block(kGTThreads);
  if (D.tb == 2) hipLaunchKernelGGL((gemm_gatherxw_kernel<DT, V, RES, 2>), grid, block, D.lds, st, P);
  else hipLaunchKernelGGL((gemm_gatherxw_kernel<DT, V, RES, 3>), grid, block, D.lds, st, P);
  return hipGetLastError();
}

template <typename DT, int V>
static hipError_t launch_gxw_v(const GemmGatherParams& P, const GemmGatherXWDecision& D, hipStream_t st) {
  switch (D.res) {
    case 0: return launch_gxw<DT, V, 0>(P, D, st);
    case 1: return launch_gxw<DT, V, 1>(P, D, st);
    case 2: return launch_gxw<DT, V, 2>(P, D, st);
    default: return hipErrorInvalidValue;
  }
}

template <typename DT>
static hipError_t launch_gxw_dt(const GemmGatherParams& P, const GemmGatherXWDecision& D, hipStream_t st) {
  switch (D.v) {
    case 8: return launch_gxw_v<DT, 8>(P, D, st);
    case 16: return launch_gxw_v<DT, 16>(P, D, st);
    default: return hipErrorInvalidValue;
  }
}

// d: a layer WITHOUT a permutation (a permuted one as gemm_gather_px_plain(d), x = x[perm])
hipError_t launch_gemm_gatherxw(const VptqLayerDesc& d, const void* x, void* y, int tokens, bool out_f32, hipStream_t st) {
  const GemmGatherXWDecision D = gemm_gatherxw_decide(d, tokens);
  if (d.perm || D.grid < 1 || tokens < 17 || tokens > 48 || D.tb < 2 || D.tb > 3 || D.lds > 65536) return hipErrorInvalidValue;
  GemmGatherParams P = gemm_gather_params(d, x, y, tokens, out_f32, D.n_groups);
  P.ib = D.ib; P.rb = D.rb; P.res_bytes = D.res_bytes;   // (the table copied into LDS is the one D.lds has room for)
  return D.f16 ? launch_gxw_dt<F16>(P, D, st) : launch_gxw_dt<BF16>(P, D, st);
}

}  // namespace vptq
