// Batched decode for the large-codebook VPTQ formats (gemm_gather.hip's layers: v = 8, k = 65536 main centroids; residual: none, 256
// or 65536), 17 - 48 tokens in ONE launch: TB = 2 / 3 blocks of 16 tokens over gemm_gather_kernel's pass.
//
// gemm_gather pays the index read, the gathers, the three-rounding rebuild and the tile write once per 1024-column tile whatever the
// token count; from the 17th token on these layers went through vptq_dequant + a dense GEMM.  Here every further block of 16 tokens
// adds its A-operand loads and 8 MFMAs per wave and tile to that pass: one index read, one set of gathers, one rebuild and one tile
// write per tile, then per K-step one B-operand read from LDS and one MFMA per token block into that block's own accumulator
// (the third block: a second round of B reads, below).
//
// Structure: gemm_gather.hip's, through the phases of gemm_gather_tile.h (same row groups, thread roles, index path, loop skeleton
// and barriers).  This file's own:
//  * lane (token mj, k group mkg) of block b reads row 16 b + mj of x, clamped to the last token and masked past it.
//  * registers: gemm_gather holds one block's A operands (32 VGPRs) a whole tile ahead, through the rebuild; block 0 is held that
//    way here.  Block 1's are requested behind the tile write, when the rebuilt weights have left their registers, in front of the
//    next tile's gathers - waiting for them does not wait for a gather.  Block 2 (TB = 3) has no registers of its own: when the 8
//    K-steps of blocks 0 and 1 are done it takes block 0's, and the 8 K-steps run again over the same tile (8 more B reads).
//    A block's 8 loads are always issued back to back: a lane's 8 steps are the 8 16-byte pieces of ONE 128-byte line of x,
//    and the gathers sweep the L1 between two requests that are a K-step apart.  (First version: a ring of 2 - 4 K-steps per later
//    block, refilled step by step - 86 / 107 / 113 us per 8192 x 8192 v8-k65536-256 fp16 layer at 33 / 40 / 48 tokens, now 77 / 82 / 86:
//    profiles/r23/README.md.)  x is at most 48 rows and L2-resident.  Every x load is the uniform base + a 32-bit lane offset
//    (gt_load_a1; block 0 too): one address register per load.
//  * the epilogue runs once per block over the tile's first 4 KiB, gt_epilogue on the block's rows of y.
// BIT CONTRACT: the K-step -> wave mapping, the order of the MFMAs into a block's accumulator (tiles in order, steps 0 - 7) and the
// wave-order sum of the epilogue are gemm_gather_kernel's for every block: a token's output bits depend neither on its slot nor on
// the batch size, and equal what gemm_gather_kernel gives that token in a launch of <= 16.
// 36 KiB of LDS at most, as gemm_gather.  No workspace, no atomics.
#include "gemm_gather_tile.h"

namespace vptq {

constexpr int kWRows = 2;                         // vector-rows per row group (16 outputs): gemm_gather's
constexpr int kWWgPerCu = 4;
// workgroups per CU the register budget is held to: 2 (256 VGPRs), which every form without a permutation meets without a spill; the
// permuted forms (8 x 8 scalar activation loads per lane, block and tile) do not, and take what they need: one workgroup per CU
constexpr int gw_min_wg(bool perm) { return perm ? 1 : 2; }

template <typename DT, int T, bool PERM, int TB>
__global__ __launch_bounds__(kGTThreads, gw_min_wg(PERM)) void gemm_gatherw_kernel(const GemmGatherParams P) {
  static_assert(TB == 2 || TB == 3, "17 - 32 / 33 - 48 tokens");
  constexpr int NW = T / 4;   // index words of 8 elements
  constexpr bool RES = T > 16;
  __shared__ __attribute__((aligned(16))) u32x4 tile[kGTChunks * 16];   // [chunk][16 outputs]: 32 KiB
  __shared__ u32x4 rtab[T == 24 ? 256 : 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int G = P.G, N = P.N, tokens = P.tokens;
  const int n_tiles = (G + kGTTile - 1) / kGTTile;
  if constexpr (T == 24) {
    rtab[tid] = *(const u32x4*)(P.rcent + (size_t)tid * 16);   // kGTThreads == 256 entries
    __syncthreads();
  }
  // dequant role: 8 consecutive columns (chunk dch) of vector-row dr of the group
  const int dr = tid >> 7, dch = tid & (kGTChunks - 1);
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
    const int row = rg * kWRows + dr;
    const uint32_t* const irow = P.idx + (size_t)(row < N ? row : N - 1) * P.row_words;
    auto dcol = [&](int t) { return gt_dcol(t, dch, G); };
    auto load_idx = [&](int t, uint32_t (&w)[NW]) {
      // (one wide coalesced load: a chunk's words are 16- (T = 16), 8- (24) or 32-byte (32) aligned - the host's checks)
      const uint32_t* src = irow + (size_t)(dcol(t) >> 3) * NW;
      if constexpr (T == 24) {
#pragma unroll
        for (int q = 0; q < 3; ++q) { const u32x2 v = ((const u32x2*)src)[q]; w[2 * q] = v[0]; w[2 * q + 1] = v[1]; }
      } else {
#pragma unroll
        for (int q = 0; q < NW / 4; ++q) {
          const u32x4 v = ((const u32x4*)src)[q];
#pragma unroll
          for (int j = 0; j < 4; ++j) w[4 * q + j] = v[j];
        }
      }
    };
    u32x4 cv[8], rv[RES ? 8 : 1];
    auto gather = [&](const uint32_t (&w)[NW]) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const uint32_t v = packed_elem<T>(w, e);
        cv[e] = *(const u32x4*)(P.cent + (size_t)(v & 0xffffu) * 16);
        if constexpr (T == 24) rv[e] = rtab[(v >> 16) & 0xffu];
        if constexpr (T == 32) rv[e] = *(const u32x4*)(P.rcent + (size_t)(v >> 16) * 16);
      }
    };
    uint32_t wq[NW], sp[4], bp[4], sp_next[4], bp_next[4];
    load_idx(0, wq);
    gt_load_sb(P, dcol(0), sp, bp);
    gather(wq);
    load_idx(1, wq);
    gt_load_sb(P, dcol(1), sp_next, bp_next);
    f32x4 acc[TB];
#pragma unroll
    for (int b = 0; b < TB; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int t = 0; t < n_tiles; ++t) {
      u32x4 xa[8];   // block 0: gt_load_a in gt_load_a1's addressing
#pragma unroll
      for (int i = 0; i < 8; ++i) xa[i] = gt_load_a1<PERM>(P.perm, P.x, xoff[0], G, t * kGTTile + (mch0 + i) * 8);
      gt_rebuild<DT, RES>(cv, rv, sp, bp, t * kGTTile + dch * 8 < G);
      __syncthreads();   // the previous tile's MFMA reads (and the previous row group's sums) are done
      gt_write_tile(tile, wslot, wx, cv);
      // ---- block 1's A operands, whole and back to back, in front of the gathers
      u32x4 xb[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) xb[i] = gt_load_a1<PERM>(P.perm, P.x, xoff[1], G, t * kGTTile + (mch0 + i) * 8);
      // ---- the next tile's gathers fly during the MFMA phase; the index words and scale / bias of the one after follow
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
        for (int i = 0; i < 8; ++i) xa[i] = gt_load_a1<PERM>(P.perm, P.x, xoff[2], G, t * kGTTile + (mch0 + i) * 8);
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
      gt_epilogue<DT>(Pb, tid, lane, wave, (float*)tile, rg, acc[b]);
    }
  }
}

// ---- host side -------------------------------------------------------------------
bool gemm_gatherw_eligible(const VptqLayerDesc& d, int tokens) {
  return tokens >= 17 && tokens <= 48 && gemm_gather_eligible(d, 16);   // gemm_gather's layers
}

// what one launch IS: the template arguments of gemm_gatherw_kernel<DT, T, PERM, TB> and the launch shape, decided once for the
// launcher and for vptq_quant_gemm_gatherw_instance
GemmGatherWDecision gemm_gatherw_decide(const VptqLayerDesc& d, int tokens) {
  GemmGatherWDecision D = {};
  D.f16 = d.dtype == VPTQ_DTYPE_F16;
  D.perm = d.perm != nullptr;
  D.T = d.num_res_centroids == 0 ? 16 : d.num_res_centroids == 256 ? 24 : 32;
  D.tok = tokens;
  D.tb = (tokens + 15) / 16;
  D.tiles = (d.group_size + kGTTile - 1) / kGTTile;
  const GemmGatherGrid g = gemm_gather_grid(d.num_indices, kWRows, kWWgPerCu);
  D.n_groups = g.n_groups; D.grid = g.grid; D.rgs = g.rgs;
  return D;
}

template <typename DT, int T, int TB>
static hipError_t launch_gw(const GemmGatherParams& P, const GemmGatherWDecision& D, hipStream_t st) {
  const dim3 grid(D.grid), block(kGTThreads);
  if (D.perm) hipLaunchKernelGGL((gemm_gatherw_kernel<DT, T, true, TB>), grid, block, 0, st, P);
  else hipLaunchKernelGGL((gemm_gatherw_kernel<DT, T, false, TB>), grid, block, 0, st, P);
  return hipGetLastError();
}

template <typename DT, int TB>
static hipError_t launch_gw_t(const GemmGatherParams& P, const GemmGatherWDecision& D, hipStream_t st) {
  switch (D.T) {
    case 16: return launch_gw<DT, 16, TB>(P, D, st);
    case 24: return launch_gw<DT, 24, TB>(P, D, st);
    case 32: return launch_gw<DT, 32, TB>(P, D, st);
    default: return hipErrorInvalidValue;
  }
}

template <typename DT>
static hipError_t launch_gw_dt(const GemmGatherParams& P, const GemmGatherWDecision& D, hipStream_t st) {
  return D.tb == 2 ? launch_gw_t<DT, 2>(P, D, st) : launch_gw_t<DT, 3>(P, D, st);
}

hipError_t launch_gemm_gatherw(const VptqLayerDesc& d, const void* x, void* y, int tokens, bool out_f32, hipStream_t st) {
  const GemmGatherWDecision D = gemm_gatherw_decide(d, tokens);
  if (D.grid < 1 || tokens < 17 || tokens > 48 || D.tb < 2 || D.tb > 3) return hipErrorInvalidValue;
  const GemmGatherParams P = gemm_gather_params(d, x, y, tokens, out_f32, D.n_groups);
  return D.f16 ? launch_gw_dt<F16>(P, D, st) : launch_gw_dt<BF16>(P, D, st);
}

}  // namespace vptq
