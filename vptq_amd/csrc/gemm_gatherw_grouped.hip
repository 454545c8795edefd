// Batched decode of SIBLING layers (q / k / v, gate / up) of the large-codebook VPTQ formats (gemm_gather.hip's layers: v = 8, k = 65536
// main centroids; residual: none, 256 or 65536), 17 - 48 tokens in ONE launch: gemm_gatherw_kernel's pass (gemm_gatherw.hip: TB = 2 / 3
// blocks of 16 tokens over one index read, one set of gathers, one rebuild and one tile write per 1024-column tile) behind
// gemm_gather_grouped_kernel's member walk (gemm_gather.hip: the row-group lists of up to 4 layers, concatenated).
//
// From the 17th token on every member of such a group went out alone - gemm_gatherw, gemm_gather_px (a permute launch, then gemm_gatherw)
// or vptq_dequant + a dense GEMM, whichever its size gave it.  Here the members' row groups are one list, walked by min(total row
// groups, CUs x 4) workgroups.  Plain form only: a member with a column permutation arrives as its descriptor without one and x[perm]
// for its x (one x gather per DISTINCT permutation: the caller's, vptq_quant_gemm_gatherw_grouped).
// BIT CONTRACT: a row group does not depend on the grid, so member m's row group rg has the bits gemm_gatherw_kernel<DT, T, false, TB>
// gives it in the member's own launch at the same token count - and through that kernel's contract a token's bits are the 16-token
// kernel's in any slot of any batch.
// 36 KiB of LDS at most, as gemm_gatherw.  No workspace of its own, no atomics.
#include "gemm_gather_tile.h"

namespace vptq {

constexpr int kWGRows = 2;                        // vector-rows per row group (16 outputs): gemm_gatherw's
constexpr int kWGWgPerCu = 4;                     // gemm_gatherw's kWWgPerCu
constexpr int kWGMembers = 4;

struct GemmGatherWGroupedParams {
  GemmGatherParams m[kWGMembers];
  int first_group[kWGMembers + 1];   // member m owns the global row groups [first_group[m], first_group[m + 1])
  int n_groups, n;
};

// one row group of one member: the row-group body of gemm_gatherw_kernel<DT, T, false, TB> (gemm_gatherw.hip), statement for statement.
// A copy, not a function both kernels share: a shared body gave the existing instantiations of the single kernels other instructions
// (profiles/r31/listings.md, "shared body"), and their device code is not to change.  A change to one copy belongs in the other.
// xoff / tok_b: block b's row of x as a byte offset and whether lane mj's token of block b is live - the member's, set at the switch.
template <typename DT, int T, int TB>
static __device__ __forceinline__ void gwg_row_group(const GemmGatherParams& P, u32x4* tile, const u32x4* rtab, const uint32_t (&xoff)[TB],
                                                     const bool (&tok_b)[TB], int rg) {
  static_assert(TB == 2 || TB == 3, "17 - 32 / 33 - 48 tokens");
  constexpr int NW = T / 4;   // index words of 8 elements
  constexpr bool RES = T > 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int G = P.G, N = P.N, tokens = P.tokens;
  const int n_tiles = (G + kGTTile - 1) / kGTTile;
  // dequant role: 8 consecutive columns (chunk dch) of vector-row dr of the group
  const int dr = tid >> 7, dch = tid & (kGTChunks - 1);
  const uint32_t wslot = (uint32_t)(dch * 16 + dr * 8), wx = (uint32_t)(dch & 7);
  // MFMA role: lane (token / output mj, k group mkg); step i reads chunk 32 wave + 8 mkg + i
  const int mj = lane & 15, mkg = lane >> 4;
  const int mch0 = wave * 32 + mkg * 8;

  const int row = rg * kWGRows + dr;
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
    u32x4 xa[8];   // block 0: held a tile ahead, through the rebuild
#pragma unroll
    for (int i = 0; i < 8; ++i) xa[i] = gt_load_a1<false>(nullptr, P.x, xoff[0], G, t * kGTTile + (mch0 + i) * 8);
    gt_rebuild<DT, RES>(cv, rv, sp, bp, t * kGTTile + dch * 8 < G);
    __syncthreads();   // the previous tile's MFMA reads (and the previous row group's sums) are done
    gt_write_tile(tile, wslot, wx, cv);
    // ---- block 1's A operands, whole and back to back, in front of the gathers
    u32x4 xb[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) xb[i] = gt_load_a1<false>(nullptr, P.x, xoff[1], G, t * kGTTile + (mch0 + i) * 8);
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
    gt_epilogue<DT>(Pb, tid, lane, wave, (float*)tile, rg, acc[b]);
  }
}

// A workgroup walks the global row groups g = blockIdx.x, + gridDim.x, ...: g rises, so the member never falls - the members are
// visited in order, and a member's state (its argument block, the per-block x offsets, T = 24: its residual table in LDS) is set up at
// the switch.  (gemm_gather_grouped_kernel's walk.)
template <typename DT, int T, int TB>
__global__ __launch_bounds__(kGTThreads, 2) void gemm_gatherw_grouped_kernel(const GemmGatherWGroupedParams GP) {
  __shared__ __attribute__((aligned(16))) u32x4 tile[kGTChunks * 16];   // [chunk][16 outputs]: 32 KiB
  __shared__ u32x4 rtab[T == 24 ? 256 : 1];
  const int tid = threadIdx.x, mj = tid & 15;
  int g = blockIdx.x;
#pragma unroll 1
  for (int m = 0; m < GP.n; ++m) {
    const int first = GP.first_group[m], end = GP.first_group[m + 1];
    if (g >= end) continue;   // (uniform: g is the workgroup's)
    const GemmGatherParams P = GP.m[m];
    // block b's row of x, 16 b + mj clamped to the last token, as a byte offset (gt_load_a1); block 0 is whole: 16 < tokens
    uint32_t xoff[TB];
    bool tok_b[TB];
#pragma unroll
    for (int b = 0; b < TB; ++b) {
      const int tk = 16 * b + mj;
      tok_b[b] = tk < P.tokens;
      xoff[b] = (uint32_t)(tk < P.tokens ? tk : P.tokens - 1) * (uint32_t)P.G * 2u;
    }
    if constexpr (T == 24) {
      __syncthreads();   // the other waves' table reads of the previous member's last row group are done
      rtab[tid] = *(const u32x4*)(P.rcent + (size_t)tid * 16);   // kGTThreads == 256 entries
      __syncthreads();
    }
#pragma unroll 1
    for (; g < end; g += gridDim.x) gwg_row_group<DT, T, TB>(P, tile, rtab, xoff, tok_b, g - first);
  }
}

// ---- host side -------------------------------------------------------------------
// what one grouped launch IS: the template arguments of gemm_gatherw_grouped_kernel<DT, T, TB>, every member's row groups and the
// launch shape, decided once for the launcher and for vptq_quant_gemm_gatherw_grouped_instance.  The members share dtype, width and T
// (the caller's check): dt, T and tiles are the first member's
GemmGatherWGroupedDecision gemm_gatherw_grouped_decide(const VptqLayerDesc* descs, int n, int tokens) {
  GemmGatherWGroupedDecision D = {};
  if (n < 1 || n > kWGMembers) return D;
  D.f16 = descs[0].dtype == VPTQ_DTYPE_F16;
  D.T = descs[0].num_res_centroids == 0 ? 16 : descs[0].num_res_centroids == 256 ? 24 : 32;
  D.tok = tokens;
  D.tb = (tokens + 15) / 16;
  D.n = n;
  D.tiles = (descs[0].group_size + kGTTile - 1) / kGTTile;
  for (int m = 0; m < n; ++m) {
    D.groups[m] = (descs[m].num_indices + kWGRows - 1) / kWGRows;
    D.first_group[m + 1] = D.first_group[m] + D.groups[m];
  }
  D.total = D.first_group[n];
  const int slots = device_cus() * kWGWgPerCu;
  D.grid = D.total < slots ? D.total : slots;
  D.rgs = D.grid > 0 ? (D.total + D.grid - 1) / D.grid : 0;
  return D;
}

template <typename DT, int T>
static hipError_t launch_gwg_t(const GemmGatherWGroupedParams& GP, const GemmGatherWGroupedDecision& D, hipStream_t st) {
  const dim3 grid(D.grid), block(kGTThreads);
  if (D.tb == 2) hipLaunchKernelGGL((gemm_gatherw_grouped_kernel<DT, T, 2>), grid, block, 0, st, GP);
  else hipLaunchKernelGGL((gemm_gatherw_grouped_kernel<DT, T, 3>), grid, block, 0, st, GP);
  return hipGetLastError();
}

template <typename DT>
static hipError_t launch_gwg_dt(const GemmGatherWGroupedParams& GP, const GemmGatherWGroupedDecision& D, hipStream_t st) {
  switch (D.T) {
    case 16: return launch_gwg_t<DT, 16>(GP, D, st);
    case 24: return launch_gwg_t<DT, 24>(GP, D, st);
    case 32: return launch_gwg_t<DT, 32>(GP, D, st);
    default: return hipErrorInvalidValue;
  }
}

// descs: the members WITHOUT a permutation (a permuted member as its plain form); x[m]: member m's activations in its own column order
hipError_t launch_gemm_gatherw_grouped(const VptqLayerDesc* descs, int n, const void* const* x, void* const* y, int tokens, bool out_f32,
                                       hipStream_t st) {
  const GemmGatherWGroupedDecision D = gemm_gatherw_grouped_decide(descs, n, tokens);
  if (D.n < 2 || D.grid < 1 || tokens < 17 || tokens > 48 || D.tb < 2 || D.tb > 3) return hipErrorInvalidValue;
  GemmGatherWGroupedParams GP = {};
  for (int m = 0; m < n; ++m) {
    if (descs[m].perm || !x[m] || !y[m]) return hipErrorInvalidValue;
    GP.m[m] = gemm_gather_params(descs[m], x[m], y[m], tokens, out_f32, D.groups[m]);
    GP.first_group[m] = D.first_group[m];
  }
  for (int m = n; m <= kWGMembers; ++m) GP.first_group[m] = D.total;
  GP.n_groups = D.total;
  GP.n = n;
  return D.f16 ? launch_gwg_dt<F16>(GP, D, st) : launch_gwg_dt<BF16>(GP, D, st);
}

}  // namespace vptq
