// Batched decode of SIBLING layers (q / k / v, gate / up) of the large-codebook VPTQ formats gemm_gatherx.hip serves (vector length 8 or
// 16, 16384 ... 65536 main centroids, any residual codebook: "v16-k65536-65536 / -32768 / -1024 / -256 / -64 / -0", "v8-k65536-4096 / -4",
// "v8-k32768-0", "v8-k16384-0"), 17 - 48 tokens in ONE launch: gemm_gatherxw_kernel's token-block pass (gemm_gatherxw.hip: TB = 2 / 3
// blocks of 16 tokens over one index window, one set of gathers, one rebuild and one tile write per 1024-column tile) behind
// gemm_gatherx_grouped_kernel's member walk (gemm_gatherx_grouped.hip: the row-group lists of up to 4 layers, concatenated, the
// member's residual table re-staged in LDS at a member switch).
//
// From the 17th token on every member of such a group went out alone - gemm_gatherxw (behind a permute launch of its own when
// permuted) or vptq_dequant + a dense GEMM, whichever its size gave it - and k / v of the 8B shapes alone (64 row groups) occupy a
// quarter of the CUs.  Here the members' row groups are one list.  Plain form only: a member with a column permutation arrives as its
// descriptor without one and x[perm] for its x (one x gather per DISTINCT permutation: the caller's, vptq_quant_gemm_gatherxw_grouped).
//
// What is the LAUNCH's and what is a MEMBER's: the members share dtype, input width, format and token count (the caller's check), so
// the index widths and masks, need9, the tile count and the per-block x offsets and token masks (GxwgLaunch) are computed once per
// workgroup, in front of the walk; a member switch takes the member's argument block (GemmGatherParams, wave uniform: it is read
// through a uniform member index and stays in scalar registers - the row-group body sits at 215 - 251 VGPRs) and, RES = 1, copies the
// member's residual table into the dynamic LDS behind the tile between two barriers.
//  * the ROW-GROUP BODY (run-time T index window of up to 9 words, clamped tail words, v_alignbit_b32 normalisation, gxwg_elem<E>,
//    need9; gathers of the main entry and of the residual entry; gemm_gatherw's register schedule for the token blocks: block 0's
//    eight A operands a tile ahead, block 1's back to back behind the tile write, block 2 (TB = 3) in block 0's registers for a second
//    round of the 8 K-steps over the same tile; one epilogue per block) is a COPY of gemm_gatherxw.hip's, the fourth of the family
//    (gemm_gatherx.hip, gemm_gatherx_grouped.hip, gemm_gatherxw.hip): as a shared function it has twice cost 3 - 8 % (profiles/r17) and
//    changed the single kernels' listings (profiles/r31).  A CHANGE TO IT HERE BELONGS IN THE OTHER THREE, and the other way round.
// BIT CONTRACT: a row group depends neither on the grid nor on the workgroup that runs it; within a block the K-step -> wave mapping,
// the order of the MFMAs into the block's accumulator (tiles in order, steps 0 - 7) and the wave-order sum of the epilogue are
// gemm_gatherxw_kernel's.  Member m's y has the bits vptq_quant_gemm_gatherxw gives on the member's own descriptor, the same x and the
// same token count.
// LDS: 32 KiB tile + the table, gemm_gatherx_decide's size.  Registers: held to 2 workgroups per CU (256 VGPRs) except where that
// spilled (gxwg_min_wg); none of the 24 instantiations has scratch (profiles/r36/listings.md).  GRID: min(total row groups, CUs x W),
// W the workgroups per CU that are RESIDENT - the smaller of the LDS bound (gemm_gatherx_decide's wgcu) and the register bound - so
// that no workgroup waits for a slot while the resident ones walk on.  No atomics, no scratch, no workspace of its own.
// NOT HERE: row groups of 32 outputs; a fourth token block (49 - 64 tokens); groups whose members differ in format; the folded /
// selective arithmetics - the reference's roundings only, like the parents.
#include "gemm_gather_tile.h"

namespace vptq {

constexpr int kGXWGMembers = 4;

struct GemmGatherXWGroupedParams {
  GemmGatherParams m[kGXWGMembers];
  int first_group[kGXWGMembers + 1];   // member m owns the global row groups [first_group[m], first_group[m + 1])
  int n_groups, n;
};

// what every member of a launch shares, computed once per workgroup (per lane: xoff / tok_b)
template <int TB>
struct GxwgLaunch {
  int T, ib, n_tiles;
  uint32_t tmask, mmask;
  bool need9;
  uint32_t xoff[TB];   // block b's row of x, 16 b + mj clamped to the last token, as a byte offset (gt_load_a1)
  bool tok_b[TB];      // is lane mj's token of block b live?
};

// element E (compile time) of T bits (wave uniform) out of the normalised window n[0..7] (gemm_gatherx.hip: gx_elem, a copy - that
// unit's device code is not to change, and a header both include is a change to it)
template <int E>
static __device__ __forceinline__ uint32_t gxwg_elem(const uint32_t (&n)[8], int T, uint32_t mask) {
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

// workgroups per CU the register budget is held to: gemm_gatherxw's rule (gxw_min_wg).  2 (256 VGPRs) where the instantiation fits
// without a spill; the 8 with a residual table AND three token blocks (the residual entries in flight beside two blocks' A operands)
// take one workgroup per CU.  The host's grid reads the same rule (gemm_gatherxw_grouped_decide)
constexpr int gxwg_min_wg(int res, int tb) { return res != 0 && tb == 3 ? 1 : 2; }

// one row group of one member: the row-group body of gemm_gatherxw_kernel<DT, V, RES, TB> (gemm_gatherxw.hip), statement for
// statement, with the launch's shared state handed in (L) instead of recomputed.  smem: the tile, behind it (RES = 1) the member's
// residual table, staged at the switch.
template <typename DT, int V, int RES, int TB>
static __device__ __forceinline__ void gxwg_row_group(const GemmGatherParams& P, const GxwgLaunch<TB>& L, unsigned char* smem, int rg) {
  constexpr int kRows = 16 / V;   // vector-rows per row group (16 outputs)
  constexpr int EB = V * 2;       // bytes per codebook entry
  u32x4* const tile = (u32x4*)smem;                              // [chunk][16 outputs]: 32 KiB
  const unsigned char* const rtab = smem + kGTTileBytes;         // RES = 1: the residual table
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int G = P.G, N = P.N, tokens = P.tokens;
  const int T = L.T, ib = L.ib;
  const uint32_t tmask = L.tmask, mmask = L.mmask;
  const bool need9 = L.need9;
  const int last = P.row_words - 1;
  const int n_tiles = L.n_tiles;
  // dequant role: 8 consecutive columns (chunk dch) of 8 outputs: V = 8 vector-row dr of the group, V = 16 half dr of its one entry
  const int dr = tid >> 7, dch = tid & (kGTChunks - 1);
  const uint32_t hoff = V == 16 ? (uint32_t)dr * 16u : 0u;
  const uint32_t wslot = (uint32_t)(dch * 16 + dr * 8), wx = (uint32_t)(dch & 7);
  // MFMA role: lane (token / output mj, k group mkg); step i reads chunk 32 wave + 8 mkg + i
  const int mj = lane & 15, mkg = lane >> 4;
  const int mch0 = wave * 32 + mkg * 8;

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
    gather1(0, gxwg_elem<0>(n, T, tmask)); gather1(1, gxwg_elem<1>(n, T, tmask));
    gather1(2, gxwg_elem<2>(n, T, tmask)); gather1(3, gxwg_elem<3>(n, T, tmask));
    gather1(4, gxwg_elem<4>(n, T, tmask)); gather1(5, gxwg_elem<5>(n, T, tmask));
    gather1(6, gxwg_elem<6>(n, T, tmask)); gather1(7, gxwg_elem<7>(n, T, tmask));
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
    // ---- block 0's A operands, a whole tile ahead, held through the rebuild
    u32x4 xa[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) xa[i] = gt_load_a1<false>(nullptr, P.x, L.xoff[0], G, t * kGTTile + (mch0 + i) * 8);
    gt_rebuild<DT, RES != 0>(cv, rv, sp, bp, t * kGTTile + dch * 8 < G);
    __syncthreads();   // the previous tile's MFMA reads (and the previous row group's sums) are done
    gt_write_tile(tile, wslot, wx, cv);
    // ---- block 1's A operands, whole and back to back, in front of the gathers
    u32x4 xb[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) xb[i] = gt_load_a1<false>(nullptr, P.x, L.xoff[1], G, t * kGTTile + (mch0 + i) * 8);
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
      acc[1] = mfma16x16x32<DT>(masked(xb[i], kin && L.tok_b[1]), b, acc[1]);
    }
    if constexpr (TB == 3) {
      // ---- block 2 takes block 0's registers: its 8 loads back to back, then the 8 K-steps again over the same tile
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 8; ++i) xa[i] = gt_load_a1<false>(nullptr, P.x, L.xoff[2], G, t * kGTTile + (mch0 + i) * 8);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const bool kin = t * kGTTile + (mch0 + i) * 8 < G;
        const u32x4 b = tile[(mch0 + i) * 16 + (mj ^ i)];
        acc[2] = mfma16x16x32<DT>(masked(xa[i], kin && L.tok_b[2]), b, acc[2]);
      }
    }
  }
  // ---- one epilogue per block, on the block's rows of the member's y (gt_epilogue's first barrier also ends the reads of the block before)
#pragma unroll
  for (int b = 0; b < TB; ++b) {
    GemmGatherParams Pb = P;
    Pb.tokens = tokens - 16 * b;
    Pb.y = (char*)P.y + (size_t)(16 * b) * P.O * (P.out_f32 ? 4 : 2);
    gt_epilogue<DT>(Pb, tid, lane, wave, (float*)smem, rg, acc[b]);
  }
}

// A workgroup walks the global row groups g = blockIdx.x, + gridDim.x, ...: g rises, so the member never falls - the members are
// visited in order, and a member's state (its argument block, RES = 1: its residual table in LDS) is set up at the switch.  What the
// members share is set up once, in front of the walk.  (gemm_gatherx_grouped_kernel's walk.)
template <typename DT, int V, int RES, int TB>
__global__ __launch_bounds__(kGTThreads, gxwg_min_wg(RES, TB)) void gemm_gatherxw_grouped_kernel(const GemmGatherXWGroupedParams GP) {
  static_assert(V == 8 || V == 16, "vector length");
  static_assert(RES >= 0 && RES <= 2, "residual: none, LDS, L2");
  static_assert(TB == 2 || TB == 3, "17 - 32 / 33 - 48 tokens");
  extern __shared__ __attribute__((aligned(16))) unsigned char gxwg_smem[];
  const int tid = threadIdx.x, mj = tid & 15;
  // ---- the launch's state: member 0's block states it for all (the host's check)
  GxwgLaunch<TB> L;
  {
    const int G = GP.m[0].G, tokens = GP.m[0].tokens;
    L.ib = GP.m[0].ib;
    L.T = GP.m[0].ib + GP.m[0].rb;
    L.tmask = L.T >= 32 ? 0xffffffffu : ((1u << L.T) - 1u);
    L.mmask = (1u << L.ib) - 1u;
    // the 9th window word: 8 T bits + the largest offset (24, 16 or 0 bits: T odd, T % 4 == 2, T % 4 == 0) beyond 8 words (T = 31)
    L.need9 = 8 * L.T + ((L.T & 1) ? 24 : (L.T & 2) ? 16 : 0) > 256;
    L.n_tiles = (G + kGTTile - 1) / kGTTile;
#pragma unroll
    for (int b = 0; b < TB; ++b) {   // block 0 is whole: 16 < tokens
      const int tk = 16 * b + mj;
      L.tok_b[b] = tk < tokens;
      L.xoff[b] = (uint32_t)(tk < tokens ? tk : tokens - 1) * (uint32_t)G * 2u;
    }
  }
  int g = blockIdx.x;
#pragma unroll 1
  for (int m = 0; m < GP.n; ++m) {
    const int first = GP.first_group[m], end = GP.first_group[m + 1];
    if (g >= end) continue;   // (uniform: g is the workgroup's)
    const GemmGatherParams P = GP.m[m];
    if constexpr (RES == 1) {
      __syncthreads();   // the other waves' table reads of the previous member's last row group are done
      const int n16 = P.res_bytes >> 4;
      for (int i = tid; i < n16; i += kGTThreads)
        *(u32x4*)(gxwg_smem + kGTTileBytes + (size_t)i * 16) = *(const u32x4*)(P.rcent + (size_t)i * 16);
      __syncthreads();
    }
#pragma unroll 1
    for (; g < end; g += gridDim.x) gxwg_row_group<DT, V, RES, TB>(P, L, gxwg_smem, g - first);
  }
}

// ---- host side -------------------------------------------------------------------
// what one grouped launch IS: the template arguments of gemm_gatherxw_grouped_kernel<DT, V, RES, TB>, the run-time index widths,
// every member's row groups and the launch shape, decided once for the launcher and for vptq_quant_gemm_gatherxw_grouped_instance.
// The members share dtype, width and format (the caller's check): everything but the row groups is gemm_gatherx_decide's of the
// first.  wgcu: the workgroups per CU that are resident - gemm_gatherx_decide's LDS bound or the register bound, whichever is less
GemmGatherXWGroupedDecision gemm_gatherxw_grouped_decide(const VptqLayerDesc* descs, int n, int tokens) {
  GemmGatherXWGroupedDecision D = {};
  if (n < 1 || n > kGXWGMembers) return D;
  const GemmGatherXDecision S = gemm_gatherx_decide(descs[0], 16);
  D.f16 = S.f16;
  D.v = S.v; D.ib = S.ib; D.rb = S.rb;
  D.res = S.res; D.res_bytes = S.res_bytes;
  D.tok = tokens;
  D.tb = (tokens + 15) / 16;
  D.n = n;
  D.tiles = S.tiles;
  D.lds = S.lds;
  const int regs_wg = gxwg_min_wg(D.res, D.tb);
  D.wgcu = S.wgcu < regs_wg ? S.wgcu : regs_wg;
  const int rows = D.v == 16 ? 1 : 2;   // vector-rows per row group of 16 outputs
  for (int m = 0; m < n; ++m) {
    D.groups[m] = (descs[m].num_indices + rows - 1) / rows;
    D.first_group[m + 1] = D.first_group[m] + D.groups[m];
  }
  D.total = D.first_group[n];
  const int slots = device_cus() * D.wgcu;
  D.grid = D.total < slots ? D.total : slots;
  D.rgs = D.grid > 0 ? (D.total + D.grid - 1) / D.grid : 0;
  return D;
}

template <typename DT, int V, int RES>
static hipError_t launch_gxwg(const GemmGatherXWGroupedParams& GP, const GemmGatherXWGroupedDecision& D, hipStream_t st) {
  const dim3 grid(D.grid), block(kGTThreads);
  if (D.tb == 2) hipLaunchKernelGGL((gemm_gatherxw_grouped_kernel<DT, V, RES, 2>), grid, block, D.lds, st, GP);
  else hipLaunchKernelGGL((gemm_gatherxw_grouped_kernel<DT, V, RES, 3>), grid, block, D.lds, st, GP);
  return hipGetLastError();
}

template <typename DT, int V>
static hipError_t launch_gxwg_v(const GemmGatherXWGroupedParams& GP, const GemmGatherXWGroupedDecision& D, hipStream_t st) {
  switch (D.res) {
    case 0: return launch_gxwg<DT, V, 0>(GP, D, st);
    case 1: return launch_gxwg<DT, V, 1>(GP, D, st);
    case 2: return launch_gxwg<DT, V, 2>(GP, D, st);
    default: return hipErrorInvalidValue;
  }
}

template <typename DT>
static hipError_t launch_gxwg_dt(const GemmGatherXWGroupedParams& GP, const GemmGatherXWGroupedDecision& D, hipStream_t st) {
  switch (D.v) {
    case 8: return launch_gxwg_v<DT, 8>(GP, D, st);
    case 16: return launch_gxwg_v<DT, 16>(GP, D, st);
    default: return hipErrorInvalidValue;
  }
}

// descs: the members WITHOUT a permutation (a permuted member as its plain form); x[m]: member m's activations in its own column order
hipError_t launch_gemm_gatherxw_grouped(const VptqLayerDesc* descs, int n, const void* const* x, void* const* y, int tokens, bool out_f32,
                                        hipStream_t st) {
  const GemmGatherXWGroupedDecision D = gemm_gatherxw_grouped_decide(descs, n, tokens);
  if (D.n < 2 || D.grid < 1 || tokens < 17 || tokens > 48 || D.tb < 2 || D.tb > 3 || D.lds > 65536) return hipErrorInvalidValue;
  GemmGatherXWGroupedParams GP = {};
  for (int m = 0; m < n; ++m) {
    // (the kernel reads width, index widths and table size from member 0's block: every member's are the first's)
    if (descs[m].perm || !x[m] || !y[m] || descs[m].group_size != descs[0].group_size || descs[m].vector_len != D.v ||
        descs[m].index_bits != D.ib || descs[m].res_bits != D.rb || descs[m].num_res_centroids * descs[m].vector_len * 2 != D.res_bytes)
      return hipErrorInvalidValue;
    GP.m[m] = gemm_gather_params(descs[m], x[m], y[m], tokens, out_f32, D.groups[m]);
    GP.m[m].ib = D.ib; GP.m[m].rb = D.rb; GP.m[m].res_bytes = D.res_bytes;
    GP.first_group[m] = D.first_group[m];
  }
  for (int m = n; m <= kGXWGMembers; ++m) GP.first_group[m] = D.total;
  GP.n_groups = D.total;
  GP.n = n;
  return D.f16 ? launch_gxwg_dt<F16>(GP, D, st) : launch_gxwg_dt<BF16>(GP, D, st);
}

}  // namespace vptq
