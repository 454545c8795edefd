// Batched decode of SIBLING layers (q / k / v, gate / up) of the large-codebook VPTQ formats gemm_gatherx.hip serves (vector length 8 or
// 16, 16384 ... 65536 main centroids, any residual codebook: "v16-k65536-65536 / -32768 / -1024 / -256 / -64 / -0", "v8-k65536-4096 / -4",
// "v8-k32768-0", "v8-k16384-0"), 1 - 16 tokens in ONE launch: gemm_gatherx_kernel's row-group body (gemm_gatherx.hip: the tile pipeline
// of gemm_gather_tile.h, the any-T index window, gx_elem) behind gemm_gather_grouped_kernel's member walk (gemm_gather.hip: the row-group
// lists of up to 4 layers, concatenated).
//
// Without it every member of such a group goes out alone - gemm_gatherx, gemm_gather_px (a permute launch, then gemm_gatherx) or
// vptq_dequant + a dense GEMM, whichever its size gives it - and k / v alone (64 row groups) occupy a quarter of the CUs.  Here the
// members' row groups are one list, walked by min(total row groups, CUs x wgcu) workgroups, wgcu as gemm_gatherx_decide gives it for
// the members' shared format (they share v, k and kr, hence V, RES, the index widths and the LDS need).  Plain form only: a member
// with a column permutation arrives as its descriptor without one and x[perm] for its x (one x gather per DISTINCT permutation: the
// caller's, vptq_quant_gemm_gatherx_grouped).
// BIT CONTRACT: a row group does not depend on the grid or on the workgroup that runs it, so member m's row group rg has the bits
// gemm_gatherx_kernel<DT, V, RES, false> gives it in the member's own launch.
// LDS: 32 KiB tile + the residual table (RES = 1), as gemm_gatherx: 4 / 3 / 2 workgroups per CU at 40 / 48 / 64 KiB.  No workspace of
// its own, no atomics, no scratch.
#include "gemm_gather_tile.h"

namespace vptq {

constexpr int kGXGMembers = 4;

struct GemmGatherXGroupedParams {
  GemmGatherParams m[kGXGMembers];
  int first_group[kGXGMembers + 1];   // member m owns the global row groups [first_group[m], first_group[m + 1])
  int n_groups, n;
};

// element E (compile time) of T bits (wave uniform) out of the normalised window n[0..7] (gemm_gatherx.hip: gx_elem, a copy - that
// unit's device code is not to change, and a header both include is a change to it)
template <int E>
static __device__ __forceinline__ uint32_t gxg_elem(const uint32_t (&n)[8], int T, uint32_t mask) {
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

// one row group of one member: the row-group body of gemm_gatherx_kernel<DT, V, RES, false> (gemm_gatherx.hip), statement for
// statement.  A copy, not a function both kernels share: a shared body gave the existing instantiations of the single kernels other
// instructions (profiles/r31/listings.md, "shared body"), and their device code is not to change.
// A change to one copy belongs in the other.  smem: the tile, behind it (RES = 1) the member's residual table, staged at the switch.
template <typename DT, int V, int RES>
static __device__ __forceinline__ void gxg_row_group(const GemmGatherParams& P, unsigned char* smem, const uint16_t* xrow, int rg) {
  constexpr int kRows = 16 / V;   // vector-rows per row group (16 outputs)
  constexpr int EB = V * 2;       // bytes per codebook entry
  u32x4* const tile = (u32x4*)smem;                              // [chunk][16 outputs]: 32 KiB
  const unsigned char* const rtab = smem + kGTTileBytes;         // RES = 1: the residual table
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int G = P.G, N = P.N, tokens = P.tokens;
  const int T = P.ib + P.rb, ib = P.ib;
  const uint32_t tmask = T >= 32 ? 0xffffffffu : ((1u << T) - 1u), mmask = (1u << ib) - 1u;
  // the 9th window word: 8 T bits + the largest offset (24, 16 or 0 bits: T odd, T % 4 == 2, T % 4 == 0) beyond 8 words (T = 31)
  const bool need9 = 8 * T + ((T & 1) ? 24 : (T & 2) ? 16 : 0) > 256;
  const int last = P.row_words - 1;
  const int n_tiles = (G + kGTTile - 1) / kGTTile;
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
    gather1(0, gxg_elem<0>(n, T, tmask)); gather1(1, gxg_elem<1>(n, T, tmask));
    gather1(2, gxg_elem<2>(n, T, tmask)); gather1(3, gxg_elem<3>(n, T, tmask));
    gather1(4, gxg_elem<4>(n, T, tmask)); gather1(5, gxg_elem<5>(n, T, tmask));
    gather1(6, gxg_elem<6>(n, T, tmask)); gather1(7, gxg_elem<7>(n, T, tmask));
  };
  uint32_t wq[8], sp[4], bp[4], sp_next[4], bp_next[4];
  load_idx(0, wq);
  gt_load_sb(P, dcol(0), sp, bp);
  gather(wq);
  load_idx(1, wq);
  gt_load_sb(P, dcol(1), sp_next, bp_next);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};

  for (int t = 0; t < n_tiles; ++t) {
    u32x4 xa[8];
    gt_load_a<false>(nullptr, xrow, G, mch0, t, xa);
    gt_rebuild<DT, RES != 0>(cv, rv, sp, bp, t * kGTTile + dch * 8 < G);
    __syncthreads();   // the previous tile's MFMA reads (and the previous row group's sums) are done
    gt_write_tile(tile, wslot, wx, cv);
    // ---- the next tile's gathers fly during the MFMA phase; the index window and scale / bias of the one after follow
    if (t + 1 < n_tiles) {
      gather(wq);
#pragma unroll
      for (int q = 0; q < 4; ++q) { sp[q] = sp_next[q]; bp[q] = bp_next[q]; }
      load_idx(t + 2, wq);
      gt_load_sb(P, dcol(t + 2), sp_next, bp_next);
    }
    __syncthreads();   // tile complete
    // ---- this wave's 8 K-steps
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const bool live = mj < tokens && t * kGTTile + (mch0 + i) * 8 < G;
      const u32x4 a = {live ? xa[i][0] : 0u, live ? xa[i][1] : 0u, live ? xa[i][2] : 0u, live ? xa[i][3] : 0u};
      const u32x4 b = tile[(mch0 + i) * 16 + (mj ^ i)];   // ((mch0 + i) & 7 == i)
      acc = mfma16x16x32<DT>(a, b, acc);
    }
  }
  gt_epilogue<DT>(P, tid, lane, wave, (float*)smem, rg, acc);
}

// A workgroup walks the global row groups g = blockIdx.x, + gridDim.x, ...: g rises, so the member never falls - the members are
// visited in order, and a member's state (its argument block - pointers, scale / bias -, its x row, RES = 1: its residual table in LDS)
// is set up at the switch.  (gemm_gather_grouped_kernel's walk.)
template <typename DT, int V, int RES>
__global__ __launch_bounds__(kGTThreads) void gemm_gatherx_grouped_kernel(const GemmGatherXGroupedParams GP) {
  static_assert(V == 8 || V == 16, "vector length");
  static_assert(RES >= 0 && RES <= 2, "residual: none, LDS, L2");
  extern __shared__ __attribute__((aligned(16))) unsigned char gxg_smem[];
  const int tid = threadIdx.x, mj = tid & 15;
  int g = blockIdx.x;
#pragma unroll 1
  for (int m = 0; m < GP.n; ++m) {
    const int first = GP.first_group[m], end = GP.first_group[m + 1];
    if (g >= end) continue;   // (uniform: g is the workgroup's)
    const GemmGatherParams P = GP.m[m];
    const uint16_t* const xrow = P.x + (size_t)(mj < P.tokens ? mj : P.tokens - 1) * P.G;
    if constexpr (RES == 1) {
      __syncthreads();   // the other waves' table reads of the previous member's last row group are done
      const int n16 = P.res_bytes >> 4;
      for (int i = tid; i < n16; i += kGTThreads)
        *(u32x4*)(gxg_smem + kGTTileBytes + (size_t)i * 16) = *(const u32x4*)(P.rcent + (size_t)i * 16);
      __syncthreads();
    }
#pragma unroll 1
    for (; g < end; g += gridDim.x) gxg_row_group<DT, V, RES>(P, gxg_smem, xrow, g - first);
  }
}

// ---- host side -------------------------------------------------------------------
// what one grouped launch IS: the template arguments of gemm_gatherx_grouped_kernel<DT, V, RES>, the run-time index widths, every
// member's row groups and the launch shape, decided once for the launcher and for vptq_quant_gemm_gatherx_grouped_instance.  The
// members share dtype, width and format (the caller's check): everything but the row groups is gemm_gatherx_decide's of the first
GemmGatherXGroupedDecision gemm_gatherx_grouped_decide(const VptqLayerDesc* descs, int n, int tokens) {
  GemmGatherXGroupedDecision D = {};
  if (n < 1 || n > kGXGMembers) return D;
  const GemmGatherXDecision S = gemm_gatherx_decide(descs[0], tokens);
  D.f16 = S.f16;
  D.v = S.v; D.ib = S.ib; D.rb = S.rb;
  D.res = S.res; D.res_bytes = S.res_bytes;
  D.tok = tokens;
  D.n = n;
  D.tiles = S.tiles;
  D.lds = S.lds; D.wgcu = S.wgcu;
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

template <typename DT, int V>
static hipError_t launch_gxg_v(const GemmGatherXGroupedParams& GP, const GemmGatherXGroupedDecision& D, hipStream_t st) {
  const dim3 grid(D.grid), block(kGTThreads);
  switch (D.res) {
    case 0: hipLaunchKernelGGL((gemm_gatherx_grouped_kernel<DT, V, 0>), grid, block, D.lds, st, GP); break;
    case 1: hipLaunchKernelGGL((gemm_gatherx_grouped_kernel<DT, V, 1>), grid, block, D.lds, st, GP); break;
    case 2: hipLaunchKernelGGL((gemm_gatherx_grouped_kernel<DT, V, 2>), grid, block, D.lds, st, GP); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

template <typename DT>
static hipError_t launch_gxg_dt(const GemmGatherXGroupedParams& GP, const GemmGatherXGroupedDecision& D, hipStream_t st) {
  switch (D.v) {
    case 8: return launch_gxg_v<DT, 8>(GP, D, st);
    case 16: return launch_gxg_v<DT, 16>(GP, D, st);
    default: return hipErrorInvalidValue;
  }
}

// descs: the members WITHOUT a permutation (a permuted member as its plain form); x[m]: member m's activations in its own column order
hipError_t launch_gemm_gatherx_grouped(const VptqLayerDesc* descs, int n, const void* const* x, void* const* y, int tokens, bool out_f32,
                                       hipStream_t st) {
  const GemmGatherXGroupedDecision D = gemm_gatherx_grouped_decide(descs, n, tokens);
  if (D.n < 2 || D.grid < 1 || tokens < 1 || tokens > 16 || D.lds > 65536) return hipErrorInvalidValue;
  GemmGatherXGroupedParams GP = {};
  for (int m = 0; m < n; ++m) {
    // (the table copied into LDS is the one D.lds has room for: every member's is the first's size)
    if (descs[m].perm || !x[m] || !y[m] || descs[m].num_res_centroids * descs[m].vector_len * 2 != D.res_bytes) return hipErrorInvalidValue;
    GP.m[m] = gemm_gather_params(descs[m], x[m], y[m], tokens, out_f32, D.groups[m]);
    GP.m[m].ib = D.ib; GP.m[m].rb = D.rb; GP.m[m].res_bytes = D.res_bytes;
    GP.first_group[m] = D.first_group[m];
  }
  for (int m = n; m <= kGXGMembers; ++m) GP.first_group[m] = D.total;
  GP.n_groups = D.total;
  GP.n = n;
  return D.f16 ? launch_gxg_dt<F16>(GP, D, st) : launch_gxg_dt<BF16>(GP, D, st);
}

}  // namespace vptq
