// Batched decode for the large-codebook VPTQ formats (v = 8, k = 65536 main centroids; residual: none, 256 or 65536 -
// gemv_gather.hip's layers): up to 16 tokens in ONE launch, tokens = the M dimension of a matrix-core contraction.
//
// gemv_gather keeps TOK x 8 fp32 sums per lane and stops at 8 tokens; 9 - 16 tokens went through vptq_dequant + a dense GEMM.
// Here the contraction is D[token][output] += X[token][k] * W[output][k] in v_mfma_f32_16x16x32_f16 / _bf16, so the token count
// costs no registers: one pass over the packed indices, one gather per index, whatever the token count.
//
// Structure: the tile pipeline described in gemm_gather_tile.h, whose phases (A load, rebuild, tile write, MFMA phase, epilogue) are
// that header's functions.  This file's own:
//  * a row group is kMRows = 2 vector-rows; thread half dr takes vector-row dr of the group.
//  * a thread reads the packed index words of its 8 columns with one wide load (gemv_gather's Fmt / elem; T = 16 / 24 / 32 bits per
//    element, compile time); main index = the low 16 bits, residual index = the rest.
//  * T = 32: 8 residual gathers from L2; T = 24: the 4 KiB residual table sits in static LDS beside the tile.
//  * the loop skeleton: load_idx / gt_load_sb / gather for tile t + 1 and t + 2 around the phases, two barriers per tile.
// 36 KiB of LDS at most: four workgroups per CU.
// gemm_gather_grouped_kernel (below the single kernel): 2 - 4 sibling layers' row groups as one list in one launch, plain form only.
#include "gemm_gather_tile.h"

namespace vptq {

constexpr int kMRows = 2;                         // vector-rows per row group (16 outputs)
constexpr int kMWgPerCu = 4;

template <typename DT, int T, bool PERM>
__global__ __launch_bounds__(kGTThreads) void gemm_gather_kernel(const GemmGatherParams P) {
  constexpr int NW = T / 4;   // index words of 8 elements
  constexpr bool RES = T > 16;
  __shared__ __attribute__((aligned(16))) u32x4 tile[kGTChunks * 16];   // [chunk][16 outputs]: 32 KiB
  __shared__ u32x4 rtab[T == 24 ? 256 : 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int G = P.G, N = P.N, O = P.O, tokens = P.tokens;
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
  const uint16_t* const xrow = P.x + (size_t)(mj < tokens ? mj : tokens - 1) * G;

  for (int rg = blockIdx.x; rg < P.n_groups; rg += gridDim.x) {
    const int row = rg * kMRows + dr;
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
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};

    for (int t = 0; t < n_tiles; ++t) {
      u32x4 xa[8];
      gt_load_a<PERM>(P.perm, xrow, G, mch0, t, xa);
      gt_rebuild<DT, RES>(cv, rv, sp, bp, t * kGTTile + dch * 8 < G);
      __syncthreads();   // the previous tile's MFMA reads (and the previous row group's sums) are done
      gt_write_tile(tile, wslot, wx, cv);
      // ---- the next tile's gathers fly during the MFMA phase; the index words and scale / bias of the one after follow
      if (t + 1 < n_tiles) {
        gather(wq);
#pragma unroll
        for (int q = 0; q < 4; ++q) { sp[q] = sp_next[q]; bp[q] = bp_next[q]; }
        load_idx(t + 2, wq);
        gt_load_sb(P, dcol(t + 2), sp_next, bp_next);
      }
      __syncthreads();   // tile complete
      // ---- this wave's 8 K-steps (kept in this file: as a shared function it cost 3 - 8 % at 16 tokens, profiles/r17)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const bool live = mj < tokens && t * kGTTile + (mch0 + i) * 8 < G;
        const u32x4 a = {live ? xa[i][0] : 0u, live ? xa[i][1] : 0u, live ? xa[i][2] : 0u, live ? xa[i][3] : 0u};
        const u32x4 b = tile[(mch0 + i) * 16 + (mj ^ i)];   // ((mch0 + i) & 7 == i)
        acc = mfma16x16x32<DT>(a, b, acc);
      }
    }
    gt_epilogue<DT>(P, tid, lane, wave, (float*)tile, rg, acc);
  }
}

// ---- sibling layers (q / k / v, gate / up) in ONE launch: the row-group lists of up to kGGMembers layers, concatenated ---------------
// A row group is independent of the grid, so member m's row group rg has the bits gemm_gather_kernel<DT, T, false> gives it in the
// member's own launch.  Plain form only: a member with a column permutation arrives as its descriptor without one and x[perm] for x.
constexpr int kGGMembers = 4;

struct GemmGatherGroupedParams {
  GemmGatherParams m[kGGMembers];
  int first_group[kGGMembers + 1];   // member m owns the global row groups [first_group[m], first_group[m + 1])
  int n_groups, n;
};

// one row group of one member: the row-group body of gemm_gather_kernel<DT, T, false>, statement for statement.  A copy, not a function
// both kernels share: with the single kernel calling it (the per-thread roles computed inside the function), all 12 instantiations of
// gemm_gather_kernel came out with other instructions (profiles/r31/listings.md, "shared body"), and that kernel's device code is
// not to change.  A change to one copy belongs in the other.
template <typename DT, int T>
static __device__ __forceinline__ void gg_row_group(const GemmGatherParams& P, u32x4* tile, const u32x4* rtab, const uint16_t* xrow, int rg) {
  constexpr int NW = T / 4;   // index words of 8 elements
  constexpr bool RES = T > 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int G = P.G, N = P.N, tokens = P.tokens;
  const int n_tiles = (G + kGTTile - 1) / kGTTile;
  const int dr = tid >> 7, dch = tid & (kGTChunks - 1);
  const uint32_t wslot = (uint32_t)(dch * 16 + dr * 8), wx = (uint32_t)(dch & 7);
  const int mj = lane & 15, mkg = lane >> 4;
  const int mch0 = wave * 32 + mkg * 8;

  const int row = rg * kMRows + dr;
  const uint32_t* const irow = P.idx + (size_t)(row < N ? row : N - 1) * P.row_words;
  auto dcol = [&](int t) { return gt_dcol(t, dch, G); };
  auto load_idx = [&](int t, uint32_t (&w)[NW]) {
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
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};

  for (int t = 0; t < n_tiles; ++t) {
    u32x4 xa[8];
    gt_load_a<false>(nullptr, xrow, G, mch0, t, xa);
    gt_rebuild<DT, RES>(cv, rv, sp, bp, t * kGTTile + dch * 8 < G);
    __syncthreads();   // the previous tile's MFMA reads (and the previous row group's sums) are done
    gt_write_tile(tile, wslot, wx, cv);
    if (t + 1 < n_tiles) {
      gather(wq);
#pragma unroll
      for (int q = 0; q < 4; ++q) { sp[q] = sp_next[q]; bp[q] = bp_next[q]; }
      load_idx(t + 2, wq);
      gt_load_sb(P, dcol(t + 2), sp_next, bp_next);
    }
    __syncthreads();   // tile complete
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const bool live = mj < tokens && t * kGTTile + (mch0 + i) * 8 < G;
      const u32x4 a = {live ? xa[i][0] : 0u, live ? xa[i][1] : 0u, live ? xa[i][2] : 0u, live ? xa[i][3] : 0u};
      const u32x4 b = tile[(mch0 + i) * 16 + (mj ^ i)];
      acc = mfma16x16x32<DT>(a, b, acc);
    }
  }
  gt_epilogue<DT>(P, tid, lane, wave, (float*)tile, rg, acc);
}

// A workgroup walks the global row groups g = blockIdx.x, + gridDim.x, ...: g rises, so the member never falls - the members are
// visited in order, and a member's state (its argument block, its x row, T = 24: its residual table in LDS) is set up at the switch.
template <typename DT, int T>
__global__ __launch_bounds__(kGTThreads) void gemm_gather_grouped_kernel(const GemmGatherGroupedParams GP) {
  __shared__ __attribute__((aligned(16))) u32x4 tile[kGTChunks * 16];   // [chunk][16 outputs]: 32 KiB
  __shared__ u32x4 rtab[T == 24 ? 256 : 1];
  const int tid = threadIdx.x, mj = tid & 15;
  int g = blockIdx.x;
#pragma unroll 1
  for (int m = 0; m < GP.n; ++m) {
    const int first = GP.first_group[m], end = GP.first_group[m + 1];
    if (g >= end) continue;   // (uniform: g is the workgroup's)
    const GemmGatherParams P = GP.m[m];
    const uint16_t* const xrow = P.x + (size_t)(mj < P.tokens ? mj : P.tokens - 1) * P.G;
    if constexpr (T == 24) {
      __syncthreads();   // the other waves' table reads of the previous member's last row group are done
      rtab[tid] = *(const u32x4*)(P.rcent + (size_t)tid * 16);   // kGTThreads == 256 entries
      __syncthreads();
    }
#pragma unroll 1
    for (; g < end; g += gridDim.x) gg_row_group<DT, T>(P, tile, rtab, xrow, g - first);
  }
}

// ---- host side -------------------------------------------------------------------
bool gemm_gather_eligible(const VptqLayerDesc& d, int tokens) {
  return gemv_gather_eligible(d, tokens, 16);   // gemv_gather's layers, 1 - 16 tokens per launch
}

// what one launch IS: the template arguments of gemm_gather_kernel<DT, T, PERM> and the launch shape, decided once for the
// launcher and for vptq_quant_gemm_gather_instance
GemmGatherDecision gemm_gather_decide(const VptqLayerDesc& d, int tokens) {
  GemmGatherDecision D = {};
  D.f16 = d.dtype == VPTQ_DTYPE_F16;
  D.perm = d.perm != nullptr;
  D.T = d.num_res_centroids == 0 ? 16 : d.num_res_centroids == 256 ? 24 : 32;
  D.tok = tokens;
  D.tiles = (d.group_size + kGTTile - 1) / kGTTile;
  const GemmGatherGrid g = gemm_gather_grid(d.num_indices, kMRows, kMWgPerCu);
  D.n_groups = g.n_groups; D.grid = g.grid; D.rgs = g.rgs;
  return D;
}

template <typename DT, int T>
static hipError_t launch_mg(const GemmGatherParams& P, const GemmGatherDecision& D, hipStream_t st) {
  const dim3 grid(D.grid), block(kGTThreads);
  if (D.perm) hipLaunchKernelGGL((gemm_gather_kernel<DT, T, true>), grid, block, 0, st, P);
  else hipLaunchKernelGGL((gemm_gather_kernel<DT, T, false>), grid, block, 0, st, P);
  return hipGetLastError();
}

template <typename DT>
static hipError_t launch_mg_dt(const GemmGatherParams& P, const GemmGatherDecision& D, hipStream_t st) {
  switch (D.T) {
    case 16: return launch_mg<DT, 16>(P, D, st);
    case 24: return launch_mg<DT, 24>(P, D, st);
    case 32: return launch_mg<DT, 32>(P, D, st);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_gemm_gather(const VptqLayerDesc& d, const void* x, void* y, int tokens, bool out_f32, hipStream_t st) {
  const GemmGatherDecision D = gemm_gather_decide(d, tokens);
  if (D.grid < 1 || tokens < 1 || tokens > 16) return hipErrorInvalidValue;
  const GemmGatherParams P = gemm_gather_params(d, x, y, tokens, out_f32, D.n_groups);
  return D.f16 ? launch_mg_dt<F16>(P, D, st) : launch_mg_dt<BF16>(P, D, st);
}

// what one grouped launch IS: the template arguments of gemm_gather_grouped_kernel<DT, T>, every member's row groups and the launch
// shape, decided once for the launcher and for vptq_quant_gemm_gather_grouped_instance.  The members share dtype, width and T (the
// caller's check): dt, T and tiles are the first member's
GemmGatherGroupedDecision gemm_gather_grouped_decide(const VptqLayerDesc* descs, int n, int tokens) {
  GemmGatherGroupedDecision D = {};
  if (n < 1 || n > kGGMembers) return D;
  D.f16 = descs[0].dtype == VPTQ_DTYPE_F16;
  D.T = descs[0].num_res_centroids == 0 ? 16 : descs[0].num_res_centroids == 256 ? 24 : 32;
  D.tok = tokens;
  D.n = n;
  D.tiles = (descs[0].group_size + kGTTile - 1) / kGTTile;
  for (int m = 0; m < n; ++m) {
    D.groups[m] = (descs[m].num_indices + kMRows - 1) / kMRows;
    D.first_group[m + 1] = D.first_group[m] + D.groups[m];
  }
  D.total = D.first_group[n];
  const int slots = device_cus() * kMWgPerCu;
  D.grid = D.total < slots ? D.total : slots;
  D.rgs = D.grid > 0 ? (D.total + D.grid - 1) / D.grid : 0;
  return D;
}

template <typename DT>
static hipError_t launch_mgg_dt(const GemmGatherGroupedParams& GP, const GemmGatherGroupedDecision& D, hipStream_t st) {
  const dim3 grid(D.grid), block(kGTThreads);
  switch (D.T) {
    case 16: hipLaunchKernelGGL((gemm_gather_grouped_kernel<DT, 16>), grid, block, 0, st, GP); break;
    case 24: hipLaunchKernelGGL((gemm_gather_grouped_kernel<DT, 24>), grid, block, 0, st, GP); break;
    case 32: hipLaunchKernelGGL((gemm_gather_grouped_kernel<DT, 32>), grid, block, 0, st, GP); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// descs: the members WITHOUT a permutation (a permuted member as its plain form); x[m]: member m's activations in its own column order
hipError_t launch_gemm_gather_grouped(const VptqLayerDesc* descs, int n, const void* const* x, void* const* y, int tokens, bool out_f32,
                                      hipStream_t st) {
  const GemmGatherGroupedDecision D = gemm_gather_grouped_decide(descs, n, tokens);
  if (D.n < 2 || D.grid < 1 || tokens < 1 || tokens > 16) return hipErrorInvalidValue;
  GemmGatherGroupedParams GP = {};
  for (int m = 0; m < n; ++m) {
    if (descs[m].perm || !x[m] || !y[m]) return hipErrorInvalidValue;
    GP.m[m] = gemm_gather_params(descs[m], x[m], y[m], tokens, out_f32, D.groups[m]);
    GP.first_group[m] = D.first_group[m];
  }
  for (int m = n; m <= kGGMembers; ++m) GP.first_group[m] = D.total;
  GP.n_groups = D.total;
  GP.n = n;
  return D.f16 ? launch_mgg_dt<F16>(GP, D, st) : launch_mgg_dt<BF16>(GP, D, st);
}

}  // namespace vptq
