// Batched decode for the large-codebook VPTQ formats gemm_gather.hip does not take: vector length 8 or 16, 16384 ... 65536 main
// centroids, ANY residual codebook (none ... 65536 entries, i.e. any total index width T = index_bits + res_bits <= 32) -
// "v16-k65536-65536 / -32768 / -1024 / -256 / -64 / -0", "v8-k65536-4096 / -4", "v8-k32768-0", "v8-k16384-0": up to 16 tokens in ONE
// launch, tokens = the M dimension of v_mfma_f32_16x16x32.  It is to gemm_gather.hip what gemv_gatherx.hip is to gemv_gather.hip.
//
// gemv_gatherx keeps TOK x V fp32 sums per lane and stops at 4 tokens for v = 16 (8 for v = 8): 5 - 8 tokens of a v = 16 layer were two
// launches, each a full pass over the indices and the gathers, and 9 - 16 tokens went through vptq_dequant + a dense GEMM.
//
// Structure: the tile pipeline described in gemm_gather_tile.h, whose phases are that header's functions, inside gemm_gather.hip's loop
// skeleton.  No atomics, no workspace, no scratch.  What differs from gemm_gather.hip:
//  * V = 16: a row group is ONE vector-row; the two thread halves (tid >> 7) take the two 16-byte halves of the same 32-byte entry
//    (cent + idx * 32 + 16 * half) and read the same index window.  V = 8: two vector-rows per group, as in gemm_gather.
//  * index path for any T (run-time, wave-uniform): a thread's 8 elements are 8 T bits that start at byte T * chunk of the packed
//    row (gemv_gatherx.hip's row format).  The window of up to 9 words is loaded from the containing word (past the row end word
//    by word with the word number clamped: the bits that matter are inside the row, row_words * 32 >= G * T), normalised once with
//    v_alignbit_b32; element e then sits at bit e * T, a wave-uniform position.  Main index = the low index_bits, residual index
//    = the next res_bits.
//  * residual table: RES = 1: a table of at most kXResLdsMax = 32 KiB is copied into the dynamic LDS behind the tile once per
//    workgroup (as gemv_gatherx does); RES = 2: gathered from L2; RES = 0: none.
// LDS: 32 KiB tile + the table: 4 workgroups per CU up to 40 KiB, 3 up to 48 KiB, 2 at 64 KiB (gemm_gatherx_decide: wgcu).
#include "gemm_gather_tile.h"

namespace vptq {

constexpr int kGXResLdsMax = 32768;                // (gemv_gatherx.hip: kXResLdsMax)
constexpr int kGXLdsPerCu = 160 * 1024;
constexpr int kGXMaxWgPerCu = 4;                   // 16 waves per CU: 128 VGPRs per lane

// element E (compile time) of T bits (wave uniform) out of the normalised window n[0..7]: it sits at bit E * T, word (E * T) >> 5 <= E
template <int E>
static __device__ __forceinline__ uint32_t gx_elem(const uint32_t (&n)[8], int T, uint32_t mask) {
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

template <typename DT, int V, int RES, bool PERM>
__global__ __launch_bounds__(kGTThreads) void gemm_gatherx_kernel(const GemmGatherParams P) {
  static_assert(V == 8 || V == 16, "vector length");
  static_assert(RES >= 0 && RES <= 2, "residual: none, LDS, L2");
  constexpr int kRows = 16 / V;   // vector-rows per row group (16 outputs)
  constexpr int EB = V * 2;       // bytes per codebook entry
  extern __shared__ __attribute__((aligned(16))) unsigned char gx_smem[];
  u32x4* const tile = (u32x4*)gx_smem;                              // [chunk][16 outputs]: 32 KiB
  const unsigned char* const rtab = gx_smem + kGTTileBytes;         // RES = 1: the residual table
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int G = P.G, N = P.N, O = P.O, tokens = P.tokens;
  const int T = P.ib + P.rb, ib = P.ib;
  const uint32_t tmask = T >= 32 ? 0xffffffffu : ((1u << T) - 1u), mmask = (1u << ib) - 1u;
  // the 9th window word: 8 T bits + the largest offset (24, 16 or 0 bits: T odd, T % 4 == 2, T % 4 == 0) beyond 8 words (T = 31)
  const bool need9 = 8 * T + ((T & 1) ? 24 : (T & 2) ? 16 : 0) > 256;
  const int last = P.row_words - 1;
  const int n_tiles = (G + kGTTile - 1) / kGTTile;
  if constexpr (RES == 1) {
    const int n16 = P.res_bytes >> 4;
    for (int i = tid; i < n16; i += kGTThreads)
      *(u32x4*)(gx_smem + kGTTileBytes + (size_t)i * 16) = *(const u32x4*)(P.rcent + (size_t)i * 16);
    __syncthreads();
  }
  // dequant role: 8 consecutive columns (chunk dch) of 8 outputs: V = 8 vector-row dr of the group, V = 16 half dr of its one entry
  const int dr = tid >> 7, dch = tid & (kGTChunks - 1);
  const uint32_t hoff = V == 16 ? (uint32_t)dr * 16u : 0u;
  const uint32_t wslot = (uint32_t)(dch * 16 + dr * 8), wx = (uint32_t)(dch & 7);
  // MFMA role: lane (token / output mj, k group mkg); step i reads chunk 32 wave + 8 mkg + i
  const int mj = lane & 15, mkg = lane >> 4;
  const int mch0 = wave * 32 + mkg * 8;
  const uint16_t* const xrow = P.x + (size_t)(mj < tokens ? mj : tokens - 1) * G;

  for (int rg = blockIdx.x; rg < P.n_groups; rg += gridDim.x) {
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
      gather1(0, gx_elem<0>(n, T, tmask)); gather1(1, gx_elem<1>(n, T, tmask));
      gather1(2, gx_elem<2>(n, T, tmask)); gather1(3, gx_elem<3>(n, T, tmask));
      gather1(4, gx_elem<4>(n, T, tmask)); gather1(5, gx_elem<5>(n, T, tmask));
      gather1(6, gx_elem<6>(n, T, tmask)); gather1(7, gx_elem<7>(n, T, tmask));
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
      gt_load_a<PERM>(P.perm, xrow, G, mch0, t, xa);
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
      // ---- this wave's 8 K-steps (kept in this file: as a shared function it cost 3 - 8 % at 16 tokens, profiles/r17)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const bool live = mj < tokens && t * kGTTile + (mch0 + i) * 8 < G;
        const u32x4 a = {live ? xa[i][0] : 0u, live ? xa[i][1] : 0u, live ? xa[i][2] : 0u, live ? xa[i][3] : 0u};
        const u32x4 b = tile[(mch0 + i) * 16 + (mj ^ i)];   // ((mch0 + i) & 7 == i)
        acc = mfma16x16x32<DT>(a, b, acc);
      }
    }
    gt_epilogue<DT>(P, tid, lane, wave, (float*)gx_smem, rg, acc);
  }
}

// ---- host side -------------------------------------------------------------------
bool gemm_gatherx_eligible(const VptqLayerDesc& d, int tokens) {
  const int v = d.vector_len, T = d.index_bits + d.res_bits;
  return (v == 8 || v == 16) && d.num_codebooks == 1 && d.outlier_size == 0 && d.weight_scale != nullptr && d.weight_bias != nullptr &&
         d.group_size >= 8 && (d.group_size % 8) == 0 && d.group_size == d.in_features &&
         d.num_centroids >= 16384 && d.num_centroids <= 65536 && d.num_res_centroids >= 0 && d.num_res_centroids <= 65536 &&
         (d.num_res_centroids > 0) == (d.res_centroids != nullptr) && d.index_bits >= 14 && d.index_bits <= 16 && d.res_bits >= 0 &&
         T <= 32 && (long long)d.row_words * 32 >= (long long)d.group_size * T &&
         (long long)d.num_indices * v >= d.out_features && d.num_indices >= 1 && tokens >= 1 && tokens <= 16 &&
         (d.perm == nullptr || (d.scale_permuted != nullptr && d.bias_permuted != nullptr)) &&
         (((uintptr_t)d.indices | (uintptr_t)d.centroids | (uintptr_t)d.res_centroids) & 15) == 0 &&
         (((uintptr_t)d.weight_scale | (uintptr_t)d.weight_bias | (uintptr_t)d.scale_permuted |
           (uintptr_t)d.bias_permuted | (uintptr_t)d.perm) & 3) == 0 &&
         !gemm_gather_eligible(d, tokens);   // a layer has one batched-decode kernel
}

// what one launch IS: the template arguments of gemm_gatherx_kernel<DT, V, RES, PERM>, the run-time index widths and the launch
// shape, decided once for the launcher and for vptq_quant_gemm_gatherx_instance
GemmGatherXDecision gemm_gatherx_decide(const VptqLayerDesc& d, int tokens) {
  GemmGatherXDecision D = {};
  D.f16 = d.dtype == VPTQ_DTYPE_F16;
  D.perm = d.perm != nullptr;
  D.v = d.vector_len;
  D.ib = d.index_bits;
  D.rb = d.res_bits;
  D.res_bytes = d.num_res_centroids * d.vector_len * 2;
  D.res = D.res_bytes == 0 ? 0 : D.res_bytes <= kGXResLdsMax ? 1 : 2;
  D.tok = tokens;
  D.tiles = (d.group_size + kGTTile - 1) / kGTTile;
  D.lds = kGTTileBytes + (D.res == 1 ? D.res_bytes : 0);
  D.wgcu = kGXLdsPerCu / D.lds < kGXMaxWgPerCu ? kGXLdsPerCu / D.lds : kGXMaxWgPerCu;
  const GemmGatherGrid g = gemm_gather_grid(d.num_indices, 16 / (D.v == 16 ? 16 : 8), D.wgcu);
  D.n_groups = g.n_groups; D.grid = g.grid; D.rgs = g.rgs;
  return D;
}

template <typename DT, int V, int RES>
static hipError_t launch_gx(const GemmGatherParams& P, const GemmGatherXDecision& D, hipStream_t st) {
  const dim3 grid(D.grid), block(kGTThreads);
  if (D.perm) hipLaunchKernelGGL((gemm_gatherx_kernel<DT, V, RES, true>), grid, block, D.lds, st, P);
  else hipLaunchKernelGGL((gemm_gatherx_kernel<DT, V, RES, false>), grid, block, D.lds, st, P);
  return hipGetLastError();
}

template <typename DT, int V>
static hipError_t launch_gx_v(const GemmGatherParams& P, const GemmGatherXDecision& D, hipStream_t st) {
  switch (D.res) {
    case 0: return launch_gx<DT, V, 0>(P, D, st);
    case 1: return launch_gx<DT, V, 1>(P, D, st);
    case 2: return launch_gx<DT, V, 2>(P, D, st);
    default: return hipErrorInvalidValue;
  }
}

template <typename DT>
static hipError_t launch_gx_dt(const GemmGatherParams& P, const GemmGatherXDecision& D, hipStream_t st) {
  switch (D.v) {
    case 8: return launch_gx_v<DT, 8>(P, D, st);
    case 16: return launch_gx_v<DT, 16>(P, D, st);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_gemm_gatherx(const VptqLayerDesc& d, const void* x, void* y, int tokens, bool out_f32, hipStream_t st) {
  const GemmGatherXDecision D = gemm_gatherx_decide(d, tokens);
  if (D.grid < 1 || tokens < 1 || tokens > 16 || D.lds > 65536) return hipErrorInvalidValue;
  GemmGatherParams P = gemm_gather_params(d, x, y, tokens, out_f32, D.n_groups);
  P.ib = D.ib; P.rb = D.rb; P.res_bytes = D.res_bytes;   // (the table copied into LDS is the one D.lds has room for)
  return D.f16 ? launch_gx_dt<F16>(P, D, st) : launch_gx_dt<BF16>(P, D, st);
}

}  // namespace vptq
