// dequant.hip's launch decision and the per-thread path predicates of dequant_kernel, each stated once: the kernel evaluates them
// on the device, vptq_dequant_instance (dequant.hip:dequant_instance) on the host over the chunks of one vector-row - the text
// cannot say anything else than what the kernel does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vptq_hip.h"

namespace vptq {

constexpr int kDqLdsMax = 16384;       // bytes of codebook a workgroup copies into LDS
constexpr int kDqBlockCols = 2048;     // output columns per workgroup: 256 threads x one chunk of 8

// What one launch IS: the template arguments of dequant_kernel<DT, V, TAB> and the launch shape.  TAB 1: one codebook group whose
// two tables together fit kDqLdsMax - both in LDS; TAB 2: only the residual table fits - it alone in LDS; TAB 0: both gathered
// through L1 / L2.  Read by launch_dequant and printed by dequant_instance.
struct DequantDecision {
  bool f16;
  int v, tab, lds, col_blocks;   // lds: dynamic LDS bytes; col_blocks: workgroups along one vector-row
  long long blocks;              // col_blocks x vector-rows
};
inline DequantDecision dequant_decide(const VptqLayerDesc& d) {
  DequantDecision D = {};
  D.f16 = d.dtype == VPTQ_DTYPE_F16;
  D.v = d.vector_len;
  D.col_blocks = (d.in_features + kDqBlockCols - 1) / kDqBlockCols;
  D.blocks = (long long)D.col_blocks * d.num_indices;
  const int tab_bytes = (d.num_centroids + d.num_res_centroids) * d.vector_len * 2;
  const int res_bytes = d.num_res_centroids * d.vector_len * 2;
  if (d.num_codebooks == 1 && tab_bytes <= kDqLdsMax) { D.tab = 1; D.lds = tab_bytes; }
  else if (d.num_codebooks == 1 && res_bytes > 0 && res_bytes <= kDqLdsMax) { D.tab = 2; D.lds = res_bytes; }
  else { D.tab = 0; D.lds = 0; }
  return D;
}

// ---- one thread = the chunk of 8 output columns j0 .. j0 + 7 of one vector-row ----
// the whole chunk inside the row, and rows a multiple of 16 bytes (so a 16-byte aligned tensor is 16-byte aligned at every chunk)
__host__ __device__ inline bool dq_full(int j0, int I) { return j0 + 8 <= I && (I & 7) == 0; }
// scale / bias of the 8 columns as two 16-byte loads
__host__ __device__ inline bool dq_vec_norm(const VptqLayerDesc& d, bool full) {
  return full && d.weight_scale != nullptr && ((((uintptr_t)d.weight_scale | (uintptr_t)d.weight_bias) & 15) == 0);
}
// the V rows of the chunk as 16-byte stores (rows are 2 I bytes, I % 8 == 0: W's alignment is every row's)
__host__ __device__ inline bool dq_vec_store(const void* W, bool full) { return full && (((uintptr_t)W) & 15) == 0; }
// the chunk's 8 index elements are contiguous in the bit stream: no permutation, no outlier columns, group ends on chunk ends
__host__ __device__ inline bool dq_contiguous(const VptqLayerDesc& d, bool full) {
  return full && !d.inv_perm && d.outlier_size == 0 && (d.group_size & 7) == 0;
}
// ... and 16 bits wide: one aligned 16-byte piece of the row
__host__ __device__ inline bool dq_vec_idx(const VptqLayerDesc& d, bool full, int T) {
  return dq_contiguous(d, full) && T == 16 && ((((uintptr_t)d.indices) & 15) == 0) && ((d.row_words & 3) == 0);
}
// ... any other width: two windows of 4 elements, each one 16-byte load at 4-byte alignment (+ a fifth word)
__host__ __device__ inline bool dq_win_form(const VptqLayerDesc& d, bool full, int T) { return dq_contiguous(d, full) && T != 16; }
// ... unless the second window (4 T bits from element g + 4 of the group's row, 5 words fetched at most) would run past the row
// end - the last chunk(s) of a row: element by element instead
__host__ __device__ inline bool dq_win_in_row(int g, int T, int row_words) {
  const uint32_t bit1 = (uint32_t)(g + 4) * (uint32_t)T;
  return (int)(bit1 >> 5) + 5 <= row_words;
}
// some lane's window of 4 T bits reaches a fifth word: a property of T (27, 29, 30, 31)
__host__ __device__ inline bool dq_need5(int T) {
  const int g32 = (4 * T) & -(4 * T) & 31 ? ((4 * T) & -(4 * T)) : 32;
  return 4 * T > 96 + g32;
}

}  // namespace vptq
