// What gemm_gather.hip and gemm_gatherx.hip (batched decode of the large-codebook formats, 1 - 16 tokens per launch) share on the
// host side: the kernels' argument block, how it is filled from a layer, and the launch-shape arithmetic.
#pragma once
#include "common.h"
#include "kernels.h"

namespace vptq {

struct GemmGatherParams {
  const uint32_t* idx;    // [N][row_words]
  const char* cent;       // [k][V] 2 V bytes per entry
  const char* rcent;      // [kr][V] or NULL
  const uint16_t* x;      // [tokens][G]
  void* y;                // [tokens][O]
  const uint16_t* scale;  // [G] column order
  const uint16_t* wbias;  // [G] column order
  const uint16_t* bias;   // [O] or NULL
  const uint16_t* perm;   // [G] or NULL
  int N, G, O, row_words, tokens, out_f32, n_groups;
  int ib, rb, res_bytes;  // gemm_gatherx: index widths; bytes of the residual table (RES = 1: copied into LDS)
};

// the launch shape: one workgroup per row group of rows_per_group vector-rows, up to wg_per_cu workgroups per CU; rgs: the most
// row groups one workgroup walks
struct GemmGatherGrid { int n_groups, grid, rgs; };
inline GemmGatherGrid gemm_gather_grid(int num_indices, int rows_per_group, int wg_per_cu) {
  GemmGatherGrid g = {};
  g.n_groups = (num_indices + rows_per_group - 1) / rows_per_group;
  const int slots = device_cus() * wg_per_cu;
  g.grid = g.n_groups < slots ? g.n_groups : slots;
  g.rgs = g.grid > 0 ? (g.n_groups + g.grid - 1) / g.grid : 0;
  return g;
}

// the kernels' argument block for (layer, x, y, tokens); ib / rb / res_bytes are gemm_gatherx's, set by its launcher from its decision
inline GemmGatherParams gemm_gather_params(const VptqLayerDesc& d, const void* x, void* y, int tokens, bool out_f32, int n_groups) {
  GemmGatherParams P = {};
  P.idx = (const uint32_t*)d.indices;
  P.cent = (const char*)d.centroids;
  P.rcent = d.num_res_centroids > 0 ? (const char*)d.res_centroids : nullptr;
  P.x = (const uint16_t*)x;
  P.y = y;
  P.scale = (const uint16_t*)(d.perm ? d.scale_permuted : d.weight_scale);
  P.wbias = (const uint16_t*)(d.perm ? d.bias_permuted : d.weight_bias);
  P.bias = (const uint16_t*)d.bias;
  P.perm = d.perm;
  P.N = d.num_indices; P.G = d.group_size; P.O = d.out_features; P.row_words = d.row_words;
  P.tokens = tokens; P.out_f32 = out_f32 ? 1 : 0;
  P.n_groups = n_groups;
  return P;
}

}  // namespace vptq
