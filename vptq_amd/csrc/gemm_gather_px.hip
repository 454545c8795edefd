// Batched decode of layers with a column permutation (vptq_quant_gemm_gather_px): x is gathered ONCE per call into a workspace,
// xp[t][c] = x[t][perm[c]], and the layer's batched-decode kernel then runs in the form it has for layers without a permutation.
//
// gemm_gather / gemm_gatherx (1 - 16 tokens) and gemm_gatherw (17 - 48) read a permuted x two bytes at a time in EVERY row group of 16
// outputs (gt_load_a / gt_load_a1 of gemm_gather_tile.h: 8 x 8 scalar loads per lane, token block and tile), which costs 1.8 - 6.8
// times the dense route's time and 256 - 328 registers (profiles/r23/table_perm.md).  The kernels' plain forms read the same values
// as 16-byte loads when they are given xp for x, scale_permuted / bias_permuted for scale / bias and no permutation: the clamped
// tail columns (G - 8) and the clamped token rows hold in xp what the permuted forms reach through perm, so the output BITS are
// those of the layer's own entry on the same descriptor.
//
// The permute launch (the chain launch's permute_x_kernel of gemv_k256c.hip is per layer and one token):
//  * a thread owns 8 consecutive columns (16 bytes of perm, loaded once) and a slice of kPxTok tokens; a workgroup is one wave.
//  * per token eight 2-byte gathers through the uniform base of x + a 32-bit lane offset (gt_load_a1's addressing; x is at most 48
//    rows), all tokens of the slice requested before the first store: kPxTok x 8 independent loads in flight.
//  * one 16-byte store per token; a wave writes 1 KiB of consecutive bytes of a row of xp.
//  * grid: (G / 8 chunks in waves of 64) x (token slices) - 17 tokens of 4096 columns are 8 x 5 workgroups.
// No LDS, no scratch memory beside xp, plain vector stores.  Rows of xp from `tokens` on are not written (and not read: the plain
// kernels clamp to the last token).
#include "common.h"
#include "kernels.h"
#include "launch.h"

namespace vptq {

constexpr int kPxThreads = 64;   // chunks of 8 columns per workgroup
constexpr int kPxTok = 4;        // tokens per thread

struct PermuteXTokParams {
  const uint16_t* x;      // [tokens][G]
  const uint16_t* perm;   // [G], 4-byte aligned
  uint16_t* xp;           // [tokens][G], 16-byte aligned
  int G, tokens;
};

__global__ __launch_bounds__(kPxThreads) void permute_x_tokens_kernel(const PermuteXTokParams P) {
  const int chunk = blockIdx.x * kPxThreads + threadIdx.x;
  if (chunk * 8 >= P.G) return;
  const int t0 = blockIdx.y * kPxTok;
  const u32x4_a4 pv = *(const u32x4_a4*)(P.perm + (size_t)chunk * 8);
  const char* const xb = (const char*)P.x;
  const uint32_t row_bytes = (uint32_t)P.G * 2u;
  u32x4 v[kPxTok];
#pragma unroll
  for (int j = 0; j < kPxTok; ++j) {
    // (a slice's rows past the last token read the last token's: every address stays inside x; they are not stored)
    const int t = t0 + j < P.tokens ? t0 + j : P.tokens - 1;
    const uint32_t rowoff = (uint32_t)t * row_bytes;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t lo = *(const uint16_t*)(xb + (rowoff + 2u * (pv[q] & 0xffffu)));
      const uint32_t hi = *(const uint16_t*)(xb + (rowoff + 2u * (pv[q] >> 16)));
      v[j][q] = lo | (hi << 16);
    }
  }
#pragma unroll
  for (int j = 0; j < kPxTok; ++j)
    if (t0 + j < P.tokens) *(u32x4*)((char*)P.xp + ((uint32_t)(t0 + j) * row_bytes + (uint32_t)chunk * 16u)) = v[j];
}

// ---- host side -------------------------------------------------------------------
// bytes of xp: tokens rows of group_size 16-bit values, rounded up to 256; 0 without a permutation
size_t gemm_gather_px_workspace_bytes(const VptqLayerDesc& d, int tokens) {
  if (!d.perm || tokens < 1) return 0;
  return ((size_t)tokens * (size_t)d.group_size * 2 + 255) & ~(size_t)255;
}

// what the permute launch IS: its grid, decided once for the launcher and for vptq_quant_gemm_gather_px_instance
GemmGatherPxDecision gemm_gather_px_decide(const VptqLayerDesc& d, int tokens) {
  GemmGatherPxDecision D = {};
  D.perm = d.perm != nullptr;
  D.g = d.group_size;
  D.tok = tokens;
  D.tpt = kPxTok;
  D.grid_x = (d.group_size / 8 + kPxThreads - 1) / kPxThreads;
  D.grid_y = (tokens + kPxTok - 1) / kPxTok;
  return D;
}

// the layer as its batched-decode kernel sees it behind the permute launch: the quantised matrix's own column order - scale and
// bias in that order, no permutation
VptqLayerDesc gemm_gather_px_plain(const VptqLayerDesc& d) {
  VptqLayerDesc p = d;
  if (d.perm) {
    p.weight_scale = d.scale_permuted;
    p.weight_bias = d.bias_permuted;
    p.perm = nullptr;
    p.inv_perm = nullptr;
    p.scale_permuted = nullptr;
    p.bias_permuted = nullptr;
  }
  return p;
}

hipError_t launch_permute_x_tokens(const VptqLayerDesc& d, const void* x, void* xp, int tokens, hipStream_t st) {
  const GemmGatherPxDecision D = gemm_gather_px_decide(d, tokens);
  if (!D.perm || tokens < 1 || D.g < 8 || D.g % 8 || D.grid_x < 1 || D.grid_y < 1) return hipErrorInvalidValue;
  PermuteXTokParams P = {};
  P.x = (const uint16_t*)x;
  P.perm = d.perm;
  P.xp = (uint16_t*)xp;
  P.G = D.g;
  P.tokens = tokens;
  hipLaunchKernelGGL(permute_x_tokens_kernel, dim3(D.grid_x, D.grid_y), dim3(kPxThreads), 0, st, P);
  return hipGetLastError();
}

}  // namespace vptq
