// The phases of the tile pipeline that gemm_gather.hip and gemm_gatherx.hip (batched decode of the large-codebook formats, 1 - 16 tokens
// per launch) share, as inlined device functions: the A-operand load, the rebuild, the transposition and tile write, the epilogue,
// scale / bias loads and the MFMA wrapper.  Each kernel keeps its own index path, gather, loop skeleton and the 8-step MFMA loop (as a
// shared function that loop cost 3 - 8 % at 16 tokens of 8192 x 8192 layers: profiles/r17/README.md).
//
// Structure of both kernels (gemm_k256.hip with the LDS codebook image replaced by L2 gathers; kGTThreads = 256 threads):
//  * a workgroup owns row groups of 16 outputs (one MFMA N block) over ALL input columns: no split-K, no atomics, no workspace, no
//    scratch; row groups blockIdx.x, + gridDim.x, ...
//  * it walks column tiles of kGTTile = 1024 columns.  A thread owns 8 consecutive columns (chunk dch) of 8 outputs (half dr of the
//    group): it reads their index bits and issues all 8 centroid gathers (+ 8 residual gathers or LDS reads) - the kernel's own part -
//    and rebuilds the weights with the reference's roundings, w = r16(r16(r16(c + r) * s) + b) - bit-identical to vptq_dequant (bf16:
//    BF16::add4 / scale_bias4, see common.h): gt_rebuild.
//  * after an in-register 8 x 8 transposition (16 v_perm_b32) the thread holds, for each of its 8 outputs, the 8 consecutive-k values
//    one lane of the 16x16x32 MFMA supplies as B operand: 8 ds_write_b128 into the tile [column chunk][output][16 bytes], the
//    output slot XOR-ed with the chunk's low bits so that the 8 lanes of a write group cover all 32 banks; the B reads
//    (ds_read_b128, 16 outputs of a chunk contiguous) are conflict free: gt_write_tile.
//  * MFMA phase (gt_load_a, then the kernel's own loop over mfma16x16x32): the tile's 32 K-steps are dealt to the 4 waves; lane (token, k group kg) of wave w takes
//    chunk 32 w + 8 kg + i in step i, so that its 8 A operands (raw x, loaded from L2) are 64 CONSECUTIVE columns - one 128-byte line
//    per token (gemm_k256.hip: K-steps of adjacent columns cost 4x the L2 traffic).  Token rows past `tokens` are zero.
//  * the gathers of tile t + 1 are issued before the MFMA phase of tile t, its index words and scale / bias one tile earlier; two
//    barriers per tile.
//  * at the end of a row group the 4 waves' partial D meet in LDS and are added in wave order: two launches give the same bits.
//    The sum is rounded once; the output bias is added in fp32: gt_epilogue.
// Tiles past the end of a row clamp to its last chunk and are masked (dvalid / live): every address stays inside the layer.
#pragma once
#include <type_traits>

#include "common.h"
#include "gemm_gather_host.h"
#include "kernels.h"

namespace vptq {

constexpr int kGTThreads = 256;
constexpr int kGTTile = 1024;                      // columns per tile: kGTThreads / 2 chunks of 8
constexpr int kGTChunks = kGTTile / 8;
constexpr int kGTTileBytes = kGTChunks * 16 * 16;  // [chunk][16 outputs][16 bytes]: 32 KiB

// first column of chunk dch of tile t (tiles past the end clamp to the last chunk of the row)
static __device__ __forceinline__ int gt_dcol(int t, int dch, int G) { const int c = t * kGTTile + dch * 8; return c < G ? c : G - 8; }

// scale / bias of the 8 columns from column col on
static __device__ __forceinline__ void gt_load_sb(const GemmGatherParams& P, int col, uint32_t (&s)[4], uint32_t (&b)[4]) {
  const uint32_t* s32 = (const uint32_t*)(P.scale + col);
  const uint32_t* b32 = (const uint32_t*)(P.wbias + col);
#pragma unroll
  for (int q = 0; q < 4; ++q) { s[q] = s32[q]; b[q] = b32[q]; }
}

// tile t's A operands: 8 x 16 bytes of x, 64 consecutive columns of one token
template <bool PERM>
static __device__ __forceinline__ void gt_load_a(const uint16_t* perm, const uint16_t* xrow, int G, int mch0, int t, u32x4 (&xa)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int col = t * kGTTile + (mch0 + i) * 8;
    const int cc = col < G ? col : G - 8;
    if constexpr (PERM) {
      const uint32_t* p32 = (const uint32_t*)(perm + cc);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t pv = p32[q];
        xa[i][q] = (uint32_t)xrow[pv & 0xffffu] | ((uint32_t)xrow[pv >> 16] << 16);
      }
    } else {
      xa[i] = *(const u32x4*)(xrow + cc);
    }
  }
}

// one K-step of gt_load_a for gemm_gatherw.hip, which requests the A operands of its later token blocks step by step: the 16 bytes
// of x from column col on (clamped as above) of the token row that starts rowoff BYTES into x.  Addresses are the uniform base plus
// a 32-bit lane offset (x is at most 48 rows): one address register per load where a per-lane row pointer takes two - with a
// permutation that is 8 loads a step, and what keeps that kernel's permuted forms under 256 registers.
template <bool PERM>
static __device__ __forceinline__ u32x4 gt_load_a1(const uint16_t* perm, const uint16_t* x, uint32_t rowoff, int G, int col) {
  const int cc = col < G ? col : G - 8;
  const char* const xb = (const char*)x;
  if constexpr (PERM) {
    const uint32_t* p32 = (const uint32_t*)((const char*)perm + (uint32_t)(cc * 2));
    u32x4 a;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t pv = p32[q];
      const uint32_t lo = *(const uint16_t*)(xb + (rowoff + 2u * (pv & 0xffffu)));
      const uint32_t hi = *(const uint16_t*)(xb + (rowoff + 2u * (pv >> 16)));
      a[q] = lo | (hi << 16);
    }
    return a;
  } else {
    return *(const u32x4*)(xb + (rowoff + (uint32_t)(cc * 2)));
  }
}

// rebuild 8 columns x 8 outputs in place: c + r, * s, + b, each rounded to 16 bits; columns past the row end become 0
template <typename DT, bool RES>
static __device__ __forceinline__ void gt_rebuild(u32x4 (&cv)[8], const u32x4 (&rv)[RES ? 8 : 1], const uint32_t (&sp)[4],
                                                  const uint32_t (&bp)[4], bool dvalid) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    uint32_t v[4] = {cv[e][0], cv[e][1], cv[e][2], cv[e][3]};
    if constexpr (RES) {
      const uint32_t r[4] = {rv[e][0], rv[e][1], rv[e][2], rv[e][3]};
      DT::add4(v, r);
    }
    DT::scale_bias4(v, sp[e >> 1], e & 1, bp[e >> 1], e & 1);
#pragma unroll
    for (int p = 0; p < 4; ++p) cv[e][p] = dvalid ? v[p] : 0u;
  }
}

// transpose to 8 outputs x 8 k values and write them in B-operand order
static __device__ __forceinline__ void gt_write_tile(u32x4* tile, uint32_t wslot, uint32_t wx, const u32x4 (&cv)[8]) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const u32x4 lo = {__builtin_amdgcn_perm(cv[1][p], cv[0][p], 0x05040100u), __builtin_amdgcn_perm(cv[3][p], cv[2][p], 0x05040100u),
                      __builtin_amdgcn_perm(cv[5][p], cv[4][p], 0x05040100u), __builtin_amdgcn_perm(cv[7][p], cv[6][p], 0x05040100u)};
    const u32x4 hi = {__builtin_amdgcn_perm(cv[1][p], cv[0][p], 0x07060302u), __builtin_amdgcn_perm(cv[3][p], cv[2][p], 0x07060302u),
                      __builtin_amdgcn_perm(cv[5][p], cv[4][p], 0x07060302u), __builtin_amdgcn_perm(cv[7][p], cv[6][p], 0x07060302u)};
    tile[wslot + ((uint32_t)(2 * p) ^ wx)] = lo;
    tile[wslot + ((uint32_t)(2 * p + 1) ^ wx)] = hi;
  }
}

// the 4 waves' partial D of row group rg, added in wave order; D element (token = (l >> 4) * 4 + reg, output = l & 15)
template <typename DT>
static __device__ __forceinline__ void gt_epilogue(const GemmGatherParams& P, int tid, int lane, int wave, float* scr, int rg, f32x4 acc) {
  const int O = P.O, tokens = P.tokens;
  __syncthreads();
  // scr [wave][reg][lane]: the tile's first 4 KiB
#pragma unroll
  for (int r = 0; r < 4; ++r) scr[(wave * 4 + r) * 64 + lane] = acc[r];
  __syncthreads();
  const int r = tid >> 6, l = tid & 63;
  float sum = scr[r * 64 + l];
#pragma unroll
  for (int w = 1; w < 4; ++w) sum += scr[(w * 4 + r) * 64 + l];
  const int token = (l >> 4) * 4 + r;
  const int o = rg * 16 + (l & 15);
  if (token < tokens && o < O) {
    if (P.bias) sum += DT::to_float(P.bias[o]);
    if (P.out_f32) ((float*)P.y)[(size_t)token * O + o] = sum;
    else ((uint16_t*)P.y)[(size_t)token * O + o] = DT::from_float(sum);
  }
}

}  // namespace vptq
