// Dequantise a layer to the dense W[O, I] straight from its EXACT sliced layout(s) (vptq_dequant_sliced, include/vptq_hip.h):
// what vptq_sliced_layout_repack + vptq_dequant compute, bit for bit, without the packed stream in between - a compacted
// layer's many-token route (vptq_amd/layers/vqlinear.py:_dense_cached) and its dequant().
//
// An element word carries `column | local << 16`; the (slice, row) list it sits in gives the rest of the main index,
// index = slice << slice_bits | local; the residual index rides beside it in the `res` side stream (uint8 / uint16); part p adds
// its first column.  Column g of the quantised matrix is column j = perm[g] of W (W[o, j] = Wq[o, argsort(perm)[j]] s[j] + b[j]):
// the kernel reads `perm`, never the inverse.  The v weights of an element are add2(mul2(add2(c, r), s[j]), b[j]) in dequant.hip's
// widened 16-bit helpers, each step rounded to 16 bits - so the steps may be split between the two phases below.
//
// One workgroup per vector-row n and column tile.  An element's v weights belong to v different rows of W at ONE column, and a
// list's elements come in bucket order: stored directly they would be v scattered 2-byte writes.  So the tile is assembled in
// LDS first, column-major - 16 bytes (8 halves of f16(c + r)) per column and plane of 8 rows, v / 8 planes:
//   gather: every wave walks whole (part, slice) lists of row n (short ones: a share of one), 4 elements per lane and 16-byte
//           element load; per element whose j falls in the tile one 16 / 32-byte gather of the main entry from device memory (the
//           table's slices are LDS-local only per (slice, row block), the wrong cut for a row image), the residual entry from
//           LDS (tables <= 16 KiB, as dequant.hip's TAB = 2) or from device memory, one ds_write_b128 per plane.  Without a
//           permutation the lists' window order (`wstart`) bounds the walk to the windows that meet the tile, and lists of a part
//           that does not meet it are skipped; with one the filter on j is the only way.
//   store : after the barrier every thread takes 8 consecutive columns of a plane: 8 ds_read_b128, scale and bias of the 8
//           columns as two 16-byte loads, the in-register transposition of dequant.hip and 8 stores of 16 bytes - a wave writes
//           1 KiB contiguous per W row.  Rows past out_features are not stored.
// Every column of a row occurs in exactly one element, so a tile is fully written: nothing is zeroed, and no result depends on
// what LDS or W held before.  LDS slot of tile column c: c ^ ((c >> 3) & 15) - the 16 lanes of a ds_read_b128 group read columns
// 8 apart (128 bytes: 2 distinct banks quads without the swizzle); XOR-ing the chunk number into the low 4 bits gives 16 distinct.
//
// Tile: the row's columns in equal tiles of a multiple of 128 columns, at most 8192 (v = 8) / 4096 (v = 16) = 128 KiB of image
// (+ <= 16 KiB residual table).  1024 threads.  Occupancy: one workgroup = 16 waves per CU, 4 per SIMD, wherever the tile holds
// more than 80 KiB (rows wider than 4096 columns, v = 16: 2048) - the next workgroup's gathers then do not overlap this one's
// stores - and for every bf16 instantiation (78 VGPRs; v = 16 with a residual stream: 91); the fp16 ones take 60 VGPRs and run
// two workgroups = 32 waves per CU on narrower rows.  VPTQ_DQS_TILE (tuning knob): another largest tile.
// Measured (profiles/r12, us per layer against repack + vptq_dequant of the same session): 4096 x 4096 19.8 against 28.1 (v8-k65536-256,
// fp16), every format and dtype 0.69 - 0.87 of it; from 8192 columns on the two phases of the one resident workgroup do not overlap
// and the kernel runs at 1.2 - 1.7 TB/s of W: level with the repack route (0.96 - 1.05) for the residual formats, behind it without
// a residual codebook and for v = 16 (1.02 - 1.27).  Smaller tiles (4096, 2048 columns) measured no better.  The module routes by that
// (vptq_amd/layers/vqlinear.py:_dense_from_layout).
#include "common.h"
#include "kernels.h"

namespace vptq {

namespace {

constexpr int kDSThreads = 1024;
constexpr int kDSWaves = kDSThreads / 64;
constexpr int kDSMaxLds = 163840;
constexpr int kDSImageMax = 131072;   // bytes of image per workgroup
constexpr int kDSResLdsMax = 16384;   // residual tables up to this size are staged in LDS

struct DSPart {
  const uint4* elems;
  const int32_t* blocks;   // [S][N]
  const int32_t* first;    // [S][N]
  const int32_t* wstart;   // [S][N][VPTQ_SLICED_WINDOWS + 1], or NULL
  const void* res;         // uint8 / uint16 per element, or NULL
  int n_slices, slice_bits, c0, width, wcols;
};

struct DSArgs {
  DSPart part[3];
  const uint32_t* cent;     // [k][v] halves
  const uint32_t* rcent;    // [kr][v] halves, or NULL
  const uint16_t* perm;     // column g of the quantised matrix is column perm[g] of W, or NULL
  const uint16_t* scale;    // [I], W's column order
  const uint16_t* wbias;
  uint16_t* W;
  int parts, N, I, O, tile, tiles, img_cols;   // img_cols: the tile rounded up to 128 columns (the swizzle's block)
  uint32_t kmask, krmask;
};

__device__ __forceinline__ uint32_t ds_slot(uint32_t c) { return c ^ ((c >> 3) & 15u); }

// SIDE: the residual side stream - 0 none, 1 uint8, 2 uint16; RLDS: the residual table sits in LDS behind the image
template <typename DT, int V, int SIDE, bool RLDS>
__global__ __launch_bounds__(kDSThreads) void dequant_sliced_kernel(const DSArgs a) {
  constexpr int PL = V / 8;   // planes of 8 rows
  extern __shared__ __attribute__((aligned(16))) u32x4 ds_img[];   // [PL][img_cols] | residual table
  const int n = blockIdx.x / a.tiles;
  const int j0 = (blockIdx.x - n * a.tiles) * a.tile;
  const int tcols = min(a.tile, a.I - j0);
  const u32x4* rtab = ds_img + (size_t)PL * a.img_cols;
  if constexpr (RLDS) {
    const int n16 = (int)(a.krmask + 1u) * PL;
    u32x4* dst = ds_img + (size_t)PL * a.img_cols;
    for (int i = threadIdx.x; i < n16; i += kDSThreads) dst[i] = reinterpret_cast<const u32x4*>(a.rcent)[i];
    __syncthreads();
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nsl = a.part[0].n_slices;   // (every part has the same slice count)
  const int lists = a.parts * nsl;
  const int nsub = lists < kDSWaves ? kDSWaves / lists : 1;   // waves that share one list
  for (int u = wave; u < lists * nsub; u += kDSWaves) {
    const int L = u / nsub, sub = u - L * nsub;
    const int p = L / nsl, s = L - p * nsl;
    const DSPart& P = a.part[p];
    const size_t sn = (size_t)s * a.N + n;
    const int nb = P.blocks[sn];
    int c_lo = 0, c_hi = nb * 16;   // the list in pieces of 4 elements
    if (!a.perm) {
      // no permutation: j = c0 + column.  The tile in the part's own columns; a part that does not meet it has nothing for us
      const int lo = max(j0 - P.c0, 0), hi = min(j0 + tcols - P.c0, P.width);
      if (lo >= hi) continue;
      if (P.wstart) {   // lists ordered by column window: only the windows that meet [lo, hi)
        const int w0 = min(lo / P.wcols, VPTQ_SLICED_WINDOWS - 1), w1 = min((hi - 1) / P.wcols, VPTQ_SLICED_WINDOWS - 1);
        const int32_t* ws = P.wstart + sn * (VPTQ_SLICED_WINDOWS + 1);
        c_lo = max(ws[w0] >> 2, 0);
        c_hi = min((ws[w1 + 1] + 3) >> 2, c_hi);
      }
    }
    const size_t e0 = (size_t)P.first[sn] * 64;
    const uint32_t hi_bits = (uint32_t)s << P.slice_bits;
    for (int c = c_lo + lane + 64 * sub; c < c_hi; c += 64 * nsub) {
      const size_t e = e0 + (size_t)c * 4;
      const uint4 w = P.elems[e >> 2];
      uint32_t r[4] = {0, 0, 0, 0};
      if constexpr (SIDE == 1) {
        const uint32_t b = *reinterpret_cast<const uint32_t*>((const uint8_t*)P.res + e);
        r[0] = b & 0xffu; r[1] = (b >> 8) & 0xffu; r[2] = (b >> 16) & 0xffu; r[3] = b >> 24;
      } else if constexpr (SIDE == 2) {
        const uint2 b = *reinterpret_cast<const uint2*>((const uint16_t*)P.res + e);
        r[0] = b.x & 0xffffu; r[1] = b.x >> 16; r[2] = b.y & 0xffffu; r[3] = b.y >> 16;
      }
      const uint32_t wd[4] = {w.x, w.y, w.z, w.w};
      // the four elements' columns first, then their gathers together, then the LDS stores
      int jl[4];
      bool ok[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int col = (int)(wd[k] & 0xffffu);
        ok[k] = col < P.width;   // (padding: column = part width)
        int j = P.c0 + (ok[k] ? col : 0);
        if (a.perm && ok[k]) j = a.perm[j];
        jl[k] = j - j0;
        ok[k] = ok[k] && (unsigned)jl[k] < (unsigned)tcols;
      }
      u32x4 cv[4][PL];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int q = 0; q < PL; ++q) cv[k][q] = u32x4{0, 0, 0, 0};
        if (ok[k]) {
          const u32x4* cp = reinterpret_cast<const u32x4*>(a.cent) + (size_t)((hi_bits | (wd[k] >> 16)) & a.kmask) * PL;
#pragma unroll
          for (int q = 0; q < PL; ++q) cv[k][q] = cp[q];
        }
      }
      if constexpr (SIDE != 0) {
        u32x4 rv[4][PL];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
          for (int q = 0; q < PL; ++q) rv[k][q] = u32x4{0, 0, 0, 0};
          if (ok[k]) {
            const u32x4* rp = (RLDS ? rtab : reinterpret_cast<const u32x4*>(a.rcent)) + (size_t)(r[k] & a.krmask) * PL;
#pragma unroll
            for (int q = 0; q < PL; ++q) rv[k][q] = rp[q];
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int q = 0; q < PL; ++q)
#pragma unroll
            for (int i = 0; i < 4; ++i) cv[k][q][i] = DT::add2(cv[k][q][i], rv[k][q][i]);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!ok[k]) continue;
        const uint32_t slot = ds_slot((uint32_t)jl[k]);
#pragma unroll
        for (int q = 0; q < PL; ++q) ds_img[(size_t)q * a.img_cols + slot] = cv[k][q];
      }
    }
  }
  __syncthreads();
  // store: (plane, 8 columns) per thread; I is a multiple of 8 (the layouts' rule), so every chunk is whole and 16-byte aligned
  const int chunks = tcols >> 3;
  for (int t = threadIdx.x; t < chunks * PL; t += kDSThreads) {
    const int q = t / chunks, ch = t - q * chunks;
    const int j = j0 + ch * 8;
    const u32x4 sv8 = *reinterpret_cast<const u32x4*>(a.scale + j);
    const u32x4 bv8 = *reinterpret_cast<const u32x4*>(a.wbias + j);
    u32x4 w2[8];   // [column][row pair]
#pragma unroll
    for (int k = 0; k < 8; ++k) w2[k] = ds_img[(size_t)q * a.img_cols + ds_slot((uint32_t)(ch * 8 + k))];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint32_t s2 = splat16((uint16_t)(sv8[k >> 1] >> (16 * (k & 1))));
      const uint32_t b2 = splat16((uint16_t)(bv8[k >> 1] >> (16 * (k & 1))));
#pragma unroll
      for (int i = 0; i < 4; ++i) w2[k][i] = DT::add2(DT::mul2(w2[k][i], s2), b2);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int o = n * V + q * 8 + 2 * i + h;
        if (o >= a.O) continue;
        u32x4 row;   // row o of the 8 columns: the low (h = 0) or high halves of w2[0..7][i]
#pragma unroll
        for (int k = 0; k < 4; ++k) row[k] = __builtin_amdgcn_perm(w2[2 * k + 1][i], w2[2 * k][i], h ? 0x07060302u : 0x05040100u);
        *reinterpret_cast<u32x4*>(a.W + (size_t)o * a.I + j) = row;
      }
    }
  }
}

// largest tile in columns for vector length v: the image of 2 v bytes per column within kDSImageMax
int ds_max_tile(int v) {
  static const int knob = tune_int("VPTQ_DQS_TILE", 0);   // columns of the largest v = 8 tile (v = 16: half), A/B
  int t = kDSImageMax / (2 * v);
  if (knob >= 128) t = min(t, knob * 8 / v);
  return max(t / 128 * 128, 128);
}

template <typename DT, int V, int SIDE, bool RLDS>
hipError_t ds_launch(const DSArgs& a, size_t lds, hipStream_t st) {
  if (const hipError_t e = allow_dynamic_lds<dequant_sliced_kernel<DT, V, SIDE, RLDS>>(kDSMaxLds); e != hipSuccess) return e;
  hipLaunchKernelGGL((dequant_sliced_kernel<DT, V, SIDE, RLDS>), dim3((unsigned)(a.N * a.tiles)), dim3(kDSThreads), lds, st, a);
  return hipGetLastError();
}

template <typename DT, int V>
hipError_t ds_launch_v(const DSArgs& a, int side, bool rlds, size_t lds, hipStream_t st) {
  if (side == 0) return ds_launch<DT, V, 0, false>(a, lds, st);
  if (side == 1) {   // (v = 8 with 256 residual centroids: 4 KiB, always in LDS)
    if constexpr (V == 8) return rlds ? ds_launch<DT, 8, 1, true>(a, lds, st) : hipErrorInvalidValue;
    else return hipErrorInvalidValue;
  }
  return rlds ? ds_launch<DT, V, 2, true>(a, lds, st) : ds_launch<DT, V, 2, false>(a, lds, st);
}

}  // namespace

bool dequant_sliced_eligible(const VptqLayerDesc& d) {
  return (d.vector_len == 8 || d.vector_len == 16) && d.weight_scale != nullptr && d.weight_bias != nullptr && (d.in_features & 7) == 0 &&
         d.group_size == d.in_features && d.num_codebooks == 1 && d.outlier_size == 0 &&
         (((uintptr_t)d.centroids | (uintptr_t)d.res_centroids | (uintptr_t)d.weight_scale | (uintptr_t)d.weight_bias) & 15) == 0 &&
         (long long)d.num_indices * ((d.in_features + 127) / 128) <= 0x7fffffffLL;
}

hipError_t launch_dequant_sliced(const VptqLayerDesc& d, const VptqSlicedLayout* L, int parts, int side_bytes, void* W, hipStream_t st) {
  DSArgs a = {};
  const int G = d.group_size, width = G / parts, v = d.vector_len;
  for (int p = 0; p < parts; ++p) {
    const int nsl = L[p].n_slices;
    int lg = 0;
    while ((1 << lg) < nsl) ++lg;
    a.part[p] = DSPart{(const uint4*)L[p].elems, (const int32_t*)L[p].blocks, (const int32_t*)L[p].first, (const int32_t*)L[p].wstart, L[p].res,
                       nsl, d.index_bits - lg, p * width, width, (width + VPTQ_SLICED_WINDOWS * 8 - 1) / (VPTQ_SLICED_WINDOWS * 8) * 8};
  }
  a.cent = (const uint32_t*)d.centroids;
  a.rcent = (const uint32_t*)d.res_centroids;
  a.perm = d.perm;
  a.scale = (const uint16_t*)d.weight_scale;
  a.wbias = (const uint16_t*)d.weight_bias;
  a.W = (uint16_t*)W;
  a.parts = parts, a.N = d.num_indices, a.I = d.in_features, a.O = d.out_features;
  const int max_tile = ds_max_tile(v);
  a.tiles = (a.I + max_tile - 1) / max_tile;
  a.tile = ((a.I + a.tiles - 1) / a.tiles + 127) / 128 * 128;   // (<= max_tile: that is a multiple of 128)
  a.tiles = (a.I + a.tile - 1) / a.tile;
  a.img_cols = a.tile;
  a.kmask = (uint32_t)d.num_centroids - 1u;
  a.krmask = d.num_res_centroids > 0 ? (uint32_t)d.num_res_centroids - 1u : 0u;
  const size_t res_bytes = (size_t)d.num_res_centroids * v * 2;
  const bool rlds = side_bytes != 0 && res_bytes <= (size_t)kDSResLdsMax;
  const size_t lds = (size_t)a.img_cols * v * 2 + (rlds ? res_bytes : 0);
  const bool f16 = d.dtype == VPTQ_DTYPE_F16;
  if (v == 8) return f16 ? ds_launch_v<F16, 8>(a, side_bytes, rlds, lds, st) : ds_launch_v<BF16, 8>(a, side_bytes, rlds, lds, st);
  return f16 ? ds_launch_v<F16, 16>(a, side_bytes, rlds, lds, st) : ds_launch_v<BF16, 16>(a, side_bytes, rlds, lds, st);
}

}  // namespace vptq
