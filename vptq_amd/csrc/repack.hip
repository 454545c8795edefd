// Rebuild a layer's packed int32 index stream [1][N][row_words] from its EXACT sliced layout(s)
// (vptq_sliced_layout_repack, include/vptq_hip.h): the inverse of what vptq_amd/utils/sliced.py builds.
//
// An element word carries `column | local << 16`; the (slice, row) list it sits in gives the rest of the index,
// index = slice << slice_bits | local; the residual index rides beside it in the `res` side stream (uint8 for v8's
// 256-entry table, uint16 for any other residual codebook); part p adds its first column.  The field of column g sits
// at bits [g T, g T + T) of the row (T = index_bits + res_bits, 14 ... 32): it straddles two words whenever T is not a
// power of two, and two column parts may share a word.
//
// One workgroup per row.  The row is assembled in LDS as its packed words (row_words x 4 bytes: at most 128 KiB for
// 32768 columns of 32 bits): the image is zeroed, every wave walks whole (slice, row) lists - 4 elements per lane and
// load, one 16-byte element load per lane - and ORs each field into the image (ds_or_b32: fields of different columns
// never overlap, so the order is free); then the image goes out with 16-byte stores (one 1 KiB stretch per wave and
// instruction; a row that does not start on a 16-byte boundary stores its first words singly).  Bits past G T stay zero.
#include "common.h"
#include "kernels.h"

namespace vptq {

namespace {

constexpr int kRPThreads = 1024;   // (16 waves: a 28672-column row image of 84 KiB leaves room for one workgroup per CU)
constexpr int kRPMaxLds = 163840;

struct RepackPart {
  const uint4* elems;
  const int32_t* blocks;   // [S][N]
  const int32_t* first;    // [S][N]
  const void* res;         // uint8 / uint16 per element, or NULL
  int n_slices, slice_bits, c0, width;
};

struct RepackArgs {
  RepackPart part[3];
  uint32_t* out;
  int parts, N, T, index_bits, row_words, side;   // side: 0 none, 1 uint8, 2 uint16
};

__device__ inline void rp_put(uint32_t* img, int col, int T, uint64_t val) {
  const uint32_t bit = (uint32_t)col * (uint32_t)T;
  const uint64_t v = val << (bit & 31u);
  atomicOr(&img[bit >> 5], (uint32_t)v);
  if ((bit & 31u) + (uint32_t)T > 32u) atomicOr(&img[(bit >> 5) + 1], (uint32_t)(v >> 32));
}

__global__ __launch_bounds__(kRPThreads) void sliced_repack_kernel(RepackArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t img[];
  const int n = blockIdx.x;
  const int words4 = (a.row_words + 3) >> 2;
  for (int i = threadIdx.x; i < words4; i += kRPThreads) reinterpret_cast<uint4*>(img)[i] = make_uint4(0, 0, 0, 0);
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, waves = kRPThreads / 64;
  const int lists = a.parts * a.part[0].n_slices;   // (every part has the same slice count)
  for (int L = wave; L < lists; L += waves) {
    const int p = L / a.part[0].n_slices, s = L - p * a.part[0].n_slices;
    const RepackPart& P = a.part[p];
    const int nb = P.blocks[(size_t)s * a.N + n];
    const size_t e0 = (size_t)P.first[(size_t)s * a.N + n] * 64;
    const uint32_t hi = (uint32_t)s << P.slice_bits;
    for (int c = lane; c < nb * 16; c += 64) {
      const size_t e = e0 + (size_t)c * 4;
      const uint4 w = P.elems[e >> 2];
      uint32_t r[4] = {0, 0, 0, 0};
      if (a.side == 1) {
        const uint32_t b = *reinterpret_cast<const uint32_t*>((const uint8_t*)P.res + e);
        r[0] = b & 0xffu; r[1] = (b >> 8) & 0xffu; r[2] = (b >> 16) & 0xffu; r[3] = b >> 24;
      } else if (a.side == 2) {
        const uint2 b = *reinterpret_cast<const uint2*>((const uint16_t*)P.res + e);
        r[0] = b.x & 0xffffu; r[1] = b.x >> 16; r[2] = b.y & 0xffffu; r[3] = b.y >> 16;
      }
      const uint32_t wd[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = (int)(wd[j] & 0xffffu);
        if (col >= P.width) continue;   // padding (column = part width)
        const uint64_t val = (uint64_t)(hi | (wd[j] >> 16)) | ((uint64_t)r[j] << a.index_bits);
        rp_put(img, P.c0 + col, a.T, val);
      }
    }
  }
  __syncthreads();
  uint32_t* row = a.out + (size_t)n * a.row_words;
  const int head = min((int)((4 - (((size_t)n * a.row_words) & 3)) & 3), a.row_words);   // words up to a 16-byte boundary
  if ((int)threadIdx.x < head) row[threadIdx.x] = img[threadIdx.x];
  const int body4 = (a.row_words - head) >> 2;
  uint4* dst = reinterpret_cast<uint4*>(row + head);
  for (int i = threadIdx.x; i < body4; i += kRPThreads) {
    const int j = head + 4 * i;
    dst[i] = make_uint4(img[j], img[j + 1], img[j + 2], img[j + 3]);
  }
  for (int j = head + 4 * body4 + (int)threadIdx.x; j < a.row_words; j += kRPThreads) row[j] = img[j];
}

}  // namespace

size_t sliced_repack_lds_bytes(const VptqLayerDesc& d) { return (size_t)((d.row_words + 3) / 4) * 16; }

hipError_t launch_sliced_repack(const VptqLayerDesc& d, const VptqSlicedLayout* L, int parts, int side_bytes, void* out, hipStream_t st) {
  if (const hipError_t e = allow_dynamic_lds<sliced_repack_kernel>(kRPMaxLds); e != hipSuccess) return e;
  RepackArgs a = {};
  const int G = d.group_size, width = G / parts;
  for (int p = 0; p < parts; ++p) {
    const int nsl = L[p].n_slices;
    int lg = 0;
    while ((1 << lg) < nsl) ++lg;
    a.part[p] = RepackPart{(const uint4*)L[p].elems, (const int32_t*)L[p].blocks, (const int32_t*)L[p].first, L[p].res, nsl,
                           d.index_bits - lg, p * width, width};
  }
  a.out = (uint32_t*)out;
  a.parts = parts;
  a.N = d.num_indices;
  a.T = d.index_bits + d.res_bits;
  a.index_bits = d.index_bits;
  a.row_words = d.row_words;
  a.side = side_bytes;
  hipLaunchKernelGGL(sliced_repack_kernel, dim3((unsigned)d.num_indices), dim3(kRPThreads), sliced_repack_lds_bytes(d), st, a);
  return hipGetLastError();
}

}  // namespace vptq
