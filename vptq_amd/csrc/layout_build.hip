// Build a sliced layout from a layer's packed int32 index stream [1][N][row_words] on the device
// (vptq_sliced_layout_plan / vptq_sliced_layout_fill, include/vptq_hip.h): the forward direction of repack.hip, and byte for
// byte what the torch recipe vptq_amd/utils/sliced.py:layout_from_indices builds (that recipe stays the model of this file).
//
// The recipe is a deterministic function of ONE row, and its two sorts can be replaced by counting:
//   slice s (top bits of the bucket index, or - whole table - the column range), window w = min(col / window_cols, 3),
//   class cls = local & 15; rank = how many earlier columns of the row share (s, w, cls); per (s, w): full = the smallest of
//   the 16 class counts, rest = the segment's length - 16 full.
//   rank < full : position 16 rank + cls of the (s, w) segment - integers only.
//   the others  : behind those, ordered by the recipe's float64 key
//                     ((s 4 + w) 2 G + (16 full + ((rank - full) + 0.5) rest / (count - full))) + cls / 64
//                 evaluated in fp64 in exactly that order, contraction off (the (s, w) offset is added BEFORE cls / 64: it
//                 changes the rounding); an element's place is the number of surplus elements of its segment with a smaller
//                 key.  EQUAL KEYS do occur (about one pair in a few thousand segments); the recipe's argsort is not asked to
//                 be stable, so it leaves their order open - here a tie is broken the way a stable sort of the recipe's
//                 first order would: by class, then by column.
//   wstart, blocks, first are counts and prefix sums; padding is (column = G, local 0), side 0, to the end of the last block.
//
// Plan: one workgroup per row counts the (s, w) segments (LDS atomics: counts do not depend on order) and writes wstart and
// blocks; one workgroup then scans blocks [S][N] into first and the total.  Fill: one workgroup per (row, window) - a window is
// at most 8192 columns, so class ids, ranks, the surplus keys and the staged output fit the LDS (14 bytes per column).  Ranks
// come from a ballot match inside each wave over consecutive columns and a per-wave histogram, so they are those of column
// order whatever the scheduling.  The window's elements are staged in LDS in list order and leave as S contiguous runs.
// Nothing here is tuned: load-time code, one read of the stream per step and one write of the layout.
#include "common.h"
#include "kernels.h"

namespace vptq {

namespace {

constexpr int kLBThreads = 512, kLBWaves = kLBThreads / 64;
constexpr int kLBMaxSlices = 32, kLBMaxKeys = kLBMaxSlices * 16;
constexpr int kLBWindows = VPTQ_SLICED_WINDOWS;

__device__ inline uint32_t lb_field(const uint32_t* row, int g, int T) {
  const uint32_t bit = (uint32_t)g * (uint32_t)T, o = bit & 31u;
  uint64_t v = row[bit >> 5];
  if (o + (uint32_t)T > 32u) v |= (uint64_t)row[(bit >> 5) + 1] << 32;   // (a straddling field: the next word is inside the row)
  return (uint32_t)(v >> o) & (T == 32 ? 0xffffffffu : ((1u << T) - 1u));
}

// (slice << 4 | class) and the index inside the slice of part-column `col` with packed field f
__device__ inline uint32_t lb_classify(const LayoutBuildParams& a, int col, uint32_t f, uint32_t* local) {
  const uint32_t b = (f >> a.bucket_shift) & a.bucket_mask;
  const uint32_t s = a.whole ? (uint32_t)(((long long)col * a.S) / a.W) : b >> a.slice_bits;
  *local = a.whole ? b : b & ((1u << a.slice_bits) - 1u);
  return s << 4 | (*local & 15u);
}

__global__ __launch_bounds__(256) void layout_plan_kernel(LayoutBuildParams a) {
  __shared__ int cnt[kLBMaxSlices * kLBWindows];
  const int n = blockIdx.x;
  for (int i = threadIdx.x; i < a.S * kLBWindows; i += 256) cnt[i] = 0;
  __syncthreads();
  const uint32_t* row = a.packed + (size_t)n * a.row_words;
  for (int col = threadIdx.x; col < a.W; col += 256) {
    uint32_t local;
    const uint32_t key = lb_classify(a, col, lb_field(row, a.c0 + col, a.T), &local);
    const int w = min(col / a.wcols, kLBWindows - 1);
    atomicAdd(&cnt[(key >> 4) * kLBWindows + w], 1);
  }
  __syncthreads();
  if ((int)threadIdx.x < a.S) {
    const int s = threadIdx.x;
    int32_t* ws = a.wstart + ((size_t)s * a.N + n) * (kLBWindows + 1);
    int len = 0;
    for (int w = 0; w < kLBWindows; ++w) { ws[w] = len; len += cnt[s * kLBWindows + w]; }
    ws[kLBWindows] = len;
    a.blocks[(size_t)s * a.N + n] = (len + 63) >> 6;
  }
}

// first[i] = blocks[0] + ... + blocks[i - 1] over the flattened [S][N]; *total = the sum.  One workgroup.
__global__ __launch_bounds__(1024) void layout_scan_kernel(const int32_t* blocks, int32_t* first, long long* total, int M) {
  __shared__ long long part[1024];
  const int t = threadIdx.x, per = (M + 1023) / 1024;
  const int lo = min(t * per, M), hi = min(lo + per, M);
  long long sum = 0;
  for (int i = lo; i < hi; ++i) sum += blocks[i];
  part[t] = sum;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const long long add = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  long long base = part[t] - sum;
  for (int i = lo; i < hi; ++i) { first[i] = (int32_t)base; base += blocks[i]; }
  if (t == 1023) *total = part[1023];
}

__global__ __launch_bounds__(kLBThreads) void layout_fill_kernel(LayoutBuildParams a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ int cnt[kLBMaxKeys];
  __shared__ int full[kLBMaxSlices], rest[kLBMaxSlices], segoff[kLBMaxSlices + 1], soff[kLBMaxSlices + 1], scur[kLBMaxSlices];
  __shared__ long long dbase[kLBMaxSlices];
  const int n = blockIdx.x, w = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.S * 16;
  // dynamic LDS: surplus keys (later: the staged words and side values), then 16-bit arrays
  double* skey = reinterpret_cast<double*>(lds);
  uint32_t* st_word = reinterpret_cast<uint32_t*>(lds);
  uint16_t* st_side = reinterpret_cast<uint16_t*>(lds + (size_t)a.cap * 4);
  uint16_t* sidx = reinterpret_cast<uint16_t*>(lds + (size_t)a.cap * 8);
  uint16_t* scl = sidx + a.cap;
  uint16_t* rnk = scl + a.cap;
  uint16_t* hist = rnk + a.cap;   // [waves][K]
  const int wlo = min(w * a.wcols, a.W), whi = w == kLBWindows - 1 ? a.W : min((w + 1) * a.wcols, a.W);
  const int nw = whi - wlo;
  const uint32_t* row = a.packed + (size_t)n * a.row_words;
  const size_t limit = (size_t)a.total_blocks * 64;

  for (int i = tid; i < kLBWaves * K; i += kLBThreads) hist[i] = 0;
  if (tid < a.S) scur[tid] = 0;
  __syncthreads();
  // every wave takes a contiguous range of the window's columns, 64 at a time in column order: rank inside the range
  const int per = ((nw + kLBWaves - 1) / kLBWaves + 63) & ~63;
  const int r0 = min(wave * per, nw), r1 = min(r0 + per, nw);
  for (int base = r0; base < r1; base += 64) {
    const int i = base + lane;
    const bool valid = i < r1;
    uint32_t key = 0, local;
    if (valid) key = lb_classify(a, wlo + i, lb_field(row, a.c0 + wlo + i, a.T), &local);
    unsigned long long same = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 9; ++b) {
      const bool bit = (key >> b) & 1u;
      const unsigned long long m = __ballot(valid && bit);
      same &= bit ? m : ~m;
    }
    const int before = __popcll(same & ((1ull << lane) - 1ull));
    const int leader = valid ? __ffsll((long long)same) - 1 : lane;
    int start = 0;
    if (valid && before == 0) {   // (the first lane of every key present: distinct words, this wave's histogram)
      start = hist[wave * K + key];
      hist[wave * K + key] = (uint16_t)(start + __popcll(same));
    }
    start = __shfl(start, leader);
    if (valid) {
      scl[i] = (uint16_t)key;
      rnk[i] = (uint16_t)(start + before);
    }
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  // per key: the waves' counts -> their offsets (exclusive, in wave = column order) and the total
  for (int k = tid; k < K; k += kLBThreads) {
    int acc = 0;
    for (int v = 0; v < kLBWaves; ++v) {
      const int t = hist[v * K + k];
      hist[v * K + k] = (uint16_t)acc;
      acc += t;
    }
    cnt[k] = acc;
  }
  __syncthreads();
  if (tid < a.S) {
    int mn = cnt[tid * 16], len = 0;
    for (int c = 0; c < 16; ++c) { mn = min(mn, cnt[tid * 16 + c]); len += cnt[tid * 16 + c]; }
    full[tid] = mn;
    rest[tid] = len - 16 * mn;
    const size_t sn = (size_t)tid * a.N + n;
    dbase[tid] = (long long)a.first[sn] * 64 + a.wstart[sn * (kLBWindows + 1) + w];
  }
  __syncthreads();
  if (tid == 0) {
    int e = 0, u = 0;
    for (int s = 0; s < a.S; ++s) {
      segoff[s] = e;
      soff[s] = u;
      e += rest[s] + 16 * full[s];
      u += rest[s];
    }
    segoff[a.S] = e;
    soff[a.S] = u;
  }
  __syncthreads();
  // pass 1: positions of the complete rows of 16 classes; the surplus elements' keys into their segment's list
  for (int i = tid; i < nw; i += kLBThreads) {
    const int key = scl[i], s = key >> 4, cls = key & 15;
    const int rank = rnk[i] + hist[(i / per) * K + key];
    const int f = full[s];
    if (rank < f) {
      rnk[i] = (uint16_t)(16 * rank + cls);
    } else {
      const int c = cnt[key] - f;
      const double spread = (double)(16 * f) + (((double)(rank - f) + 0.5) * (double)rest[s]) / (double)(c < 1 ? 1 : c);
      const double dk = ((double)((long long)(s * kLBWindows + w) * (2ll * a.W)) + spread) + (double)cls / 64.0;
      const int slot = soff[s] + atomicAdd(&scur[s], 1);
      skey[slot] = dk;
      sidx[slot] = (uint16_t)i;
      rnk[i] = (uint16_t)(0x8000 | slot);
    }
  }
  __syncthreads();
  // pass 2: a surplus element's place = the surplus elements of its segment in front of it
  for (int i = tid; i < nw; i += kLBThreads) {
    const int r = rnk[i];
    if (!(r & 0x8000)) continue;
    const int key = scl[i], s = key >> 4;
    const double mine = skey[r & 0x7fff];
    const int my_id = (key & 15) << 16 | i;
    int ahead = 0;
    for (int j = soff[s]; j < soff[s + 1]; ++j) {
      const double kj = skey[j];
      if (kj < mine) {
        ++ahead;
      } else if (kj == mine) {   // a tie: class, then column (a stable sort of the recipe's first order)
        const int oj = sidx[j];
        ahead += (((int)(scl[oj] & 15) << 16 | oj) < my_id) ? 1 : 0;
      }
    }
    rnk[i] = (uint16_t)(16 * full[s] + ahead);   // (a position is below 8192: bit 15, the mark of a slot, is clear again)
  }
  __syncthreads();
  // stage the window's elements in list order (over the keys, no longer needed), then S contiguous runs go out
  for (int i = tid; i < nw; i += kLBThreads) {
    const int key = scl[i], s = key >> 4;
    const uint32_t f = lb_field(row, a.c0 + wlo + i, a.T);
    uint32_t local;
    lb_classify(a, wlo + i, f, &local);
    const int q = segoff[s] + rnk[i];
    st_word[q] = (uint32_t)(wlo + i) | local << 16;
    if (a.side) st_side[q] = (uint16_t)(f >> a.side_shift);
  }
  __syncthreads();
  for (int q = tid; q < nw; q += kLBThreads) {
    int s = 0;
    while (segoff[s + 1] <= q) ++s;
    const size_t dest = (size_t)dbase[s] + (size_t)(q - segoff[s]);
    if (dest >= limit) continue;
    a.elems[dest] = st_word[q];
    if (a.side == 1) reinterpret_cast<uint8_t*>(a.res)[dest] = (uint8_t)st_side[q];
    else if (a.side == 2) reinterpret_cast<uint16_t*>(a.res)[dest] = st_side[q];
  }
  // the last window's workgroup pads every list of the row to the end of its last block: (column = G, local 0), side 0
  if (w == kLBWindows - 1) {
    for (int s = 0; s < a.S; ++s) {
      const size_t sn = (size_t)s * a.N + n;
      const int len = a.wstart[sn * (kLBWindows + 1) + kLBWindows], end = a.blocks[sn] * 64;
      const size_t e0 = (size_t)a.first[sn] * 64;
      for (int p = len + tid; p < end; p += kLBThreads) {
        if (e0 + p >= limit) continue;
        a.elems[e0 + p] = (uint32_t)a.W;
        if (a.side == 1) reinterpret_cast<uint8_t*>(a.res)[e0 + p] = 0;
        else if (a.side == 2) reinterpret_cast<uint16_t*>(a.res)[e0 + p] = 0;
      }
    }
  }
}

// a layer without a single element (the recipe's max(total, 1)): one block of padding
__global__ __launch_bounds__(64) void layout_pad_block_kernel(LayoutBuildParams a) {
  a.elems[threadIdx.x] = (uint32_t)a.W;
  if (a.side == 1) reinterpret_cast<uint8_t*>(a.res)[threadIdx.x] = 0;
  else if (a.side == 2) reinterpret_cast<uint16_t*>(a.res)[threadIdx.x] = 0;
}

}  // namespace

size_t layout_fill_lds_bytes(const LayoutBuildParams& a) { return (size_t)a.cap * 14 + (size_t)kLBWaves * a.S * 16 * 2 + 16; }

hipError_t launch_layout_plan(const LayoutBuildParams& a, hipStream_t st) {
  hipLaunchKernelGGL(layout_plan_kernel, dim3((unsigned)a.N), dim3(256), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(layout_scan_kernel, dim3(1), dim3(1024), 0, st, (const int32_t*)a.blocks, a.first, a.total, a.S * a.N);
  return hipGetLastError();
}

hipError_t launch_layout_fill(const LayoutBuildParams& a, hipStream_t st) {
  if (const hipError_t e = allow_dynamic_lds<layout_fill_kernel>(131072); e != hipSuccess) return e;
  if (a.total_blocks <= 0) {
    hipLaunchKernelGGL(layout_pad_block_kernel, dim3(1), dim3(64), 0, st, a);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(layout_fill_kernel, dim3((unsigned)a.N, kLBWindows), dim3(kLBThreads), layout_fill_lds_bytes(a), st, a);
  return hipGetLastError();
}

}  // namespace vptq
