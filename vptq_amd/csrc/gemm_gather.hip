// Batched decode for the large-codebook VPTQ formats (v = 8, k = 65536 main centroids; residual: none, 256 or 65536 -
// gemv_gather.hip's layers): up to 16 tokens in ONE launch, tokens = the M dimension of a matrix-core contraction.
//
// gemv_gather keeps TOK x 8 fp32 sums per lane and stops at 8 tokens; 9 - 16 tokens went through vptq_dequant + a dense GEMM.
// Here the contraction is D[token][output] += X[token][k] * W[output][k] in v_mfma_f32_16x16x32_f16 / _bf16, so the token count
// costs no registers: one pass over the packed indices, one gather per index, whatever the token count.
//
// Structure (gemm_k256.hip with the LDS codebook image replaced by L2 gathers; 256 threads):
//  * a workgroup owns row groups of kMRows = 2 vector-rows (16 outputs = one MFMA N block) over ALL input columns: no split-K, no
//    atomics, no workspace; row groups blockIdx.x, + gridDim.x, ...
//  * it walks column tiles of kMTile = 1024 columns.  A thread owns 8 consecutive columns of one vector-row: it reads their packed
//    index words with one wide load (gemv_gather's Fmt / elem), issues all 8 centroid gathers (T = 32: + 8 residual gathers; T = 24:
//    the 4 KiB residual table sits in LDS) and rebuilds the weights with the reference's roundings, w = r16(r16(r16(c + r) * s) + b) -
//    bit-identical to vptq_dequant (bf16: BF16::add4 / scale_bias4, see common.h).
//  * after an in-register 8 x 8 transposition (16 v_perm_b32) the thread holds, for each of its 8 outputs, the 8 consecutive-k values
//    one lane of the 16x16x32 MFMA supplies as B operand: 8 ds_write_b128 into the tile [column chunk][output][16 bytes], the
//    output slot XOR-ed with the chunk's low bits so that the 8 lanes of a write group cover all 32 banks; the B reads
//    (ds_read_b128, 16 outputs of a chunk contiguous) are conflict free.
//  * MFMA phase: the tile's 32 K-steps are dealt to the 4 waves; lane (token, k group kg) of wave w takes chunk 32 w + 8 kg + i in
//    step i, so that its 8 A operands (raw x, loaded from L2) are 64 CONSECUTIVE columns - one 128-byte line per token
//    (gemm_k256.hip: K-steps of adjacent columns cost 4x the L2 traffic).  Token rows past `tokens` are zero.
//  * the gathers of tile t + 1 are issued before the MFMA phase of tile t, its index words and scale / bias one tile earlier.
//  * at the end of a row group the 4 waves' partial D meet in LDS and are added in wave order: two launches give the same bits.
//    The sum is rounded once; the output bias is added in fp32.
// 36 KiB of LDS at most: four workgroups per CU.
#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace vptq {

constexpr int kMThreads = 256;
constexpr int kMRows = 2;                         // vector-rows per row group (16 outputs)
constexpr int kMTile = 1024;                      // columns per tile: kMThreads / kMRows chunks of 8
constexpr int kMChunks = kMTile / 8;
constexpr int kMWgPerCu = 4;

struct GemmGatherParams {
  const uint32_t* idx;    // [N][row_words]
  const char* cent;       // [65536][8]
  const char* rcent;      // [kr][8] or NULL
  const uint16_t* x;      // [tokens][G]
  void* y;                // [tokens][O]
  const uint16_t* scale;  // [G] column order
  const uint16_t* wbias;  // [G] column order
  const uint16_t* bias;   // [O] or NULL
  const uint16_t* perm;   // [G] or NULL
  int N, G, O, row_words, tokens, out_f32, n_groups;
};

typedef _Float16 mg_h8_t __attribute__((ext_vector_type(8)));
typedef __bf16 mg_b8_t __attribute__((ext_vector_type(8)));
template <typename DT>
static __device__ __forceinline__ f32x4 mg_mfma(u32x4 a, u32x4 b, f32x4 c) {
  if constexpr (std::is_same<DT, F16>::value)
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(mg_h8_t, a), __builtin_bit_cast(mg_h8_t, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(mg_b8_t, a), __builtin_bit_cast(mg_b8_t, b), c, 0, 0, 0);
}

// element e of 8 elements of T bits in T / 4 words (gemv_gather.hip: elem)
template <int T>
static __device__ __forceinline__ uint32_t mg_elem(const uint32_t (&w)[T / 4], int e) {
  if (T == 16) return (e & 1) ? (w[e >> 1] >> 16) : (w[e >> 1] & 0xffffu);
  if (T == 32) return w[e];
  const int b = (e >> 2) * 3;
  switch (e & 3) {
    case 0: return w[b] & 0xffffffu;
    case 1: return __builtin_amdgcn_alignbit(w[b + 1], w[b], 24) & 0xffffffu;
    case 2: return __builtin_amdgcn_alignbit(w[b + 2], w[b + 1], 16) & 0xffffffu;
    default: return w[b + 2] >> 8;
  }
}

template <typename DT, int T, bool PERM>
__global__ __launch_bounds__(kMThreads) void gemm_gather_kernel(const GemmGatherParams P) {
  constexpr int NW = T / 4;   // index words of 8 elements
  constexpr bool RES = T > 16;
  __shared__ __attribute__((aligned(16))) u32x4 tile[kMChunks * 16];   // [chunk][16 outputs]: 32 KiB
  __shared__ u32x4 rtab[T == 24 ? 256 : 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int G = P.G, N = P.N, O = P.O, tokens = P.tokens;
  const int n_tiles = (G + kMTile - 1) / kMTile;
  if constexpr (T == 24) {
    rtab[tid] = *(const u32x4*)(P.rcent + (size_t)tid * 16);   // kMThreads == 256 entries
    __syncthreads();
  }
  // dequant role: 8 consecutive columns (chunk dch) of vector-row dr of the group
  const int dr = tid >> 7, dch = tid & (kMChunks - 1);
  const uint32_t wslot = (uint32_t)(dch * 16 + dr * 8), wx = (uint32_t)(dch & 7);
  // MFMA role: lane (token / output mj, k group mkg); step i reads chunk 32 wave + 8 mkg + i
  const int mj = lane & 15, mkg = lane >> 4;
  const int mch0 = wave * 32 + mkg * 8;
  const uint16_t* const xrow = P.x + (size_t)(mj < tokens ? mj : tokens - 1) * G;

  for (int rg = blockIdx.x; rg < P.n_groups; rg += gridDim.x) {
    const int row = rg * kMRows + dr;
    const uint32_t* const irow = P.idx + (size_t)(row < N ? row : N - 1) * P.row_words;
    // (tiles past the end clamp to the last chunk of the row: every address stays inside the layer)
    auto dcol = [&](int t) { const int c = t * kMTile + dch * 8; return c < G ? c : G - 8; };
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
    auto load_sb = [&](int t, uint32_t (&s)[4], uint32_t (&b)[4]) {
      const uint32_t* s32 = (const uint32_t*)(P.scale + dcol(t));
      const uint32_t* b32 = (const uint32_t*)(P.wbias + dcol(t));
#pragma unroll
      for (int q = 0; q < 4; ++q) { s[q] = s32[q]; b[q] = b32[q]; }
    };
    u32x4 cv[8], rv[RES ? 8 : 1];
    auto gather = [&](const uint32_t (&w)[NW]) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const uint32_t v = mg_elem<T>(w, e);
        cv[e] = *(const u32x4*)(P.cent + (size_t)(v & 0xffffu) * 16);
        if constexpr (T == 24) rv[e] = rtab[(v >> 16) & 0xffu];
        if constexpr (T == 32) rv[e] = *(const u32x4*)(P.rcent + (size_t)(v >> 16) * 16);
      }
    };
    uint32_t wq[NW], sp[4], bp[4], sp_next[4], bp_next[4];
    load_idx(0, wq);
    load_sb(0, sp, bp);
    gather(wq);
    load_idx(1, wq);
    load_sb(1, sp_next, bp_next);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};

    for (int t = 0; t < n_tiles; ++t) {
      // ---- this tile's A operands: 8 x 16 bytes of x, 64 consecutive columns of one token
      u32x4 xa[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int col = t * kMTile + (mch0 + i) * 8;
        const int cc = col < G ? col : G - 8;
        if constexpr (PERM) {
          const uint32_t* p32 = (const uint32_t*)(P.perm + cc);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const uint32_t pv = p32[q];
            xa[i][q] = (uint32_t)xrow[pv & 0xffffu] | ((uint32_t)xrow[pv >> 16] << 16);
          }
        } else {
          xa[i] = *(const u32x4*)(xrow + cc);
        }
      }
      // ---- rebuild 8 columns x 8 outputs: c + r, * s, + b, each rounded to 16 bits
      const bool dvalid = t * kMTile + dch * 8 < G;
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
      __syncthreads();   // the previous tile's MFMA reads (and the previous row group's sums) are done
      // ---- transpose to 8 outputs x 8 k values and write them in B-operand order
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const u32x4 lo = {__builtin_amdgcn_perm(cv[1][p], cv[0][p], 0x05040100u), __builtin_amdgcn_perm(cv[3][p], cv[2][p], 0x05040100u),
                          __builtin_amdgcn_perm(cv[5][p], cv[4][p], 0x05040100u), __builtin_amdgcn_perm(cv[7][p], cv[6][p], 0x05040100u)};
        const u32x4 hi = {__builtin_amdgcn_perm(cv[1][p], cv[0][p], 0x07060302u), __builtin_amdgcn_perm(cv[3][p], cv[2][p], 0x07060302u),
                          __builtin_amdgcn_perm(cv[5][p], cv[4][p], 0x07060302u), __builtin_amdgcn_perm(cv[7][p], cv[6][p], 0x07060302u)};
        tile[wslot + ((uint32_t)(2 * p) ^ wx)] = lo;
        tile[wslot + ((uint32_t)(2 * p + 1) ^ wx)] = hi;
      }
      // ---- the next tile's gathers fly during the MFMA phase; the index words and scale / bias of the one after follow
      if (t + 1 < n_tiles) {
        gather(wq);
#pragma unroll
        for (int q = 0; q < 4; ++q) { sp[q] = sp_next[q]; bp[q] = bp_next[q]; }
        load_idx(t + 2, wq);
        load_sb(t + 2, sp_next, bp_next);
      }
      __syncthreads();   // tile complete
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const bool live = mj < tokens && t * kMTile + (mch0 + i) * 8 < G;
        const u32x4 a = {live ? xa[i][0] : 0u, live ? xa[i][1] : 0u, live ? xa[i][2] : 0u, live ? xa[i][3] : 0u};
        const u32x4 b = tile[(mch0 + i) * 16 + (mj ^ i)];   // ((mch0 + i) & 7 == i)
        acc = mg_mfma<DT>(a, b, acc);
      }
    }
    // ---- the 4 waves' partial D, added in wave order; D element (token = (l >> 4) * 4 + reg, output = l & 15)
    __syncthreads();
    float* const scr = (float*)tile;   // [wave][reg][lane]
#pragma unroll
    for (int r = 0; r < 4; ++r) scr[(wave * 4 + r) * 64 + lane] = acc[r];
    __syncthreads();
    {
      const int r = tid >> 6, l = tid & 63;
      float sum = scr[r * 64 + l];
#pragma unroll
      for (int w = 1; w < 4; ++w) sum += scr[(w * 4 + r) * 64 + l];
      const int token = (l >> 4) * 4 + r;
      const int o = rg * (kMRows * 8) + (l & 15);
      if (token < tokens && o < O) {
        if (P.bias) sum += DT::to_float(P.bias[o]);
        if (P.out_f32) ((float*)P.y)[(size_t)token * O + o] = sum;
        else ((uint16_t*)P.y)[(size_t)token * O + o] = DT::from_float(sum);
      }
    }
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
  D.tiles = (d.group_size + kMTile - 1) / kMTile;
  D.n_groups = (d.num_indices + kMRows - 1) / kMRows;
  const int slots = device_cus() * kMWgPerCu;
  D.grid = D.n_groups < slots ? D.n_groups : slots;
  D.rgs = D.grid > 0 ? (D.n_groups + D.grid - 1) / D.grid : 0;
  return D;
}

template <typename DT, int T>
static hipError_t launch_mg(const GemmGatherParams& P, const GemmGatherDecision& D, hipStream_t st) {
  const dim3 grid(D.grid), block(kMThreads);
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
  GemmGatherParams P = {};
  P.idx = (const uint32_t*)d.indices;
  P.cent = (const char*)d.centroids;
  P.rcent = (const char*)d.res_centroids;
  P.x = (const uint16_t*)x;
  P.y = y;
  P.scale = (const uint16_t*)(d.perm ? d.scale_permuted : d.weight_scale);
  P.wbias = (const uint16_t*)(d.perm ? d.bias_permuted : d.weight_bias);
  P.bias = (const uint16_t*)d.bias;
  P.perm = d.perm;
  P.N = d.num_indices; P.G = d.group_size; P.O = d.out_features; P.row_words = d.row_words;
  P.tokens = tokens; P.out_f32 = out_f32 ? 1 : 0;
  P.n_groups = D.n_groups;
  return D.f16 ? launch_mg_dt<F16>(P, D, st) : launch_mg_dt<BF16>(P, D, st);
}

}  // namespace vptq
