// Batched decode for the large-codebook VPTQ formats of VECTOR LENGTH 12 (16384 ... 65536 main centroids, any residual codebook, i.e.
// any total index width T = index_bits + res_bits <= 32 - "v12-k65536-4096" of the published checkpoints, "v12-k65536-256 / -0",
// "v12-k32768-1024"): 1 - 16 tokens in ONE launch, tokens = the M dimension of v_mfma_f32_16x16x32.
//
// gemv_gatherx keeps TOK x V fp32 sums per lane and stops at 4 token slots for v = 12: 5 - 8 tokens were two launches, each a full pass
// over the indices and the 24-byte gathers, and from 9 tokens the layer went through vptq_dequant + a dense GEMM.  The 16-output row
// group of gemm_gather_tile.h cannot hold a 12-output vector-row, so this unit has a tile geometry of its own:
//  * ROW GROUP = 4 vector-rows = 48 outputs = THREE MFMA N blocks of 16.  Vector-row r of the group supplies outputs 12 r ... 12 r + 11
//    of the 48: rows 1 and 2 straddle an N-block boundary (outputs 12 - 23 and 24 - 35 against blocks 0 - 15, 16 - 31, 32 - 47).  The A
//    operand (x) of a K-step is loaded once and feeds three MFMAs, into three f32x4 accumulators per lane: x is read once per 48
//    outputs where the 16-output kernels read it once per 16 (gemm_gatherw's open item "row groups of 32 outputs").
//  * DEQUANT ROLE: 256 threads = 4 vector-rows (the WAVE number: every row quantity is wave uniform) x 64 chunks of 8 columns, so a
//    tile is kG12Tile = 512 columns.  A thread reads its window of 8 T-bit elements - gemm_gatherx.hip's run-time index path for any
//    T <= 32 (window of up to 9 words, clamped tail words, v_alignbit_b32 normalisation, g12_elem<E>), a COPY: as a shared function
//    that body has twice cost 3 - 8 % and changed the parents' listings (profiles/r17, profiles/r31); A CHANGE TO IT THERE BELONGS HERE
//    TOO.  It issues 8 gathers of a 24-byte entry as a 16-byte and an 8-byte load - entries are only 8-byte aligned (gemv_gatherx.hip:
//    entry_align(12) == 8) - and the same for the residual entry: RES = 1 from the table copied once per workgroup into the dynamic
//    LDS behind the tile (tables of at most 32 KiB, gemm_gatherx_decide's rule), RES = 2 from L2 ("v12-k65536-4096": 96 KiB), RES = 0
//    none.  It rebuilds 8 columns x 12 outputs with the reference's roundings, w = r16(r16(r16(c + r) * s) + b): DT::add4 /
//    DT::scale_bias4 on the 16-byte part (gt_rebuild's), and on the 8-byte part the same arithmetic two pairs at a time - add4 over
//    the tails of two columns, DT::mul2_bcast / add2_bcast per column (bf16: the widened forms vptq_dequant itself uses).
//  * TILE [N block 0..2][chunk 0..63][16 outputs][16 bytes] = 48 KiB, written after the in-register transposition to "8 consecutive
//    k per output" (gt_write_tile's v_perm_b32 pairs, here for 12 outputs: 12 ds_write_b128 per thread).  Output o of vector-row r
//    is output g = 12 r + o of the group: N block g >> 4, slot g & 15 - both wave uniform, so a straddling row costs no lane work.
//    SWIZZLE AND BANKS: the slot is XOR-ed with the chunk's low 3 bits, slot' = (g & 15) ^ (chunk & 7).  One ds_write_b128 of a wave
//    goes out in groups of 8 lanes = 8 consecutive chunks of ONE output; chunks are 256 bytes apart (= 0 mod the 128 bytes of the 32
//    banks), so un-swizzled the 8 lanes would share 4 banks (8-way conflict); swizzled, lane j of the group lands in 16-byte column
//    (g ^ j) & 7 - the 8 lanes cover the 32 banks once, for every g, on either side of an N-block boundary (the N block only moves
//    the address by a multiple of 16 KiB).  The B reads (ds_read_b128) of the 16 lanes of a k group are the 16 slots of one chunk,
//    256 contiguous bytes in a permuted order: every group of 8 lanes covers the 32 banks once.
//  * MFMA PHASE: the tile's 16 K-steps are dealt to the 4 waves, 4 each x 3 N blocks.  Lane (token / output mj, k group mkg) of
//    wave w takes chunk 16 w + 4 mkg + i in step i, so its 4 A operands of a tile are 32 CONSECUTIVE columns of x - one 64-byte run
//    per token.  Token rows past `tokens` are zero, columns past G masked, addresses clamped inside the layer (gt_load_a1).
//  * PIPELINE: gemm_gatherx.hip's skeleton - the gathers of tile t + 1 are issued before the MFMA phase of tile t, its index words and
//    scale / bias one tile earlier; two barriers per tile.
//  * EPILOGUE: the 4 waves' three partial D meet in LDS (the tile's first 12 KiB) and are added in wave order: two launches give the
//    same bits.  The sum is rounded once, the output bias added in fp32.  Outputs o >= O (the reference pads O up to a multiple of
//    12) and vector-rows >= N (clamped to the last row when read) are masked.
// There is no form with a permutation: a permuted layer comes here as gemm_gather_px_plain(d) with x[perm] for x
// (vptq_quant_gemm_gather12 runs permute_x_tokens in front, as vptq_quant_gemm_gatherxw does).
// LDS: 48 KiB + the table.  Registers: g12_min_wg workgroups per CU; no instantiation has scratch (profiles/r37/listings.md).  No
// atomics, no scratch, plain vector stores.
// NOT HERE: 17 - 48 tokens (gemm_gather12w.hip), sibling groups, v = 6 (8 vector-rows per 48 outputs), the folded / selective arithmetics.
// gemm_gather12c.hip (column parts), gemm_gather12w.hip (token blocks), gemm_gather12_grouped.hip (sibling groups) and gemm_gather12w_grouped.hip (sibling groups, token blocks) hold COPIES of the row-group body: A CHANGE HERE BELONGS THERE TOO.
#include "gemm_gather_tile.h"
#include "launch.h"

namespace vptq {

constexpr int kG12V = 12;
constexpr int kG12EB = kG12V * 2;                    // bytes per codebook entry
constexpr int kG12Rows = 4;                          // vector-rows per row group
constexpr int kG12Out = kG12Rows * kG12V;            // 48 outputs = 3 N blocks
constexpr int kG12Tile = 512;                        // columns per tile: kGTThreads / 4 chunks of 8
constexpr int kG12Chunks = kG12Tile / 8;
constexpr int kG12TileBytes = 3 * kG12Chunks * 16 * 16;   // [N block][chunk][16 outputs][16 bytes]: 48 KiB
constexpr int kG12ResLdsMax = 32768;                 // (gemm_gatherx.hip: kGXResLdsMax)
constexpr int kG12LdsPerCu = 160 * 1024;

typedef uint32_t u32x4_a8 __attribute__((ext_vector_type(4), aligned(8)));
typedef uint32_t u32x2_a8 __attribute__((ext_vector_type(2), aligned(8)));

// workgroups per CU the register budget is held to: 2 (256 VGPRs) for every instantiation.  RES = 0 has the LDS for 3 (48 KiB) but
// spilled there (168 VGPRs: 68 / 140 bytes of scratch in fp16 / bf16) and is relaxed to 2 as well (profiles/r37/listings.md)
constexpr int g12_min_wg(int) { return 2; }

// element E (compile time) of T bits (wave uniform) out of the normalised window n[0..7] (gemm_gatherx.hip: gx_elem, a copy)
template <int E>
static __device__ __forceinline__ uint32_t g12_elem(const uint32_t (&n)[8], int T, uint32_t mask) {
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

// first column of chunk dch of tile t (tiles past the end clamp to the last chunk of the row)
static __device__ __forceinline__ int g12_dcol(int t, int dch, int G) { const int c = t * kG12Tile + dch * 8; return c < G ? c : G - 8; }

template <typename DT, int RES>
__global__ __launch_bounds__(kGTThreads, g12_min_wg(RES)) void gemm_gather12_kernel(const GemmGatherParams P) {
  static_assert(RES >= 0 && RES <= 2, "residual: none, LDS, L2");
  extern __shared__ __attribute__((aligned(16))) unsigned char g12_smem[];
  u32x4* const tile = (u32x4*)g12_smem;                              // [N block][chunk][16 outputs]: 48 KiB
  const unsigned char* const rtab = g12_smem + kG12TileBytes;        // RES = 1: the residual table
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int G = P.G, N = P.N, O = P.O, tokens = P.tokens;
  const int T = P.ib + P.rb, ib = P.ib;
  const uint32_t tmask = T >= 32 ? 0xffffffffu : ((1u << T) - 1u), mmask = (1u << ib) - 1u;
  // the 9th window word: 8 T bits + the largest offset (24, 16 or 0 bits: T odd, T % 4 == 2, T % 4 == 0) beyond 8 words (T = 31)
  const bool need9 = 8 * T + ((T & 1) ? 24 : (T & 2) ? 16 : 0) > 256;
  const int last = P.row_words - 1;
  const int n_tiles = (G + kG12Tile - 1) / kG12Tile;
  if constexpr (RES == 1) {
    const int n8 = P.res_bytes >> 3;   // (24-byte entries: the table is whole 8-byte units)
    for (int i = tid; i < n8; i += kGTThreads)
      *(u32x2*)(g12_smem + kG12TileBytes + (size_t)i * 8) = *(const u32x2_a8*)(P.rcent + (size_t)i * 8);
    __syncthreads();
  }
  // dequant role: 8 consecutive columns (chunk dch) of the 12 outputs of vector-row dr = wave of the group
  const int dr = wave, dch = lane;
  const uint32_t wx = (uint32_t)(dch & 7);
  // MFMA role: lane (token / output mj, k group mkg); step i reads chunk 16 wave + 4 mkg + i
  const int mj = lane & 15, mkg = lane >> 4;
  const int mch0 = wave * 16 + mkg * 4;
  const uint32_t xoff = (uint32_t)(mj < tokens ? mj : tokens - 1) * (uint32_t)G * 2u;

  for (int rg = blockIdx.x; rg < P.n_groups; rg += gridDim.x) {
    const int row = rg * kG12Rows + dr;
    const uint32_t* const irow = P.idx + (size_t)(row < N ? row : N - 1) * P.row_words;
    auto dcol = [&](int t) { return g12_dcol(t, dch, G); };
    // ---- the index window: gemm_gatherx.hip's (see the head of the file)
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
    // ---- the gathers: a 24-byte entry as 16 + 8 bytes (ca / cb: outputs 0 - 7 / 8 - 11 of the 8 columns)
    u32x4 ca[8], ra[RES ? 8 : 1];
    u32x2 cb[8], rb[RES ? 8 : 1];
    auto gather1 = [&](int e, uint32_t v) {
      const char* const c = P.cent + (size_t)(v & mmask) * kG12EB;
      ca[e] = *(const u32x4_a8*)c;
      cb[e] = *(const u32x2_a8*)(c + 16);
      if constexpr (RES == 1) {
        const unsigned char* const r = rtab + (v >> ib) * (uint32_t)kG12EB;
        ra[e] = *(const u32x4_a8*)r;
        rb[e] = *(const u32x2_a8*)(r + 16);
      }
      if constexpr (RES == 2) {
        const char* const r = P.rcent + (size_t)(v >> ib) * kG12EB;
        ra[e] = *(const u32x4_a8*)r;
        rb[e] = *(const u32x2_a8*)(r + 16);
      }
    };
    auto gather = [&](const uint32_t (&n)[8]) {
      gather1(0, g12_elem<0>(n, T, tmask)); gather1(1, g12_elem<1>(n, T, tmask));
      gather1(2, g12_elem<2>(n, T, tmask)); gather1(3, g12_elem<3>(n, T, tmask));
      gather1(4, g12_elem<4>(n, T, tmask)); gather1(5, g12_elem<5>(n, T, tmask));
      gather1(6, g12_elem<6>(n, T, tmask)); gather1(7, g12_elem<7>(n, T, tmask));
    };
    // ---- the rebuild in place: c + r, * s, + b, each rounded to 16 bits; columns past the row end become 0
    auto rebuild = [&](const uint32_t (&sp)[4], const uint32_t (&bp)[4], bool dvalid) {
      gt_rebuild<DT, RES != 0>(ca, ra, sp, bp, dvalid);
#pragma unroll
      for (int e = 0; e < 8; e += 2) {
        uint32_t v[4] = {cb[e][0], cb[e][1], cb[e + 1][0], cb[e + 1][1]};
        if constexpr (RES != 0) {
          const uint32_t r[4] = {rb[e][0], rb[e][1], rb[e + 1][0], rb[e + 1][1]};
          DT::add4(v, r);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int h = q >> 1;   // column e + h: half h of the pair registers sp / bp[e >> 1]
          v[q] = DT::add2_bcast(DT::mul2_bcast(v[q], sp[e >> 1], h), bp[e >> 1], h);
          v[q] = dvalid ? v[q] : 0u;
        }
        cb[e] = u32x2{v[0], v[1]};
        cb[e + 1] = u32x2{v[2], v[3]};
      }
    };
    // ---- transpose to 12 outputs x 8 k values and write them in B-operand order (head of the file: swizzle and banks)
    auto write_tile = [&]() {
#pragma unroll
      for (int p = 0; p < 6; ++p) {
        uint32_t c[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) c[e] = p < 4 ? ca[e][p & 3] : cb[e][p & 1];
        const u32x4 lo = {__builtin_amdgcn_perm(c[1], c[0], 0x05040100u), __builtin_amdgcn_perm(c[3], c[2], 0x05040100u),
                          __builtin_amdgcn_perm(c[5], c[4], 0x05040100u), __builtin_amdgcn_perm(c[7], c[6], 0x05040100u)};
        const u32x4 hi = {__builtin_amdgcn_perm(c[1], c[0], 0x07060302u), __builtin_amdgcn_perm(c[3], c[2], 0x07060302u),
                          __builtin_amdgcn_perm(c[5], c[4], 0x07060302u), __builtin_amdgcn_perm(c[7], c[6], 0x07060302u)};
        const uint32_t g0 = (uint32_t)(dr * kG12V + 2 * p), g1 = g0 + 1u;   // outputs 2 p, 2 p + 1 of the row, as outputs of the group
        tile[((g0 >> 4) * kG12Chunks + (uint32_t)dch) * 16u + ((g0 & 15u) ^ wx)] = lo;
        tile[((g1 >> 4) * kG12Chunks + (uint32_t)dch) * 16u + ((g1 & 15u) ^ wx)] = hi;
      }
    };
    uint32_t wq[8], sp[4], bp[4], sp_next[4], bp_next[4];
    load_idx(0, wq);
    gt_load_sb(P, dcol(0), sp, bp);
    gather(wq);
    load_idx(1, wq);
    gt_load_sb(P, dcol(1), sp_next, bp_next);
    f32x4 acc[3];
#pragma unroll
    for (int b = 0; b < 3; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int t = 0; t < n_tiles; ++t) {
      // ---- this tile's A operands: 4 x 16 bytes of x, 32 consecutive columns of one token
      u32x4 xa[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) xa[i] = gt_load_a1<false>(nullptr, P.x, xoff, G, t * kG12Tile + (mch0 + i) * 8);
      rebuild(sp, bp, t * kG12Tile + dch * 8 < G);
      __syncthreads();   // the previous tile's MFMA reads (and the previous row group's sums) are done
      write_tile();
      // ---- the next tile's gathers fly during the MFMA phase; the index window and scale / bias of the one after follow
      if (t + 1 < n_tiles) {
        gather(wq);
#pragma unroll
        for (int q = 0; q < 4; ++q) { sp[q] = sp_next[q]; bp[q] = bp_next[q]; }
        load_idx(t + 2, wq);
        gt_load_sb(P, dcol(t + 2), sp_next, bp_next);
      }
      __syncthreads();   // tile complete
      // ---- this wave's 4 K-steps: the A operand once, three B reads and three MFMAs
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool live = mj < tokens && t * kG12Tile + (mch0 + i) * 8 < G;
        const u32x4 a = {live ? xa[i][0] : 0u, live ? xa[i][1] : 0u, live ? xa[i][2] : 0u, live ? xa[i][3] : 0u};
        const uint32_t slot = (uint32_t)((mch0 + i) * 16) + ((uint32_t)mj ^ (uint32_t)((mch0 + i) & 7));
#pragma unroll
        for (int b = 0; b < 3; ++b) acc[b] = mfma16x16x32<DT>(a, tile[(uint32_t)(b * kG12Chunks * 16) + slot], acc[b]);
      }
    }
    // ---- the 4 waves' partial D of the three N blocks, added in wave order; D element (token = (l >> 4) * 4 + reg, output = l & 15)
    {
      float* const scr = (float*)g12_smem;   // [wave][N block][reg][lane]: the tile's first 12 KiB
      __syncthreads();
#pragma unroll
      for (int b = 0; b < 3; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) scr[((wave * 3 + b) * 4 + r) * 64 + lane] = acc[b][r];
      __syncthreads();
      const int r = wave, token = (lane >> 4) * 4 + r;
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        float sum = scr[(b * 4 + r) * 64 + lane];
#pragma unroll
        for (int w = 1; w < 4; ++w) sum += scr[((w * 3 + b) * 4 + r) * 64 + lane];
        const int o = rg * kG12Out + b * 16 + (lane & 15);
        if (token < tokens && o < O) {
          if (P.bias) sum += DT::to_float(P.bias[o]);
          if (P.out_f32) ((float*)P.y)[(size_t)token * O + o] = sum;
          else ((uint16_t*)P.y)[(size_t)token * O + o] = DT::from_float(sum);
        }
      }
    }
  }
}

// ---- host side -------------------------------------------------------------------
bool gemm_gather12_eligible(const VptqLayerDesc& d, int tokens) {
  const int T = d.index_bits + d.res_bits;
  return d.vector_len == kG12V && d.num_codebooks == 1 && d.outlier_size == 0 && d.weight_scale != nullptr && d.weight_bias != nullptr &&
         d.group_size >= 8 && (d.group_size % 8) == 0 && d.group_size == d.in_features &&
         d.num_centroids >= 16384 && d.num_centroids <= 65536 && d.num_res_centroids >= 0 && d.num_res_centroids <= 65536 &&
         (d.num_res_centroids > 0) == (d.res_centroids != nullptr) && d.index_bits >= 14 && d.index_bits <= 16 && d.res_bits >= 0 &&
         T <= 32 && (long long)d.row_words * 32 >= (long long)d.group_size * T &&
         (long long)d.num_indices * kG12V >= d.out_features && d.num_indices >= 1 && tokens >= 1 && tokens <= 16 &&
         (d.perm == nullptr || (d.scale_permuted != nullptr && d.bias_permuted != nullptr)) &&
         (((uintptr_t)d.indices) & 15) == 0 && (((uintptr_t)d.centroids | (uintptr_t)d.res_centroids) & 7) == 0 &&
         (((uintptr_t)d.weight_scale | (uintptr_t)d.weight_bias | (uintptr_t)d.scale_permuted |
           (uintptr_t)d.bias_permuted | (uintptr_t)d.perm) & 3) == 0;
}

// what one launch IS: the template arguments of gemm_gather12_kernel<DT, RES>, the run-time index widths and the launch shape,
// decided once for the launcher and for vptq_quant_gemm_gather12_instance
GemmGather12Decision gemm_gather12_decide(const VptqLayerDesc& d, int tokens) {
  GemmGather12Decision D = {};
  D.f16 = d.dtype == VPTQ_DTYPE_F16;
  D.ib = d.index_bits;
  D.rb = d.res_bits;
  D.res_bytes = d.num_res_centroids * kG12EB;
  D.res = D.res_bytes == 0 ? 0 : D.res_bytes <= kG12ResLdsMax ? 1 : 2;
  D.tok = tokens;
  D.tiles = (d.group_size + kG12Tile - 1) / kG12Tile;
  D.lds = kG12TileBytes + (D.res == 1 ? D.res_bytes : 0);
  const int by_lds = kG12LdsPerCu / D.lds, by_regs = g12_min_wg(D.res);
  D.wgcu = by_lds < by_regs ? by_lds : by_regs;   // the RESIDENT workgroups per CU
  const GemmGatherGrid g = gemm_gather_grid(d.num_indices, kG12Rows, D.wgcu);
  D.n_groups = g.n_groups; D.grid = g.grid; D.rgs = g.rgs;
  return D;
}

template <typename DT>
static hipError_t launch_g12(const GemmGatherParams& P, const GemmGather12Decision& D, hipStream_t st) {
  const dim3 grid(D.grid), block(kGTThreads);
  hipError_t e = hipSuccess;
  switch (D.res) {
    case 0: hipLaunchKernelGGL((gemm_gather12_kernel<DT, 0>), grid, block, D.lds, st, P); break;
    case 1:   // 48 KiB + the table: past the 64 KiB a kernel may use unasked
      e = allow_dynamic_lds<gemm_gather12_kernel<DT, 1>>(kG12TileBytes + kG12ResLdsMax);
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL((gemm_gather12_kernel<DT, 1>), grid, block, D.lds, st, P);
      break;
    case 2: hipLaunchKernelGGL((gemm_gather12_kernel<DT, 2>), grid, block, D.lds, st, P); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// d: a layer WITHOUT a permutation (a permuted one as gemm_gather_px_plain(d), x = x[perm])
hipError_t launch_gemm_gather12(const VptqLayerDesc& d, const void* x, void* y, int tokens, bool out_f32, hipStream_t st) {
  const GemmGather12Decision D = gemm_gather12_decide(d, tokens);
  if (d.perm || D.grid < 1 || tokens < 1 || tokens > 16 || D.lds > kG12TileBytes + kG12ResLdsMax) return hipErrorInvalidValue;
  GemmGatherParams P = gemm_gather_params(d, x, y, tokens, out_f32, D.n_groups);
  P.ib = D.ib; P.rb = D.rb; P.res_bytes = D.res_bytes;   // (the table copied into LDS is the one D.lds has room for)
  return D.f16 ? launch_g12<F16>(P, D, st) : launch_g12<BF16>(P, D, st);
}

}  // namespace vptq
