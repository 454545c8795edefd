// Batched decode for the canonical "2-bit" VPTQ format (v = 8, 256 + 256 centroids, norm on):
// up to 16 tokens in ONE launch, tokens = the M dimension of a real matrix-core contraction.
//
// Reference: vptq/ops/quant_gemm.py:213-274 - its fused GEMV takes < 3 tokens, everything else
// is dequant to a dense W + F.linear; its v2 kernel takes < 16 (csrc/quant_gemv_v2.cu:58).
// Round 1 served 5-16 tokens as launches of <= 4 tokens of gemv_k256m_kernel (48 us per
// 8192^2 layer at 16 tokens); the 4x4x4 MFMA of that kernel multiplies 4 tokens at most.
//
// Structure (one 1024-thread workgroup per CU, persistent over groups of 4 vector-rows):
//  * the 64 KiB conflict-free codebook image of gemv_k256m.hip (8 replicas per table, the
//    two gathers of an index split across the lanes).
//  * per step a TILE of 4 vector-rows x 1024 columns (4096 indices, 4 per thread) is
//    dequantised with the reference CPU path's roundings, w = r16(r16(r16(c + r) * s) + b)
//    in packed f16 - bit-identical to vptq_dequant - and written to LDS IN MFMA-OPERAND ORDER:
//    a thread owns 4 consecutive columns of one vector-row, so after an in-register 4 x 8
//    transposition (4 v_perm_b32 per index) it holds, for each of its 8 outputs, the 4
//    consecutive-k values one lane of v_mfma_f32_16x16x16_f16 supplies as B operand: one
//    64-byte run of the tile per thread, written with 4 ds_write_b128 whose 16-byte column is
//    XOR-swizzled with the k position so that the 8 lanes of a write group hit 8 different
//    bank quads; the B reads (ds_read_b64, [k group][output] contiguous) are conflict free.
//  * MFMA phase: the 64 K-steps of a tile are dealt to the 16 waves (4 each, both 16-output
//    blocks): D[token][output] += X[token][k] * W[output][k], fp32.  The A operands (raw x, 8
//    bytes per lane and K-step) are loaded from L2 once per column block and reused for every
//    row group of the workgroup (columns outer, row groups inner).
//  * at the end the 16 waves' partial D are summed through LDS and stored (+ output bias).
// Per index: 2 address perms + 12 packed-f16 ops + 4 transposition perms on the VALU, 2
// gathers + 16 bytes of LDS writes + 16 bytes of LDS operand reads; the MFMA work is 1 / 16 of
// the instruction stream.  bf16 (round 6): the same tile, its roundings as blocks of v_dot2_f32_bf16 (common.h: BF16::add4 /
// scale_bias4 - 44 instructions per index instead of 12) and v_mfma_f32_16x16x16_bf16; before, bf16 kept the <= 4-token launches.
//
// 17 - 64 tokens (gemm_k256w_kernel, vptq_quant_gemm_k256w): the same pass over TB = 2 ... 4 blocks of 16 tokens.  Image, tile, index
// queue and epilogue are shared; only the MFMA phase knows about TB (one B read feeds TB MFMAs, TB x 2 accumulators, the x of the
// blocks past the first requested once the tile is written).  The weights are unpacked, gathered and rebuilt once per launch where
// vptq_quant_gemv runs TB launches of 16 tokens; x (from L2, one 128-byte line per lane and token) is the only traffic that grows.
#include <stdlib.h>

#include <type_traits>

#include "common.h"
#include "kernels.h"
#include "k256.h"

namespace vptq {

constexpr int kGThreads = 1024;
constexpr int kGWaves = 16;
constexpr int kGRows = 4;            // vector-rows per row group (32 outputs = 2 MFMA N blocks)
constexpr int kGTileCols = 1024;     // columns per tile
constexpr int kGImage = 65536;
constexpr int kGTile = kGRows * 8 * kGTileCols * 2;  // 64 KiB
constexpr int kGLds = kGImage + kGTile;

struct GemmK256Params {
  const uint32_t* idx;    // [N][row_words]
  const uint32_t* cent;
  const uint32_t* rcent;
  const uint16_t* x;      // [tokens][G]
  void* y;                // [tokens][O]
  const uint16_t* scale;  // [G] column order
  const uint16_t* wbias;  // [G] column order
  const uint16_t* bias;   // [O] or NULL
  const uint16_t* perm;   // [G] or NULL
  int N, G, O, row_words, tokens, out_f32, n_groups;
};

typedef _Float16 h4v_t __attribute__((ext_vector_type(4)));

// Tile geometry.  A tile is 4 vector-rows (2 blocks nb of 16 outputs) x 1024 columns = 256
// column quads.  MFMA wave wq consumes quads [16 wq, 16 wq + 16): local quad Q = kg * 4 + i is
// K-step i, lane group kg - so that a lane's four K-steps are 16 CONSECUTIVE columns (its x
// operands are two 16-byte loads of one 128-byte line per token; with K-steps of 16 adjacent
// columns a lane read four 8-byte pieces of four different lines, 4x the L2 traffic - that
// was 80 % of the first version's time).  Operand row R = ((nb * 16 + wq) * 4 + i) * 4 + kg:
// 128 bytes = 16 outputs x 4 k values; kg fastest, so the 32 lanes of half a ds_read_b64
// read 256 contiguous bytes.  Inside a row the 16-byte column is XOR-ed with i: the 8 lanes
// of a ds_write_b128 group (4 consecutive quads x the two rows of nb) then cover all 32 banks.
static __device__ __forceinline__ uint32_t tile_row(int nb, int wq, int i, int kg) {
  return (uint32_t)((((nb * 16 + wq) * 4 + i) * 4) + kg);
}

// One pass: NRG row groups x TB blocks of 16 tokens (NRG * TB <= 4: the 32 accumulator registers).  TB = 1 is gemm_k256_kernel's
// pass; TB = 2 ... 4 are gemm_k256w_kernel's, which differ in the MFMA phase only: every B operand read from the tile is used for
// the TB token blocks, and the x operands of the blocks past the first are requested AFTER the tile has been written (the 16
// registers of the rebuilt weights are free by then) instead of being held through the dequantisation.
template <typename DT, bool PERM, int NRG, int TB = 1>
static __device__ __forceinline__ void gemm_k256_pass(const GemmK256Params& P, unsigned char* gsmem,
                                                      const int rg0) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int G = P.G, N = P.N, O = P.O, tokens = P.tokens;
  const uint32_t row_bytes = (uint32_t)P.row_words * 4u;
  const int n_tiles = (G + kGTileCols - 1) / kGTileCols;
  const int grid = (int)gridDim.x;

  const uint32_t hi = (lane >> 3) & 1u;
  const uint32_t baseA = ((hi << 3) | (lane & 7u)) << 4;
  const uint32_t baseB = (((hi ^ 1u) << 3) | (lane & 7u)) << 4;
  const uint32_t selGA[2] = {0x0c0c0400u | (hi << 8), 0x0c0c0600u | (hi << 8)};
  const uint32_t selGB[2] = {0x0c0c0400u | ((hi ^ 1u) << 8), 0x0c0c0600u | ((hi ^ 1u) << 8)};

  // ---- dequant role: thread = 4 consecutive columns (one quad) of one vector-row
  const int dnb = wave >> 3;                                        // 16-output block
  const int drp = (lane >> 2) & 1;                                  // row of the block
  const int drow = dnb * 2 + drp;                                   // vector-row inside the group
  const int dq = (wave & 7) * 32 + (lane >> 3) * 4 + (lane & 3);    // quad inside the tile
  const int di = dq & 3, dkg = (dq >> 2) & 3, dwq = dq >> 4;
  const uint32_t tile_wr = kGImage + tile_row(dnb, dwq, di, dkg) * 128u + (uint32_t)drp * 64u;
  // ---- MFMA role: wave wq = wave, lane (output j / token, k group)
  const int mj = lane & 15, mkg = lane >> 4;

  static_assert(NRG * TB <= 4, "32 accumulator registers");
  f32x4 acc[NRG][TB][2];
#pragma unroll
  for (int g = 0; g < NRG; ++g)
#pragma unroll
    for (int t = 0; t < TB; ++t) { acc[g][t][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[g][t][1] = acc[g][t][0]; }

  // A pass is a flat sequence of steps (tile, row group), row groups fastest; the step loop is
  // unrolled by kQ = 4 (NRG divides it), so every register-queue slot, the row group and "is
  // this the first / last row group of its tile" are compile-time facts of each unrolled
  // body, and every body issues a fixed, unconditional set of loads: the compiler counts
  // them (s_waitcnt vmcnt(n), never 0) and nothing waits for a load it has just issued.
  constexpr int kQ = 4;
  const int n_steps = n_tiles * NRG;
  auto load_idx = [&](int step) -> u32x2 {
    const int sc = step < n_steps ? step : n_steps - 1;   // past the end: the last step again (unused)
    const int tile = sc / NRG, g = sc % NRG;
    const int row = (rg0 + g * grid) * kGRows + drow;
    const int col = tile * kGTileCols + dq * 4;
    const uint32_t roff = (uint32_t)(row < N ? row : N - 1) * row_bytes;
    const uint32_t coff = (uint32_t)(col < G ? col : G - 4) * 2u;
    return __builtin_nontemporal_load((const u32x2*)as_global((const char*)P.idx + (size_t)roff + coff));
  };
  // (token block t: rows 16 t + mj; a row past `tokens` reads the last row and is zeroed in the MFMA phase)
  const uint16_t* const xrow0 = as_global(P.x + (size_t)(mj < tokens ? mj : tokens - 1) * G);
  auto load_x = [&](int tile, int t, u32x4& lo, u32x4& hi4) {
    const int row = t * 16 + mj;
    const uint16_t* const xrow = t == 0 ? xrow0 : as_global(P.x + (size_t)(row < tokens ? row : tokens - 1) * G);
    const int col = tile * kGTileCols + wave * 64 + mkg * 16;
    const int c0 = col < G ? col : G - 8, c1 = col + 8 < G ? col + 8 : G - 8;
    if constexpr (PERM) {
      const u32x4 p0 = *(const u32x4*)as_global(P.perm + c0), p1 = *(const u32x4*)as_global(P.perm + c1);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        lo[q] = (uint32_t)xrow[p0[q] & 0xffffu] | ((uint32_t)xrow[p0[q] >> 16] << 16);
        hi4[q] = (uint32_t)xrow[p1[q] & 0xffffu] | ((uint32_t)xrow[p1[q] >> 16] << 16);
      }
    } else {
      lo = *(const u32x4*)(xrow + c0);
      hi4 = *(const u32x4*)(xrow + c1);
    }
  };
  auto load_sb = [&](int tile, u32x2& sv, u32x2& bv) {
    const int dcol = tile * kGTileCols + dq * 4;
    const int dcc = dcol < G ? dcol : G - 4;
    sv = *(const u32x2*)as_global(P.scale + dcc);
    bv = *(const u32x2*)as_global(P.wbias + dcc);
  };
  // (scale / bias first: the loop waits for them with the index words still in flight)
  u32x2 sv, bv, sv_next, bv_next;
  load_sb(0, sv_next, bv_next);
  __builtin_amdgcn_sched_barrier(0);
  u32x2 iq[kQ];
#pragma unroll
  for (int k = 0; k < kQ; ++k) iq[k] = load_idx(k);
  u32x4 xa_lo[TB], xa_hi[TB];
#pragma unroll
  for (int t = 0; t < TB; ++t) { xa_lo[t] = u32x4{0, 0, 0, 0}; xa_hi[t] = xa_lo[t]; }

  auto do_step = [&](auto kc, int step) {
    constexpr int K = decltype(kc)::value;
    constexpr int g = K % NRG;
    const int tile = step / NRG;
    const u32x2 iw = iq[K];
    if constexpr (g == 0) {
      // new column block: scale / bias requested during the previous block; x of this block
      // (used in the MFMA phase, ~1000 cycles from here)
      sv = sv_next; bv = bv_next;
      __builtin_amdgcn_sched_barrier(0);
      load_x(tile, 0, xa_lo[0], xa_hi[0]);
    }
    if constexpr (g == NRG - 1) load_sb(tile + 1 < n_tiles ? tile + 1 : tile, sv_next, bv_next);
    __builtin_amdgcn_sched_barrier(0);
    const bool dvalid = tile * kGTileCols + dq * 4 < G;
    // ---- dequantise 4 indices: gathers, c + r, * s, + b (each rounded to f16)
    uint32_t w2[4][4];
#pragma unroll
    for (int u0 = 0; u0 < 4; u0 += 2) {   // two columns (one index word) at a time: registers
      u32x4 cA[2], cB[2];
      const uint32_t w = iw[u0 >> 1];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        cA[h] = lds_load16(__builtin_amdgcn_perm(w, baseA, selGA[h]));
        cB[h] = lds_load16(__builtin_amdgcn_perm(w, baseB, selGB[h]));
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        // (four packed pairs per call: for bf16 each stage is one scheduled block of dot instructions, common.h)
        uint32_t v[4] = {cA[h][0], cA[h][1], cA[h][2], cA[h][3]};
        const uint32_t r[4] = {cB[h][0], cB[h][1], cB[h][2], cB[h][3]};
        DT::add4(v, r);
        DT::scale_bias4(v, sv[u0 >> 1], h, bv[u0 >> 1], h);
#pragma unroll
        for (int p = 0; p < 4; ++p) w2[u0 + h][p] = dvalid ? v[p] : 0u;
      }
    }
    // this slot's index words are consumed: request the step kQ ahead into it
    __builtin_amdgcn_sched_barrier(0);
    iq[K] = load_idx(step + kQ);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();  // the previous step's MFMA reads of the tile are done
    // ---- transpose 4 columns x 8 outputs -> 8 operands of 4 k values; 64 bytes per thread
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const u32x4 v = {__builtin_amdgcn_perm(w2[1][p], w2[0][p], 0x05040100u),
                       __builtin_amdgcn_perm(w2[3][p], w2[2][p], 0x05040100u),
                       __builtin_amdgcn_perm(w2[1][p], w2[0][p], 0x07060302u),
                       __builtin_amdgcn_perm(w2[3][p], w2[2][p], 0x07060302u)};
      lds_store16(tile_wr + (((uint32_t)p ^ (uint32_t)di) << 4), v);
    }
    if constexpr (TB > 1) {
      // the other token blocks' x: requested here, where the registers of the rebuilt weights are free, and waited for behind the barrier
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 1; t < TB; ++t) load_x(tile, t, xa_lo[t], xa_hi[t]);
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();  // tile complete
    // ---- MFMA: this wave's 64 columns = 4 K-steps x 2 output blocks, into row group g
    const int colw = tile * kGTileCols + wave * 64 + mkg * 16;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      u32x2 av[TB];
#pragma unroll
      for (int t = 0; t < TB; ++t) {
        const bool live = t * 16 + mj < tokens && colw + 4 * i < G;
        const u32x4& xs4 = i < 2 ? xa_lo[t] : xa_hi[t];
        av[t] = u32x2{live ? xs4[(i & 1) * 2] : 0u, live ? xs4[(i & 1) * 2 + 1] : 0u};
      }
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        const uint32_t pair = ((uint32_t)mj >> 1) ^ (uint32_t)i;
        typedef __attribute__((address_space(3))) const u32x2 lds_u32x2_t;
        const u32x2 b = *(lds_u32x2_t*)(uintptr_t)(kGImage + tile_row(nb, wave, i, mkg) * 128u + pair * 16u +
                                                   ((uint32_t)mj & 1u) * 8u);
#pragma unroll
        for (int t = 0; t < TB; ++t) {
          if constexpr (std::is_same<DT, F16>::value)
            acc[g][t][nb] = __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(h4v_t, av[t]),
                                                                  __builtin_bit_cast(h4v_t, b), acc[g][t][nb], 0, 0, 0);
          else
            acc[g][t][nb] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s4_t, av[t]),
                                                                      __builtin_bit_cast(s4_t, b), acc[g][t][nb], 0, 0, 0);
        }
      }
    }
  };
  for (int step = 0; step < n_steps; step += kQ) {
    do_step(std::integral_constant<int, 0>{}, step);
    if (step + 1 < n_steps) do_step(std::integral_constant<int, 1>{}, step + 1);
    if (step + 2 < n_steps) do_step(std::integral_constant<int, 2>{}, step + 2);
    if (step + 3 < n_steps) do_step(std::integral_constant<int, 3>{}, step + 3);
  }
  // ---- sum the 16 waves' partial D and store, one row group and token block at a time (tile area as scratch)
  float* const scr = (float*)(gsmem + kGImage);  // [nb][reg][wave][lane]
#pragma unroll
  for (int gt = 0; gt < NRG * TB; ++gt) {
    const int g = gt / TB, t = gt % TB;
    __syncthreads();
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int r = 0; r < 4; ++r) scr[((nb * 4 + r) * kGWaves + wave) * 64 + lane] = acc[g][t][nb][r];
    __syncthreads();
    if (tid < 512) {
      // D element (token = (l >> 4) * 4 + r, output = l & 15) of block nb
      const int nb = tid >> 8, r = (tid >> 6) & 3, l = tid & 63;
      float sum = 0.f;
#pragma unroll
      for (int w = 0; w < kGWaves; ++w) sum += scr[((nb * 4 + r) * kGWaves + w) * 64 + l];
      const int token = t * 16 + (l >> 4) * 4 + r;
      const int o = (rg0 + g * grid) * (kGRows * 8) + nb * 16 + (l & 15);
      if (token < tokens && o < O) {
        if (P.bias) sum += DT::to_float(as_global(P.bias)[o]);
        if (P.out_f32) ((float*)as_global((uint16_t*)P.y))[(size_t)token * O + o] = sum;
        else as_global((uint16_t*)P.y)[(size_t)token * O + o] = DT::from_float(sum);
      }
    }
  }
  __syncthreads();
}

// ---- codebook image (see gemv_k256m.hip): row e = 8 main replicas | 8 residual replicas
static __device__ __forceinline__ void gemm_k256_image(const GemmK256Params& P) {
  {
    typedef __attribute__((address_space(3))) unsigned char lds_u8_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char gsmem[];
    if ((uint32_t)(uintptr_t)(lds_u8_t*)gsmem != 0u) __builtin_trap();  // absolute LDS addressing
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  {
    const char* const tab = __builtin_amdgcn_readfirstlane(wave) < 8 ? (const char*)P.cent : (const char*)P.rcent;
    const u32x4 centry = *(const u32x4*)as_global(tab + (uint32_t)((tid >> 1) & 255) * 16u);
    const uint32_t rowp = ((uint32_t)((tid >> 1) & 255) << 8) | ((uint32_t)(tid >> 9) << 7) |
                          ((uint32_t)(tid & 1) << 6);
#pragma unroll
    for (int q = 0; q < 4; ++q) lds_store16(rowp + (((q + (lane >> 1)) & 3) << 4), centry);
  }
  __syncthreads();  // image complete
}

template <typename DT, bool PERM>
__global__ __launch_bounds__(kGThreads) void gemm_k256_kernel(const GemmK256Params P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gsmem[];
  gemm_k256_image(P);
  // this workgroup's row groups bid, bid + grid, ...: passes of 4, 2, 1 (the x operands of a
  // column block are loaded once per pass and reused for every row group of the pass)
  const int grid = (int)gridDim.x;
  int left = ((int)P.n_groups - (int)blockIdx.x + grid - 1) / grid;
  int rg = blockIdx.x;
  for (; left >= 4; left -= 4, rg += 4 * grid) gemm_k256_pass<DT, PERM, 4>(P, gsmem, rg);
  if (left >= 2) { gemm_k256_pass<DT, PERM, 2>(P, gsmem, rg); left -= 2; rg += 2 * grid; }
  if (left >= 1) gemm_k256_pass<DT, PERM, 1>(P, gsmem, rg);
}

// 17 - 64 tokens: TB = 2 ... 4 blocks of 16 tokens in one pass over the indices.  The image, the tile, the K-step -> wave mapping and
// the order of every sum are gemm_k256_kernel's and do not depend on the token count or on a token's block, so a token's output
// bits are those of the 16-token kernel in any slot of any batch.  One row group per pass, <NRG, TB> = <1, 2>, <1, 3>, <1, 4>: a pass
// <2, 2> (the x of a column block shared by two row groups) spilled 24 - 50 registers and was measured slower in every cell
// (profiles/r19/README.md).
template <typename DT, bool PERM, int TB>
__global__ __launch_bounds__(kGThreads) void gemm_k256w_kernel(const GemmK256Params P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gsmem[];
  gemm_k256_image(P);
  const int grid = (int)gridDim.x;
  int left = ((int)P.n_groups - (int)blockIdx.x + grid - 1) / grid;
  int rg = blockIdx.x;
  for (; left >= 1; --left, rg += grid) gemm_k256_pass<DT, PERM, 1, TB>(P, gsmem, rg);
}

// ---- sibling layers (q / k / v, gate / up) in ONE launch: the row-group lists of up to kGKMembers layers, concatenated ----------------
// gemm_k256_pass addresses its row groups as rg0 + g * gridDim.x and the order of every sum depends neither on the grid, nor on NRG,
// nor on the workgroup that runs the row group (above): member m's row group rg has the bits gemm_k256_kernel<DT, false> (TB = 1) /
// gemm_k256w_kernel<DT, false, TB> gives it in the member's own launch.  Plain form only: a member with a column permutation arrives
// as its descriptor without one and x[perm] for x (gemm_gather_px.hip).
constexpr int kGKMembers = 4;

struct GemmK256GroupedParams {
  GemmK256Params m[kGKMembers];
  int first_group[kGKMembers + 1];   // member m owns the global row groups [first_group[m], first_group[m + 1])
  int n, n_groups;
};

// A workgroup walks the global row groups g = blockIdx.x, + gridDim.x, ...: g rises, so the member never falls - the members are
// visited in order.  The switch is uniform per workgroup: a local copy of the member's argument block (kernarg, uniform index) and the
// member's codebook image, rebuilt only where the workgroup has a row group in the member.  No barrier around the rebuild beside the
// image function's own: every pass ends in __syncthreads() (no wave still gathers from the previous image) and gemm_k256_image ends
// in one (the image is complete before the first gather).  The image is built through gemm_k256_image_call (above).
// NO static __shared__ object here: it would move the dynamic LDS base off 0 and gemm_k256_image traps (absolute LDS addressing).  All
// member state lives in kernel arguments and registers; the only LDS is the dynamic kGLds block.
// gemm_k256_image behind a call, given the two tables it reads.  Inlined into the member loop, the image's per-thread addresses are
// loop invariants: the compiler keeps them in registers through every pass, and <F16, 2> then spills 3 registers where
// gemm_k256w_kernel<F16, false, 2> has no scratch memory (profiles/r32/listings.md).  Behind the call they die with it; the call
// runs once per member and workgroup.  (The callee finds the dynamic LDS base through the compiler's per-kernel table: 0 for these
// kernels, which have no static LDS.)
static __device__ __attribute__((noinline)) void gemm_k256_image_call(const uint32_t* cent, const uint32_t* rcent) {
  GemmK256Params P = {};
  P.cent = cent; P.rcent = rcent;
  gemm_k256_image(P);
}
template <typename DT, int TB>
__global__ __launch_bounds__(kGThreads) void gemm_k256_grouped_kernel(const GemmK256GroupedParams GP) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gsmem[];
  const int grid = (int)gridDim.x;
  int g = blockIdx.x;
#pragma unroll 1
  for (int m = 0; m < GP.n; ++m) {
    const int first = GP.first_group[m], end = GP.first_group[m + 1];
    if (g >= end) continue;   // (uniform: g is the workgroup's)
    const GemmK256Params P = GP.m[m];
    gemm_k256_image_call(P.cent, P.rcent);
    int left = (end - g + grid - 1) / grid;   // this workgroup's row groups inside [first, end)
    int rg = g - first;                       // member-local: rg, rg + grid, ...
    g += left * grid;
    if constexpr (TB == 1) {
      // (gemm_k256_kernel's loop)
      for (; left >= 4; left -= 4, rg += 4 * grid) gemm_k256_pass<DT, false, 4>(P, gsmem, rg);
      if (left >= 2) { gemm_k256_pass<DT, false, 2>(P, gsmem, rg); left -= 2; rg += 2 * grid; }
      if (left >= 1) gemm_k256_pass<DT, false, 1>(P, gsmem, rg);
    } else {
      // (gemm_k256w_kernel's loop)
      for (; left >= 1; --left, rg += grid) gemm_k256_pass<DT, false, 1, TB>(P, gsmem, rg);
    }
  }
}

// ---- host side -------------------------------------------------------------------
bool gemm_k256_eligible(const VptqLayerDesc& d, int tokens, int flags) {
  (void)flags;
  if (!gemv_k256_eligible(d, 1)) return false;      // canonical format, norm on, aligned
  if (d.group_size < 8 || (d.group_size & 7)) return false;
  if (d.perm && !(d.scale_permuted && d.bias_permuted)) return false;
  return tokens >= 1 && tokens <= 16;
}

// The launch shape: row groups, grid, and the passes (NRG = 4, 2, 1: the instantiations of gemm_k256_pass) the busiest
// workgroup - workgroup 0 - runs, as the kernel's pass loop takes them.
GemmK256Decision gemm_k256_decide(const VptqLayerDesc& d) {
  GemmK256Decision D = {};
  D.f16 = d.dtype == VPTQ_DTYPE_F16;
  D.perm = d.perm != nullptr;
  D.n_groups = (d.num_indices + kGRows - 1) / kGRows;
  const int ncu = device_cus();
  D.grid = D.n_groups < ncu ? D.n_groups : ncu;
  if (D.grid < 1) return D;
  int left = (D.n_groups + D.grid - 1) / D.grid;   // (gemm_k256_kernel, blockIdx.x = 0)
  if (left >= 4) { D.passes |= 4; left %= 4; }
  if (left >= 2) { D.passes |= 2; left -= 2; }
  if (left >= 1) D.passes |= 1;
  return D;
}

template <typename DT, bool PERM>
static hipError_t launch_g(const GemmK256Params& P, int grid, hipStream_t st) {
  if (const hipError_t e = allow_dynamic_lds<gemm_k256_kernel<DT, PERM>>(kGLds); e != hipSuccess) return e;
  hipLaunchKernelGGL((gemm_k256_kernel<DT, PERM>), dim3(grid), dim3(kGThreads), kGLds, st, P);
  return hipGetLastError();
}

static GemmK256Params gemm_k256_params(const VptqLayerDesc& d, const void* x, void* y, int tokens, bool out_f32, int n_groups) {
  GemmK256Params P = {};
  P.idx = (const uint32_t*)d.indices;
  P.cent = (const uint32_t*)d.centroids;
  P.rcent = (const uint32_t*)d.res_centroids;
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

hipError_t launch_gemm_k256(const VptqLayerDesc& d, const void* x, void* y, int tokens, bool out_f32,
                            hipStream_t st) {
  const GemmK256Decision D = gemm_k256_decide(d);
  if (D.grid < 1) return hipErrorInvalidValue;
  const GemmK256Params P = gemm_k256_params(d, x, y, tokens, out_f32, D.n_groups);
  if (D.f16) return D.perm ? launch_g<F16, true>(P, D.grid, st) : launch_g<F16, false>(P, D.grid, st);
  return D.perm ? launch_g<BF16, true>(P, D.grid, st) : launch_g<BF16, false>(P, D.grid, st);
}

// ---- 17 - 64 tokens (gemm_k256w_kernel)
bool gemm_k256w_eligible(const VptqLayerDesc& d, int tokens) {
  return gemm_k256_eligible(d, 16, 0) && tokens >= 17 && tokens <= 64;
}

// tb token blocks; the row groups and the grid are gemm_k256_decide's; rgs: the row groups (= passes <1, tb>) of the busiest workgroup
GemmK256WDecision gemm_k256w_decide(const VptqLayerDesc& d, int tokens) {
  const GemmK256Decision B = gemm_k256_decide(d);
  GemmK256WDecision D = {};
  D.f16 = B.f16; D.perm = B.perm; D.n_groups = B.n_groups; D.grid = B.grid;
  D.tok = tokens;
  D.tb = (tokens + 15) / 16;
  if (D.grid < 1) return D;
  D.rgs = (D.n_groups + D.grid - 1) / D.grid;   // (gemm_k256w_kernel, blockIdx.x = 0)
  return D;
}

template <typename DT, bool PERM, int TB>
static hipError_t launch_gw(const GemmK256Params& P, int grid, hipStream_t st) {
  if (const hipError_t e = allow_dynamic_lds<gemm_k256w_kernel<DT, PERM, TB>>(kGLds); e != hipSuccess) return e;
  hipLaunchKernelGGL((gemm_k256w_kernel<DT, PERM, TB>), dim3(grid), dim3(kGThreads), kGLds, st, P);
  return hipGetLastError();
}

template <typename DT, bool PERM>
static hipError_t launch_gw_tb(const GemmK256Params& P, int tb, int grid, hipStream_t st) {
  switch (tb) {
    case 2: return launch_gw<DT, PERM, 2>(P, grid, st);
    case 3: return launch_gw<DT, PERM, 3>(P, grid, st);
    case 4: return launch_gw<DT, PERM, 4>(P, grid, st);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_gemm_k256w(const VptqLayerDesc& d, const void* x, void* y, int tokens, bool out_f32, hipStream_t st) {
  const GemmK256WDecision D = gemm_k256w_decide(d, tokens);
  if (D.grid < 1 || D.tb < 2 || D.tb > 4) return hipErrorInvalidValue;
  const GemmK256Params P = gemm_k256_params(d, x, y, tokens, out_f32, D.n_groups);
  if (D.f16) return D.perm ? launch_gw_tb<F16, true>(P, D.tb, D.grid, st) : launch_gw_tb<F16, false>(P, D.tb, D.grid, st);
  return D.perm ? launch_gw_tb<BF16, true>(P, D.tb, D.grid, st) : launch_gw_tb<BF16, false>(P, D.tb, D.grid, st);
}

// ---- 2 - 4 sibling layers, 1 - 48 tokens (gemm_k256_grouped_kernel)
// what one grouped launch IS: the template arguments of gemm_k256_grouped_kernel<DT, TB>, every member's row groups and the launch
// shape, decided once for the launcher and for vptq_quant_gemm_k256_grouped_instance.  The members share dtype and width (the caller's
// check).  grid <= CUs, so rgs (the most row groups of any workgroup) and passes (the bit mask of every NRG any workgroup runs in any
// member; tb > 1: NRG = 1 only) are found by walking every workgroup's list as the kernel does.
GemmK256GroupedDecision gemm_k256_grouped_decide(const VptqLayerDesc* descs, int n, int tokens) {
  GemmK256GroupedDecision D = {};
  if (n < 1 || n > kGKMembers) return D;
  D.f16 = descs[0].dtype == VPTQ_DTYPE_F16;
  D.tok = tokens;
  D.tb = (tokens + 15) / 16;
  D.n = n;
  for (int m = 0; m < n; ++m) {
    D.groups[m] = (descs[m].num_indices + kGRows - 1) / kGRows;
    D.first_group[m + 1] = D.first_group[m] + D.groups[m];
  }
  D.total = D.first_group[n];
  const int ncu = device_cus();
  D.grid = D.total < ncu ? D.total : ncu;
  for (int b = 0; b < D.grid; ++b) {
    int g = b, rgs = 0;
    for (int m = 0; m < n; ++m) {
      const int end = D.first_group[m + 1];
      if (g >= end) continue;
      int left = (end - g + D.grid - 1) / D.grid;
      g += left * D.grid;
      rgs += left;
      if (D.tb > 1) { D.passes |= 1; continue; }
      if (left >= 4) { D.passes |= 4; left %= 4; }
      if (left >= 2) { D.passes |= 2; left -= 2; }
      if (left >= 1) D.passes |= 1;
    }
    if (rgs > D.rgs) D.rgs = rgs;
  }
  return D;
}

template <typename DT, int TB>
static hipError_t launch_gg(const GemmK256GroupedParams& GP, int grid, hipStream_t st) {
  if (const hipError_t e = allow_dynamic_lds<gemm_k256_grouped_kernel<DT, TB>>(kGLds); e != hipSuccess) return e;
  hipLaunchKernelGGL((gemm_k256_grouped_kernel<DT, TB>), dim3(grid), dim3(kGThreads), kGLds, st, GP);
  return hipGetLastError();
}

template <typename DT>
static hipError_t launch_gg_tb(const GemmK256GroupedParams& GP, int tb, int grid, hipStream_t st) {
  switch (tb) {
    case 1: return launch_gg<DT, 1>(GP, grid, st);
    case 2: return launch_gg<DT, 2>(GP, grid, st);
    case 3: return launch_gg<DT, 3>(GP, grid, st);
  }
  return hipErrorInvalidValue;
}

// descs: the members WITHOUT a permutation (a permuted member as its plain form); x[m]: member m's activations in its own column order
hipError_t launch_gemm_k256_grouped(const VptqLayerDesc* descs, int n, const void* const* x, void* const* y, int tokens, bool out_f32,
                                    hipStream_t st) {
  const GemmK256GroupedDecision D = gemm_k256_grouped_decide(descs, n, tokens);
  if (D.n < 2 || D.grid < 1 || tokens < 1 || D.tb < 1 || D.tb > 3) return hipErrorInvalidValue;
  GemmK256GroupedParams GP = {};
  for (int m = 0; m < n; ++m) {
    if (descs[m].perm || !x[m] || !y[m]) return hipErrorInvalidValue;
    GP.m[m] = gemm_k256_params(descs[m], x[m], y[m], tokens, out_f32, D.groups[m]);
    GP.first_group[m] = D.first_group[m];
  }
  for (int m = n; m <= kGKMembers; ++m) GP.first_group[m] = D.total;
  GP.n = n;
  GP.n_groups = D.total;
  return D.f16 ? launch_gg_tb<F16>(GP, D.tb, D.grid, st) : launch_gg_tb<BF16>(GP, D.tb, D.grid, st);
}

}  // namespace vptq
